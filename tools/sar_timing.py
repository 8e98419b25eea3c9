"""SAR averaging: the device call (fdtd_sar_average, csrc/sar.hip) against the numpy specification (sar.average_spec).

  python tools/sar_timing.py [--box N] [--out FILE] [--no-spec]

A phantom of N^3 cells (default 48) of 1 mm: tissue of 950 to 1100 kg/m^3 with 3 % air pockets and a slab of air on top (a sixth of
the box), a random loss density.  Averaged over 1 g and over 10 g, method "ieee": the whole device call (host validation, uploads,
the cube search, the second pass, downloads), best of three, and the specification once.  Writes FILE (default
profiles/sar/timing.txt); without a GPU, or without the SAR entry points in the library, the file says "unmeasured".
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "fdtd-solver-antennas_amd"
imp = lambda m: importlib.import_module(PKG + "." + m)


def phantom(n, seed=1):
    rng = np.random.default_rng(seed)
    d = [np.full(n, 1e-3)] * 3
    rho = rng.uniform(950.0, 1100.0, (n, n, n))
    rho[rng.random(rho.shape) < 0.03] = 0.0
    rho[n - n // 6:] = 0.0
    return d, rho, rng.uniform(0.1, 5.0, rho.shape) * (rho > 0)


def device_lib():
    try:
        capi = imp("_capi")
        lib = capi.load_hip_library()
        return lib if capi.has_sar(lib) and lib.fdtd_device_count() >= 1 else None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--box", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sar", "timing.txt"))
    ap.add_argument("--no-spec", action="store_true", help="skip the numpy specification (minutes at 48^3)")
    a = ap.parse_args()
    capi, sar = imp("_capi"), imp("sar")
    lib = device_lib()
    d, rho, p = phantom(a.box)
    head = [f"SAR averaging, {a.box}^3 cells of 1 mm ({int((rho > 0).sum())} tissue voxels), method \"ieee\": `python tools/sar_timing.py`.",
            "No bars: a record, not a test.  Device: the whole fdtd_sar_average call (uploads, cube search, second pass, downloads), wall",
            "clock, best of 3 after one warm-up call.  Specification: sar.average_spec (numpy, one Python loop over the voxels), once.", ""]
    lines = []
    if lib is None:
        lines.append("unmeasured: no GPU (or no SAR entry points in the library) where the tool ran.")
    else:
        for tag, mass in (("1 g", 1e-3), ("10 g", 10e-3)):
            capi.sar_average_raw(lib, *d, rho, p, mass)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                got = capi.sar_average_raw(lib, *d, rho, p, mass)
                ts.append(time.perf_counter() - t0)
            line = (f"{tag}: device {min(ts) * 1e3:.1f} ms (status 0 / 1 / 2 / 3: {' / '.join(str(int(c)) for c in got[3])}; "
                    f"cubes {2e3 * np.nanmin(got[1]):.1f} to {2e3 * np.nanmax(got[1]):.1f} mm wide)")
            print(line, flush=True)
            if not a.no_spec:
                t0 = time.perf_counter()
                want = sar.average_spec(*d, rho, p, mass)
                ts_spec = time.perf_counter() - t0
                fin = np.isfinite(want[0]) & np.isfinite(got[0])
                err = float(np.max(np.abs(got[0][fin] / np.where(want[0][fin] != 0, want[0][fin], 1.0) - (want[0][fin] != 0))))
                line += (f"; specification {ts_spec:.1f} s ({ts_spec / min(ts):.0f} x); status bytes equal: "
                         f"{bool(np.array_equal(got[2], want[2]))}, largest relative difference of sar_avg {err:.1e}")
                print(line, flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(head + lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
