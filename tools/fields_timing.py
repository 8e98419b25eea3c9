"""Field-dump interpolation: the device call (fdtd_field_interp, csrc/fields.hip) against the numpy specification (fields.interp_spec).

  python tools/fields_timing.py [--box NX NY NZ] [--out FILE]

A box of NX x NY x NZ cells (default 300 x 300 x 60) on a graded mesh, random complex spectra on its recorded region.  Per kind, node
mode and cell mode: the whole device call (host validation, uploads, the kernel, the download), best of three after one warm-up call,
the specification once, and whether the two results have the same bits.  Writes FILE (default profiles/fields/timing.txt); without a
GPU, or without the entry point in the library, the file says "unmeasured".
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


def inputs(cells, seed=1):
    rng = np.random.default_rng(seed)
    lines = [np.concatenate([[0.0], np.cumsum(1e-3 * rng.uniform(0.75, 1.3, k + 2))]) for k in cells]     # one cell of margin each side
    lo, hi = (1, 1, 1), tuple(k + 1 for k in cells)
    shape = tuple(hi[a] - lo[a] + 2 for a in (2, 1, 0))
    rec = [rng.standard_normal(shape) + 1j * rng.standard_normal(shape) for _ in range(3)]
    kap = [rng.uniform(0.0, 2.0, shape) for _ in range(3)]
    return lines, lo, hi, rec, kap


def device_lib():
    try:
        capi = imp("_capi")
        lib = capi.load_hip_library()
        return lib if capi.has_fields(lib) and lib.fdtd_device_count() >= 1 else None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--box", type=int, nargs=3, default=(300, 300, 60))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fields", "timing.txt"))
    a = ap.parse_args()
    capi, fields = imp("_capi"), imp("fields")
    lib = device_lib()
    lines, lo, hi, rec, kap = inputs(a.box)
    head = [f"Field-dump interpolation, a box of {' x '.join(map(str, a.box))} cells on a graded mesh, complex spectra: `python tools/fields_timing.py`.",
            "No bars: a record, not a test.  Device: the whole fdtd_field_interp call (uploads, kernel, download), wall clock, best of 3",
            "after one warm-up call.  Specification: fields.interp_spec (numpy), once.", ""]
    out = []
    if lib is None:
        out.append("unmeasured: no GPU (or no fdtd_field_interp in the library) where the tool ran.")
    else:
        for kind in fields.KINDS:
            for mode in (fields.MODE_NODE, fields.MODE_CELL):
                args = (kind, mode, lines, lo, hi, rec, rec, kap if kind == "J" else None)
                capi.field_interp_raw(lib, *args)
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    got = capi.field_interp_raw(lib, *args)
                    ts.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                want = fields.interp_spec(*args)
                t_spec = time.perf_counter() - t0
                same = got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))
                line = (f"{kind:4s} {'node' if mode == 1 else 'cell'}: device {min(ts) * 1e3:7.1f} ms, specification {t_spec * 1e3:8.1f} ms "
                        f"({t_spec / min(ts):.1f} x), {got.size // 3} points, same bits: {same}")
                print(line, flush=True)
                out.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(head + out) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
