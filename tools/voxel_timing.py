"""Voxelisation: the numpy specification (primitives.rasterise_spec) on the host against fdtd_voxelize (csrc/voxel.hip) on the device.

  python tools/voxel_timing.py [--repeats N] [--small] [--only WORD] [--against LIBDIR] [--out FILE]

Wall clock of one rasterisation of both owner arrays from the same primitives.Table.  The device figure is the whole call: table and
mesh-line upload, both kernels, a device synchronise, and the download of the owners into host memory — what voxelize() waits for.
One warm-up call, then N repeats (default 5): median (min, max).  The host figure is the median of min(N, 3) calls (no warm-up
needed).  Both results are compared (np.array_equal) and the comparison is printed.  Scenes:
  * the 2 x 2 multi-patch scene at 800 x 800 x 120 as the plugin draws it (boxes only);
  * the same with a SphericalShell radome around the array and a Sphere lens above it;
  * a 1000-segment Wire helix over the patch workload at 300 x 300 x 60;
  * the radome scene again at 400 x 400 x 60, 200 x 200 x 30, 100 x 100 x 15 and 50 x 50 x 7: where, if anywhere, the host overtakes
    the device.  _capi.default_rasteriser follows these lines (profiles/primitives/timing.txt says what they were).
  * an icosphere solid (primitives.Polyhedron; tests/polyhedron_cases.icosphere_tris) of 1280 and of 20480 triangles over the patch
    workload at 300 x 300 x 60, as a material and as a metal (one host call: the specification loops over the triangles in Python).
--only WORD keeps the scenes whose name contains WORD.  --against LIBDIR times every kept scene on a second build of the library too
(<LIBDIR>/libfdtd_hip.so, e.g. the parent commit's), its calls interleaved with the first's: the one comparison across builds that
holds, because both run in one process on one machine.
The kernels' resource lines are copied from profiles/primitives/costs.txt (tools/kernel_resources.py k_voxel wrote them).
--small divides every grid dimension by 4 (a rehearsal, not a measurement).  The comparison is host against device in one process on
one machine, never against an earlier run.
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

SWEEP = (2, 4, 8, 16)                   # divisors of 800 x 800 x 120 for the size sweep
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "fdtd-solver-antennas_amd"
imp = lambda m: importlib.import_module(PKG + "." + m)


def multi_patch(n):
    s, wl = imp("solver_fdtd_hip"), imp("workloads")
    p = imp("params").PatchAntennaParams.from_user_units(frequency_ghz=2.45, er=4.3, h_mm=1.6, loss_tangent=0.02)
    pitch = 0.0612
    arr = [s.PatchInstance(f"P{q}", p, (ix - 0.5) * pitch, (iy - 0.5) * pitch, 0.0, s.FeedDirection.NEG_X)
           for q, (ix, iy) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)])]
    prep = s.prepare_hip_microstrip_multi_3d(arr, boundary="PML_8")
    if not prep.ok:
        raise RuntimeError(prep.message)
    return wl.workload_from_prepared("multi", prep, n[0], n[1], n[2], 1)


def radome(n):
    w = multi_patch(n)
    u = w.scene.unit
    span = [(l[-1] - l[0]) / u for l in w.grid.lines]
    mid = [0.5 * (l[-1] + l[0]) / u for l in w.grid.lines]
    r = 0.4137 * min(span[0], span[1])
    w.scene.add_material("radome", 3.1).add_spherical_shell((mid[0], mid[1], 0.0), r, 0.0513 * r, priority=0)
    w.scene.add_material("lens", 2.2).add_sphere((mid[0], mid[1], 0.2213 * span[2]), 0.1317 * min(span), priority=0)
    return w


def scenes(small):
    q = 4 if small else 1
    w = multi_patch((800 // q, 800 // q, 120 // q))
    yield f"2x2 multi-patch, boxes only, {'x'.join(map(str, w.grid.shape))}", w.grid, w.scene
    w = radome((800 // q, 800 // q, 120 // q))
    yield f"the same + SphericalShell radome + Sphere lens, {'x'.join(map(str, w.grid.shape))}", w.grid, w.scene
    w = imp("workloads").patch_workload("helix", nx=300 // q, ny=300 // q, nz=60 // q)
    u = w.scene.unit
    span = [(l[-1] - l[0]) / u for l in w.grid.lines]
    mid = [0.5 * (l[-1] + l[0]) / u for l in w.grid.lines]
    t = np.linspace(0.0, 10.0 * 2.0 * np.pi, 1001)
    rh = 0.1713 * min(span[0], span[1])
    z0 = w.grid.z[-1] / u - 0.45 * span[2]
    w.scene.add_metal("helix").add_wire([mid[0] + rh * np.cos(t), mid[1] + rh * np.sin(t), z0 + 0.35 * span[2] * t / t[-1]], 0.0213 * rh)
    yield f"patch + 1000-segment Wire helix, {'x'.join(map(str, w.grid.shape))}", w.grid, w.scene
    for sub in (3, 5):
        w = imp("workloads").patch_workload("mesh", nx=300 // q, ny=300 // q, nz=60 // q)
        u = w.scene.unit
        span = [(l[-1] - l[0]) / u for l in w.grid.lines]
        mid = [0.5 * (l[-1] + l[0]) / u for l in w.grid.lines]
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        tris = importlib.import_module("polyhedron_cases").icosphere_tris
        r = 0.2113 * min(span)
        w.scene.add_material("ball", 2.2).add_polyhedron(tris((mid[0] - 1.1 * r, mid[1], mid[2]), r, sub), priority=0)
        w.scene.add_metal("shot").add_polyhedron(tris((mid[0] + 1.1 * r, mid[1], mid[2]), r, sub), priority=0)
        yield f"patch + two icosphere meshes of {20 * 4 ** sub} triangles, {'x'.join(map(str, w.grid.shape))}", w.grid, w.scene
    for d in SWEEP:                                                      # the radome scene again, on smaller grids
        w = radome((800 // d // q, 800 // d // q, 120 // d // q))
        yield f"size sweep: radome scene, {'x'.join(map(str, w.grid.shape))}", w.grid, w.scene


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--only")
    ap.add_argument("--against")
    ap.add_argument("--out")
    a = ap.parse_args()
    P, capi = imp("primitives"), imp("_capi")
    lib = capi.load_hip_library()
    with open(os.path.join(ROOT, "profiles", "primitives", "costs.txt")) as fh:
        res = [l.rstrip() for l in fh if l.lstrip().startswith("k_voxel<")]
    lines = res + [f"host CPUs: {os.cpu_count()} (numpy specification: one thread); device: {lib.fdtd_backend().decode()}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)
    other = capi.bind(__import__("ctypes").CDLL(os.path.join(a.against, capi.HIP_LIB_NAME))) if a.against else None
    for name, grid, scene in scenes(a.small):
        if a.only and a.only not in name:
            continue
        table = P.pack_table(scene, grid)
        host = []
        for _ in range(1 if "mesh" in name else min(a.repeats, 3)):
            t0 = time.perf_counter(); spec = P.rasterise_spec(grid, table); host.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); capi.voxelize_raw(lib, grid, table); first = time.perf_counter() - t0   # warm-up: code object load, first allocations
        dev, dev2 = [], []
        if other is not None:
            capi.voxelize_raw(other, grid, table)
        for _ in range(a.repeats):
            t0 = time.perf_counter(); got = capi.voxelize_raw(lib, grid, table); dev.append(time.perf_counter() - t0)
            if other is not None:
                t0 = time.perf_counter(); got2 = capi.voxelize_raw(other, grid, table); dev2.append(time.perf_counter() - t0)
        same = np.array_equal(spec[0], got[0]) and np.array_equal(spec[1], got[1])
        mb = (got[0].nbytes + got[1].nbytes) / 1e6
        say(f"{name}: {len(table.rec)} records, {int(np.prod(grid.shape))} nodes, owners {mb:.1f} MB")
        say(f"  host   median {statistics.median(host):8.4f} s  (min {min(host):.4f}, max {max(host):.4f}; {len(host)} calls)")
        say(f"  device median {statistics.median(dev):8.4f} s  (min {min(dev):.4f}, max {max(dev):.4f}; {len(dev)} calls after one warm-up of {first:.4f} s; upload + kernels + download)")
        say(f"  host / device {statistics.median(host) / statistics.median(dev):.2f}x; owners identical: {same}")
        if other is not None:
            same2 = np.array_equal(got2[0], got[0]) and np.array_equal(got2[1], got[1])
            say(f"  --against median {statistics.median(dev2):8.4f} s  (min {min(dev2):.4f}, max {max(dev2):.4f}; {len(dev2)} calls, interleaved); "
                f"this / against {statistics.median(dev) / statistics.median(dev2):.3f}; owners identical: {same2}")
        del spec, got
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
