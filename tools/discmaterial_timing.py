"""Voxel maps: the numpy specification (primitives.rasterise_spec with maps) on the host against fdtd_voxelize_maps (csrc/voxel.hip) on
the device, and the identity checks that profiles/discmaterial/kat.txt records.

  python tools/discmaterial_timing.py [--repeats N] [--small] [--out FILE]

1. Identity: every case of tests/discmaterial_cases.py (the ones tests/test_discmaterial_gpu.py asserts), owners and cell_voxel
   compared with np.array_equal, the counts printed.
2. Wall clock on the patch workload's 300 x 300 x 60 grid with a 256^3-voxel map (9 tissues, 35 % zeros, rotated and shifted, a box
   over the whole grid as the delimiter) beside the patch's own boxes.  The device figure is the whole call: uploads (the map's 16 MiB
   among them), the launches, a device synchronise and the three downloads; one warm-up call, then N repeats (default 5): median
   (min, max).  The host figure is the median of min(N, 3) calls.  One process, one machine.
--small divides the grid and the map by 4 per axis (a rehearsal, not a measurement).
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "fdtd-solver-antennas_amd"
imp = lambda m: importlib.import_module(PKG + "." + m)


def big_scene(small):
    q = 4 if small else 1
    dc = importlib.import_module("discmaterial_cases")
    w = imp("workloads").patch_workload("phantom", nx=300 // q, ny=300 // q, nz=60 // q)
    u = w.scene.unit
    lo = [l[0] / u for l in w.grid.lines]
    hi = [l[-1] / u for l in w.grid.lines]
    mid = [0.5 * (a + b) for a, b in zip(lo, hi)]
    n = 256 // q
    half = [0.45 * (b - a) for a, b in zip(lo, hi)]
    lines = tuple(dc.uneven_lines(n + 1, -half[a], half[a], 50 + a) for a in range(3))
    dm = w.scene.add_disc_material("phantom", lines, dc.random_data((n, n, n), 9, 0.35, 7), *dc.table_of(9),
                                   matrix=dc.rotation((0.2, -0.1, 0.97), 7.0, mid))
    dm.add_box(lo, hi, priority=-1)
    return w.grid, w.scene


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    P, capi = imp("primitives"), imp("_capi")
    dc = importlib.import_module("discmaterial_cases")
    lib = capi.load_hip_library()
    lines = [f"host CPUs: {os.cpu_count()} (numpy specification: one thread); device: {lib.fdtd_backend().decode()}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)
    cases = [("(a) tiles and placement", dc.crowded_scene()), ("(b) database background", dc.crowded_scene(use_db_background=True)),
             ("(c) two maps", dc.two_maps_scene()), ("(d) centres on lines", dc.on_lines_scene()),
             ("(e) map outside the grid", dc.crowded_scene(outside=True)), ("(f) extremes", dc.extremes_scene())]
    for name, (grid, scene) in cases:
        table = P.pack_table(scene, grid)
        spec, got = P.rasterise_spec(grid, table), capi.voxelize_raw(lib, grid, table)
        same = [bool(np.array_equal(x, y)) for x, y in zip(spec, got)]
        say(f"{name}: {'x'.join(map(str, grid.shape))} nodes, {len(table.rec)} records, {len(table.maps)} maps; cells owned by a map "
            f"{int((spec[2] >= 0).sum())} of {spec[2].size}; cell_owner, edge_owner, cell_voxel identical: {same}")
    grid, scene = big_scene(a.small)
    table = P.pack_table(scene, grid)
    host = []
    for _ in range(min(a.repeats, 3)):
        t0 = time.perf_counter(); spec = P.rasterise_spec(grid, table); host.append(time.perf_counter() - t0)
    t0 = time.perf_counter(); capi.voxelize_raw(lib, grid, table); first = time.perf_counter() - t0
    dev = []
    for _ in range(a.repeats):
        t0 = time.perf_counter(); got = capi.voxelize_raw(lib, grid, table); dev.append(time.perf_counter() - t0)
    same = [bool(np.array_equal(x, y)) for x, y in zip(spec, got)]
    say(f"timing: {'x'.join(map(str, grid.shape))} nodes, {len(table.rec)} records, one map of {'x'.join(str(l.size - 1) for l in table.maps[0].lines)} voxels "
        f"({table.maps[0].data.nbytes / 2**20:.1f} MiB); cells owned by the map {int((spec[2] >= 0).sum())} of {spec[2].size}")
    say(f"  host   median {statistics.median(host):8.4f} s  (min {min(host):.4f}, max {max(host):.4f}; {len(host)} calls)")
    say(f"  device median {statistics.median(dev):8.4f} s  (min {min(dev):.4f}, max {max(dev):.4f}; {len(dev)} calls after one warm-up of {first:.4f} s; "
        f"uploads + launches + downloads)")
    say(f"  host / device {statistics.median(host) / statistics.median(dev):.2f}x; cell_owner, edge_owner, cell_voxel identical: {same}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if all(same) else 1


if __name__ == "__main__":
    sys.exit(main())
