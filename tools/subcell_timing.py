"""Sub-cell averaged dielectric surfaces: what the set-up costs (fdtd_voxel_subcell, csrc/voxel.hip, next to fdtd_voxelize on the same
scene) and what leaving the packed class form costs the step loop.

  python tools/subcell_timing.py [--grid NX NY NZ]

The patch workload (default 300 x 300 x 60, CPML 8) with its substrate plus a dielectric sphere (eps 10) of 40 cells radius above the
patch.  Whole calls, best of three.  Then wall clock of fdtd_run per timestep (a device synchronise ends every timed block), contexts
of one process in interleaved rounds, median (min, max), with subcell off and on, and the operator form each build ended in.
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


def workload(n):
    w = imp("workloads").patch_workload("timing", nx=n[0], ny=n[1], nz=n[2])
    pitch = float(w.grid.x[1] - w.grid.x[0]) / 1e-3
    w.scene.add_material("ball", 10.0).add_sphere((3.1, -2.3, 45.0 * pitch), 40.0 * pitch, priority=1)
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", nargs=3, type=int, default=[300, 300, 60])
    ap.add_argument("--nsub", type=int, default=4)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warm", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    capi, sc, sim, sub, prims = imp("_capi"), imp("scene"), imp("simulation"), imp("subcell"), imp("primitives")
    lib = capi.load_hip_library()
    n = tuple(a.grid)
    w = workload(n)
    table = prims.pack_table(w.scene, w.grid)
    vox0 = sc.voxelize(w.scene, w.grid, rasteriser=capi.default_rasteriser(lib))
    tabs, skip = sub.prop_tables(w.scene), sub.skip_mask(w.grid, vox0.pec)
    best = {}
    for tag, fn in (("fdtd_voxelize", lambda: capi.voxelize_raw(lib, w.grid, table)),
                    ("fdtd_voxel_subcell", lambda: capi.subcell_raw(lib, w.grid, table, a.nsub, *tabs, skip))):
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            res = fn()
            ts.append(time.perf_counter() - t0)
        best[tag] = (min(ts), res)
    ls = best["fdtd_voxel_subcell"][1]
    print(f"{n[0]}x{n[1]}x{n[2]}, substrate + sphere of 40 cells radius ({table.rec.size} records), nsub {a.nsub}, whole call, best of 3: fdtd_voxelize "
          f"{best['fdtd_voxelize'][0] * 1e3:.1f} ms, fdtd_voxel_subcell {best['fdtd_voxel_subcell'][0] * 1e3:.1f} ms ({len(ls)} listed edges {ls.edges()})", flush=True)
    total = a.warm + a.rounds * a.steps + 16
    eng = []
    for on in (False, True):
        vox = sc.voxelize(w.scene, w.grid, rasteriser=capi.default_rasteriser(lib), subcell=a.nsub if on else 0, device_subcell=capi.default_subcell(lib))
        r = sim.Simulation(w.grid, vox, f0=w.f0, fc=w.fc, boundary="CPML", cpml_cells=8, nr_ts=total, end_criteria=0.0, subcell=on, subcell_samples=a.nsub)
        e = r.build(lib)
        e.run(a.warm)
        e.energy()
        eng.append((on, e, r, []))
    for _ in range(a.rounds):
        for on, e, r, t in eng:
            t0 = time.perf_counter()
            e.run(a.steps)
            e.energy()
            t.append((time.perf_counter() - t0) / a.steps * 1e6)
    cells = n[0] * n[1] * n[2]
    for on, e, r, t in eng:
        info, v = e.schedule_info(), np.array(t)
        print(f"subcell={on}: operator form {e.operator_form()}, median {np.median(v):.2f} us/timestep (min {v.min():.2f}, max {v.max():.2f}; {a.rounds} rounds "
              f"of {a.steps}) = {cells / np.median(v):.0f} Mcells/s, {info['launches_per_timestep']} launches/timestep, resident {info['resident']}", flush=True)
        e.close()


if __name__ == "__main__":
    main()
