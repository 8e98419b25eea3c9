"""Conformal PEC boundaries: what they cost a run (k_conformal, csrc/conformal.hip, the schedule such a context takes and the
reduced timestep), and the device fractions (fdtd_voxel_fractions, csrc/voxel.hip) against numpy.

  python tools/conformal_timing.py [--grid NX NY NZ]

Wall clock of fdtd_run per timestep (a device synchronise ends every timed block), contexts of one process in interleaved rounds,
median (min, max), on the patch workload (default 300 x 300 x 60, CPML 8) with a circular patch (a flat disc of 17.1 mm radius) for
  * conformal=False as AUTO schedules it (the multi-timestep schedule);
  * conformal=False under FDTD_FLAG_KERNEL_DIRECT (the two-launch schedule a context with listed faces runs);
  * conformal=True: the same two launches + k_conformal.  The difference to the line above is k_conformal's cost per timestep; the
    run also needs sqrt(R) times as many timesteps for the same physical time (dt = courant_dt / sqrt(R)).
Then the fractions of the same scene: conformal.fractions on the device and in numpy, best of three, the results compared.
Run under rocprofv3 --kernel-trace --stats (a run of its own) for k_conformal's duration.
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
    patch = w.scene.metals[0]
    z = patch.boxes[0].start[2]
    patch.boxes.clear()
    patch.add_cylinder((0.0, 0.0, z), (0.0, 0.0, z), 17.1, priority=10)
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", nargs=3, type=int, default=[300, 300, 60])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warm", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    capi, sc, sim, cf = imp("_capi"), imp("scene"), imp("simulation"), imp("conformal")
    lib = capi.load_hip_library()
    n = tuple(a.grid)
    total = a.warm + a.rounds * a.steps + 16
    w = workload(n)
    vox = sc.voxelize(w.scene, w.grid, rasteriser=capi.default_rasteriser(lib), conformal=True, device_fractions=capi.default_fractions(lib))
    runs = [("conformal=False, AUTO", False, 0), ("conformal=False, two launches (DIRECT)", False, capi.FLAG_KERNEL_DIRECT),
            ("conformal=True (R = 2), two launches + k_conformal", True, 0)]
    eng = []
    for tag, on, flags in runs:
        r = sim.Simulation(w.grid, vox, f0=w.f0, fc=w.fc, boundary="CPML", cpml_cells=8, nr_ts=total, end_criteria=0.0, conformal=on)
        e = r.build(lib, flags=flags)
        e.run(a.warm)
        e.energy()
        eng.append((tag, e, r, []))
    for _ in range(a.rounds):
        for tag, e, r, t in eng:
            t0 = time.perf_counter()
            e.run(a.steps)
            e.energy()
            t.append((time.perf_counter() - t0) / a.steps * 1e6)
    for tag, e, r, t in eng:
        info, v = e.schedule_info(), np.array(t)
        c = r.conformal
        faces = "no listed faces" if c is None else f"{len(c)} listed faces {c.faces()}, {c.clamped} clamped, {c.frac.idx.size} cut edges, dt factor {c.dt_factor:.4f}"
        print(f"circular patch {n[0]}x{n[1]}x{n[2]} CPML-8, {tag}: median {np.median(v):.2f} us/timestep (min {v.min():.2f}, max {v.max():.2f}; "
              f"{a.rounds} rounds of {a.steps}), {info['launches_per_timestep']} launches/timestep, resident {info['resident']}, {faces}", flush=True)
        e.close()
    table = cf.plain_metal_table(w.scene, w.grid)
    best = {}
    for tag, dev in (("device", capi.default_fractions(lib)), ("numpy", None)):
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            fr = cf.fractions(w.scene, w.grid, dev)
            ts.append(time.perf_counter() - t0)
        best[tag] = (min(ts), fr)
    same = np.array_equal(best["device"][1].f.view(np.uint64), best["numpy"][1].f.view(np.uint64)) and np.array_equal(best["device"][1].node_in, best["numpy"][1].node_in)
    print(f"fractions of the same scene ({table.rec.size} metal records, {best['numpy'][1].idx.size} cut edges), whole call, best of 3: device "
          f"{best['device'][0] * 1e3:.1f} ms, numpy {best['numpy'][0] * 1e3:.1f} ms; identical: {same}", flush=True)


if __name__ == "__main__":
    main()
