"""Lorentz / Drude media: what a resonant substrate costs a run (k_lorentz, csrc/lorentz.hip, and the schedule such a context takes).

  python tools/lorentz_timing.py [--parent-lib DIR] [--grid NX NY NZ] [--poles K]

Wall clock of fdtd_run per timestep (a device synchronise ends every timed block), contexts of one process in interleaved rounds,
median (min, max), on the patch workload (default 300 x 300 x 60, CPML 8) for
  * the plain substrate: as AUTO schedules it, and under FDTD_FLAG_KERNEL_DIRECT (the two-launch schedule a context with Lorentz media
    runs); with --parent-lib DIR also on a libfdtd_hip.so built from the commit before Lorentz media — the plain case must be
    unchanged within run-to-run noise;
  * the substrate as a Lorentz medium of K poles (default 1) with the same eps_inf: class operator + k_lorentz.
It also prints the dispersive edges and the bytes k_lorentz moves per launch (per edge 8 (V) + 4 (vi) + 4 (w) + 8 (v_prev) + 16 K).
Run under rocprofv3 --kernel-trace --stats (a run of its own) for k_lorentz's duration; `python tools/kernel_resources.py k_lorentz`
reports its registers and scratch.
"""
import argparse
import ctypes
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "fdtd-solver-antennas_amd"
imp = lambda m: importlib.import_module(PKG + "." + m)


def make_sim(n, poles, nr_ts):
    sc, sim = imp("scene"), imp("simulation")
    w = imp("workloads").patch_workload("timing", nx=n[0], ny=n[1], nz=n[2])
    if poles:
        sub = w.scene.materials[0]
        k = np.arange(poles)
        lor = sc.LorentzMaterial(sub.name, sub.eps_r, sub.kappa, boxes=sub.boxes,
                                 medium=imp("lorentz").LorentzMedium(sub.eps_r, sub.kappa, 2 * np.pi * 1e9 * (1.0 + k), 2 * np.pi * 5e9 * (1.0 + k),
                                                                     np.full(poles, 1e9)))
        w.scene.materials[0] = lor
    return sim.Simulation(w.grid, sc.voxelize(w.scene, w.grid), f0=w.f0, fc=w.fc, boundary="CPML", cpml_cells=8, nr_ts=nr_ts, end_criteria=0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--grid", nargs=3, type=int, default=[300, 300, 60])
    ap.add_argument("--poles", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warm", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    capi = imp("_capi")
    lib = capi.load_hip_library()
    parent = capi.bind(ctypes.CDLL(os.path.join(a.parent_lib, capi.HIP_LIB_NAME))) if a.parent_lib else None
    n = tuple(a.grid)
    total = a.warm + a.rounds * a.steps + 16
    runs = []
    if parent is not None:
        runs += [("plain substrate, parent build, AUTO", parent, 0, 0),
                 ("plain substrate, parent build, two launches (DIRECT)", parent, 0, capi.FLAG_KERNEL_DIRECT)]
    runs += [("plain substrate, this build, AUTO", lib, 0, 0),
             ("plain substrate, this build, two launches (DIRECT)", lib, 0, capi.FLAG_KERNEL_DIRECT),
             (f"Lorentz substrate, {a.poles} pole(s), classes + k_lorentz", lib, a.poles, 0)]
    eng = []
    for tag, l, poles, flags in runs:
        r = make_sim(n, poles, total)
        e = r.build(l, flags=flags)
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
        d = r.lorentz
        edges = "no dispersive edges"
        if d is not None:
            box = sum(int(np.prod(w.shape[:2])) * ((w.shape[2] + 6) & ~3) for w in d.w)      # (an upper bound of the widened boxes)
            edges = f"{len(d)} dispersive edges in boxes of {sum(int(w.size) for w in d.w)}, ~{box * (24 + 16 * d.K) / 1e6:.2f} MB per k_lorentz launch"
        print(f"patch {n[0]}x{n[1]}x{n[2]} CPML-8, {tag}: median {np.median(v):.2f} us/timestep (min {v.min():.2f}, max {v.max():.2f}; "
              f"{a.rounds} rounds of {a.steps}), operator {e.operator_form()[0]}, {info['launches_per_timestep']} launches/timestep, "
              f"resident {info['resident']}, {edges}", flush=True)
        e.close()


if __name__ == "__main__":
    main()
