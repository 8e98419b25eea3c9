"""Magnetic materials: what a magnetic substrate costs a run (k_magnetic, csrc/magnetic.hip, and the schedule such a context takes),
and what the same scene would cost in raw operator form.

  python tools/magnetic_timing.py [--parent-lib DIR] [--grid NX NY NZ]

Wall clock of fdtd_run per timestep (a device synchronise ends every timed block), contexts of one process in interleaved rounds,
median (min, max), on the patch workload (default 300 x 300 x 60, CPML 8) for
  * no magnetic material: as AUTO schedules it, and under FDTD_FLAG_KERNEL_DIRECT (the two-launch schedule a context with magnetic
    faces runs); with --parent-lib DIR also on a libfdtd_hip.so built from the commit before magnetic materials — the no-magnetic
    case must be unchanged within run-to-run noise;
  * the substrate with mu_r = 2 and magnetic loss: class operator + k_magnetic (what the product runs);
  * the same scene in RAW form with the magnetic faces in ii / iv (magnetic.raw_ii_iv), as AUTO schedules it: 48 B per cell and
    timestep of coefficients over the whole grid against ~17 B per magnetic face.
Run under rocprofv3 --kernel-trace --stats (a run of its own) for k_magnetic's duration; `python tools/kernel_resources.py k_magnetic`
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


def make_sim(n, magnetic, nr_ts):
    sc, sim = imp("scene"), imp("simulation")
    w = imp("workloads").patch_workload("timing", nx=n[0], ny=n[1], nz=n[2])
    if magnetic:
        sub = w.scene.materials[0]
        sub.mu_r, sub.sigma_m = 2.0, 50.0
    return sim.Simulation(w.grid, sc.voxelize(w.scene, w.grid), f0=w.f0, fc=w.fc, boundary="CPML", cpml_cells=8, nr_ts=nr_ts, end_criteria=0.0)


def build_raw(run, lib, flags):
    """The engine of `run` with the operator in raw form and the magnetic faces in it (tests and this record only)."""
    mag, op = run.magnetic, run.op

    class Raw:
        def classes(self, *a):
            return None

        def raw(self, k0=0, nk=None):
            vv, vi, _, _ = op.raw(k0, nk)
            ii, iv = imp("magnetic").raw_ii_iv(op, mag, k0, nk)
            return vv, vi, ii, iv
    saved = run.magnetic, run.device_operator, run.use_classes
    run.magnetic, run.device_operator, run.use_classes, run._op = None, False, False, Raw()
    try:
        return run.build(lib, flags=flags)
    finally:
        run.magnetic, run.device_operator, run.use_classes = saved
        run._op = op


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--grid", nargs=3, type=int, default=[300, 300, 60])
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
        runs += [("no magnetic, parent build, AUTO", parent, False, 0, False),
                 ("no magnetic, parent build, two launches (DIRECT)", parent, False, capi.FLAG_KERNEL_DIRECT, False)]
    runs += [("no magnetic, this build, AUTO", lib, False, 0, False),
             ("no magnetic, this build, two launches (DIRECT)", lib, False, capi.FLAG_KERNEL_DIRECT, False),
             ("magnetic substrate, classes + k_magnetic", lib, True, 0, False),
             ("magnetic substrate, raw form, AUTO", lib, True, 0, True)]
    eng = []
    for tag, l, mag, flags, raw in runs:
        r = make_sim(n, mag, total)
        e = build_raw(r, l, flags) if raw else r.build(l, flags=flags)
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
        m = r.magnetic
        faces = "no magnetic faces" if m is None else f"{len(m)} magnetic faces in boxes of {sum(int(c.size) for c in m.cls)}, {m.ncls} classes"
        print(f"patch {n[0]}x{n[1]}x{n[2]} CPML-8, {tag}: median {np.median(v):.2f} us/timestep (min {v.min():.2f}, max {v.max():.2f}; "
              f"{a.rounds} rounds of {a.steps}), operator {e.operator_form()[0]}, {info['launches_per_timestep']} launches/timestep, "
              f"resident {info['resident']}, {faces}", flush=True)
        e.close()


if __name__ == "__main__":
    main()
