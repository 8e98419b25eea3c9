"""Lumped elements: what one element costs a run (k_lumped, csrc/lumped.hip, and the schedule a context with elements takes).

  python tools/lumped_timing.py [--parent-lib DIR]

Wall clock of fdtd_run per timestep (a device synchronise ends every timed block), contexts of one process in interleaved rounds,
median (min, max), for
  * the open test scene (26 x 24 x 22, CPML 4, a port) with and without one series R-L-C on one edge,
  * the patch workload on 300 x 300 x 60 (CPML 8) with and without one series R-L-C from patch to ground (4 edges),
  * the patch workload on 56 x 55 x 50 (the plugin's default size): as AUTO schedules it, under FDTD_FLAG_KERNEL_DIRECT, and with
    the element — a context with an element leaves the resident / one-launch schedule.
--parent-lib DIR: a libfdtd_hip.so built from the commit before lumped elements, for the runs without an element (the same scene
under FDTD_FLAG_KERNEL_DIRECT, the two-launch schedule a context with elements runs).  Run under rocprofv3 --kernel-trace --stats
(a run of its own) for k_lumped's duration.
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


def open_scene(element):
    sc, G = imp("scene"), imp("grid")
    g = G.RectGrid(*[np.arange(k) * 1e-3 for k in (26, 24, 22)])
    s = sc.Scene(unit=1e-3)
    s.add_lumped_port(1, 50.0, [12, 11, 8], [12, 11, 12], "z", 1.0)
    if element:
        s.add_lumped_element("trap", "z", R=5.0, L=3e-9, C=0.2e-12, kind="series").add_box([15, 11, 10], [15, 11, 11])
    return g, s, dict(f0=6e9, fc=4e9, boundary="CPML", cpml_cells=4)


def patch_scene(n, element):
    w = imp("workloads").patch_workload("timing", nx=n[0], ny=n[1], nz=n[2])
    if element:
        w.scene.add_lumped_element("choke", "z", R=1.0, L=5e-9, C=1e-12, kind="series").add_box([6, 0, 0], [6, 0, 1.6])
    return w.grid, w.scene, dict(f0=w.f0, fc=w.fc, boundary="CPML", cpml_cells=8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warm", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    capi, sc, sim = imp("_capi"), imp("scene"), imp("simulation")
    lib = capi.load_hip_library()
    parent = capi.bind(ctypes.CDLL(os.path.join(a.parent_lib, capi.HIP_LIB_NAME))) if a.parent_lib else None
    D = capi.FLAG_KERNEL_DIRECT
    cases = [("open scene 26x24x22 CPML-4", lambda el: open_scene(el), 1),
             ("patch 300x300x60 CPML-8", lambda el: patch_scene((300, 300, 60), el), 1),
             ("patch 56x55x50 CPML-8", lambda el: patch_scene((56, 55, 50), el), 4)]
    for name, make, mult in cases:
        steps = a.steps * mult
        runs = []
        if parent is not None:
            runs.append(("no element, parent build, two launches (DIRECT)", parent, False, D))
        runs += [("no element, this build, two launches (DIRECT)", lib, False, D), ("no element, this build, AUTO", lib, False, 0),
                 ("one element, this build, AUTO", lib, True, 0)]
        eng = []
        for tag, l, el, flags in runs:
            g, s, kw = make(el)
            r = sim.Simulation(g, sc.voxelize(s, g), nr_ts=a.warm + a.rounds * steps + 16, end_criteria=0.0, **kw)
            e = r.build(l, flags=flags)
            e.run(a.warm)
            e.energy()
            eng.append((tag, e, r, []))
        for _ in range(a.rounds):
            for tag, e, r, t in eng:
                t0 = time.perf_counter()
                e.run(steps)
                e.energy()
                t.append((time.perf_counter() - t0) / steps * 1e6)
        for tag, e, r, t in eng:
            info, v = e.schedule_info(), np.array(t)
            print(f"{name}, {tag}: median {np.median(v):.2f} us/timestep (min {v.min():.2f}, max {v.max():.2f}; {a.rounds} rounds of {steps}), "
                  f"{info['launches_per_timestep']} launches/timestep, resident {info['resident']}, {r.element_stepped.size if hasattr(r, 'element_stepped') else 0} "
                  f"element edges", flush=True)
            e.close()


if __name__ == "__main__":
    main()
