"""Debye media: what the per-timestep correction (k_debye, csrc/dispersion.hip) and substrate_dispersion=True cost.

  python tools/debye_timing.py --kernel GRID THICK K    one synthetic case, N timesteps: a PEC box GRID ("ns": 300 x 300 x 60,
                                          "default": 56 x 55 x 50) with a Debye slab THICK cells thick across it, K poles.  Prints the
                                          dispersive edges and the bytes k_debye must move per launch — per edge 8 (V) + 4 (vi) + 4 (w)
                                          + 8 (v_prev) + 8 K (u) — and the wall clock per timestep.  Run it under
                                          rocprofv3 --kernel-trace --stats (a run of its own) for k_debye's duration.
  python tools/debye_timing.py --whole    the 3-D microstrip scene (2.45 GHz, FR-4, MUR): us per timestep of substrate_dispersion
                                          False as AUTO schedules it, False under the two-launch schedule (FDTD_FLAG_KERNEL_DIRECT: the
                                          schedule a context with media runs), and True — interleaved blocks of N timesteps in one
                                          process, median of the rounds.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import importlib  # noqa: E402

PKG = "fdtd-solver-antennas_amd"
imp = lambda m: importlib.import_module(PKG + "." + m)
GRIDS = {"ns": (300, 300, 60), "default": (56, 55, 50)}


def kernel_case(grid, thick, K, steps, warm):
    capi, sc, sim, d, G = imp("_capi"), imp("scene"), imp("simulation"), imp("dispersion"), imp("grid")
    n = GRIDS[grid]
    g = G.RectGrid(*[np.arange(k) * 0.4e-3 for k in n])
    med = d.fit_constant_loss_tangent(4.3, 0.02, 2.45e9, 1.2e9, 3.7e9, K=K)
    s = sc.Scene(unit=0.4e-3)
    z0 = n[2] // 3
    s.add_debye_material("sub", med.eps_inf, 0.0, med.delta_eps, med.tau).add_box([2, 2, z0], [n[0] - 3, n[1] - 3, z0 + thick])
    s.add_lumped_port(1, 50.0, [n[0] // 2, n[1] // 2, z0], [n[0] // 2, n[1] // 2, z0 + thick], "z", 1.0)
    run = sim.Simulation(g, sc.voxelize(s, g), f0=2.45e9, fc=1.2e9, boundary="PEC", nr_ts=steps + warm, end_criteria=0.0)
    e = run.build(capi.load_hip_library())
    e.run(warm)
    e.energy()
    t0 = time.perf_counter()
    e.run(steps)
    e.energy()
    us = (time.perf_counter() - t0) / steps * 1e6
    edges = len(run.debye)
    box = sum(int(np.prod(w.shape)) for w in run.debye.w)
    per_edge = 8 + 4 + 4 + 8 + 8 * K
    print(f"k_debye case {grid} {n[0]}x{n[1]}x{n[2]}, slab {thick} cells, K = {K}: {edges} dispersive edges ({box} in the boxes), "
          f"{per_edge} B/edge = {edges * per_edge / 1e6:.3f} MB per launch; whole timestep {us:.2f} us wall clock, "
          f"schedule {e.schedule_info()['launches_per_timestep']} launches + k_debye, {steps} timesteps")


def whole(steps, rounds, work):
    capi, s, P = imp("_capi"), imp("solver_fdtd_hip"), imp("params").PatchAntennaParams
    p = P.from_user_units(frequency_ghz=2.45, er=4.3, h_mm=1.6, loss_tangent=0.02)
    eng = {}
    for tag, on, flags in (("kappa, AUTO schedule", False, 0), ("kappa, two launches", False, capi.FLAG_KERNEL_DIRECT), ("Debye", True, 0)):
        prep = s.prepare_hip_microstrip_patch_3d(p, work_dir=os.path.join(work, tag.replace(" ", "_").replace(",", "")), substrate_dispersion=on)
        assert prep.ok, prep.message
        prep.FDTD.Run(prep.sim_path, setup_only=True)
        sim = prep.FDTD.sim
        e = sim.engine
        if flags:
            e.close()
            e = sim.build(sim.lib, flags=flags)
        e.run(200)
        e.energy()
        eng[tag] = (e, sim)
    t = {k: [] for k in eng}
    for _ in range(rounds):
        for tag, (e, _) in eng.items():
            t0 = time.perf_counter()
            e.run(steps)
            e.energy()
            t[tag].append((time.perf_counter() - t0) / steps * 1e6)
    for tag, (e, sim) in eng.items():
        info = e.schedule_info()
        v = np.array(t[tag])
        print(f"microstrip 3-D {'x'.join(map(str, sim.grid.shape))}, {tag}: median {np.median(v):.2f} us/timestep (min {v.min():.2f}, max {v.max():.2f}, "
              f"{rounds} rounds of {steps}), {info['launches_per_timestep']} launches/timestep, resident {info['resident']}, "
              f"{0 if sim.debye is None else len(sim.debye)} dispersive edges")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", nargs=3, metavar=("GRID", "THICK", "K"))
    ap.add_argument("--whole", action="store_true")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warm", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--work", default="fdtd_hip_out_debye_timing")
    a = ap.parse_args()
    if a.kernel:
        kernel_case(a.kernel[0], int(a.kernel[1]), int(a.kernel[2]), a.steps, a.warm)
    if a.whole:
        whole(a.steps, a.rounds, a.work)


if __name__ == "__main__":
    main()
