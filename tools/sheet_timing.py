"""Conducting sheets: what they cost per timestep and what they give, on the reference's scenes.

  python tools/sheet_timing.py            fixed default scene: us per timestep PEC against copper (wall clock of fdtd_run over N
                                          timesteps after a warm-up), then efficiency / gain per metal at the default tan delta (0)
  python tools/sheet_timing.py --multi    the two-patch multi-3D MUR scene with copper sheets, N timesteps (run it under
                                          rocprofv3 --kernel-trace --stats for k_sheet's share of the timestep)
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
s = importlib.import_module(PKG + ".solver_fdtd_hip")
P = importlib.import_module(PKG + ".params").PatchAntennaParams


def step_time(prep, n=2000, warm=200):
    prep.FDTD.Run(prep.sim_path, setup_only=True)
    sim = prep.FDTD.sim
    e = sim.engine
    e.run(warm)
    t0 = time.perf_counter()
    e.run(n)
    dt = (time.perf_counter() - t0) / n
    return dt * 1e6, e.schedule_info(), e.operator_form(), 0 if sim.sheets is None else len(sim.sheets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--multi", action="store_true")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--work", default="fdtd_hip_out_sheet_timing")
    a = ap.parse_args()
    if a.multi:
        p = P.from_user_units(frequency_ghz=2.45, er=4.3, h_mm=1.6, metal="copper")
        inst = [s.PatchInstance(f"P{n}", p, (ix - 0.5) * 0.09, 0.0, 0.0, s.FeedDirection.NEG_X) for n, ix in enumerate([0, 1])]
        prep = s.prepare_hip_microstrip_multi_3d(inst, boundary="MUR", work_dir=a.work, metal_loss=True)
        assert prep.ok, prep.message
        us, info, form, n = step_time(prep, a.steps)
        print(f"multi-3D two patches, MUR, copper sheets: {us:.2f} us/timestep, {n} sheet edges, operator {form}, schedule {info}")
        return
    p = P.from_user_units(frequency_ghz=2.45, er=4.3, h_mm=1.6, metal="copper")
    for loss in (False, True):
        prep = s.prepare_hip_patch_fixed(p, work_dir=a.work, metal_loss=loss)
        assert prep.ok, prep.message
        us, info, form, n = step_time(prep, a.steps)
        print(f"fixed default scene, {'copper sheets' if loss else 'PEC'}: {us:.2f} us/timestep, {n} sheet edges, operator {form}, "
              f"{info['launches_per_timestep']} launches/timestep, resident {info['resident']}")
    for metal in (None, "copper", "aluminum", "gold", "silver", "tin"):
        p = P.from_user_units(frequency_ghz=2.45, er=4.3, h_mm=1.6, metal=metal or "copper")   # the default tan delta (0)
        prep = s.prepare_hip_patch_fixed(p, work_dir=a.work, metal_loss=metal is not None)
        res = s.run_prepared_hip(prep, frequency_hz=2.45e9, verbose=0)
        assert res.ok, res.message
        print(f"fixed scene, default tan d, {metal or 'PEC'}: eta {res.radiation_efficiency:.4f}, gain {res.gain_dBi:.2f} dBi, "
              f"realised {res.realized_gain_dBi:.2f} dBi, Dmax {10 * np.log10(res.Dmax):.2f} dBi, {res.stats['steps']} steps")


if __name__ == "__main__":
    main()
