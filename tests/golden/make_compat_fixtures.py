#!/usr/bin/env python3
"""Records the numbers the reference's solver files produce when they run over this package's openEMS / CSXCAD mirror
(fdtd-solver-antennas_amd/compat) with the CPU oracle as the engine, so that tests/test_compat_reference_cpu.py can hold
this package's plugin functions against them without the reference being present:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_compat_fixtures.py <directory of the reference checkout>

Writes compat_reference.npz: for every run the test file names, theta / phi [rad], the dBi grid and the mesh shape;
the closed-form design values over the test file's random inputs; the step count and end energy of the tutorial run."""
import contextlib
import ctypes
import importlib
import io
import os
import runpy
import subprocess
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
PKG = "fdtd-solver-antennas_amd"


def main(ref):
    import test_compat_reference_cpu as T
    sys.path.insert(0, os.path.join(ROOT, PKG, "compat"))
    sys.path.insert(0, ref)
    if not hasattr(os, "add_dll_directory"):
        os.add_dll_directory = lambda p: None
    capi = importlib.import_module(PKG + "._capi")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    ora = capi.bind(ctypes.CDLL(os.path.join(ROOT, "oracle", "libfdtd_oracle.so")))
    from antenna_sim.models import PatchAntennaParams
    tmp = tempfile.mkdtemp()
    dll = os.path.join(tmp, "dll")
    os.makedirs(dll)
    open(os.path.join(dll, "openEMS.dll"), "w").close()
    out = {}

    def keep(key, res, prep):
        assert res.ok, res.message
        out[key + "/theta"] = np.asarray(res.theta, np.float64)
        out[key + "/phi"] = np.asarray(res.phi, np.float64)
        out[key + "/intensity"] = np.asarray(res.intensity, np.float64)
        out[key + "/grid"] = np.asarray(prep.FDTD.sim.grid.shape, np.int64)

    p = PatchAntennaParams.from_user_units(frequency_ghz=2.45, er=4.3, h_mm=1.6, loss_tangent=0.02)
    feed = importlib.import_module("antenna_sim.solver_fdtd_openems_microstrip").FeedDirection
    with contextlib.redirect_stdout(io.StringIO()):
        fx = importlib.import_module("antenna_sim.solver_fdtd_openems_fixed")
        prep = fx.prepare_openems_patch_fixed(p, dll_dir=dll, work_dir=os.path.join(tmp, "fixed"))
        prep.FDTD.NrTS = 4000
        prep.FDTD._lib = ora
        keep("fixed", fx.run_prepared_openems_fixed(prep, frequency_hz=2.45e9, verbose=0), prep)
        for module, prep_name, run_name, _ in T.VARIANTS:
            mod = importlib.import_module("antenna_sim." + module)
            if "multi" in module:
                arg = [SimpleNamespace(name=f"P{n}", params=p, center_x_m=cx, center_y_m=cy, center_z_m=0.0, feed_direction=feed.NEG_X,
                                       rot_x_deg=0.0, rot_y_deg=0.0, rot_z_deg=0.0) for n, (cx, cy) in enumerate(T.VARIANT_ARRAY)]
                prep = getattr(mod, prep_name)(arg, dll_dir=dll, work_dir=os.path.join(tmp, module), **T.VARIANT_ARRAY_KW)
            else:
                prep = getattr(mod, prep_name)(p, dll_dir=dll, work_dir=os.path.join(tmp, module))
            prep.FDTD.NrTS = T.variant_nrts(module)
            prep.FDTD._lib = ora
            keep("variant/" + module, getattr(mod, run_name)(prep, frequency_hz=2.45e9, verbose=0), prep)
        multi = importlib.import_module("antenna_sim.solver_fdtd_openems_microstrip_multi_3d")
        for case, (items, kw) in T.PLACEMENTS.items():
            arg = [SimpleNamespace(name=f"P{n}", params=p, center_x_m=cx, center_y_m=cy, center_z_m=cz, feed_direction=getattr(feed, fd),
                                   rot_x_deg=float(rx), rot_y_deg=float(ry), rot_z_deg=float(rz)) for n, (cx, cy, cz, fd, rx, ry, rz) in enumerate(items)]
            pr = multi.prepare_openems_microstrip_multi_3d(arg, dll_dir=dll, work_dir=os.path.join(tmp, "pl_" + case), theta_step_deg=4.0, phi_step_deg=10.0, **kw)
            pr.FDTD.NrTS = 2500
            pr.FDTD._lib = ora
            keep("placement/" + case, multi.run_prepared_openems_microstrip_multi_3d(pr, frequency_hz=2.45e9, verbose=0), pr)
        for (variant, design, kw), tid in zip(T.OPTIONS, T.OPTION_IDS):
            module, prep_name, run_name = T.OPTION_MODULES[variant]
            mod = importlib.import_module("antenna_sim." + module)
            kw_ref = dict(kw)
            if "feed_direction" in kw:
                kw_ref["feed_direction"] = getattr(feed, kw["feed_direction"])
            pr = getattr(mod, prep_name)(PatchAntennaParams.from_user_units(**design), dll_dir=dll, work_dir=os.path.join(tmp, "opt_" + tid), **kw_ref)
            pr.FDTD.NrTS = 1500
            pr.FDTD._lib = ora
            keep("option/" + tid, getattr(mod, run_name)(pr, frequency_hz=design["frequency_ghz"] * 1e9, verbose=0), pr)

    ref_phys = importlib.import_module("antenna_sim.physics")
    ref_models = importlib.import_module("antenna_sim.models")
    design, width, model, refused = [], [], [], []
    for f, er, h, kw in T.random_designs():
        design.append([float(x) for x in ref_phys.design_patch_for_frequency(f, er, h)])
        width.append(float(importlib.import_module("antenna_sim.solver_fdtd_openems_microstrip").calculate_microstrip_width(f, er, h)))
        try:
            r = ref_models.PatchAntennaParams.from_user_units(**kw)
        except Exception:      # noqa: BLE001  (a bound of the reference's model: ours must refuse too)
            r = None
        refused.append(r is None)
        # a field the model leaves unset (None) is stored as NaN
        model.append([float("nan") if r is None or getattr(r, n) is None else float(getattr(r, n)) for n in T.MODEL_FIELDS])
    out["design/patch"], out["design/feed_width"], out["design/model"] = np.array(design), np.array(width), np.array(model)
    out["design/refused"] = np.array(refused)

    capi.load_hip_library = lambda *a, **k: ora
    tempfile.tempdir = tmp
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        g = runpy.run_path(os.path.join(ref, "test_openems.py"), run_name="__main__")
    assert "SUCCESS: Tutorial-aligned patch simulation ran!" in buf.getvalue() and "FAILED" not in buf.getvalue()
    fd = g["FDTD"]
    out["tutorial/grid"] = np.asarray(fd.sim.grid.shape, np.int64)
    out["tutorial/steps_energy_db"] = np.array([fd.stats.steps, fd.stats.energy_db], np.float64)
    np.savez_compressed(os.path.join(OUT, "compat_reference.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(os.path.abspath(sys.argv[1]))
