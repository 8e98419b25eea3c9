"""INTEGRATION.md §A, exercised: the reference's own solver files run unmodified on top of
fdtd-solver-antennas_amd/compat/{openEMS,CSXCAD} (their prepare drawing into our API mirror, their run_prepared returning
an OpenEMSResult produced by our engine path, the oracle injected as the engine), and this package's mirrored plugin
functions return the SAME results.  What the reference's files returned over the mirror is recorded in
tests/golden/compat_reference.npz (tests/golden/make_compat_fixtures.py), so the comparisons run without the reference;
the tests that read the reference's signatures, dataclasses or plotting code, or run its quasi-2D solver, need a checkout
of it and skip without one."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg

REF = "/root/reference"
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "antenna_sim")), reason="reference not present")
GOLD = os.path.join(ROOT, "tests", "golden", "compat_reference.npz")


def _gold(key):
    with np.load(GOLD) as z:
        return {k[len(key) + 1:]: z[k] for k in z.files if k.startswith(key + "/")}


def _params(**kw):
    return pkg("params").PatchAntennaParams.from_user_units(**(kw or dict(frequency_ghz=2.45, er=4.3, h_mm=1.6, loss_tangent=0.02)))


def _same_as_recorded(key, prep, res):
    """The run of this package's plugin function against what the reference's solver file returned over the mirror."""
    g = _gold(key)
    assert res.ok, res.message
    assert list(prep.FDTD.sim.grid.shape) == g["grid"].tolist()
    assert np.asarray(res.intensity).shape == g["intensity"].shape
    assert np.allclose(res.theta, g["theta"], rtol=0, atol=1e-12) and np.allclose(res.phi, g["phi"], rtol=0, atol=1e-12)
    assert np.max(np.abs(np.asarray(res.intensity) - g["intensity"])) < 1e-9


def test_reference_solver_runs_on_compat_shims(oracle_lib, tmp_path):
    """The fixed scene (the reference GUI's default): prepare_hip_patch_fixed + run_prepared_hip, 4 000 timesteps on the oracle, against the
    dBi grid the reference's solver_fdtd_openems_fixed returned over the mirror for the same input."""
    p = _params()
    s = pkg("solver_fdtd_hip")
    own = s.prepare_hip_patch_fixed(p, work_dir=str(tmp_path / "own"), lib=oracle_lib)
    assert own.ok, own.message
    assert isinstance(own.FDTD, pkg("openems_api").openEMS)
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "scene_calls.json")))["fixed_2g45"]["calls"]
    assert [c["op"] for c in json.loads(json.dumps(own.FDTD.calls))] == [c["op"] for c in gold]
    own.FDTD.NrTS = 4000                       # keep the CPU run short
    mine = s.run_prepared_hip(own, frequency_hz=2.45e9, verbose=0)
    assert mine.is_dBi and np.asarray(mine.intensity).shape == (90, 2)
    assert 3.0 < np.asarray(mine.intensity).max() < 9.5
    assert np.allclose(mine.phi, [0.0, np.pi / 2])
    _same_as_recorded("fixed", own, mine)      # the mirrored plugin == the reference's own code


VARIANTS = [
    ("solver_fdtd_openems_microstrip", "prepare_openems_microstrip_patch", "run_prepared_openems_microstrip", (91, 2)),
    ("solver_fdtd_openems_microstrip_3d", "prepare_openems_microstrip_patch_3d", "run_prepared_openems_microstrip_3d", (91, 73)),
    ("solver_fdtd_openems", "prepare_openems_patch", "run_prepared_openems", (91, 181)),
    ("solver_fdtd_openems_microstrip_multi_3d", "prepare_openems_microstrip_multi_3d", "run_prepared_openems_microstrip_multi_3d", (91, 73)),
]
VARIANT_ARRAY = [((ix - 0.5) * 0.07, (iy - 0.5) * 0.07) for ix, iy in [(0, 0), (1, 0)]]
VARIANT_ARRAY_KW = dict(theta_step_deg=2.0, phi_step_deg=5.0, mesh_quality=1)


def variant_nrts(module):
    return 16000 if "multi" in module else 3000      # (the array's graded mesh has the smaller timestep: its pulse alone is ~12 000 long)


@pytest.mark.parametrize("module,prep_name,run_name,shape", VARIANTS, ids=[v[0].replace("solver_fdtd_openems", "ref") or "ref" for v in VARIANTS])
def test_every_reference_solver_file_runs_on_the_shims(oracle_lib, tmp_path, module, prep_name, run_name, shape):
    """The other four solver files of the reference — inset-fed microstrip, microstrip-3D, the legacy variant and the multi-patch
    array — ran UNMODIFIED over compat/{openEMS,CSXCAD} (prepare, run on the oracle with NrTS cut, their own post-processing and
    conversion to dBi; recorded): the mirrored plugin function of this package, given the same input, returns the SAME result — same
    mesh, same engine, same post-processing and conversion, end to end."""
    s = pkg("solver_fdtd_hip")
    p = _params()
    own_prep = {"solver_fdtd_openems_microstrip": s.prepare_hip_microstrip_patch, "solver_fdtd_openems_microstrip_3d": s.prepare_hip_microstrip_patch_3d,
                "solver_fdtd_openems": s.prepare_hip_patch, "solver_fdtd_openems_microstrip_multi_3d": s.prepare_hip_microstrip_multi_3d}[module]
    if "multi" in module:
        own_arg = [s.PatchInstance(f"P{n}", p, cx, cy, 0.0, s.FeedDirection.NEG_X) for n, (cx, cy) in enumerate(VARIANT_ARRAY)]
        own = own_prep(own_arg, work_dir=str(tmp_path / "own"), lib=oracle_lib, **VARIANT_ARRAY_KW)
    else:
        own = own_prep(p, work_dir=str(tmp_path / "own"), lib=oracle_lib)
    assert own.ok, own.message
    own.FDTD.NrTS = variant_nrts(module)
    mine = s.run_prepared_hip(own, frequency_hz=2.45e9, verbose=0)
    assert mine.ok, mine.message
    inten = np.asarray(mine.intensity)
    assert inten.shape == shape and np.isfinite(inten).all() and 3.0 < inten.max() < 13.0
    _same_as_recorded("variant/" + module, own, mine)


@needs_reference
def test_plugin_signatures_are_the_references(monkeypatch):
    """Every keyword a caller of the reference's probe / prepare / run_prepared functions may pass exists, with the same default, on the
    function that replaces it (`dll_dir` is accepted and optional here; only the default work directories are named differently)."""
    import importlib
    import inspect
    compat = os.path.join(ROOT, "fdtd-solver-antennas_amd", "compat")
    monkeypatch.syspath_prepend(REF)
    monkeypatch.syspath_prepend(compat)
    monkeypatch.setattr(sys, "dont_write_bytecode", True)
    if not hasattr(os, "add_dll_directory"):
        monkeypatch.setattr(os, "add_dll_directory", lambda p: None, raising=False)
    for m in [k for k in sys.modules if k.split(".")[0] in ("openEMS", "CSXCAD", "antenna_sim")]:
        monkeypatch.delitem(sys.modules, m)
    s = pkg("solver_fdtd_hip")
    pairs = [("solver_fdtd_openems_fixed", "probe_openems_fixed", "probe_hip"),
             ("solver_fdtd_openems_fixed", "prepare_openems_patch_fixed", "prepare_hip_patch_fixed"),
             ("solver_fdtd_openems_fixed", "run_prepared_openems_fixed", "run_prepared_hip"),
             ("solver_fdtd_openems_microstrip", "prepare_openems_microstrip_patch", "prepare_hip_microstrip_patch"),
             ("solver_fdtd_openems_microstrip", "run_prepared_openems_microstrip", "run_prepared_hip"),
             ("solver_fdtd_openems_microstrip_3d", "prepare_openems_microstrip_patch_3d", "prepare_hip_microstrip_patch_3d"),
             ("solver_fdtd_openems_microstrip_3d", "run_prepared_openems_microstrip_3d", "run_prepared_hip"),
             ("solver_fdtd_openems_microstrip_multi_3d", "prepare_openems_microstrip_multi_3d", "prepare_hip_microstrip_multi_3d"),
             ("solver_fdtd_openems_microstrip_multi_3d", "run_prepared_openems_microstrip_multi_3d", "run_prepared_hip"),
             ("solver_fdtd_openems", "prepare_openems_patch", "prepare_hip_patch"),
             ("solver_fdtd_openems", "run_prepared_openems", "run_prepared_hip")]
    for module, ref_name, own_name in pairs:
        ref = inspect.signature(getattr(importlib.import_module("antenna_sim." + module), ref_name)).parameters
        own = inspect.signature(getattr(s, own_name)).parameters
        for name, par in ref.items():
            assert name in own, f"{own_name} lacks {name!r} of {ref_name}"
            if par.default is not inspect.Parameter.empty and name not in ("work_dir", "dll_dir"):
                assert own[name].default == par.default, f"{own_name}({name}=...) defaults to {own[name].default!r}, {ref_name} to {par.default!r}"


PLACEMENTS = {
    "rotated_pair_manual_box": ([(-0.04, 0.0, 0.0, "NEG_X", 0, 0, 0), (0.045, 0.01, 0.02, "POS_Y", 0, 0, 90)],
                                dict(boundary="PML_8", mesh_quality=2, nf_center_mode="centroid", simbox_mode="manual", manual_size_mm=(260.0, 240.0, 220.0))),
    "tilted": ([(0.0, 0.0, 0.0, "NEG_X", 30, 0, 0)], dict(boundary="MUR", mesh_quality=1)),
    "cube_faces": ([(0.0, 0.0, 0.04, "NEG_X", 0, 0, 0), (0.04, 0.0, 0.0, "NEG_Y", 0, 90, 0)], dict(boundary="MUR", mesh_quality=1)),
}


@pytest.mark.parametrize("case", ["rotated_pair_manual_box", "tilted", "cube_faces"])
def test_multi_patch_placements_equal_the_reference(oracle_lib, tmp_path, case):
    """Rotated, tilted and cube-face placements, automatic and manual simulation box, origin / centroid far-field centre, MUR / PML_8:
    prepare_hip_microstrip_multi_3d + run_prepared_hip against the reference's multi-patch solver over the shims (recorded) — same mesh,
    same dBi grid."""
    import contextlib
    import io
    s = pkg("solver_fdtd_hip")
    p = _params()
    items, kw = PLACEMENTS[case]
    own_arg = [s.PatchInstance(f"P{n}", p, cx, cy, cz, getattr(s.FeedDirection, fd), rot_x_deg=float(rx), rot_y_deg=float(ry), rot_z_deg=float(rz))
               for n, (cx, cy, cz, fd, rx, ry, rz) in enumerate(items)]
    with contextlib.redirect_stdout(io.StringIO()):
        po = s.prepare_hip_microstrip_multi_3d(own_arg, work_dir=str(tmp_path / "o"), theta_step_deg=4.0, phi_step_deg=10.0, lib=oracle_lib, **kw)
        assert po.ok, po.message
        po.FDTD.NrTS = 2500
        ro = s.run_prepared_hip(po, frequency_hz=2.45e9, verbose=0)
    _same_as_recorded("placement/" + case, po, ro)


OPTIONS = [
    ("microstrip", dict(frequency_ghz=2.45, er=4.3, h_mm=1.6, loss_tangent=0.02), dict(feed_direction="NEG_Y", feed_line_length_mm=14.0)),
    ("microstrip_3d", dict(frequency_ghz=2.45, er=4.3, h_mm=1.6, loss_tangent=0.02), dict(feed_direction="POS_X", boundary="PML_8", mesh_quality=1, phi_step_deg=15.0)),
    ("fixed", dict(frequency_ghz=3.5, er=10.2, h_mm=1.27, loss_tangent=0.002, L_mm=12.0, W_mm=16.0), {}),
    ("legacy", dict(frequency_ghz=2.45, er=2.2, h_mm=0.8, loss_tangent=0.001), {}),
]
OPTION_IDS = ["microstrip_negy", "microstrip3d_posx_pml_q1", "fixed_explicit_LW", "legacy_er2.2"]
OPTION_MODULES = {
    "fixed": ("solver_fdtd_openems_fixed", "prepare_openems_patch_fixed", "run_prepared_openems_fixed"),
    "microstrip": ("solver_fdtd_openems_microstrip", "prepare_openems_microstrip_patch", "run_prepared_openems_microstrip"),
    "microstrip_3d": ("solver_fdtd_openems_microstrip_3d", "prepare_openems_microstrip_patch_3d", "run_prepared_openems_microstrip_3d"),
    "legacy": ("solver_fdtd_openems", "prepare_openems_patch", "run_prepared_openems")}


@pytest.mark.parametrize("variant,design,kw", OPTIONS, ids=OPTION_IDS)
def test_plugin_options_equal_the_reference(oracle_lib, tmp_path, variant, design, kw):
    """Feed directions, feed-line length, boundary, mesh quality, angular steps, explicit patch dimensions, other substrates: the option
    handling of every mirrored prepare function against the reference's (recorded), through the run, to the dBi grid."""
    import contextlib
    import io
    s = pkg("solver_fdtd_hip")
    own_prep = {"fixed": s.prepare_hip_patch_fixed, "microstrip": s.prepare_hip_microstrip_patch,
                "microstrip_3d": s.prepare_hip_microstrip_patch_3d, "legacy": s.prepare_hip_patch}[variant]
    kw_own = dict(kw)
    if "feed_direction" in kw:
        kw_own["feed_direction"] = getattr(s.FeedDirection, kw["feed_direction"])
    with contextlib.redirect_stdout(io.StringIO()):
        po = own_prep(_params(**design), work_dir=str(tmp_path / "o"), lib=oracle_lib, **kw_own)
        assert po.ok, po.message
        po.FDTD.NrTS = 1500
        ro = s.run_prepared_hip(po, frequency_hz=design["frequency_ghz"] * 1e9, verbose=0)
    _same_as_recorded("option/" + OPTION_IDS[[o[0] for o in OPTIONS].index(variant)], po, ro)


def test_the_references_own_test_script_runs(oracle_lib, tmp_path):
    """The reference's test_openems.py — the openEMS tutorial patch, its one test of its engine ("SUCCESS" when Run() returns) — ran as it
    is over the shims on the oracle (recorded: mesh, timesteps to its end criterion, end energy).  The same scene through this package's
    mirror (tests/tutorial_scene.py, NrTS 60 000, EndCriteria 1e-5) ends on the same mesh, at the same timestep, at the same energy."""
    import tutorial_scene
    g = _gold("tutorial")
    r = tutorial_scene.build_and_run(oracle_lib, str(tmp_path / "run"), nr_ts=60000, end_criteria=1e-5)
    assert list(r["grid"]) == g["grid"].tolist()
    assert r["steps"] < 60000 and r["energy_db"] < -50.0
    assert r["steps"] == int(g["steps_energy_db"][0]) and abs(r["energy_db"] - g["steps_energy_db"][1]) < 1e-6


MODEL_FIELDS = ("frequency_hz", "eps_r", "h_m", "loss_tangent", "patch_length_m", "patch_width_m")


def random_designs():
    """300 seeded random designs: (f, eps_r, h, keyword arguments of the input model)."""
    rng = np.random.default_rng(5)
    out = []
    for _ in range(300):
        f = float(rng.uniform(0.5e9, 30e9)); er = float(rng.uniform(1.5, 12.0)); h = float(rng.uniform(0.1e-3, 4e-3))
        kw = dict(frequency_ghz=f / 1e9, er=er, h_mm=h * 1e3, loss_tangent=float(rng.uniform(0, 0.05)))
        if rng.random() < 0.3:
            kw.update(L_mm=float(rng.uniform(2, 80)), W_mm=float(rng.uniform(2, 80)))
        out.append((f, er, h, kw))
    return out


def test_closed_form_design_equals_the_reference_over_random_inputs():
    """design_patch_for_frequency / calculate_microstrip_width (physics.py:19-48, solver_fdtd_openems_microstrip.py:84-112) and the input model's
    unit conversion against the reference's values (recorded), over 300 random designs (the committed design_values.json holds a handful);
    where the reference's model refused an input, ours must refuse too; a field it left unset (recorded as NaN) is unset here too."""
    own, own_params = pkg("patch_design"), pkg("params")
    g = _gold("design")
    for n, (f, er, h, kw) in enumerate(random_designs()):
        assert np.allclose(g["patch"][n], own.design_patch_for_frequency(f, er, h), rtol=1e-12, atol=0)
        assert abs(g["feed_width"][n] - own.calculate_microstrip_width(f, er, h)) <= 1e-12 * h
        if g["refused"][n]:
            with pytest.raises(Exception):
                own_params.PatchAntennaParams.from_user_units(**kw)
            continue
        o = own_params.PatchAntennaParams.from_user_units(**kw)
        for name, r in zip(MODEL_FIELDS, g["model"][n]):
            if np.isnan(r):
                assert getattr(o, name) is None, name
                continue
            assert r == getattr(o, name) or np.isclose(r, getattr(o, name), rtol=1e-15, atol=0), name


@needs_reference
def test_patch_instance_fields_and_defaults_are_the_references():
    """`multi_patch_designer.PatchInstance` (`:18-28`) cannot be imported here (the module pulls in Tk and matplotlib); its dataclass is read
    from the source text: same field names, same order, same defaults (positions default to 0.0: `PatchInstance("A", params)` must work)."""
    import ast
    import dataclasses
    tree = ast.parse(open(os.path.join(REF, "antenna_sim", "multi_patch_designer.py")).read())
    cls = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == "PatchInstance")
    ref_fields = [(st.target.id, None if st.value is None else ast.unparse(st.value)) for st in cls.body if isinstance(st, ast.AnnAssign)]
    own = dataclasses.fields(pkg("solver_fdtd_hip").PatchInstance)
    assert [f.name for f in own] == [n for n, _ in ref_fields]
    for f, (name, default) in zip(own, ref_fields):
        if default is None:
            assert f.default is dataclasses.MISSING, name
        elif default.startswith("FeedDirection."):
            assert f.default.name == default.split(".")[1], name
        else:
            assert f.default == float(default), name


@needs_reference
def test_probe_prepared_result_types_hold_every_field_of_the_references(monkeypatch):
    """OpenEMSProbe / OpenEMSPrepared / OpenEMSResult of every solver file: each field exists, with the same default, on FDTDProbe / FDTDPrepared /
    FDTDResult (which add fields: port, ports, variant, freq, s11, ...; never rename or drop one)."""
    import dataclasses
    import importlib
    compat = os.path.join(ROOT, "fdtd-solver-antennas_amd", "compat")
    monkeypatch.syspath_prepend(REF)
    monkeypatch.syspath_prepend(compat)
    monkeypatch.setattr(sys, "dont_write_bytecode", True)
    if not hasattr(os, "add_dll_directory"):
        monkeypatch.setattr(os, "add_dll_directory", lambda p: None, raising=False)
    for m in [k for k in sys.modules if k.split(".")[0] in ("openEMS", "CSXCAD", "antenna_sim")]:
        monkeypatch.delitem(sys.modules, m)
    s = pkg("solver_fdtd_hip")
    seen = 0
    for module in ("solver_fdtd_openems_fixed", "solver_fdtd_openems_microstrip", "solver_fdtd_openems_microstrip_3d",
                   "solver_fdtd_openems_microstrip_multi_3d", "solver_fdtd_openems"):
        ref = importlib.import_module("antenna_sim." + module)
        for ref_name, own in (("OpenEMSProbe", s.FDTDProbe), ("OpenEMSPrepared", s.FDTDPrepared), ("OpenEMSResult", s.FDTDResult)):
            rc = getattr(ref, ref_name, None)
            if rc is None or not dataclasses.is_dataclass(rc):
                continue
            own_fields = {f.name: f for f in dataclasses.fields(own)}
            for f in dataclasses.fields(rc):
                assert f.name in own_fields, f"{own.__name__} lacks {f.name!r} of {module}.{ref_name}"
                if f.default is not dataclasses.MISSING:
                    assert own_fields[f.name].default == f.default, (module, ref_name, f.name)
                seen += 1
    assert seen > 40


@needs_reference
def test_result_feeds_the_references_plotting(oracle_lib, tmp_path, monkeypatch):
    """The sink side of the path (north_star: "same S11/far-field results out to plotting.py"): θ, φ [rad] and the dBi grid of run_prepared_hip go
    into the reference's own `plotting.plot_3d_pattern_from_grid` / `plotting_new.plot_3d_pattern_from_grid` (Agg backend) and come out as figures."""
    pytest.importorskip("matplotlib")
    import importlib
    monkeypatch.setenv("MPLBACKEND", "Agg")
    compat = os.path.join(ROOT, "fdtd-solver-antennas_amd", "compat")
    monkeypatch.syspath_prepend(REF)
    monkeypatch.syspath_prepend(compat)
    monkeypatch.setattr(sys, "dont_write_bytecode", True)
    if not hasattr(os, "add_dll_directory"):
        monkeypatch.setattr(os, "add_dll_directory", lambda p: None, raising=False)
    for m in [k for k in sys.modules if k.split(".")[0] in ("openEMS", "CSXCAD", "antenna_sim")]:
        monkeypatch.delitem(sys.modules, m)
    import matplotlib
    matplotlib.use("Agg", force=True)
    s = pkg("solver_fdtd_hip")
    p = pkg("params").PatchAntennaParams.from_user_units(frequency_ghz=2.45, er=4.3, h_mm=1.6, loss_tangent=0.02)
    prep = s.prepare_hip_microstrip_patch_3d(p, work_dir=str(tmp_path / "o"), lib=oracle_lib, mesh_quality=1, phi_step_deg=15.0)
    prep.FDTD.NrTS = 2000
    res = s.run_prepared_hip(prep, frequency_hz=2.45e9, verbose=0)
    assert res.ok, res.message
    from matplotlib.figure import Figure
    old = importlib.import_module("antenna_sim.plotting")
    fig = old.plot_3d_pattern_from_grid(res.theta, res.phi, 10.0 ** (np.asarray(res.intensity) / 10.0), colors_db=res.intensity)
    assert isinstance(fig, Figure) and fig.axes
    new = importlib.import_module("antenna_sim.plotting_new")
    fig2 = new.plot_3d_pattern_from_grid(res.theta, res.phi, res.intensity)
    assert isinstance(fig2, Figure) and fig2.axes
    import matplotlib.pyplot as plt
    plt.close("all")


@needs_reference
def test_the_unexported_quasi_2d_variant_runs_on_the_shims_too(oracle_lib, tmp_path, monkeypatch):
    """`solver_fdtd_openems_2d.prepare_openems_patch_2d` (out of scope, no mirrored function here) is still reachable from the
    reference's Streamlit page, which runs it through the legacy `run_prepared_openems`: over the shims that works as it is."""
    import importlib
    compat = os.path.join(ROOT, "fdtd-solver-antennas_amd", "compat")
    monkeypatch.syspath_prepend(REF)
    monkeypatch.syspath_prepend(compat)
    monkeypatch.setattr(sys, "dont_write_bytecode", True)
    if not hasattr(os, "add_dll_directory"):
        monkeypatch.setattr(os, "add_dll_directory", lambda p: None, raising=False)
    for m in [k for k in sys.modules if k.split(".")[0] in ("openEMS", "CSXCAD", "antenna_sim")]:
        monkeypatch.delitem(sys.modules, m)
    dll = tmp_path / "dll"
    dll.mkdir()
    (dll / "openEMS.dll").write_text("")
    from antenna_sim.models import PatchAntennaParams
    two_d = importlib.import_module("antenna_sim.solver_fdtd_openems_2d")
    legacy = importlib.import_module("antenna_sim.solver_fdtd_openems")
    p = PatchAntennaParams.from_user_units(frequency_ghz=2.45, er=4.3, h_mm=1.6, loss_tangent=0.02)
    prep = two_d.prepare_openems_patch_2d(p, dll_dir=str(dll), work_dir=str(tmp_path / "run"), cleanup=True, verbose=0)
    assert prep.ok, prep.message
    prep.FDTD.NrTS = 2000
    prep.FDTD._lib = oracle_lib
    res = legacy.run_prepared_openems(prep, frequency_hz=2.45e9, verbose=0)
    assert res.ok, res.message
    assert np.isfinite(np.asarray(res.intensity)).all()
