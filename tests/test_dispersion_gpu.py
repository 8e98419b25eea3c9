"""Debye media on the GPU (csrc/dispersion.hip, include/fdtd_hip_dispersion.h): the HIP step loop against the oracle's half-steps
plus the numpy restatement of the correction (dispersion.correction), bit for bit — fields, branch states u_k and v_prev; fdtd_run
against half-steps; the refusals; the schedules; and the plugin's substrate_dispersion option."""
import numpy as np
import pytest

from conftest import pkg
from helpers import patch_sim
from test_dispersion_model_cpu import Restated, _fr4, _graded, _grid, restating_build


def _media_scene(g, boxes, port=None, sheets=(), plain=()):
    """boxes: (name, medium, lo, hi) in node indices of g."""
    sc = pkg("scene")
    x, y, z = (l * 1e3 for l in g.lines)
    at = lambda p: [x[p[0]], y[p[1]], z[p[2]]]
    s = sc.Scene(unit=1e-3)
    for name, eps, lo, hi in plain:
        s.add_material(name, eps_r=eps).add_box(at(lo), at(hi))
    for name, m, lo, hi in boxes:
        s.add_debye_material(name, m.eps_inf, m.kappa, m.delta_eps, m.tau).add_box(at(lo), at(hi), priority=1)
    for name, sigma, t, lo, hi in sheets:
        s.add_conducting_sheet(name, sigma, t).add_box(at(lo), at(hi))
    if port is not None:
        s.add_lumped_port(1, port[0], at(port[1]), at(port[2]), "z", 1.0)
    return sc.voxelize(s, g)


def _sim(name, nr_ts):
    d, sim = pkg("dispersion"), pkg("simulation")
    hi_band = _fr4(9e9, 5e9, 15e9)                    # K = 3
    one = d.DebyeMedium(2.5, 0.02, [0.8], [2e-11])    # K = 1, with a conductivity of its own
    wide = d.fit_constant_loss_tangent(4.3, 0.02, 9e9, 0.1e9, 30e9, K=8)
    kw = dict(f0=9e9, fc=5e9, nr_ts=nr_ts, end_criteria=0.0)
    if name in ("pec-uniform", "pec-uniform-raw"):
        # nx = 14 (rows padded to 16); the medium's x-edges run 3 .. 8: odd start, odd end, partial groups of four at both ends
        g = _grid((14, 13, 12))
        v = _media_scene(g, [("m", hi_band, (3, 2, 2), (9, 10, 9))], port=(50.0, (6, 5, 3), (6, 5, 7)))
        return sim.Simulation(g, v, boundary="PEC", use_classes=name == "pec-uniform", **kw)
    if name == "pec-graded-k8":
        g = _graded((17, 13, 14))
        v = _media_scene(g, [("m", wide, (1, 1, 1), (15, 11, 12))], port=(50.0, (7, 5, 4), (7, 5, 8)))
        return sim.Simulation(g, v, boundary="PEC", **kw)
    if name == "mur-graded":
        g = _graded((23, 21, 19))
        v = _media_scene(g, [("m", hi_band, (5, 4, 4), (17, 16, 13))], port=(50.0, (11, 10, 5), (11, 10, 9)))
        return sim.Simulation(g, v, boundary="MUR", **kw)
    if name == "cpml8-graded":
        g = _graded((29, 27, 26))
        v = _media_scene(g, [("m", hi_band, (9, 9, 9), (19, 17, 16))], port=(50.0, (13, 12, 10), (13, 12, 14)))
        return sim.Simulation(g, v, boundary="CPML", cpml_cells=8, **kw)
    if name == "two-media-mur":
        # two different media a cell apart (K = 3 and K = 1: the shorter one padded), a plain dielectric between and around them
        g = _graded((26, 19, 17))
        v = _media_scene(g, [("a", hi_band, (4, 4, 4), (11, 14, 12)), ("b", one, (12, 3, 5), (21, 15, 11))],
                         port=(50.0, (7, 8, 5), (7, 8, 9)), plain=[("p", 2.2, (3, 3, 3), (22, 16, 13))])
        return sim.Simulation(g, v, boundary="MUR", **kw)
    if name == "media-and-sheets-mur":
        # a substrate between a resolved copper slab and a zero-thickness tin sheet: sheet edges ARE dispersive edges there
        g = _grid((26, 24, 22))
        v = _media_scene(g, [("sub", hi_band, (6, 6, 8), (19, 17, 12))], port=(50.0, (12, 11, 8), (12, 11, 12)),
                         sheets=[("cu", 5.8e7, 2e-3, (7, 7, 6), (18, 16, 8)), ("tin", 9.1e6, 5e-6, (9, 8, 12), (16, 15, 12))])
        return sim.Simulation(g, v, boundary="MUR", **kw)
    raise KeyError(name)


CASES = ["pec-uniform", "pec-uniform-raw", "pec-graded-k8", "mur-graded", "cpml8-graded", "two-media-mur", "media-and-sheets-mur"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_matches_restatement_bit_for_bit(hip_lib, oracle_lib, name):
    nsteps = 300
    ref_sim = _sim(name, nsteps)
    ref = Restated(ref_sim, oracle_lib)
    ref.run(nsteps)
    s = _sim(name, nsteps)
    e = s.build(hip_lib)
    assert (e.operator_form()[0] == "raw") == (name == "pec-uniform-raw"), e.operator_form()
    info = e.schedule_info()
    mur = "mur" in name
    assert not info["resident"] and info["launches_per_timestep"] in ((2, 3) if mur else (2,)), info
    e.run(nsteps)
    assert np.abs(ref.e.fields()).max() > 0
    assert np.array_equal(e.fields(), ref.e.fields())
    nonzero = 0
    for c in range(3):
        hv, hu, hvi = e.debye_state(c)
        assert np.array_equal(hvi, ref.vi[c])                      # the vi the library took from its own operator
        assert np.array_equal(hv, ref.vprev[c]) and np.array_equal(hu, ref.u[c])
        off = ref.w[c] == 0
        assert np.all(hv[off] == 0) and np.all(hu[:, off] == 0)    # edges of the box outside the medium are left alone
        nonzero += np.count_nonzero(hu)
    assert nonzero > 0
    for (pu, pi), (qu, qi) in zip(s.port_series(), [(ref.e.get_probe(u), ref.e.get_probe(i)) for u, i in ref_sim._port_probe_ids]):
        assert np.abs(qu).max() > 0 and np.array_equal(pu, qu) and np.array_equal(pi, qi)
    if name == "media-and-sheets-mur":
        hv, hib = e.sheet_state()
        assert np.abs(hib).max() > 0 and np.array_equal(hv, ref.sheet["vprev"]) and np.array_equal(hib, ref.sheet["ib"])
        on = [np.count_nonzero(ref.w[c].reshape(-1)) for c in range(3)]
        assert min(on) > 0
    if name == "pec-uniform":
        assert s.debye.lo[0][0] == 3 and s.debye.hi[0][0] == 9 and s.grid.shape[0] % 4 != 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mur-graded", "media-and-sheets-mur"])
def test_run_equals_half_steps(hip_lib, name):
    n = 200
    a, b = _sim(name, n), _sim(name, n)
    ea, eb = a.build(hip_lib), b.build(hip_lib)
    ea.run(n)
    for _ in range(n):
        eb.half_step(0)
        eb.half_step(1)
    assert np.abs(ea.fields()).max() > 0 and np.array_equal(ea.fields(), eb.fields())
    for c in range(3):
        for x, y in zip(ea.debye_state(c), eb.debye_state(c)):
            assert np.array_equal(x, y)
    # fdtd_set_field does not touch the states
    before = [ea.debye_state(c) for c in range(3)]
    for c in range(3):
        ea.set_field(0, c, np.zeros(ea.local_shape, np.float32))
    for c in range(3):
        for x, y in zip(before[c], ea.debye_state(c)):
            assert np.array_equal(x, y)


@pytest.mark.gpu
def test_refusals(hip_lib, oracle_lib):
    capi = pkg("_capi")
    s = _sim("pec-uniform", 50)
    tabs = s.debye_tables()
    # forced one-launch / resident schedules: FDTD_E_UNSUPPORTED (-5), by message
    for flag in (capi.FLAG_KERNEL_WAVEFRONT, capi.FLAG_KERNEL_RESIDENT):
        e = s.build(hip_lib, flags=flag)
        with pytest.raises(capi.FdtdError, match=r"\(-5\): Debye media: the two-launch schedule only"):
            e.run(1)
        e.close()
    # after the first timestep: FDTD_E_STATE (-2)
    e = s.build(hip_lib)
    e.run(1)
    with pytest.raises(capi.FdtdError, match=r"\(-2\): fdtd_debye_set: before the first timestep"):
        e.set_debye(*tabs)
    e.close()
    # before the operator: FDTD_E_STATE
    nx, ny, nz = s.grid.shape
    e = capi.Engine(hip_lib, nx, ny, nz, s.dt)
    with pytest.raises(capi.FdtdError, match=r"\(-2\): fdtd_debye_set: set the operator first"):
        e.set_debye(*tabs)
    e.close()
    # decomposed contexts: refused by the library (-5) and by Simulation.build
    e = capi.Engine(hip_lib, nx, ny, nz, s.dt, k0=0, nk=6, rank=0, world=2)
    with pytest.raises(capi.FdtdError, match=r"\(-5\): Debye media: single slab only"):
        e.set_debye(*tabs)
    e.close()
    with pytest.raises(capi.FdtdError, match="single slab"):
        s.build(hip_lib, world=2, rank=0)
    # bad arguments: (-1)
    e = s.build(hip_lib)
    alpha, oma, beta, lo, hi, w, med = tabs
    with pytest.raises(capi.FdtdError, match=r"\(-1\): fdtd_debye_set: component 0: box \[3, 14\) along axis 0 leaves the grid's edges"):
        e.set_debye(alpha, oma, beta, lo, [(14, hi[0][1], hi[0][2]), hi[1], hi[2]],
                    [np.zeros((hi[0][2] - lo[0][2], hi[0][1] - lo[0][1], 11), np.float32), w[1], w[2]])
    with pytest.raises(capi.FdtdError, match=r"\(-1\): fdtd_debye_set: at most 8 media"):
        e.set_debye(np.ones((9, 1)), np.zeros((9, 1)), np.zeros((9, 1)), lo, hi, w, [np.zeros(x.shape, np.uint8) for x in w])
    with pytest.raises(capi.FdtdError, match=r"\(-1\): fdtd_debye_set: component 0: medium id 2 out of range"):
        e.set_debye(np.ones((2, 1)), np.zeros((2, 1)), np.zeros((2, 1)), lo, hi, w,
                    [np.full(w[0].shape, 2, np.uint8)] + [np.zeros(x.shape, np.uint8) for x in w[1:]])
    e.run(2)      # (the refused calls left the context steppable)
    e.close()
    # the oracle has no such entry points
    e = capi.Engine(oracle_lib, 8, 8, 8, 1e-12)
    with pytest.raises(capi.FdtdError, match="no Debye media"):
        e.debye_state(0)
    e.close()
    assert capi.has_dispersion(hip_lib) and not capi.has_dispersion(oracle_lib)


@pytest.mark.gpu
def test_schedules_without_and_with_media(hip_lib):
    """A context without media takes the schedule it took before Debye media existed — the three the suite pins (test_round3_gpu,
    test_resident_gpu): resident, one launch per timestep, two launches — and one with media two launches (three with Mur's apply
    pass where the planner needs it)."""
    info = patch_sim(64, 60, 36, nr_ts=10).build(hip_lib).schedule_info()
    assert info["resident"] and info["launches_per_timestep"] == 1 and info["lag_planes"] == -1
    big = patch_sim(300, 300, 60, boundary="MUR", nr_ts=10, nf2ff=False).build(hip_lib)
    assert not big.schedule_info()["resident"] and big.schedule_info()["launches_per_timestep"] == 1
    big.close()
    mid = patch_sim(150, 140, 36, boundary="MUR", nr_ts=10, nf2ff=False).build(hip_lib)
    assert not mid.schedule_info()["resident"] and mid.schedule_info()["launches_per_timestep"] == 2
    for name, want in (("pec-uniform", (2,)), ("cpml8-graded", (2,)), ("mur-graded", (2, 3))):
        info = _sim(name, 10).build(hip_lib).schedule_info()
        assert not info["resident"] and info["launches_per_timestep"] in want and info["lag_planes"] == 0, (name, info)
    # removing the media gives the plain context's schedule back
    s = _sim("cpml8-graded", 10)
    e = s.build(hip_lib)
    plain = dict(e.schedule_info())
    e.set_debye(np.zeros((0, 1)), np.zeros((0, 1)), np.zeros((0, 1)), [(0, 0, 0)] * 3, [(0, 0, 0)] * 3, [None] * 3)
    saved, s.debye = s.debye, None
    try:
        want = s.build(hip_lib).schedule_info()
    finally:
        s.debye = saved
    assert e.schedule_info() == want and not plain["resident"] and plain["launches_per_timestep"] == 2


def _plugin_pair(prepare, hip_lib, oracle_lib, tmp_path, monkeypatch, nsteps, f):
    s = pkg("solver_fdtd_hip")
    restating_build(monkeypatch)
    out = []
    for lib, tag in ((hip_lib, "gpu"), (oracle_lib, "cpu")):
        prep = prepare(lib, str(tmp_path / tag))
        assert prep.ok, prep.message
        prep.FDTD.NrTS = nsteps
        r = s.run_prepared_hip(prep, frequency_hz=f, verbose=0)
        assert r.ok, r.message
        out.append((r, prep.FDTD.sim.port_series(), s.s11_from_port(prep.port, prep.sim_path, f)[1], prep.FDTD.sim))
    (g, sg, s11g, simg), (c, sc_, s11c, simc) = out
    assert hasattr(simc, "restated") and not hasattr(simg, "restated")
    assert g.stats["grid"] == c.stats["grid"] and g.stats["steps"] == c.stats["steps"] == nsteps
    for (ug, ig), (uc, ic) in zip(sg, sc_):
        assert np.abs(uc).max() > 0 and np.array_equal(ug, uc) and np.array_equal(ig, ic)
    assert np.linalg.norm(s11g - s11c) <= 1e-3 * np.linalg.norm(s11c)
    assert np.linalg.norm(g.intensity - c.intensity) <= 1e-3 * np.linalg.norm(c.intensity)
    dsp = g.stats["dispersion"]
    assert dsp["K"] == 3 and dsp["edges"] > 0 and dsp["poles"] == 3 * len(dsp["media"]) and dsp["fit_errors"]["tan_delta"] <= 0.02
    assert g.stats["schedule"]["launches_per_timestep"] in (2, 3) and not g.stats["schedule"]["resident"]
    return g, dsp


@pytest.mark.gpu
def test_plugin_microstrip_3d_with_dispersion_equals_checker(hip_lib, oracle_lib, tmp_path, monkeypatch):
    s, P = pkg("solver_fdtd_hip"), pkg("params").PatchAntennaParams
    p = P.from_user_units(frequency_ghz=5.8, er=4.3, h_mm=1.6, loss_tangent=0.02)
    g, dsp = _plugin_pair(lambda lib, wd: s.prepare_hip_microstrip_patch_3d(p, work_dir=wd, lib=lib, mesh_quality=1, substrate_dispersion=True),
                          hip_lib, oracle_lib, tmp_path, monkeypatch, 500, 5.8e9)
    assert len(dsp["media"]) == 1 and dsp["media"][0]["names"] == ["substrate"]
    assert abs(dsp["media"][0]["fit"]["tan_delta"] - 0.02) < 1e-15


@pytest.mark.gpu
def test_plugin_multi_patch_with_dispersion_and_metal_loss_equals_checker(hip_lib, oracle_lib, tmp_path, monkeypatch):
    """2 x 2 patches: substrate_0..3 are one medium (identical parameters merge); with copper sheets on top of it."""
    s, P = pkg("solver_fdtd_hip"), pkg("params").PatchAntennaParams
    p = P.from_user_units(frequency_ghz=5.8, er=4.3, h_mm=1.6, loss_tangent=0.02, metal="copper")
    pitch = 0.03
    inst = [s.PatchInstance(name=f"P{n}", params=p, center_x_m=(ix - 0.5) * pitch, center_y_m=(iy - 0.5) * pitch, center_z_m=0.0,
                            feed_direction=s.FeedDirection.NEG_X) for n, (ix, iy) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)])]
    g, dsp = _plugin_pair(lambda lib, wd: s.prepare_hip_microstrip_multi_3d(inst, boundary="MUR", mesh_quality=1, work_dir=wd, lib=lib,
                                                                           substrate_dispersion=True, metal_loss=True),
                          hip_lib, oracle_lib, tmp_path, monkeypatch, 300, 5.8e9)
    names = dsp["media"][0]["names"]
    assert len(dsp["media"]) == 1 and len(names) == 4 and all(n.startswith("substrate_") for n in names), dsp["media"]
    assert g.stats["sheet_edges"] > 0


@pytest.mark.gpu
def test_efficiency_lower_with_dispersion_above_f0(hip_lib, tmp_path):
    """The microstrip scene designed for 2.45 GHz resonates well above it (profiles: 2.9 GHz).  There the plain kappa material has
    tan delta * f0 / f_res, the Debye substrate the tan delta the user typed: its radiation efficiency at f_res must be lower."""
    s, P = pkg("solver_fdtd_hip"), pkg("params").PatchAntennaParams
    p = P.from_user_units(frequency_ghz=2.45, er=4.3, h_mm=1.6, loss_tangent=0.02)
    runs = {}
    for on in (False, True):
        prep = s.prepare_hip_microstrip_patch_3d(p, work_dir=str(tmp_path / str(on)), lib=hip_lib, mesh_quality=2, substrate_dispersion=on)
        assert prep.ok, prep.message
        prep.FDTD.EndCriteria = 1e-5
        prep.FDTD.NrTS = 120000
        res = s.run_prepared_hip(prep, frequency_hz=2.45e9, verbose=0)
        assert res.ok, res.message
        assert res.stats["energy_db"] < -50.0, res.stats
        assert ("dispersion" in res.stats) == on
        runs[on] = (prep, res)
    res0 = runs[False][1]
    fr = float(res0.freq[int(np.argmin(res0.s11_dB))])
    assert fr > 1.05 * 2.45e9, fr
    eta = {}
    for on, (prep, res) in runs.items():
        nfr = prep.nf.CalcNF2FF(prep.sim_path, [fr], np.arange(0.0, 181.0, 6.0), np.arange(0.0, 360.0, 12.0), center=[0, 0, 0])
        eta[on] = float(np.asarray(nfr.Prad)[0]) / float(prep.port.CalcPort(prep.sim_path, np.array([fr])).P_acc[0])
    print(f"microstrip 3-D, FR-4 tan delta 0.02, resonance {fr / 1e9:.3f} GHz: radiation efficiency kappa model {eta[False]:.4f}, "
          f"Debye substrate {eta[True]:.4f}")
    assert 0 < eta[True] < eta[False] < 1.05, eta
