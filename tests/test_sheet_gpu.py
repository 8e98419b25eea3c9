"""Conducting sheets on the GPU (csrc/sheet.hip): the HIP step loop against the oracle's half-steps plus the numpy restatement of the
correction (sheet.correction), bit for bit; the schedules a context with sheets may take; the Q of a lossy cavity against Pozar's
closed form; and the plugin's efficiency / gain fields."""
import os

import numpy as np
import pytest

from conftest import pkg
from restatement import Restatement
from test_sheet_model_cpu import MU0, _grid, cavity_sim


def _resolved_sim(boundary, nr_ts):
    """A resolved (two-cell) copper slab and a zero-thickness tin sheet in one scene, a port between them."""
    sc, sim = pkg("scene"), pkg("simulation")
    g = _grid((26, 24, 22))
    s = sc.Scene(unit=1e-3)
    s.add_material("sub", eps_r=3.0).add_box([6, 6, 8], [19, 17, 12])
    s.add_conducting_sheet("cu", 5.8e7, 2e-3).add_box([7, 7, 6], [18, 16, 8])
    s.add_conducting_sheet("tin", 9.1e6, 5e-6).add_box([9, 8, 12], [16, 15, 12])
    s.add_lumped_port(1, 50.0, [12, 11, 8], [12, 11, 12], "z", 1.0)
    return sim.Simulation(g, sc.voxelize(s, g), f0=6e9, fc=4e9, boundary=boundary, cpml_cells=4, nr_ts=nr_ts, end_criteria=0.0)


CASES = [("pec-zero-thickness", lambda n: cavity_sim(3e5, 1e-3, nr_ts=n), True),
         ("pec-zero-thickness-raw", lambda n: cavity_sim(3e5, 1e-3, nr_ts=n), False),
         ("cpml-resolved", lambda n: _resolved_sim("CPML", n), True),
         ("mur-resolved", lambda n: _resolved_sim("MUR", n), True),
         ("mur-resolved-raw", lambda n: _resolved_sim("MUR", n), False)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,make,classes", CASES, ids=[c[0] for c in CASES])
def test_hip_matches_restatement_bit_for_bit(hip_lib, oracle_lib, name, make, classes):
    nsteps = 400
    ref_sim = make(nsteps)
    ref_sim.use_classes = classes
    r = Restatement(ref_sim, oracle_lib)
    r.run(nsteps)
    ref, vprev, ib = r.e, r.sheets.vprev, r.sheets.ib
    s = make(nsteps)
    s.use_classes = classes
    e = s.build(hip_lib)
    assert e.operator_form()[0].startswith("classes") == classes, e.operator_form()
    # the vi the host hands fdtd_sheet_set is the device operator's own
    assert np.array_equal(s.sheet_vi(), e.get_operator()[1].reshape(3, -1)[s.sheets.comp.astype(np.int64), s.sheets.idx])
    info = e.schedule_info()
    assert not info["resident"] and info["launches_per_timestep"] in (2, 3), info
    e.run(nsteps)
    assert np.abs(ref.fields()).max() > 0 and np.abs(vprev).max() > 0
    assert np.array_equal(e.fields(), ref.fields())
    hv, hib = e.sheet_state()
    assert np.array_equal(hv, vprev) and np.array_equal(hib, ib)
    for (pu, pi), (qu, qi) in zip(s.port_series(), [(ref.get_probe(u), ref.get_probe(i)) for u, i in ref_sim._port_probe_ids]):
        assert np.array_equal(pu, qu) and np.array_equal(pi, qi)


def _raw_sheet_tables(e, edges):
    """(idx, comp, vi, cls, alpha, b) of fdtd_sheet_set for hand-picked edges [(comp, i, j, k)]: two poles, one class, vi the operator's."""
    nz, ny, nx = e.local_shape
    vi_all = e.get_operator()[1]
    idx = np.array([(k * ny + j) * nx + i for _, i, j, k in edges], np.int64)
    comp = np.array([c for c, _, _, _ in edges], np.int8)
    vi = np.array([vi_all[c][k, j, i] for c, i, j, k in edges], np.float32)
    return idx, comp, vi, np.zeros(idx.size, np.int32), np.array([[0.9, 0.5]], np.float32), np.array([[2e-5, 1e-4]], np.float32)


def _restated_with_raw_sheets(sim, lib, tables, seed):
    return Restatement(sim, lib, seed=seed, tables={"sheets": tables})


@pytest.mark.gpu
def test_v_probe_on_a_sheet_edge_is_sampled_before_the_correction(hip_lib, oracle_lib):
    """fdtd_hip_sheet.h: the correction follows the V-probes.  The scene layer keeps sheet edges off probe lines; the C ABI states no
    such restriction, so a probe added there must read the voltage BEFORE k_sheet changed it, under fdtd_run as under fdtd_half_step
    and in the restatement (with fused sources fdtd_run used to sample it in update_H's probe block, after the correction)."""
    from helpers import seeded_fields
    capi = pkg("_capi")
    nsteps = 150
    sims = [cavity_sim(3e5, 1e-3, nr_ts=nsteps) for _ in range(3)]
    sh = sims[0].sheets
    on = [int(q) for q in np.nonzero(sims[0].sheet_vi() != 0)[0][[3, 40, 77]]]                  # three sheet edges, live ones
    idx, comp, w = sh.idx[on], sh.comp[on], np.array([1.0, -0.5, 2.0], np.float32)
    ref = Restatement(sims[0], oracle_lib, seed=4)
    e_run, e_half = sims[1].build(hip_lib), sims[2].build(hip_lib)
    pids = [e.add_probe(capi.KIND_V, idx, comp, w) for e in (ref, e_run, e_half)]
    for e in (e_run, e_half):
        seeded_fields(e, 4)
    ref.run(nsteps)
    e_run.run(70)
    e_run.run(80)
    for _ in range(nsteps):
        e_half.half_step(0)
        e_half.half_step(1)
    want = ref.get_probe(pids[0])[:nsteps]
    assert np.abs(want).max() > 0 and np.abs(ref.sheets.ib).max() > 0
    # (the correction does change what the probe would read: sampled after it, the series differs)
    after = sum(float(wq) * float(ref.V[c].reshape(-1)[g]) for wq, c, g in zip(w, comp, idx))
    assert after != want[-1]
    assert np.array_equal(e_half.get_probe(pids[2])[:nsteps], want)
    assert np.array_equal(e_run.get_probe(pids[1])[:nsteps], want)
    assert np.array_equal(e_run.fields(), ref.e.fields()) and np.array_equal(e_run.sheet_state()[1], ref.sheets.ib)
    for (pu, pi), (qu, qi) in zip(sims[1].port_series(), [(ref.get_probe(u), ref.get_probe(i)) for u, i in sims[0]._port_probe_ids]):
        assert np.array_equal(pu, qu) and np.array_equal(pi, qi)


@pytest.mark.gpu
def test_sheet_edges_on_a_mur_face_node_plane(hip_lib, oracle_lib, monkeypatch):
    """The scene layer keeps sheets two planes inside Mur faces; fdtd_sheet_set takes any edge.  Edges on the node plane of a Mur face
    (the operator holds them: vi = 0, so only their states can tell) and live ones inside: k_sheet must read the face's FINAL voltage, so
    such a context takes the apply pass as a launch of its own — fields and states equal the restatement with the environment asking
    for either schedule."""
    from helpers import seeded_fields
    nsteps = 120
    edges = [(1, 0, j, k) for j in range(3, 9) for k in range(3, 9)] + [(2, 5, 0, k) for k in range(3, 8)] + \
            [(1, 6, j, k) for j in range(3, 9) for k in range(4, 7)] + [(0, i, 5, 5) for i in range(3, 9)]
    mk = lambda: cavity_sim(1.0, 1.0, sheet=False, boundary="MUR", nr_ts=nsteps)
    ref_sim = mk()
    probe = Restatement(ref_sim, oracle_lib)
    tables = _raw_sheet_tables(probe.e, edges)
    assert np.count_nonzero(tables[2] == 0) == 36 + 5 and np.count_nonzero(tables[2]) == 18 + 6
    ref = _restated_with_raw_sheets(mk(), oracle_lib, tables, seed=6)
    ref.run(nsteps)
    assert np.all(np.abs(ref.sheets.ib).max(axis=0) > 0)
    for apply_pass in (None, "1"):
        if apply_pass is None:
            monkeypatch.delenv("FDTD_MUR_APPLY_PASS", raising=False)
        else:
            monkeypatch.setenv("FDTD_MUR_APPLY_PASS", apply_pass)
        s = mk()
        e = s.build(hip_lib)
        e.set_sheets(*[t[41:] if q < 4 else t for q, t in enumerate(tables)])      # the live edges alone: the environment decides
        assert e.schedule_info()["launches_per_timestep"] == (2 if apply_pass is None else 3)
        e.set_sheets(*tables)
        info = e.schedule_info()
        assert info["launches_per_timestep"] == 3 and not info["resident"], info
        seeded_fields(e, 6)
        e.run(nsteps)
        assert np.array_equal(e.fields(), ref.e.fields())
        hv, hib = e.sheet_state()
        assert np.array_equal(hv, ref.sheets.vprev) and np.array_equal(hib, ref.sheets.ib)
        e.close()


@pytest.mark.gpu
def test_schedules_with_sheets(hip_lib, oracle_lib):
    capi = pkg("_capi")
    s = cavity_sim(3e5, 1e-3, nr_ts=50)
    e = s.build(hip_lib)
    info = e.schedule_info()
    assert info["launches_per_timestep"] == 2 and not info["resident"] and info["lag_planes"] == 0, info
    e.run(10)
    e.close()
    for flag in (capi.FLAG_KERNEL_WAVEFRONT, capi.FLAG_KERNEL_RESIDENT):
        e = s.build(hip_lib, flags=flag)
        with pytest.raises(capi.FdtdError, match=r"\(-5\)"):
            e.run(1)
        e.close()
    with pytest.raises(capi.FdtdError, match="single slab"):
        s.build(hip_lib, world=2, rank=0)
    # the library itself refuses a decomposed context
    e2 = capi.Engine(hip_lib, 14, 13, 12, s.dt, k0=0, nk=6, rank=0, world=2)
    with pytest.raises(capi.FdtdError, match="single slab"):
        e2.set_sheets([0], [0], [1.0], [0], np.ones((1, 1)), np.ones((1, 1)))
    e2.close()
    e3 = capi.Engine(oracle_lib, 8, 8, 8, 1e-12)
    with pytest.raises(capi.FdtdError, match="no conducting sheets"):
        e3.sheet_state()
    e3.close()


@pytest.mark.gpu
def test_cavity_q_against_closed_form(hip_lib):
    """TE101 of a 24 x 12 x 20 mm cavity walled by six sheets (sigma = 1e5 S/m, t = 1 mm >> delta): Q from the decay of the stored energy
    against Pozar (Microwave Engineering, 6.7) with all walls lossy.  Half-millimetre cells (48 x 24 x 40 inside): on 1 mm cells the
    wall loss, which sits on the wall's node plane while the tangential H it balances sits half a cell inside, reads Q 3.5 % low."""
    sc, sim = pkg("scene"), pkg("simulation")
    h = 0.5e-3
    a_, b_, d_ = 48, 24, 40                 # cells
    n = (a_ + 6, b_ + 6, d_ + 6)
    g = _grid(n, h)
    s = sc.Scene(unit=h)
    lo, hi = (3, 3, 3), (3 + a_, 3 + b_, 3 + d_)
    sigma = 1e5
    for ax in range(3):
        for side in (lo[ax], hi[ax]):
            st, sp = list(lo), list(hi)
            st[ax] = sp[ax] = side
            s.add_conducting_sheet(f"w{ax}{side}", sigma, 1e-3).add_box(st, sp)
    a, b, d = a_ * h, b_ * h, d_ * h
    c0, eta0 = 299792458.0, 376.730313668
    k = np.pi * np.sqrt(1 / a ** 2 + 1 / d ** 2)
    f = c0 * k / (2 * np.pi)
    # a y-directed soft source in the middle: TE101 (E along y) is the lowest mode it couples to; a narrow pulse around it
    xc, yc, zc = 3 + a_ // 2, 3 + b_ // 2, 3 + d_ // 2
    s.add_lumped_port(1, 0.0, [xc, yc - 1, zc], [xc, yc, zc], "y", 1.0)
    vox = sc.voxelize(s, g)
    nsteps = 60000
    run = sim.Simulation(g, vox, f0=f, fc=0.15 * f, boundary="PEC", nr_ts=nsteps, end_criteria=0.0)
    e = run.build(hip_lib)
    start = len(run.signal) + 2000
    e.run(start)
    t, en = [], []
    every = 50
    for q in range((nsteps - start) // every):
        e.run(every)
        sv, si = e.energy()
        t.append((start + (q + 1) * every) * run.dt)
        en.append(8.854187817e-12 * sv + MU0 * si)
    t, en = np.array(t), np.array(en)
    slope = np.polyfit(t, np.log(en), 1)[0]
    Q = 2 * np.pi * f / -slope
    Rs = np.sqrt(2 * np.pi * f * MU0 / (2 * sigma))
    l = 1
    Qc = (k * a * d) ** 3 * b * eta0 / (2 * np.pi ** 2 * Rs) / (2 * l ** 2 * a ** 3 * b + 2 * b * d ** 3 + l ** 2 * a ** 3 * d + a * d ** 3)
    print(f"cavity TE101 {f / 1e9:.3f} GHz: Q {Q:.1f}, closed form {Qc:.1f}")
    assert abs(Q / Qc - 1) <= 0.03, (Q, Qc)


def _fixed(metal, lib, tmp, metal_loss):
    s, P = pkg("solver_fdtd_hip"), pkg("params").PatchAntennaParams
    p = P.from_user_units(frequency_ghz=2.45, er=4.3, h_mm=1.6, loss_tangent=0.0, metal=metal)
    prep = s.prepare_hip_patch_fixed(p, work_dir=os.path.join(tmp, metal + str(metal_loss)), lib=lib, metal_loss=metal_loss)
    assert prep.ok, prep.message
    prep.FDTD.EndCriteria = 1e-6
    prep.FDTD.NrTS = max(int(prep.FDTD.NrTS), 200000)
    res = s.run_prepared_hip(prep, frequency_hz=2.45e9, verbose=0)
    assert res.ok, res.message
    assert res.stats["energy_db"] < -60.0, res.stats
    k = int(np.argmin(res.s11_dB))
    fr = float(res.freq[k])
    nfr = prep.nf.CalcNF2FF(prep.sim_path, [fr], np.arange(0.0, 181.0, 6.0), np.arange(0.0, 360.0, 12.0), center=[0, 0, 0])
    eta = float(np.asarray(nfr.Prad)[0]) / float(prep.port.CalcPort(prep.sim_path, np.array([fr])).P_acc[0])
    return eta, res, prep


def _eta_at_pattern(prep, res):
    f = res.f_pattern
    nfr = prep.nf.CalcNF2FF(prep.sim_path, [f], np.arange(0.0, 181.0, 6.0), np.arange(0.0, 360.0, 12.0), center=[0, 0, 0])
    return float(np.asarray(nfr.Prad)[0]) / float(prep.port.CalcPort(prep.sim_path, np.array([f])).P_acc[0])


@pytest.mark.gpu
def test_plugin_efficiency_pec_copper_tin(hip_lib, tmp_path):
    out = {}
    for name, loss in (("copper", False), ("copper", True), ("tin", True)):
        eta, res, prep = _fixed(name, hip_lib, str(tmp_path), loss)
        out["pec" if not loss else name] = eta
        assert res.radiation_efficiency is not None and res.gain_dBi is not None and res.realized_gain_dBi is not None
        # the result's efficiency against Prad / P_acc recomputed here at the frequency the pattern was evaluated at
        nfp = _eta_at_pattern(prep, res)
        assert abs(res.radiation_efficiency - nfp) <= 1e-9 * nfp, (res.radiation_efficiency, nfp)
        assert abs(res.gain_dBi - (10 * np.log10(res.Dmax) + 10 * np.log10(res.radiation_efficiency))) < 1e-9
        assert abs(np.max(res.intensity) - 10 * np.log10(res.Dmax)) < 1e-6
        assert res.realized_gain_dBi <= res.gain_dBi + 1e-12
        if loss:
            assert res.stats["sheet_edges"] > 0 and res.stats["sheet_fit_error"] <= 0.01
            assert res.stats["schedule"]["launches_per_timestep"] in (2, 3) and not res.stats["schedule"]["resident"]
    print("fixed scene, tan d = 0: eta at the S11 minimum", out,
          {k: 1 - out[k] / out["pec"] for k in ("copper", "tin")})
    assert 0.97 <= out["pec"] <= 1.03, out
    assert out["pec"] > out["copper"] > out["tin"], out
