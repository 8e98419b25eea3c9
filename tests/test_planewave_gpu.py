"""Plane-wave excitation on the GPU (csrc/planewave.hip): the HIP step loop against the oracle's half-steps plus the numpy restatement
of the corrections (Debye media, sheets, elements, then the plane wave — in the headers' order), bit for bit; block boundaries through
the raw ABI; the schedules a context with a plane wave may take; replacing and removing the set; and the RCS of a PEC sphere through
the openEMS API mirror against the restatement's."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT, pkg
from helpers import seeded_fields
from restatement import Restatement
from test_dispersion_model_cpu import _fr4
from test_sheet_model_cpu import _grid
from test_lumped_model_cpu import pec_cavity
from test_planewave_model_cpu import SPHERE, SPHERE_KA, sphere_csx, sphere_freqs

N_BIG = (26, 24, 22)
OBLIQUE = dict(e0=(2, -2, 1), direction=(1, 2, 2))
GOLDEN = os.path.join(ROOT, "tests", "golden", "planewave_sphere_rcs.json")


def _cavity_case(classes):
    add = lambda s: s.add_plane_wave("pw", **OBLIQUE).add_box([8, 6, 6], [19, 18, 16])
    return lambda n: pec_cavity(add, n=N_BIG, nr_ts=n, use_classes=classes)


def _open_scene(boundary):
    """Inside the plane-wave box: a Debye slab on a ground plane, a conducting sheet on it, a terminated port through it and a lumped
    element in the air above — everything at least one cell off the box surface."""
    def make(n):
        sc, sim = pkg("scene"), pkg("simulation")
        g = _grid(N_BIG)
        s = sc.Scene(unit=1e-3)
        med = _fr4(6e9, 2e9, 10e9)
        s.add_debye_material("sub", med.eps_inf, med.kappa, med.delta_eps, med.tau).add_box([8, 8, 8], [17, 15, 10])
        s.add_metal("gnd").add_box([8, 8, 8], [17, 15, 8])
        s.add_conducting_sheet("tin", 9.1e6, 5e-6).add_box([10, 9, 10], [15, 14, 10])
        s.add_lumped_port(1, 50.0, [12, 11, 8], [12, 11, 10], "z", 0.0)
        s.add_lumped_element("load", "x", R=100.0, L=3e-9, C=0.2e-12).add_box([11, 11, 12], [13, 11, 12])
        s.add_plane_wave("pw", **OBLIQUE).add_box([6, 6, 6], [19, 17, 15])
        return sim.Simulation(g, sc.voxelize(s, g), f0=6e9, fc=4e9, boundary=boundary, cpml_cells=4, nr_ts=n, end_criteria=0.0)
    return make


CASES = [("pec-oblique-classes", _cavity_case(True), True),
         ("pec-oblique-raw", _cavity_case(False), False),
         ("cpml-debye-sheet-port-element", _open_scene("CPML"), True),
         ("mur-debye-sheet-port-element", _open_scene("MUR"), True)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,make,classes", CASES, ids=[c[0] for c in CASES])
def test_hip_matches_restatement_bit_for_bit(hip_lib, oracle_lib, name, make, classes):
    nsteps = 300
    ref_sim = make(nsteps)
    ref = Restatement(ref_sim, oracle_lib)
    ref.run(nsteps)
    s = make(nsteps)
    e = s.build(hip_lib)
    assert e.operator_form()[0].startswith("classes") == classes, e.operator_form()
    # the tables the host hands fdtd_planewave_set come from the device operator, and equal the restatement's from the oracle's
    for a, b in zip(s.planewave_tables.args(), ref.pw_e.tables.args()):
        assert np.array_equal(a, b)
    assert s.planewave_tables.E[0].size > 256 and s.planewave_tables.H[0].size > 256
    info = e.schedule_info()
    assert not info["resident"] and info["launches_per_timestep"] == 2, info
    e.run(nsteps)
    tot = pkg("planewave").total_masks(s.grid.shape, s.plane_wave.lo, s.plane_wave.hi)[0]
    V = ref.e.fields()[0]
    assert all(np.abs(V[c][tot[c]]).max() > 0 for c in range(3))             # the wave is in the box
    assert np.array_equal(e.fields(), ref.e.fields())
    if "debye" in name:
        r = ref
        assert r.sheets is not None and np.abs(r.sheets.ib).max() > 0 and max(np.abs(u).max() for u in r.debye.u) > 0 and np.abs(r.elements.x).max() > 0
        assert np.array_equal(e.sheet_state()[1], r.sheets.ib) and np.array_equal(e.lumped_state()[1], r.elements.x)
    series = list(zip(s.port_series(), [(ref.get_probe(u), ref.get_probe(i)) for u, i in ref_sim._port_probe_ids]))
    assert len(series) == 1
    for (pu, pi), (qu, qi) in series:
        assert np.abs(qu).max() > 0 and np.array_equal(pu, qu) and np.array_equal(pi, qi)


def _hand_tables(n, nsig2=80, seed=3):
    """Hand-made lists of n edges and n faces inside the 14 x 13 x 12 cavity: random coefficients, delays of 0..40 half-steps in both
    terms (every fourth entry has no second term), and a pulse table short enough that late steps read past its end."""
    pwm = pkg("planewave")
    rng = np.random.default_rng(seed)
    nx, ny = 14, 13
    elems = [(c, i, j, k) for k in range(3, 9) for j in range(3, 10) for i in range(3, 11) for c in (2, 0, 1)]
    lists = []
    for q in range(2):
        pick = elems[:n] if q == 0 else elems[::-1][:n]
        idx = np.array([(k * ny + j) * nx + i for _, i, j, k in pick], np.int64)
        comp = np.array([c for c, _, _, _ in pick], np.int8)
        coef = (1e-3 * rng.standard_normal((n, 2))).astype(np.float32)
        coef[::4, 1] = 0
        m0 = rng.integers(0, 41, (n, 2)).astype(np.int32)
        w = rng.uniform(0, 1, (n, 2)).astype(np.float32)
        w[w >= 1] = 0
        lists.append((idx, comp, coef, m0, w))
    return pwm.Tables(lists[0], lists[1], pwm.signal2(10e9, 4e9, 2e-12, nsig2 // 2))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 600])
def test_entry_counts_across_block_boundaries(hip_lib, oracle_lib, n):
    nsteps = 60
    mk = lambda: pec_cavity(None, nr_ts=nsteps)
    tables = _hand_tables(n)
    assert tables.E[0].size == n and tables.H[0].size == n and 2 * nsteps > tables.sig2.size
    ref = Restatement(mk(), oracle_lib, tables={"pw": tables})
    seeded_fields(ref.e, 9)
    ref.run(nsteps)
    e = mk().build(hip_lib)
    e.set_planewave(*tables.args())
    seeded_fields(e, 9)
    assert e.schedule_info()["launches_per_timestep"] == 2
    e.run(nsteps)
    assert np.array_equal(e.fields(), ref.e.fields())
    # (the corrections did act: without them the fields differ)
    bare = mk().build(hip_lib)
    seeded_fields(bare, 9)
    bare.run(nsteps)
    assert not np.array_equal(bare.fields(), e.fields())


@pytest.mark.gpu
def test_schedules_with_a_plane_wave(hip_lib, oracle_lib, monkeypatch):
    capi = pkg("_capi")
    monkeypatch.delenv("FDTD_MUR_APPLY_PASS", raising=False)
    s = _cavity_case(True)(80)
    bare = pec_cavity(None, n=N_BIG, nr_ts=80).build(hip_lib)
    before = bare.schedule_info()
    bare.close()
    e = s.build(hip_lib)
    info = e.schedule_info()
    assert info["launches_per_timestep"] == 2 and not info["resident"] and info["lag_planes"] == 0, info
    assert before != info, before                   # (without the wave AUTO takes another schedule for this cavity)
    # Mur faces: the apply pass as a launch of its own makes three (the planner's own rule for a scene whose Mur faces nothing else
    # touches is two: the box stays two cells clear of them)
    m = _open_scene("MUR")(10)
    em = m.build(hip_lib)
    assert em.schedule_info()["launches_per_timestep"] == 2 and not em.schedule_info()["resident"]
    em.close()
    monkeypatch.setenv("FDTD_MUR_APPLY_PASS", "1")
    em = _open_scene("MUR")(10).build(hip_lib)
    assert em.schedule_info()["launches_per_timestep"] == 3 and not em.schedule_info()["resident"]
    em.close()
    monkeypatch.delenv("FDTD_MUR_APPLY_PASS")
    # fdtd_run(n) == n x (half_step E, half_step H); chunked calls == one call
    e.run(69)
    one = e.fields()
    e.close()
    e = s.build(hip_lib)
    for n in (1, 7, 61):
        e.run(n)
    assert np.array_equal(e.fields(), one)
    e.close()
    e = s.build(hip_lib)
    for _ in range(69):
        e.half_step(capi.PHASE_E)
        e.half_step(capi.PHASE_H)
    assert np.array_equal(e.fields(), one) and np.abs(one).max() > 0
    e.close()
    for flag in (capi.FLAG_KERNEL_WAVEFRONT, capi.FLAG_KERNEL_RESIDENT):
        e = s.build(hip_lib, flags=flag)
        with pytest.raises(capi.FdtdError, match=r"\(-5\).*plane-wave excitation: the two-launch schedule only"):
            e.run(1)
        e.close()
    with pytest.raises(capi.FdtdError, match="single slab"):
        s.build(hip_lib, world=2, rank=0)
    # the library itself refuses a decomposed context, a duplicate element and an element outside the grid
    t = _hand_tables(4)
    e2 = capi.Engine(hip_lib, 14, 13, 12, s.dt, k0=0, nk=6, rank=0, world=2)
    with pytest.raises(capi.FdtdError, match=r"plane-wave excitation: single slab only \(world = 1, no p2p transport, no linked contexts\)"):
        e2.set_planewave(*t.args())
    e2.close()
    e3 = pec_cavity(None, nr_ts=10).build(hip_lib)
    dup = list(t.E)
    dup[0] = dup[0].copy(); dup[1] = dup[1].copy()
    dup[0][3], dup[1][3] = dup[0][0], dup[1][0]
    with pytest.raises(capi.FdtdError, match="an edge given twice"):
        e3.set_planewave(*dup, *t.H, t.sig2)
    far = list(t.H)
    far[0] = far[0].copy()
    far[0][2] = 14 * 13 * 12
    with pytest.raises(capi.FdtdError, match="face 2 out of range"):
        e3.set_planewave(*t.E, *far, t.sig2)
    e3.run(3)                                        # (a refused set leaves the context as it was)
    e3.close()
    e4 = capi.Engine(oracle_lib, 8, 8, 8, 1e-12)
    with pytest.raises(capi.FdtdError, match="no plane-wave excitation"):
        e4.set_planewave(*t.args())
    e4.close()


@pytest.mark.gpu
def test_replacing_and_removing_the_set(hip_lib, oracle_lib):
    nsteps = 60
    mk = lambda: pec_cavity(None, nr_ts=nsteps)
    t1, t2 = _hand_tables(300, seed=3), _hand_tables(129, seed=5)
    empty = [a[:0] for a in t1.E] + [a[:0] for a in t1.H] + [None]
    # a second set replaces the first
    ref = Restatement(mk(), oracle_lib, tables={"pw": t2})
    seeded_fields(ref.e, 2)
    ref.run(nsteps)
    e = mk().build(hip_lib)
    before = e.schedule_info()
    e.set_planewave(*t1.args())
    assert e.schedule_info() != before
    e.set_planewave(*t2.args())
    seeded_fields(e, 2)
    e.run(nsteps)
    assert np.array_equal(e.fields(), ref.e.fields())
    e.close()
    # n = 0 removes it: the schedule and every bit are those of a context that never had one — the oracle's
    o = mk().build(oracle_lib)
    seeded_fields(o, 2)
    o.run(nsteps)
    for removed in (True, False):
        e = mk().build(hip_lib)
        if removed:
            e.set_planewave(*t1.args())
            e.set_planewave(*empty)
        assert e.schedule_info() == before
        seeded_fields(e, 2)
        e.run(nsteps)
        assert np.array_equal(e.fields(), o.fields())
        e.close()
    assert not np.array_equal(o.fields(), ref.e.fields())


@pytest.mark.gpu
def test_sphere_rcs_through_openems_api(hip_lib, tmp_path):
    """The RCS tutorial's calls on the HIP library: back- and forward-scatter RCS of the conformal PEC sphere at ka = 0.8, 1.6, 2.5 against
    the values the CPU restatement gives for the same scene (tests/golden/planewave_sphere_rcs.json, which
    test_planewave_model_cpu.test_pec_sphere_against_mie holds the restatement to), to 1e-6 relative."""
    api = pkg("openems_api")
    FDTD = api.openEMS(NrTS=SPHERE["nr_ts"], EndCriteria=0, lib=hip_lib, conformal=True, nf2ff_freqs=sphere_freqs(), nf2ff_mode="dft")
    CSX = api.ContinuousStructure()
    nf = sphere_csx(FDTD, CSX)
    FDTD.Run(str(tmp_path), verbose=0)
    sim = FDTD.sim
    assert sim.plane_wave is not None and FDTD.stats.planewave["edges"] > 0 and FDTD.stats.conformal["faces"] and FDTD.stats.steps == SPHERE["nr_ts"]
    assert FDTD.stats.schedule["launches_per_timestep"] == 2 and os.path.isfile(os.path.join(str(tmp_path), "et"))
    a = SPHERE["radius"] * SPHERE["h"]
    want = json.load(open(GOLDEN))["rcs_over_pi_a2"]
    for ka, f, (wb, wf) in zip(SPHERE_KA, sphere_freqs(), want):
        r = sim.rcs(f, [np.pi, 0.0], [0.0]) / (np.pi * a * a)
        print(f"ka = {ka}: back {r[0, 0]:.6f} (restatement {wb:.6f}), forward {r[1, 0]:.6f} ({wf:.6f})")
        assert abs(r[0, 0] / wb - 1) <= 1e-6 and abs(r[1, 0] / wf - 1) <= 1e-6, (ka, r[:, 0], wb, wf)
        # upstream's route: P_rad of CalcNF2FF over the spectrum of the et file is the same number
        res = nf.CalcNF2FF(str(tmp_path), f, [180.0, 0.0], [0.0], center=[0, 0, 0])
        et = np.loadtxt(os.path.join(str(tmp_path), "et"))
        ef = 2 * sim.dt * np.sum(et[:, 1] * np.exp(-2j * np.pi * f * et[:, 0]))
        rcs = 4 * np.pi * res.P_rad[0][:, 0] / (0.5 * abs(ef) ** 2 / 376.730313668) / (np.pi * a * a)
        assert np.allclose(rcs, r[:, 0], rtol=1e-6)
