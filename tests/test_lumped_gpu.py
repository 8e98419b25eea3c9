"""Lumped R-L-C elements on the GPU (csrc/lumped.hip): the HIP step loop against the oracle's half-steps plus the numpy restatement of
the corrections (Debye media, sheets, elements — in the header's order), bit for bit; block boundaries through the raw ABI; the order
of V-probes, Mur passes and the correction; the schedules a context with elements may take; and S11 of a loaded strip through the
openEMS API mirror."""
import numpy as np
import pytest

from conftest import pkg
from test_dispersion_model_cpu import _fr4
from test_sheet_model_cpu import _grid, cavity_sim
from restatement import Restatement, install
from test_lumped_model_cpu import pec_cavity

N_BIG = (26, 24, 22)


def _cavity_case(kind, classes):
    def add(s):
        if kind == "parallel":
            s.add_lumped_element("coil", "z", L=2e-9).add_box([12, 11, 9], [12, 11, 12])
        else:
            s.add_lumped_element("trap", "y", R=3.0, L=4e-9, C=0.3e-12, kind="series").add_box([12, 9, 10], [13, 12, 10])
    return lambda n: pec_cavity(add, n=N_BIG, nr_ts=n, use_classes=classes)


def _open_scene(boundary):
    """A Debye substrate, a conducting sheet on it, a port through it and two elements — one inside the substrate (a Debye edge too),
    one in the air above the sheet."""
    def make(n):
        sc, sim = pkg("scene"), pkg("simulation")
        g = _grid(N_BIG)
        s = sc.Scene(unit=1e-3)
        med = _fr4(6e9, 2e9, 10e9)
        s.add_debye_material("sub", med.eps_inf, med.kappa, med.delta_eps, med.tau).add_box([6, 6, 8], [19, 17, 12])
        s.add_metal("gnd").add_box([6, 6, 8], [19, 17, 8])
        s.add_conducting_sheet("tin", 9.1e6, 5e-6).add_box([9, 8, 12], [16, 15, 12])
        s.add_lumped_port(1, 50.0, [12, 11, 8], [12, 11, 12], "z", 1.0)
        s.add_lumped_element("via-l", "z", R=1.0, L=1e-9, kind="series").add_box([15, 14, 8], [15, 14, 12])
        s.add_lumped_element("load", "x", R=100.0, L=3e-9, C=0.2e-12).add_box([11, 11, 14], [13, 11, 14])
        return sim.Simulation(g, sc.voxelize(s, g), f0=6e9, fc=4e9, boundary=boundary, cpml_cells=4, nr_ts=n, end_criteria=0.0)
    return make


CASES = [("pec-parallel-L-classes", _cavity_case("parallel", True), True),
         ("pec-series-RLC-raw", _cavity_case("series", False), False),
         ("cpml-debye-sheet-port-two-elements", _open_scene("CPML"), True),
         ("mur-debye-sheet-port-two-elements", _open_scene("MUR"), True)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,make,classes", CASES, ids=[c[0] for c in CASES])
def test_hip_matches_restatement_bit_for_bit(hip_lib, oracle_lib, name, make, classes):
    nsteps = 400
    ref_sim = make(nsteps)
    ref = Restatement(ref_sim, oracle_lib)
    ref.run(nsteps)
    s = make(nsteps)
    e = s.build(hip_lib)
    assert e.operator_form()[0].startswith("classes") == classes, e.operator_form()
    # the vi the host hands fdtd_lumped_set is the device operator's own
    idx, comp = s.lumped_tables()[:2]
    assert np.array_equal(s.lumped_vi(), e.get_operator()[1].reshape(3, -1)[comp.astype(np.int64), idx])
    info = e.schedule_info()
    assert not info["resident"] and info["launches_per_timestep"] in (2, 3), info
    e.run(nsteps)
    assert np.abs(ref.e.fields()).max() > 0 and np.all(np.abs(ref.elements.x).max(axis=1)[:1] > 0)
    if "debye" in name:
        assert ref.sheets is not None and np.abs(ref.sheets.ib).max() > 0 and max(np.abs(u).max() for u in ref.debye.u) > 0
    assert np.array_equal(e.fields(), ref.e.fields())
    hv, hx = e.lumped_state()
    assert np.array_equal(hv, ref.elements.vprev) and np.array_equal(hx, ref.elements.x)
    if ref.sheets is not None:
        assert np.array_equal(e.sheet_state()[1], ref.sheets.ib)
    for (pu, pi), (qu, qi) in zip(s.port_series(), [(ref.get_probe(u), ref.get_probe(i)) for u, i in ref_sim._port_probe_ids]):
        assert np.array_equal(pu, qu) and np.array_equal(pi, qi)


def _three_classes(dt):
    """Class tables that mix one-state and two-state rows: a parallel L, a series R-L-C, a series R-C.  (h at a thousandth: these edges'
    operator has no g0 folded in, and hundreds of explicit branches side by side would grow.)"""
    lm = pkg("lumped")
    els = [lm.Element("l", L=5e-9), lm.Element("rlc", R=4.0, L=6e-9, C=0.4e-12, kind="series"), lm.Element("rc", R=80.0, C=0.5e-12, kind="series")]
    _, phi, gam, h = lm.tables(els, np.arange(3), dt)
    assert not phi[0, 1].any() and phi[1, 1].any() and not phi[2, 1].any()
    return phi, gam, (h * np.float32(0.001)).astype(np.float32)


def _raw_tables(e, edges, dt):
    """(idx, comp, vi, cls, phi, gam, h) of fdtd_lumped_set for hand-picked edges [(comp, i, j, k)]: classes in turn, vi the operator's."""
    nz, ny, nx = e.local_shape
    vi_all = e.get_operator()[1]
    idx = np.array([(k * ny + j) * nx + i for _, i, j, k in edges], np.int64)
    comp = np.array([c for c, _, _, _ in edges], np.int8)
    vi = np.array([vi_all[c][k, j, i] for c, i, j, k in edges], np.float32)
    return (idx, comp, vi, (np.arange(idx.size) % 3).astype(np.int32)) + _three_classes(dt)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 600])
def test_edge_counts_across_block_boundaries(hip_lib, oracle_lib, n):
    nsteps = 60
    mk = lambda: pec_cavity(None, nr_ts=nsteps)
    edges = [(c, i, j, k) for k in range(3, 9) for j in range(3, 10) for i in range(3, 11) for c in (2, 0, 1)][:n]
    assert len(edges) == n
    tables = _raw_tables(mk().build(oracle_lib), edges, mk().dt)
    ref = Restatement(mk(), oracle_lib, seed=9, tables={"elements": tables})
    ref.run(nsteps)
    e = mk().build(hip_lib)
    e.set_lumped(*tables)
    from helpers import seeded_fields
    seeded_fields(e, 9)
    e.run(nsteps)
    assert np.all(np.isfinite(ref.elements.x)) and np.all(np.abs(ref.elements.x[0]) > 0)
    assert np.array_equal(e.fields(), ref.e.fields())
    hv, hx = e.lumped_state()
    assert np.array_equal(hv, ref.elements.vprev) and np.array_equal(hx, ref.elements.x)
    assert not hx[1][tables[3] != 1].any() and (n < 2 or hx[1][tables[3] == 1].any())


@pytest.mark.gpu
def test_v_probe_on_a_lumped_edge_is_sampled_before_the_correction(hip_lib, oracle_lib):
    """fdtd_hip_lumped.h: the correction follows the V-probes.  The scene layer keeps elements off probe lines; the C ABI states no such
    restriction, so a probe added there must read the voltage BEFORE k_lumped changed it, under fdtd_run as under fdtd_half_step."""
    from helpers import seeded_fields
    capi = pkg("_capi")
    nsteps = 150
    add = lambda s: s.add_lumped_element("trap", "z", R=2.0, L=3e-9, C=0.3e-12, kind="series").add_box([7, 6, 4], [7, 6, 7])
    sims = [pec_cavity(add, nr_ts=nsteps) for _ in range(3)]
    idx, comp = sims[0].lumped_tables()[:2]
    assert idx.size == 3
    w = np.array([1.0, -0.5, 2.0], np.float32)
    ref = Restatement(sims[0], oracle_lib, seed=4)
    e_run, e_half = sims[1].build(hip_lib), sims[2].build(hip_lib)
    pids = [e.add_probe(capi.KIND_V, idx, comp, w) for e in (ref, e_run, e_half)]
    for e in (e_run, e_half):
        seeded_fields(e, 4)
    assert e_run.schedule_info()["launches_per_timestep"] == 2
    ref.run(nsteps)
    e_run.run(70)
    e_run.run(80)
    for _ in range(nsteps):
        e_half.half_step(0)
        e_half.half_step(1)
    want = ref.get_probe(pids[0])[:nsteps]
    assert np.abs(want).max() > 0 and np.abs(ref.elements.x).max() > 0
    # (the correction does change what the probe would read: sampled after it, the series differs)
    after = sum(float(wq) * float(ref.V[c].reshape(-1)[g]) for wq, c, g in zip(w, comp, idx))
    assert after != want[-1]
    assert np.array_equal(e_half.get_probe(pids[2])[:nsteps], want)
    assert np.array_equal(e_run.get_probe(pids[1])[:nsteps], want)
    assert np.array_equal(e_run.fields(), ref.e.fields()) and np.array_equal(e_run.lumped_state()[1], ref.elements.x)
    assert np.array_equal(e_half.fields(), ref.e.fields()) and np.array_equal(e_half.lumped_state()[1], ref.elements.x)


@pytest.mark.gpu
def test_lumped_edges_on_a_mur_face_node_plane(hip_lib, oracle_lib, monkeypatch):
    """The scene layer has no reason to draw elements on a Mur face; fdtd_lumped_set takes any edge.  Edges on the node plane of a Mur
    face (the operator holds them: vi = 0, so only their states can tell) and live ones inside: k_lumped must read the face's FINAL
    voltage, so such a context takes the apply pass as a launch of its own — fields and states equal the restatement with the
    environment asking for either schedule."""
    from helpers import seeded_fields
    nsteps = 120
    edges = [(1, 0, j, k) for j in range(3, 9) for k in range(3, 9)] + [(2, 5, 0, k) for k in range(3, 8)] + \
            [(1, 6, j, k) for j in range(3, 9) for k in range(4, 7)] + [(0, i, 5, 5) for i in range(3, 9)]
    mk = lambda: cavity_sim(1.0, 1.0, sheet=False, boundary="MUR", nr_ts=nsteps)
    tables = _raw_tables(mk().build(oracle_lib), edges, mk().dt)
    assert np.count_nonzero(tables[2] == 0) == 36 + 5 and np.count_nonzero(tables[2]) == 18 + 6
    ref = Restatement(mk(), oracle_lib, seed=6, tables={"elements": tables})
    ref.run(nsteps)
    assert np.all(np.abs(ref.elements.x[0]) > 0)
    for apply_pass in (None, "1"):
        if apply_pass is None:
            monkeypatch.delenv("FDTD_MUR_APPLY_PASS", raising=False)
        else:
            monkeypatch.setenv("FDTD_MUR_APPLY_PASS", apply_pass)
        e = mk().build(hip_lib)
        e.set_lumped(*[t[41:] if q < 4 else t for q, t in enumerate(tables)])      # the live edges alone: the environment decides
        assert e.schedule_info()["launches_per_timestep"] == (2 if apply_pass is None else 3)
        e.set_lumped(*tables)
        info = e.schedule_info()
        assert info["launches_per_timestep"] == 3 and not info["resident"], info
        seeded_fields(e, 6)
        e.run(nsteps)
        assert np.array_equal(e.fields(), ref.e.fields())
        hv, hx = e.lumped_state()
        assert np.array_equal(hv, ref.elements.vprev) and np.array_equal(hx, ref.elements.x)
        e.close()


@pytest.mark.gpu
def test_schedules_with_elements(hip_lib, oracle_lib):
    capi = pkg("_capi")
    add = lambda s: s.add_lumped_element("trap", "z", R=2.0, L=3e-9, C=0.3e-12, kind="series").add_box([7, 6, 5], [7, 6, 6])
    s = pec_cavity(add, nr_ts=50)
    bare = pec_cavity(None, nr_ts=50).build(hip_lib)
    before = bare.schedule_info()
    e = s.build(hip_lib)
    info = e.schedule_info()
    assert info["launches_per_timestep"] == 2 and not info["resident"] and info["lag_planes"] == 0, info
    assert before != info, before                   # (without an element AUTO takes another schedule for this small cavity)
    e.run(10)
    e.close()
    # a set removed with n = 0 leaves the schedule the context had before
    tables = s.lumped_tables()
    bare.set_lumped(*tables)
    assert bare.schedule_info() == info
    bare.set_lumped(*[t[:0] for t in tables])
    assert bare.schedule_info() == before
    bare.run(10)
    bare.close()
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
        e2.set_lumped([0], [0], [1.0], [0], np.ones((1, 2, 2)), np.ones((1, 2)), np.ones((1, 2)))
    e2.close()
    e3 = capi.Engine(oracle_lib, 8, 8, 8, 1e-12)
    with pytest.raises(capi.FdtdError, match="no lumped elements"):
        e3.lumped_state()
    e3.close()


def _loaded_strip(lib):
    """A strip on a substrate over a ground plane, fed by a port at one end, with a gap bridged by a series R-L-C."""
    oa = pkg("openems_api")
    csx = oa.ContinuousStructure()
    csx.GetGrid().SetDeltaUnit(1e-3)
    for a, l in zip("xyz", (25, 23, 21)):
        csx.GetGrid().AddLine(a, np.arange(0.0, l + 1, 1.0))
    csx.AddMaterial("sub", epsilon=3.0).AddBox([5, 5, 8], [20, 18, 10])
    csx.AddMetal("gnd").AddBox([5, 5, 8], [20, 18, 8])
    csx.AddMetal("strip").AddBox([8, 11, 10], [12, 12, 10])
    csx.AddMetal("strip2").AddBox([14, 11, 10], [18, 12, 10])
    csx.AddLumpedElement("trap", "x", caps=True, R=5.0, C=0.3e-12, L=2e-9, LEtype=1).AddBox([12, 11, 10], [14, 12, 10])
    f = oa.openEMS(NrTS=1500, EndCriteria=0, lib=lib, cpml_cells=4)
    f.SetGaussExcite(6e9, 4e9)
    f.SetBoundaryCond(["PML_4"] * 6)
    f.SetCSX(csx)
    port = f.AddLumpedPort(1, 50.0, [8, 11, 8], [8, 12, 10], "z", 1.0)
    return f, port


@pytest.mark.gpu
def test_s11_of_a_loaded_strip_through_openems_api(hip_lib, oracle_lib, tmp_path, monkeypatch):
    install(monkeypatch)                          # the oracle library steps through the restatement
    freq = np.linspace(3e9, 9e9, 13)
    s11 = []
    for lib, tag in ((hip_lib, "hip"), (oracle_lib, "oracle")):
        f, port = _loaded_strip(lib)
        f.Run(str(tmp_path / tag), verbose=0)
        assert f.sim.element_stepped.size == 4 and f.stats.lumped[0]["n_ser"] == 2 and f.stats.lumped[0]["n_par"] == 2
        assert f.stats.lumped[0]["resonance_warped_hz"] < f.stats.lumped[0]["resonance_hz"]
        port.CalcPort(str(tmp_path / tag), freq)
        s11.append(port.uf_ref / port.uf_inc)
    print("S11 (HIP):", np.array2string(20 * np.log10(np.abs(s11[0])), precision=2))
    assert np.all(np.isfinite(s11[1])) and np.abs(s11[1]).min() < 0.99
    assert np.linalg.norm(s11[0] - s11[1]) <= 1e-3 * np.linalg.norm(s11[1])
