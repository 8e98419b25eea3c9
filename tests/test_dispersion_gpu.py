"""Debye media on the GPU (csrc/dispersion.hip, include/fdtd_hip_dispersion.h): the HIP step loop against the oracle's half-steps
plus the numpy restatement of the correction (dispersion.correction), bit for bit — fields, branch states u_k and v_prev; fdtd_run
against half-steps; the refusals; the schedules; and the plugin's substrate_dispersion option."""
import numpy as np
import pytest

from conftest import pkg
from helpers import patch_sim, seeded_fields
from restatement import Restatement, install
from test_dispersion_model_cpu import _fr4, _graded, _grid


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
    if name == "multi-k8-three":
        # three media with K = 8 / 3 / 1: k_debye<true, 8>, two media padded
        g = _graded((45, 30, 22), seed=11)
        v = _media_scene(g, [("a", wide, (3, 3, 3), (17, 26, 18)), ("b", hi_band, (18, 5, 4), (30, 24, 17)), ("c", one, (31, 2, 2), (42, 27, 19))],
                         port=(50.0, (9, 14, 6), (9, 14, 11)))
        return sim.Simulation(g, v, boundary="MUR", **kw)
    if name == "multi-k8-eight":
        # the most media a context holds, every one with the most poles: medium ids 0 ... 7 in the lanes' bytes
        g = _graded((76, 20, 16), seed=12)
        boxes = [(f"m{q}", d.fit_constant_loss_tangent(3.0 + 0.4 * q, 0.01 + 0.004 * q, 9e9, 0.1e9, 30e9, K=8), (2 + 9 * q, 2 + q % 3, 2), (10 + 9 * q, 17 - q % 2, 13))
                 for q in range(8)]
        v = _media_scene(g, boxes, port=(50.0, (32, 9, 4), (32, 9, 9)))
        return sim.Simulation(g, v, boundary="PEC", **kw)
    if name == "many-blocks":
        # 41 x 30 x 20 cells of medium: 11 groups of four per row, 27-28 blocks of k_debye per component, the second and third component
        # start at a non-zero block, the last block of each is partial
        g = _graded((70, 50, 38), seed=13)
        v = _media_scene(g, [("m", hi_band, (14, 10, 9), (55, 40, 29))], port=(50.0, (30, 25, 12), (30, 25, 18)),
                         plain=[("p", 2.2, (10, 9, 6), (60, 42, 32))])
        return sim.Simulation(g, v, boundary="CPML", cpml_cells=8, **kw)
    if name in ("slab-to-four-mur", "slab-to-four-pec", "filled-mur", "filled-pec"):
        # a substrate slab that runs into the four side faces / a medium that fills the grid up to all six: dispersive cells on face nodes
        g = _graded((23, 21, 19), seed=14)
        box = ("m", hi_band, (0, 0, 6), (22, 20, 10)) if name.startswith("slab") else ("m", hi_band, (0, 0, 0), (22, 20, 18))
        v = _media_scene(g, [box], port=(50.0, (11, 10, 6), (11, 10, 10)))
        return sim.Simulation(g, v, boundary="MUR" if name.endswith("mur") else "PEC", **kw)
    raise KeyError(name)


def _x_aligned_sim(x0, x1, nx, nr_ts):
    """A medium over the cells [x0, x1) of a small PEC grid of nx nodes along x (a hole of plain dielectric inside when there is room)."""
    sim = pkg("simulation")
    g = _grid((nx, 11, 10))
    plain = [("hole", 2.0, (x0 + 2, 4, 3), (x0 + 5, 7, 7))] if x1 - x0 >= 7 else []
    sc = pkg("scene")
    x, y, z = (l * 1e3 for l in g.lines)
    s = sc.Scene(unit=1e-3)
    m = _fr4(9e9, 5e9, 15e9)
    s.add_debye_material("m", m.eps_inf, m.kappa, m.delta_eps, m.tau).add_box([x[x0], y[2], z[2]], [x[x1], y[8], z[7]], priority=1)
    for name, eps, lo, hi in plain:
        s.add_material(name, eps_r=eps).add_box([x[lo[0]], y[lo[1]], z[lo[2]]], [x[hi[0]], y[hi[1]], z[hi[2]]], priority=2)
    px = min(max(x0 + 1, 2), nx - 3)
    s.add_lumped_port(1, 50.0, [x[px], y[5], z[3]], [x[px], y[5], z[6]], "z", 1.0)
    return sim.Simulation(g, sc.voxelize(s, g), f0=9e9, fc=5e9, boundary="PEC", nr_ts=nr_ts, end_criteria=0.0)


def _same_as_restatement(s, e, ref_sim, ref):
    """Fields, Debye and sheet states and port series of the HIP context `e` (of `s`) against the restatement `ref` (of `ref_sim`), bit
    for bit; the reference side alone finite, moving, and with every live branch state off zero."""
    import fuzz_parity
    assert fuzz_parity.media_reference_problems(ref) == []
    fo = ref.e.fields()
    fh = e.fields()
    assert np.array_equal(fh, fo), f"fields differ at {np.count_nonzero(fh != fo)} entries, first {tuple(np.argwhere(fh != fo)[0])}"
    assert np.array_equal(fh[fo != 0].view(np.uint32), fo[fo != 0].view(np.uint32))
    for c in range(3 if ref.debye else 0):
        hv, hu, hvi = e.debye_state(c)
        assert np.array_equal(hvi, ref.debye.vi[c])
        assert np.array_equal(hv, ref.debye.vprev[c]), (c, np.count_nonzero(hv != ref.debye.vprev[c]))
        assert np.array_equal(hu, ref.debye.u[c]), (c, np.count_nonzero(hu != ref.debye.u[c]))
        off = ref.debye.w[c] == 0
        assert np.all(hv[off] == 0) and np.all(hu[:, off] == 0)
    if ref.sheets is not None:
        hv, hib = e.sheet_state()
        assert np.array_equal(hv, ref.sheets.vprev) and np.array_equal(hib, ref.sheets.ib)
    for (pu, pi), (qu, qi) in zip(s.port_series(), [(ref.get_probe(u), ref.get_probe(i)) for u, i in ref_sim._port_probe_ids]):
        assert np.abs(qu).max() > 0 and np.abs(qi).max() > 0 and np.array_equal(pu, qu) and np.array_equal(pi, qi)


CASES = ["pec-uniform", "pec-uniform-raw", "pec-graded-k8", "mur-graded", "cpml8-graded", "two-media-mur", "media-and-sheets-mur"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_matches_restatement_bit_for_bit(hip_lib, oracle_lib, name):
    nsteps = 300
    ref_sim = _sim(name, nsteps)
    ref = Restatement(ref_sim, oracle_lib)
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
        assert np.array_equal(hvi, ref.debye.vi[c])                      # the vi the library took from its own operator
        assert np.array_equal(hv, ref.debye.vprev[c]) and np.array_equal(hu, ref.debye.u[c])
        off = ref.debye.w[c] == 0
        assert np.all(hv[off] == 0) and np.all(hu[:, off] == 0)    # edges of the box outside the medium are left alone
        nonzero += np.count_nonzero(hu)
    assert nonzero > 0
    for (pu, pi), (qu, qi) in zip(s.port_series(), [(ref.get_probe(u), ref.get_probe(i)) for u, i in ref_sim._port_probe_ids]):
        assert np.abs(qu).max() > 0 and np.array_equal(pu, qu) and np.array_equal(pi, qi)
    if name == "media-and-sheets-mur":
        hv, hib = e.sheet_state()
        assert np.abs(hib).max() > 0 and np.array_equal(hv, ref.sheets.vprev) and np.array_equal(hib, ref.sheets.ib)
        on = [np.count_nonzero(ref.debye.w[c].reshape(-1)) for c in range(3)]
        assert min(on) > 0
    if name == "pec-uniform":
        assert s.debye.lo[0][0] == 3 and s.debye.hi[0][0] == 9 and s.grid.shape[0] % 4 != 0


# ---- directed cases: what the randomised batch below reaches by chance, by name ---------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,nsteps", [("multi-k8-three", 150), ("multi-k8-eight", 150), ("many-blocks", 80)])
def test_every_instantiation_and_many_blocks(hip_lib, oracle_lib, name, nsteps):
    """k_debye<true, 8> (three media of 8 / 3 / 1 poles; eight media of 8 poles) and a launch of 83 blocks whose components start at
    non-zero blocks, from seeded fields."""
    ref_sim, s = _sim(name, nsteps), _sim(name, nsteps)
    ref = Restatement(ref_sim, oracle_lib, seed=21)
    e = s.build(hip_lib)
    seeded_fields(e, 21)
    ref.run(nsteps)
    e.run(nsteps)
    d = s.debye
    if name == "many-blocks":
        blocks = [-(-(w.shape[0] * w.shape[1] * (-(-hi[0] // 4) - lo[0] // 4)) // 256) for w, lo, hi in zip(d.w, d.lo, d.hi)]
        assert min(blocks) >= 20 and all((w.shape[0] * w.shape[1] * (-(-hi[0] // 4) - lo[0] // 4)) % 256 for w, lo, hi in zip(d.w, d.lo, d.hi)), blocks
    else:
        assert d.K == 8 and len(d.media) == (3 if name == "multi-k8-three" else 8)
        assert all(set(np.unique(d.med[c][d.w[c] != 0])) == set(range(len(d.media))) for c in range(3))
    _same_as_restatement(s, e, ref_sim, ref)


X_ALIGN = [(4 + r0, 12 + r1, 20 + (r0 + 2 * r1 + r0 * r1) % 4) for r0 in range(4) for r1 in range(4)] + \
          [(0, 9, 18)] + [(5, nx - 1, nx) for nx in (17, 18, 19, 20)]


@pytest.mark.gpu
@pytest.mark.parametrize("x0,x1,nx", X_ALIGN, ids=[f"x{a}-{b}-nx{n}" for a, b, n in X_ALIGN])
def test_box_alignment_in_x(hip_lib, oracle_lib, x0, x1, nx):
    """The library widens every box to multiples of 4 in x: all 16 (x0 mod 4, x1 mod 4), every nx mod 4, the box that starts at x = 0 and
    the box whose x-edges end at nx - 2 and whose y- / z-edges sit on the last column.  Whole-grid field equality also pins that the
    widened columns outside the caller's box keep their bits."""
    nsteps = 60
    ref_sim, s = _x_aligned_sim(x0, x1, nx, nsteps), _x_aligned_sim(x0, x1, nx, nsteps)
    assert s.debye.lo[0][0] == x0 and s.debye.hi[0][0] == x1 and s.debye.lo[1][0] == x0 and s.debye.hi[1][0] == min(x1 + 1, nx)
    ref = Restatement(ref_sim, oracle_lib, seed=x0 + 100 * x1)
    e = s.build(hip_lib)
    seeded_fields(e, x0 + 100 * x1)
    ref.run(nsteps)
    e.run(nsteps)
    _same_as_restatement(s, e, ref_sim, ref)


def test_box_alignment_cases_cover_every_residue():
    assert {(a % 4, b % 4) for a, b, _ in X_ALIGN[:16]} == {(p, q) for p in range(4) for q in range(4)}
    assert {n % 4 for _, _, n in X_ALIGN[:16]} == {0, 1, 2, 3} and {n % 4 for _, _, n in X_ALIGN[17:]} == {0, 1, 2, 3}


@pytest.mark.gpu
def test_run_in_chunks(hip_lib, oracle_lib):
    """fdtd_run in calls of 1, 2, 97 and 100 timesteps (the V-probe launch in front of the corrections, the I-probe flush per call) on
    media + sheets + a port inside the medium: against ONE restatement run, and against fdtd_half_step on the library itself."""
    chunks = (1, 2, 97, 100)
    n = sum(chunks)
    ref_sim, s, h = (_sim("media-and-sheets-mur", n) for _ in range(3))
    ref = Restatement(ref_sim, oracle_lib, seed=3)
    e, eh = s.build(hip_lib), h.build(hip_lib)
    seeded_fields(e, 3)
    seeded_fields(eh, 3)
    ref.run(n)
    for k in chunks:
        e.run(k)
        for _ in range(k):
            eh.half_step(0)
            eh.half_step(1)
    _same_as_restatement(s, e, ref_sim, ref)
    _same_as_restatement(h, eh, ref_sim, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["slab-to-four-mur", "filled-mur", "slab-to-four-pec", "filled-pec"])
def test_media_on_grid_faces_under_both_mur_schedules(hip_lib, oracle_lib, monkeypatch, name):
    """Dispersive cells on the node planes of Mur (and PEC) faces.  Without an apply pass (two launches) the face voltages in memory
    between update_E and update_H are not the timestep's final ones, and k_debye runs exactly there; with FDTD_MUR_APPLY_PASS=1 (three
    launches) they are.  Every edge of a face node plane is held by the operator (vi = 0), and such edges are no dispersive edges
    (fdtd_hip_dispersion.h): fields, probe series and the states of EVERY edge agree among both schedules and the restatement."""
    nsteps = 120
    ref_sim = _sim(name, nsteps)
    ref = Restatement(ref_sim, oracle_lib, seed=8)
    ref.run(nsteps)
    held = sum(int(np.count_nonzero((ref_sim.debye.w[c] != 0) & (ref.debye.vi[c] == 0))) for c in range(3))
    assert held > 300, held                      # the edges in question exist, in numbers
    mur = name.endswith("mur")
    for apply_pass, want in ((None, 2), ("1", 3 if mur else 2)):
        if apply_pass is None:
            monkeypatch.delenv("FDTD_MUR_APPLY_PASS", raising=False)
        else:
            monkeypatch.setenv("FDTD_MUR_APPLY_PASS", apply_pass)
        s = _sim(name, nsteps)
        e = s.build(hip_lib)
        assert e.schedule_info()["launches_per_timestep"] == want, e.schedule_info()
        seeded_fields(e, 8)
        e.run(nsteps)
        _same_as_restatement(s, e, ref_sim, ref)
        for c in range(3):
            hv, hu, hvi = e.debye_state(c)
            rest = hvi == 0
            assert np.all(hv[rest] == 0) and np.all(hu[:, rest] == 0)
        e.close()


@pytest.mark.gpu
def test_randomised_media_cases_equal_the_restatement(hip_lib, oracle_lib):
    """The fixed-seed batch of tests/fuzz_parity.py --media (what it covers: tests/test_media_fuzz_cpu.py): drawn grids, boundaries,
    0 ... 8 media, holes, sheets, a port, NF2FF modes, Mur schedules, tilings and run() calls — fields and all states bit for bit, port
    series, energy and NF2FF face spectra.  (Further seeds: profiles/dispersion/randomised_media_parity.txt.)"""
    import fuzz_parity
    lines = []
    failed = fuzz_parity.run_batch(fuzz_parity.MEDIA_BATCH[0], fuzz_parity.MEDIA_BATCH[1], hip_lib, oracle_lib, log=lines.append, media=True)
    ran = [l for l in lines if ": ok " in l or ": FAIL" in l]
    assert 6 * len(ran) >= 5 * fuzz_parity.MEDIA_BATCH[0], "\n".join(lines)
    assert not failed, "\n".join(l for l in lines if "FAIL" in l)
    assert any("launches/ts 3" in l for l in ran) and any("launches/ts 2" in l for l in ran)


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
    install(monkeypatch)
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
