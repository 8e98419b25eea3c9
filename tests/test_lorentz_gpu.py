"""Lorentz and Drude media on the GPU (csrc/lorentz.hip): the HIP step loop against the oracle's half-steps plus the numpy restatement
of every correction (Debye media, Lorentz media, sheets, elements after the E phase, magnetic faces after the H update), bit for bit;
block and vector boundaries through the raw ABI; the order of the V-probes, the V-DFT boxes and the correction; media on the node
planes of grid faces under both Mur schedules; the schedules a context with Lorentz media may take and what the library refuses; S11
through the openEMS API mirror."""
import numpy as np
import pytest

from conftest import pkg
from helpers import seeded_fields
from test_dispersion_model_cpu import _fr4, _graded
from test_sheet_model_cpu import _grid
from restatement import Restatement, install
from test_lorentz_model_cpu import TWO_PI, lorentz_cavity, lorentz_patch

N_SMALL, N_BIG = (14, 13, 12), (26, 24, 22)


def _lor():
    return pkg("lorentz")


def _cavity_case(classes):
    def add(s):
        s.add_lorentz_material("plasma", 1.0, 0.0, [TWO_PI * 7e9], [0.0], [3e9]).add_box([6, 6, 5], [12, 14, 12])
        s.add_lorentz_material("meta", 2.0, 0.01, TWO_PI * np.array([5e9, 8e9]), TWO_PI * np.array([9e9, 14e9]), [1e9, 0.0]).add_box([14, 6, 5], [19, 14, 9])
    return lambda n: lorentz_cavity(add, n=N_BIG, nr_ts=n, use_classes=classes)


def _open_scene(boundary):
    """The open scene of test_magnetic_gpu._open_scene with every correction in one context: a Debye substrate, a conducting sheet on
    it, a port through it, two elements, a Lorentz superstrate a cell above the sheet (around the upper element) and a lossy magnetic
    slab on top of that."""
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
        s.add_lorentz_material("super", 1.5, 0.0, TWO_PI * np.array([4e9, 6e9]), TWO_PI * np.array([0.0, 7e9]), [2e9, 5e8]).add_box([7, 7, 13], [18, 16, 15])
        s.add_material("ferrite", eps_r=1.5, mu_r=2.0, sigma_m=300.0).add_box([7, 7, 15], [18, 16, 17])
        return sim.Simulation(g, sc.voxelize(s, g), f0=6e9, fc=4e9, boundary=boundary, cpml_cells=4, nr_ts=n, end_criteria=0.0)
    return make


CASES = [("pec-blocks-classes", _cavity_case(True), True),
         ("pec-blocks-raw", _cavity_case(False), False),
         ("cpml-debye-lorentz-sheet-port-elements-magnetic", _open_scene("CPML"), True),
         ("mur-debye-lorentz-sheet-port-elements-magnetic", _open_scene("MUR"), True)]


def _same_state(e, ref):
    for c in range(3):
        vp, x, vi = e.lorentz_state(c)
        assert np.array_equal(vp, ref.lorentz.vprev[c]), c
        assert np.array_equal(x, ref.lorentz.x[c]), c
        assert np.array_equal(vi, ref.lorentz.vi[c]), c


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
    assert s.lorentz is not None and s.lorentz.K == 2
    info = e.schedule_info()
    assert not info["resident"] and info["launches_per_timestep"] in (2, 3), info
    e.run(nsteps)
    assert np.abs(ref.e.fields()).max() > 0 and min(np.abs(x).max() for x in ref.lorentz.x) > 0
    assert min(np.abs(v).max() for v in ref.lorentz.vprev) > 0
    if "debye" in name:
        assert ref.sheets is not None and np.abs(ref.sheets.ib).max() > 0 and max(np.abs(u).max() for u in ref.debye.u) > 0
        assert np.abs(ref.elements.x).max() > 0 and max(np.abs(p).max() for p in ref.magnetic.iprev) > 0
    else:
        assert len(s.lorentz.media) == 2
    assert np.array_equal(e.fields(), ref.e.fields())
    _same_state(e, ref)
    if ref.elements is not None:
        assert np.array_equal(e.lumped_state()[1], ref.elements.x)
    if ref.sheets is not None:
        assert np.array_equal(e.sheet_state()[1], ref.sheets.ib)
    if ref.debye:
        for c in range(3):
            assert np.array_equal(e.debye_state(c)[1], ref.debye.u[c])
    if ref.magnetic is not None:
        for c in range(3):
            assert np.array_equal(e.magnetic_state(c)[0], ref.magnetic.iprev[c])
    got = s.port_series()
    want = [(ref.get_probe(u), ref.get_probe(i)) for u, i in ref_sim._port_probe_ids]
    assert len(got) == len(want) == 1
    for (pu, pi), (qu, qi) in zip(got, want):
        assert np.abs(qu).max() > 0 and np.abs(qi).max() > 0
        assert np.array_equal(pu[:nsteps], qu[:nsteps]) and np.array_equal(pi[:nsteps], qi[:nsteps])


# threads (groups of four x-edges) over the components: one block less one, one block, one block and a thread of the NEXT component,
# several blocks; x ranges with an odd x0 (but for the single thread, whose four edges end at the grid face) and an x1 that is no multiple of 4 and reaches the last existing edge — i = 24 for x-edges
# (widened to [20, 28)), i = 25 for the others ([24, 28) / [20, 28)); per case the number of poles and of media (one medium: the
# wave-uniform table; several: the table in LDS), so that every instantiation of k_lorentz runs
BOXES = {1: {2: ((24, 5, 7), (26, 6, 8))},
         255: {1: ((17, 2, 2), (26, 19, 7))},
         256: {0: ((21, 2, 2), (25, 18, 10))},
         257: {0: ((21, 2, 2), (25, 18, 10)), 2: ((24, 5, 7), (26, 6, 8))},
         600: {2: ((21, 2, 1), (26, 22, 16))}}
RAW_CASES = [(1, 4, 2), (255, 2, 2), (256, 1, 1), (256, 4, 2), (257, 1, 2), (257, 4, 1), (600, 2, 1), (600, 4, 2)]


def _raw_media(K, nmedia):
    lo = _lor()
    a = lo.LorentzMedium(1.0, 0.0, TWO_PI * np.array([7e9, 5e9, 9e9, 3e9])[:K], TWO_PI * np.array([0.0, 9e9, 15e9, 0.0])[:K], np.array([3e9, 1e9, 0.0, 0.0])[:K])
    b = lo.LorentzMedium(1.0, 0.0, TWO_PI * np.array([4e9, 6e9, 2e9])[:min(K, 3)], TWO_PI * np.array([11e9, 0.0, 6e9])[:min(K, 3)], np.array([0.0, 8e9, 2e9])[:min(K, 3)])
    return [a, b][:nmedia]


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,nmedia", RAW_CASES)
def test_block_and_vector_boundaries_through_the_raw_abi(hip_lib, oracle_lib, n, K, nmedia):
    nsteps = 60
    mk = lambda: lorentz_cavity(None, n=N_BIG, nr_ts=nsteps)
    rng = np.random.default_rng(1000 * n + 10 * K + nmedia)
    lo, hi, w, med, threads = [], [], [], [], 0
    for c in range(3):
        if c in BOXES[n]:
            l, h = BOXES[n][c]
            shape = (h[2] - l[2], h[1] - l[1], h[0] - l[0])
            ww = (1e-3 * rng.uniform(0.2, 1.0, shape) * (rng.uniform(size=shape) > 0.3)).astype(np.float32)
            ww.reshape(-1)[0] = 1e-3
            if ww.size > 2:
                ww.reshape(-1)[1] = 0.0
            mm = rng.integers(0, nmedia, shape).astype(np.uint8)
            threads += shape[0] * shape[1] * ((((h[0] + 3) & ~3) - (l[0] & ~3)) // 4)
            assert (l[0] % 2 == 1 or h[0] - l[0] == 2) and h[0] % 4 != 0 and h[0] == N_BIG[0] - (1 if c == 0 else 0)
        else:
            l, h, ww, mm = (0, 0, 0), (0, 0, 0), np.zeros((0, 0, 0), np.float32), np.zeros((0, 0, 0), np.uint8)
        lo.append(l); hi.append(h); w.append(ww); med.append(mm)
    assert threads == n
    sim0 = mk()
    phi, gam, h_ = _lor().tables(_raw_media(K, nmedia), sim0.dt, K=K)
    assert phi.shape == (nmedia, K, 2, 2)
    tables = (phi, gam, h_, lo, hi, w, med if nmedia > 1 else None)
    ref = Restatement(sim0, oracle_lib, seed=9, tables={"lorentz": tables})
    ref.run(nsteps)
    e = mk().build(hip_lib)
    seeded_fields(e, 9)
    e.set_lorentz(*tables)
    info = e.schedule_info()
    assert info["launches_per_timestep"] == 2 and not info["resident"], info
    e.run(nsteps)
    assert np.array_equal(e.fields(), ref.e.fields())
    _same_state(e, ref)
    for c in BOXES[n]:
        vp, x, vi = e.lorentz_state(c)
        off = (w[c] == 0) | (vi == 0)                     # holes, and edges the operator holds at zero (the grid face at i = 25)
        assert not vp[off].any() and not x[:, :, off].any()                      # untouched edges keep their bits
        assert (~off).any() and np.all(vp[~off] != 0) and np.any(x[:, 0][:, ~off] != 0)
        if c != 0:
            assert np.all(vi[..., -1] == 0)               # i = 25: a grid face
        if w[c].size > 2:
            assert np.any(w[c] == 0)


def _order_sim(n):
    return lorentz_cavity(lambda s: s.add_lorentz_material("block", 2.0, 0.0, TWO_PI * np.array([8e9, 6e9]), TWO_PI * np.array([0.0, 12e9]),
                                                           [4e9, 1e9]).add_box([4, 4, 3], [9, 8, 8]), nr_ts=n)


@pytest.mark.gpu
def test_v_probe_and_v_dft_box_read_the_voltage_before_the_correction(hip_lib, oracle_lib):
    """fdtd_hip_lorentz.h: the correction follows the V-probes and the V-DFT boxes.  A V-probe and a V-DFT box on dispersive edges read
    the uncorrected voltage under fdtd_run (chunks of 70 + 80) as under fdtd_half_step; the corrected voltage differs."""
    capi, exc = pkg("_capi"), pkg("excitation")
    nsteps, every = 150, 5
    sims = [_order_sim(nsteps) for _ in range(3)]
    g = sims[0].grid
    cells = [(0, 6, 5, 5), (1, 5, 6, 4), (2, 7, 5, 6)]
    idx = np.array([g.flat(i, j, k) for _, i, j, k in cells], np.int64)
    comp = np.array([c for c, _, _, _ in cells], np.int8)
    w = np.array([1.0, -0.5, 2.0], np.float32)
    d = sims[0].lorentz
    for c, i, j, k in cells:
        assert d.w[c][k - d.lo[c][2], j - d.lo[c][1], i - d.lo[c][0]] != 0
    lo, hi = (5, 5, 4), (7, 6, 6)
    freqs = np.array([8e9, 11e9])
    nsamp = nsteps // every + 1
    tw_v = exc.dft_twiddles(freqs, sims[0].dt, every, nsamp, 0.0)
    tw_i = exc.dft_twiddles(freqs, sims[0].dt, every, nsamp, 0.5)
    ref = Restatement(sims[0], oracle_lib, seed=4)
    e_run, e_half = sims[1].build(hip_lib), sims[2].build(hip_lib)
    pids, bids = [], []
    for e in (ref, e_run, e_half):
        pids.append(e.add_probe(capi.KIND_V, idx, comp, w))
    for e in (e_run, e_half):
        e.set_dft(every, tw_v, tw_i)
        bids.append(e.add_dft_box(capi.KIND_V, 1, lo, hi))
        seeded_fields(e, 4)
    assert e_run.schedule_info()["launches_per_timestep"] == 2
    sl = (slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1), slice(lo[0], hi[0] + 1))
    acc = np.zeros((2,) + tuple(s.stop - s.start for s in sl), np.complex128)
    acc_after = np.zeros_like(acc)
    after_series, seen = [], ref.record("lorentz")
    for n in range(nsteps):
        ref.step()
        V_before, V_after = seen["lorentz"]
        after_series.append(sum(float(wq) * float(V_after[c].reshape(-1)[q]) for wq, c, q in zip(w, comp, idx)))
        if n % every == 0:
            t = tw_v[n // every, :, 0] + 1j * tw_v[n // every, :, 1]
            acc += t[:, None, None, None] * V_before[1][sl].astype(np.float64)[None]
            acc_after += t[:, None, None, None] * V_after[1][sl].astype(np.float64)[None]
    e_run.run(70)
    e_run.run(80)
    for _ in range(nsteps):
        e_half.half_step(0)
        e_half.half_step(1)
    want = ref.get_probe(pids[0])[:nsteps]
    assert want.size == nsteps and np.abs(want).max() > 0
    assert np.max(np.abs(want - np.array(after_series))) > 1e-3 * np.abs(want).max()      # the correction does change these voltages
    assert np.array_equal(e_half.get_probe(pids[2])[:nsteps], want)
    assert np.array_equal(e_run.get_probe(pids[1])[:nsteps], want)
    assert np.array_equal(e_run.fields(), ref.e.fields()) and np.array_equal(e_half.fields(), ref.e.fields())
    _same_state(e_run, ref)
    _same_state(e_half, ref)
    scale = np.abs(acc).max()
    assert np.abs(acc - acc_after).max() > 1e-3 * scale
    for e, bid in ((e_run, bids[0]), (e_half, bids[1])):
        box = e.get_dft_box(bid)[0]
        assert box.shape == acc.shape
        assert np.abs(box - acc).max() <= 1e-12 * scale, np.abs(box - acc).max() / scale


def _face_sim(name, nr_ts):
    """The four scenes of test_dispersion_gpu.test_media_on_grid_faces_under_both_mur_schedules with the Debye medium replaced by the
    two-pole Lorentz medium of _order_sim: a substrate slab that runs into the four side faces / a medium that fills the grid up to all
    six, on the graded 23 x 21 x 19 mesh, a port inside the medium."""
    sc, sim = pkg("scene"), pkg("simulation")
    g = _graded((23, 21, 19), seed=14)
    x, y, z = (l * 1e3 for l in g.lines)
    at = lambda p: [x[p[0]], y[p[1]], z[p[2]]]
    lo, hi = ((0, 0, 6), (22, 20, 10)) if name.startswith("slab") else ((0, 0, 0), (22, 20, 18))
    s = sc.Scene(unit=1e-3)
    s.add_lorentz_material("m", 2.0, 0.0, TWO_PI * np.array([8e9, 6e9]), TWO_PI * np.array([0.0, 12e9]), [4e9, 1e9]).add_box(at(lo), at(hi))
    s.add_lumped_port(1, 50.0, at((11, 10, 6)), at((11, 10, 10)), "z", 1.0)
    return sim.Simulation(g, sc.voxelize(s, g), f0=9e9, fc=5e9, boundary="MUR" if name.endswith("mur") else "PEC", nr_ts=nr_ts, end_criteria=0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["slab-to-four-mur", "filled-mur", "slab-to-four-pec", "filled-pec"])
def test_lorentz_media_on_grid_faces_under_both_mur_schedules(hip_lib, oracle_lib, monkeypatch, name):
    """Lorentz cells on the node planes of Mur (and PEC) faces, as test_dispersion_gpu has them for Debye media (the two share
    media_set and the dense box).  Without an apply pass the face voltages in memory between update_E and update_H are not the
    timestep's final ones, and k_lorentz runs exactly there; with FDTD_MUR_APPLY_PASS=1 they are.  The operator holds every edge of a
    face node plane (vi = 0) and such edges are no dispersive edges (fdtd_hip_lorentz.h): fields, port series and fdtd_lorentz_get's
    v_prev, states and vi of EVERY edge agree among both schedules and the restatement, bit for bit."""
    nsteps = 120
    ref_sim = _face_sim(name, nsteps)
    ref = Restatement(ref_sim, oracle_lib, seed=8)
    ref.run(nsteps)
    d = ref_sim.lorentz
    held = sum(int(np.count_nonzero((np.asarray(d.w[c]).reshape(ref.lorentz.vi[c].shape) != 0) & (ref.lorentz.vi[c] == 0))) for c in range(3))
    assert held > 300, held                      # the edges in question exist, in numbers
    fo = ref.e.fields()
    assert np.all(np.isfinite(fo)) and np.abs(fo).max() > 0 and min(np.abs(x).max() for x in ref.lorentz.x) > 0
    mur = name.endswith("mur")
    for apply_pass, want in ((None, 2), ("1", 3 if mur else 2)):
        if apply_pass is None:
            monkeypatch.delenv("FDTD_MUR_APPLY_PASS", raising=False)
        else:
            monkeypatch.setenv("FDTD_MUR_APPLY_PASS", apply_pass)
        s = _face_sim(name, nsteps)
        e = s.build(hip_lib)
        assert e.schedule_info()["launches_per_timestep"] == want, e.schedule_info()
        seeded_fields(e, 8)
        e.run(nsteps)
        fh = e.fields()
        assert np.array_equal(fh, fo), f"fields differ at {np.count_nonzero(fh != fo)} entries, first {tuple(np.argwhere(fh != fo)[0])}"
        _same_state(e, ref)
        for c in range(3):
            vp, x, vi = e.lorentz_state(c)
            rest = vi == 0
            assert rest.any() and np.all(vp[rest] == 0) and np.all(x[:, :, rest] == 0)
        for (pu, pi), (qu, qi) in zip(s.port_series(), [(ref.get_probe(u), ref.get_probe(i)) for u, i in ref_sim._port_probe_ids]):
            assert np.abs(qu).max() > 0 and np.abs(qi).max() > 0 and np.array_equal(pu[:nsteps], qu[:nsteps]) and np.array_equal(pi[:nsteps], qi[:nsteps])
        e.close()


@pytest.mark.gpu
def test_schedules_and_refusals_with_lorentz_media(hip_lib, oracle_lib):
    capi = pkg("_capi")
    s = _order_sim(50)
    bare = lorentz_cavity(None, nr_ts=50).build(hip_lib)
    before = bare.schedule_info()
    e = s.build(hip_lib)
    info = e.schedule_info()
    assert info["launches_per_timestep"] == 2 and not info["resident"] and info["lag_planes"] == 0, info
    assert before != info, before                   # (without media AUTO takes another schedule for this small cavity)
    e.run(10)
    e.close()
    mur = lorentz_cavity(lambda sc: sc.add_lorentz_material("block", 1.0, 0.0, [TWO_PI * 8e9]).add_box([4, 4, 3], [9, 8, 8]), nr_ts=50, boundary="MUR").build(hip_lib)
    info_m = mur.schedule_info()
    assert info_m["launches_per_timestep"] in (2, 3) and not info_m["resident"], info_m
    mur.run(10)
    mur.close()
    # a set removed with nmedia = 0 leaves the schedule the context had before
    tables = s.lorentz_tables()
    bare.set_lorentz(*tables)
    assert bare.schedule_info() == info
    bare.set_lorentz(tables[0][:0], tables[1][:0], tables[2][:0], *tables[3:])
    assert bare.schedule_info() == before
    assert all(a.size == 0 for c in range(3) for a in bare.lorentz_state(c))
    bare.run(10)
    bare.close()
    for flag in (capi.FLAG_KERNEL_WAVEFRONT, capi.FLAG_KERNEL_RESIDENT):
        e = s.build(hip_lib, flags=flag)
        with pytest.raises(capi.FdtdError, match=r"\(-5\).*Lorentz media"):
            e.run(1)
        e.close()
    with pytest.raises(capi.FdtdError, match="single slab"):
        s.build(hip_lib, world=2, rank=0)
    # the library itself refuses a decomposed context, too many poles or media, and a box that leaves the grid
    one_w, one_m = [np.full((1, 1, 1), 1e-3, np.float32)] * 3, [np.zeros((1, 1, 1), np.uint8)] * 3
    box = ([(1, 1, 1)] * 3, [(2, 2, 2)] * 3)
    tab = lambda nm, K: (np.zeros((nm, K, 2, 2), np.float32), np.zeros((nm, K, 2), np.float32), np.zeros((nm, K, 2), np.float32))
    e2 = capi.Engine(hip_lib, 14, 13, 12, s.dt, k0=0, nk=6, rank=0, world=2)
    with pytest.raises(capi.FdtdError, match=r"\(-5\).*single slab"):
        e2.set_lorentz(*tab(1, 1), *box, one_w, one_m)
    e2.close()
    e4 = lorentz_cavity(None, nr_ts=50).build(hip_lib)
    with pytest.raises(capi.FdtdError, match="K must be 1..4"):
        e4.set_lorentz(*tab(1, 5), *box, one_w, one_m)
    with pytest.raises(capi.FdtdError, match="at most 8 media"):
        e4.set_lorentz(*tab(9, 1), *box, one_w, one_m)
    with pytest.raises(capi.FdtdError, match="medium id 3 out of range"):
        e4.set_lorentz(*tab(2, 1), *box, one_w, [np.full((1, 1, 1), 3, np.uint8)] * 3)
    with pytest.raises(capi.FdtdError, match="leaves the grid"):
        e4.set_lorentz(*tab(1, 1), [(12, 1, 1)] * 3, [(14, 2, 2)] * 3, [np.full((1, 1, 2), 1e-3, np.float32)] * 3, None)
    e4.set_lorentz(*tab(1, 1), [(12, 1, 1), (12, 1, 1), (12, 1, 1)], [(13, 2, 2), (14, 2, 2), (14, 2, 2)],
                   [np.full((1, 1, 1), 1e-3, np.float32)] + [np.full((1, 1, 2), 1e-3, np.float32)] * 2, None)     # the last existing edges
    e4.run(2)
    with pytest.raises(capi.FdtdError, match="before the first timestep"):
        e4.set_lorentz(*tab(1, 1), *box, one_w, one_m)
    e4.close()
    e3 = capi.Engine(oracle_lib, 8, 8, 8, 1e-12)
    with pytest.raises(capi.FdtdError, match="no Lorentz media"):
        e3.lorentz_state(0)
    with pytest.raises(capi.FdtdError, match="no Lorentz media"):
        e3.set_lorentz(*tab(1, 1), *box, one_w, one_m)
    e3.close()


@pytest.mark.gpu
def test_s11_of_a_patch_under_a_lorentz_superstrate_through_openems_api(hip_lib, oracle_lib, tmp_path, monkeypatch):
    install(monkeypatch)
    freq = np.linspace(3e9, 9e9, 13)
    s11 = []
    for lib, tag in ((hip_lib, "hip"), (oracle_lib, "oracle")):
        f, port = lorentz_patch(lib)
        f.Run(str(tmp_path / tag), verbose=0)
        assert f.sim.lorentz is not None and f.stats.lorentz["media"][0]["names"] == ["super"] and sum(f.stats.lorentz["edges"]) > 0
        assert (tag == "oracle") == hasattr(f.sim, "restated")
        port.CalcPort(str(tmp_path / tag), freq)
        s11.append(port.uf_ref / port.uf_inc)
    print("S11 (HIP):", np.array2string(20 * np.log10(np.abs(s11[0])), precision=2))
    assert np.all(np.isfinite(s11[1])) and np.abs(s11[1]).min() < 0.99
    assert np.linalg.norm(s11[0] - s11[1]) <= 1e-3 * np.linalg.norm(s11[1])
