"""Magnetic materials on the GPU (csrc/magnetic.hip): the HIP step loop against the oracle's half-steps plus the numpy restatement of
the corrections (Debye media, sheets, elements after the E phase, magnetic faces after the H update), bit for bit; the correction
against the oracle's raw operator within the float32 budget; block and vector boundaries through the raw ABI; the order of the H
update, the correction and whatever samples I; fdtd_set_field; the schedules a context with magnetic faces may take; S11 through
the openEMS API mirror; and PMC walls under every schedule."""
import numpy as np
import pytest

from conftest import pkg
from helpers import seeded_fields
from test_dispersion_model_cpu import _fr4
from test_sheet_model_cpu import _grid
from restatement import Restatement, install
from test_magnetic_model_cpu import (BUDGET_SEEDS, FP32_BUDGET_F, budget_case, budget_sim, magnetic_cavity,
                                     magnetic_patch)

N_SMALL, N_BIG = (14, 13, 12), (26, 24, 22)


def _cavity_case(classes):
    def add(s):
        s.add_material("block", eps_r=2.0, mu_r=3.0).add_box([6, 6, 5], [15, 14, 12])
        s.add_material("lossy", mu_r=1.5, sigma_m=800.0).add_box([15, 6, 5], [19, 14, 9])
    return lambda n: magnetic_cavity(add, n=N_BIG, nr_ts=n, use_classes=classes)


def _open_scene(boundary):
    """The open scene of test_lumped_gpu._open_scene — a Debye substrate, a conducting sheet on it, a port through it and two
    elements — plus a lossy magnetic slab in the air above the sheet, around the upper element: every correction in one context."""
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
        s.add_material("ferrite", eps_r=1.5, mu_r=2.0, sigma_m=300.0).add_box([7, 7, 13], [18, 16, 16])
        return sim.Simulation(g, sc.voxelize(s, g), f0=6e9, fc=4e9, boundary=boundary, cpml_cells=4, nr_ts=n, end_criteria=0.0)
    return make


CASES = [("pec-blocks-classes", _cavity_case(True), True),
         ("pec-blocks-raw", _cavity_case(False), False),
         ("cpml-debye-sheet-port-elements-magnetic", _open_scene("CPML"), True),
         ("mur-debye-sheet-port-elements-magnetic", _open_scene("MUR"), True)]


def _same_state(e, ref):
    for c in range(3):
        ip, iv0 = e.magnetic_state(c)
        assert np.array_equal(ip, ref.magnetic.iprev[c]), c
        assert np.array_equal(iv0, ref.e.get_operator()[3][c][ref.magnetic.sl[c]]), c


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
    assert s.magnetic is not None and s.magnetic.ncls >= 2
    info = e.schedule_info()
    assert not info["resident"] and info["launches_per_timestep"] in (2, 3), info
    e.run(nsteps)
    assert np.abs(ref.e.fields()).max() > 0 and max(np.abs(p).max() for p in ref.magnetic.iprev) > 0
    if "debye" in name:
        assert ref.sheets is not None and np.abs(ref.sheets.ib).max() > 0 and max(np.abs(u).max() for u in ref.debye.u) > 0
        assert np.abs(ref.elements.x).max() > 0
    assert np.array_equal(e.fields(), ref.e.fields())
    _same_state(e, ref)
    # the base operator is what fdtd_get_operator keeps returning: ii = 1 everywhere
    assert np.all(e.get_operator()[2] == 1.0)
    if ref.elements is not None:
        assert np.array_equal(e.lumped_state()[1], ref.elements.x)
    if ref.sheets is not None:
        assert np.array_equal(e.sheet_state()[1], ref.sheets.ib)
    got = s.port_series()
    want = [(ref.get_probe(u), ref.get_probe(i)) for u, i in ref_sim._port_probe_ids]
    assert len(got) == len(want) == 1
    for (pu, pi), (qu, qi) in zip(got, want):
        assert np.abs(qi).max() > 0
        assert np.array_equal(pu[:nsteps], qu[:nsteps]) and np.array_equal(pi[:nsteps], qi[:nsteps])


@pytest.mark.gpu
def test_hip_correction_against_the_raw_operator(hip_lib, oracle_lib):
    """Independent of the kernel's restatement: e_hip = rel. L2 of the HIP fields (class operator + k_magnetic) and e_ref = rel. L2 of
    the float32 oracle on the raw operator, both against the double-precision oracle on the same float32 raw coefficients.
    e_hip <= F e_ref, F = FP32_BUDGET_F (profiles/magnetic/fp32_budget.txt)."""
    from helpers import load_oracle_f64
    lib64 = load_oracle_f64()

    def stepper(sim, seed, nsteps):
        e = sim.build(hip_lib)
        seeded_fields(e, seed)
        e.run(nsteps)
        out = e.fields()
        e.close()
        return out
    worst = 0.0
    for seed in BUDGET_SEEDS:
        e_hip, e_ref = budget_case(budget_sim, oracle_lib, lib64, seed, 300, stepper)
        print(f"seed {seed}: e_hip {e_hip:.3e}, e_ref {e_ref:.3e}, ratio {e_hip / e_ref:.3f} (F = {FP32_BUDGET_F})")
        assert 0 < e_ref < 1e-4
        worst = max(worst, e_hip / e_ref)
    assert FP32_BUDGET_F <= 10 and worst <= FP32_BUDGET_F, worst


# threads (groups of four x-faces) per component: one block less one, one block, one block and a thread of the NEXT component, several
# blocks; x ranges with an odd x0, an x1 that is no multiple of 4 and reaches i = nx - 1 = 25 (widened to [24, 28) / [20, 28))
BOXES = {1: [((25, 2, 2), (26, 3, 3))],
         255: [((25, 2, 2), (26, 19, 17))],
         256: [((21, 2, 2), (26, 18, 10))],
         257: [((21, 2, 2), (26, 18, 10)), ((25, 5, 7), (26, 6, 8))],
         600: [((21, 2, 1), (26, 22, 16))]}


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(BOXES))
def test_block_and_vector_boundaries_through_the_raw_abi(hip_lib, oracle_lib, n):
    nsteps = 60
    mk = lambda: magnetic_cavity(None, n=N_BIG, nr_ts=nsteps)
    rng = np.random.default_rng(n)
    lo, hi, cls, threads = [], [], [], 0
    for c in range(3):
        if c < len(BOXES[n]):
            l, h = BOXES[n][c]
            shape = (h[2] - l[2], h[1] - l[1], h[0] - l[0])
            q = rng.integers(0, 3, shape).astype(np.uint8)
            q.reshape(-1)[:3] = (1, 0, 2)[:q.size]
            threads += shape[0] * shape[1] * ((((h[0] + 3) & ~3) - (l[0] & ~3)) // 4)
            assert l[0] % 2 == 1 and h[0] % 4 != 0 and h[0] == N_BIG[0]
        else:
            l, h, q = (0, 0, 0), (0, 0, 0), np.zeros((0, 0, 0), np.uint8)
        lo.append(l); hi.append(h); cls.append(q)
    assert threads == n
    tables = (np.array([0.97, 1.0], np.float32), np.array([0.5, 0.25], np.float32), lo, hi, cls)
    ref = Restatement(mk(), oracle_lib, seed=9, tables={"magnetic": tables})
    seed_I = [ref.e.get_field(1, c) for c in range(3)]
    ref.run(nsteps)
    e = mk().build(hip_lib)
    seeded_fields(e, 9)
    e.set_magnetic(*tables)                 # i_prev is loaded from the seeded currents
    info = e.schedule_info()
    assert info["launches_per_timestep"] == 2 and not info["resident"], info
    e.run(nsteps)
    assert np.array_equal(e.fields(), ref.e.fields())
    _same_state(e, ref)
    for c in range(len(BOXES[n])):
        ip = e.magnetic_state(c)[0]
        off = cls[c] == 0
        assert np.array_equal(ip[off], seed_I[c][ref.magnetic.sl[c]][off])         # faces of class 0 keep their bits
        if cls[c].size > 2:
            assert off.any() and np.any(ip[~off] != seed_I[c][ref.magnetic.sl[c]][~off])


def _order_sim(n):
    return magnetic_cavity(lambda s: s.add_material("block", eps_r=2.0, mu_r=3.0, sigma_m=900.0).add_box([4, 4, 3], [9, 8, 8]), nr_ts=n)


@pytest.mark.gpu
def test_i_probe_and_i_dft_box_read_the_corrected_current(hip_lib, oracle_lib):
    """fdtd_hip_magnetic.h: the correction runs before anything samples I.  An I-probe and an I-DFT box on magnetic faces read the
    corrected current under fdtd_run (chunks of 70 + 80: the last I-probe sample of a call is flushed at its end) as under
    fdtd_half_step; the current the H update leaves differs."""
    capi, exc = pkg("_capi"), pkg("excitation")
    nsteps, every = 150, 5
    sims = [_order_sim(nsteps) for _ in range(3)]
    g = sims[0].grid
    cells = [(0, 6, 5, 5), (1, 5, 6, 4), (2, 7, 5, 6)]
    idx = np.array([g.flat(i, j, k) for _, i, j, k in cells], np.int64)
    comp = np.array([c for c, _, _, _ in cells], np.int8)
    w = np.array([1.0, -0.5, 2.0], np.float32)
    full = sims[0].magnetic.full_classes((N_SMALL[2], N_SMALL[1], N_SMALL[0]))
    assert all(full[c, k, j, i] for c, i, j, k in cells)
    lo, hi = (5, 5, 4), (7, 6, 6)
    freqs = np.array([8e9, 11e9])
    nsamp = nsteps // every + 1
    tw_v = exc.dft_twiddles(freqs, sims[0].dt, every, nsamp, 0.0)
    tw_i = exc.dft_twiddles(freqs, sims[0].dt, every, nsamp, 0.5)
    ref = Restatement(sims[0], oracle_lib, seed=4)
    e_run, e_half = sims[1].build(hip_lib), sims[2].build(hip_lib)
    pids, bids = [], []
    for e in (ref, e_run, e_half):
        pids.append(e.add_probe(capi.KIND_I, idx, comp, w))
    for e in (e_run, e_half):
        e.set_dft(every, tw_v, tw_i)
        bids.append(e.add_dft_box(capi.KIND_I, 1, lo, hi))
        for kind in (0, 1):          # seeded currents after the set: fdtd_set_field re-primes i_prev
            rng = np.random.default_rng(4) if kind == 0 else rng
            for c in range(3):
                e.set_field(kind, c, (1e-3 * rng.standard_normal(e.local_shape)).astype(np.float32))
    assert e_run.schedule_info()["launches_per_timestep"] == 2
    sl = (slice(None), slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1), slice(lo[0], hi[0] + 1))
    acc = np.zeros((2,) + tuple(s.stop - s.start for s in sl[1:]), np.complex128)
    acc_raw = np.zeros_like(acc)
    raw_series, seen = [], ref.record("magnetic")
    for n in range(nsteps):
        ref.step()
        uncorrected = seen["magnetic"][0]
        raw_series.append(sum(float(wq) * float(uncorrected[c].reshape(-1)[q]) for wq, c, q in zip(w, comp, idx)))
        if n % every == 0:
            t = tw_i[n // every, :, 0] + 1j * tw_i[n // every, :, 1]
            acc += t[:, None, None, None] * ref.I[1][sl[1:]].astype(np.float64)[None]
            acc_raw += t[:, None, None, None] * uncorrected[1][sl[1:]].astype(np.float64)[None]
    e_run.run(70)
    e_run.run(80)
    for _ in range(nsteps):
        e_half.half_step(0)
        e_half.half_step(1)
    want = ref.get_probe(pids[0])
    assert want.size == nsteps and np.abs(want).max() > 0
    assert np.max(np.abs(want - np.array(raw_series))) > 1e-3 * np.abs(want).max()      # the correction does change what the probe reads
    assert np.array_equal(e_half.get_probe(pids[2])[:nsteps], want)
    assert np.array_equal(e_run.get_probe(pids[1])[:nsteps], want)
    assert np.array_equal(e_run.fields(), ref.e.fields()) and np.array_equal(e_half.fields(), ref.e.fields())
    scale = np.abs(acc).max()
    assert np.abs(acc - acc_raw).max() > 1e-3 * scale
    for e, bid in ((e_run, bids[0]), (e_half, bids[1])):
        box = e.get_dft_box(bid)[0]
        assert box.shape == acc.shape
        assert np.abs(box - acc).max() <= 1e-12 * scale, np.abs(box - acc).max() / scale


@pytest.mark.gpu
def test_set_field_reprimes_i_prev(hip_lib, oracle_lib):
    """fdtd_set_field(FDTD_KIND_I) after fdtd_magnetic_set loads i_prev again: a run from seeded fields equals the restatement, and
    i_prev holds the seeded currents before the first step."""
    nsteps = 120
    ref = Restatement(_order_sim(nsteps), oracle_lib)
    e = _order_sim(nsteps).build(hip_lib)
    assert all(not e.magnetic_state(c)[0].any() for c in range(3))
    rng = np.random.default_rng(21)
    for kind in (0, 1):
        for c in range(3):
            a = (1e-3 * rng.standard_normal(e.local_shape)).astype(np.float32)
            e.set_field(kind, c, a)
            ref.set_field(kind, c, a)
            if kind == 1:
                assert np.array_equal(e.magnetic_state(c)[0], a[ref.magnetic.sl[c]])
    ref.run(nsteps)
    e.run(nsteps)
    assert np.array_equal(e.fields(), ref.e.fields())
    _same_state(e, ref)


@pytest.mark.gpu
def test_schedules_with_magnetic_faces(hip_lib, oracle_lib):
    capi = pkg("_capi")
    s = _order_sim(50)
    bare = magnetic_cavity(None, nr_ts=50).build(hip_lib)
    before = bare.schedule_info()
    e = s.build(hip_lib)
    info = e.schedule_info()
    assert info["launches_per_timestep"] == 2 and not info["resident"] and info["lag_planes"] == 0, info
    assert before != info, before                   # (without magnetic faces AUTO takes another schedule for this small cavity)
    e.run(10)
    e.close()
    mur = magnetic_cavity(lambda sc: sc.add_material("block", mu_r=3.0).add_box([4, 4, 3], [9, 8, 8]), nr_ts=50, boundary="MUR").build(hip_lib)
    info_m = mur.schedule_info()
    assert info_m["launches_per_timestep"] in (2, 3) and not info_m["resident"], info_m
    mur.run(10)
    mur.close()
    # a set removed with ncls = 0 leaves the schedule the context had before
    tables = s.magnetic.tables()
    bare.set_magnetic(*tables)
    assert bare.schedule_info() == info
    bare.set_magnetic(tables[0][:0], tables[1][:0], *tables[2:])
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
    # the library itself refuses a decomposed context, and more classes than a byte holds
    e2 = capi.Engine(hip_lib, 14, 13, 12, s.dt, k0=0, nk=6, rank=0, world=2)
    one = [np.ones((1, 1, 1), np.uint8)] * 3
    with pytest.raises(capi.FdtdError, match="single slab"):
        e2.set_magnetic([1.0], [0.5], [(1, 1, 1)] * 3, [(2, 2, 2)] * 3, one)
    e2.close()
    e4 = magnetic_cavity(None, nr_ts=50).build(hip_lib)
    with pytest.raises(capi.FdtdError, match=r"\(-5\).*256 distinct"):
        e4.set_magnetic(np.ones(256), np.ones(256), [(1, 1, 1)] * 3, [(2, 2, 2)] * 3, one)
    with pytest.raises(capi.FdtdError, match="leaves the grid"):
        e4.set_magnetic([1.0], [0.5], [(13, 1, 1)] * 3, [(15, 2, 2)] * 3, [np.ones((1, 1, 2), np.uint8)] * 3)
    e4.close()
    e3 = capi.Engine(oracle_lib, 8, 8, 8, 1e-12)
    with pytest.raises(capi.FdtdError, match="no magnetic materials"):
        e3.magnetic_state(0)
    e3.close()


@pytest.mark.gpu
def test_s11_of_a_patch_on_a_magnetic_substrate_through_openems_api(hip_lib, oracle_lib, tmp_path, monkeypatch):
    install(monkeypatch)
    freq = np.linspace(3e9, 9e9, 13)
    s11 = []
    for lib, tag in ((hip_lib, "hip"), (oracle_lib, "oracle")):
        f, port = magnetic_patch(lib)
        f.Run(str(tmp_path / tag), verbose=0)
        assert f.sim.magnetic is not None and f.stats.magnetic["media"] == ["sub"] and sum(f.stats.magnetic["faces"]) > 0
        assert (tag == "oracle") == hasattr(f.sim, "restated")
        port.CalcPort(str(tmp_path / tag), freq)
        s11.append(port.uf_ref / port.uf_inc)
    print("S11 (HIP):", np.array2string(20 * np.log10(np.abs(s11[0])), precision=2))
    assert np.all(np.isfinite(s11[1])) and np.abs(s11[1]).min() < 0.99
    assert np.linalg.norm(s11[0] - s11[1]) <= 1e-3 * np.linalg.norm(s11[1])


@pytest.mark.gpu
def test_pmc_walls_hip_equals_oracle_under_every_schedule(hip_lib, oracle_lib):
    """PMC is in the H metric tables, which every schedule takes as an argument: faces PMC / CPML / PEC / MUR mixed, HIP against the
    oracle bit for bit under AUTO, DIRECT, WAVEFRONT and RESIDENT — each where the planner accepts the grid (a refusal is
    FDTD_E_UNSUPPORTED at the first step; AUTO and DIRECT always run)."""
    from helpers import patch_sim
    capi = pkg("_capi")
    nsteps = 200
    ran = {}
    for bc in (["PMC", "PML_4", "PEC", "MUR", "PML_4", "PMC"], ["PML_4", "PMC", "PMC", "PML_4", "PEC", "PML_4"]):
        mk = lambda: patch_sim(*N_BIG, boundary=bc, cpml_cells=4, nr_ts=nsteps, nf2ff=False)
        ref = mk().build(oracle_lib)
        seeded_fields(ref, 5)
        ref.run(nsteps)
        want = ref.fields()
        hmet_zero = [int(np.count_nonzero(ref.get_operator()[3][c] == 0)) for c in range(3)]
        assert np.abs(want).max() > 0
        for name, flag in (("auto", 0), ("direct", capi.FLAG_KERNEL_DIRECT), ("wavefront", capi.FLAG_KERNEL_WAVEFRONT),
                           ("resident", capi.FLAG_KERNEL_RESIDENT)):
            e = mk().build(hip_lib, flags=flag)
            assert [int(np.count_nonzero(e.get_operator()[3][c] == 0)) for c in range(3)] == hmet_zero
            seeded_fields(e, 5)
            try:
                e.run(nsteps)
            except capi.FdtdError as err:
                assert "(-5)" in str(err) and name in ("wavefront", "resident"), err
                e.close()
                continue
            assert np.array_equal(e.fields(), want), (bc, name)
            ran.setdefault(name, 0)
            ran[name] += 1
            e.close()
    print("schedules that ran:", ran)
    assert ran.get("auto") == 2 and ran.get("direct") == 2 and ("wavefront" in ran or "resident" in ran), ran
