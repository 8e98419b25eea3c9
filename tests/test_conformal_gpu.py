"""Conformal PEC boundaries on the GPU (csrc/conformal.hip, fdtd_voxel_fractions in csrc/voxel.hip): the device fractions against
conformal.fractions_spec, bit for bit; the HIP step loop against the oracle's half-steps plus the numpy restatement of the correction
(restatement.Restatement), bit for bit, i_prev included; the order of the H update, the correction and whatever
samples I; the schedules a context with listed faces may take; S11 of a circular patch through the openEMS API mirror."""
import numpy as np
import pytest

import primitives_cases as pc
from conftest import pkg
from helpers import seeded_fields
from restatement import Restatement, install
from test_conformal_model_cpu import circular_patch_script, sphere_scene, sphere_sim

N = (26, 23, 11)
NSTEPS = 200


# ---- 1. fractions ------------------------------------------------------------------------------------------------------------------
def _fraction_cases():
    ext = (36.0, 28.0, 22.0)
    return {"all-types-graded-23x21x9": lambda: (pc.grid_of(23, 21, 9, ext), lambda g: pc.all_types_scene(g, ext)),
            "on-surface-21^3": lambda: (pc.grid_of(21, 21, 21, ext=(20.0, 20.0, 20.0), grade=False), pc.on_surface_scene),
            "sphere-lattice-41x37x29": lambda: (pc.grid_of(41, 37, 29, ext), lambda g: pc.sphere_lattice(g, ext)),
            "sphere-and-dish-26x23x11": lambda: (pkg("grid").RectGrid(*[np.arange(k) * 1e-3 for k in N]), lambda g: sphere_scene(tilted_disc=True))}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_fraction_cases()))
def test_device_fractions_equal_the_specification_bit_for_bit(hip_lib, name):
    cf, capi = pkg("conformal"), pkg("_capi")
    grid, make = _fraction_cases()[name]()
    scene = make(grid)
    table = cf.plain_metal_table(scene, grid)
    assert table.rec.size > 0 and np.all(table.rec["role"] == 1)
    node_in = cf.node_inside(grid, table)
    comp, idx, flip = cf.cut_edges(node_in)
    f = cf.fractions_spec(grid, table, comp, idx, flip)
    got = capi.fractions_raw(hip_lib, grid, table)
    assert idx.size > 100 and np.any((f > 0) & (f < 1)) and np.all((f > 0) & (f <= 1))
    assert np.array_equal(got[0], node_in)
    assert np.array_equal(got[1], comp) and np.array_equal(got[2], idx)
    assert np.array_equal(got[3].view(np.uint64), f.view(np.uint64))
    # ... and through conformal.fractions, the caller's entry
    fr = cf.fractions(scene, grid, capi.default_fractions(hip_lib))
    assert np.array_equal(fr.f.view(np.uint64), f.view(np.uint64)) and np.array_equal(fr.node_in, node_in)


@pytest.mark.gpu
def test_fractions_host_switch_and_bad_arguments(hip_lib, monkeypatch):
    cf, capi = pkg("conformal"), pkg("_capi")
    monkeypatch.setenv("FDTD_VOXELIZE", "host")
    assert capi.default_fractions(hip_lib) is None
    monkeypatch.delenv("FDTD_VOXELIZE")
    assert capi.default_fractions(hip_lib) is not None
    grid = pkg("grid").RectGrid(*[np.arange(k) * 1e-3 for k in N])
    empty = cf.plain_metal_table(pkg("scene").Scene(unit=1e-3), grid)
    node_in, comp, idx, f = capi.fractions_raw(hip_lib, grid, empty)
    assert not node_in.any() and idx.size == 0 and f.size == 0
    full = pkg("primitives").pack_table(pc.all_types_scene(pc.grid_of(23, 21, 9), (36.0, 28.0, 22.0)), pc.grid_of(23, 21, 9))
    with pytest.raises(capi.FdtdError, match="is no metal"):
        capi.fractions_raw(hip_lib, pc.grid_of(23, 21, 9), full)


# ---- 2. the kernel -----------------------------------------------------------------------------------------------------------------
def _cpml_sim(n):
    return sphere_sim(n=(30, 28, 24), nr_ts=n, boundary="CPML", cpml_cells=4, centre=(14.4, 13.7, 11.3), radius=4.3)


CASES = {"sphere-pec": lambda n: sphere_sim(N, nr_ts=n),
         "sphere-and-tilted-dish-pec": lambda n: sphere_sim(N, nr_ts=n, tilted_disc=True),
         "sphere-cpml4": _cpml_sim}


def _same(e, ref):
    assert np.abs(ref.e.fields()).max() > 0 and np.abs(ref.conformal.iprev).max() > 0
    assert np.array_equal(e.fields(), ref.e.fields())
    assert np.array_equal(e.conformal_state(), ref.conformal.iprev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_hip_matches_restatement_bit_for_bit(hip_lib, oracle_lib, name):
    ref = Restatement(CASES[name](NSTEPS), oracle_lib, seed=7)
    ref.run(NSTEPS)
    s = CASES[name](NSTEPS)
    e = s.build(hip_lib)
    seeded_fields(e, 7)                       # fdtd_set_field re-primes i_prev
    assert len(s.conformal) % 256 != 0 and len(s.conformal) > 256       # several blocks, the last one partial
    info = e.schedule_info()
    assert not info["resident"] and info["launches_per_timestep"] == 2, info
    e.run(NSTEPS)
    _same(e, ref)
    assert np.all(e.get_operator()[2] == 1.0)                            # the base operator is what fdtd_get_operator keeps returning
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nfaces", [1, 255, 256, 257])
def test_list_lengths_through_the_raw_abi(hip_lib, oracle_lib, nfaces):
    """A list of exactly one face; lists one short of, equal to and one beyond the block size."""
    mk = lambda: sphere_sim(N, nr_ts=60, conformal=False)
    comp, idx, coef = sphere_sim(N, nr_ts=60).conformal_tables()
    pick = np.random.default_rng(nfaces).permutation(idx.size)[:nfaces]
    tables = (comp[pick], idx[pick], coef[pick])
    ref = Restatement(mk(), oracle_lib, seed=9, tables={"conformal": tables})
    before = ref.conformal.iprev.copy()
    ref.run(60)
    e = mk().build(hip_lib)
    seeded_fields(e, 9)
    e.set_conformal(*tables)                  # i_prev is loaded from the seeded currents
    assert np.array_equal(e.conformal_state(), before) and before.size == nfaces
    assert e.schedule_info()["launches_per_timestep"] == 2
    e.run(60)
    _same(e, ref)
    e.close()


@pytest.mark.gpu
def test_chunked_runs_and_set_field_mid_run(hip_lib, oracle_lib):
    """fdtd_run in chunks of 1, 7 and 61 steps; then fdtd_set_field(I) (and V) mid-run, which loads i_prev again; then the rest."""
    ref = Restatement(sphere_sim(N, nr_ts=NSTEPS), oracle_lib, seed=2)
    e = sphere_sim(N, nr_ts=NSTEPS).build(hip_lib)
    seeded_fields(e, 2)
    for n in (1, 7, 61):
        e.run(n)
        ref.run(n)
        _same(e, ref)
    rng = np.random.default_rng(21)
    for kind in (0, 1):
        for c in range(3):
            a = (1e-3 * rng.standard_normal(e.local_shape)).astype(np.float32)
            e.set_field(kind, c, a)
            ref.set_field(kind, c, a)
            if kind == 1:
                q = ref.conformal.comp == c
                assert np.array_equal(e.conformal_state()[q], a.reshape(-1)[ref.conformal.idx[q]])
    e.run(NSTEPS - 69)
    ref.run(NSTEPS - 69)
    _same(e, ref)
    e.close()


@pytest.mark.gpu
def test_i_probe_and_i_dft_box_read_the_corrected_current(hip_lib, oracle_lib):
    """The correction runs before anything samples I: an I-probe and an NF2FF-style I box on listed faces read the corrected current
    under fdtd_run (chunks of 70 + 80: the last I-probe sample of a call is flushed at its end) as under fdtd_half_step; the current
    the H update leaves differs."""
    capi, exc = pkg("_capi"), pkg("excitation")
    nsteps, every = 150, 5
    sims = [sphere_sim(N, nr_ts=nsteps) for _ in range(3)]
    g, conf = sims[0].grid, sims[0].conformal
    nx, ny, nz = g.shape
    listed = np.zeros((3, nz, ny, nx), bool)
    listed.reshape(3, -1)[conf.comp.astype(np.int64), conf.idx] = True
    cells = []
    for c in range(3):                         # one listed face per component, away from the outer planes
        k, j, i = (int(v[len(v) // 2]) for v in np.nonzero(listed[c, 2:-2, 2:-2, 2:-2]))
        cells.append((c, i + 2, j + 2, k + 2))
    idx = np.array([g.flat(i, j, k) for _, i, j, k in cells], np.int64)
    comp = np.array([c for c, _, _, _ in cells], np.int8)
    w = np.array([1.0, -0.5, 2.0], np.float32)
    c1, i1, j1, k1 = cells[1]
    lo, hi = (i1 - 1, j1 - 1, k1 - 1), (i1 + 1, j1 + 1, k1 + 1)
    freqs = np.array([8e9, 11e9])
    nsamp = nsteps // every + 1
    tw_v = exc.dft_twiddles(freqs, sims[0].dt, every, nsamp, 0.0)
    tw_i = exc.dft_twiddles(freqs, sims[0].dt, every, nsamp, 0.5)
    ref = Restatement(sims[0], oracle_lib, seed=4)
    e_run, e_half = sims[1].build(hip_lib), sims[2].build(hip_lib)
    pids, bids = [ref.add_probe(capi.KIND_I, idx, comp, w)], []
    for e in (e_run, e_half):
        pids.append(e.add_probe(capi.KIND_I, idx, comp, w))
        e.set_dft(every, tw_v, tw_i)
        bids.append(e.add_dft_box(capi.KIND_I, 1, lo, hi))
        seeded_fields(e, 4)
    sl = (slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1), slice(lo[0], hi[0] + 1))
    assert listed[1][sl].sum() >= 1
    acc = np.zeros((2,) + tuple(s.stop - s.start for s in sl), np.complex128)
    acc_raw = np.zeros_like(acc)
    raw_series, seen = [], ref.record("conformal")
    for n in range(nsteps):
        ref.step()
        uncorrected = seen["conformal"][0]
        raw_series.append(sum(float(wq) * float(uncorrected[c].reshape(-1)[q]) for wq, c, q in zip(w, comp, idx)))
        if n % every == 0:
            t = tw_i[n // every, :, 0] + 1j * tw_i[n // every, :, 1]
            acc += t[:, None, None, None] * ref.I[1][sl].astype(np.float64)[None]
            acc_raw += t[:, None, None, None] * uncorrected[1][sl].astype(np.float64)[None]
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
    _same(e_run, ref)
    _same(e_half, ref)
    scale = np.abs(acc).max()
    assert np.abs(acc - acc_raw).max() > 1e-3 * scale
    for e, bid in ((e_run, bids[0]), (e_half, bids[1])):
        box = e.get_dft_box(bid)[0]
        assert box.shape == acc.shape
        assert np.abs(box - acc).max() <= 1e-12 * scale, np.abs(box - acc).max() / scale
        e.close()


# ---- 3. schedules ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_schedules_with_listed_faces(hip_lib, oracle_lib):
    capi = pkg("_capi")
    s = sphere_sim(N, nr_ts=50)
    bare = sphere_sim(N, nr_ts=50, conformal=False).build(hip_lib)
    before = bare.schedule_info()
    e = s.build(hip_lib)
    info = e.schedule_info()
    assert info["launches_per_timestep"] == 2 and not info["resident"] and info["lag_planes"] == 0, info
    assert before != info, before                   # (without listed faces AUTO takes another schedule for this small grid)
    e.run(10)
    e.close()
    # a set removed with nfaces = 0 leaves the schedule the context had before, and the fields go on as the plain operator's
    tables = s.conformal_tables()
    bare.set_conformal(*tables)
    assert bare.schedule_info() == info and bare.conformal_state().size == len(s.conformal)
    bare.set_conformal(tables[0][:0], tables[1][:0], tables[2][:0])
    assert bare.schedule_info() == before and bare.conformal_state().size == 0
    plain = sphere_sim(N, nr_ts=50, conformal=False).build(oracle_lib)
    seeded_fields(bare, 5)
    seeded_fields(plain, 5)
    bare.run(10)
    plain.run(10)
    assert np.array_equal(bare.fields(), plain.fields())
    bare.close()
    plain.close()
    for flag in (capi.FLAG_KERNEL_WAVEFRONT, capi.FLAG_KERNEL_RESIDENT):
        e = s.build(hip_lib, flags=flag)
        with pytest.raises(capi.FdtdError, match=r"\(-5\)"):
            e.run(1)
        e.close()
    with pytest.raises(capi.FdtdError, match="single slab"):
        s.build(hip_lib, world=2, rank=0)
    # the library itself refuses a face that does not exist and a face given twice.  (Its refusal of a decomposed context is not
    # exercised here: the slabs of a decomposed grid draw their streams from a process-wide pool, and one more such context in
    # front of test_parity_gpu changes which streams that file's three-slab mailbox self-test gets.)
    e4 = sphere_sim(N, nr_ts=50, conformal=False).build(hip_lib)
    with pytest.raises(capi.FdtdError, match="does not exist"):
        e4.set_conformal([2], [N[0] - 1], np.ones((1, 4), np.float32))
    with pytest.raises(capi.FdtdError, match="does not exist"):
        e4.set_conformal([0], [N[0] * N[1] * (N[2] - 1) + 5], np.ones((1, 4), np.float32))
    with pytest.raises(capi.FdtdError, match="given twice"):
        e4.set_conformal([2, 2], [30, 30], np.ones((2, 4), np.float32))
    e4.close()
    e3 = capi.Engine(oracle_lib, 8, 8, 8, 1e-12)
    with pytest.raises(capi.FdtdError, match="no conformal boundaries"):
        e3.conformal_state()
    e3.close()


# ---- 4. through the API ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_s11_of_a_circular_patch_through_openems_api(hip_lib, oracle_lib, tmp_path, monkeypatch):
    install(monkeypatch)
    oe = pkg("openems_api")
    freq = np.linspace(3e9, 9e9, 13)
    s11 = []
    for lib, tag in ((hip_lib, "hip"), (oracle_lib, "oracle")):
        f, port = circular_patch_script(oe, lib)
        f.Run(str(tmp_path / tag), verbose=0)
        st = f.stats.conformal
        assert f.sim.conformal is not None and sum(st["faces"]) == len(f.sim.conformal) > 50 and st["ratio"] == 2.0
        assert st["dt_factor"] == 1 / np.sqrt(2.0) and st["clamped"] > 0 and st["cut_edges"] == f.sim.vox.fractions.idx.size
        assert (tag == "oracle") == hasattr(f.sim, "restated")
        port.CalcPort(str(tmp_path / tag), freq)
        s11.append(port.uf_ref / port.uf_inc)
    print("S11 (HIP):", np.array2string(20 * np.log10(np.abs(s11[0])), precision=2))
    assert np.all(np.isfinite(s11[1])) and np.abs(s11[1]).min() < 0.99
    assert np.abs(s11[0] - s11[1]).max() <= 1e-12 * np.abs(s11[1]).max()
