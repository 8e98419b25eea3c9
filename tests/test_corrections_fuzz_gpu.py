"""All eight corrections of the step loop in one context on the GPU (Debye and Lorentz media, sheets, elements and the plane wave's edge
list behind the E phase; magnetic faces, conformal faces, the plane wave's face list and the H-field excitations behind the H update): a fixed-seed batch of
tests/fuzz_parity.py --corrections against restatement.Restatement; lists that overlap, through the raw C ABI, against the headers'
statement lists applied in the headers' order; fdtd_set_field of every component between two calls with everything present."""
import numpy as np
import pytest

import corrections_overlap_cases as oc
import fuzz_parity
from conftest import pkg
from helpers import seeded_fields

GROUP = 4      # cases per parametrised group of the batch


_BATCH = []


def _batch():
    """The drawn cases, once per session (drawing the excitations builds each case's scene); nobody changes them."""
    if not _BATCH:
        _BATCH.extend(fuzz_parity.corrections_batch())
    return _BATCH


@pytest.mark.gpu
@pytest.mark.parametrize("group", range(-(-fuzz_parity.CORRECTIONS_BATCH[0] // GROUP)))
def test_randomised_correction_cases_equal_the_restatement(hip_lib, oracle_lib, group):
    """Fields, every state array, port series, NF2FF spectra and the schedule after every run() call of each drawn case."""
    ran = 0
    for q, case in list(enumerate(_batch()))[GROUP * group:GROUP * (group + 1)]:
        try:
            problems, info = fuzz_parity.run_corrections_case(case, hip_lib, oracle_lib)
        except ValueError:      # a set-up the host layer refuses (test_corrections_fuzz_cpu.py holds them to one case in six)
            continue
        assert problems == [], (q, case, problems)
        assert info["launches_per_timestep"] in (2, 3) and not info["resident"], info
        ran += 1
    assert ran >= GROUP - 1


# ---- overlapping lists through the raw C ABI --------------------------------------------------------------------------------------------
def _hip_overlap(hip_lib, T, mur, drive):
    capi = pkg("_capi")
    sim = oc.overlap_sim(mur)
    e = sim.build(hip_lib, flags=capi.FLAG_KERNEL_DIRECT if drive == "direct" else 0)
    oc.set_tables(e, T)
    ids = oc.add_probes_and_boxes(e, sim.dt)
    seeded_fields(e, oc.SEED)
    for n in oc.CALLS:
        if drive == "half":
            for _ in range(n):
                e.half_step(0)
                e.half_step(1)
        else:
            e.run(n)
    return e, ids


@pytest.mark.gpu
@pytest.mark.parametrize("mur", [False, True], ids=["pec", "one-mur-face"])
def test_overlapping_lists_follow_the_headers_order(hip_lib, oracle_lib, monkeypatch, mur):
    """One edge listed for a sheet, an element and the plane wave inside a Debye box, another inside a Lorentz box; one face that is
    magnetic, conformal, on the plane wave's face list and twice on the soft list of the H-field excitations, a second one that is
    magnetic, on the plane wave's face list and on the hard list (corrections_overlap_cases.py).  fdtd_run under AUTO and DIRECT in two calls
    and fdtd_half_step pairs give the bits of the headers' statement lists applied in the headers' order; with a Mur face, under both
    Mur schedules.  The setters accept every overlap."""
    ref = oc.reference(oracle_lib, mur)
    T = ref.T
    assert np.isfinite(ref.fields).all() and all(np.abs(a).max() > 0 for k in ref.state for a in ref.state[k])
    runs = [(None, drive) for drive in ("auto", "direct", "half")] + ([("1", "auto")] if mur else [])
    launches = set()
    for apply_pass, drive in runs:
        if apply_pass is None:
            monkeypatch.delenv("FDTD_MUR_APPLY_PASS", raising=False)
        else:
            monkeypatch.setenv("FDTD_MUR_APPLY_PASS", apply_pass)
        e, (vp, ip, vb, ib) = _hip_overlap(hip_lib, T, mur, drive)
        tag = f"{drive}, apply pass {apply_pass}"
        info = e.schedule_info()
        assert not info["resident"] and info["launches_per_timestep"] in (2, 3), (tag, info)
        launches.add(info["launches_per_timestep"])
        fh = e.fields()
        assert np.array_equal(fh, ref.fields), f"{tag}: fields differ at {np.count_nonzero(fh != ref.fields)} entries, first {tuple(np.argwhere(fh != ref.fields)[0])}"
        got = oc.hip_state(e, T)
        for name, arrays in ref.state.items():
            for q, (a, b) in enumerate(zip(got[name], arrays)):
                assert np.array_equal(a, b), (tag, name, q, int(np.count_nonzero(a != b)))
        for pid, want in zip(vp, ref.v_series):      # voltages in front of every E-side correction
            assert np.array_equal(e.get_probe(pid)[:oc.STEPS], np.array(want)), (tag, "V-probe")
        for pid, want in zip(ip, ref.i_series):      # currents behind every H-side one
            assert np.array_equal(e.get_probe(pid)[:oc.STEPS], np.array(want)), (tag, "I-probe")
        # the hard face G: amp * sigH[n - delay] exactly, whatever the magnetic faces and the plane wave's list did there
        hard = np.concatenate([np.zeros(oc.HARD_G[1], np.float32), T["excite"][8], np.zeros(oc.STEPS, np.float32)])[:oc.STEPS]
        assert np.array_equal(e.get_probe(ip[2])[:oc.STEPS], (np.float32(oc.HARD_G[0]) * hard).astype(np.float64)), (tag, "hard face")
        for bid, want in list(zip(vb, ref.v_acc)) + list(zip(ib, ref.i_acc)):
            box = e.get_dft_box(bid)[0]
            assert box.shape == want.shape and np.abs(box - want).max() <= 1e-12 * np.abs(want).max(), (tag, "DFT box", np.abs(box - want).max() / np.abs(want).max())
        e.close()
    assert launches == ({2, 3} if mur else {2}), launches      # the Mur faces inside update_H, and as a pass of their own


# ---- fdtd_set_field with everything present ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_set_field_of_every_component_with_all_seven_present(hip_lib, oracle_lib):
    """The first drawn case with all eight corrections (the name is from when there were seven), two calls; between them fdtd_set_field of every V and every I component: i_prev
    of the magnetic and the conformal faces is re-primed from the new currents, the states of the Debye and Lorentz media, the sheets and
    the elements keep their bits, and everything equals the restatement, which does the same, after both calls."""
    case = next(c for c in _batch() if fuzz_parity.corrections_present(fuzz_parity.corrections_case_sim(c)) == set(fuzz_parity.CORRECTION_NAMES))
    case = dict(case, calls=[30, 30], sets=[None], env={}, drive="auto")
    so, sh = fuzz_parity.corrections_case_sim(case), fuzz_parity.corrections_case_sim(case)
    ref = fuzz_parity.corrections_reference(so, oracle_lib, seed=case["seed"])
    e = sh.build(hip_lib)
    seeded_fields(e, case["seed"])
    ref.run(30)
    e.run(30)
    assert fuzz_parity.corrections_state_problems(e, ref) == []
    e_side = lambda: ([a.copy() for c in range(3) for a in e.debye_state(c)[:2]] + [a.copy() for c in range(3) for a in e.lorentz_state(c)[:2]]
                      + list(e.sheet_state()) + list(e.lumped_state()))
    before = e_side()
    assert all(np.abs(a).max() > 0 for a in before if a.size)
    rng = np.random.default_rng(77)
    new = {}
    for kind in (0, 1):
        for c in range(3):
            new[kind, c] = (1e-3 * rng.standard_normal(e.local_shape)).astype(np.float32)
            ref.set_field(kind, c, new[kind, c])
            e.set_field(kind, c, new[kind, c])
    for a, b in zip(before, e_side()):
        assert np.array_equal(a, b)
    mag = sh.magnetic
    for c in range(3):
        (i0, j0, k0), (i1, j1, k1) = mag.lo[c], mag.hi[c]
        assert np.array_equal(e.magnetic_state(c)[0], new[1, c][k0:k1, j0:j1, i0:i1])
    comp, idx, _ = sh.conformal_tables()
    want = np.array([new[1, int(c)].reshape(-1)[g] for c, g in zip(comp, idx)], np.float32)
    assert want.size > 0 and np.array_equal(e.conformal_state(), want)
    assert fuzz_parity.corrections_state_problems(e, ref) == []
    ref.run(30)
    e.run(30)
    assert fuzz_parity.corrections_reference_problems(ref) == []
    assert fuzz_parity.corrections_state_problems(e, ref) == []
    for (uid, iid), (ru, ri) in zip(sh._port_probe_ids, so._port_probe_ids):
        assert np.array_equal(e.get_probe(uid)[:60], ref.get_probe(ru)[:60]) and np.array_equal(e.get_probe(iid)[:60], ref.get_probe(ri)[:60])
    e.close()
