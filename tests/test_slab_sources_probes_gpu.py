"""Soft sources and probes of libfdtd_hip.so on z-slabs of one process under every halo transport against the oracle's ONE slab (cases and
runner: tests/source_probe_cases.py; the oracle's side, where the cases sit and what the drawn batch covers:
tests/test_sources_probes_cpu.py).  The transports: the mailbox inside the two-launch kernels and inside k_step, linked contexts with
split and unsplit sweeps, half-steps with the halos carried by the host.

Fields as the single slab's bit for bit.  EVERY rank's series of EVERY probe equal, entry by entry, to probe_block's reduction tree
restated in float64 over the oracle's fields and the cells the rank owns, in list order (source_probe_cases.tree_series with planes=) —
a rank that samples its bottom plane's V before the H halo has arrived, or its top plane's I before the E halo has, fails here even
where its neighbour's error cancels it in the sum; the sum over the ranks within 1e-12 of the oracle's own series (a sum taken in
another association: the suite's bar for that); fdtd_schedule_info of every rank shows the transport and the launches per timestep the
run was forced into."""
import numpy as np
import pytest

import source_probe_cases as spc
from conftest import pkg
from helpers import rel_l2
from test_sources_probes_gpu import _fields_equal, _knobs

pytestmark = pytest.mark.gpu


def _cut_id(cuts):
    return "cut" + "-".join(str(k0) for k0, _ in cuts[1:])


def _schedules_are(engs, case, transport, what):
    """Every rank reports the transport; one launch per timestep inside k_step, two without Mur faces, five with (several slabs: the
    post, apply and source passes are launches of their own); a context driven by fdtd_half_step reports 0, as the header documents."""
    infos = [e.schedule_info() for e in engs]
    print(f"SCHEDULE {what} -> {infos}")
    for e, info in zip(engs, infos):
        b = case.boundary      # (a z face is the Mur face of the rank that owns its plane only)
        mur = "MUR" in b[:4] or (b[4] == "MUR" and e.k0 == 0) or (b[5] == "MUR" and e.k0 + e.nk == e.nz)
        assert info["transport"] == spc.TRANSPORT_REPORTED[transport] and not info["resident"], (what, info)
        n = info["launches_per_timestep"]
        if transport == "p2p-one":
            assert n == 1, (what, info)
        elif transport == "half-steps":
            assert n == 0, (what, info)       # include/fdtd_hip.h: "0: driven by fdtd_half_step"
        else:
            assert n >= 2 and n == (5 if mur else 2), (what, info)
        if "FDTD_TYS" in case.env:
            assert info["rows_per_strip"] == min(int(case.env["FDTD_TYS"]), case.shape[1]), (what, info)


def check_slabs(engs, cuts, probes, ids, nrec, want_fields, trees, own, what):
    """What every slab run asserts.  probes: [(first timestep, (kind, idx, comp, w))], ids: their probe ids on every rank; nrec: entries a
    series holds; trees[r][q]: the rank's reference, own[q]: the oracle's series of the single slab."""
    assert [(e.k0, e.nk) for e in engs] == [tuple(s) for s in cuts]
    _fields_equal(np.concatenate([e.fields() for e in engs], axis=2), want_fields, what)
    plane = engs[0].nx * engs[0].ny
    for q, (first, p) in enumerate(probes):
        parts = [e.get_probe(ids[q]) for e in engs]
        for r, (got, (k0, nk)) in enumerate(zip(parts, cuts)):
            tree = trees[r][q]
            k = p[1] // plane
            owned = int(np.sum((k >= k0) & (k < k0 + nk)))
            assert len(got) == nrec == len(tree), (what, r, q, len(got))
            assert not got[:first].any(), (what, r, q, "entries before the probe was added")
            if owned == 0:
                assert not got.any(), (what, r, q, "a rank that owns no cell of the probe")
            bad = np.flatnonzero(got != tree)
            assert bad.size == 0, (what, f"rank {r} (planes {k0}..{k0 + nk - 1}), probe {q} (kind {p[0]}, {owned} of {p[1].size} cells)",
                                   f"{bad.size} entries differ, first at {bad[:1]}", f"rel L2 to the tree {rel_l2(got, tree):.3e}")
        assert rel_l2(sum(parts), own[q]) < 1e-12, (what, q, rel_l2(sum(parts), own[q]))


def _run_and_check(case, cuts, transport, hip_lib, oracle_lib, monkeypatch):
    env = _knobs(monkeypatch, case, extra={"FDTD_RESIDENT": "0"})
    what = (case.name, _cut_id(cuts), transport, env)
    ref = spc.reference(case, oracle_lib)
    engs = spc.run_slabs(case, hip_lib, cuts, transport)      # (an FdtdError — the bound of p2p_pinned_blocks included — is a failure)
    assert all(e.step == case.nsteps == ref["step"] for e in engs)
    _schedules_are(engs, case, transport, what)
    probes = case.all_probes()
    check_slabs(engs, cuts, probes, list(range(len(probes))), min(case.nsteps, case.cap), ref["fields"], spc.slab_trees(case, oracle_lib, cuts),
                ref["own"], what)
    if case.hard is not None:
        _hard_edges_hold(case, engs, cuts, what)


def _hard_edges_hold(case, engs, cuts, what):
    """Every rank's operator shows vv = vi = 0 on the hard edges it owns (fdtd_build_operator keeps the overrides of its slab); on the
    owning rank a V-probe on a hard edge reads float32(amp * sig[n - d]) exactly, 0.0 outside the table, and 0.0 on every other rank —
    the check of test_excite_gpu.test_hard_e_under_all_three_schedules, per rank."""
    idx, comp, amp, delay = case.hard
    plane = case.shape[0] * case.shape[1]
    owned_any = 0
    for e, (k0, nk) in zip(engs, cuts):
        own = spc.in_planes(case, idx, (k0, nk))
        op = e.get_operator()
        local = idx[own] - k0 * plane
        assert op[0].shape[1] == nk and not op[0].reshape(3, -1)[comp[own].astype(int), local].any(), (what, "vv", k0)
        assert not op[1].reshape(3, -1)[comp[own].astype(int), local].any(), (what, "vi", k0)
        owned_any += int(own.sum())
    assert owned_any == idx.size
    checked = 0
    for q, (first, (kind, pidx, pcomp, w)) in enumerate(case.all_probes()):
        if kind != spc.KIND_V or pidx.size != 1:
            continue
        hit = np.flatnonzero((idx == pidx[0]) & (comp == pcomp[0]))
        if not hit.size:
            continue
        want = spc.hard_table(case, int(hit[0]))
        for e, planes in zip(engs, cuts):
            got = e.get_probe(q)
            if spc.in_planes(case, pidx, planes)[0]:
                assert np.array_equal(got, want) and want.any(), (what, q, planes)
            else:
                assert not got.any(), (what, q, planes)
        checked += 1
    assert checked >= 4, what


@pytest.mark.parametrize("name,cuts,transport,outcome", spc.SLAB_RUNS,
                         ids=[f"{n}-{_cut_id(c)}-{t}" + ("-refused" if o != "ok" else "") for n, c, t, o in spc.SLAB_RUNS])
def test_directed_case_on_slabs(hip_lib, oracle_lib, monkeypatch, name, cuts, transport, outcome):
    capi = pkg("_capi")
    case = spc.DIRECTED[name]
    if outcome == "ok":
        _run_and_check(case, cuts, transport, hip_lib, oracle_lib, monkeypatch)
        return
    # Mur faces on the mailbox transport: refused by name, before a timestep is taken
    _knobs(monkeypatch, case, extra={"FDTD_RESIDENT": "0"})
    with pytest.raises(capi.FdtdError) as err:
        spc.run_slabs(case, hip_lib, cuts, transport)
    assert str(err.value).startswith("run_linked failed (-2): rank 0: " + outcome[len("refused: "):]), str(err.value)


@pytest.mark.parametrize("n", range(spc.N_SLAB_DRAWN), ids=[f"slabs-{n:02d}" for n in range(spc.N_SLAB_DRAWN)])
def test_drawn_case_on_slabs(hip_lib, oracle_lib, monkeypatch, n):
    case, cuts, transport = spc.drawn_slabs(n)
    try:
        _run_and_check(case, cuts, transport, hip_lib, oracle_lib, monkeypatch)
    except BaseException:
        print("FAILED CASE", transport, cuts, case.describe())
        raise
    finally:
        spc.forget(case)
