"""Soft sources and probes on the oracle alone (tests/source_probe_cases.py): what the oracle does with a source list and a probe is
restated in numpy, so that the reference of tests/test_sources_probes_gpu.py is itself pinned; every source call and every probe of
every case is live; and every directed case sits on the side of each kernel threshold it was built for (integer arithmetic restated
from csrc/, so a case that drifts is caught without a GPU)."""
import numpy as np
import pytest

import source_probe_cases as spc
from helpers import rel_l2

DIRECTED = sorted(spc.DIRECTED)
DRAWN = [f"case-{n:02d}" for n in range(spc.N_DRAWN)]


def _case(name):
    return spc.DIRECTED[name] if name in spc.DIRECTED else spc.drawn(int(name[5:]))[0]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _twin_fields(case, lib):
    """The case without its sources, half-stepped, the sources added in numpy after every E half-step: in list order
    V = float32(V + float32(amp * sig[step - delay])) where 0 <= step - delay < nsig."""
    e = spc.raw_engine(lib, (case.scene, case.shape), case.boundary, 0, case.cap, cpml_cells=case.cpml_cells)
    e.set_signal(case.signal)
    if case.seed is not None:
        spc.seeded_fields(e, case.seed)
    sig, nsig = case.signal.astype(np.float32), len(case.signal)
    srcs = case.all_sources()
    for step in range(case.nsteps):
        e.half_step(0)
        V = [None, None, None]
        for first, (idx, comp, amp, delay) in srcs:
            if step < first:
                continue
            t = step - delay.astype(np.int64)
            for q in np.flatnonzero((t >= 0) & (t < nsig)):
                c = int(comp[q])
                if V[c] is None:
                    V[c] = e.get_field(spc.KIND_V, c).reshape(-1)
                V[c][idx[q]] = np.float32(V[c][idx[q]] + np.float32(amp[q] * sig[t[q]]))
        for c in range(3):
            if V[c] is not None:
                e.set_field(spc.KIND_V, c, V[c].reshape(e.local_shape))
        e.half_step(1)
    return e.fields()


@pytest.mark.parametrize("name", DIRECTED + DRAWN)
def test_sources_and_probes_restated(oracle_lib, name):
    case = _case(name)
    ref = spc.reference(case, oracle_lib)
    fields = ref["fields"]
    assert np.isfinite(fields).all() and ref["step"] == case.nsteps
    # (a) the source list
    if "MUR" not in case.boundary:
        twin = _twin_fields(case, oracle_lib)
        assert np.array_equal(_bits(twin), _bits(fields)), case.describe()
    # (c) every source call moves the fields (with Mur faces this is all that is asserted of the list)
    for n in range(len(case.all_sources())):
        e = spc.engine_for(case, oracle_lib, without=n)
        spc.run(case, e, without=n)
        assert not np.array_equal(e.fields(), fields), (n, case.describe())
    # (b) probe_block's tree against the oracle's sequential sum, (c) live probes
    for q, (first, (kind, idx, comp, w)) in enumerate(case.all_probes()):
        own, tree = ref["own"][q], ref["tree"][q]
        assert len(own) == len(tree) == min(case.nsteps, case.cap)
        if idx.size == 0:
            assert not own.any() and not tree.any()
            continue
        assert np.abs(own[first:]).max() > 0 and not own[:first].any() and not tree[:first].any(), (q, case.describe())
        assert rel_l2(tree, own) < 1e-12, (q, rel_l2(tree, own), case.describe())


@pytest.mark.parametrize("name", DIRECTED)
def test_directed_cases_sit_where_they_were_built_to(name):
    case = spc.DIRECTED[name]
    r = spc.regimes(case)
    for key, want in case.expect.items():
        assert r[key] == want, (name, key, r[key], want)
    if case.nsteps > len(case.signal):      # late timesteps read past the end of the signal table
        assert 40 <= case.nsteps <= 120
    for cname, sched, outcome, env in spc.RUNS:
        if cname == name:
            assert spc.predict(case, sched, env) == outcome, (name, sched, env)


def test_directed_thresholds_are_all_present():
    """Both sides of every threshold the kernels have, by the regimes the cases compute for themselves."""
    r = {n: spc.regimes(c) for n, c in spc.DIRECTED.items()}
    d1 = {n: v for n, v in r.items() if n.startswith("D1-")}
    assert {v["sp_max"] for v in d1.values() if not v["dup"]} == {1, 32, 33, 255, 256, 257, 480}
    assert {v["sp_max"] for v in d1.values() if v["dup"]} == {2, 33, 256, 257}
    assert {(v["sp_max"] <= spc.SRC_SCAN_MAX, v["path"]) for v in d1.values() if not v["dup"]} == {(True, "scan"), (False, "dense")}
    assert {(v["sp_max"] <= spc.BLOCK, v["path"]) for v in d1.values() if v["dup"]} == {(True, "scan"), (False, "post")}
    assert r["D2-tys8"]["src_blocks"] == [0, 1] and r["D2-tys3"]["src_blocks"] == [0]
    assert sorted(v["near_mur"] for n, v in r.items() if n.startswith("D3-") and n != "D3-mixed") == [False] * 6 + [True] * 12
    for kind in ("mur", "cpml"):
        assert (r[f"D4-{kind}"]["tile_src_max"], r[f"D4-{kind}-src129"]["tile_src_max"]) == (spc.RES_MAX_SRC, spc.RES_MAX_SRC + 1)
        assert (r[f"D4-{kind}"]["tile_prb_max"], r[f"D4-{kind}-prb257"]["tile_prb_max"]) == (spc.RES_MAX_PRB, spc.RES_MAX_PRB + 1)
    sizes = [p[1].size for p in spc.DIRECTED["D5"].probes]
    assert len(sizes) == spc.MAX_PROBES and {0, 1, 255, 256, 257, 600, 288} <= set(sizes) and r["D5"]["owner_blocks_max"] > spc.BLOCK
    assert spc.DIRECTED["D6"].cap == 94 and spc.DIRECTED["D6"].nsteps == 99


def test_drawn_cases_cover_the_three_schedules():
    """What plan_schedule is expected to decide for the drawn batch (the GPU module tallies what it did decide)."""
    got = [spc.predict(*spc.drawn(n)) for n in range(spc.N_DRAWN)]
    assert min(got.count(k) for k in ("resident", "one", "two")) >= 4, got


def test_tree_sum_is_the_documented_order():
    """Cells 0 and 256 belong to thread 0 and cancel there, before cell 1 joins in the tree: 1; the sequential 1e16 + 1 - 1e16 is 0."""
    w = np.ones(300, np.float32)
    f = np.zeros(300, np.float32)
    f[0], f[1], f[256] = 1e16, 1.0, -1e16
    assert spc.tree_sum(w, f) == 1.0 and float(np.float32(1e16)) + 1.0 - float(np.float32(1e16)) == 0.0
    assert spc.tree_sum([], []) == 0.0
