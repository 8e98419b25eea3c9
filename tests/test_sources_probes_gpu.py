"""Soft sources and probes of libfdtd_hip.so under every step schedule against the oracle (cases: tests/source_probe_cases.py; the
oracle's side of them: tests/test_sources_probes_cpu.py).  Fields bit for bit; every probe series EQUAL to probe_block's reduction
tree restated in float64 over the oracle's fields (source_probe_cases.tree_series) — the kernels document "identical sums to every
other schedule" for probe_block, wf_probe_tail and k_res_probes, and this pins them to a reference instead of to each other —; the
schedule a case was built to reach is the one fdtd_schedule_info reports; what a schedule asked for by name cannot run is refused with
FDTD_E_UNSUPPORTED and the documented text."""
import numpy as np
import pytest

import source_probe_cases as spc
from conftest import pkg
from helpers import rel_l2

pytestmark = pytest.mark.gpu


def _flags(sched):
    capi = pkg("_capi")
    return {"AUTO": capi.FLAG_KERNEL_AUTO, "DIRECT": capi.FLAG_KERNEL_DIRECT, "WF1": capi.FLAG_KERNEL_WAVEFRONT, "WFM": capi.FLAG_KERNEL_WAVEFRONT,
            "RESIDENT": capi.FLAG_KERNEL_RESIDENT}[sched]


def _knobs(monkeypatch, case, sched=None, extra=None):
    """The knobs fdtd_create reads, set before the engine is built; returns what is set."""
    env = {**case.env, **(extra or {})}
    if sched == "WF1":
        env["FDTD_WF_MULTI"] = "1"
    elif sched == "WFM":
        env["FDTD_WF_MULTI"] = None
    for k in spc.KNOBS:
        monkeypatch.delenv(k, raising=False)
    env = {k: v for k, v in env.items() if v is not None}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return env


def _fields_equal(fh, fo, what):
    assert np.isfinite(fo).all() and np.abs(fo).max() > 0
    assert np.array_equal(fh, fo), (what, f"rel L2 {rel_l2(fh, fo):.3e}", int(np.sum(fh != fo)))
    nz = fo != 0
    assert np.array_equal(fh[nz].view(np.uint32), fo[nz].view(np.uint32)), what


def _series_equal(case, engine, ref, what):
    for q, (first, p) in enumerate(case.all_probes()):
        got, tree, own = engine.get_probe(q), ref["tree"][q], ref["own"][q]
        assert len(got) == min(case.nsteps, case.cap) == len(tree), (what, q, len(got))
        assert not got[:first].any(), (what, q, "entries before the probe was added")
        bad = np.flatnonzero(got != tree)
        assert bad.size == 0, (what, f"probe {q} (kind {p[0]}, {p[1].size} cells)", f"{bad.size} entries differ, first at {bad[:1]}",
                               f"rel L2 to the tree {rel_l2(got, tree):.3e}, to the oracle's series {rel_l2(got, own):.3e}")
        assert rel_l2(got, own) < 1e-12, (what, q, rel_l2(got, own))


def _schedule_is(info, outcome, case, sched, env):
    """fdtd_schedule_info against what the case was built to reach."""
    what = (case.name, sched, env, info)
    mur = "MUR" in case.boundary
    if outcome == "resident":
        assert info["resident"] and info["launches_per_timestep"] == 1, what
        assert info["rows_per_strip"] == spc.regimes(case)["res_strips"], what          # (a resident context reports its tiles' strips here)
        assert info["timesteps_per_launch_max"] == int(env.get("FDTD_RES_CHUNK", 256)), what
        return
    assert not info["resident"], what
    if "FDTD_TYS" in env:
        assert info["rows_per_strip"] == min(int(env["FDTD_TYS"]), case.shape[1]), what
    if outcome == "one":
        assert info["launches_per_timestep"] == 1, what
        if env.get("FDTD_WF_MULTI") == "1":
            assert info["timesteps_per_launch_max"] == 1, what
        elif "FDTD_WF_MULTI" not in env:
            assert info["timesteps_per_launch_max"] > 1, what
    else:
        assert outcome == "two"
        assert info["launches_per_timestep"] >= 2 and (mur or info["launches_per_timestep"] == 2), what
        if mur and not spc.regimes(case)["fusable"]:
            assert info["launches_per_timestep"] == 5, what      # pre, E, post, apply, sources, H in passes of their own: no fused order left


def _run_and_compare(case, sched, outcome, env, hip_lib, oracle_lib):
    ref = spc.reference(case, oracle_lib)
    e = spc.engine_for(case, hip_lib, _flags(sched))
    spc.run(case, e)
    info = e.schedule_info()
    print(f"SCHEDULE {case.name} {sched} {env} -> {info}")
    assert e.step == ref["step"] == case.nsteps
    _schedule_is(info, outcome, case, sched, env)
    _fields_equal(e.fields(), ref["fields"], (case.name, sched, env))
    _series_equal(case, e, ref, (case.name, sched, env))
    if case.hard is not None:      # hard E edges: the overridden operator, and on every hard edge under a V-probe amp * sig[n - d] exactly
        idx, comp, amp, delay = case.hard
        op = e.get_operator()
        assert not op[0].reshape(3, -1)[comp.astype(int), idx].any() and not op[1].reshape(3, -1)[comp.astype(int), idx].any(), (case.name, sched)
        checked = 0
        for q, (first, (kind, pidx, pcomp, w)) in enumerate(case.all_probes()):
            hit = np.flatnonzero((idx == pidx[0]) & (comp == pcomp[0])) if (kind == spc.KIND_V and pidx.size == 1) else np.zeros(0, int)
            if hit.size:
                want = spc.hard_table(case, int(hit[0]))
                assert want.any() and np.array_equal(e.get_probe(q), want), (case.name, sched, q)
                checked += 1
        assert checked >= 4, (case.name, sched)
    return e


@pytest.mark.parametrize("name,sched,outcome,extra", spc.RUNS,
                         ids=[f"{n}-{s}" + "".join(f"-{k[5:].lower()}{v}" for k, v in x.items() if v) for n, s, _, x in spc.RUNS])
def test_directed_case_under_schedule(hip_lib, oracle_lib, monkeypatch, name, sched, outcome, extra):
    capi = pkg("_capi")
    case = spc.DIRECTED[name]
    env = _knobs(monkeypatch, case, sched, extra)
    if not outcome.startswith("refused: "):
        _run_and_compare(case, sched, outcome, env, hip_lib, oracle_lib)
        return
    # asked for by name where it cannot run: FDTD_E_UNSUPPORTED and the text, no fallback
    e = spc.engine_for(case, hip_lib, _flags(sched))
    info = e.schedule_info()
    print(f"SCHEDULE {case.name} {sched} {env} -> refused, {info}")
    assert info["launches_per_timestep"] == 0 and not info["resident"]
    with pytest.raises(capi.FdtdError) as err:
        e.run(1)
    assert str(err.value).startswith("run failed (-5): " + outcome[len("refused: "):]), str(err.value)
    assert e.step == 0


def test_a_65th_probe_is_refused(hip_lib):
    capi = pkg("_capi")
    case = spc.DIRECTED["D5"]
    e = spc.engine_for(case, hip_lib)
    with pytest.raises(capi.FdtdError, match="too many probes"):
        e.add_probe(*case.probes[1])


def test_slabs_cut_through_a_port(hip_lib, oracle_lib, monkeypatch):
    """D7: the source line, the current loop and the voltage path of a port on both sides of the cut between two slabs on the mailbox
    transport — fields as one slab's and the oracle's bit for bit; the two ranks' partial series add up to the single slab's."""
    capi = pkg("_capi")
    case = spc.DIRECTED["D7"]
    env = _knobs(monkeypatch, case)
    one = _run_and_compare(case, "AUTO", "resident", env, hip_lib, oracle_lib)
    ref = spc.reference(case, oracle_lib)
    engs = [spc.engine_for(case, hip_lib, rank=r, world=2, slab=(8 * r, 8)) for r in range(2)]
    blobs = [e.p2p_export() for e in engs]
    for r, e in enumerate(engs):
        e.p2p_attach(blobs[r - 1] if r > 0 else None, blobs[r + 1] if r + 1 < len(engs) else None)
    for n in case.calls:
        capi.run_linked(engs, n)
    print(f"SCHEDULE {case.name} two p2p slabs -> {[e.schedule_info() for e in engs]}")
    assert all(e.schedule_info()["transport"] == "p2p" for e in engs)
    both = np.concatenate([e.fields() for e in engs], axis=2)
    assert np.array_equal(both.view(np.uint32), one.fields().view(np.uint32))
    _fields_equal(both, ref["fields"], "two slabs")
    for q in range(len(case.probes)):
        parts = [e.get_probe(q) for e in engs]
        assert all(np.abs(p).max() > 0 for p in parts), q       # both ranks own cells of every probe
        assert rel_l2(parts[0] + parts[1], one.get_probe(q)) < 1e-12, q


@pytest.mark.parametrize("n", range(spc.N_DRAWN), ids=[f"case-{n:02d}" for n in range(spc.N_DRAWN)])
def test_drawn_case(hip_lib, oracle_lib, monkeypatch, n):
    case, flag = spc.drawn(n)
    env = _knobs(monkeypatch, case)
    try:
        ref = spc.reference(case, oracle_lib)
        e = spc.engine_for(case, hip_lib, _flags(flag))
        spc.run(case, e)                    # (AUTO and DIRECT cannot be refused: an FdtdError is a failure)
        info = e.schedule_info()
        print(f"SCHEDULE {case.name} {flag} {env} -> {info}")
        assert e.step == case.nsteps
        if "FDTD_TYS" in env and not info["resident"]:
            assert info["rows_per_strip"] == min(int(env["FDTD_TYS"]), case.shape[1])
        _fields_equal(e.fields(), ref["fields"], case.name)
        _series_equal(case, e, ref, case.name)
    except BaseException:
        print("FAILED CASE", flag, case.describe())
        raise


def test_drawn_cases_reach_all_three_schedules(hip_lib, monkeypatch):
    """The tally of fdtd_schedule_info over the drawn batch: the resident kernel, one launch per timestep and two or more launches
    each step at least four of the cases."""
    tally = {"resident": 0, "one": 0, "two": 0}
    for n in range(spc.N_DRAWN):
        case, flag = spc.drawn(n)
        _knobs(monkeypatch, case)
        info = spc.engine_for(case, hip_lib, _flags(flag)).schedule_info()
        assert info["launches_per_timestep"] >= 1, (n, info)
        tally["resident" if info["resident"] else "one" if info["launches_per_timestep"] == 1 else "two"] += 1
    print(f"SCHEDULE tally of the drawn batch -> {tally}")
    assert min(tally.values()) >= 4, tally
