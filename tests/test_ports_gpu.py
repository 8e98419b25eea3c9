"""The port lists of ports.py on libfdtd_hip.so under every step schedule against the oracle (scenes: tests/ports_cases.py).  No step kernel
is new: a port is lists for fdtd_add_source and fdtd_add_probe — but a weighted source over a whole guide cross-section abutting PEC
walls (the dense source path), I-probes of 240 non-uniformly weighted faces over two half-planes, and ten probes in one scene are
regimes of those paths that the engine's own tests do not reach.  Fields bit for bit; every probe series EQUAL to probe_block's
reduction tree restated over the oracle's fields, and within 1e-12 relative L2 of the oracle's own (sequential) sums; the schedule a
run was forced into is the one fdtd_schedule_info reports; a schedule that cannot run a scene refuses it with its stated reason.  The
guide cut into z-slabs at its ports' planes, under the mailbox and the linked transports: the same, for every rank.  And one run through the public API: S21 of the guide on the device against the same run on the oracle."""
import numpy as np
import pytest

import ports_cases as pc
import source_probe_cases as spc
from conftest import pkg
from helpers import rel_l2
from test_slab_sources_probes_gpu import check_slabs
from test_sources_probes_gpu import _flags, _knobs, _schedule_is, _fields_equal

pytestmark = pytest.mark.gpu

FP32_BUDGET = 1.7e-5      # tests/fp32_error_budget.py: what the float32 step loop may cost a port quantity


@pytest.mark.parametrize("name,sched,outcome", pc.RAW_RUNS, ids=[f"{n}-{s}" for n, s, _ in pc.RAW_RUNS])
def test_port_lists_under_schedule(hip_lib, oracle_lib, monkeypatch, name, sched, outcome):
    capi = pkg("_capi")
    _, case = pc.raw(name)
    env = _knobs(monkeypatch, case, sched)
    assert spc.predict(case, sched, env) == outcome
    e, ids = pc.raw_engine(name, hip_lib, _flags(sched))
    info = e.schedule_info()
    print(f"SCHEDULE {name} {sched} {env} -> {info}")
    if outcome.startswith("refused: "):
        assert info["launches_per_timestep"] == 0 and not info["resident"]
        with pytest.raises(capi.FdtdError) as err:
            e.run(1)
        assert str(err.value).startswith("run failed (-5): " + outcome[len("refused: "):]), str(err.value)
        assert e.step == 0
        return
    ref = pc.raw_reference(name, oracle_lib)
    e.run(pc.RAW_STEPS)
    assert e.step == ref["step"] == pc.RAW_STEPS
    _schedule_is(e.schedule_info(), outcome, case, sched, env)
    _fields_equal(e.fields(), ref["fields"], (name, sched))
    for q, pid in enumerate(ids):
        got, tree, own = e.get_probe(pid), ref["tree"][q], ref["own"][q]
        assert len(got) == pc.RAW_STEPS and np.abs(own).max() > 0
        bad = np.flatnonzero(got != tree)
        assert bad.size == 0, (name, sched, f"probe {q} ({case.probes[q][1].size} cells)", f"{bad.size} entries differ, first at {bad[:1]}",
                               f"rel L2 to the tree {rel_l2(got, tree):.3e}, to the oracle's series {rel_l2(got, own):.3e}")
        assert rel_l2(got, own) < 1e-12, (name, sched, q, rel_l2(got, own))


SLAB_RUNS = [(cut, t) for cut in sorted(pc.WG_CUTS) for t in pc.WG_SLAB_TRANSPORTS]


@pytest.mark.parametrize("cut,transport", SLAB_RUNS, ids=[f"WG-{c}-{t}" for c, t in SLAB_RUNS])
def test_port_lists_on_slabs(hip_lib, oracle_lib, monkeypatch, cut, transport):
    """WG as z-slabs of one process, every rank built by Simulation.build with the port lists unchanged.  Cut at plane 24: port 1's 120
    source edges (the dense path) and its V-probe's 120 cells all lie in the bottom plane of the upper slab, which takes its V only after
    the H halo has arrived, and the 240 faces of its I-probe in planes 23 — the lower slab's top plane, which takes its I only after the E
    halo has arrived — and 24.  The second cut, at 40, does the same to port 2's V-plane.  Fields as the oracle's single slab; every
    rank's series EQUAL to probe_block's tree over the cells it owns; the ranks' series add up to the oracle's within 1e-12."""
    cuts = pc.WG_CUTS[cut]
    _, case = pc.raw("WG")
    _knobs(monkeypatch, case, extra={"FDTD_RESIDENT": "0"})
    ref = pc.raw_reference("WG", oracle_lib)
    engs, ids = pc.slab_engines("WG", hip_lib, cuts, spc.transport_flags(transport))
    spc.slab_stepper(engs, transport)(pc.RAW_STEPS)
    infos = [e.schedule_info() for e in engs]
    print(f"SCHEDULE WG {cut} {transport} -> {infos}")
    assert all(e.step == pc.RAW_STEPS == ref["step"] for e in engs)
    for info in infos:
        assert info["transport"] == spc.TRANSPORT_REPORTED[transport] and not info["resident"], info
        assert info["launches_per_timestep"] == (1 if transport == "p2p-one" else 2), info
    check_slabs(engs, cuts, [(0, p) for p in case.probes], ids, pc.RAW_STEPS, ref["fields"], ref["slab_trees"][cut], ref["own"], ("WG", cut, transport))


def test_the_guide_source_takes_the_dense_path():
    """More than SRC_SCAN_MAX distinct source edges in one strip-plane: the case, not the kernel, says which path the runs above took."""
    for name in ("WG", "WG-slab", "WG-odd"):
        r = spc.regimes(pc.raw(name)[1])
        assert r["sp_max"] == 120 > spc.SRC_SCAN_MAX and not r["dup"] and r["path"] == "dense" and r["fusable"], r
    # under the resident schedule the same plane is 120 source edges of ONE tile (at most 128), next to tiles of 120 and 240 probe cells
    r = spc.regimes(pc.raw("WG-odd")[1])
    assert (r["tile_src_max"], r["tile_prb_max"], r["res_why"]) == (120, 240, ""), r


def test_waveguide_s21_through_the_public_api(hip_lib, oracle_lib):
    """WG drawn, run and post-processed through openEMS.AddRectWaveGuidePort / CalcPort on the device and on the oracle."""
    f = pc.wg_freqs()
    got = pc.s_params(*pc.ran(hip_lib, "wg", pc.wg)[1], f)
    want = pc.s_params(*pc.ran(oracle_lib, "wg", pc.wg)[1], f)
    print("S21 device - oracle, worst:", np.abs(got[1] - want[1]).max(), " S11:", np.abs(got[0] - want[0]).max())
    assert np.all(np.abs(want[1]) > 0.99)
    assert np.abs(got[1] - want[1]).max() <= FP32_BUDGET
    assert np.abs(got[0] - want[0]).max() <= FP32_BUDGET
