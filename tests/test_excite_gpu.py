"""H-field excitations on the GPU (csrc/excite.hip) and hard E edges under every schedule: the HIP step loop against the oracle's
half-steps plus the numpy statement of include/fdtd_hip_excite.h (excite_cases.HLists), all six fields bit for bit; the corrections
that share a context with it; what the planner does with a set (slab contexts in a child process); and a scene drawn through the openEMS API mirror."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg
from helpers import seeded_fields
from excite_cases import ExciteRestatement, HLists, main_lists, main_sim, node
from test_dispersion_model_cpu import _fr4


@pytest.mark.gpu
def test_main_parity_case(hip_lib, oracle_lib):
    nsteps = 100
    lists = main_lists()
    assert lists.soft[0].size == 315 and lists.hard[0].size == 4 and lists.sigH.size == 40
    assert set(lists.soft[3].tolist()) == {0, 3, 57} and set(lists.faces()[1].tolist()) == {0, 1, 2}
    ref = ExciteRestatement(main_sim(), oracle_lib, lists, seed=4)
    ref.run(nsteps)
    e = main_sim().build(hip_lib)
    assert e.nx == 21
    e.set_excite(*lists.args())
    seeded_fields(e, 4)
    assert e.schedule_info()["launches_per_timestep"] == 2
    for n in (1, 7, 92):
        e.run(n)
    assert np.array_equal(e.fields(), ref.e.fields())
    # (the excitations did act, and the order within a face shows: the triples' entries as (1, -1, 1e-7) give other bits)
    bare = main_sim().build(hip_lib)
    seeded_fields(bare, 4)
    bare.run(nsteps)
    assert not np.array_equal(bare.fields(), e.fields())
    idx, comp, amp, delay = [a.copy() for a in lists.soft]
    amp[300:] = amp[300:].reshape(5, 3)[:, [0, 2, 1]].ravel()
    rev = ExciteRestatement(main_sim(), oracle_lib, HLists(lists.hard, (idx, comp, amp, delay), lists.sigH), seed=4)
    rev.run(nsteps)
    assert not np.array_equal(rev.e.fields(), ref.e.fields())
    e.close(); bare.close()


def _coexistence_scene(s):
    med = _fr4(10e9, 6e9, 14e9)
    s.add_debye_material("sub", med.eps_inf, med.kappa, med.delta_eps, med.tau).add_box([2, 2, 5], [8, 6, 7])
    s.add_material("ferrite", eps_r=1.5, mu_r=2.0, sigma_m=300.0).add_box([11, 2, 5], [17, 6, 7])
    s.add_lumped_element("load", "x", R=100.0, L=3e-9, C=0.2e-12).add_box([8, 6, 6], [10, 6, 6])


@pytest.mark.gpu
def test_coexistence_with_debye_magnetic_and_lumped(hip_lib, oracle_lib):
    nsteps = 100
    lists = main_lists(seed=2, rows=(8, 13))
    ref = ExciteRestatement(main_sim(_coexistence_scene), oracle_lib, lists, seed=6)
    assert ref.debye is not None and ref.magnetic is not None and ref.elements is not None
    # disjoint: no excited face is a magnetic face
    fi, fc = lists.faces()
    for c in range(3):
        full = np.zeros(ref.e.local_shape, np.uint8)
        full[ref.magnetic.sl[c]] = ref.magnetic.cls[c]
        assert not full.reshape(-1)[fi[fc == c]].any()
    ref.run(nsteps)
    s = main_sim(_coexistence_scene)
    e = s.build(hip_lib)
    e.set_excite(*lists.args())
    seeded_fields(e, 6)
    for c in range(3):                     # (i_prev of the magnetic faces restarts from the seeded currents, as in the restatement)
        assert np.array_equal(e.magnetic_state(c)[0], e.get_field(1, c)[ref.magnetic.sl[c]])
    assert e.schedule_info()["launches_per_timestep"] == 2
    for n in (1, 7, 92):
        e.run(n)
    assert np.array_equal(e.fields(), ref.e.fields())
    assert max(np.abs(u).max() for u in ref.debye.u) > 0 and np.abs(ref.elements.x).max() > 0
    for c in range(3):
        assert np.array_equal(e.debye_state(c)[1], ref.debye.u[c])
        assert np.array_equal(e.magnetic_state(c)[0], ref.magnetic.iprev[c])
    assert np.array_equal(e.lumped_state()[1], ref.elements.x)
    e.close()


@pytest.mark.gpu
def test_planner_with_a_set(hip_lib, oracle_lib):
    capi = pkg("_capi")
    lists = main_lists()
    empty = [a[:0] for a in lists.hard] + [a[:0] for a in lists.soft] + [None]
    e = main_sim().build(hip_lib)
    before = e.schedule_info()
    e.set_excite(*lists.args())
    info = e.schedule_info()
    assert info["launches_per_timestep"] == 2 and not info["resident"] and info["lag_planes"] == 0, info
    assert before != info, before                  # (without the set AUTO takes another schedule for a grid this small)
    e.set_excite(*empty)
    assert e.schedule_info() == before             # removing the set gives the schedule back ...
    o = main_sim().build(oracle_lib)
    for q in (e, o):
        seeded_fields(q, 3)
        q.run(30)
    assert np.array_equal(e.fields(), o.fields())  # ... and every bit of a context that never had one
    e.close()
    # fdtd_run(n) == n x (half_step E, half_step H)
    runs = []
    for half in (False, True):
        e = main_sim().build(hip_lib)
        e.set_excite(*lists.args())
        seeded_fields(e, 3)
        if half:
            for _ in range(70):
                e.half_step(capi.PHASE_E)
                e.half_step(capi.PHASE_H)
        else:
            e.run(70)
        runs.append(e.fields())
        e.close()
    assert np.array_equal(runs[0], runs[1]) and np.abs(runs[0]).max() > 0
    for flag in (capi.FLAG_KERNEL_WAVEFRONT, capi.FLAG_KERNEL_RESIDENT):
        e = main_sim().build(hip_lib, flags=flag)
        e.set_excite(*lists.args())
        assert e.schedule_info()["launches_per_timestep"] == 0
        with pytest.raises(capi.FdtdError, match=r"\(-5\).*H-field excitations: the two-launch schedule only"):
            e.run(1)
        e.close()
    # what the library refuses of the lists themselves; a refused set leaves the context as it was
    e = main_sim().build(hip_lib)
    hard = [a.copy() for a in lists.hard]
    hard[0][1], hard[1][1] = hard[0][0], hard[1][0]
    with pytest.raises(capi.FdtdError, match="a face given twice in the hard list"):
        e.set_excite(*hard, *lists.soft, lists.sigH)
    soft = [a.copy() for a in lists.soft]
    soft[0][5] = 21 * 14 * 12
    with pytest.raises(capi.FdtdError, match="soft face 5 out of range"):
        e.set_excite(*lists.hard, *soft, lists.sigH)
    soft[0][5], soft[1][5] = node(20, 3, 3), 2                   # a z-face needs a cell along x
    with pytest.raises(capi.FdtdError, match="soft face 5 does not exist"):
        e.set_excite(*lists.hard, *soft, lists.sigH)
    assert e.schedule_info() == before
    e.run(3)
    e.close()
    eo = capi.Engine(oracle_lib, 8, 8, 8, 1e-12)
    with pytest.raises(capi.FdtdError, match="no H-field excitations"):
        eo.set_excite(*lists.args())
    eo.close()


@pytest.mark.gpu
def test_decomposed_and_linked_contexts_are_refused():
    """In a child process (excite_slab_child.py says why): a slab of a decomposed grid and a linked context refuse the set."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "excite_slab_child.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    said = json.loads(r.stdout.strip().splitlines()[-1])
    want = r"\(-5\).*H-field excitations: single slab only \(world = 1, no p2p transport, no linked contexts\)"
    assert len(said) == 2 and all(m is not None and re.search(want, m) for m in said), said


# ---- hard E edges: no kernel of their own, every schedule --------------------------------------------------------------------------
HARD_GRID = (16, 12, 10)
HARD_LISTS = {"sparse": [("hard", 1, [0, 0, 2.0], [5, 5, 4], [5, 5, 7], dict(delay=1e-11, weight=[None, None, "1 + z/10"]))],
              # 80 z edges in one plane, more than the 32 a strip-plane scans: the dense source image
              "dense": [("hard", 1, [0, 0, 2.0], [3, 2, 4.5], [12, 9, 4.5], dict(delay=1e-11, weight=[None, None, "cos(x/5) + y/7"])),
                        ("soft", 0, [0, 1.0, 0], [4, 3.5, 7], [9, 3.5, 7])]}


def _hard_sim(which, nr_ts=100):
    from test_field_excitation_cpu import _sim
    s = _sim(None, HARD_LISTS[which], n=HARD_GRID)
    s.signal = s.signal[60:100].copy()              # a table of 40 samples: the run goes on past its end
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["sparse", "dense"])
def test_hard_e_under_all_three_schedules(hip_lib, oracle_lib, which):
    capi = pkg("_capi")
    nsteps = 100

    def run(lib, flags):
        s = _hard_sim(which)
        e = s.build(lib, flags=flags)
        h = s.excite_lists.hard_e
        pids = [e.add_probe(capi.KIND_V, [g], [c], [1.0]) for g, c in list(zip(h[0], h[1]))[:6]]
        info = e.schedule_info()
        seeded_fields(e, 8)
        for n in (1, 7, 92):
            e.run(n)
        out = (e.fields(), [e.get_probe(p) for p in pids], info, e.get_operator(), h)
        e.close()
        return out
    ref_f, ref_p, _, ref_op, h = run(oracle_lib, 0)
    assert h[0].size == (3 if which == "sparse" else 80) and not ref_op[0].reshape(3, -1)[h[1].astype(int), h[0]].any()
    d = int(h[3][0])
    assert 0 < d < 60
    sig = _hard_sim(which).signal
    table = np.concatenate([np.zeros(d, np.float32), sig, np.zeros(nsteps, np.float32)])[:nsteps]
    want = {"resident": 0, "one-launch": capi.FLAG_KERNEL_WAVEFRONT, "two-launch": capi.FLAG_KERNEL_DIRECT}
    for name, flags in want.items():
        f, p, info, op, _ = run(hip_lib, flags)
        if name == "resident":
            assert info["resident"], info
        elif name == "one-launch":
            assert info["launches_per_timestep"] == 1 and not info["resident"] and info["timesteps_per_launch_max"] > 1, info
        else:
            assert info["launches_per_timestep"] == 2 and not info["resident"], info
        for a, b in zip(op, ref_op):
            assert np.array_equal(a, b), name                 # the same overridden operator
        assert np.array_equal(f, ref_f), name
        for q, series in enumerate(p):                        # fp32(amp * sig[n - d]) inside the table, 0.0 before and after
            assert np.array_equal(series, (h[2][q] * table).astype(np.float64)), (name, q)
            assert series[d:d + 40].any() and not series[:d].any() and not series[d + 40:].any()
            assert np.array_equal(series, ref_p[q])


# ---- through the API ----------------------------------------------------------------------------------------------------------------
def _api_scene(lib, nr_ts=160):
    api = pkg("openems_api")
    fd = api.openEMS(NrTS=nr_ts, EndCriteria=0, lib=lib)
    fd.SetGaussExcite(12e9, 8e9)
    fd.SetBoundaryCond(["MUR"] * 6)
    csx = api.ContinuousStructure()
    fd.SetCSX(csx)
    mesh = csx.GetGrid()
    mesh.SetDeltaUnit(1e-3)
    mesh.AddLine("x", np.arange(20.0))
    mesh.AddLine("y", np.arange(18.0))
    mesh.AddLine("z", np.arange(16.0))
    csx.AddMaterial("sub", epsilon=2.2).AddBox([3, 3, 3], [16, 14, 6])
    fd.AddFieldExcitation("soft_e", 0, [1, 0, 0], [4, 4, 8], [10, 10, 8], weight=["cos(pi*(y-7)/12)", "0", "0"])
    fd.AddFieldExcitation("hard_e", 1, [0, 0, 1], [14, 5, 4], [14, 5, 8], weight=["0", "0", "1 + z/10"], delay=4e-12)
    fd.AddFieldExcitation("soft_h", 2, [0, 0, 1], [4, 4, 11], [10, 10, 11], weight=["0", "0", "x/(x^2+y^2) * (rho>6) * (rho<12)"], delay=2e-12)
    fd.AddFieldExcitation("hard_h", 3, [2, 0, 0], [12, 11.5, 6.5], [12, 12.5, 6.5], weight=["if(y > 12, 1, -1)", "0", "0"])
    csx.AddProbe("ut", 0).AddBox([6, 6, 7], [9, 8, 9])
    csx.AddProbe("it", 1, norm_dir="z").AddBox([6, 6, 10.5], [8, 8, 10.5])
    csx.AddProbe("et", 2).AddBox([14, 5, 5], [14, 5, 5])                 # on the hard E line
    csx.AddProbe("ht", 3).AddBox([12, 11, 6], [12, 11, 6])               # on a hard H face: sampled behind the excitation
    return fd, csx


@pytest.mark.gpu
def test_scene_through_the_api(hip_lib, oracle_lib, monkeypatch, tmp_path):
    from excite_cases import install
    fd, _ = _api_scene(hip_lib)
    fd.Run(str(tmp_path))
    install(monkeypatch)
    fo, _ = _api_scene(oracle_lib)
    fo.Run(None)
    assert fo.sim.restated.excite is not None
    assert [(q["kind"], q.get("edges", q.get("faces"))) for q in fd.stats.excitations] == [("soft E", 42), ("hard E", 4), ("soft H", 36), ("hard H", 2)]
    assert fd.stats.schedule["launches_per_timestep"] in (2, 3) and not fd.stats.schedule["resident"]
    assert np.array_equal(fd.sim.engine.fields(), fo.sim.engine.fields())
    for name in ("ut", "it", "et", "ht"):
        a, b = fd.GetProbe(name), fo.GetProbe(name)
        assert np.array_equal(a["t"], b["t"]) and np.abs(b["val"]).max() > 0
        err = np.abs(a["val"] - b["val"]).max() / np.abs(b["val"]).max()
        print(f"probe {name}: {err:.3e}")
        assert err <= 1e-12
    # the H-field probe on the hard face reads the excitation itself: amp * sigH[n] over the dual length
    l = fd.sim.excite_lists.hard_h
    q = int(np.nonzero(l[0] == fd.sim.grid.flat(12, 11, 6))[0][0])
    want = (l[2][q] * fd.sim.signal_h[:160]).astype(np.float64) / fd.sim.grid.dd[0][12]
    assert np.array_equal(fd.GetProbe("ht")["val"][0], want)
    rec = json.load(open(os.path.join(str(tmp_path), "fdtd_hip_run.json")))
    assert [q["name"] for q in rec["excitations"]] == ["soft_e", "hard_e", "soft_h", "hard_h"] and len(rec["probes"]) == 4
