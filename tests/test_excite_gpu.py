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
import excite_cases as xc
from excite_cases import ExciteRestatement, HLists, main_lists, main_sim, node
from restatement import Restatement
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


# ---- list shapes of fdtd_excite_set and k_excite through the raw C ABI (excite_cases.py; CPU side: test_field_excitation_cpu.py) -------
CALLS = (1, 7, 72)       # 80 timesteps


def _parity(hip_lib, oracle_lib, lists, *, n=xc.MAIN_GRID, seed=4, use_classes=True, before=None):
    """The HIP context with `lists` stepped in CALLS against the restatement: all six fields bit for bit.  -> (fields, engine)."""
    ref = Restatement(main_sim(n=n, use_classes=use_classes), oracle_lib, seed=seed, tables={"excite": lists.args()})
    ref.run(sum(CALLS))
    e = main_sim(n=n, use_classes=use_classes).build(hip_lib)
    if before is not None:
        before(e)
    e.set_excite(*lists.args())
    seeded_fields(e, seed)
    assert e.schedule_info()["launches_per_timestep"] == 2
    for k in CALLS:
        e.run(k)
    f, fo = e.fields(), ref.e.fields()
    assert np.isfinite(fo).all() and np.array_equal(f, fo), f"fields differ at {np.count_nonzero(f != fo)} entries, first {tuple(np.argwhere(f != fo)[0])}"
    return f, e


_BARE = {}


def _bare(hip_lib, n=xc.MAIN_GRID, seed=4):
    """The same seeded run without a set, once per grid."""
    if n not in _BARE:
        e = main_sim(n=n).build(hip_lib)
        seeded_fields(e, seed)
        e.run(sum(CALLS))
        _BARE[n] = e.fields()
        e.close()
    return _BARE[n]


@pytest.mark.gpu
@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
@pytest.mark.parametrize("count", xc.PLANE_COUNTS)
def test_distinct_faces_around_one_block(hip_lib, oracle_lib, count, hard):
    """1, 255, 256 and 257 distinct faces on one node plane (one thread per face, blocks of 256), soft entries only and with a hard
    entry on every face."""
    lists = xc.plane_lists(count, hard)
    assert lists.faces()[0].size == count and lists.hard[0].size == (count if hard else 0) and lists.soft[0].size == count
    f, e = _parity(hip_lib, oracle_lib, lists)
    e.close()
    bare = _bare(hip_lib)
    fi, fc = lists.faces()
    for g, c in ((fi[0], fc[0]), (fi[-1], fc[-1])):         # the first and the last face of the grouped set did get their entries
        assert f[1, c].reshape(-1)[g] != bare[1, c].reshape(-1)[g]


@pytest.mark.gpu
def test_one_face_with_300_soft_entries(hip_lib, oracle_lib):
    """One thread walks 300 entries in list order (test_field_excitation_cpu: the reversed list gives other bits on the reference)."""
    lists = xc.many_entries_lists()
    assert lists.faces()[0].size == 1 and lists.soft[0].size == 300
    _, e = _parity(hip_lib, oracle_lib, lists)
    e.close()


@pytest.mark.gpu
def test_scattered_entries_of_a_face_are_grouped_in_list_order(hip_lib, oracle_lib):
    """40 faces x 3 entries, listed face by face and entry by entry: the same grouped set, the same bits, those of the restatement."""
    fields = []
    for order in ("face-major", "entry-major"):
        f, e = _parity(hip_lib, oracle_lib, xc.forty_faces_lists(order))
        fields.append(f)
        e.close()
    assert np.array_equal(fields[0].view(np.uint32), fields[1].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
@pytest.mark.parametrize("nx", xc.NX_EXTREMES)
def test_faces_at_the_grid_extremes(hip_lib, oracle_lib, nx, hard):
    """The origin and the last existing face of every component along every axis, for every nx mod 4; the node one step further along a
    transverse axis is a node of the grid without that face: refused by name, and the context keeps the set it had."""
    capi = pkg("_capi")
    n = (nx,) + xc.MAIN_GRID[1:]
    lists = xc.extreme_lists(nx, hard)
    f, e = _parity(hip_lib, oracle_lib, lists, n=n)
    bare = _bare(hip_lib, n)
    faces = xc.extreme_faces(n)
    differ = [f[1, c, k, j, i] != bare[1, c, k, j, i] for c, i, j, k in faces]
    assert all(differ), [fc for fc, d in zip(faces, differ) if not d]
    e.close()
    e = main_sim(n=n).build(hip_lib)
    col = lambda fc, amp: ([node(*fc[1:], n)], [fc[0]], [amp], [0])
    none = ([], [], [], [])
    refused = 0
    for fc in faces:
        for b in xc.beyond(fc, n):
            for args, what in (((*col(b, 1.0), *none), "hard"), ((*none, *col(b, 1.0)), "soft")):
                with pytest.raises(capi.FdtdError, match=f"{what} face 0 does not exist"):
                    e.set_excite(*args, lists.sigH)
                refused += 1
    assert refused == 2 * 12
    e.close()


@pytest.mark.gpu
def test_main_case_on_the_raw_operator_form(hip_lib, oracle_lib):
    lists = main_lists()
    form = []
    _, e = _parity(hip_lib, oracle_lib, lists, use_classes=False, before=lambda q: form.append(q.operator_form()))
    e.close()
    e = main_sim().build(hip_lib)
    assert form[0] != e.operator_form(), form          # (the two forms do differ: the main case above runs on class bytes)
    e.close()


@pytest.mark.gpu
def test_a_second_set_replaces_the_first(hip_lib, oracle_lib):
    """fdtd_excite_set twice before the first timestep: the run is that of a context that only ever had the second set; after a
    timestep the call is refused and the context steps on unchanged."""
    capi = pkg("_capi")
    first, second = main_lists(), xc.plane_lists(257, True)
    assert first.faces()[0].size != second.faces()[0].size
    f, e = _parity(hip_lib, oracle_lib, second, before=lambda q: q.set_excite(*first.args()))
    e.close()
    once, e = _parity(hip_lib, oracle_lib, second)
    e.close()
    assert np.array_equal(f.view(np.uint32), once.view(np.uint32))
    e = main_sim().build(hip_lib)
    e.set_excite(*second.args())
    seeded_fields(e, 4)
    e.run(CALLS[0])
    with pytest.raises(capi.FdtdError, match="before the first timestep"):
        e.set_excite(*first.args())
    with pytest.raises(capi.FdtdError, match="before the first timestep"):
        e.set_excite(*[a[:0] for a in first.hard], *[a[:0] for a in first.soft], None)      # (removing it is refused too)
    for k in CALLS[1:]:
        e.run(k)
    assert np.array_equal(e.fields().view(np.uint32), once.view(np.uint32))
    e.close()


@pytest.mark.gpu
def test_hard_faces_held_at_zero(hip_lib, oracle_lib):
    """A hard entry with amp = +0.0 and one whose delay lies past the run, read with get_field after every timestep.  The second holds
    +0.0 bits throughout (0.7f * 0.0f).  The first holds a zero in every timestep: +0.0 outside the table and, inside it, 0.0f * s —
    the statement I = amp * s of the header in IEEE arithmetic, a zero with the sign of s; the bits are asked exactly so."""
    nsteps = sum(CALLS)
    lists = xc.held_lists(nsteps)
    ref = Restatement(main_sim(), oracle_lib, seed=4, tables={"excite": lists.args()})
    e = main_sim().build(hip_lib)
    e.set_excite(*lists.args())
    seeded_fields(e, 4)
    (g0, g1), (c0, c1), d0 = lists.hard[0], lists.hard[1], int(lists.hard[3][0])
    assert e.get_field(1, int(c0)).reshape(-1)[g0] != 0 and e.get_field(1, int(c1)).reshape(-1)[g1] != 0      # (seeded: not zero to begin with)
    signs = set()
    for n in range(nsteps):
        e.run(1)
        ref.step()
        a0, a1 = e.get_field(1, int(c0)).reshape(-1)[g0], e.get_field(1, int(c1)).reshape(-1)[g1]
        s = lists.sigH[n - d0] if 0 <= n - d0 < lists.sigH.size else np.float32(0.0)
        want = np.float32(0.0) * s
        assert a1.view(np.uint32) == 0, (n, a1)
        assert a0 == 0 and a0.view(np.uint32) == want.view(np.uint32), (n, a0, s)
        signs.add(int(a0.view(np.uint32) >> 31))
    assert signs == {0, 1}                        # (the table has samples of both signs under the first face)
    assert np.array_equal(e.fields(), ref.e.fields())
    e.close()


@pytest.mark.gpu
def test_set_field_of_the_currents_between_two_calls(hip_lib, oracle_lib):
    """fdtd_set_field(FDTD_KIND_I) of all three components between two calls: the correction keeps no state, so the run is the
    restatement's given the same fields at the same timestep."""
    lists = main_lists()
    ref = Restatement(main_sim(), oracle_lib, seed=4, tables={"excite": lists.args()})
    e = main_sim().build(hip_lib)
    e.set_excite(*lists.args())
    seeded_fields(e, 4)
    rng = np.random.default_rng(23)
    for q, k in enumerate((8, 30, 42)):
        if q:
            for c in range(3):
                a = (1e-3 * rng.standard_normal(e.local_shape)).astype(np.float32)
                ref.set_field(1, c, a)
                e.set_field(1, c, a)
        ref.run(k)
        e.run(k)
        assert np.array_equal(e.fields(), ref.e.fields()), q
    e.close()


# ---- what samples I behind the excitation: I-probe, I-DFT box, recorder face (excite_cases.observer_scene) ---------------------------
def _observers(hip_lib, kind, mode, drive, late_at=None):
    """The observer scene on the HIP library: `mode` "dft" or "record", `drive` "auto", "direct" or "half", in calls of 8 and 72
    timesteps; late_at = 8: the second I-probe is added between the two calls.  -> (engine, probe id, box id, late probe id)."""
    capi = pkg("_capi")
    sc, sim = xc.observer_scene(kind), xc.observer_sim(kind)
    e = sim.build(hip_lib, flags=capi.FLAG_KERNEL_DIRECT if drive == "direct" else 0)
    e.set_excite(*sc["lists"].args())
    if sc["source"] is not None:
        e.add_source(*sc["source"])
    tw_v, tw_i, _ = xc.observer_twiddles(sim.dt)
    if mode == "dft":
        e.set_dft(xc.OBS_EVERY, tw_v, tw_i)
    else:
        e.set_recorder(xc.OBS_EVERY, tw_i.shape[0])
    pid = e.add_probe(capi.KIND_I, *sc["probe"])
    bid = e.add_dft_box(capi.KIND_I, *sc["box"])
    seeded_fields(e, 5)
    late = None
    for q, k in enumerate((8, xc.OBS_STEPS - 8)):
        if q and late_at is not None:
            late = e.add_probe(capi.KIND_I, *sc["late"])
        if drive == "half":
            for _ in range(k):
                e.half_step(capi.PHASE_E)
                e.half_step(capi.PHASE_H)
        else:
            e.run(k)
    return e, pid, bid, late


def _check_observers(e, ref, mode, pid, bid, late, tag):
    tw_i, ident = xc.observer_twiddles(ref.sim.dt)[1:]
    assert np.array_equal(e.fields(), ref.fields), tag
    assert np.array_equal(e.get_probe(pid)[:xc.OBS_STEPS], ref.series), (tag, "I-probe")              # bit-equal, as the suite asks of I-probes
    if late is not None:         # 0.0 before its first timestep, the restated series from there on
        got = e.get_probe(late)[:xc.OBS_STEPS]
        assert not got[:ref.late_at].any() and np.array_equal(got[ref.late_at:], ref.late), (tag, "late I-probe")
    scale = np.abs(ref.acc).max()
    if mode == "dft":            # 1e-12 of the largest entry, as the suite asks of I-DFT boxes
        box = e.get_dft_box(bid)[0]
        assert box.shape == ref.acc.shape and np.abs(box - ref.acc).max() <= 1e-12 * scale, (tag, np.abs(box - ref.acc).max() / scale)
    else:                        # the record itself (the identity table: exact), and its transform
        rec = e.rec_transform(bid, ident)[0]
        ns = ref.rec.shape[0]
        assert not rec.imag.any() and np.array_equal(rec.real[:ns], ref.rec.astype(np.float64)) and not rec.real[ns:].any(), (tag, "record")
        box = e.rec_transform(bid, tw_i)[0]
        assert box.shape == ref.acc.shape and np.abs(box - ref.acc).max() <= 1e-12 * scale, (tag, np.abs(box - ref.acc).max() / scale)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["pec", "mur", "mur-near"])
def test_observers_sample_the_current_behind_the_excitation(hip_lib, oracle_lib, monkeypatch, kind):
    """An I-probe, an I-DFT box (dft mode) and a recorder face (record mode), each over a hard and a soft H face: fdtd_run under AUTO
    and DIRECT and fdtd_half_step pairs, in two calls; with six Mur faces under both Mur schedules (two launches, three with the apply
    pass); "mur-near": an excited face one node from a Mur face plane, probes sampled by k_post.  The second I-probe is added between
    the two calls."""
    ref = xc.observed(oracle_lib, kind)
    assert np.abs(ref.series).max() > 0 and np.abs(ref.late).max() > 0 and ref.late.size == xc.OBS_STEPS - ref.late_at
    runs = [(None, drive) for drive in ("auto", "direct", "half")] + ([("1", "auto"), ("1", "direct")] if kind != "pec" else [])
    launches = set()
    for apply_pass, drive in runs:
        if apply_pass is None:
            monkeypatch.delenv("FDTD_MUR_APPLY_PASS", raising=False)
        else:
            monkeypatch.setenv("FDTD_MUR_APPLY_PASS", apply_pass)
        for mode in ("dft", "record"):
            tag = f"{kind}, {drive}, apply pass {apply_pass}, {mode}"
            e, pid, bid, late = _observers(hip_lib, kind, mode, drive, late_at=ref.late_at)
            info = e.schedule_info()
            assert not info["resident"] and info["launches_per_timestep"] >= 2, (tag, info)
            launches.add(info["launches_per_timestep"])
            _check_observers(e, ref, mode, pid, bid, late, tag)
            e.close()
    # fused sources and probes: two launches, three with the Mur apply pass; "mur-near": more — the sources and the probes (k_post) and
    # the Mur passes are launches of their own
    assert launches == {2} if kind == "pec" else launches == {2, 3} if kind == "mur" else min(launches) > 3, launches


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
