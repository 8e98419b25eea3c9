"""Guards of the randomised parity run of all eight corrections in one context (tests/fuzz_parity.py --corrections) that need no GPU: the
fixed-seed batch of the -m gpu suite is accepted by the host layer and covers, together, what it was written to reach; the same seed
gives the same cases; the reference side of the first cases moves every state of every correction present; raw tables handed
to the restatement give the bits of the simulation's own."""
import collections

import numpy as np
import pytest

import corrections_overlap_cases as oc
import fuzz_parity
from conftest import pkg
from restatement import Restatement
from test_conformal_model_cpu import sphere_sim
from test_lorentz_model_cpu import TWO_PI, lorentz_cavity
from test_planewave_model_cpu import _placed

NAMES = fuzz_parity.CORRECTION_NAMES
WANTED = ({f"k_debye<{m},{k}>" for m in ("false", "true") for k in (4, 8)} | {f"k_lorentz<{m},{k}>" for m in ("false", "true") for k in (1, 2, 4)}
          | {f"{what} {x} mod 4 = {r}" for what in ("lorentz", "magnetic") for x in ("x0", "x1") for r in range(4)}
          | {f"nx mod 4 = {r}" for r in range(4)} | {f"{kind} element along {a}" for kind in ("series", "parallel") for a in "xyz"}
          | {f"drive {d}" for d in ("auto", "direct", "half")} | {f"face {k}" for k in ("PEC", "MUR", "CPML")}
          | {"sheet on a Debye face", "sheet on a Lorentz face", "element inside a Debye medium", "element inside a Lorentz medium",
             "element inside a magnetic material", "magnetic faces on a dispersive medium's face plane", "cut face next to a dispersive edge",
             "port loop through a magnetic material", "mu_r only", "sigma_m only", "mu_r and sigma_m", "box at x = 0", "box on the last column",
             "medium on a Mur face node, no apply pass", "medium on a Mur face node, apply pass", "set_field of a V component", "set_field of an I component",
             ">= 3 calls", "nf2ff none", "nf2ff dft", "nf2ff record", "raw operator", "graded", "uniform", "plane wave", "no plane wave",
             "oblique plane wave", "axis-aligned plane wave", "sphere", "tilted cylinder", "R, L and C in one element"}
          | {f"excited {what} face of component {c}" for what in ("soft", "hard") for c in "xyz"}
          | {f"{what} excitation delay {d}" for what in ("soft", "hard") for d in ("0", "inside the run", "past the run")}
          | {"one face with three soft entries", "excitations", "no excitations", "excitations with magnetic faces", "excitations with conformal faces",
             "excitations with a plane wave", "excitations under drive half", "excitations under drive direct", "excitations under drive auto",
             "excitations with Mur faces, apply pass", "excitations with Mur faces, no apply pass", "excitations with nf2ff record", "excitations with nf2ff dft",
             "set_field of an I component with excitations"})


def _edge_mask(d, shape):
    """bool [3][nz][ny][nx]: the dispersive edges (w != 0) of a DebyeEdges / LorentzEdges, None -> all False."""
    out = np.zeros((3,) + shape, bool)
    if d is not None:
        for c in range(3):
            if d.w[c].size:
                (i0, j0, k0), (i1, j1, k1) = d.lo[c], d.hi[c]
                out[c, k0:k1, j0:j1, i0:i1] = np.asarray(d.w[c]).reshape(k1 - k0, j1 - j0, i1 - i0) != 0
    return out


def _list_mask(comp, idx, shape):
    out = np.zeros((3,) + shape, bool)
    out.reshape(3, -1)[np.asarray(comp, np.int64), np.asarray(idx, np.int64)] = True
    return out


def _faces_next_to(faces, edges):
    """Is one of the faces (bool [3][nz][ny][nx]) spanned by one of the edges (same layout)?"""
    for n in range(3):
        for ce, off in pkg("conformal").face_edges(n):
            em = edges[ce]
            if off is not None:      # the edge at p + e_off, seen from p
                sh = np.zeros_like(em)
                src = [slice(None)] * 3
                dst = [slice(None)] * 3
                src[2 - off], dst[2 - off] = slice(1, None), slice(0, -1)
                sh[tuple(dst)] = em[tuple(src)]
                em = sh
            if np.any(faces[n] & em):
                return True
    return False


def features(case, sim):
    """What a drawn, accepted case reaches (the table of the randomised corrections run in docs/HISTORY.md)."""
    n = case["shape"]
    shape = (n[2], n[1], n[0])
    out = {f"nx mod 4 = {n[0] % 4}", f"nf2ff {case['nf2ff']}", "graded" if case["graded"] else "uniform", f"drive {case['drive']}"}
    out |= {f"face {k}" for k in case["kinds"]}
    if len(case["calls"]) >= 3:
        out.add(">= 3 calls")
    if not case["classes"]:
        out.add("raw operator")
    for st in case["sets"]:
        if st is not None:
            out.add("set_field of a V component" if st[0] == 0 else "set_field of an I component")
    deb, lor = _edge_mask(sim.debye, shape), _edge_mask(sim.lorentz, shape)
    if sim.debye is not None:
        out.add(f"k_debye<{'true' if len(sim.debye.media) > 1 else 'false'},{4 if sim.debye.K <= 4 else 8}>")
    if sim.lorentz is not None:
        K = sim.lorentz.K
        out.add(f"k_lorentz<{'true' if len(sim.lorentz.media) > 1 else 'false'},{1 if K <= 1 else 2 if K <= 2 else 4}>")
    for d in (sim.debye, sim.lorentz):
        for c in range(3 if d is not None else 0):
            if not d.w[c].size:
                continue
            for f in range(6):
                a = f // 2
                if case["kinds"][f] == "MUR" and c != a and (d.hi[c][a] == n[a] if f % 2 else d.lo[c][a] == 0):
                    out.add("medium on a Mur face node, " + ("apply pass" if case["env"].get("FDTD_MUR_APPLY_PASS") == "1" else "no apply pass"))
    mag = np.zeros((3,) + shape, bool)
    if sim.magnetic is not None:
        mag = sim.magnetic.full_classes(shape) != 0
        if _faces_next_to(mag, deb | lor):
            out.add("magnetic faces on a dispersive medium's face plane")
        p = sim.vox.ports[0]
        if np.any(mag.reshape(3, -1)[np.asarray(p.i_comp, np.int64), np.asarray(p.i_idx, np.int64)]):
            out.add("port loop through a magnetic material")
    for what, d in (("lorentz", sim.lorentz), ("magnetic", sim.magnetic)):
        for c in range(3 if d is not None else 0):
            if d.hi[c][0] <= d.lo[c][0]:
                continue
            out |= {f"{what} x0 mod 4 = {d.lo[c][0] % 4}", f"{what} x1 mod 4 = {d.hi[c][0] % 4}"}
            if d.lo[c][0] == 0:
                out.add("box at x = 0")
            last = (n[0] - 1 if c == 0 else n[0]) if what == "lorentz" else (n[0] if c == 0 else n[0] - 1)      # edges / faces along x
            if d.hi[c][0] == last:
                out.add("box on the last column")
    if sim.sheets is not None:
        sh = _list_mask(sim.sheets.comp, sim.sheets.idx, shape)
        if np.any(sh & deb):
            out.add("sheet on a Debye face")
        if np.any(sh & lor):
            out.add("sheet on a Lorentz face")
    if sim.element_stepped.size:
        st = sim.element_stepped
        el = _list_mask(sim.elements.comp[st], sim.elements.idx[st], shape)
        if np.any(el & deb):
            out.add("element inside a Debye medium")
        if np.any(el & lor):
            out.add("element inside a Lorentz medium")
        if _faces_next_to(mag, el):
            out.add("element inside a magnetic material")
        for e in case["elements"]:
            out.add(f"{e['kind']} element along {'xyz'[e['dir']]}")
            if None not in (e["R"], e["L"], e["C"]):
                out.add("R, L and C in one element")
    for m in case["magnetic"]:
        out.add("mu_r only" if m["sigma_m"] == 0 else "sigma_m only" if m["mu_r"] == 1 else "mu_r and sigma_m")
    if sim.conformal is not None:
        out.add("sphere" if case["metal"]["shape"] == "sphere" else "tilted cylinder")
        cut = _list_mask(sim.conformal.comp, sim.conformal.idx, shape)
        if _faces_next_to(cut, deb | lor):
            out.add("cut face next to a dispersive edge")
        assert not np.any(cut & mag)
    if sim.plane_wave is not None:
        out |= {"plane wave", "axis-aligned plane wave" if sorted(map(abs, case["planewave"]["dir"]))[1] == 0 else "oblique plane wave"}
    else:
        out.add("no plane wave")
    if sim.excite_h_args is None:
        out.add("no excitations")
    else:
        total = sum(case["calls"])
        hard, soft = sim.excite_h_args[0:4], sim.excite_h_args[4:8]
        assert hard[0].size == sum(x["type"] == 3 for x in case["excite"]) and soft[0].size == sum(x["type"] == 2 for x in case["excite"])
        for what, l in (("hard", hard), ("soft", soft)):
            for c, d in zip(l[1].tolist(), l[3].tolist()):
                out |= {f"excited {what} face of component {'xyz'[c]}",
                        f"{what} excitation delay " + ("0" if d == 0 else "inside the run" if d < total else "past the run")}
        if np.unique(soft[0] * 3 + soft[1], return_counts=True)[1].max() == 3:
            out.add("one face with three soft entries")
        out |= {"excitations", f"excitations under drive {case['drive']}"}
        if sim.magnetic is not None:
            out.add("excitations with magnetic faces")
        if sim.conformal is not None:
            out.add("excitations with conformal faces")
        if sim.plane_wave is not None:
            out.add("excitations with a plane wave")
        if "MUR" in case["kinds"]:
            out.add("excitations with Mur faces, " + ("apply pass" if case["env"].get("FDTD_MUR_APPLY_PASS") == "1" else "no apply pass"))
        if case["nf2ff"] != "none":
            out.add(f"excitations with nf2ff {case['nf2ff']}")
        if any(st is not None and st[0] == 1 for st in case["sets"]):
            out.add("set_field of an I component with excitations")
    return out


def _excited_faces_are_free(sim):
    """What field_excitation.check_placement demands of the excited faces, asked again here of the lists the simulation holds."""
    n = sim.grid.shape
    key = np.concatenate([sim.excite_h_args[0] * 3 + sim.excite_h_args[1], sim.excite_h_args[4] * 3 + sim.excite_h_args[5]]).astype(np.int64)
    g, c = key // 3, key % 3
    pos = np.stack([g % n[0], g // n[0] % n[1], g // (n[0] * n[1])])
    for a in range(3):
        assert np.all(pos[a][c != a] < n[a] - 1) and np.all((pos[a][c == a] > 0) & (pos[a][c == a] < n[a] - 1))
    if sim.magnetic is not None:
        assert not sim.magnetic.full_classes(n[::-1]).reshape(3, -1)[c, g].any()
    if sim.conformal is not None:
        assert not np.isin(key, np.asarray(sim.conformal.idx, np.int64) * 3 + np.asarray(sim.conformal.comp, np.int64)).any()
    if sim.plane_wave is not None:
        pw = np.array([sim.grid.flat(i, j, k) * 3 + f for f, i, j, k, *_ in pkg("planewave").terms(sim.grid, sim.plane_wave, 1)], np.int64)
        assert pw.size and not np.isin(key, pw).any()
    for r in ([] if sim.nf2ff_box is None else sim.nf2ff_box.requests):      # (no NF2FF box samples one: fuzz_parity.draw_excitations says why)
        on = (c == r.comp) & np.all([(pos[a] >= r.lo[a]) & (pos[a] <= r.hi[a]) for a in range(3)], axis=0)
        assert r.kind == 0 or not on.any()


def test_fixed_seed_batch_is_accepted_and_covers_what_it_is_for():
    ncases, seed = fuzz_parity.CORRECTIONS_BATCH
    rng = np.random.default_rng(seed)
    bare = np.random.default_rng(seed)
    seen, accepted, refused, count, how_many = set(), 0, [], collections.Counter(), []
    for q in range(ncases):
        case = fuzz_parity.draw_corrections_case(rng, excite=(seed, q))
        # the excitations come from a generator of their own: without them the case is what draw_corrections_case(rng) draws — the
        # parent commit's case (test_batch_without_excitations_is_the_recorded_one holds that to the record)
        assert {k: v for k, v in case.items() if k != "excite"} == {k: v for k, v in fuzz_parity.draw_corrections_case(bare).items() if k != "excite"}
        nx, ny, nz = case["shape"]
        assert 14 <= nx <= 70 and 12 <= ny <= 36 and 12 <= nz <= 28 and 2 <= case["cells"] <= 6
        assert 1 <= len(case["calls"]) <= 5 and all(1 <= k <= 60 for k in case["calls"]) and sum(case["calls"]) <= 150
        assert len(case["sets"]) == len(case["calls"]) - 1
        assert len(case["debye"]) <= 3 and len(case["lorentz"]) <= 2 and len(case["sheets"]) <= 3 and len(case["elements"]) <= 4 and len(case["magnetic"]) <= 2
        assert all(1 <= e["hi"][e["dir"]] - e["lo"][e["dir"]] <= 5 for e in case["elements"])
        assert eval(repr(case)) == case                      # printable, and reproducible from what the log prints
        try:
            sim = fuzz_parity.corrections_case_sim(case)
        except ValueError as exc:
            refused.append((q, str(exc)))
            continue
        accepted += 1
        have = fuzz_parity.corrections_present(sim)
        assert len(have) >= 3, (q, have, case)
        count.update(have)
        how_many.append(len(have))
        seen |= features(case, sim)
        assert ("excite" in have) == (case["excite"] is not None)
        if case["excite"] is not None:
            assert 7 <= len(case["excite"]) <= 14
            _excited_faces_are_free(sim)
    print(f"{accepted} of {ncases} accepted; refused: {refused}; cases per correction: {dict(count)}; corrections per case: {sorted(how_many)}")
    assert 6 * accepted >= 5 * ncases, refused
    assert accepted == ncases == 24 and refused == []      # this batch: every case, with its excitations, is accepted by the host layer
    assert all(count[name] >= 4 for name in NAMES), count
    assert how_many.count(8) >= 8 and 3 * sum(h >= 5 for h in how_many) >= accepted, how_many
    assert not WANTED - seen, sorted(WANTED - seen)


def test_same_seed_same_cases():
    first = fuzz_parity.draw_corrections_case(np.random.default_rng(5))
    rng = np.random.default_rng(5)
    assert fuzz_parity.draw_corrections_case(rng) == first and fuzz_parity.draw_corrections_case(rng) != first
    a, b = fuzz_parity.corrections_batch(6, 5), fuzz_parity.corrections_batch(6, 5)
    assert a == b and a[0] == dict(first, excite=a[0]["excite"]) and any(c["excite"] is not None for c in a)


def test_batch_without_excitations_is_the_recorded_one():
    """The descriptions of the fixed-seed batch with the excitation part removed, against tests/golden/corrections_batch_seed2.json: the
    repr() of each case as the commit before the excitations drew it (written there by that commit's draw_corrections_case)."""
    import json
    import os
    from conftest import ROOT
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "corrections_batch_seed2.json")))
    got = [repr({k: v for k, v in c.items() if k != "excite"}) for c in fuzz_parity.corrections_batch()]
    assert len(want) == 24 and got == want


def test_reference_side_of_the_first_cases_moves_everywhere(oracle_lib):
    """The first cases of the batch stepped on the restatement alone: finite, non-zero, every state of every correction present
    off zero, the plane wave's lists changing V and I on their elements."""
    ran, have, acted = 0, set(), 0
    for q, case in enumerate(fuzz_parity.corrections_batch()[:8]):
        try:
            problems, _ = fuzz_parity.run_corrections_case(case, None, oracle_lib)
        except ValueError:
            continue
        assert problems == [], (q, case, problems)
        have |= fuzz_parity.corrections_present(fuzz_parity.corrections_case_sim(case))
        ran += 1
        if case["excite"] is not None:      # the set acts: the same case without it ends with other fields
            fields = []
            for c in (case, dict(case, excite=None)):
                ref = fuzz_parity.corrections_reference(fuzz_parity.corrections_case_sim(c), oracle_lib, seed=case["seed"])
                ref.run(case["calls"][0])
                fields.append(ref.e.fields())
            assert not np.array_equal(fields[0][1], fields[1][1]), q
            acted += 1
    assert ran >= 7 and have == set(NAMES) and acted >= 4, (ran, have, acted)


def test_composed_with_conformal_faces_alone_is_restated_conformal(oracle_lib):
    """The conformal faces handed over as the raw tables of fdtd_conformal_set against the simulation's own, the fuzz harness's way."""
    nsteps = 40
    sim = sphere_sim(nr_ts=nsteps, tilted_disc=True)
    a = Restatement(sim, oracle_lib, seed=5, tables={"conformal": sim.conformal_tables()})
    b = fuzz_parity.corrections_reference(sphere_sim(nr_ts=nsteps, tilted_disc=True), oracle_lib, seed=5)
    assert b.conformal is not None and b.pw_e is None and b.lorentz is None and b.magnetic is None and b.debye is None
    g = a.sim.grid
    probe = (np.array([g.flat(7, 10, 5), g.flat(12, 5, 4)], np.int64), np.array([2, 0], np.int8), np.array([1.0, -2.0], np.float32))
    pa, pb = a.add_probe(1, *probe), b.add_probe(1, *probe)
    for r in (a, b):
        r.run(nsteps // 2)
        r.set_field(1, 2, np.full(r.e.local_shape, 1e-4, np.float32))
        r.run(nsteps // 2)
    assert a.conformal.iprev.size > 100 and np.all(a.conformal.iprev != 0)
    assert np.array_equal(a.e.fields(), b.e.fields()) and np.array_equal(a.conformal.iprev, b.conformal.iprev)
    sa, sb = a.get_probe(pa), b.get_probe(pb)
    assert sa.size == nsteps and np.abs(sa).max() > 0 and np.array_equal(sa, sb)


def test_composed_with_lorentz_media_alone_is_restated_lorentz(oracle_lib):
    """The Lorentz media handed over as the raw tables of fdtd_lorentz_set against the simulation's own, the fuzz harness's way."""
    nsteps = 40
    mk = lambda: lorentz_cavity(lambda s: s.add_lorentz_material("block", 2.0, 0.0, TWO_PI * np.array([8e9, 6e9]), TWO_PI * np.array([0.0, 12e9]),
                                                                 [4e9, 1e9]).add_box([4, 4, 3], [9, 8, 8]), nr_ts=nsteps)
    sim = mk()
    a = Restatement(sim, oracle_lib, seed=4, tables={"lorentz": sim.lorentz_tables()})
    b = fuzz_parity.corrections_reference(mk(), oracle_lib, seed=4)
    assert list(b.parts) == ["lorentz"]
    a.run(nsteps)
    b.run(nsteps)
    assert np.abs(a.lorentz.x[0]).max() > 0 and np.array_equal(a.e.fields(), b.e.fields())
    for c in range(3):
        assert np.array_equal(a.lorentz.x[c], b.lorentz.x[c]) and np.array_equal(a.lorentz.vprev[c], b.lorentz.vprev[c])
    assert fuzz_parity.corrections_reference_problems(b) == []


def test_composed_with_a_plane_wave_and_conformal_faces_is_the_pair_it_was(oracle_lib):
    """A plane wave and conformal faces: the restatement test_planewave_model_cpu's plugin tests install against the fuzz harness's, whose
    hooks watch the plane wave's lists."""
    nsteps = 60
    mk = lambda: _placed(lambda s: s.add_metal("ball").add_sphere((12.3, 11.8, 12.1), 2.4), conformal=True, nr_ts=nsteps)
    a = Restatement(mk(), oracle_lib)
    b = fuzz_parity.corrections_reference(mk(), oracle_lib)
    assert b.pw_e is not None and b.pw_h is not None and b.conformal is not None
    a.run(nsteps)
    b.run(nsteps)
    assert all(b.pw_changed.values()) and np.abs(a.e.fields()).max() > 0 and np.all(a.conformal.iprev != 0)
    assert np.array_equal(a.e.fields(), b.e.fields()) and np.array_equal(a.conformal.iprev, b.conformal.iprev)


@pytest.mark.parametrize("mur", [False, True], ids=["pec", "one-mur-face"])
def test_overlap_reference_tells_every_correction_apart(oracle_lib, mur):
    """The hand tables of corrections_overlap_cases.py on the reference alone: the lists do overlap where the case says, the run is
    finite and every state moves, the V-probes kept here are the oracle's own (sampled in front of every E-side correction), the
    I-probes are not (sampled behind every H-side one), and dropping any one of the ten lists (the plane wave's two and the
    excitations' two counted singly) changes the values the GPU test compares on the shared edge or face itself."""
    ref = oc.reference(oracle_lib, mur)
    T = ref.T
    key = lambda el: (int(el[0]), oc.flat(*el[1:]))
    listed = lambda idx, comp: set(zip(map(int, comp), map(int, idx)))
    for edge, box in ((oc.A, "debye"), (oc.B, "lorentz")):
        assert key(edge) in listed(*T["sheets"][:2]) & listed(*T["elements"][:2]) & listed(*T["pw"].E[:2])
        c, i, j, k = edge
        lo, w = T[box][3][c], T[box][5][c]
        assert w[k - lo[2], j - lo[1], i - lo[0]] != 0 and ref.e.get_operator()[1][c][k, j, i] != 0
    c, i, j, k = oc.F
    lo = T["magnetic"][2][c]
    assert T["magnetic"][4][c][k - lo[2], j - lo[1], i - lo[0]] != 0
    assert key(oc.F) in listed(T["conformal"][1], T["conformal"][0]) & listed(*T["pw"].H[:2])
    x = T["excite"]
    assert list(zip(x[5].tolist(), x[4].tolist())).count(key(oc.F)) == 2 and key(oc.F) not in listed(*x[:2])
    c, i, j, k = oc.G
    assert T["magnetic"][4][c][k - lo[2], j - lo[1], i - lo[0]] != 0 and key(oc.G) in listed(*T["pw"].H[:2]) & listed(*x[:2])
    assert key(oc.G) not in listed(x[4], x[5]) and key(oc.G) not in listed(T["conformal"][1], T["conformal"][0])
    assert np.isfinite(ref.fields).all() and all(np.abs(a).max() > 0 for name in ref.state for a in ref.state[name])
    for pid, s in zip(ref.own_v, ref.v_series):
        assert np.array_equal(ref.e.get_probe(pid)[:oc.STEPS], np.array(s)) and np.abs(s).max() > 0
    at = lambda r, kind, el: r.fields[kind][el[0]][el[3], el[2], el[1]]
    for name in oc.NAMES:
        d = oc.reference(oracle_lib, mur, name)
        assert not np.array_equal(d.fields, ref.fields), name
        if name in ("magnetic", "conformal", "pw_h", "excite_soft"):
            assert at(d, 1, oc.F) != at(ref, 1, oc.F) and not np.array_equal(d.i_series[0], ref.i_series[0]), name
            assert np.abs(d.i_acc[0] - ref.i_acc[0]).max() > 1e-6 * np.abs(ref.i_acc[0]).max(), name
        elif name == "excite_hard":
            assert not np.array_equal(d.i_series[2], ref.i_series[2])
            assert np.abs(d.i_acc[1] - ref.i_acc[1]).max() > 1e-6 * np.abs(ref.i_acc[1]).max()
            assert not np.array_equal(d.state["magnetic"][1], ref.state["magnetic"][1])      # i_prev of G restarts from another current
        else:
            shared = [oc.A, oc.B] if name in ("sheets", "elements", "pw_e") else [oc.A] if name == "debye" else [oc.B]
            for q, el in enumerate([oc.A, oc.B]):
                if el in shared:
                    assert at(d, 0, el) != at(ref, 0, el), (name, el)
                    assert not np.array_equal(d.v_series[q], ref.v_series[q]), (name, el)


def _hard_series(T, amp_delay=oc.HARD_G):
    """float32(amp * sigH[n - delay]), 0.0 outside the table: what a hard face holds, per timestep."""
    amp, d = amp_delay
    sig = np.concatenate([np.zeros(d, np.float32), T["excite"][8], np.zeros(oc.STEPS, np.float32)])[:oc.STEPS]
    return (np.float32(amp) * sig).astype(np.float64)


@pytest.mark.parametrize("mur", [False, True], ids=["pec", "one-mur-face"])
def test_overlap_reference_tells_the_excitations_place_in_the_order(oracle_lib, monkeypatch, mur):
    """The reference alone: the hard face G holds amp * sigH[n - delay] whatever the magnetic faces and the plane wave did there; the
    two soft entries on F in the other list order give other bits; and with the excitations in front of the plane wave's face list
    instead of behind it (restatement.H_SIDE swapped) both faces read other bits — F by float32 association ((I + pw) + t against
    (I + t) + pw), G because the plane wave then adds to the hard value."""
    import restatement
    ref = oc.reference(oracle_lib, mur)
    T = ref.T
    want = _hard_series(T)
    assert np.array_equal(np.array(ref.i_series[2]), want) and np.count_nonzero(want) == oc.NSIG_H and not want[:oc.HARD_G[1]].any() and not want[42:].any()
    at = lambda r, el: r.fields[1][el[0]][el[3], el[2], el[1]]
    # the soft list reversed: the same entries per face, F's two in the other order
    x = T["excite"]
    rev = dict(T, excite=x[:4] + tuple(a[::-1].copy() for a in x[4:8]) + x[8:])
    r = oc.Ordered(oracle_lib, rev, mur).run()
    assert not np.array_equal(r.i_series[0], ref.i_series[0]) and at(r, oc.F) != at(ref, oc.F)
    assert np.array_equal(np.array(r.i_series[2]), want)
    # plane wave (face list) <-> excitations
    assert restatement.H_SIDE[-2:] == ("pw_h", "excite")
    monkeypatch.setattr(restatement, "H_SIDE", restatement.H_SIDE[:-2] + ("excite", "pw_h"))
    sw = oc.Ordered(oracle_lib, T, mur).run()
    monkeypatch.undo()
    assert not np.array_equal(sw.i_series[0], ref.i_series[0]) and at(sw, oc.F) != at(ref, oc.F)
    got = np.array(sw.i_series[2])
    assert not np.array_equal(got, want) and np.count_nonzero(got != want) >= 20      # the plane wave's term on top of the hard value
    assert np.abs(sw.i_acc[1] - ref.i_acc[1]).max() > 1e-6 * np.abs(ref.i_acc[1]).max()
    assert not np.array_equal(sw.state["magnetic"][1], ref.state["magnetic"][1])
