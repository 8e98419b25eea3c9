"""Soft sources and probes on the oracle alone (tests/source_probe_cases.py): what the oracle does with a source list and a probe is
restated in numpy, so that the reference of tests/test_sources_probes_gpu.py is itself pinned; every source call and every probe of
every case is live; and every directed case sits on the side of each kernel threshold it was built for (integer arithmetic restated
from csrc/, so a case that drifts is caught without a GPU).  For the slab cases of tests/test_slab_sources_probes_gpu.py: where their
lists sit relative to the cuts, what the drawn slab batch covers, and the oracle stepped as those slabs against the oracle as one."""
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
    e = spc.raw_engine(lib, (case.scene, case.shape), case.boundary, 0, case.cap, cpml_cells=case.cpml_cells,
                       hard=None if case.hard is None else case.hard[:2])
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


# ---- z-slabs: where the directed slab cases sit, what the drawn slab batch covers, and the oracle cut into slabs -----------------------
def test_slab_cases_sit_on_the_cut():
    """Integer facts of S1 (S2: its thin cuts), S3, S4 and D7 on their cuts (source_probe_cases.slab_facts)."""
    S1, S3 = spc.DIRECTED["S1"], spc.DIRECTED["S3"]
    assert {c.shape for c in map(spc.DIRECTED.get, spc.SLAB_CASES)} == {spc.SLAB_SHAPE}
    assert all(60 <= spc.DIRECTED[n].nsteps <= 100 for n in spc.SLAB_CASES)
    # S1: 200 entries in strip-plane (plane 7, rows 8..11) and 200 in (plane 8, rows 8..11) — the dense path, on whichever rank owns the plane
    for cuts in (spc.CUT_2, spc.CUT_3, spc.CUT_4):
        facts = spc.slab_facts(S1, cuts)
        for plane in (7, 8):
            r = next(q for q, (k0, nk) in enumerate(cuts) if k0 <= plane < k0 + nk)
            assert facts[r]["sp"][plane - cuts[r][0]].tolist() == [0, 0, 200, 0, 0, 0] and 200 >= spc.SRC_SCAN_MAX + 1 and facts[r]["dense"]
        assert sum(f["dense"] for f in facts) == (1 if cuts == spc.CUT_3 else 2)       # (CUT_3: planes 7 and 8 are ONE slab, the two-plane one)
        # probes 2 (V, plane 8) and 3 (I, plane 7): every cell on a halo-dependent plane of its owner, where the cut runs between the two
        v8 = [f["halo_cells_V"][2] for f in facts]
        i7 = [f["halo_cells_I"][3] for f in facts]
        if cuts == spc.CUT_3:      # (planes 7 and 8 are the two-plane slab's own: its halo-dependent cells are those of probes 0 and 1)
            assert not any(v8) and not any(i7) and facts[1]["cells"][2:4] == [280, 270] and facts[1]["halo_cells_V"][0] >= 40 <= facts[1]["halo_cells_I"][1]
        else:
            assert max(v8) == 280 == sum(v8) and max(i7) == 270 == sum(i7), (cuts, v8, i7)
        assert max(f["cells"][2] for f in facts) == 280 > spc.BLOCK and max(f["cells"][3] for f in facts) == 270 > spc.BLOCK
        # probes 0 and 1 (300 cells over planes 6..9): cells on both sides of every cut between 6 and 9, some of them halo-dependent
        for q, key in ((0, "halo_cells_V"), (1, "halo_cells_I")):
            assert sum(f["cells"][q] for f in facts) == 300 and sum(f["cells"][q] > 0 for f in facts) == {2: 2, 3: 3, 4: 2}[len(cuts)]
            assert sum(f[key][q] for f in facts) >= 40
        # probe 4 (planes 2..4): the lowest rank's alone
        assert [f["cells"][4] for f in facts] == [20] + [0] * (len(cuts) - 1)
    assert [nk for _, nk in spc.CUT_3].count(2) == 1 and [nk for _, nk in spc.CUT_4].count(2) == 2
    never = sum(int(np.sum((s[3] >= S1.nsteps))) for _, s in S1.all_sources())
    assert never == 6
    # S3: the repeated edge arrives after the second call, on plane 8; the series stop short of the run
    first, more = S3.all_sources()[1]
    key = more[0] * 4 + more[1]
    rep = np.flatnonzero(key[1:] == key[:-1])
    assert first == 8 and more[0].size == 40 and rep.size == 1 and np.unique(key).size == 39
    assert more[0][rep[0]] // (40 * 24) == 8 and more[2][rep[0]] != more[2][rep[0] + 1] and more[3][rep[0]] != more[3][rep[0] + 1]
    assert set((more[0] // (40 * 24)).tolist()) == {7, 8}
    assert S3.calls == (1, 7, 40, 12) and S3.cap == 55 < S3.nsteps and [f for f, _ in S3.all_probes()][-2:] == [8, 8]
    for cuts in (spc.CUT_2, spc.CUT_3):
        facts = spc.slab_facts(S3, cuts)
        assert any(f["dup"] for f in facts) and not any(f["dense"] for f in facts)
        assert all(sum(f["cells"][q] > 0 for f in facts) >= 2 for q in (8, 9)) or cuts == spc.CUT_3      # the later probes straddle 7 | 8
    # S4: near a Mur face (x-low) in plane 8; V-probe cells ON the x-low node plane in planes 7 and 8
    for name in ("S4-zcpml", "S4-zmur"):
        c = spc.DIRECTED[name]
        r = spc.regimes(c)
        assert r["near_mur"] and not r["fusable"] and c.boundary[:4] == ("MUR",) * 4
        k, j, i = spc._kji(c, c.probes[0][1])
        assert c.probes[0][0] == spc.KIND_V and set(i.tolist()) == {0} and sorted(set(k.tolist())) == [7, 8]
        sk, _, si = spc._kji(c, c.sources[0][0])
        assert (int(si[0]), int(sk[0])) == (1, 8) and np.all(si[1:] >= 3)
        for cuts in (spc.CUT_2, spc.CUT_3, spc.CUT_4):
            assert sum(f["halo_cells_V"][0] for f in spc.slab_facts(c, cuts)) == 6
    assert {n for n, _, t, o in spc.SLAB_RUNS if n.startswith("S4")} == {"S4-zcpml", "S4-zmur"}
    assert all(t.startswith("linked") or t == "half-steps" or o.startswith("refused") for n, _, t, o in spc.SLAB_RUNS if n.startswith("S4"))
    # D7 and S1, S3: under every transport
    for name in ("D7", "S1", "S3"):
        assert {t for n, _, t, _ in spc.SLAB_RUNS if n == name} == set(spc.TRANSPORTS)
    facts = spc.slab_facts(spc.DIRECTED["D7"], spc.CUT_2)
    assert [f["cells"] for f in facts] == [[2, 4], [2, 4]]


def test_drawn_slab_batch_covers_what_it_claims():
    """Conditions on the seed (source_probe_cases.SLAB_SEED): if one fails, another seed is due, not a lower floor."""
    t = spc.slab_batch_coverage()
    print(t)
    assert min(t["transports"].values()) >= 3, t
    assert t["two_plane_slabs"] >= 2 and t["probes_across_a_cut"] >= 8 and t["rank_probe_pairs_without_cells"] >= 4, t
    assert t["slabs_with_a_dense_strip_plane"] >= 2 and t["mur_cases"] >= 3, t
    assert 3 * t["cuts_on_a_held_plane"] >= t["cuts"], t          # (half are placed there; others land there by chance)
    for n in range(spc.N_SLAB_DRAWN):
        case, cuts, transport = spc.drawn_slabs(n)
        assert case.shape[2] >= 8 and 2 <= len(cuts) <= 4 and min(nk for _, nk in cuts) >= 2
        assert cuts[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(cuts[:-1], cuts[1:])) and sum(cuts[-1]) == case.shape[2]
        assert transport in spc.TRANSPORTS and not ("MUR" in case.boundary and transport.startswith("p2p"))


ORACLE_SLABS = sorted({(n, c) for n, c, _, o in spc.SLAB_RUNS if o == "ok"})


@pytest.mark.parametrize("name,cuts", ORACLE_SLABS, ids=[f"{n}-{len(c)}slabs" for n, c in ORACLE_SLABS])
def test_oracle_as_slabs_is_the_oracle_as_one_slab(oracle_lib, name, cuts):
    """The cases and the ownership rule before a GPU sees them: the oracle half-stepped as slabs, halos carried by the host, has the
    single slab's fields bit for bit; every rank's series is the series of the cells it owns (all zero where it owns none, zero before
    a later probe's first timestep), and the ranks' series add up to the single slab's.

    Bit for bit as the GPU tests' _fields_equal has it: every value equal, and the bits wherever the value is not zero.  The SIGN of a zero
    on a dead edge (both coefficients 0) is not the single slab's everywhere: on the wall row j = 0 the oracle's difference along y reads
    the last row of the plane below, and below a slab's plane 0 lies the ghost plane, which holds the two halo components only (S1, cut
    7 | 8: Vx at (16, 0, 8) is +0 instead of -0)."""
    case = spc.DIRECTED[name]
    ref = spc.reference(case, oracle_lib)
    engs = spc.run_slabs(case, oracle_lib, cuts, "half-steps")
    assert all(e.step == case.nsteps for e in engs)
    got, want = np.concatenate([e.fields() for e in engs], axis=2), ref["fields"]
    assert np.array_equal(got, want) and np.array_equal(_bits(got)[want != 0], _bits(want)[want != 0])
    trees, facts = spc.slab_trees(case, oracle_lib, cuts), spc.slab_facts(case, cuts)
    for q, (first, p) in enumerate(case.all_probes()):
        parts = [e.get_probe(q) for e in engs]
        for r, got in enumerate(parts):
            assert len(got) == min(case.nsteps, case.cap) == len(trees[r][q]) and not got[:first].any()
            assert got.any() == (facts[r]["cells"][q] > 0) == trees[r][q].any(), (name, r, q)
            assert rel_l2(got, trees[r][q]) < 1e-12, (name, r, q)
        assert rel_l2(sum(parts), ref["own"][q]) < 1e-12 and rel_l2(sum(t[q] for t in trees), ref["own"][q]) < 1e-12, (name, q)


def test_tree_series_of_a_slab_takes_the_clipped_list():
    """Thread t takes the entries t, t + 256, ... of the list a slab KEEPS.  Entries 0 and 256 of the whole list share thread 0 and cancel
    there: 298.  The upper slab does not own entry 0: -2^62 becomes entry 255, a thread of its own, and swallows every other thread's sum
    in the tree (half a unit in the last place of 2^62 is 512).  So the ranks' series need not add up to the single slab's in exact
    arithmetic — 1e-12 bounds that sum, the per-rank series are pinned to the clipped tree."""
    shape = (4, 4, 4)
    idx = np.concatenate([[0], np.full(299, 40)])            # one cell in plane 0, 299 in plane 2
    w = np.ones(300, np.float32)
    w[0], w[256] = 2.0 ** 62, -2.0 ** 62
    case = spc.Case("clip", shape, ("PEC",) * 6, 0, spc.signal(), [], [spc.prb(spc.KIND_V, idx, [0] * 300, w)], (1,))
    V = np.zeros((3, 4, 4, 4), np.float32)
    V[0].reshape(-1)[[0, 40]] = 1.0
    whole, = spc.tree_series(case, [(V, V)])
    lower, = spc.tree_series(case, [(V, V)], planes=(0, 2))
    upper, = spc.tree_series(case, [(V, V)], planes=(2, 2))
    assert whole[0] == 298.0 and lower[0] == 2.0 ** 62 and upper[0] == -2.0 ** 62 and lower[0] + upper[0] != whole[0]


def test_tree_sum_is_the_documented_order():
    """Cells 0 and 256 belong to thread 0 and cancel there, before cell 1 joins in the tree: 1; the sequential 1e16 + 1 - 1e16 is 0."""
    w = np.ones(300, np.float32)
    f = np.zeros(300, np.float32)
    f[0], f[1], f[256] = 1e16, 1.0, -1e16
    assert spc.tree_sum(w, f) == 1.0 and float(np.float32(1e16)) + 1.0 - float(np.float32(1e16)) == 0.0
    assert spc.tree_sum([], []) == 0.0


# ---- hard E edges and probes.py lists on the slabs (source_probe_cases H1 ... H4) -------------------------------------------------------
def test_hard_cases_sit_on_the_cut_planes():
    """Integer arithmetic: every hard edge lies on a plane its case claims, each edge once; H1 has an edge on planes k0 - 1 and k0 of
    every cut, H2 x and y edges IN every cut plane; H3's soft list spans every slab with three delays and one edge twice, and its
    probes.py lists (voltage line, current loop) have cells on both sides of every cut, its point probes a node on either side of 7 | 8;
    H4 has hard edges in the second block of a strip-plane."""
    plane = spc.SLAB_SHAPE[0] * spc.SLAB_SHAPE[1]
    for name in spc.HARD_CASES:
        c = spc.DIRECTED[name]
        idx, comp, amp, delay = c.hard
        k = idx // (c.shape[0] * c.shape[1])
        assert sorted(set(k.tolist())) == list(spc.HARD_PLANES[name]) and np.unique(idx * 3 + comp).size == idx.size and np.all(delay >= 0) and np.all(amp != 0)
        for q in range(idx.size):
            t = spc.hard_table(c, q)
            assert t.any() and t.size == c.nsteps and not t[:int(delay[q])].any() and not t[int(delay[q]) + len(c.signal):].any()
    cuts_k0 = sorted({k0 for cuts in (spc.CUT_2, spc.CUT_3) for k0, _ in cuts[1:]})
    assert cuts_k0 == [7, 8, 9]
    h1, h2 = spc.DIRECTED["H1-line"], spc.DIRECTED["H2-plate"]
    k1 = set((h1.hard[0] // plane).tolist())
    assert set(h1.hard[1].tolist()) == {2} and all({k0 - 1, k0} <= k1 for k0 in cuts_k0)
    for k0 in cuts_k0:
        on = h2.hard[0] // plane == k0
        assert set(h2.hard[1][on].tolist()) == {0, 1} and on.sum() == 40 > spc.SRC_SCAN_MAX
    assert np.array_equal(spc.DIRECTED["H2-plate-mur"].hard[0], h2.hard[0]) and spc.DIRECTED["H2-plate-mur"].boundary[:4] == ("MUR",) * 4
    h3 = spc.DIRECTED["H3-soft-and-probes"]
    idx, comp, amp, delay = h3.sources[0]
    key = idx * 3 + comp
    assert set(delay.tolist()) == {0, 4, 9} and np.unique(key).size == key.size - 1 and np.unique(amp).size > 20
    for cuts in (spc.CUT_2, spc.CUT_3):
        facts = spc.slab_facts(h3, cuts)
        assert all(f["sp_max"] > 0 for f in facts) and any(f["dup"] for f in facts)
        for q, pname in enumerate(h3.probe_names):
            owners = sum(f["cells"][q] > 0 for f in facts)
            assert owners == (len(cuts) if pname in ("ut", "it") else 1), (pname, cuts, owners)      # the line and the loop: cells on every slab
    node_k = {pname: int(h3.probes[q][1][0] // plane) for q, pname in enumerate(h3.probe_names)}
    assert (node_k["et7"], node_k["et8"], node_k["ht7"], node_k["ht8"]) == (7, 8, 7, 8)
    assert [p[0] for p in h3.probes] == [0, 1] + [0] * 6 + [1] * 6 and h3.probes[0][1].size == 6 and h3.probes[1][1].size == 18
    r = spc.regimes(spc.DIRECTED["H4-second-block"])
    assert r["src_blocks"] == [0, 1] and r["blocks_per_strip_plane"] == 2
    for name in ("H1-line", "H2-plate", "H3-soft-and-probes"):
        assert {t for n, _, t, _ in spc.SLAB_RUNS if n == name} == set(spc.TRANSPORTS)
        assert {(s, o) for n, s, o, _ in spc.RUNS if n == name} == {("RESIDENT", "resident"), ("WF1", "one"), ("DIRECT", "two")}
    assert any(o.startswith("refused") for n, _, _, o in spc.SLAB_RUNS if n == "H2-plate-mur")


@pytest.mark.parametrize("name", spc.HARD_CASES)
def test_hard_edges_on_the_oracle(oracle_lib, name):
    """The oracle's operator holds vv = vi = 0 on every hard edge and its V-probes on them read float32(amp * sig[n - d]) exactly; with
    the override of ONE hard edge dropped the fields are others."""
    case = spc.DIRECTED[name]
    ref = spc.reference(case, oracle_lib)
    e = spc.engine_for(case, oracle_lib)
    op = e.get_operator()
    idx, comp, amp, delay = case.hard
    assert not op[0].reshape(3, -1)[comp.astype(int), idx].any() and not op[1].reshape(3, -1)[comp.astype(int), idx].any()
    for q, (first, (kind, pidx, pcomp, w)) in enumerate(case.all_probes()):
        hit = np.flatnonzero((idx == pidx[0]) & (comp == pcomp[0])) if pidx.size == 1 and kind == spc.KIND_V else []
        if len(hit):
            assert np.array_equal(ref["own"][q], spc.hard_table(case, int(hit[0]))) and np.array_equal(ref["tree"][q], ref["own"][q])
    assert sum(1 for _, p in case.all_probes() if p[1].size == 1) >= 4
    keep = np.arange(idx.size) != idx.size // 2
    e2 = spc.raw_engine(oracle_lib, (case.scene, case.shape), case.boundary, 0, case.cap, cpml_cells=case.cpml_cells, hard=(idx[keep], comp[keep]))
    spc.apply(case, e2)
    spc.run(case, e2)
    assert not np.array_equal(e2.fields(), ref["fields"])
