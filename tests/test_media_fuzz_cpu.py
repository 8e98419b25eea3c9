"""Guards of the randomised media / sheet parity run (tests/fuzz_parity.py --media) that need no GPU: the fixed-seed batch of the -m gpu
suite is accepted by the host layer and covers, together, what it was written to reach; the reference side of the first cases and of
the directed GPU scenes is finite and moving everywhere it has to be; the one checker equals the sheets-only one it replaced."""
import numpy as np
import pytest

import fuzz_parity
from restatement import Restatement
from test_sheet_model_cpu import MU0, _sheet, cavity_sim

WANTED = ({f"k_debye<{m},{k}>" for m in ("false", "true") for k in (4, 8)} | {"8 media"} | {f"x0 mod 4 = {r}" for r in range(4)}
          | {f"x1 mod 4 = {r}" for r in range(4)} | {f"nx mod 4 = {r}" for r in range(4)}
          | {"box at x0 = 0", "box at the last column", ">= 20 blocks", "medium on a Mur face node, no apply pass", "medium on a Mur face node, apply pass",
             "sheets without media", "sheets with media", "port edge inside a medium", "nf2ff none", "nf2ff dft", "nf2ff record", ">= 3 run() calls",
             "hole inside a box", "graded", "uniform", "raw operator", "sheet edges that are dispersive edges"})


def features(case, sim):
    """What a drawn, accepted case reaches (the table of the randomised media run in docs/HISTORY.md)."""
    out = {f"nx mod 4 = {case['shape'][0] % 4}", f"nf2ff {case['nf2ff']}", "graded" if case["graded"] else "uniform"}
    if len(case["calls"]) >= 3:
        out.add(">= 3 run() calls")
    if not case["classes"]:
        out.add("raw operator")
    d, n = sim.debye, case["shape"]
    if sim.sheets is not None:
        out.add("sheets with media" if d is not None else "sheets without media")
    if d is None:
        return out
    out.add(f"k_debye<{'true' if len(d.media) > 1 else 'false'},{4 if d.K <= 4 else 8}>")
    if len(d.media) == 8:
        out.add("8 media")
    for c in range(3):
        if not d.w[c].size:
            continue
        lo, hi, w = d.lo[c], d.hi[c], d.w[c]
        out |= {f"x0 mod 4 = {lo[0] % 4}", f"x1 mod 4 = {hi[0] % 4}"}
        if lo[0] == 0:
            out.add("box at x0 = 0")
        if hi[0] == (n[0] - 1 if c == 0 else n[0]):
            out.add("box at the last column")
        groups = w.shape[0] * w.shape[1] * (-(-hi[0] // 4) - lo[0] // 4)
        if groups >= 20 * 256:
            out.add(">= 20 blocks")
        if np.any(w[1:-1, 1:-1, 1:-1] == 0):
            out.add("hole inside a box")
        for f in range(6):
            a = f // 2
            if case["kinds"][f] == "MUR" and c != a and (hi[a] == n[a] if f % 2 else lo[a] == 0):      # tangential edges on the face's node plane
                out.add("medium on a Mur face node, " + ("apply pass" if case["env"].get("FDTD_MUR_APPLY_PASS") == "1" else "no apply pass"))
    px, py, z0, _ = case["port"]
    lo, hi = d.lo[2], d.hi[2]
    if d.w[2].size and all(l <= p < h for l, p, h in zip(lo, (px, py, z0), hi)) and d.w[2][z0 - lo[2], py - lo[1], px - lo[0]] != 0:
        out.add("port edge inside a medium")
    if sim.sheets is not None:
        nx, ny, _ = n
        k, r = np.divmod(sim.sheets.idx, nx * ny)
        j, i = np.divmod(r, nx)
        for c in range(3):
            q = sim.sheets.comp == c
            lo, hi = d.lo[c], d.hi[c]
            ins = q & (i >= lo[0]) & (i < hi[0]) & (j >= lo[1]) & (j < hi[1]) & (k >= lo[2]) & (k < hi[2])
            if ins.any() and np.any(d.w[c][k[ins] - lo[2], j[ins] - lo[1], i[ins] - lo[0]] != 0):
                out.add("sheet edges that are dispersive edges")
    return out


def test_fixed_seed_batch_is_accepted_and_covers_what_it_is_for():
    ncases, seed = fuzz_parity.MEDIA_BATCH
    rng = np.random.default_rng(seed)
    seen, accepted, refused = set(), 0, []
    for n in range(ncases):
        case = fuzz_parity.draw_media_case(rng)
        assert case["media"] or case["sheets"]
        assert 14 <= case["shape"][0] <= 90 and 12 <= case["shape"][1] <= 60 and 12 <= case["shape"][2] <= 40 and 2 <= case["cells"] <= 8
        assert 1 <= len(case["calls"]) <= 5 and all(1 <= k <= 60 for k in case["calls"]) and len(case["media"]) <= 8 and len(case["sheets"]) <= 3
        assert eval(repr(case)) == case                      # printable, and reproducible from what the log prints
        try:
            sim = fuzz_parity.media_case_sim(case)
        except ValueError as exc:
            refused.append((n, str(exc)))
            continue
        accepted += 1
        assert sim.debye is not None or sim.sheets is not None
        seen |= features(case, sim)
    print(f"{accepted} of {ncases} accepted; refused: {refused}")
    assert 6 * accepted >= 5 * ncases, refused
    assert not WANTED - seen, sorted(WANTED - seen)


def test_same_seed_same_cases():
    first = fuzz_parity.draw_media_case(np.random.default_rng(5))
    rng = np.random.default_rng(5)
    assert fuzz_parity.draw_media_case(rng) == first and fuzz_parity.draw_media_case(rng) != first


def test_reference_side_of_the_first_cases_moves_everywhere(oracle_lib):
    """The first cases of the batch stepped on the reference alone: finite, non-zero, every branch state of every dispersive edge the
    operator does not hold, and the branch currents of every sheet edge, off zero."""
    rng = np.random.default_rng(fuzz_parity.MEDIA_BATCH[1])
    ran = 0
    for n in range(6):
        case = fuzz_parity.draw_media_case(rng)
        try:
            problems, _ = fuzz_parity.run_media_case(case, None, oracle_lib)
        except ValueError:
            continue
        assert problems == [], (n, case, problems)
        ran += 1
    assert ran >= 5


@pytest.mark.parametrize("name", ["multi-k8-three", "multi-k8-eight", "many-blocks", "slab-to-four-mur", "filled-mur", "filled-pec",
                                  "media-and-sheets-mur"])
def test_reference_side_of_the_directed_scenes(oracle_lib, name):
    import test_dispersion_gpu as tg
    sim = tg._sim(name, 40)
    r = Restatement(sim, oracle_lib, seed=21)
    r.run(12)
    assert fuzz_parity.media_reference_problems(r) == []
    if name.startswith(("slab", "filled")):       # dispersive cells on face nodes: edges the operator holds are at rest, and they exist
        held = [(sim.debye.w[c] != 0) & (r.debye.vi[c] == 0) for c in range(3)]
        assert sum(int(h.sum()) for h in held) > 300
        assert all(np.all(r.debye.u[c][:, held[c]] == 0) and np.all(r.debye.vprev[c][held[c]] == 0) for c in range(3))


def test_reference_side_of_the_alignment_scenes(oracle_lib):
    import test_dispersion_gpu as tg
    for x0, x1, nx in (tg.X_ALIGN[0], tg.X_ALIGN[7], tg.X_ALIGN[16], tg.X_ALIGN[18]):
        r = Restatement(tg._x_aligned_sim(x0, x1, nx, 20), oracle_lib, seed=1)
        r.run(8)
        assert fuzz_parity.media_reference_problems(r) == []


def _sheet_run_as_it_was(sim, lib, nsteps):
    """The sheets-only restatement spelt out on its own, as the sheet tests first had it: an independent check of restatement.Restatement."""
    saved, sim.sheets = sim.sheets, None
    try:
        e = sim.build(lib)
    finally:
        sim.sheets = saved
    idx, comp, vi, cls, alpha, b = sim.sheet_tables()
    al, bb = alpha[cls].T.copy(), b[cls].T.copy()
    vprev = np.zeros(idx.size, np.float32)
    ib = np.zeros((alpha.shape[1], idx.size), np.float32)
    by_c = [np.nonzero(comp == c)[0] for c in range(3)]
    for n in range(nsteps):
        e.half_step(0)
        Vs = [e.get_field(0, c) for c in range(3)]
        V = np.empty(idx.size, np.float32)
        for c in range(3):
            V[by_c[c]] = Vs[c].reshape(-1)[idx[by_c[c]]]
        vnew = _sheet().correction(V, vi, vprev, ib, al, bb)
        vprev = vnew
        for c in range(3):
            if by_c[c].size:
                Vs[c].reshape(-1)[idx[by_c[c]]] = vnew[by_c[c]]
                e.set_field(0, c, Vs[c])
        e.half_step(1)
    return e, vprev, ib


def test_one_checker_equals_the_sheets_only_one(oracle_lib):
    n = 300
    e0, v0, i0 = _sheet_run_as_it_was(cavity_sim(3e5, 1e-3, nr_ts=n), oracle_lib, n)
    r1, en = Restatement(cavity_sim(3e5, 1e-3, nr_ts=n), oracle_lib), []
    for q in range(n):                               # step by step, with the energy every 100 timesteps
        r1.step()
        if (q + 1) % 100 == 0:
            sv, si = r1.e.energy()
            en.append(8.854187817e-12 * sv + MU0 * si)
    e1, v1, i1, en = r1.e, r1.sheets.vprev, r1.sheets.ib, np.array(en)
    r = Restatement(cavity_sim(3e5, 1e-3, nr_ts=n), oracle_lib)
    assert r.debye is None and r.sheets is not None
    r.run(n)
    assert np.abs(i0).max() > 0 and np.abs(e0.fields()).max() > 0
    for e, v, i in ((e1, v1, i1), (r.e, r.sheets.vprev, r.sheets.ib)):
        assert np.array_equal(e.fields(), e0.fields()) and np.array_equal(v, v0) and np.array_equal(i, i0)
    sv, si = e0.energy()
    want = 8.854187817e-12 * sv + MU0 * si      # (a threaded reduction: equal to rounding, not to the bit)
    assert en.shape == (3,) and abs(en[-1] - want) <= 1e-12 * want
