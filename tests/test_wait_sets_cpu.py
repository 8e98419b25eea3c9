"""Host proof of the flag wait sets of the one-launch schedule (csrc/wait_sets.hpp: what k_step's blocks poll, compiled for the host by
`make -C csrc waitsets_host` and loaded with ctypes).  A set that is one block short is a race that field parity does not see — the flags
are almost always "long set" —, so the sets are checked against the stencil itself, every thread of every block of every tiling enumerated.

The model (csrc/wait_sets_model.hpp states it in full; plain divisions, nothing shared with the arithmetic under test):
  * H thread (k, j, c) — c its four-cell group — reads V written by, and overwrites I read by, the E threads (k, j, c), (k, j, c + 1),
    (k, j + 1, c), (k + 1, j, c)  (kernels.hip body_H: vz_ip / vy_ip, vz_jp / vx_jp, vy_kp / vx_kp; body_E: iz_im / iy_im, iz_jm / ix_jm,
    iy_km / ix_km); an E thread of a later timestep of a launch mirrors it.
  * Mur: the candidate of a face point is written by the E thread that owns the point's INNER node (kernels.hip:60-96, mur_post_inline,
    called by body_E's post pass: a z face by the threads of plane `in`, a y face by those of row `in`, an x face by the thread whose group
    holds cell `in`; in = b + 1 / b - 1).  An H thread loads candidates in place of boundary voltages as kernels.hip:392-449 (mur_load_V)
    selects them: z over y over x for its own cells, row j + 1, plane k + 1 and cell 4c + 4, and four x-face candidates of their own.
Tilings: the sweep of the issue that introduced this file — P4 (threads per row), tys (rows per strip), ny, nk below."""
import ctypes

import pytest

from helpers import WsFail, load_wait_sets, ws_geom

B = 256
P4S = (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 1024, 1925, 7679)
TYS = (1, 2, 3, 4, 5, 7, 17, 40)
NKS = (2, 3)
# WAIT_SETS_DROP = n: the clause the library lacks, and the check that has to notice (0 wf_wait, 1 wf_wait_back, 2 Mur)
DROPS = {1: ("wf_wait: same-strip neighbours", 0), 2: ("wf_wait: next strip", 0), 3: ("wf_wait: plane above", 0),
         4: ("wf_wait_back: same-strip neighbours", 1), 5: ("wf_wait_back: previous strip", 1), 6: ("wf_wait_back: plane below", 1),
         7: ("wf_mur_wide: plane on the lower z face", 2), 8: ("wf_mur_wide: plane on the upper z face", 2),
         9: ("wf_mur_wide: row on the lower y face", 2), 10: ("wf_mur_wide: row on the upper y face", 2),
         11: ("wf_mur_wide: upper x face starts a group", 2), 12: ("wf_wait_mur: plane k - 1", 2), 13: ("wf_wait_mur: plane k + 1", 2),
         14: ("wf_wait_mur: strip s - 1", 2), 15: ("wf_wait_mur: strip s + 1", 2)}


def tilings():
    """(P4, ny, tys, nk), small ones first (a library that lacks a clause fails early)"""
    out = []
    for P4 in P4S:
        for tys in TYS:
            nys = {tys, tys + 1, 2 * tys + 1, 3 * tys - 1} | ({tys // 2} if tys > 1 else set())   # ... and one value below the strip height
            out += [(P4, ny, tys, nk) for ny in sorted(nys) for nk in NKS]
    return sorted(out, key=lambda t: t[0] * t[1] * t[3])


def first_failure(lib, which):
    """The first tiling whose brute force fails, as text, or None.  which 0 / 1: wf_wait_flag / wf_wait_back_flag; 2: wf_mur_wide with the
    set it selects, all 64 subsets of the six faces, nx = 4 P4 - 3 .. 4 P4 (upper x index = 0, 1, 2, 3 mod 4); a Mur face needs an
    inner node (ny, nx >= 2), and the tilings whose 9 nbs flags exceed the workgroup are not the schedule's."""
    fail, faces, proven = WsFail(), ctypes.c_int(0), 0
    for P4, ny, tys, nk in tilings():
        if which < 2:
            g = ws_geom(lib, P4, ny, tys, nk)
            assert 2 * (1 + P4 // B) + 3 <= 64
            if lib.ws_check(g, which, 4 * P4 - 1, fail):
                return f"P4 {P4} ny {ny} tys {tys} nk {nk}: {fail!r}"
            proven += 1
        elif ny >= 2:
            for nx in range(max(2, 4 * P4 - 3), 4 * P4 + 1):
                r = lib.ws_check_mur_faces(nx, ny, tys, nk, faces, fail)
                if r < 0:
                    assert 9 * ((min(tys, ny) * P4 + B - 1) // B) > B
                    break
                if r:
                    return f"nx {nx} (P4 {P4}) ny {ny} tys {tys} nk {nk} faces {faces.value:#04x}: {fail!r}"
                proven += 1
    assert proven > (800 if which < 2 else 3000)
    return None


@pytest.fixture(scope="module")
def ws():
    return load_wait_sets()


def test_forward_flag_set_covers_raw_and_war_of_every_h_thread(ws):
    """wf_wait: the E flags of own group, i + 1, row j + 1 (running into the next strip) and plane k + 1 — the E blocks that wrote what the
    H block reads are the ones that read what it overwrites."""
    assert first_failure(ws, 0) is None


def test_backward_flag_set_covers_every_h_block_an_e_block_depends_on(ws):
    """wf_wait_back over the whole sweep, plane lane included (test_host_logic_cpu.py keeps the hand-enumerated cases)."""
    assert first_failure(ws, 1) is None


def test_plane_lanes_and_lane_budgets(ws):
    """Lane 2 hop + 2 of both sets is the same block one plane on (none beyond the slab), no lane beyond it polls, 2 hop + 3 <= 64 lanes
    on every tiling; the wide set stays within 9 nbs threads, which fit the workgroup wherever the host takes Mur faces into the launch."""
    for P4, ny, tys, nk in tilings():
        g = ws_geom(ws, P4, ny, tys, nk)
        hop = 1 + P4 // B
        assert 2 * hop + 3 <= 64
        per_plane = g.nstrips * g.nbs
        for k in range(nk):
            for strip in range(g.nstrips):
                rows = min(tys, ny - strip * tys)
                for pb in {0, (rows * P4 - 1) // B // 2, (rows * P4 - 1) // B}:
                    me = (k * g.nstrips + strip) * g.nbs + pb
                    assert ws.ws_wait_flag(g, k, strip, pb, 2 * hop + 2) == (me + per_plane if k + 1 < nk else -1)
                    assert ws.ws_wait_back_flag(g, k, strip, pb, 2 * hop + 2) == (me - per_plane if k > 0 else -1)
                    assert ws.ws_wait_flag(g, k, strip, pb, 0) == me == ws.ws_wait_back_flag(g, k, strip, pb, 0)
                    for lane in range(2 * hop + 3, 64):
                        assert ws.ws_wait_flag(g, k, strip, pb, lane) == -1 == ws.ws_wait_back_flag(g, k, strip, pb, lane)
                    if 9 * g.nbs <= B:
                        polled = [ws.ws_wait_mur_flag(g, k, strip, t) for t in range(B)]
                        assert all(f == -1 for f in polled[9 * g.nbs:])
                        want = {(kk * g.nstrips + ss) * g.nbs + q for kk in range(max(k - 1, 0), min(k + 2, nk))
                                for ss in range(max(strip - 1, 0), min(strip + 2, g.nstrips)) for q in range(g.nbs)}
                        got = [f for f in polled if f >= 0]
                        assert set(got) == want and len(got) == len(want)


def test_mur_candidates_come_from_blocks_of_the_set_the_block_takes(ws):
    """wf_mur_wide together with wf_wait_mur / wf_wait: every candidate a thread loads, and every plain dependence, lies in the set its
    block actually takes — 64 face subsets, upper x index = 0 .. 3 (mod 4)."""
    assert first_failure(ws, 2) is None


@pytest.mark.parametrize("drop", sorted(DROPS))
def test_a_library_without_one_clause_fails_the_proof(drop):
    """Negative control: the proof notices each clause of the wait sets when it is missing (a clause nobody misses is dead, or untested)."""
    name, which = DROPS[drop]
    assert first_failure(load_wait_sets(drop), which) is not None, f"nobody misses: {name}"
