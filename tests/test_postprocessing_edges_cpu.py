"""The post-processing kernels beyond their first chunk: the case builders and references of test_postprocessing_edges_gpu.py, and
every condition those cases have to meet, checked here on the references alone — the spans the SAR cubes reach (more x cells than
one wave's 64 lanes, more (j, k) columns than 64, both), the extended-precision far-field reference with its bar and two mutations
the bar must see, the frequency sets of the recorder transform, and long probes whose cells lie in every strip-plane of the grid."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ROOT, pkg
from helpers import patch_sim, seeded_fields
from test_sar_model_cpu import MARGIN, MAX_EXCLUDED, _pockets, graded

EDGES = os.path.join(ROOT, "profiles", "postprocessing", "edges.txt")
U = 2.0 ** -53           # the unit roundoff of float64


def _note(tag, lines):
    """Replace the block `tag` of profiles/postprocessing/edges.txt when FDTD_WRITE_KAT is set (the committed record of the measured
    values)."""
    if not os.environ.get("FDTD_WRITE_KAT"):
        return
    os.makedirs(os.path.dirname(EDGES), exist_ok=True)
    old = open(EDGES).read().split("\n") if os.path.isfile(EDGES) else []
    keep, skip = [], False
    for l in old:
        if l.startswith("## "):
            skip = l == f"## {tag}"
        if not skip and l != "":
            keep.append(l)
    with open(EDGES, "w") as fh:
        fh.write("\n".join(keep + [f"## {tag}"] + list(lines)) + "\n")


def _note_line(tag, key, line):
    """Put the line `key: line` into the block `tag` (replacing the block's line of that key, the block kept sorted): tests that run
    case by case, in any order or selection, each leave their own line."""
    if not os.environ.get("FDTD_WRITE_KAT"):
        return
    old = open(EDGES).read().split("\n") if os.path.isfile(EDGES) else []
    mine, on = [], False
    for l in old:
        if l.startswith("## "):
            on = l == f"## {tag}"
        elif on and l != "" and not l.startswith(key + ": "):
            mine.append(l)
    _note(tag, sorted(mine + [f"{key}: {line}"]))


def test_extended_precision_is_extended():
    """np.longdouble must carry at least 64 mantissa bits: on a platform where it is float64 the references below would compare
    float64 with itself — fail here, visibly."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


# ---- A. SAR averaging with cubes wider than a wave ---------------------------------------------------------------------------------
def sar_cases():
    """name -> (dx, dy, dz, rho, p, mass): boxes whose cubes take more than one chunk of cube_sums (csrc/sar.hip: 64 x cells at a time,
    one weight per lane; 64 (j, k) columns at a time)."""
    out = {}
    d = [graded(110, 101, 0.1e-3), graded(5, 102, 2.6e-3), graded(5, 103, 2.6e-3)]
    rho, p = _pockets((5, 5, 110), 104)
    out["x-around-64"] = (*d, rho, p, 1000.0 * (6.5e-3) ** 3)
    d = [graded(200, 116, 0.05e-3), graded(5, 117, 2.6e-3), graded(5, 118, 2.6e-3)]
    rho, p = _pockets((5, 5, 200), 119)
    out["x-around-128"] = (*d, rho, p, 1000.0 * (6.5e-3) ** 3)
    d = [graded(16, 148 + a, 1e-3) for a in range(3)]
    rho, p = _pockets((16, 16, 16), 151, share=0.05)
    rho[6:9, 5:8, 4:7] = 0.0                                         # an air block of 27 cells
    out["columns-around-64"] = (*d, rho, p, 1000.0 * (7.6e-3) ** 3)
    d = [graded(100, 131, 0.1e-3), graded(13, 132, 0.8e-3), graded(13, 133, 0.8e-3)]
    rho, p = _pockets((13, 13, 100), 134)
    rho[:, :, 48:51] = 0.0                                           # an air slab 0.3 mm thick: with the pockets about 10 % of a cube
    out["both-at-once"] = (*d, rho, p, 1000.0 * (7.0e-3) ** 3)
    return out


_SPEC = {}


def sar_spec_of(name, method):
    """average_spec(..., margins=True) of a case, computed once per process."""
    if (name, method) not in _SPEC:
        _SPEC[(name, method)] = pkg("sar").average_spec(*sar_cases()[name], method, margins=True)
    return _SPEC[(name, method)]


def cube_spans(case, half, status):
    """(x cells, (j, k) columns) the final cube of every valid or used voxel overlaps, by sar.overlap."""
    sar = pkg("sar")
    lines = [sar.node_lines(np.asarray(a, np.float64)) for a in case[:3]]
    xs, cols = [], []
    for k, j, i in zip(*np.nonzero((status == 0) | (status == 1))):
        n = [sar.overlap(lines[a][0], lines[a][1][q], half[k, j, i])[1].size for a, q in enumerate((i, j, k))]
        xs.append(n[0])
        cols.append(n[1] * n[2])
    return np.array(xs, int), np.array(cols, int)


def cube_sums_longdouble(lines, rho, p, cell, h):
    """(m, P) of the cube of half-side h about `cell` = (i, j, k) in np.longdouble: the outer product of the three overlap weight
    vectors times rho and p.  No part of average_spec but sar.overlap's choice of the cells that can overlap."""
    sar = pkg("sar")
    ld = np.longdouble
    w, sl = [], []
    for a in range(3):
        e, c = lines[a][0].astype(ld), ld(lines[a][1][cell[a]])
        first, w64 = sar.overlap(lines[a][0], lines[a][1][cell[a]], float(h))
        lo, hi = c - ld(h), c + ld(h)
        n = w64.size
        w.append(np.maximum(ld(0), np.minimum(e[first + 1:first + n + 1], hi) - np.maximum(e[first:first + n], lo)))
        sl.append(slice(first, first + n))
    W = w[2][:, None, None] * w[1][None, :, None] * w[0][None, None, :]
    sub = (sl[2], sl[1], sl[0])
    return np.sum(W * rho[sub].astype(ld)), np.sum(W * p[sub].astype(ld))


def check_valid_cubes_in_longdouble(case, sar_avg, half, status):
    """A check that does not go through average_spec: every voxel called valid, at its own half_side — sar_avg is P / m of that
    cube, the cube holds the mass, and a cube 1e-9 narrower does not (unless the cube is the largest the box allows).  The three
    factors are conditions: each is far above float64 rounding of sums of <= 1e4 non-negative terms.  Returns the largest
    |P / m - sar_avg| / sar_avg."""
    sar = pkg("sar")
    dx, dy, dz, rho, p, mass = case
    lines = [sar.node_lines(np.asarray(a, np.float64)) for a in (dx, dy, dz)]
    ext = [l[0][-1] for l in lines]
    ld = np.longdouble
    worst, n = 0.0, 0
    for k, j, i in zip(*np.nonzero(status == 0)):
        cell, h = (i, j, k), half[k, j, i]
        m, P = cube_sums_longdouble(lines, rho, p, cell, h)
        assert m >= ld(mass) * (1 - ld(1e-12)), (cell, float(m), mass)
        if sar_avg[k, j, i] > 0:
            dev = float(abs(P / m - ld(sar_avg[k, j, i])) / ld(sar_avg[k, j, i]))
            assert dev <= 1e-12, (cell, dev)
            worst = max(worst, dev)
        else:
            assert P == 0
        c = [lines[a][1][cell[a]] for a in range(3)]
        h_max = min(min(c[a], ext[a] - c[a]) for a in range(3))
        assert h <= h_max
        if h < h_max:
            assert cube_sums_longdouble(lines, rho, p, cell, h * (1.0 - 1e-9))[0] < ld(mass), cell
        n += 1
    assert n > 0
    return worst


@pytest.mark.parametrize("method", ["ieee", "simple"])
@pytest.mark.parametrize("name", sorted(sar_cases()))
def test_sar_cases_reach_their_spans_and_keep_clear_of_the_thresholds(name, method):
    """The conditions the cases were chosen for, on the specification alone (the seeds may change, the conditions may not)."""
    case = sar_cases()[name]
    sa, half, status, counts, marg = sar_spec_of(name, method)
    tissue = status >= 0
    assert tissue.any() and np.count_nonzero(marg[tissue] < MARGIN) <= MAX_EXCLUDED * status.size
    assert np.count_nonzero(marg[tissue] < MARGIN) == 0              # (what was measured: no voxel of these cases near a threshold)
    xs, cols = cube_spans(case, half, status)
    print(f"{name} / {method}: status counts {counts.tolist()}, x spans {sorted(set(xs.tolist()))}, columns {sorted(set(cols.tolist()))}")
    if name == "x-around-64":
        assert {63, 64, 65} <= set(xs.tolist()) and (status == 0).sum() >= 200
    elif name == "x-around-128":
        assert {127, 128, 129} <= set(xs.tolist())                   # a third chunk, full and partial
    elif name == "columns-around-64":
        assert 64 in cols and (cols < 64).any() and (cols > 64).any()
        if method == "ieee":                                         # k_sar_second walks ranges of +-5 cells
            assert (status == 1).sum() >= 50 and (status == 0).sum() >= 300
    else:
        valid = status == 0
        vx, vc = cube_spans(case, half, np.where(valid, 0, -1).astype(np.int8))
        assert valid.any() and vx.min() > 64 and vc.min() > 64
        if method == "ieee":
            assert (status == 1).sum() >= 20
    worst = check_valid_cubes_in_longdouble(case, sa, half, status)
    print(f"    largest |P/m - sar_avg| / sar_avg of the specification against np.longdouble: {worst:.2e}")


# ---- B. the far field per direction ------------------------------------------------------------------------------------------------
ETA0 = 376.730313668
C0 = 299792458.0
TRIG = 4          # a double sin / cos of the device library: taken as within 2 ulp = 4 units of 2^-53 of its value


def farfield_reference(pos, Js, Ms, kw, theta, phi):
    """The radiation integral in np.longdouble, from the formula:

        N = sum_p J_p exp(j k r^ . r_p),  L = sum_p M_p exp(j k r^ . r_p),   r^ = (sin th cos ph, sin th sin ph, cos th)
        X_th = X_x cos th cos ph + X_y cos th sin ph - X_z sin th,   X_ph = -X_x sin ph + X_y cos ph        (X = N, L)
        E_th = -j k / (4 pi) (L_ph + eta0 N_th),   E_ph = +j k / (4 pi) (L_th - eta0 N_ph),   eta0 = 376.730313668

    Returns (E_th, E_ph) complex longdouble [nang] and S_a float64 [nang][2]: per direction, for E_th and E_ph, the sums of the
    ABSOLUTE values of every term of the twelve real sums (Re and Im of N_x .. L_z; a term is one product like Re J_x cos(phase)),
    the larger of a component's Re and Im sum, times the absolute projection factors and k / (4 pi) — what a rounding error of the
    kernel is relative to.  (The larger of the two: an error of the phase moves the real part by a share of the imaginary part's
    terms and the other way round.)"""
    ld, cld = np.longdouble, np.clongdouble
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    npts = pos.shape[0]
    th, ph = np.asarray(theta, np.float64).astype(ld).ravel(), np.asarray(phi, np.float64).astype(ld).ravel()
    nang = th.size
    st, ct, sp, cp = np.sin(th), np.cos(th), np.sin(ph), np.cos(ph)
    r = np.stack([st * cp, st * sp, ct], 1)                          # [nang][3]
    F = np.concatenate([np.asarray(Js, np.complex128).reshape(npts, 3), np.asarray(Ms, np.complex128).reshape(npts, 3)], 1)
    Fr, Fi = F.real.astype(ld), F.imag.astype(ld)                    # [npts][6]: J_x J_y J_z M_x M_y M_z
    aFr, aFi = np.abs(F.real), np.abs(F.imag)
    P = pos.astype(ld)
    k = ld(kw)

    def chunk(a):
        arg = k * (r[a] @ P.T)                                       # [dirs][npts]
        c, s = np.cos(arg), np.sin(arg)
        re, im = c @ Fr - s @ Fi, s @ Fr + c @ Fi
        ac, as_ = np.abs(c).astype(np.float64), np.abs(s).astype(np.float64)
        return re, im, np.maximum(ac @ aFr + as_ @ aFi, as_ @ aFr + ac @ aFi)

    X = np.zeros((nang, 6), cld)
    A = np.zeros((nang, 6), np.float64)
    if npts > 0 and nang > 0:
        parts = [slice(a, min(a + 64, nang)) for a in range(0, nang, 64)]
        with ThreadPoolExecutor(max(1, min(16, os.cpu_count() or 1))) as ex:
            for a, (re, im, ab) in zip(parts, ex.map(chunk, parts)):
                X[a] = re + 1j * im
                A[a] = ab
    N, L = X[:, :3], X[:, 3:]
    proj_th = np.stack([ct * cp, ct * sp, -st], 1)
    proj_ph = np.stack([-sp, cp, np.zeros(nang, ld)], 1)
    fac = k / (4 * ld("3.14159265358979323846264338327950288"))
    eta = ld(ETA0)
    E_th = -1j * fac * (np.sum(L * proj_ph, 1) + eta * np.sum(N * proj_th, 1))
    E_ph = 1j * fac * (np.sum(L * proj_th, 1) - eta * np.sum(N * proj_ph, 1))
    a_th, a_ph = np.abs(proj_th).astype(np.float64), np.abs(proj_ph).astype(np.float64)
    f64 = float(fac)
    S = np.stack([f64 * (np.sum(A[:, 3:] * a_ph, 1) + ETA0 * np.sum(A[:, :3] * a_th, 1)),
                  f64 * (np.sum(A[:, 3:] * a_th, 1) + ETA0 * np.sum(A[:, :3] * a_ph, 1))], 1)
    return E_th, E_ph, S


def farfield_K(pos, kw):
    """K of the bar |err| <= K 2^-53 S_a, counted in units of 2^-53 relative to the absolute sums, from k_farfield's operations:

      the strided sum of a thread, ceil(npts / 256) additions of a term                          ceil(npts / 256)
      8 levels of the tree                                                                        8
      a term Re J cos - Im J sin: cos / sin of the phase TRIG, the product 1, the difference 1    TRIG + 2 = 6
      the projection, per product X cos th cos ph: two factors TRIG each, two products 2         2 TRIG + 2 = 10
        ... its two additions 2, eta0 times 1, L + eta0 N 1, k / (4 M_PI) 1 (M_PI itself is 0.35
        off pi), the last product 1                                                               6
      the rounded phase argument: an error d of the phase moves a term by d times its partner
        term (hence the larger of the Re and Im sums in S_a).  r^ . p is a product and two
        fused multiply-adds, then k times: 4 roundings, the first two relative to a part of the
        sum only — counted as 3, relative to k sum_a |r^_a p_a| <= k |p| = PHI                    3 PHI

    K = ceil(npts / 256) + 30 + 3 PHI with PHI = k max |p| of the case: 30 to 55 for the cases at 2.45 GHz within +-0.05 m (PHI <=
    4.5), and 170 to 215 for those at 5.8 GHz within +-0.25 m (PHI up to 53).  (A remark: the 3 leaves out the rounding of r^
    itself — r^_x = sin th cos ph carries up to 2 TRIG + 1 = 9 — which in the worst case would make it 13 PHI; that error is
    the same small turn of the direction for every point, and the bar does not allow for its worst case.)  Measured
    (profiles/postprocessing/edges.txt): the oracle, another float64 order of the same sums, below 5 on every case, below 1
    where there are 255 points or more at 2.45 GHz; a point dropped from the reference misses the bar millions of times over."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    npts = pos.shape[0]
    phi_max = float(kw) * float(np.max(np.linalg.norm(pos, axis=1))) if npts else 0.0
    return -(-npts // 256) + 8 + (TRIG + 2) + (2 * TRIG + 2) + 6 + 3 * phi_max


def farfield_cases():
    """name -> (pos, Js, Ms, kw, theta, phi): random complex currents and random directions.  theta = 0 and theta = pi are added
    explicitly: at 2.45 GHz as cases of their own per point count (one direction at a pole; both poles), so that the cases of
    1, 2, 3, 5 and 7 directions are generic ones; in the cases of 6 and 6643 directions as the first two."""
    out = {}
    spec = [(n, a, 2.45e9, 0.05) for n in (0, 1, 255, 256, 257, 3000) for a in (1, 2, 3, 5, 7, "pole", "poles")]
    spec += [(n, a, 5.8e9, 0.25) for n in (257, 6000) for a in (6, 6643)]
    for q, (npts, dirs, f, ext) in enumerate(spec):
        rng = np.random.default_rng(1000 + q)
        pos = rng.uniform(-ext, ext, (npts, 3))
        Js = rng.standard_normal((npts, 3)) + 1j * rng.standard_normal((npts, 3))
        Ms = rng.standard_normal((npts, 3)) + 1j * rng.standard_normal((npts, 3))
        nang = {"pole": 1, "poles": 2}.get(dirs, dirs)
        th, ph = rng.uniform(0.0, np.pi, nang), rng.uniform(0.0, 2 * np.pi, nang)
        if dirs == "pole":
            th[0] = np.pi
        elif dirs == "poles" or f > 5e9:
            th[0], th[1] = 0.0, np.pi
        tag = f"{nang}dirs" if dirs == nang else dirs
        out[f"{npts}pts-{tag}-{f / 1e9:g}GHz"] = (pos, Js, Ms, 2 * np.pi * f / C0, th, ph)
    return out


_FF = {}


def farfield_ref_of(name):
    """(E_th, E_ph, S_a, K) of a case, computed once per process."""
    if name not in _FF:
        pos, Js, Ms, kw, th, ph = farfield_cases()[name]
        _FF[name] = (*farfield_reference(pos, Js, Ms, kw, th, ph), farfield_K(pos, kw))
    return _FF[name]


def farfield_ratio(got, ref):
    """|err| / (2^-53 S_a) of (E_th, E_ph) against a reference (E_th, E_ph, S_a, ...), per direction the largest of the four
    components (Re and Im of E_th, E_ph); where S_a = 0 the value must be an exact zero (ratio 0) and is infinitely off otherwise."""
    out = np.zeros(ref[2].shape[0])
    for c in range(2):
        d = np.asarray(got[c]).astype(np.clongdouble) - ref[c]
        err = np.maximum(np.abs(d.real), np.abs(d.imag)).astype(np.float64)
        S = ref[2][:, c]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(S > 0, err / (U * S), np.where(err == 0, 0.0, np.inf))
        out = np.maximum(out, r)
    return out


def test_farfield_reference_bar_holds_for_the_oracle_and_sees_two_mutations(oracle_lib):
    """The oracle (another float64 order of the same sums) stays inside the bar on every case, far inside; with the LAST POINT dropped
    from the reference it misses the bar in every direction, and with one direction's theta moved by 1e-9 in that direction —
    the bar sees an error of that size in the kernel."""
    capi = pkg("_capi")
    lines, Ks = [], []
    for name, (pos, Js, Ms, kw, th, ph) in farfield_cases().items():
        ref = farfield_ref_of(name)
        K = ref[3]
        Ks.append(K)
        got = capi.farfield(oracle_lib, pos, Js, Ms, kw, th, ph)
        ratio = farfield_ratio(got, ref)
        npts = pos.shape[0]
        if npts == 0:
            assert np.all(ref[2] == 0) and all(np.all(g == 0) for g in got)
            continue
        assert np.all(ref[2] > 0)
        lines.append(f"{name}: K = {K:.0f}, oracle at most {ratio.max():.3f} x 2^-53 S_a")
        assert ratio.max() <= K, (name, ratio.max())
        # a point dropped from the reference (the tail of the strided loop forgotten)
        short = farfield_reference(pos[:-1], Js[:-1], Ms[:-1], kw, th, ph)
        miss = farfield_ratio(got, (short[0], short[1], ref[2]))
        assert np.all(miss > K), (name, miss.min() / K)
        # one direction 1e-9 off (the clamp of the tail block taking the neighbour's angle would be off by far more)
        a = th.size // 2
        th2 = th.copy()
        th2[a] += 1e-9 if th2[a] < 3.0 else -1e-9
        moved = farfield_reference(pos, Js, Ms, kw, th2[a:a + 1], ph[a:a + 1])
        miss1 = farfield_ratio([g[a:a + 1] for g in got], (moved[0], moved[1], ref[2][a:a + 1]))
        assert miss1[0] > K, (name, miss1[0] / K)
        lines[-1] += f"; a point dropped: {miss.min() / K:.1e} K at least; theta + 1e-9: {miss1[0] / K:.1e} K"
    print("\n".join(lines))
    assert max(Ks) < 220          # 24 + 30 + 3 * 53 at the most: the 6000 points at 5.8 GHz
    _note("far field, oracle against the np.longdouble reference (test_farfield_reference_bar_holds_for_the_oracle_and_sees_two_mutations)", lines)


# ---- C. the recorder transform past eight frequencies ------------------------------------------------------------------------------
REC_SHAPE, REC_STEPS, REC_F0 = (64, 60, 36), 300, 2.45e9
REC_NFREQ = (1, 8, 9, 16, 17)
REC_ROWS = (0, 7, 8, 16)        # rows of the 17-frequency transform: first and last of the first pass, first of the second, the tail


def rec_freqs(nfreq):
    return np.array([REC_F0]) if nfreq == 1 else np.linspace(0.7 * REC_F0, 1.3 * REC_F0, nfreq)


def rec_sim(mode, freqs):
    return patch_sim(*REC_SHAPE, nr_ts=REC_STEPS, nf2ff_freqs=np.asarray(freqs, float), nf2ff_mode=mode)


def test_recorder_cases_take_a_second_pass_and_an_odd_box():
    """k_rec_dft<8>: 9 and 17 frequencies take a second and a third pass with one live frequency, 16 two full ones; the same
    sampling whatever the frequency set; and the scene's faces hold a box whose point count is no multiple of the block."""
    assert [(-(-n // 8), n % 8) for n in REC_NFREQ] == [(1, 1), (1, 0), (2, 1), (2, 0), (3, 1)]
    sims = [rec_sim("record", rec_freqs(17))] + [rec_sim("dft", rec_freqs(n)) for n in (9, 17)]
    assert len({(s.dft_every, s.dft_nsamples) for s in sims}) == 1 and sims[0].dft_nsamples >= 8
    assert all(rec_freqs(n).max() <= sims[0].nf2ff_fmax for n in REC_NFREQ)
    npts = [int(np.prod([h - l + 1 for l, h in zip(r.lo, r.hi)])) for r in sims[0].nf2ff_box.requests]
    assert len(npts) == 24 and any(n % 256 for n in npts) and max(npts) > 256
    print(f"recorder: {sims[0].dft_nsamples} samples every {sims[0].dft_every} steps; points per box {sorted(set(npts))}")


# ---- D. long probes ----------------------------------------------------------------------------------------------------------------
PRB_SHAPE, PRB_STEPS, PRB_CALLS = (40, 36, 20), 200, (1, 7, 61, 131)
PRB_LENGTHS = (1, 256, 257, 600)


def probe_sim(boundary):
    return patch_sim(*PRB_SHAPE, boundary=boundary, cpml_cells=4, nr_ts=PRB_STEPS, nf2ff=False)


def probe_rows(ny):
    """Rows j such that every strip of >= 4 rows of a grid of ny rows, and a shorter last one, holds one of them."""
    return sorted(set(range(0, ny, 4)) | {ny - 1})


def draw_probes(inner=False, seed=77):
    """[(kind, idx int64, comp int8, w float32)]: V- and I-probes of 1, 256, 257 and 600 entries, weights of both signs, all three
    components; the cells of the 257- and 600-entry ones lie in every plane k on every row of probe_rows (so in every strip-plane
    of any tiling with strips of >= 4 rows), the rest anywhere.  `inner`: no cell on a face of the grid (Mur faces)."""
    nx, ny, nz = PRB_SHAPE
    rng = np.random.default_rng(seed)
    lo, span = (1, (nx - 2, ny - 2, nz - 2)) if inner else (0, (nx, ny, nz))
    ks = range(1, nz - 1) if inner else range(nz)
    rows = [j for j in probe_rows(ny) if not inner or 0 < j < ny - 1]
    out = []
    for kind in (0, 1):
        for n in PRB_LENGTHS:
            cells = []
            if n > 256:
                cells = [(lo + int(rng.integers(span[0])), j, k) for k in ks for j in rows]
                assert len(cells) <= n
            while len(cells) < n:
                cells.append(tuple(lo + int(rng.integers(s)) for s in span))
            cells = np.array(cells, np.int64)[rng.permutation(n)]
            idx = (cells[:, 2] * ny + cells[:, 1]) * nx + cells[:, 0]
            comp = rng.integers(0, 3, n).astype(np.int8)
            w = (rng.uniform(0.25, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
            out.append((kind, idx, comp, w))
    return out


def strip_planes_covered(idx, rows_per_strip):
    """Does every strip-plane (plane k, strip of rows_per_strip rows) of PRB_SHAPE hold a cell of idx?"""
    nx, ny, nz = PRB_SHAPE
    k, j = idx // (nx * ny), (idx // nx) % ny
    nstrips = -(-ny // rows_per_strip)
    return len(set(zip(k.tolist(), (j // rows_per_strip).tolist()))) == nz * nstrips


def probe_sum_longdouble(fields, kind, idx, comp, w):
    """(sum w F, sum |w F|) over the fields [2][3][nz][ny][nx] in np.longdouble."""
    ld = np.longdouble
    F = np.stack([fields[kind][c].reshape(-1) for c in range(3)])[comp, idx].astype(ld)
    t = w.astype(ld) * F
    return np.sum(t), float(np.sum(np.abs(t)))


def add_probes(e, probes):
    return [e.add_probe(kind, idx, comp, w) for kind, idx, comp, w in probes]


def test_long_probes_cover_every_strip_plane_and_match_a_longdouble_sum(oracle_lib):
    """The probes on the oracle: drawn into every strip-plane of every tiling with strips of 4 rows or more, and the sample that
    belongs to the final fields (the last: V after the E update of the last timestep, I after its H update) against sum w F in
    np.longdouble — the oracle adds in order, n roundings at most."""
    nx, ny, nz = PRB_SHAPE
    for inner in (False, True):
        probes = draw_probes(inner)
        assert [p[1].size for p in probes] == list(PRB_LENGTHS) * 2
        for kind, idx, comp, w in probes:
            assert idx.min() >= 0 and idx.max() < nx * ny * nz and set(comp.tolist()) <= {0, 1, 2}
            if idx.size > 1:
                assert (w < 0).any() and (w > 0).any() and set(comp.tolist()) == {0, 1, 2}
            if idx.size > 256 and not inner:
                assert all(strip_planes_covered(idx, t) for t in range(4, ny + 1))
            if inner:
                i, j, k = idx % nx, (idx // nx) % ny, idx // (nx * ny)
                assert i.min() > 0 and i.max() < nx - 1 and j.min() > 0 and j.max() < ny - 1 and k.min() > 0 and k.max() < nz - 1
    assert sum(PRB_CALLS) == PRB_STEPS
    lines = []
    for boundary, inner in (("CPML", False), ("MUR", True)):
        probes = draw_probes(inner)
        s = probe_sim(boundary)
        e = s.build(oracle_lib)
        pids = add_probes(e, probes)
        seeded_fields(e, 9)
        e.run(PRB_STEPS)
        f = e.fields()
        assert np.isfinite(f).all() and np.abs(f).max() > 0
        for (kind, idx, comp, w), pid in zip(probes, pids):
            series = e.get_probe(pid)
            assert series.size == PRB_STEPS and np.abs(series).max() > 0
            want, scale = probe_sum_longdouble(f, kind, idx, comp, w)
            dev = float(abs(np.longdouble(series[-1]) - want))
            assert dev <= (idx.size + 1) * U * scale, (boundary, kind, idx.size, dev / (U * scale))
            lines.append(f"oracle, {boundary}, {'VI'[kind]}-probe of {idx.size}: |last sample - longdouble sum| = {dev / (U * scale):.3f} x 2^-53 sum |w F|")
    print("\n".join(lines))
