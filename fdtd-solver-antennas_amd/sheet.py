"""Conducting sheets: finite-conductivity metal as a surface impedance on the faces of PEC-voxelised metal
(openEMS users know it as ``CSX.AddConductingSheet(name, conductivity, thickness)``).

Model.  A conductor of conductivity sigma and thickness t, seen from one face:

    gamma = (1+j)/delta,  delta = sqrt(2/(w mu0 sigma)),  Z_c = gamma/sigma,  Z_s(w) = Z_c coth(gamma t),  Y_s = 1/Z_s

(DC limit 1/(sigma t); thick-conductor limit (1+j) R_s, R_s = sqrt(w mu0 / 2 sigma)).  The admittance is ONE-SIDED: exact for a
face whose current flows on one side only (a patch's underside, a ground plane's top, the inner wall of a cavity).  A zero-thickness
sheet that carries equal currents on both faces is over-charged by up to 2x (its loss is counted as if all the current flowed on
one face of the full conductance).

Y_s is fitted over a band [f_lo, f_hi] as  Y_s(jw) ~= G0 + sum_k c_k / (jw + p_k)  (K <= 8 fixed, log-spaced poles a decade beyond
each band edge; G0, c_k >= 0 by non-negative least squares on the relative error: RL branches, passive by construction) and
discretised for a timestep dt as alpha_k = exp(-p_k dt), b_k = c_k (1 - alpha_k) / p_k.  In EC units, with the branch currents at
half steps like curl I, an edge e of the sheet steps as

    C_e (V'-V)/dt + G_e (V'+V)/2 + sum_k i_k = curlI,      i_k' = alpha_k i_k + scale_e b_k (V'+V)/2

The implicit b_k part is folded into the edge's conductance, G_e += scale_e (G0 + sum_k b_k) (the lumped-edge overrides of the
operator build); what remains is the sparse correction of include/fdtd_hip_sheet.h (csrc/sheet.hip; ``correction`` below restates
it in numpy, operation for operation).

Geometry.  scale_e = w_e / l_e: l_e the primal edge length, w_e the length of the metal surface's trace across the edge's dual
face — the dual width inside a sheet, half of it at a sheet's rim.  A grid face is a metal surface face when its four nodes lie in a
box of the metal and not both cells beside it are filled by that metal (a cell is filled when its centre lies inside a box).  Sheet
metals of the same conductivity and thickness share one surface (scene.voxelize), so a patch and the feed line drawn against it meet
inside one conductor rather than at two rims.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple
import numpy as np

from .constants import MU0

MAX_K = 8


# ---- surface impedance ---------------------------------------------------------------------------------
def Z_s(f, sigma: float, t: float) -> np.ndarray:
    """Surface impedance [ohm] of one face of a conductor (sigma [S/m], thickness t [m]) at frequencies f [Hz]."""
    f = np.atleast_1d(np.asarray(f, float))
    out = np.empty(f.shape, np.complex128)
    dc = f <= 0
    out[dc] = 1.0 / (sigma * t)
    w = 2 * np.pi * f[~dc]
    delta = np.sqrt(2.0 / (w * MU0 * sigma))
    gamma = (1 + 1j) / delta
    x = gamma * t
    # coth x = (1 + e^-2x) / (1 - e^-2x), overflow-free for Re x > 0 and accurate for small |x|
    em = np.exp(-2 * x)
    coth = (1 + em) / (-np.expm1(-2 * x))
    out[~dc] = gamma / sigma * coth
    return out


def Y_s(f, sigma: float, t: float) -> np.ndarray:
    return 1.0 / Z_s(f, sigma, t)


# ---- rational fit -----------------------------------------------------------------------------------
@dataclass
class SheetFit:
    sigma: float
    thickness: float
    f_lo: float
    f_hi: float
    poles: np.ndarray        # p_k [1/s]
    c: np.ndarray            # c_k [S/s]
    G0: float                # [S]
    band_error: float        # max relative error |Y_fit - Y_s| / |Y_s| over the band

    def Y(self, f) -> np.ndarray:
        jw = 2j * np.pi * np.atleast_1d(np.asarray(f, float))
        return self.G0 + np.sum(self.c[:, None] / (jw[None, :] + self.poles[:, None]), axis=0)

    def discretise(self, dt: float):
        """(alpha_k, b_k) float64 for timestep dt."""
        alpha = np.exp(-self.poles * dt)
        b = self.c * (-np.expm1(-self.poles * dt)) / self.poles
        return alpha, b

    def implicit_G(self, dt: float) -> float:
        """G0 + sum_k b_k [S]: the conductance per square folded into the operator."""
        return float(self.G0 + np.sum(self.discretise(dt)[1]))


def fit_band(f0: float, fc: float) -> Tuple[float, float]:
    """The default fit band: the excitation band [max(0, f0 - fc), f0 + fc]."""
    return max(0.0, f0 - fc), f0 + fc


def _nnls_fit(f, y, poles):
    from scipy.optimize import nnls
    jw = 2j * np.pi * f
    cols = np.concatenate([np.ones((f.size, 1)), poles[None, :] / (jw[:, None] + poles[None, :])], axis=1)   # unknowns G0, c_k / p_k
    wgt = 1.0 / np.abs(y)
    A = np.concatenate([(cols * wgt[:, None]).real, (cols * wgt[:, None]).imag])
    rhs = np.concatenate([(y * wgt).real, (y * wgt).imag])
    x, _ = nnls(A, rhs)
    return x, float(np.max(np.abs(cols @ x - y) / np.abs(y)))


def fit(sigma: float, thickness: float, f_lo: float, f_hi: float, K: int = MAX_K, nsamples: int = 400) -> SheetFit:
    """Fit Y_s over [f_lo, f_hi] (f_lo = 0: the fit covers [f_hi / 100, f_hi], where an FDTD pulse's energy lies).  K poles
    log-spaced from 2 pi f_lo / s_lo to 2 pi f_hi s_hi, with the margins s_lo, s_hi in 3 ... 30 (about a decade beyond each band
    edge) that give the smallest band error; G0, c_k >= 0 by NNLS on the relative error."""
    if not (0 < K <= MAX_K):
        raise ValueError(f"K must be 1..{MAX_K}")
    if not (f_hi > 0 and 0 <= f_lo < f_hi):
        raise ValueError("fit band must satisfy 0 <= f_lo < f_hi")
    lo = max(f_lo, f_hi / 100.0)
    f = np.unique(np.concatenate([np.geomspace(lo, f_hi, nsamples // 2), np.linspace(lo, f_hi, nsamples // 2)]))
    y = Y_s(f, sigma, thickness)
    best = None
    for s_lo in (3.0, 5.0, 10.0, 30.0):
        for s_hi in (3.0, 5.0, 10.0, 30.0):
            poles = 2 * np.pi * np.geomspace(lo / s_lo, f_hi * s_hi, K)
            x, err = _nnls_fit(f, y, poles)
            if best is None or err < best[2]:
                best = (poles, x, err)
    poles, x, err = best
    return SheetFit(float(sigma), float(thickness), float(f_lo), float(f_hi), poles, x[1:] * poles, float(x[0]), err)


# ---- per-edge geometry ------------------------------------------------------------------------------
@dataclass
class SheetMetal:
    name: str
    conductivity: float
    thickness: float


@dataclass
class SheetEdges:
    """The sheet edges of a voxelised scene (global flat node index, component, scale_e = w_e / l_e, index into `metals`)."""
    idx: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    comp: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int8))
    scale: np.ndarray = field(default_factory=lambda: np.zeros(0, np.float64))
    metal: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    metals: List[SheetMetal] = field(default_factory=list)

    def __len__(self):
        return int(self.idx.size)


def _shift(a: np.ndarray, axis: int, s: int) -> np.ndarray:
    """out[pos] = a[pos + s * e_axis] (physical axis), False / 0 outside."""
    npa = 2 - axis
    out = np.zeros_like(a)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if s > 0:
        src[npa] = slice(s, None); dst[npa] = slice(0, -s)
    else:
        src[npa] = slice(0, s); dst[npa] = slice(-s, None)
    out[tuple(dst)] = a[tuple(src)]
    return out


def surface_faces(node_masks: Sequence[np.ndarray], filled: np.ndarray):
    """Metal surface faces per normal axis, [nz][ny][nx] at the face's lowest node.  node_masks: per box, bool [nz][ny][nx] of
    the nodes inside it; filled: bool [nz][ny][nx] of the cells (lowest node) filled by the metal."""
    S = []
    for n in range(3):
        a, b = (n + 1) % 3, (n + 2) % 3
        F = np.zeros_like(filled)
        for nm in node_masks:
            F |= nm & _shift(nm, a, 1) & _shift(nm, b, 1) & _shift(_shift(nm, a, 1), b, 1)
        both = _shift(filled, n, -1) & filled
        S.append(F & ~both)
    return S


def edge_geometry(grid, comp: int, cand: np.ndarray, S, filled: np.ndarray):
    """(sheet mask, w_e / l_e) of the comp-directed candidate edges `cand` (bool [nz][ny][nx])."""
    nx, ny, nz = grid.shape
    c = comp
    a1, a2 = (c + 1) % 3, (c + 2) % 3
    shp = (1, 1, 1)

    def along(a, arr):
        s = [1, 1, 1]
        s[2 - a] = arr.size
        return arr.reshape(s)

    half = [np.concatenate([np.diff(l), [0.0]]) * 0.5 for l in grid.lines]           # half of the cell above node q
    half_lo = [np.concatenate([[0.0], np.diff(l)]) * 0.5 for l in grid.lines]        # half of the cell below node q
    w = (S[a2] * along(a1, half[a1]) + _shift(S[a2], a1, -1) * along(a1, half_lo[a1])
         + S[a1] * along(a2, half[a2]) + _shift(S[a1], a2, -1) * along(a2, half_lo[a2]))
    nfill = (filled.astype(np.int8) + _shift(filled, a1, -1) + _shift(filled, a2, -1) + _shift(_shift(filled, a1, -1), a2, -1))
    sheet = cand & (nfill < 4) & (w > 0)
    # edges on the outermost grid planes stay PEC
    n = (nx, ny, nz)
    for a in (a1, a2):
        idx = [slice(None)] * 3
        idx[2 - a] = 0
        sheet[tuple(idx)] = False
        idx[2 - a] = n[a] - 1
        sheet[tuple(idx)] = False
    idx = [slice(None)] * 3
    idx[2 - c] = n[c] - 1
    sheet[tuple(idx)] = False
    l = along(c, np.concatenate([np.diff(grid.lines[c]), [1.0]]))
    return sheet, np.broadcast_to(w / l, sheet.shape)


def check_placement(grid, sheets: SheetEdges, *, mur_faces: Sequence[int] = (0,) * 6, dft_boxes=()):
    """Refuse (ValueError) sheet edges on a Mur face node or its first interior layer, or inside a V-DFT / NF2FF box
    (`dft_boxes`: (kind, comp, lo, hi) with kind 0 = V): there the correction would not commute with the rest of the E phase."""
    if not len(sheets):
        return
    nx, ny, nz = grid.shape
    n = (nx, ny, nz)
    k, r = np.divmod(sheets.idx, nx * ny)
    j, i = np.divmod(r, nx)
    pos = (i, j, k)
    for f in range(6):
        if not mur_faces[f]:
            continue
        a = f // 2
        bad = pos[a] >= n[a] - 2 if f % 2 else pos[a] <= 1
        if np.any(bad):
            e = int(np.argmax(bad))
            raise ValueError(f"conducting sheet edge at node {(int(i[e]), int(j[e]), int(k[e]))} lies on the Mur face "
                             f"{'xyz'[a]}{'+' if f % 2 else '-'} or its first interior layer")
    for kind, comp, lo, hi in dft_boxes:
        if kind != 0:
            continue
        bad = sheets.comp == comp
        for a in range(3):
            bad &= (pos[a] >= lo[a]) & (pos[a] <= hi[a])
        if np.any(bad):
            e = int(np.argmax(bad))
            raise ValueError(f"conducting sheet edge at node {(int(i[e]), int(j[e]), int(k[e]))} lies inside a voltage DFT / NF2FF box")


# ---- the correction, restated ---------------------------------------------------------------------------
def class_tables(sheets: SheetEdges, fits: Sequence[SheetFit], dt: float, K: int):
    """(cls int32 [n], alpha float32 [ncls][K], b float32 [ncls][K]) with one class per (metal, scale_e): b = scale_e * b_k."""
    keys = np.stack([sheets.metal.astype(np.float64), sheets.scale])
    uniq, cls = np.unique(keys, axis=1, return_inverse=True)
    alpha = np.zeros((uniq.shape[1], K), np.float32)
    b = np.zeros((uniq.shape[1], K), np.float32)
    for q in range(uniq.shape[1]):
        fa, fb = fits[int(uniq[0, q])].discretise(dt)
        alpha[q] = fa
        b[q] = uniq[1, q] * fb
    return cls.astype(np.int32).ravel(), alpha, b


def correction(V: np.ndarray, vi: np.ndarray, vprev: np.ndarray, ib: np.ndarray, alpha: np.ndarray, b: np.ndarray):
    """The per-timestep correction of include/fdtd_hip_sheet.h in float32, statement for statement.  V, vi, vprev: [n];
    ib: [K][n] (updated in place); alpha, b: [K][n] (the edge's class rows).  Returns V_new (also the new vprev)."""
    f32 = np.float32
    S = np.zeros(V.shape, f32)
    for k in range(ib.shape[0]):
        S = S + alpha[k] * ib[k]
    v = V - vi * S
    avg = f32(0.5) * (v + vprev)
    for k in range(ib.shape[0]):
        ib[k] = alpha[k] * ib[k] + b[k] * avg
    return v
