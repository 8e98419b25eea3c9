"""Dispersive dielectrics: multi-pole Debye media, and the constant-loss-tangent substrate built from them.

Why.  A plain material turns a loss tangent into ONE conductivity, kappa = w0 eps0 eps_r tan_delta: the requested tan delta at the
design frequency only, tan_delta * f0 / f everywhere else.  A substrate such as FR-4 has a nearly constant loss tangent over
decades (Djordjevic-Sarkar): a sum of Debye relaxations with log-spaced relaxation frequencies and equal weights gives exactly
that, and Kramers-Kronig then forces the slight fall of Re eps with frequency that real laminates show.

Model.
    eps(w) = eps_inf + sum_k deps_k / (1 + j w tau_k) - j kappa / (w eps0),        deps_k >= 0, tau_k > 0, eps_inf >= 1
(passive; eps_inf >= 1 keeps the Courant limit no worse than vacuum's — grid.courant_dt uses the vacuum speed whatever eps is).

Scheme (include/fdtd_hip_dispersion.h spells the fp32 order; csrc/dispersion.hip runs it, ``correction`` below restates it in numpy
operation for operation).  Each pole is a series R-C branch across the edge capacitance, its state u_k the branch capacitor's voltage.
With Vm = (V_new + V_prev)/2 held over the step,

    u_k <- alpha_k u_k + (1 - alpha_k) Vm,                  alpha_k = exp(-dt / tau_k)
    mean branch current = w_e beta_k (Vm - u_k),            beta_k = eps0 deps_k (1 - alpha_k) / dt

(the exact integral of the branch current for a constant Vm).  w_e [m] is the share of the edge's A~/l that lies in the medium: the
area-weighted four-cell average ecoperator._edge_average applies to eps and kappa, applied to the medium's indicator.  The Vm part is
a conductance and linear in per-cell values, so it folds exactly into the per-cell kappa handed to the operator build:

    kappa_cell = kappa + sum_k beta_k,        eps_cell = eps_inf

and the class count of the operator grows by at most the number of media.  The rest, -w_e sum_k beta_k u_k on the left of the edge's
equation, is the per-timestep correction.  Its bias against Re eps / -Im eps is first order in w dt (about -0.7 % at w dt = 0.03).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple
import numpy as np

from .constants import EPS0

MAX_K = 8
MAX_MEDIA = 8
TAN_DELTA_BAR = 0.02      # fit_constant_loss_tangent: largest relative error of tan delta over the band it accepts


# ---- the medium -------------------------------------------------------------------------------------
@dataclass
class DebyeMedium:
    eps_inf: float
    kappa: float
    delta_eps: np.ndarray      # [K]
    tau: np.ndarray            # [K] seconds
    fit_info: Optional[dict] = None    # fit_constant_loss_tangent: target, band and the errors reached

    def __post_init__(self):
        self.eps_inf, self.kappa = float(self.eps_inf), float(self.kappa)
        self.delta_eps = np.atleast_1d(np.asarray(self.delta_eps, np.float64)).copy()
        self.tau = np.atleast_1d(np.asarray(self.tau, np.float64)).copy()
        if self.delta_eps.ndim != 1 or self.delta_eps.shape != self.tau.shape or not (1 <= self.delta_eps.size <= MAX_K):
            raise ValueError(f"a Debye medium has 1..{MAX_K} poles: delta_eps and tau of equal length")
        if np.any(self.delta_eps < 0) or np.any(self.tau <= 0) or self.kappa < 0 or self.eps_inf < 1:
            raise ValueError("a Debye medium needs delta_eps >= 0, tau > 0, kappa >= 0 and eps_inf >= 1 (passivity; a Courant limit no worse than vacuum's)")

    @property
    def K(self) -> int:
        return int(self.tau.size)

    def key(self) -> tuple:
        """Media with the same key are one medium."""
        return (self.eps_inf, self.kappa, tuple(self.delta_eps.tolist()), tuple(self.tau.tolist()))

    def eps(self, f) -> np.ndarray:
        """Complex relative permittivity at frequencies f [Hz] (> 0), e^{+jwt} convention: Im eps <= 0."""
        w = 2 * np.pi * np.atleast_1d(np.asarray(f, float))
        e = self.eps_inf + np.sum(self.delta_eps[:, None] / (1 + 1j * w[None, :] * self.tau[:, None]), axis=0)
        return e - 1j * self.kappa / (w * EPS0)

    def tan_delta(self, f) -> np.ndarray:
        e = self.eps(f)
        return -e.imag / e.real

    def discretise(self, dt: float):
        """(alpha_k, beta_k) float64 for timestep dt: alpha_k = exp(-dt/tau_k), beta_k = eps0 deps_k (1 - alpha_k) / dt [S/m]."""
        alpha = np.exp(-dt / self.tau)
        beta = EPS0 * self.delta_eps * (-np.expm1(-dt / self.tau)) / dt
        return alpha, beta

    def one_minus_alpha(self, dt: float) -> np.ndarray:
        return -np.expm1(-dt / self.tau)

    def folded(self, dt: float) -> Tuple[float, float]:
        """(eps_cell, kappa_cell) handed to the operator build for a cell of this medium."""
        return self.eps_inf, self.kappa + float(np.sum(self.discretise(dt)[1]))


# ---- constant loss tangent --------------------------------------------------------------------------
def _fit_once(eps_r, tan_delta, f_ref, f, K, margin):
    from scipy.optimize import nnls
    w = 2 * np.pi * f
    tau = 1.0 / (2 * np.pi * np.geomspace(f[0] / margin, f[-1] * margin, K))
    x = w[:, None] * tau[None, :]
    A_im = x / (1 + x * x)                    # -Im of 1 / (1 + j w tau)
    A_re = 1.0 / (1 + x * x)
    xr = 2 * np.pi * f_ref * tau
    re = np.full(f.shape, float(eps_r))       # Re eps(f) of the previous iterate: the target is -Im eps = tan_delta * Re eps
    d = np.zeros(K)
    for _ in range(6):
        d, _ = nnls(A_im / re[:, None], np.full(f.size, float(tan_delta)))
        eps_inf = eps_r - float(np.sum(d / (1 + xr * xr)))
        re = eps_inf + A_re @ d
    return eps_inf, d, tau


def fit_constant_loss_tangent(eps_r: float, tan_delta: float, f_ref: float, f_lo: float, f_hi: float, K: Optional[int] = None,
                              nsamples: int = 200) -> DebyeMedium:
    """A Debye medium whose tan delta(f) stays within TAN_DELTA_BAR (2 %) of `tan_delta` over [f_lo, f_hi] and whose Re eps(f_ref)
    is eps_r exactly.  Relaxation frequencies log-spaced over about [f_lo / 3, 3 f_hi] (the margin in 2 ... 5 that fits best),
    delta_eps_k >= 0 by non-negative least squares.  K = None: the fewest poles from 3 up that meet the bar (bands up to about 3:1
    take 3, wider ones more); a given K that cannot meet it, or K = 8 failing, raises ValueError instead of returning a worse fit."""
    if not (eps_r >= 1 and tan_delta > 0 and 0 < f_lo < f_hi and f_lo <= f_ref <= f_hi):
        raise ValueError("fit_constant_loss_tangent: need eps_r >= 1, tan_delta > 0 and 0 < f_lo <= f_ref <= f_hi, f_lo < f_hi")
    if K is not None and not (1 <= int(K) <= MAX_K):
        raise ValueError(f"K must be 1..{MAX_K}")
    f = np.geomspace(f_lo, f_hi, nsamples)
    last = None
    for k in ([int(K)] if K is not None else range(3, MAX_K + 1)):
        best = None
        for margin in (2.0, 2.5, 3.0, 4.0, 5.0):
            eps_inf, d, tau = _fit_once(eps_r, tan_delta, f_ref, f, k, margin)
            if eps_inf < 1.0:
                continue
            med = DebyeMedium(eps_inf, 0.0, d, tau)
            e = med.eps(f)
            err_t = float(np.max(np.abs(-e.imag / e.real / tan_delta - 1.0)))
            err_e = float(np.max(np.abs(e.real / eps_r - 1.0)))
            if best is None or err_t < best[0]:
                best = (err_t, err_e, med)
        if best is None:
            continue
        last = best
        if best[0] <= TAN_DELTA_BAR:
            err_t, err_e, med = best
            med.fit_info = {"eps_r": float(eps_r), "tan_delta": float(tan_delta), "f_ref": float(f_ref), "f_lo": float(f_lo),
                            "f_hi": float(f_hi), "tan_delta_error": err_t, "eps_error": err_e}
            return med
    got = "no passive fit with eps_inf >= 1" if last is None else f"tan delta error {100 * last[0]:.1f} %"
    raise ValueError(f"fit_constant_loss_tangent: {'K = %d' % K if K is not None else 'K up to %d' % MAX_K} cannot hold tan delta within "
                     f"{100 * TAN_DELTA_BAR:.0f} % over {f_lo / 1e9:.3g}-{f_hi / 1e9:.3g} GHz ({got})"
                     + ("; leave K unset to let it grow" if K is not None else "; narrow the band"))


def substrate_band(f0: float, fc: float) -> Tuple[float, float]:
    """The band a prepare_hip_* substrate is fitted over: the excitation band [f0 - fc, f0 + fc], its lower edge no lower than
    (f0 + fc) / 3.1 — below that a Gaussian pulse carries next to no energy, and three poles cover a 3.1 : 1 band."""
    f_hi = f0 + fc
    return min(max(f0 - fc, f_hi / 3.1), f0), f_hi


# ---- geometry: weights and boxes -------------------------------------------------------------------
@dataclass
class DebyeEdges:
    """The dispersive edges of a voxelised scene: the media (merged), the cells' medium ids (-1: none), and per component the
    bounding box of the edges with w_e != 0 — lo, hi (exclusive) as (x, y, z) node indices — with w_e [m] and the medium id
    (uint8) over it, [z][y][x]."""
    media: List[DebyeMedium] = field(default_factory=list)
    names: List[List[str]] = field(default_factory=list)          # the scene materials merged into each medium
    cell_medium: Optional[np.ndarray] = None                      # int8 [nz-1][ny-1][nx-1]
    lo: List[Tuple[int, int, int]] = field(default_factory=list)
    hi: List[Tuple[int, int, int]] = field(default_factory=list)
    w: List[np.ndarray] = field(default_factory=list)
    med: List[np.ndarray] = field(default_factory=list)

    def __len__(self):
        return int(sum(np.count_nonzero(w) for w in self.w))

    @property
    def K(self) -> int:
        return max(m.K for m in self.media)


def edge_weights(grid, cell_medium: np.ndarray, nmedia: int, names: Optional[Sequence[str]] = None, kind: str = "Debye"):
    """Per component (w [nz][ny][nx] float64, medium id [nz][ny][nx] uint8): w_e = A~/l times the area-weighted four-cell share of
    the edge that lies in its medium (ecoperator._edge_average of the medium's indicator); 0 where no cell around the edge is
    dispersive and on the edges that do not exist.  An edge whose cells belong to two different media is refused (`kind`: what the
    message calls the media — lorentz.py shares this function)."""
    from .ecoperator import _edge_average
    nx, ny, nz = grid.shape
    out = []
    for c in range(3):
        a1, a2 = (c + 1) % 3, (c + 2) % 3

        def along(a, arr):
            s = [1, 1, 1]
            s[2 - a] = arr.size
            return arr.reshape(s)

        geo = along(a1, grid.dd[a1]) * along(a2, grid.dd[a2]) / along(c, grid.d[c])
        w = np.zeros((nz, ny, nx))
        med = np.zeros((nz, ny, nx), np.uint8)
        for m in range(nmedia):
            share = _edge_average((cell_medium == m).astype(np.float64), grid, c)
            idx = [slice(None)] * 3
            idx[2 - c] = -1
            share[tuple(idx)] = 0.0                       # the last edges along c do not exist
            on = share > 0
            clash = on & (w > 0)
            if np.any(clash):
                k, j, i = (int(v[0]) for v in np.nonzero(clash))
                other = int(med[k, j, i])
                nm = (lambda q: names[q] if names else str(q))
                raise ValueError(f"the {'xyz'[c]}-edge at node {(i, j, k)} is shared by two different {kind} media "
                                 f"('{nm(other)}' and '{nm(m)}'): give them the same parameters or separate them by a cell")
            w[on] = (share * geo)[on]
            med[on] = m
        out.append((w, med))
    return out


def bounding_boxes(weights) -> Tuple[list, list, list, list]:
    """(lo, hi, w, med) per component: the tight box of the edges with w != 0, cropped arrays (empty component: lo = hi = 0s)."""
    lo, hi, ws, ms = [], [], [], []
    for w, med in weights:
        nz_ = np.nonzero(w)
        if nz_[0].size == 0:
            lo.append((0, 0, 0)); hi.append((0, 0, 0))
            ws.append(np.zeros((0, 0, 0), np.float32)); ms.append(np.zeros((0, 0, 0), np.uint8))
            continue
        k0, j0, i0 = (int(v.min()) for v in nz_)
        k1, j1, i1 = (int(v.max()) + 1 for v in nz_)
        lo.append((i0, j0, k0)); hi.append((i1, j1, k1))
        ws.append(np.ascontiguousarray(w[k0:k1, j0:j1, i0:i1]))
        ms.append(np.ascontiguousarray(med[k0:k1, j0:j1, i0:i1]))
    return lo, hi, ws, ms


def make_edges(grid, media: Sequence[DebyeMedium], names, cell_medium: np.ndarray) -> DebyeEdges:
    flat = [" / ".join(n) for n in names]
    lo, hi, w, med = bounding_boxes(edge_weights(grid, cell_medium, len(media), flat))
    return DebyeEdges(list(media), [list(n) for n in names], cell_medium, lo, hi, w, med)


def check_placement(grid, cell_medium: np.ndarray, cpml_cells: Sequence[int], names: Optional[Sequence[str]] = None, kind: str = "Debye"):
    """Refuse (ValueError) dispersive cells inside CPML layers (`cpml_cells`: layer thickness in cells per face, x-, x+, y-, ...):
    the layers' psi recursion assumes the folded eps / kappa only."""
    n = grid.shape
    for f in range(6):
        t = int(cpml_cells[f])
        if t <= 0:
            continue
        a = f // 2
        sl = [slice(None)] * 3
        sl[2 - a] = slice(n[a] - 1 - t, None) if f % 2 else slice(0, t)
        sub = cell_medium[tuple(sl)]
        if np.any(sub >= 0):
            m = int(sub[sub >= 0][0])
            raise ValueError(f"{kind} medium '{names[m] if names else m}' reaches into the CPML layer {'xyz'[a]}{'+' if f % 2 else '-'} "
                             f"({t} cells): dispersive cells inside absorbing layers are not supported — end the medium before the "
                             f"layer or use Mur faces")


# ---- tables and the correction, restated ----------------------------------------------------------------
def tables(media: Sequence[DebyeMedium], dt: float, K: Optional[int] = None):
    """(alpha, oma, beta) float32 [nmedia][K] of fdtd_debye_set: oma = 1 - alpha; media with fewer poles are padded with beta = 0."""
    K = max(m.K for m in media) if K is None else int(K)
    alpha = np.ones((len(media), K), np.float32)
    oma = np.zeros((len(media), K), np.float32)
    beta = np.zeros((len(media), K), np.float32)
    for q, m in enumerate(media):
        a, b = m.discretise(dt)
        alpha[q, :m.K], oma[q, :m.K], beta[q, :m.K] = a, m.one_minus_alpha(dt), b
    return alpha, oma, beta


def correction(V: np.ndarray, vi: np.ndarray, w: np.ndarray, vprev: np.ndarray, u: np.ndarray,
               alpha: np.ndarray, oma: np.ndarray, beta: np.ndarray) -> np.ndarray:
    """The per-timestep correction of include/fdtd_hip_dispersion.h in float32, statement for statement.  V, vi, w, vprev: any
    one shape (float32); u: [K] + that shape; alpha, oma, beta: [K] + that shape or [K] scalars broadcast (the edge's medium
    rows).  Edges with w == 0 keep V, u and vprev.  u and vprev are updated in place; returns V_new."""
    f32 = np.float32
    K = u.shape[0]
    bc = lambda t, k: t[k] if t.ndim > 1 else f32(t[k])
    S = np.zeros(V.shape, f32)
    for k in range(K):
        t = w * bc(beta, k)
        p = t * u[k]
        S = S + p
    q = vi * S
    vn = V + q
    s = vn + vprev
    avg = f32(0.5) * s
    on = w != 0
    for k in range(K):
        a = bc(alpha, k) * u[k]
        b = bc(oma, k) * avg
        u[k] = np.where(on, a + b, u[k])
    out = np.where(on, vn, V)
    vprev[...] = np.where(on, vn, vprev)
    return out


def branch_energy(dis: "DebyeEdges", u: Sequence[np.ndarray]) -> float:
    """Energy stored in the branch capacitors, 1/2 sum C_k u_k^2 with C_k = eps0 deps_k w_e; u[c]: [K] + box shape."""
    tot = 0.0
    for c in range(3):
        if dis.w[c].size == 0:
            continue
        for k in range(u[c].shape[0]):
            d = np.array([m.delta_eps[k] if k < m.K else 0.0 for m in dis.media])[dis.med[c]]
            tot += 0.5 * EPS0 * float(np.sum(d * dis.w[c] * u[c][k].astype(np.float64) ** 2))
    return tot
