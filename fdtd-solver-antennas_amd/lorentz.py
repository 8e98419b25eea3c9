"""Resonant dielectrics: Lorentz and Drude poles (openEMS users know them as ``CSX.AddLorentzMaterial``).

Why.  A sum of Debye relaxations (dispersion.py) has no resonance and Re eps never falls below eps_inf: plasmas, Drude conductors above
their collision frequency, artificial (metamaterial) loadings and laminate datasheets fitted with resonant terms need poles of second
order.

Model.
    eps(w) = eps_inf (1 + sum_k wp_k^2 / (w0_k^2 - w^2 + j w gamma_k)) - j kappa / (w eps0),    wp_k > 0, w0_k >= 0, gamma_k >= 0,
                                                                                               eps_inf >= 1, 1..4 poles
(w0_k = 0: a Drude pole; e^{+jwt} convention, Im eps <= 0; eps_inf >= 1 keeps the Courant limit no worse than vacuum's).

Scheme (include/fdtd_hip_lorentz.h spells the fp32 order; csrc/lorentz.hip runs it, ``correction`` below restates it in numpy operation
for operation).  Each pole is a series R-L-C branch (R-L for a Drude pole) across the edge capacitance.  Per unit of the edge weight
w_e [m] — the share of the edge's A~/l that lies in the medium, dispersion.edge_weights —

    l_k = 1 / (eps0 eps_inf wp_k^2),    r_k = gamma_k l_k,    c_k = eps0 eps_inf wp_k^2 / w0_k^2  (absent for a Drude pole)
    states (j_k, u_k):  l dj/dt = v - r j - u,  c du/dt = j;        the branch current of an edge is w_e j_k

which is the series element of lumped.py, and is discretised BY it (lumped.Element.discretise: trapezoidal rule driven by
Vm = (V_new + V_prev)/2) into Phi [2][2], Gam [2], h [2] and g0 per (medium, pole): passive, the Courant limit untouched, the discrete
admittance the continuous one at the warped frequency s_d = j (2/dt) tan(w dt/2).  g0 is a conductance per unit weight and linear in
per-cell values, so it folds exactly into the per-cell kappa handed to the operator build:

    kappa_cell = kappa + sum_k g0_k,        eps_cell = eps_inf

and the class count of the operator grows by at most the number of media.  The rest, w_e sum_k h_k . x_k on the edge's equation, is
the per-timestep correction.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple
import numpy as np

from .constants import EPS0
from . import dispersion as _disp
from . import lumped as _lumped

MAX_K = 4
MAX_MEDIA = 8


# ---- the medium -------------------------------------------------------------------------------------
@dataclass
class LorentzMedium:
    eps_inf: float
    kappa: float
    wp: np.ndarray             # [K] plasma frequencies, rad/s
    w0: np.ndarray = ()        # [K] pole frequencies, rad/s (0, or left out: Drude poles)
    gamma: np.ndarray = ()     # [K] collision / damping rates, 1/s (left out: loss-free poles)

    def __post_init__(self):
        self.eps_inf, self.kappa = float(self.eps_inf), float(self.kappa)
        self.wp = np.atleast_1d(np.asarray(self.wp, np.float64)).copy()
        K = self.wp.size
        fill = lambda v: np.zeros(K) if np.size(v) == 0 else np.atleast_1d(np.asarray(v, np.float64)).copy()
        self.w0, self.gamma = fill(self.w0), fill(self.gamma)
        if self.wp.ndim != 1 or self.w0.shape != self.wp.shape or self.gamma.shape != self.wp.shape or not (1 <= K <= MAX_K):
            raise ValueError(f"a Lorentz medium has 1..{MAX_K} poles: wp, w0 and gamma of equal length")
        ok = np.all(np.isfinite(self.wp)) and np.all(np.isfinite(self.w0)) and np.all(np.isfinite(self.gamma))
        if not ok or np.any(self.wp <= 0) or np.any(self.w0 < 0) or np.any(self.gamma < 0) or not (self.kappa >= 0) or not (self.eps_inf >= 1):
            raise ValueError("a Lorentz medium needs wp > 0, w0 >= 0, gamma >= 0, kappa >= 0 and eps_inf >= 1 (passivity; a Courant "
                             "limit no worse than vacuum's)")

    @property
    def K(self) -> int:
        return int(self.wp.size)

    def key(self) -> tuple:
        """Media with the same key are one medium."""
        return (self.eps_inf, self.kappa, tuple(self.wp.tolist()), tuple(self.w0.tolist()), tuple(self.gamma.tolist()))

    def eps(self, f) -> np.ndarray:
        """Complex relative permittivity at frequencies f [Hz] (> 0), e^{+jwt} convention: Im eps <= 0."""
        w = 2 * np.pi * np.atleast_1d(np.asarray(f, float))
        chi = np.sum(self.wp[:, None] ** 2 / (self.w0[:, None] ** 2 - w[None, :] ** 2 + 1j * w[None, :] * self.gamma[:, None]), axis=0)
        return self.eps_inf * (1 + chi) - 1j * self.kappa / (w * EPS0)

    def branches(self) -> List[_lumped.Element]:
        """The poles as series elements per unit of edge weight: R = gamma l [ohm m], L = l [H m], C = c [F/m] (None: a Drude pole)."""
        out = []
        for k in range(self.K):
            l = 1.0 / (EPS0 * self.eps_inf * self.wp[k] ** 2)
            c = None if self.w0[k] == 0 else EPS0 * self.eps_inf * self.wp[k] ** 2 / self.w0[k] ** 2
            out.append(_lumped.Element(f"pole {k}", R=self.gamma[k] * l, L=l, C=c, kind="series"))
        return out

    def discretise(self, dt: float):
        """(Phi [K][2][2], Gam [K][2], h [K][2], g0 [K]) float64 for timestep dt, per unit weight: lumped.Element.discretise of
        every branch.  A Drude pole leaves the second row and column of its Phi, Gam[1] and h[1] at zero."""
        d = [b.discretise(dt) for b in self.branches()]
        return (np.array([q[0] for q in d]), np.array([q[1] for q in d]), np.array([q[2] for q in d]), np.array([q[3] for q in d]))

    def folded(self, dt: float) -> Tuple[float, float]:
        """(eps_cell, kappa_cell) handed to the operator build for a cell of this medium."""
        return self.eps_inf, self.kappa + float(np.sum(self.discretise(dt)[3]))

    def energy_weights(self) -> np.ndarray:
        """[K][2]: the energy stored per unit weight is sum_k weights[k][0] j_k^2 + weights[k][1] u_k^2 (1/2 l, 1/2 c)."""
        return np.array([b.energy_weights() for b in self.branches()])


# ---- geometry ---------------------------------------------------------------------------------------
@dataclass
class LorentzEdges(_disp.DebyeEdges):
    """The dispersive edges of a voxelised scene, in the layout of dispersion.DebyeEdges: media are LorentzMedium."""


def make_edges(grid, media: Sequence[LorentzMedium], names, cell_medium: np.ndarray) -> LorentzEdges:
    flat = [" / ".join(n) for n in names]
    lo, hi, w, med = _disp.bounding_boxes(_disp.edge_weights(grid, cell_medium, len(media), flat, kind="Lorentz"))
    return LorentzEdges(list(media), [list(n) for n in names], cell_medium, lo, hi, w, med)


def check_disjoint(lor: "LorentzEdges", deb: Optional[_disp.DebyeEdges]):
    """Refuse (ValueError) an edge shared by a Lorentz and a Debye medium: each correction assumes it alone acts on its edges."""
    if deb is None:
        return
    for c in range(3):
        if lor.w[c].size == 0 or deb.w[c].size == 0:
            continue
        lo = [max(a, b) for a, b in zip(lor.lo[c], deb.lo[c])]
        hi = [min(a, b) for a, b in zip(lor.hi[c], deb.hi[c])]
        if any(h <= l for l, h in zip(lo, hi)):
            continue
        cut = lambda e: tuple(slice(lo[a] - e.lo[c][a], hi[a] - e.lo[c][a]) for a in (2, 1, 0))
        both = (lor.w[c][cut(lor)] != 0) & (deb.w[c][cut(deb)] != 0)
        if np.any(both):
            k, j, i = (int(v[0]) for v in np.nonzero(both))
            ml, md = int(lor.med[c][cut(lor)][k, j, i]), int(deb.med[c][cut(deb)][k, j, i])
            raise ValueError(f"the {'xyz'[c]}-edge at node {(i + lo[0], j + lo[1], k + lo[2])} is shared by the Lorentz medium "
                             f"'{' / '.join(lor.names[ml])}' and the Debye medium '{' / '.join(deb.names[md])}': separate them by a cell")


def check_placement(grid, cell_medium: np.ndarray, cpml_cells: Sequence[int], names: Optional[Sequence[str]] = None):
    """dispersion.check_placement for Lorentz media: dispersive cells inside CPML layers are refused."""
    _disp.check_placement(grid, cell_medium, cpml_cells, names, kind="Lorentz")


# ---- tables and the correction, restated ----------------------------------------------------------------
def tables(media: Sequence[LorentzMedium], dt: float, K: Optional[int] = None, dtype=np.float32):
    """(phi [nmedia][K][2][2], gam [nmedia][K][2], h [nmedia][K][2]) float32 of fdtd_lorentz_set; media with fewer poles are padded
    with zeros (their padding states stay 0)."""
    K = max(m.K for m in media) if K is None else int(K)
    phi = np.zeros((len(media), K, 2, 2), dtype)
    gam = np.zeros((len(media), K, 2), dtype)
    h = np.zeros((len(media), K, 2), dtype)
    for q, m in enumerate(media):
        P, G, H, _ = m.discretise(dt)
        phi[q, :m.K], gam[q, :m.K], h[q, :m.K] = P, G, H
    return phi, gam, h


def correction(V: np.ndarray, vi: np.ndarray, w: np.ndarray, vprev: np.ndarray, x: np.ndarray,
               phi: np.ndarray, gam: np.ndarray, h: np.ndarray) -> np.ndarray:
    """The per-timestep correction of include/fdtd_hip_lorentz.h, statement for statement, in the arrays' own precision (float32 to
    restate the kernel).  V, vi, w, vprev: any one shape; x: [K][2] + that shape; phi: [K][2][2] + that shape, gam, h: [K][2] + that
    shape — or without it: scalars broadcast (the edge's medium rows).  Edges with w == 0 keep V, x and vprev.  x and vprev are
    updated in place; returns V_new."""
    ty = V.dtype.type
    K = x.shape[0]
    S = np.zeros(V.shape, V.dtype)
    for k in range(K):
        p0 = h[k][0] * x[k][0]
        p1 = h[k][1] * x[k][1]
        s = p0 + p1
        S = S + s
    t = w * S
    q = vi * t
    vn = V - q
    s = vn + vprev
    avg = ty(0.5) * s
    on = w != 0
    for k in range(K):
        a = phi[k][0][0] * x[k][0]
        b = phi[k][0][1] * x[k][1]
        c = a + b
        d = gam[k][0] * avg
        jn = c + d
        a = phi[k][1][0] * x[k][0]
        b = phi[k][1][1] * x[k][1]
        c = a + b
        d = gam[k][1] * avg
        un = c + d
        x[k][0] = np.where(on, jn, x[k][0])
        x[k][1] = np.where(on, un, x[k][1])
    out = np.where(on, vn, V)
    vprev[...] = np.where(on, vn, vprev)
    return out


def branch_energy(lor: "LorentzEdges", x: Sequence[np.ndarray]) -> float:
    """Energy stored in the branches, 1/2 sum w_e (l_k j_k^2 + c_k u_k^2); x[c]: [K][2] + box shape."""
    tot = 0.0
    for c in range(3):
        if lor.w[c].size == 0:
            continue
        for k in range(x[c].shape[0]):
            ew = np.array([m.energy_weights()[k] if k < m.K else (0.0, 0.0) for m in lor.media])[lor.med[c]]     # box + [2]
            xx = x[c][k].astype(np.float64)
            tot += float(np.sum(lor.w[c] * (ew[..., 0] * xx[0] ** 2 + ew[..., 1] * xx[1] ** 2)))
    return tot
