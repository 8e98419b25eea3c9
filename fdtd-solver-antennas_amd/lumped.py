"""Lumped R-L-C elements on mesh edges (openEMS users know them as ``CSX.AddLumpedElement(name, ny, caps, R, C, L, LEtype)``).

Model.  An element is a one-port between the two ends of its box along ``direction``:

    parallel (LEtype = 0):  Y(s) = 1/R + s C + 1/(s L)        an absent part carries no current
    series   (LEtype = 1):  Z(s) = R + s L + 1/(s C)          absent R, L = 0; absent C = a short

An edge of the mesh, in circuit form, steps as  C_e (V' - V)/dt + G_e (V' + V)/2 = curl I - ibar,  ibar the element's mean current
over the step.  The element is written as a state space with at most two states,  dx/dt = A_c x + B_c v,  i = C_c x + D_c v,  and
discretised with the trapezoidal rule driven by Vm = (V' + V)/2:

    Phi = (I - dt/2 A_c)^-1 (I + dt/2 A_c)     Gam = (I - dt/2 A_c)^-1 dt B_c
    x'  = Phi x + Gam Vm                       ibar = h.x + g0 Vm
    h   = C_c (Phi + I)/2                      g0 = C_c Gam/2 + D_c   (>= 0)

g0 is a conductance and is folded into G_e (the lumped-edge overrides of the operator build), as a plain 1/R is; a plain C is folded
into C_e.  What remains is the sparse correction of include/fdtd_hip_lumped.h (csrc/lumped.hip; ``correction`` below restates it in
numpy, operation for operation).  The branch is passive: per step it takes dt Vm ibar from the fields, stores the change of
1/2 L i^2 + 1/2 C u^2 exactly and turns dt R i_m^2 (i_m the mean branch current) into heat, so the timestep and the Courant limit
are untouched.  Its discrete admittance is the continuous one at the warped frequency, Y(s_d) with s_d = j (2/dt) tan(w dt/2).

Cases (per edge values):

    parallel             1/R -> G_e, C -> C_e;  L: one state i_L,  A_c = 0, B_c = 1/L, C_c = 1
    series, L > 0        states (i, u) — (i) without C:  L di/dt = v - R i - u,  C du/dt = i
    series, L = 0, R > 0, C    state u:  du/dt = (v - u)/(R C),  i = (v - u)/R  (D_c = 1/R)
    series, L = 0, R > 0       a plain conductance, no state
    series, L = 0, R = 0, C    a plain capacitance, no state
    series, nothing            refused: a short is a metal

Geometry.  An element box maps onto edges as a port box does: n_ser edges along its direction, n_par parallel lines across it; each
edge carries R n_par/n_ser, L n_par/n_ser, C n_ser/n_par.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence
import numpy as np

KINDS = ("parallel", "series")


def _value(name, what, v):
    """None / NaN: absent.  Negative or infinite values are refused."""
    if v is None:
        return None
    v = float(v)
    if np.isnan(v):
        return None
    if not np.isfinite(v) or v < 0:
        raise ValueError(f"lumped element '{name}': {what} = {v!r} must be finite and >= 0")
    return v


@dataclass
class Element:
    """One lumped element; n_ser / n_par: the split of its box over mesh edges (1, 1: the values are the edge's own)."""
    name: str = ""
    R: Optional[float] = None
    L: Optional[float] = None
    C: Optional[float] = None
    kind: str = "parallel"
    n_ser: int = 1
    n_par: int = 1

    def __post_init__(self):
        kind = {0: "parallel", 1: "series"}.get(self.kind, self.kind)
        if kind not in KINDS:
            raise ValueError(f"lumped element '{self.name}': kind must be 'parallel' (0) or 'series' (1), got {self.kind!r}")
        self.kind = kind
        self.R, self.L, self.C = (_value(self.name, w, v) for w, v in (("R", self.R), ("L", self.L), ("C", self.C)))
        if int(self.n_ser) < 1 or int(self.n_par) < 1:
            raise ValueError(f"lumped element '{self.name}': n_ser and n_par must be >= 1")
        self.n_ser, self.n_par = int(self.n_ser), int(self.n_par)
        if kind == "parallel":
            if self.R == 0 or self.L == 0:
                raise ValueError(f"lumped element '{self.name}': a parallel element with R = 0 or L = 0 is a short: draw a metal")
            if self.R is None and self.L is None and not self.C:
                raise ValueError(f"lumped element '{self.name}': no R, L or C given")
            if self.C == 0:
                self.C = None
        else:
            if self.C == 0:
                raise ValueError(f"lumped element '{self.name}': a series element with C = 0 is an open circuit")
            if not self.R and not self.L and self.C is None:
                raise ValueError(f"lumped element '{self.name}': a series element without R, L and C is a short: draw a metal")

    # ---- per-edge values ------------------------------------------------------------------------------------
    def split(self, n_ser: int, n_par: int) -> "Element":
        return Element(self.name, self.R, self.L, self.C, self.kind, n_ser, n_par)

    @property
    def R_edge(self):
        return None if self.R is None else self.R * self.n_par / self.n_ser

    @property
    def L_edge(self):
        return None if self.L is None else self.L * self.n_par / self.n_ser

    @property
    def C_edge(self):
        return None if self.C is None else self.C * self.n_ser / self.n_par

    def _G_edge(self):
        # the association a lumped port's resistor uses (scene._port_on_grid), so that an R-only element IS that resistor
        return self.n_ser / (self.R * self.n_par)

    # ---- the case table -------------------------------------------------------------------------------------
    def state_space(self):
        """(A_c [ns][ns], B_c [ns], C_c [ns], D_c, G_fold, C_fold, energy weights [ns]) of one edge; ns = 0, 1 or 2 states.
        The stored energy is sum_q weights[q] x_q^2."""
        R, L, C = self.R_edge, self.L_edge, self.C_edge
        z = np.zeros
        if self.kind == "parallel":
            G = 0.0 if R is None else self._G_edge()
            Cf = 0.0 if C is None else C
            if L is None:
                return z((0, 0)), z(0), z(0), 0.0, G, Cf, z(0)
            return z((1, 1)), np.array([1.0 / L]), np.array([1.0]), 0.0, G, Cf, np.array([0.5 * L])
        R = 0.0 if R is None else R
        if L:
            if C is None:
                return np.array([[-R / L]]), np.array([1.0 / L]), np.array([1.0]), 0.0, 0.0, 0.0, np.array([0.5 * L])
            return (np.array([[-R / L, -1.0 / L], [1.0 / C, 0.0]]), np.array([1.0 / L, 0.0]), np.array([1.0, 0.0]), 0.0, 0.0, 0.0,
                    np.array([0.5 * L, 0.5 * C]))
        if R > 0:
            if C is None:
                return z((0, 0)), z(0), z(0), 0.0, self._G_edge(), 0.0, z(0)
            return (np.array([[-1.0 / (R * C)]]), np.array([1.0 / (R * C)]), np.array([-1.0 / R]), 1.0 / R, 0.0, 0.0,
                    np.array([0.5 * C]))
        return z((0, 0)), z(0), z(0), 0.0, 0.0, C, z(0)

    @property
    def nstates(self) -> int:
        return int(self.state_space()[1].size)

    def discretise(self, dt: float):
        """(Phi [2][2], Gam [2], h [2], g0, G_fold, C_fold) in float64 for timestep dt, per edge.  A one-state element leaves the
        second row and column at zero, a stateless one everything; the operator's edge takes G = g0 + G_fold and C = C_fold."""
        A, B, Cc, D, G, Cf, _ = self.state_space()
        ns = B.size
        Phi, Gam, h = np.zeros((2, 2)), np.zeros(2), np.zeros(2)
        g0 = 0.0
        if ns:
            I = np.eye(ns)
            M = np.linalg.inv(I - 0.5 * dt * A)
            P = M @ (I + 0.5 * dt * A)
            Gm = M @ (dt * B)
            Phi[:ns, :ns], Gam[:ns] = P, Gm
            h[:ns] = Cc @ (P + I) * 0.5
            g0 = float(Cc @ Gm * 0.5 + D)
        return Phi, Gam, h, g0, float(G), float(Cf)

    def energy_weights(self) -> np.ndarray:
        w = np.zeros(2)
        ew = self.state_space()[6]
        w[:ew.size] = ew
        return w

    # ---- admittances ----------------------------------------------------------------------------------------
    def _Y(self, s):
        R, L, C = self.R_edge, self.L_edge, self.C_edge
        s = np.asarray(s, np.complex128)
        if self.kind == "parallel":
            y = np.zeros(s.shape, np.complex128)
            if R is not None:
                y = y + 1.0 / R
            if C is not None:
                y = y + s * C
            if L is not None:
                y = y + 1.0 / (s * L)
            return y
        zz = np.zeros(s.shape, np.complex128) + (R or 0.0) + s * (L or 0.0)
        if C is not None:
            zz = zz + 1.0 / (s * C)
        return 1.0 / zz

    def admittance(self, f):
        """Y(j 2 pi f) of one edge's share [S]."""
        return self._Y(2j * np.pi * np.atleast_1d(np.asarray(f, float)))

    def admittance_discrete(self, f, dt: float):
        """What the stepped element presents: Y(s_d), s_d = j (2/dt) tan(pi f dt) — the bilinear warping of the trapezoidal rule."""
        f = np.atleast_1d(np.asarray(f, float))
        return self._Y(1j * (2.0 / dt) * np.tan(np.pi * f * dt))

    def resonance(self, dt: Optional[float] = None) -> Optional[float]:
        """1 / (2 pi sqrt(L C)) of an element with L and C; with dt, the frequency the stepped element resonates at instead:
        (1/(pi dt)) atan(dt / (2 sqrt(L C)))."""
        if not self.L or not self.C:
            return None
        w0 = 1.0 / np.sqrt(self.L_edge * self.C_edge)
        return float(w0 / (2 * np.pi)) if dt is None else float(np.arctan(0.5 * w0 * dt) / (np.pi * dt))


def transfer(Phi, Gam, h, g0, f, dt):
    """The admittance of the discretised branch at frequencies f: ibar / Vm for x' = Phi x + Gam Vm, ibar = h.x + g0 Vm with
    everything ~ z^n, z = exp(j 2 pi f dt):  g0 + h (z I - Phi)^-1 Gam."""
    f = np.atleast_1d(np.asarray(f, float))
    out = np.empty(f.size, np.complex128)
    for q, fq in enumerate(f):
        z = np.exp(2j * np.pi * fq * dt)
        out[q] = g0 + h @ np.linalg.solve(z * np.eye(2) - Phi, Gam.astype(np.complex128))
    return out


# ---- the edges of a voxelised scene ---------------------------------------------------------------------------
@dataclass
class LumpedEdges:
    """The element edges of a voxelised scene: global flat node index, component, index into `elements` — one Element per box, holding
    the box's split factors."""
    idx: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    comp: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int8))
    elem: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    elements: List[Element] = field(default_factory=list)

    def __len__(self):
        return int(self.idx.size)

    def stepped(self) -> np.ndarray:
        """Positions of the edges that carry states (the set the engine steps)."""
        ns = np.array([e.nstates for e in self.elements], np.int64)
        return np.nonzero(ns[self.elem] > 0)[0] if len(self) else np.zeros(0, np.int64)


def tables(elements: Sequence[Element], elem: np.ndarray, dt: float):
    """(cls int32 [n], phi float32 [ncls][2][2], gam float32 [ncls][2], h float32 [ncls][2]) of fdtd_lumped_set for edges whose
    elements are elements[elem[e]]: one class per element that occurs."""
    used, cls = np.unique(np.asarray(elem, np.int64), return_inverse=True)
    phi = np.zeros((used.size, 2, 2), np.float32)
    gam = np.zeros((used.size, 2), np.float32)
    h = np.zeros((used.size, 2), np.float32)
    for q, m in enumerate(used):
        P, Gm, hh, _, _, _ = elements[int(m)].discretise(dt)
        phi[q], gam[q], h[q] = P, Gm, hh
    return cls.astype(np.int32).ravel(), phi, gam, h


def correction(V, vi, vprev, x, phi, gam, h):
    """The per-timestep correction of include/fdtd_hip_lumped.h, statement for statement, in the arrays' own precision (float32 to
    restate the kernel).  V, vi, vprev: [n]; x: [2][n] (updated in place); phi: [2][2][n], gam, h: [2][n] (the edge's class rows).
    Returns V_new (also the new vprev)."""
    half = V.dtype.type(0.5)
    p0 = h[0] * x[0]
    p1 = h[1] * x[1]
    S = p0 + p1
    q = vi * S
    v = V - q
    s = v + vprev
    avg = half * s
    a = phi[0][0] * x[0]
    b = phi[0][1] * x[1]
    c = a + b
    d = gam[0] * avg
    x0 = c + d
    a = phi[1][0] * x[0]
    b = phi[1][1] * x[1]
    c = a + b
    d = gam[1] * avg
    x1 = c + d
    x[0] = x0
    x[1] = x1
    return v


def stored_energy(weights: np.ndarray, x: np.ndarray) -> float:
    """1/2 L i^2 + 1/2 C u^2 summed over the edges: weights [2][n] (Element.energy_weights per edge), x [2][n]."""
    return float(np.sum(np.asarray(weights, np.float64) * np.asarray(x, np.float64) ** 2))
