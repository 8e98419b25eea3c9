"""Near-field recording surfaces + near-to-far-field transform.

Replaces ``FDTD.CreateNF2FFBox()`` / ``nf2ff.CalcNF2FF(sim_path, f, theta, phi, center=...)``
(antenna_sim/solver_fdtd_openems_fixed.py:220,296; per-phi loops solver_fdtd_openems_microstrip_3d.py
:224-225 and _multi_3d.py:620-621).  The external engine dumps time-domain E/H on six faces to HDF5
and a separate tool DFTs and integrates them; here the RAW edge voltages / face currents of the faces
are either recorded in the time domain in HBM and transformed on the device for any frequency after the
run (fdtd_set_recorder / fdtd_rec_transform: the reference's semantics, default) or accumulated as a
running DFT at frequencies fixed beforehand (fdtd_set_dft: constant memory, for very long runs);
interpolation to the face nodes, the equivalent currents and the radiation integral (fdtd_farfield, on
the GPU) happen once at the end.

Result attributes mirror what the reference reads from the openEMS result object:
``E_norm[f]`` -> (ntheta, nphi), ``Dmax[f]`` (fixed.py:304-305) and ``E_theta, E_phi, P_rad, Prad``
(solver_fdtd_openems.py:318-321).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple
import numpy as np

from .constants import C0, ETA0
from .grid import RectGrid
from ._capi import KIND_V, KIND_I


@dataclass
class _BoxReq:
    kind: int
    comp: int
    lo: Tuple[int, int, int]
    hi: Tuple[int, int, int]


MIRROR_NONE, MIRROR_PEC, MIRROR_PMC = 0, 1, 2      # upstream's numbers (CreateNF2FFBox(mirror=...)); _capi.MIRROR_PEC / MIRROR_PMC
_FACE = ("x-", "x+", "y-", "y+", "z-", "z+")


class NF2FFBox:
    """Six recording faces on node planes lo[a] / hi[a] (inclusive node indices).

    mirror: six entries per face (x-, x+, y-, y+, z-, z+), 0 none, 1 PEC, 2 PMC: the box is OPEN on that side — it reaches the
    wall and records no face there; the far field of the mirror images closes it (farfield_mirror_spec / fdtd_farfield_mirror).
    A PEC wall lies on the outer node plane: the box's index on that side is 0 (n - 1) and the mirror coordinate that line's.  A
    PMC wall lies half a cell inside (simulation.BoundarySpec): the box starts on the first live node line, 1 (n - 2), and the
    mirror coordinate is the midpoint of the two outermost lines.  lo / hi of a mirrored side are set here, whatever was passed.
    The requests of the remaining faces are clipped to the readable side of the wall (`requests`); what the node interpolation
    needs beyond it (one index) is the mirror image by the component's parity (`_extended`):

        wall   E normal   E tangential   H normal   H tangential
        PEC    even       odd            odd        even
        PMC    odd        even           even       odd

    half_space: the one PEC plane of `mirror` is an infinite ground plane, the simulated half-space the world."""

    def __init__(self, grid: RectGrid, lo: Sequence[int], hi: Sequence[int], mirror: Optional[Sequence[int]] = None,
                 half_space: bool = False):
        self.grid = grid
        n = grid.shape
        self.mirror = (0,) * 6 if mirror is None else tuple(int(v) for v in mirror)
        if len(self.mirror) != 6 or any(m not in (MIRROR_NONE, MIRROR_PEC, MIRROR_PMC) for m in self.mirror):
            raise ValueError("NF2FF mirror: six entries (x-, x+, y-, y+, z-, z+) of 0 (none), 1 (PEC) or 2 (PMC)")
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        # per axis the wall: (side, type, P2) with P2 = twice the plane's position in node indices, so that a node index i
        # mirrors to P2 - i and a staggered one (at i + 1/2) to P2 - 1 - i; and the readable index range [clip_lo, clip_hi]
        # of node-located values (a staggered value's upper end is one less)
        self._wall: List[Optional[Tuple[int, int, int]]] = [None] * 3
        self._clip = [(0, n[a] - 1) for a in range(3)]
        for a in range(3):
            ml, mh = self.mirror[2 * a], self.mirror[2 * a + 1]
            if ml and mh:
                raise ValueError(f"NF2FF mirror: both faces of the {'xyz'[a]} axis ({_FACE[2 * a]} and {_FACE[2 * a + 1]}) carry a mirror: "
                                 "one plane per axis")
            if ml:
                lo[a] = 0 if ml == MIRROR_PEC else 1
                self._wall[a] = (0, ml, 2 * lo[a] if ml == MIRROR_PEC else 1)
                self._clip[a] = (lo[a], n[a] - 1)
            elif mh:
                hi[a] = n[a] - 1 if mh == MIRROR_PEC else n[a] - 2
                self._wall[a] = (1, mh, 2 * hi[a] if mh == MIRROR_PEC else 2 * n[a] - 3)
                self._clip[a] = (0, hi[a])
        self.lo, self.hi = tuple(lo), tuple(hi)
        for a in range(3):
            lo_ok = self.mirror[2 * a] or 1 <= self.lo[a]
            hi_ok = self.mirror[2 * a + 1] or self.hi[a] <= n[a] - 2
            if not (lo_ok and hi_ok and self.lo[a] < self.hi[a]):
                raise ValueError("NF2FF box must lie strictly inside the grid")
        pec_planes = [f for f in range(6) if self.mirror[f] == MIRROR_PEC]
        self.half_space_face: Optional[int] = None
        if half_space:
            if not any(self.mirror):
                raise ValueError("NF2FF half space: needs a PEC mirror plane (the ground), and there is no mirror")
            if not pec_planes:
                f = next(f for f in range(6) if self.mirror[f])
                raise ValueError(f"NF2FF half space: the mirror on face {_FACE[f]} is a PMC plane; an infinite ground is a PEC plane")
            if len(pec_planes) > 1:
                raise ValueError(f"NF2FF half space: faces {' and '.join(_FACE[f] for f in pec_planes)} are both PEC mirrors; "
                                 "only one plane can be the ground")
            self.half_space_face = pec_planes[0]
        # the mesh the node interpolation works on: one ghost line beyond every PEC mirror plane (a PMC wall has its own: the
        # grid's outer line is the image of the first live one); _off shifts node indices into it
        self._off = tuple(1 if self.mirror[2 * a] == MIRROR_PEC else 0 for a in range(3))
        self._xg = grid
        if pec_planes:
            ext = []
            for a in range(3):
                l = grid.lines[a]
                if self.mirror[2 * a] == MIRROR_PEC:
                    l = np.concatenate([[2.0 * l[0] - l[1]], l])
                if self.mirror[2 * a + 1] == MIRROR_PEC:
                    l = np.concatenate([l, [2.0 * l[-1] - l[-2]]])
                ext.append(l)
            self._xg = RectGrid(*ext)
        self.requests: List[_BoxReq] = []                     # what is recorded: clipped to the readable side of the walls
        self._ideal: List[Tuple[tuple, tuple]] = []           # per request the index box the interpolation works on
        self._req_of: Dict[Tuple[int, int, int], int] = {}   # (face, kind, comp) -> request index
        for f in range(6):
            if self.mirror[f]:
                continue
            a, side = f // 2, f % 2
            a0 = self.hi[a] if side else self.lo[a]
            t1, t2 = (a + 1) % 3, (a + 2) % 3
            for t, u in ((t1, t2), (t2, t1)):
                lo_v, hi_v = list(self.lo), list(self.hi)
                lo_v[a] = hi_v[a] = a0
                lo_v[t] -= 1                     # E_t at a node averages edges t-1 and t
                self._add(f, KIND_V, t, lo_v, hi_v)
                lo_i, hi_i = list(self.lo), list(self.hi)
                lo_i[a], hi_i[a] = a0 - 1, a0    # H_t at a node averages the 4 faces around it
                lo_i[u] -= 1
                self._add(f, KIND_I, t, lo_i, hi_i)

    @staticmethod
    def _staggered(kind, comp, axis) -> bool:
        """Whether a value sits half a cell up along `axis`: an edge voltage along its own axis, a face current along the two others."""
        return (axis == comp) if kind == KIND_V else (axis != comp)

    def _add(self, face, kind, comp, lo, hi):
        self._req_of[(face, kind, comp)] = len(self.requests)
        self._ideal.append((tuple(lo), tuple(hi)))
        lo, hi = list(lo), list(hi)
        for a in range(3):                       # never read beyond or on the dead side of a wall
            if self._wall[a] is not None:
                cl, ch = self._clip[a]
                lo[a] = max(lo[a], cl)
                hi[a] = min(hi[a], ch - 1 if self._staggered(kind, comp, a) else ch)
        self.requests.append(_BoxReq(kind, comp, tuple(lo), tuple(hi)))

    def _extended(self, boxes, ri: int, fidx: int) -> np.ndarray:
        """The values of request ri over its whole index box [k][j][i]: what was recorded, and beyond a wall the mirror image by the
        component's parity.  An index that is its own image (an edge or dual plane lying in the wall) can only be odd: zero."""
        r, (ilo, ihi) = self.requests[ri], self._ideal[ri]
        v = boxes[ri][fidx]
        if (ilo, ihi) == (r.lo, r.hi):
            return v
        out = np.zeros([ihi[a] - ilo[a] + 1 for a in (2, 1, 0)], np.complex128)
        out[tuple(slice(r.lo[a] - ilo[a], r.hi[a] - ilo[a] + 1) for a in (2, 1, 0))] = v
        for a in range(3):
            missing = [i for i in range(ilo[a], ihi[a] + 1) if not r.lo[a] <= i <= r.hi[a]]
            if not missing:
                continue
            _, wtype, p2 = self._wall[a]
            normal = r.comp == a
            sign = (1.0 if wtype == MIRROR_PEC else -1.0) * (1.0 if normal else -1.0) * (1.0 if r.kind == KIND_V else -1.0)
            for i in missing:
                ip = p2 - 1 - i if self._staggered(r.kind, r.comp, a) else p2 - i
                dst = [slice(None)] * 3; dst[2 - a] = i - ilo[a]
                if ip == i:
                    assert sign < 0
                    out[tuple(dst)] = 0.0
                else:
                    assert r.lo[a] <= ip <= r.hi[a]
                    src = [slice(None)] * 3; src[2 - a] = ip - ilo[a]
                    out[tuple(dst)] = sign * out[tuple(src)]
        return out

    def _weights(self, t: int, lo: int, hi: int) -> np.ndarray:
        """Trapezoid weights of the nodes lo..hi (indices of the extended mesh) along axis t.  Towards a mirror plane the rule runs on
        across the wall and only the nodes on the own side are kept; a node on a PEC plane carries half its weight (its image
        coincides with it)."""
        w = self._wall[t]
        el = 1 if (w is not None and w[0] == 0) else 0
        eh = 1 if (w is not None and w[0] == 1) else 0
        x = self._xg.lines[t][lo - el:hi + 1 + eh]
        wt = np.empty_like(x)
        wt[1:-1] = 0.5 * (x[2:] - x[:-2]); wt[0] = 0.5 * (x[1] - x[0]); wt[-1] = 0.5 * (x[-1] - x[-2])
        wt = wt[el:wt.size - eh]
        if w is not None and w[1] == MIRROR_PEC:
            wt[-1 if w[0] else 0] *= 0.5
        return wt

    def mirror_planes(self, center_m: Sequence[float]):
        """([(axis, type, coordinate relative to center_m)] in axis order, index of the half-space plane in it or None)."""
        planes, hs = [], None
        for a in range(3):
            if self._wall[a] is None:
                continue
            side, wtype, _ = self._wall[a]
            l = self.grid.lines[a]
            if wtype == MIRROR_PEC:
                c = l[-1] if side else l[0]
            else:
                c = 0.5 * (l[-2] + l[-1]) if side else 0.5 * (l[0] + l[1])
            if self.half_space_face == 2 * a + side:
                hs = len(planes)
            planes.append((a, wtype, float(c) - float(center_m[a])))
        return planes, hs

    @property
    def power_factor(self) -> float:
        """What the flux through the recorded faces is multiplied by for Prad: 2 per mirror plane (the radiated power of the
        mirrored whole in all of space), except the half-space plane — the half-space is the world, so a monopole on an infinite
        ground reads D = 3.  (This rule is the package's own: upstream's treatment of Prad under mirrors was not consulted.)"""
        m = sum(1 for w in self._wall if w is not None) - (1 if self.half_space_face is not None else 0)
        return float(2 ** m)

    # -- recording ------------------------------------------------------------------------------
    def register(self, engine) -> List[int]:
        return [engine.add_dft_box(r.kind, r.comp, r.lo, r.hi) for r in self.requests]

    def collect(self, engine, ids: List[int], tw_v=None, tw_i=None) -> List[np.ndarray]:
        """Per request a complex array [nfreq][nk][nj][ni] covering the whole request box, zero where
        this slab owns nothing (sum over ranks = complete box).  With twiddle tables (recorder mode) the
        recorded time-domain samples are transformed on the device for those frequencies."""
        out = []
        for r, bid in zip(self.requests, ids):
            ext = [r.hi[a] - r.lo[a] + 1 for a in range(3)]
            if tw_v is not None:
                data, lo, hi = engine.rec_transform(bid, tw_v if r.kind == KIND_V else tw_i)
            else:
                data, lo, hi = engine.get_dft_box(bid)
            full = np.zeros((data.shape[0], ext[2], ext[1], ext[0]), np.complex128)
            if data.size:
                full[:, lo[2] - r.lo[2]:hi[2] - r.lo[2] + 1, lo[1] - r.lo[1]:hi[1] - r.lo[1] + 1,
                     lo[0] - r.lo[0]:hi[0] - r.lo[0] + 1] = data
            out.append(full)
        return out

    # -- post-processing ------------------------------------------------------------------------
    def surface_currents(self, boxes: List[np.ndarray], fidx: int, center_m: Sequence[float]):
        """Node-interpolated E,H on the six faces -> quadrature points.
        Returns pos [N][3] (relative to center), Js, Ms [N][3] complex (area weighted) and the
        outward Poynting flux 0.5*Re sum (E x H*).n dA.
        With mirror planes: the recorded faces only, the arithmetic unchanged on arrays and mesh lines extended across the walls
        (_extended, _xg) and the nodes of the own side kept (_weights); the flux is that of the recorded faces (power_factor)."""
        g = self._xg
        lo = tuple(self.lo[c] + self._off[c] for c in range(3))
        hi = tuple(self.hi[c] + self._off[c] for c in range(3))
        pos_l, js_l, ms_l = [], [], []
        flux = 0.0
        np_axis = {0: 2, 1: 1, 2: 0}
        for f in range(6):
            if self.mirror[f]:
                continue
            a, side = f // 2, f % 2
            t1, t2 = (a + 1) % 3, (a + 2) % 3
            nsign = 1.0 if side else -1.0
            E = {}
            H = {}
            for t, u in ((t1, t2), (t2, t1)):
                v = self._extended(boxes, self._req_of[(f, KIND_V, t)], fidx)      # [k][j][i] over the request box
                # divide by edge length along t, then average edges (t-1, t)
                lt = g.d[t][lo[t] - 1:hi[t] + 1]
                shp = [1, 1, 1]; shp[np_axis[t]] = lt.size
                e = v / lt.reshape(shp)
                sl_a = [slice(None)] * 3; sl_b = [slice(None)] * 3
                sl_a[np_axis[t]] = slice(0, -1); sl_b[np_axis[t]] = slice(1, None)
                E[t] = np.squeeze(0.5 * (e[tuple(sl_a)] + e[tuple(sl_b)]), axis=np_axis[a])
                i_ = self._extended(boxes, self._req_of[(f, KIND_I, t)], fidx)
                ld = g.dd[t][lo[t]:hi[t] + 1]
                shp = [1, 1, 1]; shp[np_axis[t]] = ld.size
                h = i_ / ld.reshape(shp)
                # average over the two planes along a and the pair (u-1, u)
                acc = 0.0
                for oa in (0, 1):
                    for ou in (0, 1):
                        s = [slice(None)] * 3
                        s[np_axis[a]] = slice(oa, oa + 1)
                        s[np_axis[u]] = slice(ou, ou + (hi[u] - lo[u] + 1))
                        acc = acc + h[tuple(s)]
                H[t] = np.squeeze(0.25 * acc, axis=np_axis[a])
            # trapezoid weights along the two tangential axes
            w = {}
            for t in (t1, t2):
                w[t] = self._weights(t, lo[t], hi[t])
            # 2-D arrays are ordered (slow, fast) = (larger axis id, smaller axis id) after the squeeze
            slow, fast = (t1, t2) if t1 > t2 else (t2, t1)
            dA = w[slow][:, None] * w[fast][None, :]
            coords = [None] * 3
            coords[a] = np.full(dA.shape, g.lines[a][hi[a] if side else lo[a]])
            cs, cf = np.meshgrid(g.lines[slow][lo[slow]:hi[slow] + 1],
                                 g.lines[fast][lo[fast]:hi[fast] + 1], indexing="ij")
            coords[slow], coords[fast] = cs, cf
            Ev = [np.zeros(dA.shape, np.complex128) for _ in range(3)]
            Hv = [np.zeros(dA.shape, np.complex128) for _ in range(3)]
            Ev[t1], Ev[t2] = E[t1], E[t2]
            Hv[t1], Hv[t2] = H[t1], H[t2]
            n = [0.0, 0.0, 0.0]; n[a] = nsign
            # Js = n x H ; Ms = -n x E  (only the normal component of n is non-zero)
            J = [np.zeros(dA.shape, np.complex128) for _ in range(3)]
            M = [np.zeros(dA.shape, np.complex128) for _ in range(3)]
            J[t1] = -nsign * Hv[t2]; J[t2] = nsign * Hv[t1]       # (n x H)_{t1} = -n_a H_{t2}; (n x H)_{t2} = n_a H_{t1}
            M[t1] = nsign * Ev[t2]; M[t2] = -nsign * Ev[t1]
            # Poynting: (E x H*)_a = E_t1 H_t2* - E_t2 H_t1*
            S = Ev[t1] * np.conj(Hv[t2]) - Ev[t2] * np.conj(Hv[t1])
            flux += 0.5 * nsign * float(np.sum(np.real(S) * dA))
            pos_l.append(np.stack([coords[0].ravel() - center_m[0], coords[1].ravel() - center_m[1],
                                   coords[2].ravel() - center_m[2]], axis=1))
            js_l.append(np.stack([(J[c] * dA).ravel() for c in range(3)], axis=1))
            ms_l.append(np.stack([(M[c] * dA).ravel() for c in range(3)], axis=1))
        return np.concatenate(pos_l), np.concatenate(js_l), np.concatenate(ms_l), flux


@dataclass
class NF2FFResult:
    freq: np.ndarray
    theta: np.ndarray          # rad
    phi: np.ndarray            # rad
    E_theta: List[np.ndarray] = field(default_factory=list)   # per frequency (ntheta, nphi) complex, r*E
    E_phi: List[np.ndarray] = field(default_factory=list)
    E_norm: List[np.ndarray] = field(default_factory=list)
    P_rad: List[np.ndarray] = field(default_factory=list)     # radiation intensity [W/sr]
    Prad: List[float] = field(default_factory=list)           # total radiated power [W]
    Dmax: List[float] = field(default_factory=list)


FF_HORIZON = -2.0 ** -50      # FF_HORIZON of csrc/farfield.hip: r^ . n of a direction on the horizon is a rounding error off zero


def _half_space_normal(pos, axis: int, coord: float) -> float:
    """+1 / -1: the normal of the half-space plane into the half where the points lie (fdtd_farfield_mirror's rule: the points off
    the plane must share a side; with none off it, +1)."""
    d = pos[:, axis] - coord
    if np.any(d > 0) and np.any(d < 0):
        raise ValueError("farfield: points on both sides of the half-space plane")
    return -1.0 if np.any(d < 0) else 1.0


def farfield_mirror_spec(pos, Js, Ms, k, theta, phi, mirrors, half_space: Optional[int] = None):
    """The numpy statement of fdtd_farfield_mirror (include/fdtd_hip_farfield.h): the radiation integral of k_farfield,

        N = sum J exp(j k r^ . r),  L = sum M exp(j k r^ . r),   r^ = (sin th cos ph, sin th sin ph, cos th)
        X_th = X_x cos th cos ph + X_y cos th sin ph - X_z sin th,   X_ph = -X_x sin ph + X_y cos ph        (X = N, L)
        E_th = -j k / (4 pi) (L_ph + eta0 N_th),   E_ph = +j k / (4 pi) (L_th - eta0 N_ph),

    summed over the points AND their images in `mirrors`, a sequence of up to three planes (axis a, type 1 = PEC | 2 = PMC (or
    'PEC' / 'PMC'), coordinate c), at most one per axis.  The image of a point across one plane: r'_a = 2 c - r_a; PEC: J tangential
    x(-1), J_a x(+1), M tangential x(+1), M_a x(-1); PMC the dual.  Several planes compose and the signs multiply; image i of the
    2^m has bit b set = reflected in plane b, image 0 is the point itself.  half_space = b: plane b (PEC) is an infinite ground;
    directions with r^ . n < 0 get exact zeros, n the plane's normal into the half where the points lie, and the horizon counts
    as in front (r^ . n >= FF_HORIZON).  theta / phi: paired 1-D lists; returns complex (E_theta, E_phi) * r."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    J = np.asarray(Js, np.complex128).reshape(-1, 3)
    M = np.asarray(Ms, np.complex128).reshape(-1, 3)
    th, ph = np.asarray(theta, np.float64).ravel(), np.asarray(phi, np.float64).ravel()
    if J.shape != pos.shape or M.shape != pos.shape or th.shape != ph.shape:
        raise ValueError("farfield argument shapes")
    planes = [(int(a), {"PEC": MIRROR_PEC, "PMC": MIRROR_PMC}.get(t, t), float(c)) for a, t, c in mirrors]
    if len(planes) > 3 or len({a for a, _, _ in planes}) != len(planes) or any(a not in (0, 1, 2) for a, _, _ in planes):
        raise ValueError("farfield: at most one mirror plane per axis (axis 0, 1 or 2)")
    if any(t not in (MIRROR_PEC, MIRROR_PMC) for _, t, _ in planes):
        raise ValueError("farfield: a mirror plane is of type 1 (PEC) or 2 (PMC)")
    if half_space is not None and (not 0 <= half_space < len(planes) or planes[half_space][1] != MIRROR_PEC):
        raise ValueError("farfield: the half-space plane must be one of the PEC mirror planes")
    st, ct, sp, cp = np.sin(th), np.cos(th), np.sin(ph), np.cos(ph)
    r = np.stack([st * cp, st * sp, ct], 1)
    N = np.zeros((th.size, 3), np.complex128)
    L = np.zeros((th.size, 3), np.complex128)
    for img in range(1 << len(planes)):
        q, sj, sm = pos.copy(), np.ones(3), np.ones(3)
        for b, (a, t, c) in enumerate(planes):
            if img >> b & 1:
                q[:, a] = 2.0 * c - q[:, a]
                s = 1.0 if t == MIRROR_PEC else -1.0
                normal = np.arange(3) == a
                sj *= np.where(normal, s, -s)
                sm *= np.where(normal, -s, s)
        for d0 in range(0, th.size, 256):             # in chunks of directions: [256][npts] phases at a time
            e = np.exp(1j * (k * (r[d0:d0 + 256] @ q.T)))
            N[d0:d0 + 256] += e @ (J * sj)
            L[d0:d0 + 256] += e @ (M * sm)
    Nth = N[:, 0] * ct * cp + N[:, 1] * ct * sp - N[:, 2] * st
    Nph = -N[:, 0] * sp + N[:, 1] * cp
    Lth = L[:, 0] * ct * cp + L[:, 1] * ct * sp - L[:, 2] * st
    Lph = -L[:, 0] * sp + L[:, 1] * cp
    fac = k / (4.0 * np.pi)
    eta0 = 376.730313668                              # k_farfield's constant, to the digit
    eth = -1j * fac * (Lph + eta0 * Nth)
    eph = 1j * fac * (Lth - eta0 * Nph)
    if half_space is not None:
        a, _, c = planes[half_space]
        behind = _half_space_normal(pos, a, c) * r[:, a] < FF_HORIZON
        eth[behind] = 0.0
        eph[behind] = 0.0
    return eth, eph


def calc_nf2ff(lib, box: NF2FFBox, boxes: List[np.ndarray], freqs, theta_rad, phi_rad, center_m,
               device: int = 0) -> NF2FFResult:
    """The whole theta x phi grid in one GPU launch per frequency.

    A box with mirror planes: the integral runs over the recorded faces and their images — on the device (fdtd_farfield_mirror)
    when the library exports it and FDTD_NF2FF is not "host", else by the specification (farfield_mirror_spec).  Prad is the flux
    through the recorded faces times NF2FFBox.power_factor."""
    import os
    from ._capi import farfield, farfield_mirror, has_farfield_mirror
    freqs = np.atleast_1d(np.asarray(freqs, float))
    th = np.asarray(theta_rad, float); ph = np.asarray(phi_rad, float)
    TH, PH = np.meshgrid(th, ph, indexing="ij")
    res = NF2FFResult(freq=freqs, theta=th, phi=ph)
    planes, half = box.mirror_planes(center_m)
    on_device = has_farfield_mirror(lib) and os.environ.get("FDTD_NF2FF", "").lower() != "host"
    for fi, f in enumerate(freqs):
        pos, Js, Ms, flux = box.surface_currents(boxes, fi, center_m)
        k = 2.0 * np.pi * f / C0
        if not planes:
            eth, eph = farfield(lib, pos, Js, Ms, k, TH.ravel(), PH.ravel(), device=device)
        elif on_device:
            eth, eph = farfield_mirror(lib, pos, Js, Ms, k, TH.ravel(), PH.ravel(), planes, half, device=device)
            flux *= box.power_factor
        else:
            eth, eph = farfield_mirror_spec(pos, Js, Ms, k, TH.ravel(), PH.ravel(), planes, half)
            flux *= box.power_factor
        eth = eth.reshape(TH.shape); eph = eph.reshape(TH.shape)
        U = (np.abs(eth) ** 2 + np.abs(eph) ** 2) / (2.0 * ETA0)
        res.E_theta.append(eth); res.E_phi.append(eph)
        res.E_norm.append(np.sqrt(np.abs(eth) ** 2 + np.abs(eph) ** 2))
        res.P_rad.append(U)
        res.Prad.append(flux)
        res.Dmax.append(4.0 * np.pi * float(np.max(U)) / flux if flux > 0 else float("nan"))
    return res
