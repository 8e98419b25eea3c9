"""Conformal (Dey-Mittra) PEC boundaries: curved and slanted metals without the staircase's first-order radius error.

This is the SPEC of the model (float64) and of the correction the engine applies (float32, include/fdtd_hip_conformal.h).

PEC edges stay what they are (one metal record holds both end nodes).  An edge is CUT when exactly one of its end nodes lies inside
the union of the plain metal records (conducting sheets do not count); it is free over the fraction f_e of its physical length,
0 < f_e <= 1.  The crossing is found by bisection on the inside predicates of include/fdtd_hip_voxel.h (primitives._inside), in
float64 with + - * and comparisons only, so that csrc/voxel.hip (fdtd_voxel_fractions) gives the same bits:

    t_a = 0 (the inside node), t_b = 1 (the outside node), d = x_out - x_in along the edge's axis;
    N_BISECT times:  t_m = 0.5 * (t_a + t_b);  x = x_in + t_m * d;  inside(x) ? t_a = t_m : t_b = t_m;
    f_e = (t_a * |d| <= snap) ? 1 : 1 - t_a,         snap = SNAP_TOLS * tol  (tol: the rasteriser's, 1e-6 of the smallest cell).

A record takes part in an edge's predicate when its node index box holds one of the edge's two nodes (the rasteriser's own gate).
The snap makes a metal whose surface lies on a mesh line (every box of the plugin's scenes) cut no edge: its list is empty.

The free area fraction a_f of a face follows from its four corners and the fractions of its cut edges, the boundary straight inside
the face (m = 1 - f):  one corner inside 1 - m_a m_b / 2;  two adjacent (f_a + f_b) / 2;  three f_a f_b / 2;  two diagonal
1 - m_a m_b / 2 - m_c m_d / 2.  V = E l stays the voltage of the FULL edge everywhere (ports, probes, NF2FF and the E kernels do not
change); the face current of a LISTED face becomes

    I_f <- i_prev + iv0 * sum+- g_e V_e,        g_e = f_e / a_f      (f_e = 1 on an edge that is not cut)

and a face is listed when a_f or any of its four g_e differs from 1 (a PEC edge carries no voltage: its g_e is left at 1).  Stability: with every g_e <= R the symmetric factor of the
system matrix is entrywise at most sqrt(R) times the plain one, so dt <= courant_dt / sqrt(R) is sufficient; the bound is enforced by
enlarging a_f to max_e f_e / R (the clamp; PEC edges carry no voltage and do not count), and a scene with listed faces runs at
courant_dt() / sqrt(R).  R is the user's (default 2).

The same physics in the variables V' = f V is a plain raw operator, vi' = f vi and iv' = iv0 / a_f: `raw_operator`, what the oracle
steps as it is — the independent reference.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence
import numpy as np

from . import primitives as _prims
from .grid import RectGrid

N_BISECT = 32          # bisection steps: f_e resolved to 2^-32 of the edge
SNAP_TOLS = 4.0        # snap distance in units of the rasteriser's tol
DEFAULT_RATIO = 2.0


# ---------------------------------------------------------------------------------------------------------------------------
# fractions
# ---------------------------------------------------------------------------------------------------------------------------
def plain_metal_table(scene, grid, table: Optional[_prims.Table] = None) -> _prims.Table:
    """The records of primitives.pack_table that count for the conformal model: metals that are no conducting sheets."""
    from .scene import ConductingSheet
    table = _prims.pack_table(scene, grid) if table is None else table
    rec = table.rec
    sheet = np.array([isinstance(m, ConductingSheet) for m in scene.metals] + [False], bool)
    keep = (rec["role"] == _prims.ROLE_METAL) & ~sheet[np.minimum(rec["prop"], len(scene.metals))] if rec.size else np.zeros(0, bool)
    names = [n for n, k in zip(table.names, keep) if k]
    return _prims.Table(np.ascontiguousarray(rec[keep]), table.verts, table.tol, [], names)


def node_inside(grid: RectGrid, table: _prims.Table) -> np.ndarray:
    """bool [nz][ny][nx]: the nodes inside the union of the table's (metal) records, each on its node index box."""
    nx, ny, nz = grid.shape
    out = np.zeros((nz, ny, nx), bool)
    for q in range(table.rec.size):
        res = _prims.node_mask(grid, table, q)
        if res is not None:
            out[res[1]] |= res[0]
    return out


def cut_edges(node_in: np.ndarray):
    """(comp int8, idx int64 flat node index of the lower node, flip bool: the INSIDE node is the upper one) of the edges with exactly
    one end node inside, ordered by component, then index."""
    nz, ny, nx = node_in.shape
    comp, idx, flip = [], [], []
    for c in range(3):
        ax = 2 - c
        lo = [slice(None)] * 3; hi = [slice(None)] * 3
        lo[ax] = slice(0, -1); hi[ax] = slice(1, None)
        cut = np.zeros(node_in.shape, bool)
        cut[tuple(lo)] = node_in[tuple(lo)] != node_in[tuple(hi)]
        q = np.flatnonzero(cut)
        up = np.zeros(node_in.shape, bool)
        up[tuple(lo)] = node_in[tuple(hi)]
        comp.append(np.full(q.size, c, np.int8)); idx.append(q.astype(np.int64)); flip.append(up.reshape(-1)[q])
    return np.concatenate(comp), np.concatenate(idx), np.concatenate(flip)


def snap_distance(table: _prims.Table) -> float:
    return SNAP_TOLS * float(table.tol)


def fractions_spec(grid: RectGrid, table: _prims.Table, comp, idx, flip, snap: Optional[float] = None) -> np.ndarray:
    """f_e float64 of the given cut edges by bisection (the module docstring's statements).  THE specification of
    fdtd_voxel_fractions."""
    comp, idx, flip = np.asarray(comp, np.int64), np.asarray(idx, np.int64), np.asarray(flip, bool)
    snap = snap_distance(table) if snap is None else float(snap)
    n = idx.size
    if n == 0:
        return np.zeros(0)
    nx, ny, nz = grid.shape
    k, r = np.divmod(idx, nx * ny)
    j, i = np.divmod(r, nx)
    pos = np.stack([i, j, k])                                   # [3][n]
    pos1 = pos.copy()
    pos1[comp, np.arange(n)] += 1
    pts = np.stack([grid.lines[a][pos[a]] for a in range(3)])   # the lower node
    lower = pts[comp, np.arange(n)]
    upper = np.stack([grid.lines[a][pos1[a]] for a in range(3)])[comp, np.arange(n)]
    x_in = np.where(flip, upper, lower)
    x_out = np.where(flip, lower, upper)
    d = x_out - x_in
    sel = []
    for q in range(table.rec.size):
        nb = table.rec[q]["nbox"]
        in0 = np.ones(n, bool); in1 = np.ones(n, bool)
        for a in range(3):
            in0 &= (pos[a] >= nb[a]) & (pos[a] <= nb[3 + a])
            in1 &= (pos1[a] >= nb[a]) & (pos1[a] <= nb[3 + a])
        sel.append(np.flatnonzero(in0 | in1))
    ta, tb = np.zeros(n), np.ones(n)
    ar = np.arange(n)
    for _ in range(N_BISECT):
        tm = 0.5 * (ta + tb)
        x = x_in + tm * d
        p = pts.copy()
        p[comp, ar] = x
        ins = np.zeros(n, bool)
        for q, s in enumerate(sel):
            if s.size:
                ins[s] |= _prims._inside(table.rec[q], table.verts, p[0][s], p[1][s], p[2][s], table.tol)
        ta = np.where(ins, tm, ta)
        tb = np.where(ins, tb, tm)
    length = np.abs(d)
    return np.where(ta * length <= snap, 1.0, 1.0 - ta)


@dataclass
class Fractions:
    """What the conformal model needs from the rasteriser: the nodes inside the metal union and f_e of every cut edge."""
    node_in: np.ndarray            # bool [nz][ny][nx]
    comp: np.ndarray               # int8 [ncut]
    idx: np.ndarray                # int64 [ncut], flat index of the edge's lower node
    f: np.ndarray                  # float64 [ncut]
    names: List[str] = field(default_factory=list)     # per record of the plain metal table, for messages
    table: Optional[_prims.Table] = None

    def dense(self) -> np.ndarray:
        """f_e over the whole grid, float64 [3][nz][ny][nx]: 1 on every edge that is not cut."""
        out = np.ones((3,) + self.node_in.shape)
        out.reshape(3, -1)[self.comp.astype(np.int64), self.idx] = self.f
        return out


def fractions(scene, grid: RectGrid, device_fractions=None) -> Fractions:
    """The fractions of a scene.  `device_fractions(grid, table) -> (node_in, comp, idx, f)`: _capi.fractions_device's callable
    (csrc/voxel.hip); None: numpy."""
    table = plain_metal_table(scene, grid)
    if device_fractions is not None:
        node_in, comp, idx, f = device_fractions(grid, table)
    else:
        node_in = node_inside(grid, table)
        comp, idx, flip = cut_edges(node_in)
        f = fractions_spec(grid, table, comp, idx, flip)
    return Fractions(node_in, comp, idx, f, list(table.names), table)


# ---------------------------------------------------------------------------------------------------------------------------
# faces
# ---------------------------------------------------------------------------------------------------------------------------
def _shift(a: np.ndarray, axis: int, fill):
    """a at the next index along the physical axis (the last index gets `fill`)."""
    ax = a.ndim - 1 - axis
    out = np.full(a.shape, fill, a.dtype)
    src = [slice(None)] * a.ndim; dst = [slice(None)] * a.ndim
    src[ax] = slice(1, None); dst[ax] = slice(0, -1)
    out[tuple(dst)] = a[tuple(src)]
    return out


def face_edges(n: int):
    """The four edges of a face of component n at node p, as (component, offset axis or None), in the order of the H update's
    curl:  + V_a2(p) - V_a2(p + e_a1) - V_a1(p) + V_a1(p + e_a2)."""
    a1, a2 = (n + 1) % 3, (n + 2) % 3
    return [(a2, None), (a2, a1), (a1, None), (a1, a2)]


def area_fraction(corners, fe, cut):
    """a_f from the corner pattern: corners = (c00, c10, c01, c11) bool arrays (10: the next node along a1, 01: along a2), fe and cut
    the four edges' fractions and cut flags in face_edges order (e0: 00-01, e1: 10-11, e2: 00-10, e3: 01-11).  A face with no or
    with four corners inside gets 1."""
    c00, c10, c01, c11 = corners
    e0, e1, e2, e3 = fe
    m0, m1, m2, m3 = (1.0 - e for e in fe)
    count = c00.astype(np.int8) + c10 + c01 + c11
    at = ((c00, m0 * m2, e0 * e2), (c10, m1 * m2, e1 * e2), (c01, m0 * m3, e0 * e3), (c11, m1 * m3, e1 * e3))
    corner_cut = sum(np.where(c, 0.5 * mm, 0.0) for c, mm, _ in at)                 # the triangles cut off at the inside corners
    a_one = 1.0 - corner_cut                                                        # one corner, or two diagonal ones
    a_three = sum(np.where(c, 0.0, 0.5 * ff) for c, _, ff in at)                    # the triangle left at the one outside corner
    a_adj = 0.5 * sum(np.where(c, e, 0.0) for c, e in zip(cut, fe))                 # the trapezoid between the two cut edges
    diagonal = (count == 2) & (c00 == c11)
    return np.where(count == 1, a_one, np.where(diagonal, a_one, np.where(count == 2, a_adj, np.where(count == 3, a_three, 1.0))))


@dataclass
class ConformalFaces:
    """The listed faces of a scene: per face its component, flat node index, the four g_e in face_edges order, the (clamped) area
    fraction; and the cut edges with their fractions."""
    comp: np.ndarray               # int8 [nfaces]
    idx: np.ndarray                # int64 [nfaces]
    g: np.ndarray                  # float64 [nfaces][4]
    a: np.ndarray                  # float64 [nfaces], after the clamp
    a_geo: np.ndarray              # float64 [nfaces], before it
    ratio: float
    frac: Fractions

    def __len__(self) -> int:
        return int(self.idx.size)

    @property
    def clamped(self) -> int:
        return int(np.count_nonzero(self.a > self.a_geo))

    def faces(self) -> list:
        return [int(np.count_nonzero(self.comp == c)) for c in range(3)]

    @property
    def dt_factor(self) -> float:
        return float(1.0 / np.sqrt(self.ratio)) if len(self) else 1.0


def make_faces(grid: RectGrid, frac: Fractions, pec: np.ndarray, ratio: float = DEFAULT_RATIO) -> Optional[ConformalFaces]:
    """Fractions -> area fractions -> clamp -> the face list; None when no face is listed.  pec: bool [3][nz][ny][nx]."""
    ratio = float(ratio)
    if not np.isfinite(ratio) or ratio < 1.0:
        raise ValueError(f"conformal_ratio = {ratio!r}: the bound R on g_e = f_e / a_f must be >= 1")
    if frac.idx.size == 0 or not np.any(frac.f != 1.0):
        return None
    nx, ny, nz = grid.shape
    fe = frac.dense()
    is_cut = np.zeros(fe.shape, bool)
    is_cut.reshape(3, -1)[frac.comp.astype(np.int64), frac.idx] = True
    nin = frac.node_in
    comp, idx, gs, aa, ag = [], [], [], [], []
    for n in range(3):
        a1, a2 = (n + 1) % 3, (n + 2) % 3
        corners = (nin, _shift(nin, a1, False), _shift(nin, a2, False), _shift(_shift(nin, a1, False), a2, False))
        edges = face_edges(n)
        f4 = [fe[c] if off is None else _shift(fe[c], off, 1.0) for c, off in edges]
        c4 = [is_cut[c] if off is None else _shift(is_cut[c], off, False) for c, off in edges]
        p4 = [pec[c] if off is None else _shift(pec[c], off, True) for c, off in edges]
        a_geo = area_fraction(corners, f4, c4)
        wmax = np.maximum.reduce([np.where(p, 0.0, f) for p, f in zip(p4, f4)])
        a = np.maximum(a_geo, wmax / ratio)
        exists = np.ones(nin.shape, bool)
        for t in (a1, a2):
            sl = [slice(None)] * 3; sl[2 - t] = -1
            exists[tuple(sl)] = False
        full = corners[0] & corners[1] & corners[2] & corners[3]
        g4 = [np.where(p, 1.0, f / a) for p, f in zip(p4, f4)]      # a PEC edge carries no voltage: its g_e is left at 1
        listed = exists & ~full & ((a != 1.0) | np.logical_or.reduce([g != 1.0 for g in g4]))
        q = np.flatnonzero(listed)
        comp.append(np.full(q.size, n, np.int8)); idx.append(q.astype(np.int64))
        gs.append(np.stack([g.reshape(-1)[q] for g in g4], 1).reshape(-1, 4))
        aa.append(a.reshape(-1)[q]); ag.append(a_geo.reshape(-1)[q])
    idx = np.concatenate(idx)
    if idx.size == 0:
        return None
    return ConformalFaces(np.concatenate(comp), idx, np.concatenate(gs), np.concatenate(aa), np.concatenate(ag), ratio, frac)


# ---------------------------------------------------------------------------------------------------------------------------
# placement
# ---------------------------------------------------------------------------------------------------------------------------
def _metal_at(grid: RectGrid, conf: ConformalFaces, n: int, pos) -> str:
    """The metal whose surface cuts the face of component n at node pos: the first record that holds one of its corners."""
    table = conf.frac.table
    if table is None:
        return "?"
    a1, a2 = (n + 1) % 3, (n + 2) % 3
    for o1 in (0, 1):
        for o2 in (0, 1):
            p = list(pos); p[a1] += o1; p[a2] += o2
            if not conf.frac.node_in[p[2], p[1], p[0]]:
                continue
            xyz = [np.array([grid.lines[a][p[a]]]) for a in range(3)]
            for q in range(table.rec.size):
                if bool(_prims._inside(table.rec[q], table.verts, xyz[0], xyz[1], xyz[2], table.tol)[0]):
                    return table.names[q].split(":")[0]
    return "?"


def check_placement(grid: RectGrid, conf: ConformalFaces, cpml_cells: Sequence[int] = (0,) * 6, mur_faces: Sequence[int] = (0,) * 6,
                    magnetic_classes: Optional[np.ndarray] = None) -> None:
    """Refuse (ValueError, naming the metal and the node of the face) a listed face inside a CPML layer (the layers' psi recursion
    assumes the base operator), on or next to a Mur face, or that is also a magnetic face (both corrections would own I)."""
    nx, ny, nz = grid.shape
    n = (nx, ny, nz)
    k, r = np.divmod(conf.idx, nx * ny)
    j, i = np.divmod(r, nx)
    pos = (i, j, k)

    def refuse(mask, why):
        e = int(np.argmax(mask))
        c = int(conf.comp[e])
        p = (int(i[e]), int(j[e]), int(k[e]))
        raise ValueError(f"conformal metal '{_metal_at(grid, conf, c, p)}': the cut face at node {p} ({'xyz'[c]}) {why}")
    for f in range(6):
        ax, hi = f // 2, f % 2
        t = int(cpml_cells[f])
        if t > 0:
            m = (pos[ax] >= n[ax] - 2 - t) if hi else (pos[ax] <= t)
            if np.any(m):
                refuse(m, f"lies inside the CPML layer {'xyz'[ax]}{'+' if hi else '-'} ({t} cells): listed faces inside absorbing layers "
                          f"are not supported — keep curved metal clear of the layers")
        if int(mur_faces[f]):
            m = (pos[ax] >= n[ax] - 3) if hi else (pos[ax] <= 1)
            if np.any(m):
                refuse(m, f"lies on or next to the Mur face {'xyz'[ax]}{'+' if hi else '-'}: not supported")
    if magnetic_classes is not None:
        m = magnetic_classes.reshape(3, -1)[conf.comp.astype(np.int64), conf.idx] != 0
        if np.any(m):
            refuse(m, "is also a magnetic face (mu_r != 1 or sigma_m != 0 next to the metal): not supported")


# ---------------------------------------------------------------------------------------------------------------------------
# the engine's tables, its correction, and the equivalent raw operator
# ---------------------------------------------------------------------------------------------------------------------------
def iv0_at(hmet, comp, idx, shape) -> np.ndarray:
    """float32 iv0 of the given faces, as the engine expands it: hx[i] * (hy[j] * hz[k]) in float32 (ECOperator.raw's association)."""
    nx, ny, nz = shape
    k, r = np.divmod(np.asarray(idx, np.int64), nx * ny)
    j, i = np.divmod(r, nx)
    out = np.empty(len(idx), np.float32)
    for c in range(3):
        q = np.flatnonzero(np.asarray(comp) == c)
        hx, hy, hz = (np.asarray(t, np.float32) for t in hmet[c])
        out[q] = hx[i[q]] * (hy[j[q]] * hz[k[q]])
    return out


def tables(conf: ConformalFaces, hmet, shape):
    """(comp int8 [n], idx int64 [n], coef float32 [n][4]) of fdtd_conformal_set: coef = iv0 * g_e rounded to float32."""
    iv0 = iv0_at(hmet, conf.comp, conf.idx, shape).astype(np.float64)
    return conf.comp.astype(np.int8), conf.idx.astype(np.int64), (iv0[:, None] * conf.g).astype(np.float32)


def gather_offsets(comp, idx, shape):
    """(component [n][4], flat index [n][4]) of the four edges of every face, in face_edges order."""
    nx, ny, nz = shape
    st = (1, nx, nx * ny)
    comp, idx = np.asarray(comp, np.int64), np.asarray(idx, np.int64)
    ec = np.empty((idx.size, 4), np.int64); eo = np.empty((idx.size, 4), np.int64)
    for n in range(3):
        q = np.flatnonzero(comp == n)
        for e, (c, off) in enumerate(face_edges(n)):
            ec[q, e] = c
            eo[q, e] = idx[q] + (0 if off is None else st[off])
    return ec, eo


def correction(V: np.ndarray, i_prev: np.ndarray, comp, idx, coef: np.ndarray) -> np.ndarray:
    """The per-timestep correction of include/fdtd_hip_conformal.h in float32, statement for statement.  V: float32 [3][nz][ny][nx]
    after the E phase; i_prev float32 [n], updated in place; returns the listed faces' new currents float32 [n]."""
    f32 = np.float32
    V = np.asarray(V, f32)
    ec, eo = gather_offsets(comp, idx, V.shape[:0:-1])
    flat = V.reshape(3, -1)
    coef = np.asarray(coef, f32)
    t0 = coef[:, 0] * flat[ec[:, 0], eo[:, 0]]
    t1 = coef[:, 1] * flat[ec[:, 1], eo[:, 1]]
    t2 = coef[:, 2] * flat[ec[:, 2], eo[:, 2]]
    t3 = coef[:, 3] * flat[ec[:, 3], eo[:, 3]]
    d1 = (t0 - t1).astype(f32)
    d2 = (t2 - t3).astype(f32)
    s = (d1 - d2).astype(f32)
    r = (i_prev + s).astype(f32)
    i_prev[...] = r
    return r


def raw_operator(op, conf: Optional[ConformalFaces], k0: int = 0, nk: Optional[int] = None):
    """(vv, vi, ii, iv) float32 of the equivalent raw operator in the variables V' = f V: vi' = f vi on the cut edges, iv' = iv0 / a_f
    on the listed faces, the base operator's elsewhere.  For tests and the oracle (whole grids only)."""
    vv, vi, ii, iv = op.raw(k0, nk)
    if conf is None:
        return vv, vi, ii, iv
    if k0 != 0 or (nk is not None and nk != op.grid.shape[2]):
        raise ValueError("conformal.raw_operator: whole grids only")
    vi, iv = vi.copy(), iv.copy()
    fr = conf.frac
    v = vi.reshape(3, -1)
    v[fr.comp.astype(np.int64), fr.idx] = (v[fr.comp.astype(np.int64), fr.idx].astype(np.float64) * fr.f).astype(np.float32)
    w = iv.reshape(3, -1)
    c = conf.comp.astype(np.int64)
    w[c, conf.idx] = (w[c, conf.idx].astype(np.float64) / conf.a).astype(np.float32)
    return vv, vi, ii, iv
