"""Sub-cell averaged dielectric surfaces: curved and slanted dielectrics without the staircase's half-cell placement error.

This is the SPEC of the model (float64 numpy); csrc/voxel.hip (fdtd_voxel_subcell, include/fdtd_hip_subcell.h) gives the same list,
bit for bit.  Only the set-up learns it: a LISTED edge gets its own (eps_rel, kap_e), which reach the operator as per-edge (vv, m)
overrides next to the lumped ones.  No step kernel, schedule or correction changes, and the Courant limit stays (a mean of
eps >= 1 is >= 1).

Sub-voxel lattice.  nsub in {2, 4, 8} (powers of two: (s + 0.5) / nsub is exact).  Cell q = (i, j, k) has nsub^3 sub-voxels s; the
point of a sub-voxel along axis a is

    l_a[q_a] + ((s_a + 0.5) * (1.0 / nsub)) * (l_a[q_a + 1] - l_a[q_a]).

Owner of a point.  The candidates of cell q are the MATERIAL records (role 0) of primitives.pack_table whose cbox is not empty and
holds q once grown by one cell on every side and clipped to the grid.  (cbox holds every cell whose centre is in the padded bounding
box; a cell that overlaps the box but whose centre is outside neighbours one in it.  A primitive that holds no cell centre stays
invisible, as it is to the staircase.)  Among them, those that hold the point by the material predicate of include/fdtd_hip_voxel.h
(primitives._inside with t = -tol, called unchanged); the owner is the holding record of highest priority, the later record on a
tie, -1 if none.  Metals do not take part.

Values.  A point's values for component c are (eps_axes[c], kappa_axes[c]) of its owner's material (the scalars three times for an
isotropic one), (1, 0) without an owner.  A Debye, Lorentz or Drude material is NOT PLAIN (those folds add their own per-cell terms).

Samples of an edge.  The edge of component c at node n, a1 = (c + 1) % 3, a2 = (c + 2) % 3: along c the sub-voxels s_c = 0 .. nsub-1
of cell n_c; along a1 two halves, h1 = 0: cell n_a1 - 1 with s_a1 = nsub/2 .. nsub-1, h1 = 1: cell n_a1 with s_a1 = 0 .. nsub/2 - 1;
along a2 the same with h2.  Four quarters (h1, h2), each inside one cell, each (nsub/2)^2 columns of nsub samples: the edge's dual
volume.

Listed edges.  An edge is listed iff it is live by build_operator's own `dead` rule, carries no lumped override, none of its samples
is owned by a material that is not plain, and at least one of its four cells is MIXED for component c: the nsub^3 sub-voxels of that
cell do not all have the same value pair.  Values are compared, not owners: two overlapping records of one material, or a flat
interface on a mesh plane, list nothing.  The whole cell is looked at, not only the quarter the edge samples, because the staircase
gives a cell the material of its centre: with a surface at 0.49 of a cell the lower half cell is uniformly full, yet the plain mean
counts the cell as empty — the edges of BOTH node planes next to a mixed cell take their value from their own samples (which may
all be equal).  A cell whose sub-voxels agree is taken to agree with its centre: what is left is a sliver thinner than the lattice.
The list is ordered by component, then flat node index (as conformal.cut_edges).

Value of a listed edge, float64 with + - * / only, sequential in this order:

    ne = nk = den = 0
    for h1 in (0, 1): for h2 in (0, 1):
        w = d[a1][cell_a1] * d[a2][cell_a2]          # the plain mean's weight of that cell
        for s1 ascending: for s2 ascending:
            R = 0; K = 0
            for s_c ascending: R = R + 1.0 / eps_c(sample); K = K + kappa_c(sample)
            ne = ne + (nsub / R) * w                  # series along the edge: harmonic
            nk = nk + (K / nsub) * w                  # loss: arithmetic
            den = den + w
    eps_rel = ne / den ; kap_e = nk / den

Series capacitors along the edge, parallel ones across its dual face: the equivalent-circuit picture the operator is written in.
kappa is averaged arithmetically on purpose: a series combination of kappa + j w eps is not a constant, and a harmonic mean would
switch off the loss of every edge that touches air.

Left as it is, bounded by the lattice: a cell whose sub-voxels all agree while its centre (not sampled) belongs to another
material keeps the staircase's value; dispersive surfaces stay staircased; J dumps keep the plain edge conductivity on listed edges.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional
import numpy as np

from . import primitives as _prims
from .constants import EPS0
from .grid import RectGrid

NSUB = (2, 4, 8)
SKIP_LIVE, SKIP_DEAD, SKIP_LUMPED = 0, 1, 2
STATUS_MIXED, STATUS_NONPLAIN = 1, 2          # bits of the per-edge status: one of its four cells is mixed; a sample is not plain
LATTICE_POINTS = 1 << 23                      # sub-voxels the specification holds at a time (it walks the grid in z chunks)


def check_nsub(nsub) -> int:
    if nsub not in NSUB or int(nsub) != nsub:
        raise ValueError(f"subcell_samples = {nsub!r}: the sub-voxels per cell and axis must be 2, 4 or 8")
    return int(nsub)


@dataclass
class Listed:
    """The listed edges of a scene: per edge its component, the flat index of its node, eps_rel and kap_e; and what was dropped."""
    comp: np.ndarray               # int8 [n]
    idx: np.ndarray                # int64 [n]
    eps_rel: np.ndarray            # float64 [n]
    kap_e: np.ndarray              # float64 [n]
    nsub: int
    dropped_lumped: int = 0        # live edges with a mixed cell that carry a lumped override
    dropped_nonplain: int = 0      # ... without one, with a sample owned by a dispersive material

    def __len__(self) -> int:
        return int(self.idx.size)

    def edges(self) -> list:
        return [int(np.count_nonzero(self.comp == c)) for c in range(3)]


def prop_tables(scene):
    """(prop_eps float64 [nprop+1][3], prop_kap float64 [nprop+1][3], prop_plain uint8 [nprop+1]) of the scene's materials in scene
    order (the `prop` of a material record), the background (1, 0, plain) in the last row."""
    from .scene import DebyeMaterial, LorentzMaterial, DiscMaterial
    eps, kap, plain = [], [], []
    for m in scene.materials:
        if isinstance(m, DiscMaterial):
            raise ValueError(f"subcell: disc material '{m.name}' (AddDiscMaterial): sub-cell averaging of voxel body models is not supported")
        e, k = m.axes()
        eps.append([float(v) for v in e]); kap.append([float(v) for v in k])
        plain.append(0 if isinstance(m, (DebyeMaterial, LorentzMaterial)) else 1)
    eps.append([1.0] * 3); kap.append([0.0] * 3); plain.append(1)
    return np.array(eps, np.float64).reshape(-1, 3), np.array(kap, np.float64).reshape(-1, 3), np.array(plain, np.uint8)


def skip_mask(grid: RectGrid, pec: np.ndarray, lumped_edge=None, lumped_comp=None) -> np.ndarray:
    """uint8 [3][nz][ny][nx]: SKIP_DEAD on the edges build_operator holds dead (PEC, the non-existent last edges, the tangential
    edges of the six outer planes), SKIP_LUMPED on the live edges that carry a host-fixed override, SKIP_LIVE elsewhere."""
    nx, ny, nz = grid.shape
    out = np.zeros((3, nz, ny, nx), np.uint8)
    np_axis = {0: 2, 1: 1, 2: 0}
    for c in range(3):
        dead = np.asarray(pec[c], bool).copy()
        idx = [slice(None)] * 3
        idx[np_axis[c]] = -1
        dead[tuple(idx)] = True
        for a in range(3):
            if a == c:
                continue
            for side in (0, -1):
                idx = [slice(None)] * 3
                idx[np_axis[a]] = side
                dead[tuple(idx)] = True
        out[c][dead] = SKIP_DEAD
    if lumped_edge is not None and len(lumped_edge):
        flat = out.reshape(3, -1)
        cc, ee = np.asarray(lumped_comp, np.int64), np.asarray(lumped_edge, np.int64)
        live = flat[cc, ee] == SKIP_LIVE
        flat[cc[live], ee[live]] = SKIP_LUMPED
    return out


def grown_boxes(table: _prims.Table, shape):
    """Per record (lo [3], hi [3]) of its cbox grown by one cell and clipped to the grid, or None: a metal, or an empty cbox."""
    ncell = (shape[0] - 1, shape[1] - 1, shape[2] - 1)
    out = []
    for r in table.rec:
        b = [int(v) for v in r["cbox"]]
        lo = [max(b[a], 0) for a in range(3)]
        hi = [min(b[3 + a], ncell[a] - 1) for a in range(3)]
        if int(r["role"]) != _prims.ROLE_MATERIAL or any(hi[a] < lo[a] for a in range(3)):
            out.append(None)
            continue
        out.append(([max(lo[a] - 1, 0) for a in range(3)], [min(hi[a] + 1, ncell[a] - 1) for a in range(3)]))
    return out


def sub_points(lines: np.ndarray, q0: int, q1: int, nsub: int) -> np.ndarray:
    """The sub-voxel coordinates of cells q0 .. q1 (inclusive) along one axis, [(q1 - q0 + 1) * nsub]."""
    q = np.arange(q0, q1 + 1)
    f = (np.arange(nsub) + 0.5) * (1.0 / nsub)
    return (lines[q][:, None] + f[None, :] * (lines[q + 1] - lines[q])[:, None]).reshape(-1)


def lattice_props(grid: RectGrid, table: _prims.Table, nsub: int, kc0: int = 0, kc1: Optional[int] = None) -> np.ndarray:
    """uint16 [(kc1 - kc0) * nsub][(ny - 1) * nsub][(nx - 1) * nsub]: per sub-voxel of the cell planes kc0 .. kc1 - 1 the material
    (`prop`) of its owner, nprop (the background's row) without one; nprop = 1 + the largest prop of the table's material records."""
    nx, ny, nz = grid.shape
    kc1 = nz - 1 if kc1 is None else kc1
    rec = table.rec
    mat = rec["prop"][rec["role"] == _prims.ROLE_MATERIAL] if rec.size else np.zeros(0, np.int32)
    nprop = int(mat.max()) + 1 if mat.size else 0
    shape = ((kc1 - kc0) * nsub, (ny - 1) * nsub, (nx - 1) * nsub)
    pid = np.full(shape, nprop, np.uint16)
    prio = np.full(shape, np.iinfo(np.int32).min, np.int64)
    for r, box in zip(rec, grown_boxes(table, grid.shape)):
        if box is None:
            continue
        lo, hi = box
        z0, z1 = max(lo[2], kc0), min(hi[2], kc1 - 1)
        if z1 < z0:
            continue
        x = sub_points(grid.lines[0], lo[0], hi[0], nsub).reshape(1, 1, -1)
        y = sub_points(grid.lines[1], lo[1], hi[1], nsub).reshape(1, -1, 1)
        z = sub_points(grid.lines[2], z0, z1, nsub).reshape(-1, 1, 1)
        mask = _prims._inside(r, table.verts, x, y, z, table.tol)
        sl = (slice((z0 - kc0) * nsub, (z1 + 1 - kc0) * nsub), slice(lo[1] * nsub, (hi[1] + 1) * nsub), slice(lo[0] * nsub, (hi[0] + 1) * nsub))
        pr = int(r["priority"])
        win = mask & (prio[sl] <= pr)
        prio[sl][win] = pr
        pid[sl][win] = int(r["prop"])
    return pid


def _block_edges(d, pid, nsub, prop_eps, prop_kap, prop_plain):
    """The sums of the module docstring on one block of cells.  d: the three cell-size arrays of the block; pid: its lattice
    [ncz * nsub][ncy * nsub][ncx * nsub].  Per component c the tuple (status uint8, eps_rel, kap_e), each over the block's edges
    with interior nodes along a1 and a2 and every cell along c — in [z][y][x] order."""
    out = []
    h = nsub // 2
    for c in range(3):
        a1, a2 = (c + 1) % 3, (c + 2) % 3
        perm = (2 - c, 2 - a1, 2 - a2)
        P = np.transpose(pid, perm)
        nc, S1, S2 = P.shape[0] // nsub, P.shape[1], P.shape[2]
        M1, M2 = S1 // nsub - 1, S2 // nsub - 1
        if nc < 1 or M1 < 1 or M2 < 1:
            out.append(None)
            continue
        P = P.reshape(nc, nsub, S1, S2)
        eps = prop_eps[:, c][P]
        kap = prop_kap[:, c][P]
        R = np.zeros((nc, S1, S2)); K = np.zeros((nc, S1, S2))
        for s in range(nsub):
            R = R + 1.0 / eps[:, s]
            K = K + kap[:, s]
        H = nsub / R
        A = K / nsub
        emin, emax, kmin, kmax = eps.min(axis=1), eps.max(axis=1), kap.min(axis=1), kap.max(axis=1)
        bad = (prop_plain[P] == 0).any(axis=1)
        ne = np.zeros((nc, M1, M2)); nk = np.zeros((nc, M1, M2)); den = np.zeros((1, M1, M2))
        nonplain = np.zeros((nc, M1, M2), bool)
        # a cell is mixed when its sub-voxels differ in eps_c or kappa_c; an edge when one of its four cells is
        per_cell = lambda v, f: f(f(v.reshape(nc, M1 + 1, nsub, S2), axis=2).reshape(nc, M1 + 1, M2 + 1, nsub), axis=3)
        cmix = (per_cell(emin, np.min) != per_cell(emax, np.max)) | (per_cell(kmin, np.min) != per_cell(kmax, np.max))
        mixed = cmix[:, :-1, :-1] | cmix[:, 1:, :-1] | cmix[:, :-1, 1:] | cmix[:, 1:, 1:]
        n1, n2 = np.arange(1, M1 + 1), np.arange(1, M2 + 1)
        for h1 in (0, 1):
            for h2 in (0, 1):
                w = (d[a1][n1 - 1 + h1][:, None] * d[a2][n2 - 1 + h2][None, :])[None]
                for u1 in range(h):
                    for u2 in range(h):
                        t1, t2 = h1 * h + u1, h2 * h + u2
                        sl = (slice(None), slice(h + t1, h + t1 + (M1 - 1) * nsub + 1, nsub), slice(h + t2, h + t2 + (M2 - 1) * nsub + 1, nsub))
                        ne = ne + H[sl] * w
                        nk = nk + A[sl] * w
                        den = den + w
                        nonplain |= bad[sl]
        status = (mixed * STATUS_MIXED + nonplain * STATUS_NONPLAIN).astype(np.uint8)
        inv = np.argsort(perm)
        out.append(tuple(np.ascontiguousarray(np.transpose(v, inv)) for v in (status, ne / den, nk / den)))
    return out


def edges_spec(grid: RectGrid, table: _prims.Table, nsub: int, prop_eps, prop_kap, prop_plain, skip: np.ndarray,
               lattice_points: int = LATTICE_POINTS) -> Listed:
    """THE specification of fdtd_voxel_subcell: the listed edges of the module docstring.  skip: skip_mask's array."""
    nsub = check_nsub(nsub)
    nx, ny, nz = grid.shape
    if table.maps or (table.rec_map is not None and np.any(table.rec_map)):
        raise ValueError("subcell: a record that delimits a voxel map (AddDiscMaterial) is not supported")
    prop_eps, prop_kap = np.asarray(prop_eps, np.float64).reshape(-1, 3), np.asarray(prop_kap, np.float64).reshape(-1, 3)
    prop_plain = np.asarray(prop_plain, np.uint8).reshape(-1)
    mat = table.rec["prop"][table.rec["role"] == _prims.ROLE_MATERIAL] if table.rec.size else np.zeros(0, np.int32)
    nprop = prop_plain.size - 1
    if prop_eps.shape[0] != nprop + 1 or prop_kap.shape[0] != nprop + 1 or (mat.size and (mat.min() < 0 or mat.max() >= nprop)):
        raise ValueError("subcell: the property tables need one row per material of the table's records, and the background's")
    if skip.shape != (3, nz, ny, nx):
        raise ValueError("subcell: skip must be [3][nz][ny][nx]")
    # lattice_props numbers the background 1 + the largest prop it meets: map that onto the tables' last row
    found = int(mat.max()) + 1 if mat.size else 0
    comp, idx, eps_out, kap_out = [[], [], []], [[], [], []], [[], [], []], [[], [], []]
    dropped = [0, 0]
    d = [np.diff(l) for l in grid.lines]
    per_plane = (ny - 1) * (nx - 1) * nsub ** 3
    planes = max(2, int(lattice_points // per_plane))
    kc0 = 0
    while kc0 < nz - 1:
        kc1 = min(kc0 + planes, nz - 1)
        last = kc1 == nz - 1
        pid = lattice_props(grid, table, nsub, kc0, kc1)
        if found != nprop:
            pid = np.where(pid == found, nprop, pid).astype(np.uint16)
        res = _block_edges([d[0], d[1], d[2][kc0:kc1]], pid, nsub, prop_eps, prop_kap, prop_plain)
        for c in range(3):
            if res[c] is None:
                continue
            status, er, ke = res[c]
            # the block's edges in global nodes: interior along a1, a2 (z: the chunk's), every cell along c (z: all but the chunk's last)
            if c == 2:
                nkz = status.shape[0] if last else status.shape[0] - 1
                zs = slice(kc0, kc0 + nkz)
                status, er, ke = status[:nkz], er[:nkz], ke[:nkz]
                sl = (zs, slice(1, ny - 1), slice(1, nx - 1))
            else:
                sl = (slice(kc0 + 1, kc1), slice(1, ny - 1) if c == 0 else slice(0, ny - 1), slice(0, nx - 1) if c == 0 else slice(1, nx - 1))
            if status.size == 0:
                continue
            sk = skip[c][sl]
            mixed = (status & STATUS_MIXED) != 0
            bad = (status & STATUS_NONPLAIN) != 0
            dropped[0] += int(np.count_nonzero(mixed & (sk == SKIP_LUMPED)))
            dropped[1] += int(np.count_nonzero(mixed & bad & (sk == SKIP_LIVE)))
            lst = mixed & ~bad & (sk == SKIP_LIVE)
            kk, jj, ii = np.nonzero(lst)
            g = ((kk + sl[0].start).astype(np.int64) * ny + (jj + sl[1].start)) * nx + (ii + sl[2].start)
            comp[c].append(np.full(g.size, c, np.int8)); idx[c].append(g)
            eps_out[c].append(er[lst]); kap_out[c].append(ke[lst])
        if last:
            break
        kc0 = kc1 - 1

    def cat(parts, dtype):
        flat = [p for c in range(3) for p in parts[c]]
        return np.concatenate(flat).astype(dtype) if flat else np.zeros(0, dtype)
    return Listed(cat(comp, np.int8), cat(idx, np.int64), cat(eps_out, np.float64), cat(kap_out, np.float64), nsub, dropped[0], dropped[1])


def listed(scene, grid: RectGrid, nsub: int, pec: np.ndarray, lumped_edge=None, lumped_comp=None, device_subcell=None,
           table: Optional[_prims.Table] = None) -> Listed:
    """The listed edges of a scene.  `device_subcell(grid, table, nsub, prop_eps, prop_kap, prop_plain, skip) -> Listed`:
    _capi.default_subcell's callable (csrc/voxel.hip); None: numpy."""
    nsub = check_nsub(nsub)
    tabs = prop_tables(scene)
    table = _prims.pack_table(scene, grid) if table is None else table
    skip = skip_mask(grid, pec, lumped_edge, lumped_comp)
    fn = edges_spec if device_subcell is None else device_subcell
    return fn(grid, table, nsub, tabs[0], tabs[1], tabs[2], skip)


def overrides(ls: Listed, dt: float, dtype=np.float32):
    """(edge int64, comp int8, vv, m) of the listed edges, with exactly the expressions of ecoperator.build_operator."""
    eps_e = ls.eps_rel * EPS0
    x = 0.5 * dt * ls.kap_e / eps_e
    vv = (1.0 - x) / (1.0 + x)
    m = dt / (eps_e * (1.0 + x))
    return ls.idx.astype(np.int64), ls.comp.astype(np.int8), vv.astype(dtype), m.astype(dtype)
