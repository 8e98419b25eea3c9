"""Magnetic materials: relative permeability mu_r >= 1 and magnetic loss sigma* [ohm/m] on the face currents.

This is the SPEC of the model (float64) and of the correction the engine applies (float32, include/fdtd_hip_magnetic.h).

The face current I_c at (i, j, k) lives on a dual edge: it runs along c through the two cells on either side of node plane
pos[c], with half-lengths l1 (the cell below) and l2 (the cell above), l1 + l2 = grid.dd[c][pos[c]] (a boundary line follows
grid.dd's convention: the full adjacent cell, the missing side has length 0).  Normal B is continuous, so the two cells are
reluctances in series:

    s = (l1/mu_r1 + l2/mu_r2) / (l1 + l2)              L = mu0 A / ((l1 + l2) s)
    x = (dt/2) (l1 sigma*_1/mu_1 + l2 sigma*_2/mu_2) / (l1 + l2)          (absolute mu)
    a = (1 - x) / (1 + x)        b = s / (1 + x)

and the update wanted is  I <- a I + b iv0 curl,  iv0 the operator's own coefficient (ecoperator: ii = 1, iv0 = dt/L(mu0)).  A
face with a = 1 and b = 1 exactly is not magnetic.  The operator and the H kernels stay what they are; `correction` below is what
the engine runs after the H update of every timestep (k_magnetic), restated in numpy statement for statement.  `raw_ii_iv` expands
the same coefficients into the ii / iv arrays of the raw operator form — for tests and the oracle only: the product never runs a
magnetic scene in raw form.

The timestep comes from grid.courant_dt() alone, so mu_r < 1 (a wave faster than c0 / sqrt(eps_r)) is refused.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence
import numpy as np

from .constants import MU0
from .grid import RectGrid

MAX_CLASSES = 255       # one class byte per face, 0 = not magnetic


def check_material(name: str, mu_r, sigma_m) -> None:
    """Refuse (ValueError, naming the material) what the model does not cover: anisotropic values (sequences), non-finite or
    negative values, mu_r < 1."""
    for what, v in (("mu_r", mu_r), ("sigma_m", sigma_m)):
        if isinstance(v, (str, bytes)) or np.ndim(v) != 0:
            raise ValueError(f"material '{name}': {what} = {v!r} is anisotropic (a sequence): only isotropic magnetic materials are supported")
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"material '{name}': {what} = {v!r} is not a number") from None
        if not np.isfinite(f) or f < 0:
            raise ValueError(f"material '{name}': {what} = {f!r} must be finite and non-negative")
    if float(mu_r) < 1.0:
        raise ValueError(f"material '{name}': mu_r = {float(mu_r)!r} < 1 is not supported (the timestep comes from the mesh alone: "
                         f"a medium faster than vacuum would be unstable)")


def _name_at(cell_material, names, k, j, i) -> str:
    if cell_material is None or names is None:
        return "?"
    q = int(cell_material[k, j, i])
    return names[q] if 0 <= q < len(names) else "(background)"


def check_cells(grid: RectGrid, mu_r: np.ndarray, sigma_m: np.ndarray, cpml_cells: Sequence[int] = (0,) * 6,
                cell_material: Optional[np.ndarray] = None, names: Optional[Sequence[str]] = None) -> None:
    """Refuse (ValueError, naming the material and the node of the cell) per-cell values the model does not cover, and magnetic
    cells inside CPML layers (`cpml_cells`: layer thickness in cells per face, x-, x+, y-, ...) — the Debye media's rule: the
    layers' psi recursion assumes the base operator."""
    nx, ny, nz = grid.shape
    if mu_r.shape != (nz - 1, ny - 1, nx - 1) or sigma_m.shape != mu_r.shape:
        raise ValueError("mu_r and sigma_m must be per cell, [nz-1][ny-1][nx-1]")

    def first(mask):
        k, j, i = (int(v[0]) for v in np.nonzero(mask))
        return k, j, i

    bad = ~np.isfinite(mu_r) | ~np.isfinite(sigma_m) | (sigma_m < 0) | (mu_r < 0)
    if np.any(bad):
        k, j, i = first(bad)
        raise ValueError(f"material '{_name_at(cell_material, names, k, j, i)}': the cell at node {(i, j, k)} has mu_r = {mu_r[k, j, i]!r}, "
                         f"sigma_m = {sigma_m[k, j, i]!r}: must be finite and non-negative")
    low = mu_r < 1.0
    if np.any(low):
        k, j, i = first(low)
        raise ValueError(f"material '{_name_at(cell_material, names, k, j, i)}': the cell at node {(i, j, k)} has mu_r = {mu_r[k, j, i]!r} < 1: "
                         f"not supported (the timestep comes from the mesh alone)")
    mag = (mu_r != 1.0) | (sigma_m != 0.0)
    n = grid.shape
    for f in range(6):
        t = int(cpml_cells[f])
        if t <= 0:
            continue
        ax = f // 2
        sl = [slice(None)] * 3
        sl[2 - ax] = slice(n[ax] - 1 - t, None) if f % 2 else slice(0, t)
        sub = np.zeros_like(mag)
        sub[tuple(sl)] = mag[tuple(sl)]
        if np.any(sub):
            k, j, i = first(sub)
            raise ValueError(f"magnetic material '{_name_at(cell_material, names, k, j, i)}' reaches into the CPML layer "
                             f"{'xyz'[ax]}{'+' if f % 2 else '-'} ({t} cells) with the cell at node {(i, j, k)}: magnetic cells inside "
                             f"absorbing layers are not supported — end the medium before the layer or use Mur faces")


def face_coefficients(grid: RectGrid, mu_r: np.ndarray, sigma_m: np.ndarray, dt: float):
    """(a, b, s) float64 [3][nz][ny][nx] of every face current, from the per-cell mu_r and sigma_m [nz-1][ny-1][nx-1].  Faces that
    do not exist (the last index along either transverse axis) get a = b = s = 1."""
    nx, ny, nz = grid.shape
    shape = (nz, ny, nx)
    n = (nx, ny, nz)
    inv = np.ones(shape)
    inv[:-1, :-1, :-1] = 1.0 / mu_r
    sg = np.zeros(shape)
    sg[:-1, :-1, :-1] = sigma_m / (MU0 * mu_r)
    a = np.ones((3,) + shape)
    b = np.ones((3,) + shape)
    s = np.ones((3,) + shape)
    for c in range(3):
        ax = 2 - c
        d = grid.d[c]
        l1 = np.zeros(n[c]); l2 = np.zeros(n[c])
        l1[1:-1] = 0.5 * d[:-2]; l1[-1] = d[-2]
        l2[1:-1] = 0.5 * d[1:-1]; l2[0] = d[0]
        w2 = l2 / (l1 + l2)                          # weight of the upper cell: 1 on the first line, 0 on the last
        vshape = [1, 1, 1]; vshape[ax] = n[c]
        w2 = w2.reshape(vshape)

        def below_above(cell):
            """The cell quantity of the cell below and above every node plane along c (a missing side repeats the other)."""
            up = cell.copy()
            idx = [slice(None)] * 3; idx[ax] = -1
            src = [slice(None)] * 3; src[ax] = -2
            up[tuple(idx)] = cell[tuple(src)]
            dn = np.roll(up, 1, axis=ax)
            idx[ax] = 0
            dn[tuple(idx)] = up[tuple(idx)]
            return dn, up

        i1, i2 = below_above(inv)
        g1, g2 = below_above(sg)
        s_c = i1 + w2 * (i2 - i1)                    # = (l1/mu_r1 + l2/mu_r2) / (l1 + l2); exactly 1/mu_r where the two cells agree
        x = 0.5 * dt * (g1 + w2 * (g2 - g1))
        a_c = (1.0 - x) / (1.0 + x)
        b_c = s_c / (1.0 + x)
        for t in ((c + 1) % 3, (c + 2) % 3):         # faces that do not exist
            idx = [slice(None)] * 3; idx[2 - t] = -1
            a_c[tuple(idx)] = 1.0; b_c[tuple(idx)] = 1.0; s_c[tuple(idx)] = 1.0
        a[c], b[c], s[c] = a_c, b_c, s_c
    return a, b, s


@dataclass
class MagneticFaces:
    """The magnetic faces of a scene at one dt: float64 coefficients over the whole grid, float32 class tables (classes 1..ncls) and
    per component the tight box of the magnetic faces with one class byte per face (0: not magnetic)."""
    a: np.ndarray                      # float64 [3][nz][ny][nx]
    b: np.ndarray
    s: np.ndarray
    tab_a: np.ndarray                  # float32 [ncls]
    tab_b: np.ndarray
    lo: list = field(default_factory=list)      # per component (i0, j0, k0)
    hi: list = field(default_factory=list)      # per component (i1, j1, k1), exclusive
    cls: list = field(default_factory=list)     # per component uint8 [z][y][x] over the box
    media: List[str] = field(default_factory=list)

    def __len__(self) -> int:
        return int(sum(int(np.count_nonzero(c)) for c in self.cls))

    @property
    def ncls(self) -> int:
        return int(self.tab_a.size)

    def faces(self) -> list:
        return [int(np.count_nonzero(c)) for c in self.cls]

    def full_classes(self, shape) -> np.ndarray:
        """Class bytes over the whole grid, uint8 [3][nz][ny][nx]."""
        out = np.zeros((3,) + tuple(shape), np.uint8)
        for c in range(3):
            (i0, j0, k0), (i1, j1, k1) = self.lo[c], self.hi[c]
            if self.cls[c].size:
                out[c, k0:k1, j0:j1, i0:i1] = self.cls[c]
        return out

    def tables(self):
        """(a, b, lo, hi, cls) of fdtd_magnetic_set (Engine.set_magnetic)."""
        return self.tab_a, self.tab_b, self.lo, self.hi, self.cls


def make_faces(grid: RectGrid, mu_r: np.ndarray, sigma_m: np.ndarray, dt: float, media: Sequence[str] = ()) -> Optional[MagneticFaces]:
    """Coefficients -> classes -> per-component boxes -> tables; None when the scene has no magnetic face."""
    mu_r, sigma_m = np.asarray(mu_r, np.float64), np.asarray(sigma_m, np.float64)
    if not (np.any(mu_r != 1.0) or np.any(sigma_m != 0.0)):
        return None
    a, b, s = face_coefficients(grid, mu_r, sigma_m, dt)
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    on = (a != 1.0) | (b != 1.0)
    if not np.any(on):
        return None
    key = (a32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | b32.view(np.uint32).astype(np.uint64)
    uniq, inv = np.unique(key[on], return_inverse=True)
    if uniq.size > MAX_CLASSES:
        raise ValueError(f"magnetic materials: {uniq.size} distinct (a, b) face classes on this mesh, at most {MAX_CLASSES} "
                         f"(one class byte per face): use fewer different media or a less finely graded mesh inside them")
    full = np.zeros(a.shape, np.uint8)
    full[on] = (inv + 1).astype(np.uint8)
    tab_a = (uniq >> np.uint64(32)).astype(np.uint32).view(np.float32).copy()
    tab_b = (uniq & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32).copy()
    lo, hi, cls = [], [], []
    for c in range(3):
        nzr = np.nonzero(full[c])
        if nzr[0].size == 0:
            lo.append((0, 0, 0)); hi.append((0, 0, 0)); cls.append(np.zeros((0, 0, 0), np.uint8))
            continue
        k0, j0, i0 = (int(v.min()) for v in nzr)
        k1, j1, i1 = (int(v.max()) + 1 for v in nzr)
        lo.append((i0, j0, k0)); hi.append((i1, j1, k1))
        cls.append(np.ascontiguousarray(full[c, k0:k1, j0:j1, i0:i1]))
    return MagneticFaces(a, b, s, tab_a, tab_b, lo, hi, cls, list(media))


def raw_ii_iv(op, mag: Optional[MagneticFaces], k0: int = 0, nk: Optional[int] = None):
    """(ii, iv) float32 [3][nk][ny][nx] of the raw operator form with the magnetic faces in it: ii = a, iv = b * iv0 on the faces of
    a class (the float32 table values the engine's correction uses), the base operator's elsewhere.  For tests and the oracle."""
    _, _, ii, iv = op.raw(k0, nk)
    if mag is None:
        return ii, iv
    nx, ny, nz = op.grid.shape
    nk = nz - k0 if nk is None else nk
    full = mag.full_classes((nz, ny, nx))[:, k0:k0 + nk]
    on = full != 0
    ta = np.concatenate([[np.float32(1)], mag.tab_a]).astype(np.float32)
    tb = np.concatenate([[np.float32(1)], mag.tab_b]).astype(np.float32)
    ii = np.where(on, ta[full], ii).astype(np.float32)
    iv = np.where(on, tb[full] * iv, iv).astype(np.float32)
    return ii, iv


def correction(I: np.ndarray, i_prev: np.ndarray, cls: np.ndarray, tab_a: np.ndarray, tab_b: np.ndarray) -> np.ndarray:
    """The per-timestep correction of include/fdtd_hip_magnetic.h in float32, statement for statement.  I, i_prev, cls: any one
    shape; tab_a, tab_b: the live classes' tables (class q > 0 takes entry q - 1).  Faces of class 0 keep I and i_prev.  i_prev is
    updated in place; returns I_new."""
    f32 = np.float32
    ta = np.concatenate([[f32(1)], np.asarray(tab_a, f32)]).astype(f32)
    tb = np.concatenate([[f32(1)], np.asarray(tab_b, f32)]).astype(f32)
    a, b = ta[cls], tb[cls]
    I = np.asarray(I, f32)
    d = I - i_prev
    p = a * i_prev
    q = b * d
    r = p + q
    on = cls != 0
    out = np.where(on, r, I).astype(f32)
    i_prev[...] = np.where(on, r, i_prev)
    return out


def inductance(grid: RectGrid, s: np.ndarray) -> np.ndarray:
    """L = mu0 A / (l~ s) of every face current, float64 [3][nz][ny][nx] (0 on faces that do not exist): the stored magnetic
    energy is 1/2 sum L I^2."""
    nx, ny, nz = grid.shape
    L = np.zeros((3, nz, ny, nx))
    for c in range(3):
        a1, a2 = (c + 1) % 3, (c + 2) % 3

        def along(ax, v):
            shp = [1, 1, 1]; shp[2 - ax] = v.size
            return v.reshape(shp)
        d1, d2 = grid.d[a1].copy(), grid.d[a2].copy()
        d1[-1] = 0.0; d2[-1] = 0.0
        L[c] = MU0 * along(a1, d1) * along(a2, d2) / (along(c, grid.dd[c]) * s[c])
    return L
