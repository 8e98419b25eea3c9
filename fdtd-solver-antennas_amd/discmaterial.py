"""Voxel body models (CSXCAD's CSPropDiscMaterial, ``CSX.AddDiscMaterial``): a segmented phantom — one tissue index per voxel of its
own rectilinear mesh, and a small table of eps_r, kappa and density per tissue — as plain data, its validation, the lookup rule that
csrc/voxel.hip repeats on the device (``lookup_spec`` is the specification), and the .npz round trip.

The lookup rule (include/fdtd_hip_voxel.h spells it for the device): with M the 3 x 4 world-to-map matrix (metres to map coordinates:
the scene's unit, the map's scale and the inverse of its placement folded on the host), a point (x, y, z) has the map coordinates
q_x = ((M0 x + M1 y) + M2 z) + M3, q_y and q_z with M4..7 and M8..11; per axis i_a = (the number of lines L_a[t] <= q_a) - 1, and the
point has a voxel iff 0 <= i_a <= n_a - 2 on all three axes (half-open: L[0] <= q < L[n - 1]; a NaN has none).  Its voxel is
v = data[(i_z (nY - 1) + i_y) (nX - 1) + i_x]; the map *holds* the point iff it has a voxel and (v != 0 or use_db_background).  Only
comparisons follow the three q, so the device's verdicts and voxel indices are numpy's bit for bit.
"""
from __future__ import annotations

import os
import zipfile
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

MAX_MAPS = 4                     # per scene
MAX_VOXELS = (1 << 31) - 1       # per map: a voxel's linear index is an int32 in cell_voxel
NPZ_KEYS = ("mesh_x", "mesh_y", "mesh_z", "DiscData", "epsR", "kappa", "density")    # upstream's HDF5 dataset names


@dataclass
class VoxelMap:
    name: str
    lines: Tuple[np.ndarray, np.ndarray, np.ndarray]    # float64, strictly increasing, the map's own drawing unit
    data: np.ndarray                                    # uint8 [nZ-1][nY-1][nX-1]: the tissue index of voxel (i, j, k)
    eps_r: np.ndarray                                   # float64 [db_size]; entry 0: the background
    kappa: np.ndarray
    density: np.ndarray
    scale: float = 1.0
    matrix: Optional[np.ndarray] = None                 # 4x4 map coordinates (times scale) -> the scene's drawing coordinates
    use_db_background: bool = False

    @property
    def db_size(self) -> int:
        return int(self.eps_r.size)

    @property
    def shape(self) -> Tuple[int, int, int]:
        """Voxels per axis (x, y, z)."""
        return tuple(int(l.size) - 1 for l in self.lines)

    def world_to_map(self, unit: float) -> np.ndarray:
        """M[12]: the 3 x 4 matrix from world metres to map coordinates."""
        return _world_to_map(self.name, self.scale, self.matrix, unit)


def _world_to_map(name, scale, matrix, unit) -> np.ndarray:
    F = np.eye(4) if matrix is None else np.array(matrix, dtype=float)      # map -> metres: unit * (matrix @ (scale * q))
    F = F.copy()
    F[:3, :3] *= float(scale)
    F[:3, :] *= float(unit)
    with np.errstate(all="ignore"):
        ok = np.isfinite(np.linalg.det(F[:3, :3])) and abs(np.linalg.det(F[:3, :3])) > 1e-300 and np.linalg.cond(F[:3, :3]) < 1e12
    if not ok:
        raise ValueError(f"disc material '{name}': the placement matrix is singular")
    return np.ascontiguousarray(np.linalg.inv(F)[:3, :].reshape(12))


def make_map(name, lines, data, eps_r, kappa, density, scale=1.0, matrix=None, use_db_background=False, mue_r=None, sigma=None) -> VoxelMap:
    """A validated VoxelMap; ValueError names the map and the offending thing.  mue_r / sigma: a table's magnetic columns, which must
    be 1 / 0 (magnetic tissue is out of scope)."""
    who = f"disc material '{name}'"
    if len(lines) != 3:
        raise ValueError(f"{who}: lines must be the three arrays (X, Y, Z)")
    L = []
    for a, l in zip("XYZ", lines):
        l = np.ascontiguousarray(np.asarray(l, dtype=np.float64).reshape(-1))
        if l.size < 2:
            raise ValueError(f"{who}: mesh lines {a}: at least 2 lines expected, got {l.size}")
        if not np.all(np.isfinite(l)) or not np.all(np.diff(l) > 0):
            raise ValueError(f"{who}: mesh lines {a} must be finite and strictly increasing")
        L.append(l)
    nvox = [l.size - 1 for l in L]
    if nvox[0] * nvox[1] * nvox[2] > MAX_VOXELS:
        raise ValueError(f"{who}: {nvox[0]} x {nvox[1]} x {nvox[2]} voxels: at most {MAX_VOXELS} (2^31 - 1) are supported")
    d = np.asarray(data)
    if d.dtype != np.uint8:
        if not np.issubdtype(d.dtype, np.integer) or (d.size and (d.min() < 0 or d.max() > 255)):
            raise ValueError(f"{who}: data must be tissue indices 0..255 (uint8), got dtype {d.dtype}")
        d = d.astype(np.uint8)
    if d.shape != (nvox[2], nvox[1], nvox[0]):
        raise ValueError(f"{who}: data has shape {d.shape}, the mesh lines need [nZ-1][nY-1][nX-1] = {(nvox[2], nvox[1], nvox[0])}")
    tab = {}
    for key, v, lo in (("eps_r", eps_r, 1.0), ("kappa", kappa, 0.0), ("density", density, 0.0)):
        v = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
        if not np.all(np.isfinite(v)) or np.any(v < lo):
            raise ValueError(f"{who}: table {key} must be finite and >= {lo:g}, got {v.tolist()}")
        tab[key] = v
    n = tab["eps_r"].size
    if n < 1 or n > 256 or tab["kappa"].size != n or tab["density"].size != n:
        raise ValueError(f"{who}: the tissue table needs eps_r, kappa and density of one length 1..256, got "
                         f"{n}, {tab['kappa'].size} and {tab['density'].size}")
    for key, v, want in (("mueR", mue_r, 1.0), ("sigma", sigma, 0.0)):
        if v is not None and (np.size(v) not in (0, n) or np.any(np.asarray(v, float) != want)):
            raise ValueError(f"{who}: table {key} must be {want:g} for every tissue: magnetic tissue is out of scope")
    if int(d.max()) >= n:
        raise ValueError(f"{who}: data holds tissue index {int(d.max())}, the table has {n} entries (db_size)")
    s = float(scale)
    if not (np.isfinite(s) and s > 0):
        raise ValueError(f"{who}: scale = {scale!r} must be > 0")
    M = None
    if matrix is not None:
        M = np.array(matrix, dtype=float)
        if M.shape != (4, 4) or not np.all(np.isfinite(M)):
            raise ValueError(f"{who}: the placement matrix must be 4 x 4 and finite")
    _world_to_map(name, s, M, 1.0)            # a singular placement is refused here, not at voxelisation
    return VoxelMap(str(name), tuple(L), np.ascontiguousarray(d), tab["eps_r"], tab["kappa"], tab["density"], s, M, bool(use_db_background))


def lookup_spec(M, lines, data, use_db_background, x, y, z):
    """(held bool, voxel int64) over the broadcast of the world coordinates x, y, z [m]: THE lookup rule.  voxel is the linear index
    into data (x fastest), -1 where the point has no voxel."""
    m = [float(v) for v in M]
    q = (((m[0] * x + m[1] * y) + m[2] * z) + m[3],
         ((m[4] * x + m[5] * y) + m[6] * z) + m[7],
         ((m[8] * x + m[9] * y) + m[10] * z) + m[11])
    shape = np.broadcast(x, y, z).shape
    ok = np.ones(shape, bool)
    idx = []
    for a in range(3):
        qa = np.broadcast_to(q[a], shape)
        i = np.where(np.isnan(qa), -1, np.searchsorted(lines[a], qa, side="right").astype(np.int64) - 1)   # (number of L[t] <= q) - 1
        ok &= (i >= 0) & (i <= lines[a].size - 2)
        idx.append(i)
    nX, nY = lines[0].size - 1, lines[1].size - 1
    lin = np.where(ok, (idx[2] * nY + idx[1]) * nX + idx[0], -1)
    v = np.asarray(data).reshape(-1)[np.maximum(lin, 0)]
    held = ok & ((v != 0) | bool(use_db_background))
    return held, lin


def save_npz(path, vmap: VoxelMap) -> None:
    """The map's mesh, voxels and table under upstream's dataset names (placement, scale and use_db_background are arguments of
    AddDiscMaterial, not part of the file)."""
    np.savez_compressed(path, mesh_x=vmap.lines[0], mesh_y=vmap.lines[1], mesh_z=vmap.lines[2], DiscData=vmap.data, epsR=vmap.eps_r,
                        kappa=vmap.kappa, density=vmap.density, mueR=np.ones(vmap.db_size), sigma=np.zeros(vmap.db_size))


def load_npz(path, name=None, scale=1.0, matrix=None, use_db_background=False) -> VoxelMap:
    path = os.fspath(path)
    name = os.path.basename(path) if name is None else name
    if os.path.splitext(path)[1].lower() in (".h5", ".hdf5"):
        raise ValueError(f"disc material '{name}': '{path}' is an HDF5 file, which this backend cannot read (no h5py): convert it to an "
                         f".npz holding the same datasets {', '.join(NPZ_KEYS)} (discmaterial.save_npz writes one)")
    try:
        with np.load(path, allow_pickle=False) as f:
            missing = [k for k in NPZ_KEYS if k not in f.files]
            if missing:
                raise ValueError(f"disc material '{name}': '{path}' lacks {', '.join(missing)} (expected: {', '.join(NPZ_KEYS)})")
            g = {k: f[k] for k in f.files}
    except (OSError, EOFError, zipfile.BadZipFile) as e:
        raise ValueError(f"disc material '{name}': cannot read '{path}': {e}") from None
    return make_map(name, (g["mesh_x"], g["mesh_y"], g["mesh_z"]), g["DiscData"], g["epsR"], g["kappa"], g["density"], scale, matrix,
                    use_db_background, mue_r=g.get("mueR"), sigma=g.get("sigma"))
