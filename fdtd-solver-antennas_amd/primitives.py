"""Curved and polygonal CSXCAD primitives as plain data, the flat table both rasterisers read, and the numpy rasteriser that is
the specification of csrc/voxel.hip (``rasterise_spec``; the device kernel must give the same owners, bit for bit).

The inside tests are float64 with ``+ - *`` and comparisons only (no division, no square root: distances are compared squared), in
the operation order include/fdtd_hip_voxel.h spells; ``_inside`` below and ``vx_test`` in csrc/voxel.hip are that text twice.

Two rules, as for boxes (scene._tol): a *material* owns a cell whose centre is strictly inside (every radius and half-width shrunk
by tol, a polygon point within tol of an edge is outside); a *metal* holds a node that is inside or within tol of the surface
(radii grow by tol, a polygon point within tol of an edge is inside).  Ownership: the highest priority wins, the later primitive
on a tie (materials in scene order, then drawing order inside a material); an edge is metal when ONE primitive holds both its end
nodes.  Curves (and the centre line of a wire) are snapped to grid edges on the host (``snap_curve``).

A ``Polyhedron`` is a closed triangle mesh (stl.read_stl gives one): inside is the parity of the crossings of the ray towards +x, with
the polygon's tol rule for points within tol of a triangle (``_tri_into``; DESIGN 6.1 says why the edges are taken in canonical order).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple
import numpy as np

from . import discmaterial as _disc

T_BOX, T_SPHERE, T_SPHERICAL_SHELL, T_CYLINDER, T_CYLINDRICAL_SHELL, T_DISC, T_POLYGON, T_LINPOLY, T_WIRE = range(9)
N_TYPES = 9                # the analytic types above; the triangle mesh is appended after them
T_POLYHEDRON = 9
N_TYPES_ALL = 10           # == FDTD_VOXEL_NTYPES
MAX_TRIANGLES = 1 << 20    # per record
ROLE_MATERIAL, ROLE_METAL = 0, 1
N_PAR = 8

# one record of the table == struct fdtd_voxel_prim (include/fdtd_hip_voxel.h), 248 bytes
RECORD = np.dtype([("type", "<i4"), ("role", "<i4"), ("prop", "<i4"), ("priority", "<i4"), ("order", "<i4"), ("vert0", "<i4"),
                   ("nvert", "<i4"), ("norm_dir", "<i4"), ("has_matrix", "<i4"), ("pad", "<i4"),
                   ("cbox", "<i4", 6), ("nbox", "<i4", 6), ("par", "<f8", N_PAR), ("m", "<f8", 12)])
assert RECORD.itemsize == 248


@dataclass
class _Prim:
    priority: int = 0
    matrix: Optional[np.ndarray] = None      # 4x4 local->world (drawing units), None = identity: as scene.Box.matrix


@dataclass
class Cylinder(_Prim):
    start: Tuple[float, float, float] = (0.0, 0.0, 0.0)   # axis end points, any direction; start == stop: a flat disc normal to local z
    stop: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    radius: float = 0.0


@dataclass
class CylindricalShell(_Prim):
    start: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    stop: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    radius: float = 0.0                       # mean radius
    shell_width: float = 0.0


@dataclass
class Sphere(_Prim):
    center: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    radius: float = 0.0


@dataclass
class SphericalShell(_Prim):
    center: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    radius: float = 0.0                       # mean radius
    shell_width: float = 0.0


@dataclass
class Polygon(_Prim):
    """A flat, zero-thickness polygon: points 2 x N in the plane normal to norm_dir (axes (n+1)%3, (n+2)%3) at `elevation`."""
    points: np.ndarray = None
    norm_dir: int = 2
    elevation: float = 0.0


@dataclass
class LinPoly(Polygon):
    """The polygon extruded along norm_dir from elevation to elevation + length."""
    length: float = 0.0


@dataclass
class Curve(_Prim):
    """A polyline (points 3 x N) of zero cross-section, metals only: snapped to grid edges."""
    points: np.ndarray = None


@dataclass
class Wire(Curve):
    """A curve with a radius: its snapped path plus the volume of its cylinders and joint spheres."""
    radius: float = 0.0


@dataclass
class Polyhedron(_Prim):
    """A closed triangle mesh: triangles [ntri][3][3] (triangle, corner A B C, x y z) in drawing units.  Facet normals and the winding
    of a triangle do not matter; every edge must be used by an even number of triangles (pack_table refuses an open mesh)."""
    triangles: np.ndarray = None


NEW_TYPES = (Cylinder, CylindricalShell, Sphere, SphericalShell, Polygon, LinPoly, Curve, Wire, Polyhedron)


def _f3(v, what):
    a = np.asarray(v, float).reshape(-1)
    if a.size != 3 or not np.all(np.isfinite(a)):
        raise ValueError(f"{what}: three finite coordinates expected, got {v!r}")
    return tuple(float(x) for x in a)


def make(kind: str, priority=0, **kw) -> _Prim:
    """A validated primitive: kind is the class name; coordinates in drawing units."""
    p = int(priority)

    def pos(name, strict=True):
        v = float(kw[name])
        if not np.isfinite(v) or v < 0 or (strict and v == 0):
            raise ValueError(f"{kind}: {name} must be {'> 0' if strict else '>= 0'}, got {kw[name]!r}")
        return v
    if kind == "Cylinder":
        return Cylinder(p, None, _f3(kw["start"], kind), _f3(kw["stop"], kind), pos("radius"))
    if kind == "CylindricalShell":
        return CylindricalShell(p, None, _f3(kw["start"], kind), _f3(kw["stop"], kind), pos("radius"), pos("shell_width"))
    if kind == "Sphere":
        return Sphere(p, None, _f3(kw["center"], kind), pos("radius"))
    if kind == "SphericalShell":
        return SphericalShell(p, None, _f3(kw["center"], kind), pos("radius"), pos("shell_width"))
    if kind in ("Polygon", "LinPoly"):
        pts = np.array(kw["points"], float)
        if pts.ndim != 2 or pts.shape[0] != 2 or pts.shape[1] < 3 or not np.all(np.isfinite(pts)):
            raise ValueError(f"{kind}: points must be 2 x N with N >= 3")
        nd = {"x": 0, "y": 1, "z": 2}.get(kw["norm_dir"], kw["norm_dir"])
        if nd not in (0, 1, 2):
            raise ValueError(f"{kind}: norm_dir must be 0..2 or 'x', 'y', 'z'")
        if kind == "Polygon":
            return Polygon(p, None, pts, int(nd), float(kw["elevation"]))
        return LinPoly(p, None, pts, int(nd), float(kw["elevation"]), float(kw["length"]))
    if kind in ("Curve", "Wire"):
        pts = np.array(kw["points"], float)
        if pts.ndim != 2 or pts.shape[0] != 3 or pts.shape[1] < 2 or not np.all(np.isfinite(pts)):
            raise ValueError(f"{kind}: points must be 3 x N with N >= 2")
        return Curve(p, None, pts) if kind == "Curve" else Wire(p, None, pts, pos("radius"))
    if kind.lower() == "polyhedron":
        tri = np.array(kw["triangles"], float)
        if tri.ndim != 3 or tri.shape[0] < 1 or tri.shape[1:] != (3, 3) or not np.all(np.isfinite(tri)):
            raise ValueError("Polyhedron: triangles must be ntri x 3 x 3 finite coordinates with ntri >= 1")
        return Polyhedron(p, None, tri)
    raise ValueError(f"unknown primitive '{kind}'")


def has_new(scene) -> bool:
    """Whether the scene draws anything but boxes, or has a disc material (then every primitive, boxes included, goes through the
    owner arrays)."""
    return (any(isinstance(p, NEW_TYPES) for prop in list(scene.materials) + list(scene.metals) for p in prop.boxes) or
            any(getattr(m, "vmap", None) is not None for m in scene.materials))


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class Table:
    rec: np.ndarray                    # RECORD [nprim], in ownership order
    verts: np.ndarray                  # float64: polygon vertices (u, v pairs), wire points and triangle corners (x, y, z triples), metres
    tol: float
    curves: List[tuple] = field(default_factory=list)     # (metal index, points [N][3] in world metres) of curves and wires
    names: List[str] = field(default_factory=list)        # per record: "<property>: <type>" for messages
    # voxel maps (discmaterial.py): rec_map int32 per record (0: none, m + 1: the record is a delimiter of maps[m]); None: no maps
    rec_map: Optional[np.ndarray] = None
    maps: List["PackedMap"] = field(default_factory=list)


@dataclass
class PackedMap:
    """One voxel map as both rasterisers read it: M the 3 x 4 world (metres) -> map coordinates, the map's lines, its voxels (flat,
    x fastest) and its background flag."""
    M: np.ndarray
    lines: Tuple[np.ndarray, np.ndarray, np.ndarray]
    data: np.ndarray
    use_db_background: bool


def _world_inverse(matrix, u):
    """(3x4 world->local in metres as 12 numbers, 4x4 local->world in metres) or (None, None) for the identity."""
    if matrix is None or np.allclose(matrix, np.eye(4)):
        return None, None
    M = np.array(matrix, dtype=float)
    M[:3, 3] *= u
    return np.linalg.inv(M)[:3, :].reshape(12).copy(), M


def _index_box(coords, lo, hi, pad):
    """Inclusive index box [x0, y0, z0, x1, y1, z1] of the points within [lo - pad, hi + pad] per axis (empty: x0 > x1)."""
    out = np.zeros(6, np.int32)
    for a in range(3):
        c = coords[a]
        out[a] = np.searchsorted(c, lo[a] - pad, "left")
        out[3 + a] = int(np.searchsorted(c, hi[a] + pad, "right")) - 1
    if np.any(out[3:] < out[:3]):
        out[:] = (0, 0, 0, -1, -1, -1)
    return out


def _closed_triangles(tri, what):
    """The triangles [ntri][3][3] (metres) without the zero-area ones; ValueError for an open mesh or one beyond MAX_TRIANGLES."""
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    tri = tri[((nx * nx + ny * ny) + nz * nz) != 0.0]
    if tri.shape[0] > MAX_TRIANGLES:
        raise ValueError(f"{what}: {tri.shape[0]} triangles in one polyhedron, at most {MAX_TRIANGLES} are supported")
    if tri.shape[0] == 0:
        raise ValueError(f"{what}: the polyhedron has no triangle of non-zero area")
    _, vid = np.unique(tri.reshape(-1, 3) + 0.0, axis=0, return_inverse=True)      # weld by exact coordinates (+ 0.0: -0.0 == 0.0)
    vid = vid.reshape(-1, 3)
    ends = np.stack([vid, np.roll(vid, -1, axis=1)], axis=2).reshape(-1, 2)
    ends = ends[ends[:, 0] != ends[:, 1]]
    _, uses = np.unique(np.sort(ends, axis=1), axis=0, return_counts=True)
    nopen = int(np.count_nonzero(uses % 2))
    if nopen:
        raise ValueError(f"{what}: the polyhedron is not closed: {nopen} open edges (edges used by an odd number of triangles); the "
                         f"inside of an open mesh is undefined")
    return tri


def pack_table(scene, grid) -> Table:
    """One flat table for both rasterisers: materials in scene order, then metals, each in drawing order.  Parameters in metres."""
    from .scene import Box, ConductingSheet, _tol
    u = scene.unit
    tol = _tol(grid)
    centers = [grid.centers(a) for a in range(3)]
    recs, verts, curves, names = [], [], [], []
    rec_map, maps = [], []
    nvert = 0
    for role, props in ((ROLE_MATERIAL, scene.materials), (ROLE_METAL, scene.metals)):
        for qi, prop in enumerate(props):
            vmap = getattr(prop, "vmap", None) if role == ROLE_MATERIAL else None
            if vmap is not None:
                if len(maps) == _disc.MAX_MAPS:
                    raise ValueError(f"disc material '{prop.name}': a scene takes at most {_disc.MAX_MAPS} voxel maps")
                maps.append(PackedMap(vmap.world_to_map(u), vmap.lines, np.ascontiguousarray(vmap.data.reshape(-1)),
                                      bool(vmap.use_db_background)))
            for pr in prop.boxes:
                Minv, M = _world_inverse(pr.matrix, u)
                if vmap is not None and isinstance(pr, Polyhedron):
                    raise ValueError(f"disc material '{prop.name}': a polyhedron cannot delimit a voxel map (boxes and the analytic solids can)")
                if isinstance(pr, Polyhedron) and isinstance(prop, ConductingSheet):
                    raise ValueError(f"'{prop.name}': Polyhedron is for materials and plain metals (AddMetal) only")
                if isinstance(pr, Curve):
                    if role != ROLE_METAL or isinstance(prop, ConductingSheet):
                        raise ValueError(f"'{prop.name}': {type(pr).__name__} is for metals (AddMetal) only")
                    pts = np.asarray(pr.points, float).T * u
                    if M is not None:
                        pts = pts @ M[:3, :3].T + M[:3, 3]
                    curves.append((qi, pts))
                    if not isinstance(pr, Wire):
                        continue
                r = np.zeros((), RECORD)
                r["role"], r["prop"], r["priority"], r["order"] = role, qi, int(pr.priority), len(recs)
                par = np.zeros(N_PAR)
                if isinstance(pr, Box):
                    lo, hi = np.minimum(pr.start, pr.stop) * u, np.maximum(pr.start, pr.stop) * u
                    r["type"] = T_BOX
                    par[:3], par[3:6] = lo, hi
                elif isinstance(pr, (Sphere, SphericalShell)):
                    c = np.asarray(pr.center, float) * u
                    shell = isinstance(pr, SphericalShell)
                    r["type"] = T_SPHERICAL_SHELL if shell else T_SPHERE
                    par[:3], par[3] = c, pr.radius * u
                    par[4] = pr.shell_width * u if shell else 0.0
                    ext = par[3] + 0.5 * par[4]
                    lo, hi = c - ext, c + ext
                elif isinstance(pr, (Cylinder, CylindricalShell)):
                    a, b = np.asarray(pr.start, float) * u, np.asarray(pr.stop, float) * u
                    shell = isinstance(pr, CylindricalShell)
                    par[:3], par[3:6], par[6] = a, b, pr.radius * u
                    par[7] = pr.shell_width * u if shell else 0.0
                    ext = par[6] + 0.5 * par[7]
                    if np.array_equal(a, b):
                        if shell:
                            raise ValueError(f"'{prop.name}': a cylindrical shell needs start != stop")
                        r["type"] = T_DISC
                        lo, hi = a - np.array([ext, ext, 0.0]), a + np.array([ext, ext, 0.0])
                    else:
                        r["type"] = T_CYLINDRICAL_SHELL if shell else T_CYLINDER
                        lo, hi = np.minimum(a, b) - ext, np.maximum(a, b) + ext
                elif isinstance(pr, Polygon):
                    n = int(pr.norm_dir)
                    pts = np.asarray(pr.points, float) * u
                    lin = isinstance(pr, LinPoly)
                    e0 = pr.elevation * u
                    e1 = (pr.elevation + pr.length) * u if lin else e0
                    r["type"], r["norm_dir"] = (T_LINPOLY if lin else T_POLYGON), n
                    par[0], par[1] = min(e0, e1), max(e0, e1)
                    r["vert0"], r["nvert"] = nvert, pts.shape[1]
                    verts.append(pts.T.reshape(-1))
                    nvert += 2 * pts.shape[1]
                    lo, hi = np.zeros(3), np.zeros(3)
                    lo[n], hi[n] = par[0], par[1]
                    for q, ax in enumerate(((n + 1) % 3, (n + 2) % 3)):
                        lo[ax], hi[ax] = pts[q].min(), pts[q].max()
                elif isinstance(pr, Wire):
                    pts = np.asarray(pr.points, float) * u
                    r["type"] = T_WIRE
                    par[0] = pr.radius * u
                    r["vert0"], r["nvert"] = nvert, pts.shape[1]
                    verts.append(pts.T.reshape(-1))
                    nvert += 3 * pts.shape[1]
                    lo, hi = pts.min(axis=1) - par[0], pts.max(axis=1) + par[0]
                elif isinstance(pr, Polyhedron):
                    tri = _closed_triangles(np.asarray(pr.triangles, float) * u, f"'{prop.name}'")
                    r["type"] = T_POLYHEDRON
                    r["vert0"], r["nvert"] = nvert, 3 * tri.shape[0]
                    verts.append(tri.reshape(-1))
                    nvert += tri.size
                    lo, hi = tri.reshape(-1, 3).min(axis=0), tri.reshape(-1, 3).max(axis=0)
                else:
                    raise ValueError(f"'{prop.name}': unknown primitive {type(pr).__name__}")
                r["par"] = par
                if Minv is not None:
                    r["has_matrix"] = 1
                    r["m"] = Minv
                    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
                    w = corners @ M[:3, :3].T + M[:3, 3]
                    lo, hi = w.min(axis=0), w.max(axis=0)
                pad = 2.0 * tol + 1e-9 * float(np.max(np.abs(np.concatenate([lo, hi]))))
                r["cbox"] = _index_box(centers, lo, hi, pad)
                r["nbox"] = _index_box(grid.lines, lo, hi, pad)
                recs.append(r)
                rec_map.append(len(maps) if vmap is not None else 0)
                names.append(f"{prop.name}: {type(pr).__name__}")
    rec = np.array(recs, RECORD) if recs else np.zeros(0, RECORD)
    v = np.concatenate(verts) if verts else np.zeros(0)
    return Table(np.ascontiguousarray(rec), np.ascontiguousarray(v, np.float64), float(tol), curves, names,
                 np.array(rec_map, np.int32) if maps else None, maps)


# ---------------------------------------------------------------------------------------------------------------------------
# the inside tests: include/fdtd_hip_voxel.h, statement for statement
# ---------------------------------------------------------------------------------------------------------------------------
def _seg_near(wx, wy, wz, ex, ey, ez, dx, dy, dz, lim2):
    """Point-to-segment distance^2 <= lim2, division-free: w = p - a, e = p - b, d = b - a."""
    L = (dx * dx + dy * dy) + dz * dz
    s = (wx * dx + wy * dy) + wz * dz
    ww = (wx * wx + wy * wy) + wz * wz
    ee = (ex * ex + ey * ey) + ez * ez
    return np.where(s <= 0.0, ww <= lim2, np.where(s >= L, ee <= lim2, ww * L - s * s <= lim2 * L))


def _tri_side(ax, ay, az, bx, by, bz, px, py, pz, nx, ny, nz):
    """((b - a) x (p - a)) . n >= 0: p is on the inner side of the triangle's edge a -> b."""
    dx, dy, dz = bx - ax, by - ay, bz - az
    vx, vy, vz = px - ax, py - ay, pz - az
    cx, cy, cz = dy * vz - dz * vy, dz * vx - dx * vz, dx * vy - dy * vx
    return (cx * nx + cy * ny) + cz * nz >= 0.0


def _tri_cross(Py, Pz, Qy, Qz, y, z):
    """One crossing of the projected edge P -> Q, its end points in canonical order (the smaller z first, then the smaller y)."""
    if Qz < Pz or (Qz == Pz and Qy < Py):
        Py, Pz, Qy, Qz = Qy, Qz, Py, Pz
    du, dv, wu, wv = Qy - Py, Qz - Pz, y - Py, z - Pz
    return ((Pz > z) != (Qz > z)) & (wu * dv < wv * du)


def _tri_into(par, near, x, y, z, t9, tol, g):
    """One triangle of a POLYHEDRON on the points (x, y, z), broadcastable to the bool arrays par and near, which are updated in place:
    par ^= the ray towards +x crosses it, near |= the point is within tol of it; both only inside the triangle's box grown by g."""
    ax, ay, az, bx, by, bz, cx, cy, cz = t9
    tol2 = tol * tol
    inyz = (((y >= min(ay, by, cy) - g) & (y <= max(ay, by, cy) + g)) & ((z >= min(az, bz, cz) - g) & (z <= max(az, bz, cz) + g)))
    if not inyz.any():
        return
    e1x, e1y, e1z, e2x, e2y, e2z = bx - ax, by - ay, bz - az, cx - ax, cy - ay, cz - az
    nx, ny, nz = e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x
    nn = (nx * nx + ny * ny) + nz * nz
    wx, wy, wz = x - ax, y - ay, z - az
    s = (nx * wx + ny * wy) + nz * wz
    if nx != 0.0:
        proj = (_tri_cross(ay, az, by, bz, y, z) != _tri_cross(by, bz, cy, cz, y, z)) != _tri_cross(cy, cz, ay, az, y, z)
        par ^= (proj & inyz) & ((s < 0.0) if nx > 0.0 else (s > 0.0))
    inbox = inyz & ((x >= min(ax, bx, cx) - g) & (x <= max(ax, bx, cx) + g))
    if not inbox.any():
        return
    c = (_tri_side(ax, ay, az, bx, by, bz, x, y, z, nx, ny, nz) & _tri_side(bx, by, bz, cx, cy, cz, x, y, z, nx, ny, nz) &
         _tri_side(cx, cy, cz, ax, ay, az, x, y, z, nx, ny, nz))
    ux, uy, uz, tx, ty, tz = x - bx, y - by, z - bz, x - cx, y - cy, z - cz
    edge = (_seg_near(wx, wy, wz, ux, uy, uz, bx - ax, by - ay, bz - az, tol2) |
            _seg_near(ux, uy, uz, tx, ty, tz, cx - bx, cy - by, cz - bz, tol2) |
            _seg_near(tx, ty, tz, wx, wy, wz, ax - cx, ay - cy, az - cz, tol2))
    near |= inbox & np.where(c, s * s <= tol2 * nn, edge)


def _inside(r, verts, x, y, z, tol):
    """Bool array (broadcast of x, y, z: world coordinates in metres) of the points record `r` holds under its role's rule."""
    metal = int(r["role"]) == ROLE_METAL
    t = tol if metal else -tol
    shape = np.broadcast(x, y, z).shape
    if int(r["has_matrix"]):
        m = [float(v) for v in r["m"]]
        x, y, z = (((m[0] * x + m[1] * y) + m[2] * z) + m[3],
                   ((m[4] * x + m[5] * y) + m[6] * z) + m[7],
                   ((m[8] * x + m[9] * y) + m[10] * z) + m[11])
    p = [float(v) for v in r["par"]]
    ty = int(r["type"])
    never = np.zeros(shape, bool)
    if ty == T_BOX:
        out = ((x >= p[0] - t) & (x <= p[3] + t)) & ((y >= p[1] - t) & (y <= p[4] + t)) & ((z >= p[2] - t) & (z <= p[5] + t))
    elif ty in (T_SPHERE, T_SPHERICAL_SHELL):
        dx, dy, dz = x - p[0], y - p[1], z - p[2]
        d2 = (dx * dx + dy * dy) + dz * dz
        if ty == T_SPHERE:
            re = p[3] + t
            out = (d2 <= re * re) if re >= 0.0 else never
        else:
            ro = (p[3] + 0.5 * p[4]) + t
            ri = (p[3] - 0.5 * p[4]) - t
            out = never if ro < 0.0 else ((d2 <= ro * ro) if ri <= 0.0 else ((d2 <= ro * ro) & (d2 >= ri * ri)))
    elif ty in (T_CYLINDER, T_CYLINDRICAL_SHELL):
        dx, dy, dz = p[3] - p[0], p[4] - p[1], p[5] - p[2]
        L = (dx * dx + dy * dy) + dz * dz
        wx, wy, wz = x - p[0], y - p[1], z - p[2]
        s = (wx * dx + wy * dy) + wz * dz
        ww = (wx * wx + wy * wy) + wz * wz
        q = ww * L - s * s
        tt = (tol * tol) * L
        e = s - L
        if metal:
            ax = ((s >= 0.0) | (s * s <= tt)) & ((e <= 0.0) | (e * e <= tt))
        else:
            ax = ((s >= 0.0) & (s * s >= tt)) & ((e <= 0.0) & (e * e >= tt))
        if ty == T_CYLINDER:
            re = p[6] + t
            out = (ax & (q <= (re * re) * L)) if re >= 0.0 else never
        else:
            ro = (p[6] + 0.5 * p[7]) + t
            ri = (p[6] - 0.5 * p[7]) - t
            rad = never if ro < 0.0 else ((q <= (ro * ro) * L) if ri <= 0.0 else ((q <= (ro * ro) * L) & (q >= (ri * ri) * L)))
            out = ax & rad
    elif ty == T_DISC:
        if not metal:
            out = never
        else:
            dx, dy, dz = x - p[0], y - p[1], z - p[2]
            re = p[6] + t
            out = ((dz <= tol) & (dz >= -tol)) & (dx * dx + dy * dy <= re * re)
    elif ty in (T_POLYGON, T_LINPOLY):
        n = int(r["norm_dir"])
        loc = (x, y, z)
        pn, pu, pv = loc[n], loc[(n + 1) % 3], loc[(n + 2) % 3]
        if ty == T_POLYGON:
            if not metal:
                return never
            dn = pn - p[0]
            nrm = (dn <= tol) & (dn >= -tol)
        else:
            nrm = (pn >= p[0] - t) & (pn <= p[1] + t)
        v0, nv = int(r["vert0"]), int(r["nvert"])
        V = verts[v0:v0 + 2 * nv].reshape(nv, 2)
        tol2 = tol * tol
        par = np.zeros(np.broadcast(pu, pv).shape, bool)
        near = np.zeros_like(par)
        for e in range(nv):
            au, av = float(V[e, 0]), float(V[e, 1])
            bu, bv = float(V[(e + 1) % nv, 0]), float(V[(e + 1) % nv, 1])
            du, dv = bu - au, bv - av
            wu, wv = pu - au, pv - av
            lhs, rhs = wu * dv, wv * du
            straddle = (av > pv) != (bv > pv)
            par ^= straddle & ((lhs < rhs) if dv > 0.0 else (lhs > rhs))
            eu, ev = pu - bu, pv - bv
            L = du * du + dv * dv
            s = wu * du + wv * dv
            ww = wu * wu + wv * wv
            ee = eu * eu + ev * ev
            near |= np.where(s <= 0.0, ww <= tol2, np.where(s >= L, ee <= tol2, ww * L - s * s <= tol2 * L))
        out = nrm & ((par | near) if metal else (par & ~near))
    elif ty == T_WIRE:
        re = p[0] + t
        if not metal or re < 0.0:
            return never
        v0, nv = int(r["vert0"]), int(r["nvert"])
        V = verts[v0:v0 + 3 * nv].reshape(nv, 3)
        re2 = re * re
        out = never.copy()
        for e in range(max(nv - 1, 1)):
            a = [float(v) for v in V[e]]
            b = [float(v) for v in V[min(e + 1, nv - 1)]]
            out = out | _seg_near(x - a[0], y - a[1], z - a[2], x - b[0], y - b[1], z - b[2],
                                  b[0] - a[0], b[1] - a[1], b[2] - a[2], re2)
    elif ty == T_POLYHEDRON:
        v0, nv = int(r["vert0"]), int(r["nvert"])
        T = verts[v0:v0 + 3 * nv].reshape(nv // 3, 9)
        g = 2.0 * tol
        par = np.zeros(shape, bool)
        near = np.zeros(shape, bool)
        # a block of mesh lines (x, y, z each along its own axis): a triangle is evaluated on the rows and planes its gate holds only
        rows = len(shape) == 3 and x.shape == (1, 1, shape[2]) and y.shape == (1, shape[1], 1) and z.shape == (shape[0], 1, 1)
        for tr in range(T.shape[0]):
            t9 = [float(v) for v in T[tr]]
            if not rows:
                _tri_into(par, near, x, y, z, t9, tol, g)
                continue
            js = np.flatnonzero((y.reshape(-1) >= min(t9[1], t9[4], t9[7]) - g) & (y.reshape(-1) <= max(t9[1], t9[4], t9[7]) + g))
            ks = np.flatnonzero((z.reshape(-1) >= min(t9[2], t9[5], t9[8]) - g) & (z.reshape(-1) <= max(t9[2], t9[5], t9[8]) + g))
            if js.size and ks.size:
                sj, sk = slice(js[0], js[-1] + 1), slice(ks[0], ks[-1] + 1)
                _tri_into(par[sk, sj], near[sk, sj], x, y[:, sj], z[sk], t9, tol, g)
        out = (par | near) if metal else (par & ~near)
    else:
        raise ValueError(f"primitive type {ty}")
    return np.broadcast_to(out, shape)


def _block(coords, box):
    """(x, y, z) broadcastable coordinate arrays [z][y][x] of the inclusive index box, and its slices."""
    sl = tuple(slice(int(box[a]), int(box[3 + a]) + 1) for a in (2, 1, 0))
    x = coords[0][sl[2]].reshape(1, 1, -1)
    y = coords[1][sl[1]].reshape(1, -1, 1)
    z = coords[2][sl[0]].reshape(-1, 1, 1)
    return x, y, z, sl


def node_mask(grid, table: Table, q: int, cells: bool = False, role: Optional[int] = None):
    """(mask [z][y][x] over the record's index box, slices) of record q on the nodes (or the cell centres), or None if the box is
    empty.  `role` overrides the record's role (the material rule on a metal: the cells a conductor fills)."""
    r = table.rec[q]
    box = r["cbox"] if cells else r["nbox"]
    if box[3] < box[0]:
        return None
    if role is not None and role != int(r["role"]):
        r = r.copy()
        r["role"] = role
    coords = [grid.centers(a) for a in range(3)] if cells else grid.lines
    x, y, z, sl = _block(coords, box)
    return np.ascontiguousarray(_inside(r, table.verts, x, y, z, table.tol)), sl


def _edges_of(node, c):
    npa = 2 - c
    if node.shape[npa] < 2:
        return None
    a = [slice(None)] * 3; b = [slice(None)] * 3
    a[npa] = slice(0, -1); b[npa] = slice(1, None)
    return node[tuple(a)] & node[tuple(b)]


def rasterise_spec(grid, table: Table, cells: bool = True, edges: bool = True):
    """(cell_owner int32 [nz-1][ny-1][nx-1], edge_owner int32 [3][nz][ny][nx]): the index of the owning record, -1 for none
    (None for a pass that was not asked for).  THE specification.
    A table with voxel maps (table.maps) gives a third result, cell_voxel int32 [nz-1][ny-1][nx-1]: a record that refers to a map
    holds a cell centre iff its primitive holds it AND the map holds it (discmaterial.lookup_spec); cell_voxel is the linear index of
    the centre's voxel where the owning record has a map, -1 elsewhere."""
    nx, ny, nz = grid.shape
    cown = eown = cvox = None
    has_maps = bool(table.maps)
    if cells:
        cown = np.full((nz - 1, ny - 1, nx - 1), -1, np.int32)
        cprio = np.full(cown.shape, np.iinfo(np.int32).min, np.int64)
        if has_maps:
            cvox = np.full(cown.shape, -1, np.int32)
            centers = [grid.centers(a) for a in range(3)]
    if edges:
        eown = np.full((3, nz, ny, nx), -1, np.int32)
        eprio = np.full(eown.shape, np.iinfo(np.int32).min, np.int64)
    for q, r in enumerate(table.rec):
        pr = int(r["priority"])
        if int(r["role"]) == ROLE_MATERIAL:
            if not cells:
                continue
            res = node_mask(grid, table, q, cells=True)
            if res is None:
                continue
            mask, sl = res
            lin = None
            if has_maps and int(table.rec_map[q]):
                mp = table.maps[int(table.rec_map[q]) - 1]
                x, y, z, _ = _block(centers, r["cbox"])
                held, lin = _disc.lookup_spec(mp.M, mp.lines, mp.data, mp.use_db_background, x, y, z)
                mask = mask & held
            win = mask & (cprio[sl] <= pr)
            cprio[sl][win] = pr
            cown[sl][win] = q
            if has_maps:
                cvox[sl][win] = -1 if lin is None else lin[win]
        elif edges:
            res = node_mask(grid, table, q)
            if res is None:
                continue
            node, sl = res
            for c in range(3):
                e = _edges_of(node, c)
                if e is None:
                    continue
                esl = tuple(slice(s_.start, s_.start + e.shape[n]) for n, s_ in enumerate(sl))
                win = e & (eprio[c][esl] <= pr)
                eprio[c][esl][win] = pr
                eown[c][esl][win] = q
    return (cown, eown, cvox) if has_maps else (cown, eown)


def marks_any_edge(grid, table: Table, q: int) -> bool:
    res = node_mask(grid, table, q)
    return res is not None and any((e := _edges_of(res[0], c)) is not None and bool(e.any()) for c in range(3))


# ---------------------------------------------------------------------------------------------------------------------------
# curves
# ---------------------------------------------------------------------------------------------------------------------------
def _nearest_node(grid, p):
    return [int(np.argmin(np.abs(grid.lines[a] - p[a]))) for a in range(3)]


def snap_segment(grid, p0, p1):
    """Grid edges [(comp, i, j, k)] (the edge's lower node) from the node nearest p0 to the node nearest p1: a connected staircase
    of exactly the Manhattan length between them; every step goes to the neighbour closest to the straight segment p0-p1 (ties:
    the lowest axis)."""
    cur, end = _nearest_node(grid, p0), _nearest_node(grid, p1)
    a, d = np.asarray(p0, float), np.asarray(p1, float) - np.asarray(p0, float)
    L = float(d @ d)
    out = []
    while cur != end:
        best = None
        for ax in range(3):
            if cur[ax] == end[ax]:
                continue
            nxt = list(cur)
            nxt[ax] += 1 if end[ax] > cur[ax] else -1
            w = np.array([grid.lines[q][nxt[q]] for q in range(3)]) - a
            s = min(max(float(w @ d), 0.0), L)
            dist = float(w @ w) * L - 2.0 * s * float(w @ d) + s * s if L > 0 else float(w @ w)   # |w - (s/L) d|^2 * L
            if best is None or dist < best[0]:
                best = (dist, ax, nxt)
        _, ax, nxt = best
        lower = list(cur)
        lower[ax] = min(cur[ax], nxt[ax])
        out.append((ax, lower[0], lower[1], lower[2]))
        cur = nxt
    return out


def snap_curve(grid, pts):
    """The edges of a polyline pts [N][3] (metres): snap_segment of every segment, in order."""
    out = []
    for q in range(len(pts) - 1):
        out.extend(snap_segment(grid, pts[q], pts[q + 1]))
    return out
