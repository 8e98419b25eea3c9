"""Triangle meshes, grids and scenes shared by test_polyhedron_cpu.py and test_polyhedron_gpu.py (no tests here).  Every mesh is built
here; STL files are written into a test's tmp_path (none is committed).  Scenes use unit = 1: coordinates are metres."""
import numpy as np
from conftest import pkg
import primitives_cases as pc

_QUADS = ((0, 2, 6, 4), (1, 5, 7, 3), (0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6))    # corner index = 4 ix + 2 iy + iz


def box_tris(lo, hi):
    """The 12 triangles of the box [lo, hi]."""
    c = np.array([[(lo[0], hi[0])[i], (lo[1], hi[1])[j], (lo[2], hi[2])[k]] for i in (0, 1) for j in (0, 1) for k in (0, 1)], float)
    return np.array([[c[q[0]], c[q[a]], c[q[a + 1]]] for q in _QUADS for a in (1, 2)])


def octahedron_tris(c, r):
    """The 8 triangles of |x - cx| + |y - cy| + |z - cz| <= r."""
    c = np.asarray(c, float)
    ex, ey, ez = np.eye(3) * r
    return np.array([[c + sx * ex, c + sy * ey, c + sz * ez] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])


def l_prism_tris(x, y, z):
    """The L-shaped prism ([x0, x2] x [y0, y1]  union  [x0, x1] x [y0, y2]) x [z0, z1]; x, y: three values, z: two.  Concave."""
    P = [(x[0], y[0]), (x[2], y[0]), (x[2], y[1]), (x[1], y[1]), (x[1], y[2]), (x[0], y[2])]
    fan = [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5)]            # vertex 0 sees the whole L
    tris = []
    for zz in z:
        tris += [[P[a] + (zz,), P[b] + (zz,), P[c] + (zz,)] for a, b, c in fan]
    for a in range(6):
        b = (a + 1) % 6
        A0, B0, A1, B1 = P[a] + (z[0],), P[b] + (z[0],), P[a] + (z[1],), P[b] + (z[1],)
        tris += [[A0, B0, B1], [A0, B1, A1]]
    return np.array(tris, float)


def u_prism_tris(x, y, z):
    """A U-shaped prism open towards +y: x four values, y three (floor y0..y1, arms up to y2), z two.  A ray along +x through the arms
    crosses the surface four times."""
    P = [(x[0], y[0]), (x[3], y[0]), (x[3], y[2]), (x[2], y[2]), (x[2], y[1]), (x[1], y[1]), (x[1], y[2]), (x[0], y[2])]
    fan = [(0, 1, 4), (1, 2, 4), (2, 3, 4), (0, 4, 5), (0, 5, 7), (5, 6, 7)]
    tris = []
    for zz in z:
        tris += [[P[a] + (zz,), P[b] + (zz,), P[c] + (zz,)] for a, b, c in fan]
    for a in range(8):
        b = (a + 1) % 8
        A0, B0, A1, B1 = P[a] + (z[0],), P[b] + (z[0],), P[a] + (z[1],), P[b] + (z[1],)
        tris += [[A0, B0, B1], [A0, B1, A1]]
    return np.array(tris, float)


def tetra_tris(v):
    v = np.asarray(v, float)
    return np.array([[v[0], v[1], v[2]], [v[0], v[1], v[3]], [v[0], v[2], v[3]], [v[1], v[2], v[3]]])


def tetra_closed_form(v, x, y, z, margin):
    """(inside, excluded): the four-orientation test of the tetrahedron v on the points, and the points within `margin` of one of its
    face planes (where the closed form and the rule may legitimately differ)."""
    v = np.asarray(v, float)
    p = np.stack(np.broadcast_arrays(x, y, z), -1)
    inside = np.ones(p.shape[:-1], bool)
    excluded = np.zeros(p.shape[:-1], bool)
    for f in range(4):
        a, b, c = (v[q] for q in range(4) if q != f)
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n)
        if (v[f] - a) @ n < 0:
            n = -n
        d = (p - a) @ n
        inside &= d > 0
        excluded |= np.abs(d) <= margin
    return inside, excluded


def icosphere_tris(c, r, subdiv):
    """An icosahedron subdivided `subdiv` times, its vertices on the sphere (c, r): 20 * 4^subdiv triangles."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(q, float) / np.linalg.norm(q) for q in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                w = v[a] + v[b]
                v.append(w / np.linalg.norm(w))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c3 in f:
            ab, bc, ca = m(a, b), m(b, c3), m(c3, a)
            nf += [(a, ab, ca), (b, bc, ab), (c3, ca, bc), (ab, bc, ca)]
        f = nf
    V = np.asarray(c, float) + r * np.array(v)
    return V[np.array(f)]


def shuffled_reversed(tris, seed=3):
    """The same solid: triangles in another order, every winding reversed."""
    t = np.asarray(tris)[np.random.default_rng(seed).permutation(len(tris))]
    return np.ascontiguousarray(t[:, ::-1, :])


def grid_of(lines_x, lines_y, lines_z):
    return pkg("grid").RectGrid(np.asarray(lines_x, float), np.asarray(lines_y, float), np.asarray(lines_z, float))


def graded_grid(nx=19, ny=17, nz=15, ext=(18.0, 16.0, 14.0)):
    """A graded mesh over [0, ext] (metres)."""
    return grid_of(*[pc.graded(n, 0.0, L) for n, L in zip((nx, ny, nz), ext)])


def uniform_grid(nx=19, ny=17, nz=15):
    """Unit cells, the origin on the middle node."""
    return grid_of(*[np.arange(n) - float(n // 2) for n in (nx, ny, nz)])


def scene_of(*solids):
    """A scene (unit 1) of (role, name, priority, what, matrix): role "material" / "metal"; what: triangles [n][3][3], or
    ("box", lo, hi)."""
    sc = pkg("scene")
    s = sc.Scene(unit=1.0)
    for q, (role, name, priority, what, matrix) in enumerate(solids):
        prop = s.add_material(name, 2.0 + q) if role == "material" else s.add_metal(name)
        if isinstance(what, tuple) and what[0] == "box":
            prop.add_box(what[1], what[2], priority=priority)
        else:
            prop.add_polyhedron(what, priority=priority)
        if matrix is not None:
            prop.boxes[-1].matrix = np.array(matrix, float)
    return s


def points(grid, cells):
    """Broadcastable (x, y, z) of the cell centres or the nodes, [z][y][x]."""
    P = pkg("primitives")
    c = [grid.centers(a) for a in range(3)] if cells else grid.lines
    n = [len(q) for q in c]
    return P._block(c, (0, 0, 0, n[0] - 1, n[1] - 1, n[2] - 1))[:3]


def held(grid, scene, q=0):
    """Bool [z][y][x] over the whole grid: the cell centres (a material record) or the nodes (a metal record) record q holds."""
    P = pkg("primitives")
    table = P.pack_table(scene, grid)
    cells = int(table.rec[q]["role"]) == P.ROLE_MATERIAL
    n = [len(c) - (1 if cells else 0) for c in grid.lines]
    out = np.zeros((n[2], n[1], n[0]), bool)
    res = P.node_mask(grid, table, q, cells=cells)
    if res is not None:
        out[res[1]] = res[0]
    return out


def tetra_cloud(grid, n=40, seed=11):
    """n tetrahedra inside the grid: the even ones with every vertex on the half-cell lattice (nodes and cell centres, so that rays run
    through vertices, along edges and in faces), the odd ones on random coordinates."""
    rng = np.random.default_rng(seed)
    half = [np.sort(np.concatenate([l, 0.5 * (l[1:] + l[:-1])])) for l in grid.lines]
    out = []
    while len(out) < n:
        if len(out) % 2 == 0:
            v = np.array([[h[rng.integers(2, len(h) - 2)] for h in half] for _ in range(4)])
        else:
            v = np.array([[rng.uniform(l[1], l[-2]) for l in grid.lines] for _ in range(4)])
        if abs(np.linalg.det(v[1:] - v[0])) > 0.0025 * np.prod([l[-1] - l[0] for l in grid.lines]):     # no slivers
            out.append(v)
    return out


def disjoint_tetrahedra(npairs, lo=(0.3, 0.3, 0.3), pitch=1.37, per_row=7):
    """npairs pairs of triangles: npairs / 2 closed tetrahedra (four triangles each) in disjoint cells of a lattice; npairs even."""
    assert npairs % 2 == 0
    tris = []
    for q in range(npairs // 2):
        o = np.array(lo) + pitch * np.array([q % per_row, (q // per_row) % per_row, q // (per_row * per_row)])
        tris.append(tetra_tris(o + np.array([[0.0, 0.0, 0.0], [1.13, 0.07, 0.1], [0.21, 1.09, 0.05], [0.3, 0.27, 1.17]])))
    return np.concatenate(tris)


def stl_patch_script(oe, tmp_path, lib=None, device=0, stl=True, nr_ts=60, binary=True):
    """A tutorial-sized patch through the openEMS API: ground slab, substrate, patch plate, lumped port; 24 x 24 x 16 cells of 1 mm,
    CPML 4.  stl=True draws the substrate and the ground slab as STL boxes (AddPolyhedronReader), else as AddBox."""
    S = pkg("stl")
    FDTD = oe.openEMS(NrTS=nr_ts, EndCriteria=0, lib=lib, device=device, cpml_cells=4)
    FDTD.SetGaussExcite(6e9, 3e9)
    FDTD.SetBoundaryCond(["PML_4"] * 6)
    CSX = oe.ContinuousStructure()
    FDTD.SetCSX(CSX)
    mesh = CSX.GetGrid()
    mesh.SetDeltaUnit(1e-3)
    mesh.AddLine("x", np.arange(25) - 12.0)
    mesh.AddLine("y", np.arange(25) - 12.0)
    mesh.AddLine("z", np.arange(17) - 6.0)
    gnd, sub = CSX.AddMetal("gnd"), CSX.AddMaterial("substrate", epsilon=3.38, kappa=1e-3)
    solids = ((gnd, "gnd", [-8, -8, -1], [8, 8, 0], 10), (sub, "substrate", [-7, -7, 0], [7, 7, 3], 1))
    readers = []
    for prop, name, lo, hi, prio in solids:
        if stl:
            path = tmp_path / f"{name}.stl"
            S.write_stl(path, box_tris(lo, hi), binary=binary)
            r = prop.AddPolyhedronReader(str(path), priority=prio)
            assert r.ReadFile() is True
            readers.append(r)
        else:
            prop.AddBox(lo, hi, priority=prio)
    CSX.AddMetal("patch").AddBox([-5, -4, 3], [5, 4, 3], priority=10)
    port = FDTD.AddLumpedPort(1, 50, [2, 0, 0], [2, 0, 3], "z", 1.0, priority=5)
    return FDTD, port, readers
