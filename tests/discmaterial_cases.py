"""Voxel maps, grids and scenes shared by test_discmaterial_cpu.py and test_discmaterial_gpu.py (no tests here).  Scenes use unit = 1
(coordinates are metres) unless they say otherwise."""
import numpy as np
from conftest import pkg
import primitives_cases as pc
import polyhedron_cases as ph


def rotation(axis, deg, shift=(0.0, 0.0, 0.0)):
    """4x4: a rotation by `deg` about the (skew) axis through the origin, then a translation."""
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    t = np.deg2rad(deg)
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)
    M[:3, 3] = shift
    return M


def uneven_lines(n, lo, hi, seed):
    """n strictly increasing, non-uniform lines from lo to hi."""
    w = np.random.default_rng(seed).uniform(0.6, 1.7, n - 1)
    x = np.concatenate([[0.0], np.cumsum(w)])
    return lo + (hi - lo) * x / x[-1]


def random_data(shape_xyz, db_size, zeros, seed):
    """uint8 [nZ][nY][nX] tissue indices 1..db_size-1 with a fraction `zeros` of zeros."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape_xyz
    d = rng.integers(1, max(db_size, 2), (nz, ny, nx)).astype(np.uint8)
    d[rng.random(d.shape) < zeros] = 0
    return d


def table_of(db_size, seed=1):
    """(eps_r, kappa, density) of db_size tissues; entry 0 is a background that differs from air."""
    rng = np.random.default_rng(seed)
    return 1.0 + rng.uniform(0.5, 60.0, db_size), rng.uniform(0.0, 2.0, db_size), rng.uniform(100.0, 2000.0, db_size)


def hand_map_scene(use_db_background=False):
    """The hand-computed case: 6 x 5 x 3 unit cells, a 3 x 2 x 1-voxel map, identity placement, delimited by a box over the whole
    grid.  The cell centre x = 2.5 lies on the interior map line (upper voxel), x = 5.5 on the last line (no voxel)."""
    grid = ph.grid_of(np.arange(7.0), np.arange(6.0), np.arange(4.0))
    s = pkg("scene").Scene(unit=1.0)
    data = np.array([[[1, 0, 2], [2, 1, 0]]], np.uint8)
    dm = s.add_disc_material("phantom", ([1.0, 2.5, 4.0, 5.5], [1.0, 2.0, 4.0], [1.0, 2.0]), data, [1.5, 30.0, 50.0], [0.01, 0.5, 1.5],
                             [5.0, 1000.0, 1100.0], use_db_background=use_db_background)
    dm.add_box((0.0, 0.0, 0.0), (6.0, 5.0, 3.0))
    return grid, s


# what hand_map_scene gives on the plane k = 1 (rows j = 0..4, columns i = 0..5); every other plane is unowned
HAND_OWNER = np.array([[-1, -1, -1, -1, -1, -1],
                       [-1, 0, -1, -1, 0, -1],
                       [-1, 0, 0, 0, -1, -1],
                       [-1, 0, 0, 0, -1, -1],
                       [-1, -1, -1, -1, -1, -1]], np.int32)
HAND_VOXEL = np.array([[-1, -1, -1, -1, -1, -1],
                       [-1, 0, -1, -1, 2, -1],
                       [-1, 3, 4, 4, -1, -1],
                       [-1, 3, 4, 4, -1, -1],
                       [-1, -1, -1, -1, -1, -1]], np.int32)
HAND_VOXEL_BG = np.array([[-1, -1, -1, -1, -1, -1],             # use_db_background: the zeros are owned too
                          [-1, 0, 1, 1, 2, -1],
                          [-1, 3, 4, 4, 5, -1],
                          [-1, 3, 4, 4, 5, -1],
                          [-1, -1, -1, -1, -1, -1]], np.int32)


RAGGED = dict(nx=132, ny=12, nz=7, ext=(131.0, 11.0, 6.0))      # 131 x 11 x 6 cells: a second, partial x tile (128) and y tile (8)


def crowded_scene(use_db_background=False, outside=False, with_disc=True):
    """Case (a): on the ragged graded mesh a 16 x 15 x 14-voxel map on non-uniform lines, rotated about a skew axis, scaled and
    shifted, about 35 % zeros; a higher-priority sphere inside it, equal-priority boxes drawn before and after it, and a closed STL
    tetrahedron of lower priority that shows through the zeros.  outside=True shifts the map away from the grid (case (e));
    with_disc=False leaves the disc material (records 3 and 4 of 0..5) out."""
    grid = ph.graded_grid(**RAGGED)
    s = pkg("scene").Scene(unit=1.0)
    tet = ph.tetra_tris([[3.0, 0.4, 0.3], [120.0, 1.1, 0.6], [60.0, 10.4, 1.0], [58.0, 5.2, 5.7]])
    s.add_material("tetra", 2.2, 0.0, density=50.0).add_polyhedron(tet, priority=0)
    s.add_material("before", 3.3, 0.1, density=60.0).add_box((20.3, 2.2, 1.1), (49.7, 8.3, 4.6), priority=2)
    s.add_material("ball", 4.4, 0.2, density=70.0).add_sphere((66.1, 5.4, 3.1), 2.7, priority=5)
    if with_disc:
        lines = (uneven_lines(17, -8.0, 9.1, 11), uneven_lines(16, -1.0, 1.1, 12), uneven_lines(15, -0.6, 0.5, 13))
        place = rotation((0.3, -0.2, 0.93), 9.0, (1.0e4, 5.0e3, -2.0e3) if outside else (64.2, 5.6, 2.9))
        dm = s.add_disc_material("phantom", lines, random_data((16, 15, 14), 9, 0.35, 14), *table_of(9), scale=7.3, matrix=place,
                                 use_db_background=use_db_background)
        dm.add_box((1.3, 0.2, 0.1), (130.8, 10.7, 5.8), priority=2)
        dm.boxes.append(pkg("scene").Box((-50.0, -4.1, -2.2), (51.0, 4.3, 2.4), 2, pc.rot(2, 4.0, (70.0, 5.0, 3.0))))    # + a transformed box
    s.add_material("after", 5.5, 0.3, density=80.0).add_box((75.2, 1.3, 0.7), (101.4, 9.6, 5.2), priority=2)   # equal priority, drawn after
    return grid, s


def two_maps_scene():
    """Case (c): two overlapping maps of different priority on the ragged mesh, the upper one transparent in places (half zeros),
    the lower one with its database background."""
    grid = ph.graded_grid(**RAGGED)
    s = pkg("scene").Scene(unit=1.0)
    s.add_material("slab", 2.0, 0.0).add_box((0.5, 0.5, 0.5), (130.0, 10.0, 2.9), priority=0)
    lo = s.add_disc_material("lower", (uneven_lines(12, 10.0, 90.0, 21), uneven_lines(7, 0.7, 10.2, 22), uneven_lines(5, 0.4, 5.5, 23)),
                             random_data((11, 6, 4), 5, 0.3, 24), *table_of(5, 2), use_db_background=True)
    lo.add_box((5.0, 0.1, 0.1), (125.0, 10.9, 5.9), priority=1)
    up = s.add_disc_material("upper", (uneven_lines(20, -30.0, 30.0, 25), uneven_lines(9, -4.0, 4.0, 26), uneven_lines(6, -2.0, 2.0, 27)),
                             random_data((19, 8, 5), 7, 0.5, 28), *table_of(7, 3), matrix=rotation((0.0, 0.2, 1.0), -6.0, (70.0, 5.5, 3.0)))
    up.add_sphere((72.0, 5.5, 3.0), 24.0, priority=3)
    return grid, s


def on_lines_scene():
    """Case (d): unit cells; one map whose lines ARE the cell centres of the grid (every centre on a line: it belongs to the upper voxel, the
    centre on the last line to none), and a second map, drawn elsewhere, whose last x line is a cell centre."""
    grid = ph.grid_of(np.arange(14.0), np.arange(11.0), np.arange(8.0))
    s = pkg("scene").Scene(unit=1.0)
    a = s.add_disc_material("centres", (np.arange(5) + 1.5, np.arange(6) + 2.5, np.arange(4) + 1.5), random_data((4, 5, 3), 4, 0.2, 31), *table_of(4))
    a.add_box((0.0, 0.0, 0.0), (7.0, 10.0, 7.0))
    b = s.add_disc_material("last", ([7.2, 8.9, 10.1, 11.5], [0.3, 4.4, 9.6], [0.2, 3.3, 6.9]), random_data((3, 2, 2), 3, 0.0, 32), *table_of(3))
    b.add_box((7.0, 0.0, 0.0), (13.0, 10.0, 7.0))
    return grid, s


def extremes_scene():
    """Case (f): a one-voxel map, and a map that holds index 255 with a table of 256 entries."""
    grid = ph.graded_grid(19, 17, 15)
    s = pkg("scene").Scene(unit=1.0)
    one = s.add_disc_material("one", ([2.2, 9.7], [1.4, 8.8], [3.1, 11.6]), np.array([[[1]]], np.uint8), [1.0, 7.0], [0.0, 0.3], [0.0, 900.0])
    one.add_box((0.0, 0.0, 0.0), (18.0, 16.0, 14.0))
    d = (np.arange(6 * 5 * 4) * 37 % 256).astype(np.uint8).reshape(4, 5, 6)
    d[1, 2, 3] = 255
    big = s.add_disc_material("full", (uneven_lines(7, 8.0, 17.5, 41), uneven_lines(6, 5.0, 15.5, 42), uneven_lines(5, 1.0, 13.0, 43)), d, *table_of(256))
    big.add_cylinder((12.0, 10.0, 0.5), (12.5, 10.5, 13.5), 5.1, priority=1)
    return grid, s


# ---- phantom equals primitives ----------------------------------------------------------------------------------------------------
PH_N, PH_U = (24, 20, 16), 2.0                                       # nodes and cell size [mm] of test_sar_model_cpu's block scene
PH_SPHERES = (("skin", 12.0, 0.4, 1100.0, 10.3, 1), ("bone", 6.5, 0.1, 1900.0, 7.1, 2), ("brain", 45.0, 1.3, 1040.0, 4.2, 3))
PH_CENTER = (25.1, 19.3, 18.4)
PH_BOX = ((12.0, 6.0, 6.0), (38.0, 32.0, 30.0))                      # mm, on mesh lines: the spheres' bounding box


def phantom_grid():
    return pkg("grid").RectGrid(*[(np.arange(k) * PH_U) * 1e-3 for k in PH_N])


def phantom_primitive_scene():
    """Three nested tissue spheres over a plate that a z port feeds from the floor, drawn with the existing primitives."""
    s = pkg("scene").Scene(unit=1e-3)
    for name, eps, kap, rho, r, prio in PH_SPHERES:
        s.add_material(name, eps, kap, density=rho).add_sphere(PH_CENTER, r, priority=prio)
    _phantom_feed(s)
    return s


def _phantom_feed(s):
    s.add_metal("plate").add_box((4.0, 8.0, 6.0), (40.0, 30.0, 6.0))
    s.add_lumped_port(1, 50.0, (8.0, 20.0, 0.0), (8.0, 20.0, 6.0), "z", 1.0)


def phantom_map_arrays(vox):
    """(lines [mm], data, eps_r, kappa, density) of the map that repeats the primitive scene `vox` over PH_BOX: the grid's own lines,
    data = cell_material + 1 (0 where air)."""
    lo = [int(round(PH_BOX[0][a] / PH_U)) for a in range(3)]
    hi = [int(round(PH_BOX[1][a] / PH_U)) for a in range(3)]
    lines = tuple(np.arange(lo[a], hi[a] + 1) * PH_U for a in range(3))
    data = (vox.cell_material[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] + 1).astype(np.uint8)
    assert int((vox.cell_material >= 0).sum()) == int((data > 0).sum())          # the box holds every tissue cell
    return (lines, data, [1.0] + [t[1] for t in PH_SPHERES], [0.0] + [t[2] for t in PH_SPHERES], [0.0] + [t[3] for t in PH_SPHERES])


def phantom_disc_scene(vox):
    s = pkg("scene").Scene(unit=1e-3)
    s.add_disc_material("phantom", *phantom_map_arrays(vox)).add_box(*PH_BOX)
    _phantom_feed(s)
    return s


def phantom_script(oe, lib, disc, nr_ts=300, device=0):
    """The phantom through the openEMS API: spheres (disc=False) or AddDiscMaterial (disc=True), a 1 g SAR dump over the box."""
    fd = oe.openEMS(NrTS=nr_ts, EndCriteria=0, lib=lib, device=device, nf2ff_mode="record")
    fd.SetGaussExcite(2e9, 1e9)
    fd.SetBoundaryCond(["PEC"] * 6)
    csx = oe.ContinuousStructure()
    fd.SetCSX(csx)
    g = csx.GetGrid()
    g.SetDeltaUnit(1e-3)
    for a, k in zip("xyz", PH_N):
        g.AddLine(a, np.arange(k) * PH_U)
    if disc:
        vox = pkg("scene").voxelize(phantom_primitive_scene(), phantom_grid())
        lines, data, eps, kap, rho = phantom_map_arrays(vox)
        csx.AddDiscMaterial("phantom", mesh_x=lines[0], mesh_y=lines[1], mesh_z=lines[2], DiscData=data, epsR=eps, kappa=kap,
                            density=rho).AddBox(list(PH_BOX[0]), list(PH_BOX[1]))
    else:
        for name, eps, kap, rho, r, prio in PH_SPHERES:
            csx.AddMaterial(name, epsilon=eps, kappa=kap, density=rho).AddSphere(list(PH_CENTER), r, priority=prio)
    csx.AddMetal("plate").AddBox([4.0, 8.0, 6.0], [40.0, 30.0, 6.0])
    port = fd.AddLumpedPort(1, 50, [8.0, 20.0, 0.0], [8.0, 20.0, 6.0], "z", 1.0)
    csx.AddDump("sar", dump_type=21, frequency=[2e9]).AddBox([10.0, 4.0, 4.0], [40.0, 34.0, 30.0])
    return fd, port
