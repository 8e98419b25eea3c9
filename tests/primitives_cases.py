"""Scenes and meshes shared by test_primitives_cpu.py and test_primitives_gpu.py (no tests here).  Radii and offsets are non-round
decimals, so that no point sits within rounding of a surface by accident; the few that sit ON a surface do so on purpose."""
import json
import os

import numpy as np
from conftest import ROOT, pkg

UNIT = 1e-3


def golden_scene_cases():
    """name -> prepare call for every scene of tests/golden/scene_calls.json (the plugin's scenes, rotated boxes included)."""
    s = pkg("solver_fdtd_hip")
    FD, PI = s.FeedDirection, s.PatchInstance
    par = lambda f=2.45e9, **kw: pkg("params").PatchAntennaParams.from_user_units(frequency_ghz=f / 1e9, er=4.3, h_mm=1.6, loss_tangent=0.02, **kw)
    pitch = 0.0612
    arr = [PI(name=f"P{n}", params=par(), center_x_m=(ix - 0.5) * pitch, center_y_m=(iy - 0.5) * pitch, center_z_m=0.0,
              feed_direction=FD.NEG_X) for n, (ix, iy) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)])]
    rot = [PI(name="R1", params=par(), center_x_m=0.0, center_y_m=0.0, center_z_m=0.01, feed_direction=FD.NEG_Y, rot_z_deg=90.0),
           PI(name="R2", params=par(), center_x_m=0.08, center_y_m=0.0, center_z_m=0.0, feed_direction=FD.POS_X, rot_x_deg=90.0)]
    return {
        "fixed_2g45": lambda: s.prepare_hip_patch_fixed(par()),
        "fixed_explicit_LW": lambda: s.prepare_hip_patch_fixed(par(L_mm=28.0, W_mm=36.0)),
        "microstrip_negx": lambda: s.prepare_hip_microstrip_patch(par(), feed_direction=FD.NEG_X, boundary="MUR", theta_step_deg=2.0),
        "microstrip_posy": lambda: s.prepare_hip_microstrip_patch(par(), feed_direction=FD.POS_Y, boundary="MUR", theta_step_deg=2.0),
        "microstrip3d_5g8_pml_q3": lambda: s.prepare_hip_microstrip_patch_3d(par(5.8e9), feed_direction=FD.NEG_X, boundary="PML_8",
                                                                           theta_step_deg=2.0, phi_step_deg=5.0, mesh_quality=3),
        "microstrip3d_2g45_mur_q5_posx": lambda: s.prepare_hip_microstrip_patch_3d(par(), feed_direction=FD.POS_X, boundary="MUR",
                                                                                 theta_step_deg=5.0, phi_step_deg=10.0, mesh_quality=5),
        "multi_2x2": lambda: s.prepare_hip_microstrip_multi_3d(arr, boundary="PML_8", theta_step_deg=2.0, phi_step_deg=5.0, mesh_quality=3),
        "multi_rotated": lambda: s.prepare_hip_microstrip_multi_3d(rot, boundary="MUR", theta_step_deg=4.0, phi_step_deg=10.0, mesh_quality=6,
                                                                   nf_center_mode="centroid", end_criteria_db=-40.0),
        "multi_manual_box": lambda: s.prepare_hip_microstrip_multi_3d(arr[:1], boundary="MUR", simbox_mode="manual",
                                                                      manual_size_mm=(260.0, 240.0, 200.0), mesh_quality=2),
        "legacy_2g45": lambda: s.prepare_hip_patch(par()),
    }


def golden_scenes():
    """The recorded call sequences of tests/golden/scene_calls.json, by scene name."""
    with open(os.path.join(ROOT, "tests", "golden", "scene_calls.json")) as fh:
        return json.load(fh)


def graded(n, lo, hi, ratio=1.9):
    """n strictly increasing lines from lo to hi, cells growing geometrically from the middle outwards."""
    h = (n - 1) / 2.0
    w = ratio ** (np.abs(np.arange(n - 1) + 0.5 - h) / max(h, 1.0))
    x = np.concatenate([[0.0], np.cumsum(w)])
    return lo + (hi - lo) * x / x[-1]


def grid_of(nx, ny, nz, ext=(36.0, 28.0, 22.0), grade=True):
    """RectGrid of nx x ny x nz nodes over [0, ext] in drawing units (metres inside)."""
    g = pkg("grid")
    mk = (lambda n, L: graded(n, 0.0, L)) if grade else (lambda n, L: np.linspace(0.0, L, n))
    return g.RectGrid(*[mk(n, L) * UNIT for n, L in zip((nx, ny, nz), ext)])


def rot(axis, deg, shift=(0.0, 0.0, 0.0)):
    """4x4 local->world: a rotation about `axis` followed by a translation (drawing units)."""
    M = np.eye(4)
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    a1, a2 = (axis + 1) % 3, (axis + 2) % 3
    M[a1, a1] = c; M[a1, a2] = -s; M[a2, a1] = s; M[a2, a2] = c
    M[:3, 3] = shift
    return M


def all_types_scene(grid, ext, m=None):
    """About twenty primitives of every type over a mesh spanning [0, ext]: tilted and translated ones, overlaps with priority ties
    across types, one primitive that sticks out of the grid, one wholly outside it, one thin pin that misses every node."""
    sc = pkg("scene")
    Lx, Ly, Lz = ext
    m = min(ext) if m is None else m                              # the scale of the radii
    zl = {q: float(grid.z[int(f * (len(grid.z) - 1))]) / UNIT for q, f in ((2, 0.1), (5, 0.25), (7, 0.35))}   # elevations ON mesh planes
    s = sc.Scene(unit=UNIT)
    sub = s.add_material("substrate", 4.3, 0.012)
    sub.add_box((0.0713 * Lx, 0.0871 * Ly, 0.1013 * Lz), (0.9137 * Lx, 0.8891 * Ly, 0.3217 * Lz), priority=1)
    lens = s.add_material("lens", 2.2)
    lens.add_sphere((0.4127 * Lx, 0.5213 * Ly, 0.6139 * Lz), 0.2317 * m, priority=2)
    dome = s.add_debye_material("radome", 3.1, 0.0, [1.2], [8e-12])
    dome.add_spherical_shell((0.4127 * Lx, 0.5213 * Ly, 0.5139 * Lz), 0.3713 * m, 0.1129 * m, priority=2)     # ties with the lens: later wins
    rod = s.add_material("rod", 9.8, mu_r=1.5)
    rod.add_cylinder((0.1531 * Lx, 0.2217 * Ly, 0.1719 * Lz), (0.8213 * Lx, 0.6911 * Ly, 0.8137 * Lz), 0.0917 * m, priority=2)   # tilted axis
    rod.add_cylinder((0.1 * Lx, 0.1 * Ly, 0.0), (0.1 * Lx, 0.1 * Ly, 0.0), 0.2 * m, priority=9)    # a disc holds no cell
    tube = s.add_material("tube", 5.1, 0.02)
    tube.add_cylindrical_shell((0.7113 * Lx, 0.1391 * Ly, 0.0517 * Lz), (0.7313 * Lx, 0.8731 * Ly, 0.1871 * Lz), 0.1531 * m, 0.0871 * m, priority=3)
    prism = s.add_material("prism", 6.3)
    prism.add_lin_poly([[0.1117 * Lx, 0.5713 * Lx, 0.4219 * Lx, 0.2931 * Lx, 0.0913 * Lx],
                        [0.1319 * Ly, 0.2117 * Ly, 0.8317 * Ly, 0.4419 * Ly, 0.7713 * Ly]], 2, 0.4113 * Lz, 0.3317 * Lz, priority=3)  # concave
    prism.add_box((-0.2113 * Lx, -0.1171 * Ly, -0.0613 * Lz), (0.2713 * Lx, 0.1931 * Ly, 0.1217 * Lz), priority=3)
    prism.boxes[-1].matrix = rot(2, 31.7, (0.5213 * Lx, 0.4117 * Ly, 0.7813 * Lz))                    # rotated and translated box
    prism.add_cylinder((0.0, 0.0, -0.1713 * Lz), (0.0, 0.0, 0.1913 * Lz), 0.1213 * m, priority=4)
    prism.boxes[-1].matrix = rot(0, 57.3, (0.6713 * Lx, 0.6117 * Ly, 0.4813 * Lz))                    # transformed cylinder
    prism.add_sphere((1.0213 * Lx, 0.5117 * Ly, 0.5213 * Lz), 0.1713 * m, priority=1)               # sticks out of the grid
    prism.add_sphere((2.5 * Lx, 0.5 * Ly, 0.5 * Lz), 0.1 * m, priority=5)                           # wholly outside
    gnd = s.add_metal("ground")
    gnd.add_box((0.0513 * Lx, 0.0617 * Ly, zl[2]), (0.9413 * Lx, 0.9217 * Ly, zl[2]), priority=10)
    patch = s.add_metal("patch")
    patch.add_polygon([[0.2117 * Lx, 0.6913 * Lx, 0.7713 * Lx, 0.4517 * Lx, 0.1913 * Lx],
                       [0.2213 * Ly, 0.1817 * Ly, 0.6913 * Ly, 0.8117 * Ly, 0.6313 * Ly]], 2, zl[5], priority=10)
    patch.add_cylinder((0.6117 * Lx, 0.4213 * Ly, zl[7]), (0.6117 * Lx, 0.4213 * Ly, zl[7]), 0.2713 * m, priority=10)   # a disc
    pin = s.add_metal("pin")
    pin.add_cylinder((0.4313 * Lx, 0.4717 * Ly, zl[2]), (0.4313 * Lx, 0.4717 * Ly, zl[7]), 0.1117 * m, priority=10)
    pin.add_cylinder((0.2513 * Lx, 0.7717 * Ly, 0.0913 * Lz), (0.7713 * Lx, 0.3117 * Ly, 0.9013 * Lz), 0.0913 * m, priority=11)  # tilted
    shell = s.add_metal("shells")
    shell.add_spherical_shell((0.5713 * Lx, 0.4913 * Ly, 0.5517 * Lz), 0.3917 * m, 0.1013 * m, priority=10)
    shell.add_cylindrical_shell((0.3113 * Lx, 0.5213 * Ly, 0.0713 * Lz), (0.3313 * Lx, 0.5013 * Ly, 0.9217 * Lz), 0.2113 * m, 0.0817 * m, priority=10)
    shell.add_lin_poly([[0.5117 * Ly, 0.9113 * Ly, 0.7213 * Ly], [0.1213 * Lz, 0.2117 * Lz, 0.8713 * Lz]], 0, 0.7713 * Lx, 0.1613 * Lx, priority=12)
    shell.add_polygon([[-0.3113 * m, 0.3517 * m, 0.0213 * m], [-0.2713 * m, -0.2117 * m, 0.4113 * m]], 1, 0.0, priority=12)
    shell.boxes[-1].matrix = rot(1, 0.0, (0.5 * Lx, grid.y[len(grid.y) // 2] / UNIT, 0.5 * Lz))        # translated onto a mesh plane
    wires = s.add_metal("wires")
    t = np.linspace(0.0, 4.0 * np.pi, 25)
    wires.add_wire([0.5 * Lx + 0.2213 * m * np.cos(t), 0.5 * Ly + 0.2213 * m * np.sin(t), 0.1 * Lz + 0.0613 * Lz * t], 0.0713 * m, priority=10)
    wires.add_curve([[0.0913 * Lx, 0.8713 * Lx, 0.8713 * Lx], [0.9113 * Ly, 0.9113 * Ly, 0.1213 * Ly], [0.8913 * Lz, 0.8913 * Lz, 0.6113 * Lz]])
    thin = s.add_metal("thin_pin")
    i, j = len(grid.x) // 2, len(grid.y) // 2
    thin.add_cylinder((0.5 * (grid.x[i] + grid.x[i + 1]) / UNIT, 0.5 * (grid.y[j] + grid.y[j + 1]) / UNIT, 0.1 * Lz),
                      (0.5 * (grid.x[i] + grid.x[i + 1]) / UNIT, 0.5 * (grid.y[j] + grid.y[j + 1]) / UNIT, 0.9 * Lz),
                      0.2 * float(min(np.diff(grid.x).min(), np.diff(grid.y).min())) / UNIT)
    return s


def on_surface_scene(grid):
    """all_types_scene on a uniform 21^3 mesh of 1-unit cells plus a metal sphere centred on a node whose radius is three cells: its
    six axis nodes lie ON the surface (held, by the closed rule)."""
    s = all_types_scene(grid, (20.0, 20.0, 20.0))
    s.add_metal("ball").add_sphere((10.0, 10.0, 10.0), 3.0, priority=10)
    return s


def _seg_d2(w, e, d):
    """Squared distance of points to a segment (w = p - a, e = p - b, d = b - a, tuples of components)."""
    L = sum(c * c for c in d)
    s = sum(a * c for a, c in zip(w, d))
    ww, ee = sum(c * c for c in w), sum(c * c for c in e)
    return np.where(s <= 0.0, ww, np.where(s >= L, ee, ww - s * s / L)) if L > 0 else ww


def _margins(P, r, verts, x, y, z, tol):
    """How far every comparison that can decide record r's inside test (include/fdtd_hip_voxel.h) is from equality, as a list of
    arrays in length^2: squared comparisons brought to length^2 (the cross-multiplied ones divided by their L), comparisons between
    lengths multiplied by tol.  Empty for a record whose role never holds a point (a flat polygon or a disc as a material)."""
    metal = int(r["role"]) == P.ROLE_METAL
    t = tol if metal else -tol
    if int(r["has_matrix"]):
        m = [float(v) for v in r["m"]]
        x, y, z = (((m[0] * x + m[1] * y) + m[2] * z) + m[3], ((m[4] * x + m[5] * y) + m[6] * z) + m[7],
                   ((m[8] * x + m[9] * y) + m[10] * z) + m[11])
    p = [float(v) for v in r["par"]]
    ty = int(r["type"])
    if ty == P.T_BOX:
        return [(c - (p[a] - t)) * tol for a, c in enumerate((x, y, z))] + [(c - (p[3 + a] + t)) * tol for a, c in enumerate((x, y, z))]
    if ty in (P.T_SPHERE, P.T_SPHERICAL_SHELL):
        d2 = ((x - p[0]) ** 2 + (y - p[1]) ** 2) + (z - p[2]) ** 2
        ro, ri = (p[3] + 0.5 * p[4]) + t, (p[3] - 0.5 * p[4]) - t
        return [d2 - ro * ro] + ([d2 - ri * ri] if ty == P.T_SPHERICAL_SHELL and ri > 0 else [])
    if ty in (P.T_CYLINDER, P.T_CYLINDRICAL_SHELL):
        d = np.array(p[3:6]) - np.array(p[:3])
        L = float(d @ d)
        s = ((x - p[0]) * d[0] + (y - p[1]) * d[1]) + (z - p[2]) * d[2]
        ww = ((x - p[0]) ** 2 + (y - p[1]) ** 2) + (z - p[2]) ** 2
        rho2, ax = ww - s * s / L, s / np.sqrt(L)                  # radial distance^2, axial coordinate
        ro, ri = (p[6] + 0.5 * p[7]) + t, (p[6] - 0.5 * p[7]) - t
        return [rho2 - ro * ro, (ax + t) * tol, (ax - np.sqrt(L) - t) * tol] + ([rho2 - ri * ri] if ty == P.T_CYLINDRICAL_SHELL and ri > 0 else [])
    if ty == P.T_DISC:
        re = p[6] + t
        return [((z - p[2]) - tol) * tol, ((z - p[2]) + tol) * tol, ((x - p[0]) ** 2 + (y - p[1]) ** 2) - re * re] if metal else []
    if ty in (P.T_POLYGON, P.T_LINPOLY):
        if ty == P.T_POLYGON and not metal:
            return []
        n = int(r["norm_dir"])
        pn, pu, pv = ((x, y, z)[(n + q) % 3] for q in range(3))
        out = [((pn - p[0]) - tol) * tol, ((pn - p[0]) + tol) * tol] if ty == P.T_POLYGON else [(pn - (p[0] - t)) * tol, (pn - (p[1] + t)) * tol]
        v0, nv = int(r["vert0"]), int(r["nvert"])
        V = verts[v0:v0 + 2 * nv].reshape(nv, 2)
        for e in range(nv):
            (au, av), (bu, bv) = V[e], V[(e + 1) % nv]
            straddle = (av > pv) != (bv > pv)
            out += [(pv - av) * tol, (pv - bv) * tol,                                       # which edges a point's ray can cross
                    np.where(straddle, (pu - au) * (bv - av) - (pv - av) * (bu - au), np.inf),  # on which side of a straddling edge
                    _seg_d2((pu - au, pv - av), (pu - bu, pv - bv), (bu - au, bv - av)) - tol * tol]    # within tol of the edge
        return out
    if ty == P.T_WIRE:
        re = p[0] + t
        v0, nv = int(r["vert0"]), int(r["nvert"])
        V = verts[v0:v0 + 3 * nv].reshape(nv, 3)
        return [_seg_d2((x - a[0], y - a[1], z - a[2]), (x - b[0], y - b[1], z - b[2]), tuple(b - a)) - re * re
                for a, b in zip(V[:-1], V[1:])] if metal else []
    raise ValueError(f"primitive type {ty}")


def near_surface_share(grid, table, rel=1e-9):
    """(share, closed_side) over EVERY record of the table, on the points its index box holds.  share: the points at which some
    comparison of the record's inside test is within rel * tol^2 of equality (_margins; the least margin counts, decisive or not, so
    the share errs high) — how close a bit-for-bit comparison of two rasterisers comes to a coin toss.  closed_side: the nodes a
    curved or extruded metal holds by the closed rule that the strict rule would not (within tol of its surface; boxes are left out,
    every node of a zero-thickness plate would count) — whether anything was
    near a surface at all."""
    P = pkg("primitives")
    tol = table.tol
    total = close = closed_side = 0
    centers = [grid.centers(a) for a in range(3)]
    for q, r in enumerate(table.rec):
        metal = int(r["role"]) == P.ROLE_METAL
        box = r["nbox"] if metal else r["cbox"]
        if box[3] < box[0]:
            continue
        x, y, z, _ = P._block(grid.lines if metal else centers, box)
        shape = np.broadcast(x, y, z).shape
        margins = _margins(P, r, table.verts, x, y, z, tol)
        if not margins:
            continue
        least = np.minimum.reduce([np.broadcast_to(np.abs(m), shape) for m in margins])
        total += least.size
        close += int(np.count_nonzero(least < rel * tol * tol))
        if metal and int(r["type"]) in (P.T_SPHERE, P.T_SPHERICAL_SHELL, P.T_CYLINDER, P.T_CYLINDRICAL_SHELL, P.T_LINPOLY):
            grown, strict = P.node_mask(grid, table, q)[0], P.node_mask(grid, table, q, role=P.ROLE_MATERIAL)[0]
            closed_side += int(np.count_nonzero(grown & ~strict))
    return (close / total if total else 0.0), closed_side


def sphere_lattice(grid, ext, n=320, seed=7):
    """Several hundred small spheres (alternating material / metal, seeded priorities) in the lower 60 % of the y range: a table
    several LDS chunks long, and tiles no primitive touches."""
    sc = pkg("scene")
    rng = np.random.default_rng(seed)
    s = sc.Scene(unit=UNIT)
    mats = [s.add_material(f"m{q}", 2.0 + q) for q in range(3)]
    mets = [s.add_metal(f"w{q}") for q in range(2)]
    for q in range(n):
        c = (rng.uniform(0.02, 0.98) * ext[0], rng.uniform(0.02, 0.58) * ext[1], rng.uniform(0.02, 0.98) * ext[2])
        r = rng.uniform(0.0413, 0.1317) * min(ext)
        (mats[q % 3] if q % 2 else mets[q % 4 // 2]).add_sphere(c, r, priority=int(rng.integers(0, 3)))
    return s


def probe_patch_script(oe, lib=None, device=0):
    """A coax-probe-fed circular patch through the openEMS API: ground box, substrate Cylinder, zero-height patch Cylinder, feed pin
    Cylinder two cells in radius, lumped port in the gap below the pin.  24 x 24 x 16 cells of 1 mm, CPML 4, 400 steps."""
    FDTD = oe.openEMS(NrTS=400, EndCriteria=0, lib=lib, device=device, cpml_cells=4)
    FDTD.SetGaussExcite(6e9, 3e9)
    FDTD.SetBoundaryCond(["PML_4"] * 6)
    CSX = oe.ContinuousStructure()
    FDTD.SetCSX(CSX)
    mesh = CSX.GetGrid()
    mesh.SetDeltaUnit(UNIT)
    mesh.AddLine("x", np.arange(25) - 12.0)
    mesh.AddLine("y", np.arange(25) - 12.0)
    mesh.AddLine("z", np.arange(17) - 6.0)
    CSX.AddMetal("gnd").AddBox([-8, -8, 0], [8, 8, 0], priority=10)
    CSX.AddMaterial("substrate", epsilon=3.38, kappa=1e-3).AddCylinder([0, 0, 0], [0, 0, 3], 7.31, priority=1)
    CSX.AddMetal("patch").AddCylinder([0, 0, 3], [0, 0, 3], 5.53, priority=10)
    CSX.AddMetal("pin").AddCylinder([2, 0, 1], [2, 0, 3], 2.13, priority=10)
    port = FDTD.AddLumpedPort(1, 50, [2, 0, 0], [2, 0, 1], "z", 1.0, priority=5)
    return FDTD, port
