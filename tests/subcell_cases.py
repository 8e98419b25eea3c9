"""Scenes and meshes shared by test_subcell_cpu.py and test_subcell_gpu.py (no tests here).  Radii and offsets are non-round decimals,
so that no sample sits within rounding of a surface by accident."""
import numpy as np
from conftest import pkg
import primitives_cases as pc

UNIT = pc.UNIT
EXT = (36.0, 28.0, 22.0)


def box_on_lines(grid):
    """A lossy box whose six faces lie on mesh lines."""
    s = pkg("scene").Scene(unit=UNIT)
    lo = [grid.lines[a][2] / UNIT for a in range(3)]
    hi = [grid.lines[a][-3] / UNIT for a in range(3)]
    s.add_material("block", 4.3, 0.02).add_box(lo, hi)
    return s


def slab(grid, frac, k=4, eps=4.0, kappa=0.01):
    """A slab over the whole x-y extent from z line 2 to `frac` of a cell past z line k."""
    s = pkg("scene").Scene(unit=UNIT)
    z1 = (grid.z[k] + frac * (grid.z[k + 1] - grid.z[k])) / UNIT
    s.add_material("slab", eps, kappa).add_box((-5.0, -5.0, grid.z[2] / UNIT), (EXT[0] + 5.0, EXT[1] + 5.0, z1))
    return s


def two_spheres(prio_a=0, prio_b=0, eps_a=3.3, eps_b=7.1, same=False):
    """Two overlapping spheres, a drawn before b; same: both of ONE material, as two records."""
    s = pkg("scene").Scene(unit=UNIT)
    a = s.add_material("a", eps_a)
    b = a if same else s.add_material("b", eps_b)
    a.add_sphere((14.3, 13.1, 10.7), 6.7, priority=prio_a)
    b.add_sphere((20.9, 14.6, 11.9), 6.1, priority=prio_b)
    return s


TETRA = np.array([[3.1, 4.2, 2.3], [31.7, 6.1, 4.9], [12.3, 24.9, 7.7], [15.9, 11.3, 20.1]])


def one_primitive(kind, grid=None):
    """name -> a scene with that primitive as a lossy material, over EXT (grid: the mesh, for the kind that is placed by its cells)."""
    s = pkg("scene").Scene(unit=UNIT)
    m = s.add_material(kind, 5.7, 0.013)
    if kind == "sphere":
        m.add_sphere((17.3, 13.9, 10.4), 8.3)
    elif kind == "spherical-shell":
        m.add_spherical_shell((17.3, 13.9, 10.4), 7.9, 3.1)
    elif kind == "oblique-cylinder":
        m.add_cylinder((5.3, 6.1, 3.7), (30.9, 21.3, 18.1), 4.7)
    elif kind == "cylindrical-shell":
        m.add_cylindrical_shell((7.1, 21.7, 4.3), (29.3, 7.9, 17.3), 5.9, 2.7)
    elif kind == "rotated-box":
        m.add_box((-9.3, -5.1, -3.7), (9.9, 6.3, 4.1))
        m.boxes[-1].matrix = pc.rot(2, 31.7, (18.1, 14.3, 11.2)) @ pc.rot(0, 17.9)
    elif kind == "linpoly":
        m.add_lin_poly([[4.1, 30.3, 22.7, 14.9, 6.3], [5.3, 7.9, 23.1, 12.7, 21.9]], 2, 4.3, 11.9)
    elif kind == "tetrahedron":
        t = TETRA
        m.add_polyhedron(np.array([[t[0], t[1], t[2]], [t[0], t[1], t[3]], [t[1], t[2], t[3]], [t[2], t[0], t[3]]]))
    elif kind == "equal-priority-overlap":
        m.add_sphere((14.3, 13.1, 10.7), 6.7, priority=2)
        s.add_material("other", 2.9).add_cylinder((9.1, 12.9, 3.1), (27.3, 15.1, 19.3), 4.9, priority=2)
    elif kind == "half-outside":
        m.add_sphere((35.1, 13.9, 1.3), 7.7)
    elif kind == "smaller-than-a-cell":
        c = [0.5 * (grid.lines[a][q] + grid.lines[a][q + 1]) / UNIT for a, q in enumerate((6, 5, 4))]
        m.add_sphere((c[0] + 0.11, c[1] - 0.07, c[2] + 0.05), 0.9)          # holds the centre of cell (6, 5, 4), whose sides are 2.1 mm and more
        s.add_material("speck", 3.1).add_box((9.05, 9.1, 9.07), (9.6, 9.7, 9.5))     # holds no cell centre: invisible
    elif kind == "anisotropic":
        s.materials.pop()
        s.add_material("crystal", (2.1, 5.3, 9.7), (0.0, 0.02, 0.005)).add_sphere((17.3, 13.9, 10.4), 8.3)
        s.add_material("glass", 3.9).add_cylinder((4.1, 14.1, 10.9), (33.2, 13.2, 11.7), 3.3, priority=1)
    else:
        raise KeyError(kind)
    return s


KINDS = ("sphere", "spherical-shell", "oblique-cylinder", "cylindrical-shell", "rotated-box", "linpoly", "tetrahedron",
         "equal-priority-overlap", "half-outside", "smaller-than-a-cell", "anisotropic")


def large_case():
    """48 x 40 x 36 nodes, a spherical shell of radius 15 cells and a rotated box through it: every pass spans several blocks."""
    grid = pc.grid_of(48, 40, 36, ext=(47.0, 39.0, 35.0), grade=False)
    s = pkg("scene").Scene(unit=UNIT)
    s.add_material("shell", 6.3, 0.01).add_spherical_shell((23.4, 19.7, 17.3), 15.0, 2.3)
    m = s.add_material("bar", 2.7)
    m.add_box((-21.3, -3.1, -2.7), (21.9, 3.3, 2.9), priority=1)
    m.boxes[-1].matrix = pc.rot(1, 23.0, (23.1, 19.3, 17.9)) @ pc.rot(2, 41.0)
    return grid, s


def spec_of(scene, grid, nsub, lumped=None):
    """(table, property tables, skip, subcell.edges_spec's Listed) of a scene on its staircase."""
    sc, sub, prims = pkg("scene"), pkg("subcell"), pkg("primitives")
    vs = sc.voxelize(scene, grid)
    table = prims.pack_table(scene, grid)
    tabs = sub.prop_tables(scene)
    skip = sub.skip_mask(grid, vs.pec, *(lumped or (None, None)))
    return table, tabs, skip, sub.edges_spec(grid, table, nsub, *tabs, skip)


def same_listed(a, b):
    return (np.array_equal(a.comp, b.comp) and np.array_equal(a.idx, b.idx) and a.nsub == b.nsub and
            np.array_equal(a.eps_rel.view(np.uint64), b.eps_rel.view(np.uint64)) and np.array_equal(a.kap_e.view(np.uint64), b.kap_e.view(np.uint64)) and
            (a.dropped_lumped, a.dropped_nonplain) == (b.dropped_lumped, b.dropped_nonplain))


def sphere_port_scene(metal=False):
    """20 x 18 x 16 nodes (1 mm cells): a dielectric sphere, a 50 ohm lumped port beside it that grazes the sphere's surface,
    optionally a metal sphere on the other side."""
    grid = pkg("grid").RectGrid(*[np.arange(n) * 1e-3 for n in (20, 18, 16)])
    s = pkg("scene").Scene(unit=UNIT)
    s.add_material("ball", 9.8, 0.02).add_sphere((7.6, 8.7, 7.4), 2.4)
    s.add_lumped_port(1, 50.0, (10.0, 9.0, 6.0), (10.0, 9.0, 9.0), "z", 1.0)
    if metal:                         # its cut faces stay clear of the four-cell CPML layers
        s.add_metal("bead").add_sphere((12.1, 8.3, 7.3), 1.3)
    return grid, s


def sphere_port_sim(subcell=True, conformal=False, nr_ts=60, nsub=4, device_subcell=None, **kw):
    sc, sim = pkg("scene"), pkg("simulation")
    grid, s = sphere_port_scene(metal=conformal)
    vox = sc.voxelize(s, grid, conformal=conformal, subcell=nsub if subcell else 0, device_subcell=device_subcell)
    return sim.Simulation(grid, vox, f0=12e9, fc=6e9, boundary="CPML", cpml_cells=4, nr_ts=nr_ts, end_criteria=0.0, conformal=conformal,
                          subcell=subcell, subcell_samples=nsub, **kw)


# ---- known answers: resonances from a probe spectrum ----------------------------------------------------------------------------------
C0 = 299792458.0
KAT_CELLS, KAT_SIDE, KAT_STEPS = 20, 20e-3, 40000
KAT_EPS = 4.0


def lowest_peak(u, dt, floor=0.05):
    """Frequency [Hz] of the lowest spectral line of the series u that reaches `floor` of the largest: a Gaussian window (whose
    transform is a Gaussian: the parabola through the logarithms of the three bins around the maximum is exact for a single line)."""
    n = u.size
    w = np.exp(-0.5 * ((np.arange(n) - 0.5 * (n - 1)) / (n / 8.0)) ** 2)
    spec = np.abs(np.fft.rfft(np.asarray(u, np.float64) * w))
    peaks = [q for q in range(2, spec.size - 1) if spec[q] > spec[q - 1] and spec[q] >= spec[q + 1] and spec[q] >= floor * spec.max()]
    q = peaks[0]
    a, b, c = np.log(spec[q - 1:q + 2])
    return (q + 0.5 * (a - c) / (a - 2.0 * b + c)) / (n * dt)


def _resonance(lib, scene, subcell, f0, fc, nsteps=KAT_STEPS):
    """The lowest resonance with E_z of a loss-free PEC cube of KAT_CELLS^3 cells holding `scene`, driven and probed on z edges off
    every symmetry plane."""
    sc, sim, capi, grid_m = pkg("scene"), pkg("simulation"), pkg("_capi"), pkg("grid")
    grid = grid_m.RectGrid(*[np.arange(KAT_CELLS + 1) * (KAT_SIDE / KAT_CELLS)] * 3)
    m = sim.Simulation(grid, sc.voxelize(scene, grid, subcell=4 if subcell else 0), f0=f0, fc=fc, boundary="PEC", nr_ts=nsteps, end_criteria=0.0,
                       subcell=subcell)
    e = m.build(lib)
    one = lambda i, j, k: np.array([grid.flat(i, j, k)], np.int64)
    z8, w1 = np.full(1, 2, np.int8), np.ones(1, np.float32)
    e.add_source(one(6, 5, 3), z8, w1, np.zeros(1, np.int32))
    pid = e.add_probe(capi.KIND_V, one(13, 11, 14), z8, w1)
    e.run(nsteps)
    u = np.asarray(e.get_probe(pid), np.float64)
    e.close()
    assert u.size == nsteps and np.all(np.isfinite(u))
    return lowest_peak(u, m.dt)


def layered_cavity_resonance(lib, frac, subcell):
    """The cube filled with KAT_EPS from z = 0 to `frac` of a cell past its middle plane, vacuum above: the lowest mode with E_z (TM
    to z, one half wave along x and y) has E normal and tangential to the interface."""
    s = pkg("scene").Scene(unit=1e-3)
    h = KAT_SIDE / KAT_CELLS / 1e-3
    s.add_material("fill", KAT_EPS, 0.0).add_box([-1.0, -1.0, -1.0], [KAT_SIDE / 1e-3 + 1.0, KAT_SIDE / 1e-3 + 1.0, (KAT_CELLS // 2 + frac) * h])
    return _resonance(lib, s, subcell, 6e9, 3e9)


def layered_cavity_root(frac):
    """The same mode of the continuous cavity: the lowest root of (k1 / eps1) tan(k1 d1) + (k2 / eps2) tan(k2 d2) = 0,
    k_i^2 = eps_i k0^2 - 2 (pi / a)^2 (H_t and E_t continuous at the interface, E_t = 0 on both walls), multiplied through by the two
    cosines and evaluated with complex square roots (a layer below cut-off has an imaginary k_i; the product stays real)."""
    from scipy.optimize import brentq
    a = KAT_SIDE
    d1 = (KAT_CELLS // 2 + frac) * a / KAT_CELLS
    d2 = a - d1
    kt2 = 2.0 * (np.pi / a) ** 2

    def g(k0):
        k1, k2 = np.sqrt(complex(KAT_EPS * k0 * k0 - kt2)), np.sqrt(complex(k0 * k0 - kt2))
        return ((k1 / KAT_EPS) * np.sin(k1 * d1) * np.cos(k2 * d2) + k2 * np.sin(k2 * d2) * np.cos(k1 * d1)).real
    ks = np.linspace(1.0001 * np.sqrt(kt2 / KAT_EPS), 2.0 * np.sqrt(kt2), 4000)
    v = np.array([g(k) for k in ks])
    q = int(np.flatnonzero(np.sign(v[:-1]) != np.sign(v[1:]))[0])
    return brentq(g, ks[q], ks[q + 1], xtol=1e-14, rtol=1e-14) * C0 / (2.0 * np.pi)


def sphere_resonance(lib, shift, subcell, nsteps=KAT_STEPS):
    """The lowest resonance with E_z of the cube with a dielectric sphere (eps 10, radius 5 cells) whose centre is the cube's, shifted
    by `shift` cells along x."""
    s = pkg("scene").Scene(unit=1e-3)
    h = KAT_SIDE / KAT_CELLS / 1e-3
    c = 0.5 * KAT_SIDE / 1e-3
    s.add_material("ball", 10.0, 0.0).add_sphere((c + shift * h, c, c), 5.0 * h)
    return _resonance(lib, s, subcell, 6e9, 3e9, nsteps)
