"""Sub-cell averaged dielectric surfaces (subcell.py, Simulation(subcell=True)): the empty list of scenes whose dielectrics are boxes on
mesh lines, a slab with a known face position against closed forms, the ownership and listing rules, build_operator(edge_overrides=)
against the oracle's fdtd_build_operator, two slabs against one, the resonance of a layered cavity against the root of its transcendental
equation (the known answer, profiles/subcell/kat.txt), the refusals and the off switch."""
import os

import numpy as np
import pytest

from conftest import ROOT, pkg
import primitives_cases as pc
import subcell_cases as sc_
from opbuild_cases import same_bits


def _sub():
    return pkg("subcell")


def _oracle_operator(lib, grid, eps, kap, pec, overrides, dt):
    capi, eco, const = pkg("_capi"), pkg("ecoperator"), pkg("constants")
    nx, ny, nz = grid.shape
    e = capi.Engine(lib, nx, ny, nz, dt, max_steps=8)
    emet, hmet = eco.pack_metric_tables(*eco.metric_lists(grid, dt), grid)
    e.build_operator(grid.d, eps, kap, pec, const.EPS0, overrides, emet, hmet)
    return e.get_operator()


# ---- 1. the empty list ---------------------------------------------------------------------------------------------------------------
def _empty_cases():
    def plugin():
        prep = pc.golden_scene_cases()["fixed_2g45"]()
        grid, scene = prep.FDTD._build_scene()
        return grid, scene

    def tutorial():
        w = pkg("workloads").patch_workload("smoke", nx=48, ny=44, nz=32)
        # the tutorial patch with its substrate's sides on mesh lines, as the plugin's mesher puts them
        sub = [m for m in w.scene.materials if m.name == "substrate"][0]
        b = sub.boxes[0]
        snap = lambda a, v: float(w.grid.lines[a][w.grid.snap(a, v * 1e-3)]) / 1e-3
        b.start = (snap(0, b.start[0]), snap(1, b.start[1]), b.start[2])
        b.stop = (snap(0, b.stop[0]), snap(1, b.stop[1]), b.stop[2])
        return w.grid, w.scene
    return {"box-on-lines": lambda: (pc.grid_of(13, 11, 9), sc_.box_on_lines(pc.grid_of(13, 11, 9))), "tutorial-patch": tutorial, "plugin-fixed": plugin}


@pytest.mark.parametrize("name", sorted(_empty_cases()))
def test_boxes_on_mesh_lines_list_nothing_and_keep_the_operator_bits(oracle_lib, name):
    sc, sim = pkg("scene"), pkg("simulation")
    grid, scene = _empty_cases()[name]()
    assert any(m.boxes for m in scene.materials)
    vox = sc.voxelize(scene, grid, subcell=4)
    assert vox.subcell is not None and len(vox.subcell) == 0 and vox.subcell.dropped_nonplain == 0
    if name == "plugin-fixed":           # the operator bits on the smaller two; the list is what this scene is here for
        return
    ops = []
    for on in (False, True):
        s = sim.Simulation(grid, vox, f0=2.45e9, fc=1.2e9, boundary="PEC" if name == "box-on-lines" else "CPML", cpml_cells=4, nr_ts=10, subcell=on)
        e = s.build(oracle_lib)
        ops.append((e.get_operator(), s.operator_form))
        assert (s.subcell_info() is None) == (not on)
        if on:
            assert s.subcell_info() == {"edges": [0, 0, 0], "nsub": 4, "dropped_lumped": 0, "dropped_nonplain": 0, "operator_form": s.operator_form}
    assert ops[0][1] == ops[1][1]
    for a, b in zip(ops[0][0], ops[1][0]):
        assert same_bits(a, b)


def test_the_tutorial_patch_as_drawn_lists_the_edges_at_its_substrates_sides(oracle_lib):
    """workloads.patch_workload draws its substrate to +-30 mm, between mesh lines of the 200 mm / (n - 1) pitch: with the option on the
    cells those sides cross are mixed, their edges are listed and the operator differs from the staircase's — the scene is no
    boxes-on-mesh-lines scene.  (bench.py does not switch the option on.)"""
    sc, sim = pkg("scene"), pkg("simulation")
    w = pkg("workloads").patch_workload("smoke", nx=48, ny=44, nz=32)
    assert min(np.abs(w.grid.x - 0.03).min(), np.abs(w.grid.y - 0.03).min()) > 1e-4          # the sides are off the lines
    vox = sc.voxelize(w.scene, w.grid, subcell=4)
    ls = vox.subcell
    assert min(ls.edges()) > 100 and ls.dropped_lumped == 0
    i, j = ls.idx % 48, (ls.idx // 48) % 44
    near = lambda l, q: np.minimum(np.abs(l[q] - 0.03), np.abs(l[q] + 0.03)) <= 1.01 * (l[1] - l[0])
    assert np.all(near(w.grid.x, i) | near(w.grid.y, j))                                      # all of them at the four sides
    ops = [sim.Simulation(w.grid, vox, f0=w.f0, fc=w.fc, boundary="CPML", cpml_cells=4, nr_ts=10, subcell=on).build(oracle_lib).get_operator() for on in (False, True)]
    assert not same_bits(ops[0][0], ops[1][0]) or not same_bits(ops[0][1], ops[1][1])
    assert same_bits(ops[0][3], ops[1][3])


# ---- 2. a slab with a known face position ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frac", [0.25, 0.5, 0.75, 0.1])
def test_slab_face_at_a_known_fraction_of_a_cell(frac):
    """Face normal to z at `frac` of cell 4 (graded mesh, nsub = 4: the fill fractions 1/4, 2/4, 3/4 are exact on the lattice; at 0.1 no
    sample is inside and nothing is listed).  z-edges of cell 4: 4 / (n / eps2 + (4 - n) / eps1), kappa n kappa2 / 4.  x- and y-edges on
    the two adjacent node planes, 4 and 5: the arithmetic value of their two half cells, the half of cell 4 filled to min(n, 2) / 2
    below and max(n - 2, 0) / 2 above."""
    grid = pc.grid_of(13, 11, 9)
    nx, ny, nz = grid.shape
    e1, e2, k2 = 1.0, 4.0, 0.01
    _, _, _, ls = sc_.spec_of(sc_.slab(grid, frac, k=4, eps=e2, kappa=k2), grid, 4)
    n = int(frac * 4)
    if n == 0:
        assert len(ls) == 0
        return
    k, r = np.divmod(ls.idx, nx * ny)
    z = ls.comp == 2
    assert np.count_nonzero(z) == (nx - 2) * (ny - 2) and np.all(k[z] == 4)
    want = 4.0 / (n / e2 + (4 - n) / e1)
    assert np.all(np.abs(ls.eps_rel[z] - want) <= 1e-15 * want)
    assert np.all(np.abs(ls.kap_e[z] - n * k2 / 4.0) <= 1e-15 * n * k2 / 4.0)
    dz = np.diff(grid.z)
    assert np.count_nonzero(ls.comp == 0) == 2 * (nx - 1) * (ny - 2) and np.count_nonzero(ls.comp == 1) == 2 * (nx - 2) * (ny - 1)
    assert set(k[~z].tolist()) == {4, 5}
    fill = {4: (1.0, min(n, 2) / 2.0), 5: (max(n - 2, 0) / 2.0, 0.0)}          # plane -> the fill of its lower and of its upper half cell
    for plane, (lo, hi) in fill.items():
        on = ~z & (k == plane)
        we = (dz[plane - 1] * (lo * e2 + (1.0 - lo) * e1) + dz[plane] * (hi * e2 + (1.0 - hi) * e1)) / (dz[plane - 1] + dz[plane])
        wk = (dz[plane - 1] * lo * k2 + dz[plane] * hi * k2) / (dz[plane - 1] + dz[plane])
        assert np.all(np.abs(ls.eps_rel[on] - we) <= 1e-15 * we), (plane, np.abs(ls.eps_rel[on] / we - 1).max())
        assert np.all(np.abs(ls.kap_e[on] - wk) <= 1e-15 * wk), (plane, wk, np.abs(ls.kap_e[on] - wk).max())


# ---- 3. ownership and listing rules ----------------------------------------------------------------------------------------------------
def _prop_at(grid, scene, point, nsub=4):
    sub, prims = _sub(), pkg("primitives")
    pid = sub.lattice_props(grid, prims.pack_table(scene, grid), nsub)
    at = [int(np.argmin(np.abs(sub.sub_points(grid.lines[a], 0, grid.shape[a] - 2, nsub) - point[a] * sc_.UNIT))) for a in range(3)]
    return int(pid[at[2], at[1], at[0]])


def test_priority_and_the_later_record_on_a_tie():
    grid = pc.grid_of(13, 11, 9)
    mid = (17.6, 13.85, 11.3)                                      # inside both spheres
    assert _prop_at(grid, sc_.two_spheres(0, 0), mid) == 1         # a tie: the later record
    assert _prop_at(grid, sc_.two_spheres(1, 0), mid) == 0         # the higher priority
    assert _prop_at(grid, sc_.two_spheres(0, 0), (14.3, 13.1, 10.7)) == 0 and _prop_at(grid, sc_.two_spheres(0, 0), (1.0, 1.0, 1.0)) == 2


def test_two_records_of_one_material_list_nothing_in_their_overlap():
    grid = pc.grid_of(25, 21, 17)
    _, _, _, one = sc_.spec_of(sc_.two_spheres(same=True), grid, 4)
    _, _, _, two = sc_.spec_of(sc_.two_spheres(same=False), grid, 4)
    # ONE material (values are compared): only the cells that the union's surface crosses are mixed, so every listed value is a mean of
    # the material's and the vacuum's
    assert len(one) > 100 and np.all(one.eps_rel <= 3.3 * (1 + 1e-15)) and np.any(one.eps_rel < 3.2)
    # two materials: the cells the surface of a crosses inside b are mixed too
    assert np.any(two.eps_rel > 3.3 + 1e-9) and len(two) > len(one)
    key = lambda ls: set(zip(ls.comp.tolist(), ls.idx.tolist()))
    assert key(one) < key(two)


def test_an_anisotropic_owner_makes_the_components_differ():
    grid = pc.grid_of(13, 11, 9)
    s = pkg("scene").Scene(unit=sc_.UNIT)
    s.add_material("crystal", (2.1, 5.3, 9.7), (0.0, 0.02, 0.005)).add_sphere((17.3, 13.9, 10.4), 8.3)
    _, _, _, ls = sc_.spec_of(s, grid, 4)
    top = [ls.eps_rel[ls.comp == c].max() for c in range(3)]
    up = 1 + 1e-15
    assert 1.5 < top[0] <= 2.1 * up and 2.1 * up < top[1] <= 5.3 * up and 5.3 * up < top[2] <= 9.7 * up
    assert np.all(ls.kap_e[ls.comp == 0] == 0.0) and ls.kap_e[ls.comp == 1].max() > ls.kap_e[ls.comp == 2].max() > 0.0


def test_lumped_pec_and_outer_plane_edges_are_absent():
    sc, sub = pkg("scene"), _sub()
    grid, scene = sc_.sphere_port_scene(metal=True)
    vox = sc.voxelize(scene, grid, subcell=4)
    ls = vox.subcell
    port = [(e.comp, int(grid.flat(e.i, e.j, e.k))) for e in vox.lumped]
    skip = sub.skip_mask(grid, vox.pec, [q for _, q in port], [c for c, _ in port])
    assert len(ls) > 100 and np.all(skip.reshape(3, -1)[ls.comp.astype(np.int64), ls.idx] == sub.SKIP_LIVE)
    assert vox.pec.any() and not vox.pec.reshape(3, -1)[ls.comp.astype(np.int64), ls.idx].any()
    assert len(port) == 3 and ls.dropped_lumped >= 1               # the port grazes the sphere: a mixed edge with an override
    assert not set(port) & set(zip(ls.comp.tolist(), ls.idx.tolist()))
    # a sphere that sticks out of the grid: nothing on the outer planes, no non-existent last edge
    g2 = pc.grid_of(13, 11, 9)
    _, _, skip2, out = sc_.spec_of(sc_.one_primitive("half-outside"), g2, 4)
    assert len(out) > 20 and np.all(skip2.reshape(3, -1)[out.comp.astype(np.int64), out.idx] == 0)
    k, r = np.divmod(out.idx, 13 * 11)
    assert np.all((k[out.comp != 2] >= 1) & (k[out.comp != 2] <= 7)) and np.all(k[out.comp == 2] <= 7)
    # the list is ordered by component, then index
    key = ls.comp.astype(np.int64) * grid.ncells + ls.idx
    assert np.all(np.diff(key) > 0)


def test_an_edge_with_a_debye_sample_is_dropped_and_counted():
    grid = pc.grid_of(13, 11, 9)

    def scene(debye):
        s = pkg("scene").Scene(unit=sc_.UNIT)
        m = s.add_debye_material("wet", 3.1, 0.0, [1.2], [8e-12]) if debye else s.add_material("wet", 3.1)
        m.add_sphere((17.3, 13.9, 10.4), 8.3)
        s.add_material("dry", 2.2).add_box((2.9, 3.1, 2.7), (9.3, 8.7, 7.9))       # clear of the sphere
        return s
    _, _, _, plain = sc_.spec_of(scene(False), grid, 4)
    _, _, _, disp = sc_.spec_of(scene(True), grid, 4)
    assert plain.dropped_nonplain == 0 and disp.dropped_nonplain > 100
    assert len(disp) > 0 and len(disp) + disp.dropped_nonplain == len(plain)       # the box's edges stay listed
    keep = ~np.isin(plain.comp.astype(np.int64) * grid.ncells + plain.idx, disp.comp.astype(np.int64) * grid.ncells + disp.idx)
    assert np.count_nonzero(keep) == disp.dropped_nonplain


def test_chunked_walk_gives_the_same_list():
    grid = pc.grid_of(25, 21, 17)
    table, tabs, skip, ls = sc_.spec_of(sc_.two_spheres(), grid, 2)
    assert sc_.same_listed(ls, _sub().edges_spec(grid, table, 2, *tabs, skip, lattice_points=1 << 14))


# ---- 4. build_operator(edge_overrides=) -------------------------------------------------------------------------------------------------
def test_build_operator_with_edge_overrides_equals_the_oracles(oracle_lib):
    sc, sub, eco = pkg("scene"), _sub(), pkg("ecoperator")
    grid, scene = sc_.sphere_port_scene()
    vox = sc.voxelize(scene, grid, subcell=4)
    dt = grid.courant_dt()
    ov = sub.overrides(vox.subcell, dt)
    assert ov[0].size > 100 and ov[2].dtype == np.float32
    lum = eco.lumped_overrides(grid, vox.eps_r, vox.kappa, vox.pec, dt, vox.lumped)
    both = tuple(np.concatenate([a, b]) for a, b in zip(lum, ov))
    base = eco.build_operator(grid, vox.eps_r, vox.kappa, vox.pec, dt, vox.lumped)
    none = eco.build_operator(grid, vox.eps_r, vox.kappa, vox.pec, dt, vox.lumped, edge_overrides=None)
    with_ = eco.build_operator(grid, vox.eps_r, vox.kappa, vox.pec, dt, vox.lumped, edge_overrides=ov)
    for a, b in zip(base.raw(), none.raw()):
        assert same_bits(a, b)
    for name, a, b in zip(("vv", "vi", "ii", "iv"), none.raw(), _oracle_operator(oracle_lib, grid, vox.eps_r, vox.kappa, vox.pec, lum, dt)):
        assert same_bits(a, b), name
    for name, a, b in zip(("vv", "vi", "ii", "iv"), with_.raw(), _oracle_operator(oracle_lib, grid, vox.eps_r, vox.kappa, vox.pec, both, dt)):
        assert same_bits(a, b), name
    assert not same_bits(with_.vv, base.vv) and not same_bits(with_.m, base.m)
    # ... and Simulation hands the same list to the device build and to the host arrays
    dev, host = sc_.sphere_port_sim(), sc_.sphere_port_sim()
    host.device_operator = False
    ed, eh = dev.build(oracle_lib), host.build(oracle_lib)
    for name, a, b in zip(("vv", "vi", "ii", "iv"), ed.get_operator(), eh.get_operator()):
        assert same_bits(a, b), name
    info = dev.subcell_info()
    assert info["nsub"] == 4 and sum(info["edges"]) == len(dev.subcell) and info["dropped_lumped"] >= 1 and info["operator_form"] in ("classes", "raw")


# ---- 5. two slabs -----------------------------------------------------------------------------------------------------------------------
def test_two_slabs_equal_one_slab(oracle_lib):
    import source_probe_cases as spc
    steps = 80
    one = sc_.sphere_port_sim(nr_ts=steps)
    e1 = one.build(oracle_lib)
    e1.run(steps)
    want = e1.fields()
    two = sc_.sphere_port_sim(nr_ts=steps)
    cuts = [(0, 8), (8, 8)]                                         # the cut goes through the sphere
    two.slabs = lambda world, partition="cost": list(cuts)
    engs = [two.build(oracle_lib, rank=r, world=2) for r in range(2)]
    spc.slab_stepper(engs, "half-steps")(steps)
    got = np.concatenate([e.fields() for e in engs], axis=2)
    assert np.abs(want).max() > 0 and np.array_equal(got, want)
    assert np.array_equal(got[want != 0].view(np.uint32), want[want != 0].view(np.uint32))
    ops = [e.get_operator() for e in engs]
    for q, a in enumerate(e1.get_operator()):
        assert same_bits(np.concatenate([ops[0][q], ops[1][q]], axis=1), a)


# ---- 6. known answers ------------------------------------------------------------------------------------------------------------------
KAT = os.path.join(ROOT, "profiles", "subcell", "kat.txt")
OFFSETS = (0.25, 0.49, 0.51, 0.75)


def _note(tag, lines):
    """Replace the block `tag` of profiles/subcell/kat.txt when FDTD_WRITE_KAT is set (the committed record of the measured values)."""
    if not os.environ.get("FDTD_WRITE_KAT"):
        return
    os.makedirs(os.path.dirname(KAT), exist_ok=True)
    old = open(KAT).read().split("\n") if os.path.isfile(KAT) else []
    keep, skip = [], False
    for l in old:
        if l.startswith("## "):
            skip = l == f"## {tag}"
        if not skip and l != "":
            keep.append(l)
    with open(KAT, "w") as fh:
        fh.write("\n".join(keep + [f"## {tag}"] + list(lines)) + "\n")


def test_layered_cavity_resonance_against_the_transcendental_root(oracle_lib):
    """A PEC cube of 20^3 cells, eps 4 below and 1 above an interface at 0.25 / 0.49 / 0.51 / 0.75 of a cell past the middle plane; the
    lowest mode with E_z (TM to z: E normal and tangential to the interface) from a probe spectrum of 40000 timesteps (Gaussian window,
    parabola through the logarithms of three bins: the bin is 2.1e-3 of the resonance, the fit resolves it far below 1e-4).  Reference:
    the root of the continuous cavity's transcendental equation (subcell_cases.layered_cavity_root), so each error also holds the
    mesh's own dispersion error, the same for both runs.  At every offset the sub-cell error is below a quarter of the staircase's,
    and the sub-cell jump from 0.49 to 0.51 is below a quarter of the staircase's jump.
    Measured (profiles/subcell/kat.txt): staircase +0.498 / +1.045 / -1.113 / -0.602 %, sub-cell -0.072 / -0.078 / -0.034 / -0.026 %;
    jump 2.201 % against 0.000 % (the two lattices are the same; the references differ by 0.044 %)."""
    ref = [sc_.layered_cavity_root(f) for f in OFFSETS]
    stair = [sc_.layered_cavity_resonance(oracle_lib, f, False) for f in OFFSETS]
    sub = [sc_.layered_cavity_resonance(oracle_lib, f, True) for f in OFFSETS]
    es = [a / r - 1.0 for a, r in zip(stair, ref)]
    eu = [a / r - 1.0 for a, r in zip(sub, ref)]
    jump_s, jump_u = abs(stair[2] - stair[1]) / ref[1], abs(sub[2] - sub[1]) / ref[1]
    lines = [f"offset {f:.2f}: root {r / 1e9:.5f} GHz, staircase {a / 1e9:.5f} GHz ({100 * x:+.3f} %), sub-cell {b / 1e9:.5f} GHz ({100 * y:+.3f} %), ratio {abs(y / x):.3f} (allowed 0.25)"
             for f, r, a, b, x, y in zip(OFFSETS, ref, stair, sub, es, eu)]
    lines.append(f"jump 0.49 -> 0.51: staircase {100 * jump_s:.3f} %, sub-cell {100 * jump_u:.3f} % (allowed a quarter of the staircase's; the roots differ by {100 * abs(ref[2] / ref[1] - 1):.3f} %)")
    print("\n".join(lines))
    _note("layered PEC cavity, 20^3 cells, eps 4 / 1, lowest mode with E_z, nsub 4, 40000 timesteps on the float32 oracle; errors against the transcendental root", lines)
    for f, x, y in zip(OFFSETS, es, eu):
        assert abs(y) < 0.25 * abs(x), (f, x, y)
    assert jump_u < 0.25 * jump_s


def test_sphere_resonance_record(oracle_lib):
    """No bar: the lowest resonance with E_z of a dielectric sphere (eps 10, radius 5 cells) in the 20^3 PEC cube, its centre shifted by
    0, 1/4, 1/2 cell along x, staircase and sub-cell — recorded in profiles/subcell/kat.txt (20000 timesteps; measured spread 0.95 %
    against 0.12 %).  Asserted: the resonances exist and the sub-cell spread is not the larger one."""
    shifts = (0.0, 0.25, 0.5)
    stair = [sc_.sphere_resonance(oracle_lib, s, False, 20000) for s in shifts]
    sub = [sc_.sphere_resonance(oracle_lib, s, True, 20000) for s in shifts]
    spread = lambda v: (max(v) - min(v)) / np.mean(v)
    lines = [f"shift {s:.2f} cell: staircase {a / 1e9:.5f} GHz, sub-cell {b / 1e9:.5f} GHz" for s, a, b in zip(shifts, stair, sub)]
    lines.append(f"spread: staircase {100 * spread(stair):.3f} %, sub-cell {100 * spread(sub):.3f} %")
    print("\n".join(lines))
    _note("dielectric sphere (eps 10, radius 5 cells) in the 20^3 PEC cube, lowest resonance with E_z, 20000 timesteps; no bar", lines)
    assert all(np.isfinite(v) and 5e9 < v < 12e9 for v in stair + sub) and spread(sub) <= spread(stair)


# ---- 7. refusals and the off switch ----------------------------------------------------------------------------------------------------
def test_refusals_and_the_off_switch():
    sc, sim, oe = pkg("scene"), pkg("simulation"), pkg("openems_api")
    grid, scene = sc_.sphere_port_scene()
    for bad in (3, 1, 16, 4.5):
        with pytest.raises(ValueError, match="subcell_samples"):
            sc.voxelize(scene, grid, subcell=bad)
        with pytest.raises(ValueError, match="subcell_samples"):
            oe.openEMS(NrTS=10, subcell=True, subcell_samples=bad)
    plain = sc.voxelize(scene, grid)
    assert plain.subcell is None
    with pytest.raises(ValueError, match="needs the listed edges"):
        sim.Simulation(grid, plain, f0=12e9, fc=6e9, boundary="PEC", subcell=True)
    with pytest.raises(ValueError, match="voxelised with subcell=2"):
        sim.Simulation(grid, sc.voxelize(scene, grid, subcell=2), f0=12e9, fc=6e9, boundary="PEC", subcell=True, subcell_samples=4)
    with pytest.raises(ValueError, match="subcell_samples"):
        sim.Simulation(grid, plain, f0=12e9, fc=6e9, boundary="PEC", subcell=True, subcell_samples=5)
    off = sim.Simulation(grid, sc.voxelize(scene, grid, subcell=4), f0=12e9, fc=6e9, boundary="PEC")      # listed, not asked for: today's overrides
    assert off.subcell is None and off._overrides()[0].size == 3
    s2, g2 = sc.Scene(unit=sc_.UNIT), grid
    lines = [np.linspace(4.0, 16.0, 5)] * 3
    s2.add_disc_material("body", lines, np.ones((4, 4, 4), np.uint8), [1.0, 40.0], [0.0, 0.5], [0.0, 1000.0]).add_box((4, 4, 4), (16, 16, 16))
    with pytest.raises(ValueError, match="AddDiscMaterial"):
        sc.voxelize(s2, g2, subcell=4)
    with pytest.raises(ValueError, match="AddDiscMaterial"):
        sim.Simulation(g2, sc.voxelize(s2, g2), f0=12e9, fc=6e9, boundary="PEC", subcell=True)
