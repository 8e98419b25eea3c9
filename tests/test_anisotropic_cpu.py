"""Anisotropic dielectrics (per-axis permittivity and conductivity) without a GPU: the composition identity of the specification
(ecoperator.build_operator) against itself and against the oracle's isotropic builds; scenes that see one axis only, bit for bit
against the isotropic run on the float32 oracle; the bounds a uniaxial filling puts on a cavity resonance; the Scene / CSXCAD
spellings, the refusals and both voxelisers."""
import inspect

import numpy as np
import pytest

from conftest import pkg
import helpers
import anisotropic_cases as ac
from opbuild_cases import random_scene, same_bits


# ---- 1. the composition identity of the specification --------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,shape,graded,nmat", [(1, (21, 18, 15), False, 3), (2, (24, 19, 17), True, 8), (3, (9, 8, 7), True, 5)])
def test_component_c_is_the_isotropic_operator_of_axis_c(oracle_lib, seed, shape, graded, nmat):
    eco = pkg("ecoperator")
    grid, eps, kap, pec, lumped = ac.aniso_random_scene(seed, shape, graded, nmat)
    assert all(not np.array_equal(eps[a], eps[b]) and not np.array_equal(kap[a], kap[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
    dt = grid.courant_dt()
    op = eco.build_operator(grid, eps, kap, pec, dt, lumped)
    over = eco.lumped_overrides(grid, eps, kap, pec, dt, lumped)
    assert over[0].size == len(lumped)
    for c in range(3):
        iso = eco.build_operator(grid, eps[c], kap[c], pec, dt, lumped)
        assert same_bits(op.vv[c], iso.vv[c]) and same_bits(op.m[c], iso.m[c]), c
        other = (c + 1) % 3
        assert not same_bits(op.vv[other], iso.vv[other]) or not same_bits(op.m[other], iso.m[other])
        oc = eco.lumped_overrides(grid, eps[c], kap[c], pec, dt, lumped)
        on = over[1] == c
        assert np.array_equal(over[0][on], oc[0][on]) and same_bits(over[2][on], oc[2][on]) and same_bits(over[3][on], oc[3][on])
        k = [le for le in lumped if le.comp == c]           # the overridden edges themselves, in the operator
        for le in k:
            assert op.vv[c, le.k, le.j, le.i] == iso.vv[c, le.k, le.j, le.i] != 0
    # the oracle's fdtd_build_operator gives the same three components (raw expansion: vi, ii and iv too)
    ref = ac.composed_oracle_operator(oracle_lib, grid, eps, kap, pec, lumped, dt)
    for name, a, b in zip(("vv", "vi", "ii", "iv"), op.raw(), ref):
        assert same_bits(a, b), name
    # mixed spellings: per-axis eps with per-cell kappa
    mixed = eco.build_operator(grid, eps, kap[1], pec, dt, lumped)
    want = eco.build_operator(grid, eps[0], kap[1], pec, dt, lumped)
    assert same_bits(mixed.vv[0], want.vv[0]) and same_bits(mixed.m[0], want.m[0])


@pytest.mark.parametrize("seed,shape,graded,nmat", [(1, (21, 18, 15), False, 3), (2, (24, 19, 17), True, 8)])
def test_three_equal_slices_are_the_scalar_call(seed, shape, graded, nmat):
    eco = pkg("ecoperator")
    grid, eps, kap, pec, lumped = random_scene(seed, shape, graded, nmat)
    dt = grid.courant_dt()
    a = eco.build_operator(grid, eps, kap, pec, dt, lumped)
    b = eco.build_operator(grid, np.stack([eps] * 3), np.stack([kap] * 3), pec, dt, lumped)
    assert same_bits(a.vv, b.vv) and same_bits(a.m, b.m)
    for x, y in zip(eco.lumped_overrides(grid, eps, kap, pec, dt, lumped), eco.lumped_overrides(grid, np.stack([eps] * 3), np.stack([kap] * 3), pec, dt, lumped)):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    with pytest.raises(ValueError, match="cell arrays must be"):
        eco.build_operator(grid, np.stack([eps] * 2), kap, pec, dt, lumped)


# ---- 2. an axis is the axis it says -----------------------------------------------------------------------------------------------------
_ISO_RUNS = {}


def _iso_run(lib, axis, eps, kappa):
    key = (axis, eps, kappa)
    if key not in _ISO_RUNS:
        _ISO_RUNS[key] = ac.invariant_run(lib, axis, eps, kappa)[:2]
    return _ISO_RUNS[key]


@pytest.mark.parametrize("axis,kappa", [(0, ac.INVARIANT_KAPPA), (1, ac.INVARIANT_KAPPA), (2, ac.INVARIANT_KAPPA),
                                        (2, (0.0, 0.0, 0.11)), (2, (0.02, 0.05, 0.0))],
                         ids=["x", "y", "z", "z-kappa-on-z-only", "z-kappa-off-z-only"])
def test_scene_invariant_along_an_axis_sees_that_axis_only(oracle_lib, axis, kappa):
    eps = ac.INVARIANT_EPS
    assert len(set(eps)) == 3 and (len(set(kappa)) == 3 or sorted(kappa)[1] == 0.0)
    a1, a2 = (axis + 1) % 3, (axis + 2) % 3
    probe_i, fields_i = _iso_run(oracle_lib, axis, eps[axis], kappa[axis])
    # the precondition, on the isotropic run: the two transverse E components are exactly zero (else the SCENE is wrong)
    assert not fields_i[0][a1].any() and not fields_i[0][a2].any() and not fields_i[1][axis].any()
    assert np.abs(fields_i[0][axis]).max() > 1e-3 and np.abs(probe_i).max() > 1e-3
    probe_a, fields_a, sim = ac.invariant_run(oracle_lib, axis, eps, kappa)
    assert sim.anisotropic and sim.operator_build == "host"          # the oracle has no fdtd_build_operator_axes
    assert np.array_equal(probe_a, probe_i) and np.array_equal(fields_a, fields_i)
    # ... and it is a test: the isotropic run of another axis' values is a different run
    probe_w, _ = _iso_run(oracle_lib, axis, eps[a1], kappa[a1])
    assert not np.array_equal(probe_w, probe_i)


# ---- 3. bounds ----------------------------------------------------------------------------------------------------------------------
def test_uniaxial_cavity_resonance_lies_between_the_isotropic_ones(oracle_lib):
    """The frequencies of a lossless system fall when any edge capacitance grows: eps = (2, 2, 4) lies between eps = 2 and eps = 4
    edge by edge, so its lowest resonance lies between theirs.  profiles/anisotropic/kat.txt records the three."""
    f4, df = ac.cavity_lowest_resonance(oracle_lib, 4.0)
    f2, _ = ac.cavity_lowest_resonance(oracle_lib, 2.0)
    fu, _ = ac.cavity_lowest_resonance(oracle_lib, (2.0, 2.0, 4.0))
    print(f"lowest resonance: eps 4: {f4 / 1e9:.4f} GHz, eps (2, 2, 4): {fu / 1e9:.4f} GHz, eps 2: {f2 / 1e9:.4f} GHz, bin {df / 1e6:.2f} MHz")
    assert f2 - f4 >= 10 * df
    assert f4 <= fu <= f2


# ---- 4. API and voxelisation ------------------------------------------------------------------------------------------------------------
def test_scene_spellings_and_refusals():
    sc = pkg("scene")
    s = sc.Scene()
    iso = s.add_material("fr4", 4.3, 1e-3)
    assert isinstance(iso.eps_r, float) and iso.eps_axes is None and iso.kappa_axes is None and not iso.anisotropic
    assert iso.axes() == ((4.3,) * 3, (1e-3,) * 3)
    m = s.add_material("ro3010", eps_r=[12.5, 12.5, 10.2], kappa=(1e-3, 2e-3, 3e-3))
    assert m.anisotropic and m.eps_axes == (12.5, 12.5, 10.2) and m.kappa_axes == (1e-3, 2e-3, 3e-3)
    assert isinstance(m.eps_r, float) and m.eps_r == pytest.approx(35.2 / 3) and m.kappa == pytest.approx(2e-3)
    e_only = s.add_material("sapphire", np.array([9.4, 9.4, 11.6]))
    assert e_only.anisotropic and e_only.kappa_axes is None and e_only.kappa == 0.0 and e_only.axes()[1] == (0.0, 0.0, 0.0)
    same = s.add_material("same", [3.0, 3.0, 3.0], [0.1, 0.1, 0.1])
    assert not same.anisotropic and same.eps_r == 3.0 and same.kappa == 0.1
    for kw, msg in ((dict(eps_r=[1.0, 2.0]), "must be one value or three"), (dict(eps_r=[1.0, 2.0, 3.0, 4.0]), "must be one value or three"),
                    (dict(eps_r=[[1.0, 2.0, 3.0]]), "must be one value or three"), (dict(eps_r=[1.0, float("nan"), 2.0]), "finite and > 0"),
                    (dict(eps_r=[1.0, 0.0, 2.0]), "finite and > 0"), (dict(kappa=[0.0, float("inf"), 0.0]), "finite and >= 0"),
                    (dict(kappa=[0.0, -1.0, 0.0]), "finite and >= 0"), (dict(kappa=["a", "b", "c"]), "must be one value or three")):
        with pytest.raises(ValueError, match=f"material 'bad'.*{msg}"):
            s.add_material("bad", **kw)
    # dispersive media are isotropic; magnetic sequences stay refused as before
    with pytest.raises(ValueError, match="Debye material 'wet'.*eps_inf.*must be one value"):
        s.add_debye_material("wet", [4.0, 4.0, 5.0], 0.0, [2.0], [8e-12])
    with pytest.raises(ValueError, match="Debye material 'wet'.*kappa.*must be one value"):
        s.add_debye_material("wet", 4.0, [0.0, 0.0, 0.1], [2.0], [8e-12])
    with pytest.raises(ValueError, match="Lorentz material 'res'.*eps_inf.*must be one value"):
        s.add_lorentz_material("res", [2.0, 2.0, 3.0], 0.0, wp=[2e10], w0=[4e10], gamma=[1e9])
    with pytest.raises(ValueError, match="Lorentz material 'res'.*kappa.*must be one value"):
        s.add_lorentz_material("res", 2.0, [0.0, 0.1, 0.0], wp=[2e10], w0=[4e10], gamma=[1e9])
    with pytest.raises(ValueError, match="ferrite"):
        s.add_material("ferrite", 1.0, 0.0, mu_r=[2.0, 2.0, 3.0])
    assert [q.name for q in s.materials] == ["fr4", "ro3010", "sapphire", "same"]


def _csx_fdtd():
    api = pkg("openems_api")
    fd = api.openEMS(NrTS=10)
    fd.SetGaussExcite(2e9, 1e9)
    fd.SetBoundaryCond(["PEC"] * 6)
    csx = api.ContinuousStructure()
    fd.SetCSX(csx)
    g = csx.GetGrid()
    g.SetDeltaUnit(1e-3)
    for a, n in zip("xyz", (13, 11, 9)):
        g.AddLine(a, np.arange(n) * 2.0)
    return api, fd, csx


def test_csx_material_mirror_spellings_getters_and_log():
    api, fd, csx = _csx_fdtd()
    m = csx.AddMaterial("ro3010", epsilon=[12.5, 12.5, 10.2], kappa=[1e-3, 2e-3, 3e-3])
    assert isinstance(m, api.CSPropMaterial) and m.GetIsotropy() is False
    assert np.array_equal(m.GetMaterialProperty("epsilon"), [12.5, 12.5, 10.2]) and np.array_equal(m.GetMaterialProperty("kappa"), [1e-3, 2e-3, 3e-3])
    assert m.GetMaterialProperty("mue") == 1.0 and m.GetMaterialProperty("density") == 0.0
    m.AddBox([4, 4, 2], [20, 16, 8])
    iso = csx.AddMaterial("fr4", epsilon=4.3, kappa=1e-3)
    assert iso.GetIsotropy() is True and iso.GetMaterialProperty("epsilon") == 4.3
    iso.SetMaterialProperty(epsilon=[4.6, 4.6, 4.2])
    assert iso.GetIsotropy() is False and np.array_equal(iso.GetMaterialProperty("epsilon"), [4.6, 4.6, 4.2]) and iso.GetMaterialProperty("kappa") == 1e-3
    with pytest.raises(ValueError, match="material 'fr4'.*SetIsotropy\\(True\\).*differ"):
        iso.SetIsotropy(True)
    iso.SetMaterialProperty(epsilon=4.4)
    iso.SetIsotropy(True)
    assert iso.GetIsotropy() is True and iso.GetMaterialProperty("epsilon") == 4.4
    iso.AddBox([4, 4, 8], [20, 16, 12])
    with pytest.raises(ValueError, match="material 'bad'.*epsilon.*one value or three"):
        csx.AddMaterial("bad", epsilon=[1.0, 2.0])
    with pytest.raises(ValueError, match="material 'fr4'.*kappa.*one value or three"):
        iso.SetMaterialProperty(kappa=[0.0, float("nan"), 0.0])
    with pytest.raises(ValueError, match="unknown material property"):
        iso.GetMaterialProperty("colour")
    with pytest.raises(ValueError, match="AddDebyeMaterial 'wet'.*epsilon.*must be one value"):
        csx.AddDebyeMaterial("wet", epsilon=[4.0, 4.0, 5.0], eps_delta=[2.0], eps_relax_time=[8e-12])
    with pytest.raises(ValueError, match="AddLorentzMaterial 'res'.*kappa.*must be one value"):
        csx.AddLorentzMaterial("res", epsilon=2.0, kappa=[0.0, 0.1, 0.0], eps_plasma=[3e9])
    calls = csx._log.calls
    add = [c for c in calls if c["op"] == "AddMaterial"]
    assert add[0]["epsilon"] == [12.5, 12.5, 10.2] and add[0]["kappa"] == [1e-3, 2e-3, 3e-3] and add[1]["epsilon"] == 4.3
    setp = [c for c in calls if c["op"] == "SetMaterialProperty"]
    assert [c["prop"] for c in setp] == ["fr4", "fr4"] and setp[0]["epsilon"] == [4.6, 4.6, 4.2] and setp[1]["epsilon"] == 4.4
    assert [(c["prop"], c["val"]) for c in calls if c["op"] == "SetIsotropy"] == [("fr4", True)]
    # drawn: the scene holds the triple, the isotropic material its one value
    grid, scene = fd._build_scene()[:2]
    mats = {q.name: q for q in scene.materials}
    assert mats["ro3010"].eps_axes == (12.5, 12.5, 10.2) and mats["ro3010"].kappa_axes == (1e-3, 2e-3, 3e-3)
    assert not mats["fr4"].anisotropic and mats["fr4"].eps_r == 4.4
    vox = pkg("scene").voxelize(scene, grid)
    assert vox.eps_axes is not None and vox.anisotropic_names == ["ro3010"]


def _aniso_scene(curved):
    """An anisotropic solid (a box, or a cylinder along z: the owner path) with an isotropic box of higher priority cut into it, and an
    anisotropic box of equal priority drawn later over one corner (later wins ties)."""
    sc = pkg("scene")
    grid = pkg("grid").RectGrid(np.arange(17) * 1e-3, np.arange(15) * 1e-3, np.arange(11) * 1e-3)
    s = sc.Scene(unit=1e-3)
    a = s.add_material("uni", [2.0, 3.0, 4.0], [0.1, 0.2, 0.3])
    if curved:
        a.add_cylinder([8, 7, 1], [8, 7, 9], 5.0)
    else:
        a.add_box([2, 2, 1], [14, 12, 9])
    s.add_material("plug", 6.0, 0.5).add_box([6, 5, 3], [10, 9, 7], priority=3)
    s.add_material("late", [7.0, 8.0, 9.0]).add_box([7, 6, 1], [12, 10, 5])
    return grid, s


@pytest.mark.parametrize("curved", [False, True], ids=["box-path", "owner-path"])
def test_both_voxelisers_fill_the_axes_by_ownership(curved):
    sc, prims = pkg("scene"), pkg("primitives")
    grid, s = _aniso_scene(curved)
    assert prims.has_new(s) == curved
    vs = sc.voxelize(s, grid)
    nx, ny, nz = grid.shape
    assert vs.eps_axes.shape == vs.kappa_axes.shape == (3, nz - 1, ny - 1, nx - 1) and vs.anisotropic_names == ["uni", "late"]
    own = vs.cell_material
    table_e = np.array([[2.0, 3.0, 4.0], [6.0] * 3, [7.0, 8.0, 9.0], [1.0] * 3])
    table_k = np.array([[0.1, 0.2, 0.3], [0.5] * 3, [0.0] * 3, [0.0] * 3])
    for c in range(3):
        assert np.array_equal(vs.eps_axes[c], table_e[own, c]) and np.array_equal(vs.kappa_axes[c], table_k[own, c])
    for q in range(-1, 3):
        assert (own == q).any()
    # ownership: the plug (priority 3) holds its cells whole; the later box of equal priority took the corner it shares with 'uni'
    assert np.all(own[3:7, 5:9, 6:10] == 1) and own[2, 7, 11] == 2 and own[2, 6, 8] == 2 and own[6, 7, 5] == 0
    # the scalar view: the mean of the three in anisotropic cells, the value itself elsewhere
    assert np.array_equal(vs.eps_r[own == 0], np.full((own == 0).sum(), 3.0)) and np.all(vs.eps_r[own == 1] == 6.0) and np.all(vs.kappa[own == 2] == 0.0)
    assert vs.cell_eps() is vs.eps_axes and vs.cell_kappa() is vs.kappa_axes
    if curved:          # the owner path called directly gives the same arrays
        again = sc.voxelize_owners(s, grid)
        assert np.array_equal(again.eps_axes, vs.eps_axes) and np.array_equal(again.kappa_axes, vs.kappa_axes)
        assert (own[5] == 0).sum() not in (0, own[5].size)


def test_existing_scene_builders_stay_isotropic():
    """No anisotropic material, nothing new: eps_axes / kappa_axes are None for every scene builder of tests/helpers.py."""
    builders = [f for name, f in inspect.getmembers(helpers, inspect.isfunction) if name.endswith("_sim")]
    assert builders and helpers.patch_sim in builders
    for f in builders:
        sim = f(40, 36, 24)
        assert sim.vox.eps_axes is None and sim.vox.kappa_axes is None and sim.vox.anisotropic_names is None
        assert not sim.anisotropic and sim.eps_cells is sim.vox.eps_r and sim.kappa_cells is sim.vox.kappa and sim.anisotropic_info() is None
    sc = pkg("scene")
    from test_sar_model_cpu import block_scene
    grid, s = block_scene()
    assert sc.voxelize(s, grid).eps_axes is None


def test_simulation_takes_the_axes_everywhere_and_refuses_what_it_cannot_do(oracle_lib):
    sc, sim, eco = pkg("scene"), pkg("simulation"), pkg("ecoperator")
    from test_sar_model_cpu import block_scene
    kap3, eps3 = (0.8, 1.2, 2.0), (18.0, 20.0, 26.0)
    grid, s = block_scene(kappa=kap3)
    s.materials[0].eps_axes, s.materials[0].eps_r = eps3, sum(eps3) / 3
    # a Debye cap on the block: its fold goes to all three axes of its own cells
    s.add_debye_material("wet", 4.0, 0.0, [2.0], [8e-12], density=900.0).add_box((12, 10, 18), (32, 28, 22), priority=2)
    vox = sc.voxelize(s, grid)
    m = sim.Simulation(grid, vox, f0=2e9, fc=1e9, boundary="PEC", nr_ts=50, nf2ff_mode="record")
    assert m.anisotropic and m.kappa_cells.shape == vox.kappa_axes.shape and m.kappa_cells is not vox.kappa_axes
    wet = m.debye.cell_medium == 0
    fold = m.debye.media[0].folded(m.dt)[1]
    assert wet.any() and fold > 0 and np.all(m.kappa_cells[:, wet] == fold) and np.array_equal(m.kappa_cells[:, ~wet], vox.kappa_axes[:, ~wet])
    # the edge conductivities of the J dumps: component c averages kappa[c]
    for c, k in enumerate(m.edge_conductivity()):
        assert np.array_equal(k, eco._edge_average(m.kappa_cells[c], grid, c))
        assert not np.array_equal(k, eco._edge_average(m.kappa_cells[(c + 1) % 3], grid, c))
    # the host operator and the overrides (the port's resistor edge lies in vacuum; its m comes from the same call)
    op = m.op
    for c in range(3):
        iso = eco.build_operator(grid, vox.eps_axes[c], m.kappa_cells[c], vox.pec, m.dt, vox.lumped)
        assert same_bits(op.vv[c], iso.vv[c]) and same_bits(op.m[c], iso.m[c])
    from restatement import corrections_hidden
    with corrections_hidden(m):          # the oracle steps no Debye branch; the folded operator is what is compared
        e = m.build(oracle_lib)
    assert m.operator_build == "host" and all(same_bits(a, b) for a, b in zip(e.get_operator(), op.raw()))
    info = m.anisotropic_info()
    assert info["materials"] == ["tissue"] and info["cells"] == int((vox.cell_material == 0).sum()) and info["operator_build"] == "host"
    # SAR takes one conductivity per cell
    with pytest.raises(ValueError, match="SAR box 'b'.*material 'tissue'.*kappa is anisotropic"):
        m2 = sim.Simulation(grid, vox, f0=2e9, fc=1e9, boundary="PEC", nr_ts=50, nf2ff_mode="record")
        m2.add_sar_box("b", (12e-3, 10e-3, 8e-3), (32e-3, 28e-3, 16e-3), [2e9], 1e-3)
    # ... anisotropic eps alone is fine
    grid, s = block_scene()
    s.materials[0].eps_axes, s.materials[0].eps_r = eps3, sum(eps3) / 3
    m3 = sim.Simulation(grid, sc.voxelize(s, grid), f0=2e9, fc=1e9, boundary="PEC", nr_ts=50, nf2ff_mode="record")
    m3.add_sar_box("b", (12e-3, 10e-3, 8e-3), (32e-3, 28e-3, 16e-3), [2e9], 1e-3)
    assert m3.anisotropic and "b" in m3.sar_boxes


def test_plane_wave_vacuum_check_looks_at_all_three_axes():
    sc, sim = pkg("scene"), pkg("simulation")
    grid = pkg("grid").RectGrid(*[np.arange(n) * 1e-3 for n in (26, 24, 22)])

    def make(eps, kappa=0.0):
        s = sc.Scene(unit=1e-3)
        s.add_material("slab", eps, kappa).add_box([3, 3, 3], [22, 20, 9])      # crosses the surface of the plane-wave box
        s.add_plane_wave("pw", [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]).add_box([7, 7, 7], [18, 16, 14])
        return sim.Simulation(grid, sc.voxelize(s, grid), f0=6e9, fc=4e9, boundary="CPML", cpml_cells=4, nr_ts=100)
    # the mean of (0.5, 1.0, 1.5) is the vacuum's 1.0: the scalar view would let it pass
    with pytest.raises(ValueError, match="plane wave 'pw'.*eps_r = 0.5.*must be vacuum"):
        make([0.5, 1.0, 1.5])
    with pytest.raises(ValueError, match="plane wave 'pw'.*eps_r = 2.*must be vacuum"):
        make([1.0, 1.0, 2.0])
    with pytest.raises(ValueError, match="plane wave 'pw'.*kappa = 0.3.*must be vacuum"):
        make(1.0, [0.0, 0.3, 0.0])
