"""Voxel body models (discmaterial.py, Scene.add_disc_material, ContinuousStructure.AddDiscMaterial) without a GPU: the lookup rule and
the ownership rule of primitives.rasterise_spec on hand-computed and closed-form cases, validation, the .npz round trip, the API
mirror, and a phantom that repeats a scene of primitives — identical arrays, and identical runs on the oracle."""
import json

import numpy as np
import pytest

from conftest import pkg
import discmaterial_cases as dc
import polyhedron_cases as ph


def _spec(grid, scene):
    P = pkg("primitives")
    table = P.pack_table(scene, grid)
    return table, P.rasterise_spec(grid, table)


# ---- 1. the lookup rule and ownership ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bg", [False, True])
def test_hand_computed_map(bg):
    grid, s = dc.hand_map_scene(bg)
    table, (cown, eown, cvox) = _spec(grid, s)
    assert table.rec_map.tolist() == [1] and len(table.maps) == 1 and np.array_equal(table.maps[0].M, np.eye(4)[:3].reshape(12))
    assert cown.dtype == cvox.dtype == np.int32 and cown.shape == cvox.shape == (3, 5, 6) and eown.max() == -1
    want_vox = dc.HAND_VOXEL_BG if bg else dc.HAND_VOXEL
    for k in range(3):
        assert np.array_equal(cvox[k], want_vox if k == 1 else np.full((5, 6), -1)), k
        assert np.array_equal(cown[k], np.where(want_vox >= 0, 0, -1) if k == 1 else np.full((5, 6), -1)), k
    assert bg or np.array_equal(cown[1], dc.HAND_OWNER)
    # the centre x = 2.5 on the interior line belongs to the upper voxel (1), x = 5.5 on the last line to none
    assert cvox[1, 2, 2] == 3 + 1 and cvox[1, 2, 1] == 3 and (cvox[1, :, 5] == -1).all()
    vox = pkg("scene").voxelize(s, grid)
    data = np.array([1, 0, 2, 2, 1, 0])
    sel = want_vox >= 0
    for arr, tab, bgv in ((vox.eps_r, [1.5, 30.0, 50.0], 1.0), (vox.kappa, [0.01, 0.5, 1.5], 0.0), (vox.density, [5.0, 1000.0, 1100.0], 0.0)):
        want = np.full((5, 6), bgv)
        want[sel] = np.array(tab)[data[want_vox[sel]]]
        assert np.array_equal(arr[1], want) and np.all(arr[0] == bgv) and np.all(arr[2] == bgv)
    assert np.array_equal(vox.cell_voxel, cvox) and np.array_equal(vox.cell_material >= 0, cvox >= 0)
    assert (vox.eps_r == 1.5).sum() == (4 if bg else 0)                     # table entry 0 only with use_db_background


def test_lookup_rule_half_open_and_nan():
    D = pkg("discmaterial")
    L = (np.array([0.0, 1.0, 3.0]), np.array([-1.0, 1.0]), np.array([0.0, 0.5, 1.0, 2.0]))
    data = np.arange(1, 7, dtype=np.uint8).reshape(3, 1, 2)
    M = np.eye(4)[:3].reshape(12)
    x = np.array([0.0, 1.0, 2.999, 3.0, -1e-300, np.nan, 0.5, 0.5, 0.5])
    y = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 1.0, np.nan])
    z = np.full(9, 0.5)
    held, lin = D.lookup_spec(M, L, data, False, x, y, z)
    assert lin.tolist() == [2, 3, 3, -1, -1, -1, 2, -1, -1] and np.array_equal(held, lin >= 0)
    data[1, 0, 0] = 0
    held, lin = D.lookup_spec(M, L, data, False, x, y, z)
    assert lin[0] == 2 and not held[0] and held[1]
    assert D.lookup_spec(M, L, data, True, x, y, z)[0][0]


def _slab_scene(with_box, bg):
    grid = ph.grid_of(np.arange(9.0), np.arange(8.0), np.arange(7.0))
    s = pkg("scene").Scene(unit=1.0)
    if with_box:
        s.add_material("under", 3.0, 0.2, density=10.0).add_box((0.0, 0.0, 0.0), (4.0, 7.0, 6.0), priority=-1)
    data = np.ones((4, 5, 6), np.uint8)
    data[:, :, 2:4] = 0                                                        # a transparent slot over x in [3, 5]
    dm = s.add_disc_material("phantom", (np.arange(7.0) + 1.0, np.arange(6.0) + 1.0, np.arange(5.0) + 1.0), data, [2.5, 40.0], [0.05, 1.0],
                             [20.0, 1000.0], use_db_background=bg)
    dm.add_box((0.0, 0.0, 0.0), (8.0, 7.0, 6.0))
    return grid, s


def test_index_zero_is_transparent_unless_use_db_background():
    sc = pkg("scene")
    grid, s = _slab_scene(True, False)
    vox = sc.voxelize(s, grid)
    slot = np.zeros(vox.eps_r.shape, bool)
    slot[1:5, 1:6, 3:5] = True                                                 # the cells of the zero voxels
    body = np.zeros_like(slot)
    body[1:5, 1:6, 1:7] = True
    body &= ~slot
    assert np.all(vox.eps_r[body] == 40.0) and np.all(vox.density[body] == 1000.0) and np.all(vox.cell_voxel[body] >= 0)
    under = slot & (np.arange(8)[None, None, :] < 4)                           # x < 4: the lower-priority box shows through
    assert under.sum() == 20 and np.all(vox.eps_r[under] == 3.0) and np.all(vox.cell_material[under] == 0) and np.all(vox.cell_voxel[under] == -1)
    air = slot & ~under                                                        # nothing under it: the scene's background
    assert air.sum() == 20 and np.all(vox.eps_r[air] == 1.0) and np.all(vox.cell_material[air] == -1) and np.all(vox.density[air] == 0.0)
    grid, s = _slab_scene(True, True)
    bgv = sc.voxelize(s, grid)
    assert np.all(bgv.eps_r[slot] == 2.5) and np.all(bgv.kappa[slot] == 0.05) and np.all(bgv.density[slot] == 20.0)
    assert np.all(bgv.cell_material[slot] == 1) and np.all(bgv.cell_voxel[slot] >= 0)
    assert np.array_equal(bgv.eps_r[~slot], vox.eps_r[~slot])


@pytest.mark.parametrize("disc_first", [False, True])
def test_priority_and_ties(disc_first):
    """A higher-priority sphere wins inside the phantom; at equal priority the later record wins, in both drawing orders."""
    sc = pkg("scene")
    grid = ph.grid_of(np.arange(13.0), np.arange(12.0), np.arange(11.0))
    s = sc.Scene(unit=1.0)
    add_box = lambda: s.add_material("tie", 7.0).add_box((2.0, 2.0, 2.0), (6.0, 9.0, 8.0), priority=2)
    if not disc_first:
        add_box()
    dm = s.add_disc_material("phantom", ([1.0, 11.0], [1.0, 10.0], [1.0, 9.0]), np.ones((1, 1, 1), np.uint8), [1.0, 33.0], [0.0, 0.7], [0.0, 990.0])
    dm.add_box((0.0, 0.0, 0.0), (12.0, 11.0, 10.0), priority=2)
    if disc_first:
        add_box()
    s.add_material("ball", 9.0).add_sphere((8.0, 5.5, 5.0), 2.2, priority=4)
    vox = sc.voxelize(s, grid)
    assert vox.eps_r[5, 5, 8] == 9.0 and (vox.eps_r == 9.0).sum() > 20                 # the sphere, inside the phantom
    tie = vox.eps_r[2:8, 2:9, 2:6]
    assert np.all(tie == (7.0 if disc_first else 33.0))
    assert vox.eps_r[1, 1, 1] == 33.0 and vox.eps_r[0, 0, 0] == 1.0 and set(np.unique(vox.eps_r)) == {1.0, 7.0 if disc_first else 33.0, 33.0, 9.0}


def test_scene_without_maps_is_unchanged():
    P, sc = pkg("primitives"), pkg("scene")
    grid, s = dc.crowded_scene(with_disc=False)
    table = P.pack_table(s, grid)
    assert table.maps == [] and table.rec_map is None
    res = P.rasterise_spec(grid, table)
    assert isinstance(res, tuple) and len(res) == 2
    vox = sc.voxelize(s, grid)
    assert vox.cell_voxel is None
    # a box-only scene still takes the box path: the rasteriser is never asked
    w = pkg("workloads").patch_workload("t", nx=24, ny=20, nz=16)
    assert not P.has_new(w.scene)

    def never(grid, table):
        raise AssertionError("the box path asks no rasteriser")
    assert sc.voxelize(w.scene, w.grid, rasteriser=never).cell_voxel is None
    grid, s = dc.hand_map_scene()
    assert P.has_new(s)
    with pytest.raises(ValueError, match="cell_voxel"):
        sc.voxelize(s, grid, rasteriser=lambda g, t: P.rasterise_spec(g, t)[:2])


def test_other_solids_delimit_and_a_polyhedron_is_refused():
    P, sc = pkg("primitives"), pkg("scene")
    grid, s = dc.extremes_scene()
    table, (cown, _, cvox) = _spec(grid, s)
    assert table.rec["type"].tolist() == [P.T_BOX, P.T_CYLINDER] and table.rec_map.tolist() == [1, 2]
    full = s.materials[1].vmap
    assert (cown == 1).sum() > 50 and 255 in full.data.reshape(-1)[cvox[cown == 1]]
    one = cown == 0
    assert one.sum() > 100 and np.all(cvox[one] == 0)
    grid, s = dc.hand_map_scene()
    with pytest.raises(ValueError, match="polyhedron"):
        s.materials[0].add_polyhedron(ph.box_tris((1.0, 1.0, 1.0), (3.0, 3.0, 2.0)))
    s.materials[0].boxes.append(P.make("Polyhedron", 0, triangles=ph.box_tris((1.0, 1.0, 1.0), (3.0, 3.0, 2.0))))
    with pytest.raises(ValueError, match="phantom.*polyhedron"):
        P.pack_table(s, grid)


# ---- 2. validation ------------------------------------------------------------------------------------------------------------------
GOOD = dict(lines=([0.0, 1.0, 2.0], [0.0, 1.0], [0.0, 1.0]), data=np.array([[[0, 1]]], np.uint8), eps_r=[1.0, 4.0], kappa=[0.0, 0.1],
            density=[0.0, 1000.0])


@pytest.mark.parametrize("change, match", [
    (dict(lines=([0.0, 1.0, 2.0], [0.0, 1.0])), "three arrays"),
    (dict(lines=([0.0], [0.0, 1.0], [0.0, 1.0])), "lines X.*at least 2"),
    (dict(lines=([0.0, 2.0, 1.0], [0.0, 1.0], [0.0, 1.0])), "lines X.*strictly increasing"),
    (dict(lines=([0.0, 1.0, 2.0], [0.0, 0.0], [0.0, 1.0])), "lines Y.*strictly increasing"),
    (dict(lines=([0.0, 1.0, 2.0], [0.0, 1.0], [0.0, np.nan])), "lines Z"),
    (dict(data=np.zeros((1, 2, 1), np.uint8)), r"shape \(1, 2, 1\)"),
    (dict(data=np.array([[[0.0, 1.0]]])), "uint8"),
    (dict(data=np.array([[[0, 300]]])), "uint8"),
    (dict(data=np.array([[[0, 2]]], np.uint8)), "tissue index 2.*2 entries"),
    (dict(eps_r=[1.0, 0.5]), "eps_r.*>= 1"),
    (dict(eps_r=[1.0, np.inf]), "eps_r.*finite"),
    (dict(kappa=[0.0, -0.1]), "kappa.*>= 0"),
    (dict(density=[0.0, -1.0]), "density.*>= 0"),
    (dict(density=[0.0, np.nan]), "density.*finite"),
    (dict(kappa=[0.0]), "one length"),
    (dict(scale=0.0), "scale"),
    (dict(scale=np.nan), "scale"),
    (dict(matrix=np.zeros((4, 4))), "singular"),
    (dict(matrix=np.diag([1.0, 1.0, 0.0, 1.0])), "singular"),
    (dict(matrix=np.eye(3)), "4 x 4"),
    (dict(mue_r=[1.0, 2.0]), "mueR.*magnetic"),
    (dict(sigma=[0.0, 0.5]), "sigma.*magnetic"),
])
def test_validation_names_the_map_and_the_offending_thing(change, match):
    D = pkg("discmaterial")
    assert D.make_map("head", **GOOD).db_size == 2
    assert D.make_map("head", **GOOD, mue_r=[1.0, 1.0], sigma=[0.0, 0.0]).shape == (2, 1, 1)
    with pytest.raises(ValueError, match="'head'.*" + match):
        D.make_map("head", **{**GOOD, **change})


def test_too_many_voxels_and_too_many_maps():
    D, sc, P, api = pkg("discmaterial"), pkg("scene"), pkg("primitives"), pkg("openems_api")
    n = 1292                                                                  # 1291^3 > 2^31 - 1 >= 1290^3; the data is not looked at before
    big = np.arange(n, dtype=float)
    with pytest.raises(ValueError, match=r"'huge'.*1291 x 1291 x 1291 voxels.*2\^31 - 1"):
        D.make_map("huge", (big, big, big), np.zeros((1, 1, 1), np.uint8), [1.0], [0.0], [0.0])
    s = sc.Scene(unit=1.0)
    for q in range(D.MAX_MAPS):
        s.add_disc_material(f"m{q}", **GOOD)
    with pytest.raises(ValueError, match="'m4'.*at most 4"):
        s.add_disc_material("m4", **GOOD)
    s.materials.append(sc.DiscMaterial("m4", vmap=D.make_map("m4", **GOOD)))   # past the scene's own check: the table refuses it
    with pytest.raises(ValueError, match="'m4'.*at most 4"):
        P.pack_table(s, ph.uniform_grid(5, 5, 5))
    csx = api.ContinuousStructure()
    kw = dict(mesh_x=[0.0, 1.0, 2.0], mesh_y=[0.0, 1.0], mesh_z=[0.0, 1.0], DiscData=GOOD["data"], epsR=[1.0, 4.0], kappa=[0.0, 0.1], density=[0.0, 1e3])
    for q in range(D.MAX_MAPS):
        csx.AddDiscMaterial(f"m{q}", **kw)
    with pytest.raises(ValueError, match="'m4'.*at most 4"):
        csx.AddDiscMaterial("m4", **kw)


def test_npz_round_trip_and_refused_hdf5(tmp_path):
    D = pkg("discmaterial")
    grid, s = dc.two_maps_scene()
    vmap = s.materials[2].vmap
    D.save_npz(tmp_path / "upper.npz", vmap)
    with np.load(tmp_path / "upper.npz") as f:
        assert set(D.NPZ_KEYS) <= set(f.files) and f["DiscData"].dtype == np.uint8
    back = D.load_npz(tmp_path / "upper.npz", "upper", matrix=vmap.matrix)
    for a in range(3):
        assert np.array_equal(back.lines[a], vmap.lines[a])
    for key in ("data", "eps_r", "kappa", "density", "matrix"):
        assert np.array_equal(getattr(back, key), getattr(vmap, key)), key
    assert back.scale == 1.0 and back.use_db_background is False and back.name == "upper"
    for ext in (".h5", ".hdf5", ".H5"):
        with pytest.raises(ValueError, match="HDF5.*mesh_x, mesh_y, mesh_z, DiscData, epsR, kappa, density"):
            D.load_npz(tmp_path / ("head" + ext))
    np.savez(tmp_path / "partial.npz", mesh_x=[0.0, 1.0], DiscData=np.zeros((1, 1, 1), np.uint8))
    with pytest.raises(ValueError, match="partial.npz.*lacks mesh_y, mesh_z, epsR, kappa, density"):
        D.load_npz(tmp_path / "partial.npz")
    with pytest.raises(ValueError, match="cannot read"):
        D.load_npz(tmp_path / "absent.npz")
    np.savez(tmp_path / "magnetic.npz", mesh_x=[0.0, 1.0], mesh_y=[0.0, 1.0], mesh_z=[0.0, 1.0], DiscData=np.zeros((1, 1, 1), np.uint8),
             epsR=[2.0], kappa=[0.0], density=[1.0], mueR=[1.5], sigma=[0.0])
    with pytest.raises(ValueError, match="mueR.*magnetic tissue is out of scope"):
        D.load_npz(tmp_path / "magnetic.npz")


# ---- 3. the API mirror ---------------------------------------------------------------------------------------------------------------
def test_api_mirror_call_log_and_scene(tmp_path):
    D, api, sc = pkg("discmaterial"), pkg("openems_api"), pkg("scene")
    grid, s = dc.hand_map_scene()
    D.save_npz(tmp_path / "hand.npz", s.materials[0].vmap)
    csx = api.ContinuousStructure()
    g = csx.GetGrid()
    g.SetDeltaUnit(1.0)
    for a, n in zip("xyz", (7, 6, 4)):
        g.AddLine(a, np.arange(float(n)))
    prop = csx.AddDiscMaterial("phantom", filename=str(tmp_path / "hand.npz"), use_db_background=True)
    box = prop.AddBox([0, 0, 0], [6, 5, 3], priority=3)
    assert prop.GetName() == "phantom" and box.GetPriority() == 3
    assert csx._log.calls[-2:] == [
        {"op": "AddDiscMaterial", "name": "phantom", "filename": str(tmp_path / "hand.npz"), "scale": 1.0, "transform": None,
         "use_db_background": True, "voxels": [3, 2, 1], "db_size": 3},
        {"op": "AddBox", "prop": "phantom", "priority": 3, "start": [0, 0, 0], "stop": [6, 5, 3]}]
    box.AddTransform("Translate", [0.0, 0.0, 0.0])
    assert csx._log.calls[-1]["transforms"] == [["Translate", [0.0, 0.0, 0.0]]]
    json.dumps(csx._log.calls)
    fd = api.openEMS()
    fd.SetCSX(csx)
    g2, s2 = fd._build_scene()
    assert isinstance(s2.materials[0], sc.DiscMaterial) and s2.materials[0].boxes[0].priority == 3
    vox = sc.voxelize(s2, g2)
    assert np.array_equal(vox.cell_voxel[1], dc.HAND_VOXEL_BG)
    # a transform given as steps equals its matrix; the keyword form equals the file
    a = csx.AddDiscMaterial("steps", filename=str(tmp_path / "hand.npz"), scale=2.0, transform=[["RotateAxis", "z", 30.0], ["Translate", [1.0, 2.0, 3.0]]])
    M = np.eye(4)
    M[:3, 3] = (1.0, 2.0, 3.0)
    R = np.eye(4)
    c, sn = np.cos(np.deg2rad(30.0)), np.sin(np.deg2rad(30.0))
    R[:2, :2] = [[c, -sn], [sn, c]]
    assert np.allclose(a.vmap.matrix, M @ R, rtol=0, atol=1e-15) and a.vmap.scale == 2.0
    with pytest.raises(ValueError, match="HDF5"):
        csx.AddDiscMaterial("h5", filename="head.h5")
    with pytest.raises(ValueError, match="polyhedron"):
        prop.AddPolyhedronReader("x.stl")
    with pytest.raises(TypeError, match="mesh_x"):
        csx.AddDiscMaterial("nothing")
    assert not hasattr(api.CSProperty, "AddDiscMaterial")


# ---- 4. phantom equals primitives -----------------------------------------------------------------------------------------------------
def test_phantom_equals_primitives_arrays():
    sc = pkg("scene")
    grid = dc.phantom_grid()
    ref = sc.voxelize(dc.phantom_primitive_scene(), grid)
    assert set(np.unique(ref.cell_material)) == {-1, 0, 1, 2} and ref.cell_voxel is None
    vox = sc.voxelize(dc.phantom_disc_scene(ref), grid)
    for key in ("eps_r", "kappa", "density", "pec"):
        a, b = getattr(ref, key), getattr(vox, key)
        assert a.dtype == b.dtype and np.array_equal(a, b), key
    assert np.array_equal(vox.cell_voxel >= 0, ref.cell_material >= 0) and len(np.unique(vox.eps_r)) == 4


def test_phantom_equals_primitives_on_the_oracle(oracle_lib, tmp_path):
    api = pkg("openems_api")
    runs = []
    for disc in (False, True):
        fd, port = dc.phantom_script(api, oracle_lib, disc)
        fd.Run(str(tmp_path / f"run{int(disc)}"))
        u, i, _ = fd._port_series(1)
        runs.append((fd, u, i, fd.GetSAR("sar")))
    (f0, u0, i0, r0), (f1, u1, i1, r1) = runs
    assert len(u0) == 300 and np.abs(u0).max() > 0 and np.abs(i0).max() > 0
    assert np.array_equal(u0, u1) and np.array_equal(i0, i1)
    assert np.array_equal(f0.sim.engine.fields(), f1.sim.engine.fields())
    assert np.nanmax(r0.sar_local) > 0 and (r0.status == 0).sum() > 100
    for key in ("sar_local", "sar_avg", "status"):
        assert np.array_equal(getattr(r0, key), getattr(r1, key), equal_nan=key != "status"), key
    assert r0.mass == r1.mass and r0.P_abs == r1.P_abs
    # the run dump names the map: cells and mass per tissue index among the owned cells
    with open(tmp_path / "run1" / "fdtd_hip_run.json") as fh:
        dump = json.load(fh)["disc_materials"]["phantom"]
    vox = f1.sim.vox
    tissue = f1._csx.properties[0].vmap.data.reshape(-1)[vox.cell_voxel[vox.cell_voxel >= 0]]
    assert dump["cells_per_index"] == np.bincount(tissue, minlength=4).tolist() and dump["cells_per_index"][0] == 0
    assert dump["cells_owned"] == int((vox.cell_voxel >= 0).sum()) and dump["voxels"] == [13, 13, 12] and dump["db_size"] == 4
    vol = (2e-3) ** 3
    want = [0.0] + [rho * vol * n for (_, _, _, rho, _, _), n in zip(dc.PH_SPHERES, dump["cells_per_index"][1:])]
    assert np.allclose(dump["mass_kg_per_index"], want, rtol=1e-12, atol=0)
    with open(tmp_path / "run0" / "fdtd_hip_run.json") as fh:
        assert "disc_materials" not in json.load(fh)


# ---- 5. the binding -------------------------------------------------------------------------------------------------------------------
def test_binding_symbol_struct_and_default_rasteriser(oracle_lib, monkeypatch):
    """libfdtd_hip.so exports fdtd_voxelize_maps (outside the ABI list), the oracle does not and rasterises with the specification."""
    import ctypes
    capi = pkg("_capi")
    lib = capi.bind(ctypes.CDLL(capi.hip_library_path()))
    assert capi.has_discmaterial(lib) and not capi.has_discmaterial(oracle_lib)
    assert "fdtd_voxelize_maps" not in capi.ABI_SYMBOLS and ctypes.sizeof(capi.FdtdVoxelMap) == 152
    monkeypatch.delenv("FDTD_VOXELIZE", raising=False)
    assert capi.default_rasteriser(oracle_lib) is None and capi.default_rasteriser(lib) is not None
    monkeypatch.setenv("FDTD_VOXELIZE", "host")
    assert capi.default_rasteriser(lib) is None
    grid, s = dc.hand_map_scene()
    with pytest.raises(capi.FdtdError, match="fdtd_voxelize_maps"):
        capi.voxelize_maps_raw(oracle_lib, grid, pkg("primitives").pack_table(s, grid))
