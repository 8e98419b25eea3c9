"""fdtd_voxelize_maps (csrc/voxel.hip: k_voxel_map) against its specification (primitives.rasterise_spec with voxel maps): the same
owners and the same cell_voxel, integer for integer, on cases chosen for where the pass can go wrong; and a phantom that repeats a
scene of primitives through openEMS.Run on the HIP library."""
import numpy as np
import pytest

from conftest import pkg
import discmaterial_cases as dc
import polyhedron_cases as ph

pytestmark = pytest.mark.gpu


def _both(hip_lib, grid, scene):
    P, capi = pkg("primitives"), pkg("_capi")
    assert capi.has_discmaterial(hip_lib)
    table = P.pack_table(scene, grid)
    return table, P.rasterise_spec(grid, table), capi.voxelize_raw(hip_lib, grid, table)


def _same(spec, dev):
    assert len(spec) == len(dev) == 3
    for name, a, b in zip(("cell_owner", "edge_owner", "cell_voxel"), spec, dev):
        assert a.dtype == b.dtype == np.int32 and a.shape == b.shape, name
        assert np.array_equal(a, b), f"{name}: {int(np.count_nonzero(a != b))} of {a.size} differ, first at {np.argwhere(a != b)[0]}"


@pytest.mark.parametrize("bg", [False, True])
def test_tiles_placement_and_competitors(hip_lib, bg):
    """(a), (b): the crowded scene on 131 x 11 x 6 cells, without and with the database background."""
    grid, s = dc.crowded_scene(use_db_background=bg)
    assert tuple(n - 1 for n in grid.shape) == (131, 11, 6)
    table, spec, dev = _both(hip_lib, grid, s)
    cown, _, cvox = spec
    assert table.rec_map.tolist() == [0, 0, 0, 1, 1, 0] and table.rec["has_matrix"].tolist() == [0, 0, 0, 0, 1, 0]
    data = s.materials[3].vmap.data
    assert abs(float((data == 0).mean()) - 0.35) < 0.03
    disc = (cown == 3) | (cown == 4)
    assert np.array_equal(disc, cvox >= 0) and (cown == 3).sum() > 300 and (cown == 4).sum() > 300
    assert disc[:, 8:, 128:].any() and disc[:, :8, :128].any()                       # the partial tiles hold phantom cells too
    assert len(np.unique(cvox[disc])) > 400
    assert ((cown == 2).sum() > 20) and ((cown == 5).sum() > 300)                    # the ball (higher priority), the box drawn after
    assert bg or (cown == 1).sum() > 50                                              # the box drawn before: where the phantom is transparent
    assert (data.reshape(-1)[cvox[disc]] == 0).any() == bg
    if not bg:
        assert (cown == 0).sum() > 100 and (cown == -1).sum() > 100                 # the tetrahedron and the background show through
        nodisc = pkg("primitives").rasterise_spec(grid, pkg("primitives").pack_table(dc.crowded_scene(with_disc=False)[1], grid))[0]
        assert ((cown == 0) & (nodisc == 0)).sum() == (cown == 0).sum() and (nodisc == 0).sum() > (cown == 0).sum()
    _same(spec, dev)


def test_two_maps(hip_lib):
    """(c): two overlapping maps of different priority, the upper one transparent in places."""
    grid, s = dc.two_maps_scene()
    table, spec, dev = _both(hip_lib, grid, s)
    cown, _, cvox = spec
    assert table.rec_map.tolist() == [0, 1, 2] and len(table.maps) == 2
    up = s.materials[2]
    held_up = ph.held(grid, dc_only(s, 2), 0)                                        # the upper phantom's sphere alone
    assert (cown == 2).sum() > 500 and (cown == 1).sum() > 500 and (cown == 0).sum() > 100
    assert ((cown == 1) & held_up).sum() > 100                                       # the lower map shows through the upper one's zeros
    assert set(np.unique(up.vmap.data.reshape(-1)[cvox[cown == 2]])) <= set(range(1, 7))
    assert 0 in s.materials[1].vmap.data.reshape(-1)[cvox[cown == 1]]                # the lower map's background is owned
    _same(spec, dev)


def dc_only(s, q):
    """A scene of material q's primitives alone, as a plain material (the cells its delimiters hold, whatever the map says)."""
    sc = pkg("scene")
    out = sc.Scene(unit=s.unit)
    m = out.add_material("only", 2.0)
    m.boxes.extend(s.materials[q].boxes)
    return out


def test_centres_on_map_lines(hip_lib):
    """(d): map lines laid exactly on the grid's cell centres, and a map whose last line is a cell centre."""
    grid, s = dc.on_lines_scene()
    table, spec, dev = _both(hip_lib, grid, s)
    assert all(np.array_equal(mp.M, np.eye(4)[:3].reshape(12)) for mp in table.maps)
    cown, _, cvox = spec
    a = s.materials[0].vmap
    # the centre (1.5, 2.5, 1.5) is the map's first corner: voxel 0; the centre on the last line of an axis has none
    assert cvox[1, 2, 1] == (0 if a.data[0, 0, 0] else -1) and (cvox[:, :, 5] == -1).all() and (cvox[4] <= -1)[:, :7].all()
    want = np.full(cown.shape, -1)
    blk = np.where(a.data != 0, np.arange(a.data.size).reshape(a.data.shape), -1)
    want[1:4, 2:7, 1:5] = blk
    assert np.array_equal(cvox[:, :, :7], want[:, :, :7])
    assert (cown[:, :, 11] == -1).all() and (cown[:, :, 10] == 1).sum() > 20          # x = 11.5: the last line of the second map
    _same(spec, dev)


def test_map_outside_the_grid(hip_lib):
    """(e): a map that misses the grid owns nothing: the owners are fdtd_voxelize's for the scene without it, cell_voxel is -1."""
    P, capi = pkg("primitives"), pkg("_capi")
    grid, s = dc.crowded_scene(outside=True)
    table, spec, dev = _both(hip_lib, grid, s)
    _same(spec, dev)
    assert dev[2].max() == -1 and dev[2].min() == -1
    plain = capi.voxelize_raw(hip_lib, grid, P.pack_table(dc.crowded_scene(with_disc=False)[1], grid))
    assert len(plain) == 2
    remap = np.array([-1, 0, 1, 2, 5], np.int32)[plain[0] + 1]                        # its records 0, 1, 2, 3 are 0, 1, 2, 5 here
    assert np.array_equal(dev[0], remap) and np.array_equal(dev[1], plain[1])


def test_extremes(hip_lib):
    """(f): a one-voxel map, and a map holding index 255 with db_size 256."""
    grid, s = dc.extremes_scene()
    table, spec, dev = _both(hip_lib, grid, s)
    cown, _, cvox = spec
    assert (cown == 0).sum() > 100 and (cvox[cown == 0] == 0).all()
    assert 255 in s.materials[1].vmap.data.reshape(-1)[cvox[cown == 1]] and s.materials[1].vmap.db_size == 256
    _same(spec, dev)
    vox = pkg("scene").voxelize(s, grid, rasteriser=pkg("_capi").voxelize_device(hip_lib))
    ref = pkg("scene").voxelize(s, grid)
    for key in ("eps_r", "kappa", "density", "cell_voxel", "cell_material"):
        assert np.array_equal(getattr(vox, key), getattr(ref, key)), key


def test_no_maps_equals_fdtd_voxelize(hip_lib):
    """(g): the new entry point with no maps gives fdtd_voxelize's owners on the same table, and cell_voxel -1."""
    P, capi = pkg("primitives"), pkg("_capi")
    grid, s = dc.crowded_scene(with_disc=False)
    s.add_metal("lid").add_box((10.0, 1.0, 2.0), (100.0, 9.0, 5.5))
    table = P.pack_table(s, grid)
    assert not table.maps
    nx, ny, nz = grid.shape
    plain = capi.voxelize_raw(hip_lib, grid, table)
    dev = capi.voxelize_maps_raw(hip_lib, grid, table, 0, np.empty((nz - 1, ny - 1, nx - 1), np.int32), np.empty((3, nz, ny, nx), np.int32), force=True)
    assert (plain[0] >= 0).sum() > 500 and (plain[1] >= 0).sum() > 100
    assert np.array_equal(dev[0], plain[0]) and np.array_equal(dev[1], plain[1]) and (dev[2] == -1).all()


def test_refused_arguments(hip_lib):
    """What the entry point checks on the host, before any launch."""
    P, capi = pkg("primitives"), pkg("_capi")
    grid, s = dc.hand_map_scene()
    nx, ny, nz = grid.shape
    out = lambda: (np.empty((nz - 1, ny - 1, nx - 1), np.int32), np.empty((3, nz, ny, nx), np.int32))
    for what, match in (("rec_map", "refers to map"), ("lines", "do not increase"), ("data", "voxels"), ("metal", "delimits")):
        table = P.pack_table(s, grid)
        if what == "rec_map":
            table.rec_map[0] = 2
        elif what == "lines":
            table.maps[0].lines = (np.array([1.0, 4.0, 2.5, 5.5]),) + tuple(table.maps[0].lines[1:])
        elif what == "data":
            table.maps[0].data = table.maps[0].data[:-1].copy()
        else:
            table.rec["role"][0] = P.ROLE_METAL
        with pytest.raises(capi.FdtdError, match=match):
            capi.voxelize_maps_raw(hip_lib, grid, table, 0, *out())


def test_phantom_equals_primitives_through_run(hip_lib, tmp_path, monkeypatch):
    """The nested spheres and the map that repeats them, through openEMS.Run on the HIP library (device rasteriser, device SAR):
    identical fields, port series and SARResult."""
    api, capi = pkg("openems_api"), pkg("_capi")
    monkeypatch.delenv("FDTD_VOXELIZE", raising=False)
    monkeypatch.delenv("FDTD_SAR", raising=False)
    assert capi.default_rasteriser(hip_lib) is not None
    runs = []
    for disc in (False, True):
        fd, port = dc.phantom_script(api, hip_lib, disc)
        fd.Run(str(tmp_path / f"run{int(disc)}"))
        u, i, _ = fd._port_series(1)
        runs.append((fd, u, i, fd.GetSAR("sar"), fd.sim.engine.fields()))
    (f0, u0, i0, r0, e0), (f1, u1, i1, r1, e1) = runs
    assert f1.sim.vox.cell_voxel is not None and (f1.sim.vox.cell_voxel >= 0).sum() == (f0.sim.vox.cell_material >= 0).sum() > 500
    for key in ("eps_r", "kappa", "density"):
        assert np.array_equal(getattr(f0.sim.vox, key), getattr(f1.sim.vox, key)), key
    assert len(u0) == 300 and np.abs(u0).max() > 0 and np.abs(e0).max() > 0
    assert np.array_equal(e0, e1) and np.array_equal(u0, u1) and np.array_equal(i0, i1)
    assert np.nanmax(r0.sar_local) > 0 and (r0.status == 0).sum() > 100
    for key in ("sar_local", "sar_avg", "status"):
        assert np.array_equal(getattr(r0, key), getattr(r1, key), equal_nan=key != "status"), key
    assert f0.stats.sar["sar"]["device"] is True and f1.stats.sar["sar"]["device"] is True
