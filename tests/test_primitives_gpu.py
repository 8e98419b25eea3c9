"""csrc/voxel.hip against its specification (primitives.rasterise_spec): the owner arrays must be the same integers, on meshes chosen
for where the kernel can go wrong; and a coax-probe-fed circular patch end to end, device rasteriser + HIP engine against numpy
rasteriser + oracle."""
import dataclasses

import numpy as np
import pytest

from conftest import pkg
import primitives_cases as pc

pytestmark = pytest.mark.gpu


def _both(hip_lib, grid, scene, cells=True, edges=True):
    P, capi = pkg("primitives"), pkg("_capi")
    table = P.pack_table(scene, grid)
    return table, P.rasterise_spec(grid, table, cells=cells, edges=edges), capi.voxelize_raw(hip_lib, grid, table, cells=cells, edges=edges)


def _same(spec, dev):
    for name, a, b in zip(("cell_owner", "edge_owner"), spec, dev):
        assert a.dtype == b.dtype == np.int32 and a.shape == b.shape, name
        assert np.array_equal(a, b), f"{name}: {int(np.count_nonzero(a != b))} of {a.size} owners differ, first at {np.argwhere(a != b)[0]}"


CASES = {
    # x not a multiple of 4, rows shorter than a block's 128 points, graded
    "graded_37x29x23": lambda: (pc.grid_of(37, 29, 23), (36.0, 28.0, 22.0), None),
    # one cell layer, rows longer than one block's 128 points (two x tiles, the second nearly empty)
    "flat_130x9x2": lambda: (pc.grid_of(130, 9, 2, ext=(129.0, 8.0, 1.0)), (129.0, 8.0, 1.0), 5.3),
    # node rows of 24 (int4 stores) with cell rows of 23 (scalar stores)
    "rows_24x13x6": lambda: (pc.grid_of(24, 13, 6, ext=(23.0, 12.0, 5.0)), (23.0, 12.0, 5.0), None),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_owners_equal_specification(hip_lib, name):
    grid, ext, m = CASES[name]()
    table, spec, dev = _both(hip_lib, grid, pc.all_types_scene(grid, ext, m))
    assert len(np.unique(spec[0])) > 3 and len(np.unique(spec[1])) > 3      # the case draws something
    _same(spec, dev)


def test_every_type_near_surfaces_21cubed(hip_lib):
    """The 21^3 case: every type, ties, a primitive sticking out, one outside, a pin that misses every node.  The equality is
    unconditional; the two counts only guard against a comparison in which nothing was ever near a surface (or everything was)."""
    P = pkg("primitives")
    grid = pc.grid_of(21, 21, 21, ext=(20.0, 20.0, 20.0), grade=False)
    table, spec, dev = _both(hip_lib, grid, pc.on_surface_scene(grid))
    assert len(table.rec) >= 14 and set(table.rec["type"]) == set(range(P.N_TYPES))
    assert table.rec["has_matrix"].sum() >= 3
    outside = [q for q, r in enumerate(table.rec) if r["cbox"][3] < r["cbox"][0] and r["role"] == P.ROLE_MATERIAL]
    assert outside, "one primitive lies wholly outside the grid"
    thin = [q for q, n in enumerate(table.names) if n.startswith("thin_pin")]
    assert thin and not np.any(spec[1] == thin[0]), "the thin pin misses every node"
    _same(spec, dev)
    share, closed = pc.near_surface_share(grid, table)
    assert share <= 0.01, share
    assert closed >= 1


def test_table_longer_than_one_chunk(hip_lib):
    """320 small spheres: the table spans seven LDS chunks, most records miss most tiles, and the upper 40 % of y holds nothing."""
    ext = (39.0, 39.0, 23.0)
    grid = pc.grid_of(40, 40, 24, ext=ext)
    table, spec, dev = _both(hip_lib, grid, pc.sphere_lattice(grid, ext))
    assert len(table.rec) == 320 > 6 * 48
    assert spec[0][:, 30:, :].max() == -1 and spec[1][:, :, 30:, :].max() == -1 and (spec[0] >= 0).mean() > 0.05
    assert len(np.unique(spec[0])) > 100 and len(np.unique(spec[1])) > 100
    _same(spec, dev)


def test_single_passes_and_empty_table(hip_lib):
    P, sc = pkg("primitives"), pkg("scene")
    grid = pc.grid_of(37, 29, 23)
    scene = pc.all_types_scene(grid, (36.0, 28.0, 22.0))
    table, spec, dev = _both(hip_lib, grid, scene, edges=False)
    assert dev[1] is None and np.array_equal(spec[0], dev[0])
    table, spec, dev = _both(hip_lib, grid, scene, cells=False)
    assert dev[0] is None and np.array_equal(spec[1], dev[1])
    table, spec, dev = _both(hip_lib, grid, sc.Scene(unit=pc.UNIT))
    assert len(table.rec) == 0
    _same(spec, dev)
    assert dev[0].max() == -1 and dev[1].max() == -1
    # every primitive outside the grid: the kernels run and own nothing
    far = sc.Scene(unit=pc.UNIT)
    far.add_material("far", 2.0).add_sphere((500.0, 0.0, 0.0), 3.0)
    far.add_metal("farm").add_cylinder((-300.0, 0.0, 0.0), (-300.0, 0.0, 9.0), 3.0)
    table, spec, dev = _both(hip_lib, grid, far)
    _same(spec, dev)
    assert dev[0].max() == -1 and dev[1].max() == -1
    # a record the library must refuse: an unknown type, vertices outside the side array
    capi = pkg("_capi")
    bad = P.pack_table(scene, grid)
    bad.rec["type"][0] = 99
    with pytest.raises(capi.FdtdError, match="type 99"):
        capi.voxelize_raw(hip_lib, grid, bad)
    bad = P.pack_table(scene, grid)
    bad.rec["nvert"][bad.rec["type"] == P.T_WIRE] = 10 ** 6
    with pytest.raises(capi.FdtdError, match="vertices"):
        capi.voxelize_raw(hip_lib, grid, bad)


def test_probe_fed_circular_patch_end_to_end(hip_lib, oracle_lib, tmp_path, monkeypatch):
    """openEMS.Run on the HIP library with the device rasteriser against the oracle with the numpy rasteriser: identical VoxelScene
    arrays, port series within the suite's bar for port series (1e-12 relative), and the same again with FDTD_VOXELIZE=host."""
    from helpers import rel_l2
    oe, capi = pkg("openems_api"), pkg("_capi")
    monkeypatch.delenv("FDTD_VOXELIZE", raising=False)
    assert capi.default_rasteriser(hip_lib) is not None and capi.default_rasteriser(oracle_lib) is None
    runs = {}
    for key, lib, env in (("hip", hip_lib, None), ("oracle", oracle_lib, None), ("hip_host", hip_lib, "host")):
        if env:
            monkeypatch.setenv("FDTD_VOXELIZE", env)
            assert capi.default_rasteriser(hip_lib) is None
        FDTD, port = pc.probe_patch_script(oe, lib=lib)
        FDTD.Run(str(tmp_path / key))
        runs[key] = (FDTD.sim.vox, FDTD._port_series(1))
    vox = runs["oracle"][0]
    assert vox.eps_r.shape == (16, 24, 24) and set(np.unique(vox.eps_r)) == {1.0, 3.38}
    assert vox.pec[2, 7:9, 12, 14].all() and vox.pec[0, 9, 12, 7:17].all() and not vox.pec[2, 6, 12, 14]     # pin, patch, the port's gap
    for key in ("hip", "hip_host"):
        for f in dataclasses.fields(vox):
            a, b = getattr(vox, f.name), getattr(runs[key][0], f.name)
            if isinstance(a, np.ndarray):
                assert np.array_equal(a, b), (key, f.name)
        (u, i, _), (uo, io, _) = runs[key][1], runs["oracle"][1]
        assert len(uo) == 400 and np.abs(uo).max() > 0 and np.abs(io).max() > 0
        assert rel_l2(u, uo) < 1e-12 and rel_l2(i, io) < 1e-12, (key, rel_l2(u, uo), rel_l2(i, io))
