"""csrc/voxel.hip on triangle meshes against its specification (primitives.rasterise_spec, conformal.fractions_spec): the same
integers and the same float64 bits, on meshes chosen for where the kernels can go wrong; and an STL-drawn patch end to end."""
import dataclasses

import numpy as np
import pytest

from conftest import pkg
import primitives_cases as pc
import polyhedron_cases as ph

pytestmark = pytest.mark.gpu

M30 = pc.rot(2, 30.0, (0.37, -0.21, 0.13))


def _both(hip_lib, grid, scene):
    P, capi = pkg("primitives"), pkg("_capi")
    table = P.pack_table(scene, grid)
    return table, P.rasterise_spec(grid, table), capi.voxelize_raw(hip_lib, grid, table)


def _same(spec, dev):
    for name, a, b in zip(("cell_owner", "edge_owner"), spec, dev):
        assert a.dtype == b.dtype == np.int32 and a.shape == b.shape, name
        assert np.array_equal(a, b), f"{name}: {int(np.count_nonzero(a != b))} of {a.size} owners differ, first at {np.argwhere(a != b)[0]}"


def _solids(grid, matrix=None):
    """The closed forms of the CPU tests in one scene, as materials and as metals: box, L and U prisms on mesh lines, an octahedron
    with its vertices on nodes, ten tetrahedra (half on the half-cell lattice); overlapping, at tied and at different priorities."""
    x, y, z = grid.x, grid.y, grid.z
    nx, ny, nz = len(x), len(y), len(z)
    fx, fy, fz = (lambda f: x[int(f * (nx - 1))]), (lambda f: y[int(f * (ny - 1))]), (lambda f: z[int(f * (nz - 1))])
    c, r = (fx(0.5), fy(0.5), fz(0.5)), min(fx(0.5) - x[1], fy(0.5) - y[1], fz(0.5) - z[1])
    meshes = [ph.box_tris((fx(0.2), fy(0.2), fz(0.3)), (fx(0.7), fy(0.75), fz(0.8))),
              ph.l_prism_tris((fx(0.15), fx(0.45), fx(0.8)), (fy(0.1), fy(0.4), fy(0.8)), (fz(0.25), fz(0.7))),
              ph.u_prism_tris((fx(0.1), fx(0.35), fx(0.6), fx(0.85)), (fy(0.15), fy(0.4), fy(0.85)), (fz(0.3), fz(0.75))),
              ph.shuffled_reversed(ph.octahedron_tris(c, r))]
    meshes += [ph.tetra_tris(v) for v in ph.tetra_cloud(grid, n=10)]
    solids = []
    for q, t in enumerate(meshes):
        for role in ("material", "metal"):
            solids.append((role, f"{role}{q}", q % 3, t, matrix if q % 2 == 0 else None))
    return ph.scene_of(*solids)


GRIDS = {
    "graded_19x17x15": lambda: ph.graded_grid(19, 17, 15),                    # node rows of 19, cell rows of 18: the narrow stores
    "ragged_131x11x5": lambda: ph.graded_grid(131, 11, 5, ext=(130.0, 10.0, 4.0)),   # crosses a tile in x (128) and in y (8 rows), ragged ends
    "rows_24x13x6": lambda: ph.graded_grid(24, 13, 6, ext=(23.0, 12.0, 5.0)),     # node rows of 24: int4 stores; cell rows of 23: narrow ones
    "rows_29x9x7": lambda: ph.uniform_grid(29, 9, 7),                         # cell rows of 28 with 28 * 8 * 6 a multiple of 4: int4 cell stores
}


@pytest.mark.parametrize("transformed", [False, True])
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_device_owners_equal_specification(hip_lib, name, transformed):
    grid = GRIDS[name]()
    table, spec, dev = _both(hip_lib, grid, _solids(grid, M30 if transformed else None))
    P = pkg("primitives")
    assert len(table.rec) == 28 and set(table.rec["type"]) == {P.T_POLYHEDRON} and table.rec["has_matrix"].sum() == (14 if transformed else 0)
    assert len(np.unique(spec[0])) > 3 and len(np.unique(spec[1])) > 3
    _same(spec, dev)


@pytest.mark.parametrize("ntetra", [63, 64, 65, 130])
def test_one_record_around_the_triangle_chunk(hip_lib, ntetra):
    """The polyhedron launch stages a record's triangles in chunks of 256 (one per thread): one record of 252, of 256 and of 260
    triangles (a triangle pair short of the chunk, the chunk, one pair beyond), and one of 520 (three chunks, the last ragged) — each
    a union of disjoint closed tetrahedra, as a material and as a metal."""
    grid = ph.graded_grid(23, 21, 9, ext=(10.5, 10.5, 4.6))
    tris = ph.disjoint_tetrahedra(2 * ntetra)
    assert tris.shape[0] == 4 * ntetra
    scene = ph.scene_of(("material", "foam", 0, tris, None), ("metal", "grit", 0, tris, None))
    table, spec, dev = _both(hip_lib, grid, scene)
    assert (spec[0] >= 0).sum() >= ntetra // 4 and (spec[1] >= 0).sum() >= ntetra // 4
    _same(spec, dev)


def test_fifty_mixed_records_cross_the_record_chunk(hip_lib):
    """all_types_scene's records of every analytic type, then polyhedra of both roles up to 50 records and beyond 48: the polyhedron
    launch merges into owners of earlier AND later records, at lower, equal and higher priorities."""
    P = pkg("primitives")
    ext = (36.0, 28.0, 22.0)
    grid = pc.grid_of(37, 29, 23)
    scene = pc.all_types_scene(grid, ext)
    rng = np.random.default_rng(5)
    mats, mets = scene.materials, scene.metals
    q = 0
    while len(P.pack_table(scene, grid).rec) < 50:
        c = np.array([rng.uniform(0.2, 0.8) * e for e in ext])
        tris = ph.icosphere_tris(c, rng.uniform(3.0, 7.0), 0) if q % 3 else ph.box_tris(c - 4.1, c + 3.7)
        (mats[q % len(mats)] if q % 2 else mets[q % len(mets)]).add_polyhedron(tris, priority=int(rng.integers(0, 13)))
        q += 1
    # a later analytic record at a tie, after the polyhedra in the table
    mats[0].add_sphere(tuple(0.5 * e for e in ext), 6.0, priority=2)
    mets[0].add_box((5.0, 5.0, 5.0), (25.0, 20.0, 15.0), priority=10)
    table, spec, dev = _both(hip_lib, grid, scene)
    types = table.rec["type"]
    assert len(table.rec) > 48 and (types == P.T_POLYHEDRON).sum() >= 20 and set(types) == set(range(P.N_TYPES)) | {P.T_POLYHEDRON}
    assert np.any(types[48:] == P.T_POLYHEDRON) and np.any(types[:48] == P.T_POLYHEDRON)
    poly = np.flatnonzero(types == P.T_POLYHEDRON)
    assert np.isin(spec[0], poly).sum() > 100 and np.isin(spec[1], poly).sum() > 100
    assert (~np.isin(spec[0], poly) & (spec[0] >= 0)).sum() > 100
    _same(spec, dev)


def test_outside_larger_and_refused_records(hip_lib):
    P, capi = pkg("primitives"), pkg("_capi")
    grid = ph.graded_grid(19, 17, 15)
    far = ph.box_tris((100.0, 100.0, 100.0), (110.0, 120.0, 130.0))
    scene = ph.scene_of(("material", "far", 0, far, None), ("metal", "farm", 0, far, None))
    table, spec, dev = _both(hip_lib, grid, scene)
    assert np.all(table.rec["cbox"][:, 3] < table.rec["cbox"][:, 0])
    _same(spec, dev)
    assert dev[0].max() == -1 and dev[1].max() == -1
    huge = ph.icosphere_tris((9.0, 8.0, 7.0), 60.0, 1)                  # the grid lies inside the solid
    scene = ph.scene_of(("material", "sea", 0, huge, None), ("metal", "block", 0, huge, M30))
    table, spec, dev = _both(hip_lib, grid, scene)
    _same(spec, dev)
    assert dev[0].min() == 0 and dev[1][0, :, :, :-1].min() == 1
    bad = P.pack_table(scene, grid)
    bad.rec["vert0"][1] += 9                                           # vert0 + 9 ntri runs past nvert
    with pytest.raises(capi.FdtdError, match="vertices"):
        capi.voxelize_raw(hip_lib, grid, bad)
    bad = P.pack_table(scene, grid)
    bad.rec["nvert"][0] -= 1                                           # no whole number of triangles
    with pytest.raises(capi.FdtdError, match="vertices"):
        capi.voxelize_raw(hip_lib, grid, bad)


def test_conformal_fractions_of_an_octahedron(hip_lib):
    """The bisection kernels take the polyhedron from the shared predicate: node_in and every f_e have the specification's bits."""
    C, capi = pkg("conformal"), pkg("_capi")
    grid = ph.uniform_grid(15, 15, 15)
    scene = ph.scene_of(("metal", "octa", 0, ph.octahedron_tris((0.0, 0.0, 0.0), 4.3), None),
                        ("metal", "tilted", 0, ph.octahedron_tris((1.0, -1.0, 0.5), 3.1), M30))
    table = C.plain_metal_table(scene, grid)
    node_in = C.node_inside(grid, table)
    comp, idx, flip = C.cut_edges(node_in)
    f = C.fractions_spec(grid, table, comp, idx, flip)
    assert idx.size > 200 and np.all((f > 0) & (f <= 1)) and np.count_nonzero(f < 1) > 200
    dn, dc, di, df = capi.fractions_raw(hip_lib, grid, table)
    assert np.array_equal(dn, node_in) and np.array_equal(dc, comp) and np.array_equal(di, idx)
    assert np.array_equal(df, f), int(np.count_nonzero(df != f))


def test_stl_patch_end_to_end(hip_lib, oracle_lib, tmp_path, monkeypatch):
    """The STL-drawn patch of the CPU test for 60 timesteps: HIP library with the device rasteriser, the oracle with the numpy one, and
    the HIP library with FDTD_VOXELIZE=host — the same VoxelScene arrays, every field value identical, the port series within the suite's bar for them (1e-12 relative)."""
    from helpers import rel_l2
    oe, capi = pkg("openems_api"), pkg("_capi")
    monkeypatch.delenv("FDTD_VOXELIZE", raising=False)
    runs = {}
    for key, lib, env in (("hip", hip_lib, None), ("oracle", oracle_lib, None), ("hip_host", hip_lib, "host")):
        if env:
            monkeypatch.setenv("FDTD_VOXELIZE", env)
            assert capi.default_rasteriser(hip_lib) is None
        else:
            assert (capi.default_rasteriser(lib) is not None) == (lib is hip_lib)
        (tmp_path / key).mkdir()
        FDTD, port, _ = ph.stl_patch_script(oe, tmp_path / key, lib=lib, nr_ts=60)
        FDTD.Run(str(tmp_path / key / "run"))
        runs[key] = (FDTD.sim.vox, FDTD.sim.engine.fields(), FDTD._port_series(1))
    vox, fields, (uo, io, _) = runs["oracle"]
    assert set(np.unique(vox.eps_r)) == {1.0, 3.38} and vox.pec.sum() > 500 and np.abs(fields).max() > 0 and len(uo) == 60
    for key in ("hip", "hip_host"):
        for f in dataclasses.fields(vox):
            a, b = getattr(vox, f.name), getattr(runs[key][0], f.name)
            if isinstance(a, np.ndarray):
                assert np.array_equal(a, b), (key, f.name)
        assert np.array_equal(runs[key][1], fields), key
        (u, i, _) = runs[key][2]
        assert np.abs(uo).max() > 0 and rel_l2(u, uo) < 1e-12 and rel_l2(i, io) < 1e-12, (key, rel_l2(u, uo), rel_l2(i, io))
