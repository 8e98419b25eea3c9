"""STL solids (primitives.Polyhedron, AddPolyhedronReader) on the specification: closed forms, ownership, the STL reader, the API."""
import dataclasses
import os

import numpy as np
import pytest

from conftest import pkg
import primitives_cases as pc
import polyhedron_cases as ph

M30 = pc.rot(2, 30.0, (0.37, -0.21, 0.13))        # about z by 30 degrees, then a translation
VARIANTS = ("plain", "shuffled_reversed", "transformed")


def _variant(tris, variant):
    """(triangles, matrix) of a variant of the same solid."""
    if variant == "shuffled_reversed":
        return ph.shuffled_reversed(tris), None
    return tris, (M30 if variant == "transformed" else None)


def _local(grid, cells, matrix):
    """The points the closed form is asked at: the grid's, through the inverse of `matrix` in the table's own arithmetic."""
    x, y, z = ph.points(grid, cells)
    if matrix is None:
        return x, y, z
    m = np.linalg.inv(matrix)[:3, :].reshape(12)
    return (((m[0] * x + m[1] * y) + m[2] * z) + m[3], ((m[4] * x + m[5] * y) + m[6] * z) + m[7], ((m[8] * x + m[9] * y) + m[10] * z) + m[11])


def _owners(grid, scene):
    P = pkg("primitives")
    return P.rasterise_spec(grid, P.pack_table(scene, grid))


# ---- closed forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("role", ["metal", "material"])
def test_box_mesh_owns_what_the_box_owns(role, variant):
    """Faces on mesh lines: a metal's nodes are decided by `near`, a material's centres by the crossings; no point is excluded."""
    grid = ph.graded_grid()
    lo, hi = (grid.x[4], grid.y[3], grid.z[5]), (grid.x[13], grid.y[12], grid.z[11])
    tris, M = _variant(ph.box_tris(lo, hi), variant)
    mesh = _owners(grid, ph.scene_of((role, "solid", 0, tris, M)))
    box = _owners(grid, ph.scene_of((role, "solid", 0, ("box", lo, hi), M)))
    which = 1 if role == "metal" else 0
    assert (box[which] >= 0).sum() > 100
    assert np.array_equal(mesh[0], box[0]) and np.array_equal(mesh[1], box[1])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", ["L", "U"])
@pytest.mark.parametrize("role", ["metal", "material"])
def test_concave_prisms_are_unions_of_boxes(role, shape, variant):
    """The L (two boxes) and the U (three; a ray along +x crosses its arms four times), faces on mesh lines, no point excluded."""
    grid = ph.graded_grid()
    x, y, z = grid.x, grid.y, grid.z
    if shape == "L":
        tris = ph.l_prism_tris((x[3], x[8], x[14]), (y[2], y[7], y[13]), (z[4], z[10]))
        boxes = [((x[3], y[2], z[4]), (x[14], y[7], z[10])), ((x[3], y[2], z[4]), (x[8], y[13], z[10]))]
    else:
        tris = ph.u_prism_tris((x[2], x[6], x[11], x[15]), (y[2], y[6], y[13]), (z[4], z[10]))
        boxes = [((x[2], y[2], z[4]), (x[15], y[6], z[10])), ((x[2], y[2], z[4]), (x[6], y[13], z[10])), ((x[11], y[2], z[4]), (x[15], y[13], z[10]))]
    tris, M = _variant(tris, variant)
    got = ph.held(grid, ph.scene_of((role, "solid", 0, tris, M)))
    want = np.zeros_like(got)
    for lo, hi in boxes:
        want |= ph.held(grid, ph.scene_of((role, "solid", 0, ("box", lo, hi), M)))
    assert want.sum() > 100 and np.array_equal(got, want), int(np.count_nonzero(got != want))


@pytest.mark.parametrize("variant", VARIANTS)
def test_octahedron_with_vertices_on_nodes(variant):
    """|x| + |y| + |z| <= r on the nodes (metal), < r on the cell centres (material): rays run through vertices, along edges and in
    faces.  On the integer mesh the closed form is exact, so no point is excluded; through the rotation the points within 1e-9 m of a
    face plane are, and they stay under 1 %."""
    grid = ph.uniform_grid(19, 17, 15)
    r = 5.0
    tris, M = _variant(ph.octahedron_tris((0.0, 0.0, 0.0), r), variant)
    for role, cells in (("metal", False), ("material", True)):
        got = ph.held(grid, ph.scene_of((role, "octa", 0, tris, M)))
        x, y, z = _local(grid, cells, M)
        d = (np.abs(x) + np.abs(y)) + np.abs(z)
        want = (d < r) if cells else (d <= r)
        excluded = np.abs(d - r) <= 1e-9 * np.sqrt(3.0) if M is not None else np.zeros(want.shape, bool)
        assert want.sum() > 50
        assert excluded.mean() < 0.01
        assert np.array_equal(got | excluded, want | excluded), (role, int(np.count_nonzero((got != want) & ~excluded)))
    if M is None:                                                 # the surface nodes are the metal's and not the material's
        nodes = ph.held(grid, ph.scene_of(("metal", "octa", 0, tris, None)))
        x, y, z = ph.points(grid, False)
        assert nodes[((np.abs(x) + np.abs(y)) + np.abs(z)) == r].all() and (((np.abs(x) + np.abs(y)) + np.abs(z)) == r).sum() >= 6 + 12 * 4


@pytest.mark.parametrize("variant", VARIANTS)
def test_forty_tetrahedra_match_the_orientation_test(variant):
    grid = ph.graded_grid(19, 17, 15)
    P = pkg("primitives")
    share = {0: [0, 0], 1: [0, 0]}
    for q, v in enumerate(ph.tetra_cloud(grid)):
        tris, M = _variant(ph.tetra_tris(v), variant)
        for role, cells in (("metal", False), ("material", True)):
            got = ph.held(grid, ph.scene_of((role, "t", 0, tris, M)))
            want, excluded = ph.tetra_closed_form(v, *_local(grid, cells, M), margin=1e-9)
            assert np.array_equal(got | excluded, want | excluded), (q, role, int(np.count_nonzero((got != want) & ~excluded)))
            share[q % 2][0] += int(excluded.sum())
            share[q % 2][1] += excluded.size
    assert share[1][1] > 0 and share[1][0] / share[1][1] < 0.01          # off-lattice vertices: nearly nothing is near a face
    if variant != "transformed":
        assert share[0][0] > 0                                            # on the half-cell lattice, points do lie in faces


# ---- priority and ownership -------------------------------------------------------------------------------------------------
def test_overlap_priority_and_later_wins():
    grid = ph.graded_grid()
    lo, hi = (grid.x[3], grid.y[3], grid.z[3]), (grid.x[10], grid.y[10], grid.z[10])
    lo2, hi2 = (grid.x[7], grid.y[6], grid.z[5]), (grid.x[15], grid.y[13], grid.z[12])
    mesh = ph.box_tris(lo2, hi2)
    for role, which in (("material", 0), ("metal", 1)):
        for first_mesh in (False, True):
            for pa, pb in ((0, 0), (3, 1), (1, 3)):
                a, b = (role, "a", pa, ("box", lo, hi), None), (role, "b", pb, mesh, None)
                order = (b, a) if first_mesh else (a, b)
                own = _owners(grid, ph.scene_of(*order))[which]
                only = [_owners(grid, ph.scene_of(s))[which] >= 0 for s in order]
                both = only[0] & only[1]
                assert both.sum() > 20
                prio = (order[0][2], order[1][2])
                winner = 1 if prio[1] >= prio[0] else 0                 # equal priority: the later one
                assert np.all(own[both] == winner), (role, first_mesh, pa, pb)
                assert np.all(own[only[0] & ~only[1]] == 0) and np.all(own[only[1] & ~only[0]] == 1)


# ---- the table ----------------------------------------------------------------------------------------------------------------
def test_table_record_and_refusals():
    P, sc = pkg("primitives"), pkg("scene")
    grid = ph.graded_grid()
    tris = ph.box_tris((1.0, 1.0, 1.0), (5.0, 6.0, 7.0))
    degenerate = np.array([[[1.0, 1.0, 1.0], [5.0, 1.0, 1.0], [3.0, 1.0, 1.0]]])      # zero area: dropped
    table = P.pack_table(ph.scene_of(("metal", "m", 4, np.concatenate([tris, degenerate]), None)), grid)
    r = table.rec[0]
    assert (r["type"], r["vert0"], r["nvert"], r["priority"]) == (P.T_POLYHEDRON, 0, 36, 4) and P.T_POLYHEDRON == 9 and P.N_TYPES == 9
    assert table.verts.size == 108 and np.array_equal(table.verts.reshape(12, 3, 3), tris) and not np.any(r["par"])
    assert isinstance(P.make("polyhedron", 2, triangles=tris), P.Polyhedron) and P.Polyhedron in P.NEW_TYPES
    with pytest.raises(ValueError, match="not closed: 3 open edges"):
        P.pack_table(ph.scene_of(("metal", "m", 0, tris[1:], None)), grid)
    with pytest.raises(ValueError, match="ntri x 3 x 3"):
        P.make("polyhedron", triangles=np.zeros((4, 3)))
    with pytest.raises(ValueError, match=f"at most {1 << 20}"):
        P._closed_triangles(np.tile(tris, ((1 << 20) // 12 + 1, 1, 1)), "'big'")
    s = sc.Scene(unit=1.0)
    with pytest.raises(ValueError, match="conducting sheet 'cu': a polyhedron is for materials and plain metals"):
        s.add_conducting_sheet("cu", 5.8e7, 35e-6).add_polyhedron(tris)


def test_scene_without_a_mesh_packs_the_parent_table():
    """No polyhedron drawn: the table is what the code without the polyhedron branch packs — rebuilt here record by record from the
    primitives themselves, with nothing of the new path reachable (no type 9, N_TYPES == 9)."""
    P = pkg("primitives")
    grid = pc.grid_of(21, 21, 21, ext=(20.0, 20.0, 20.0), grade=False)
    scene = pc.on_surface_scene(grid)
    assert not any(isinstance(p, P.Polyhedron) for prop in list(scene.materials) + list(scene.metals) for p in prop.boxes)
    table = P.pack_table(scene, grid)
    assert P.N_TYPES == 9 and P.T_POLYHEDRON not in set(table.rec["type"]) and set(table.rec["type"]) == set(range(P.N_TYPES))

    class NoPolyhedron:                                            # isinstance(x, Polyhedron) is False for everything
        pass
    saved, saved_closed = P.Polyhedron, P._closed_triangles
    P.Polyhedron = NoPolyhedron

    def unreachable(*a, **k):
        raise AssertionError("the polyhedron path ran")
    P._closed_triangles = unreachable
    try:
        without = P.pack_table(scene, grid)
    finally:
        P.Polyhedron, P._closed_triangles = saved, saved_closed
    assert table.rec.tobytes() == without.rec.tobytes() and table.verts.tobytes() == without.verts.tobytes()
    assert table.rec.dtype.itemsize == 248 and table.verts.size == 2 * (5 + 5 + 3 + 3) + 3 * 25      # the four polygons' and the wire's
    assert table.names == without.names and len(table.curves) == len(without.curves)


# ---- the STL reader -----------------------------------------------------------------------------------------------------------
def test_stl_binary_and_ascii_give_identical_tables(tmp_path):
    P, S = pkg("primitives"), pkg("stl")
    grid = ph.uniform_grid()
    tris = ph.icosphere_tris((0.25, -0.5, 0.125), 4.3, 1)
    S.write_stl(tmp_path / "b.stl", tris, binary=True)
    S.write_stl(tmp_path / "a.stl", tris, binary=False)
    assert os.path.getsize(tmp_path / "b.stl") == 84 + 50 * 80
    tb, ta = S.read_stl(tmp_path / "b.stl"), S.read_stl(str(tmp_path / "a.stl"))
    assert tb.shape == (80, 3, 3) and tb.dtype == np.float64 and np.array_equal(tb, tris.astype(np.float32).astype(np.float64))
    tables = [P.pack_table(ph.scene_of(("metal", "ball", 1, t, None)), grid) for t in (tb, ta)]
    assert tables[0].rec.tobytes() == tables[1].rec.tobytes() and tables[0].verts.tobytes() == tables[1].verts.tobytes()
    assert tables[0].rec["nvert"][0] == 240


def test_stl_reader_refusals(tmp_path):
    P, S = pkg("primitives"), pkg("stl")
    tris = ph.box_tris((0.0, 0.0, 0.0), (1.0, 2.0, 3.0))
    S.write_stl(tmp_path / "b.stl", tris, binary=True)
    S.write_stl(tmp_path / "a.stl", tris, binary=False)
    raw, text = (tmp_path / "b.stl").read_bytes(), (tmp_path / "a.stl").read_text()
    (tmp_path / "cut_b.stl").write_bytes(raw[:-7])
    (tmp_path / "cut_a.stl").write_text(text[:len(text) // 2])
    (tmp_path / "none_b.stl").write_bytes(raw[:80] + np.array([0], "<u4").tobytes())
    (tmp_path / "none_a.stl").write_text("solid empty\nendsolid empty\n")
    bad = bytearray(raw)
    bad[84 + 12:84 + 16] = np.array([np.nan], "<f4").tobytes()
    (tmp_path / "nan_b.stl").write_bytes(bytes(bad))
    (tmp_path / "nan_a.stl").write_text(text.replace("vertex 1.0 ", "vertex nan ", 1))
    for name, what in (("cut_b.stl", "truncated"), ("cut_a.stl", "truncated"), ("none_b.stl", "no facet"), ("none_a.stl", "no facet"),
                       ("nan_b.stl", "non-finite"), ("nan_a.stl", "non-finite"), ("missing.stl", "cannot be read")):
        with pytest.raises(ValueError, match=what):
            S.read_stl(tmp_path / name)
    S.write_stl(tmp_path / "open.stl", tris[:-1])
    with pytest.raises(ValueError, match="'hull': the polyhedron is not closed: 3 open edges"):
        P.pack_table(ph.scene_of(("metal", "hull", 0, S.read_stl(tmp_path / "open.stl"), None)), ph.uniform_grid())


# ---- the API ------------------------------------------------------------------------------------------------------------------
def test_add_polyhedron_reader_call_log_and_refusals(tmp_path):
    import importlib
    import sys
    from conftest import ROOT
    oe, S = pkg("openems_api"), pkg("stl")
    path = str(tmp_path / "box.stl")
    S.write_stl(path, ph.box_tris((-1.0, -2.0, 0.0), (1.0, 2.0, 3.0)))
    CSX = oe.ContinuousStructure()
    r = CSX.AddMetal("horn").AddPolyhedronReader(path, priority=7)
    r.AddTransform("Translate", [1.0, 0.0, 0.0])
    assert CSX._log.calls[-1] == {"op": "AddPolyhedronReader", "prop": "horn", "priority": 7, "filename": path,
                                  "transforms": [["Translate", [1.0, 0.0, 0.0]]]}
    assert r.GetFileName() == path and r.GetPriority() == 7 and r.ReadFile() is True
    lo, hi = r.bounding_box()
    assert np.array_equal(lo, [0.0, -2.0, 0.0]) and np.array_equal(hi, [2.0, 2.0, 3.0])
    r.SetFileName(str(tmp_path / "nowhere.stl"))
    assert r.GetFileName().endswith("nowhere.stl") and r.ReadFile() is False
    with pytest.raises(ValueError, match="AddPolyhedronReader: STL file .*nowhere.stl.*cannot be read"):
        r.to_scene()
    with pytest.raises(ValueError, match="AddPolyhedronReader on ConductingSheet 'cu'"):
        CSX.AddConductingSheet("cu", 5.8e7, 35e-6).AddPolyhedronReader(path)
    with pytest.raises(ValueError, match="AddPolyhedronReader on lumped element 'R1': lumped elements take boxes only"):
        CSX.AddLumpedElement("R1", "z", R=50.0).AddPolyhedronReader(path)
    with pytest.raises(ValueError, match="file_type 'PLY' is not supported"):
        CSX.AddMetal("m").AddPolyhedronReader(path, file_type="PLY")
    with pytest.raises(ValueError, match="only .stl is supported"):
        CSX.AddMetal("m1").AddPolyhedronReader(str(tmp_path / "horn.ply"))
    assert CSX.AddMetal("m2").AddPolyhedronReader(str(tmp_path / "horn.dat"), file_type="STL").GetFileName().endswith("horn.dat")
    for name in ("AddPolyhedron", "AddRotPoly", "AddMultiBox"):
        with pytest.raises(ValueError, match=name + " is not supported.*out of scope"):
            getattr(CSX.AddMetal("m3"), name)()
    sys.path.insert(0, os.path.join(ROOT, pkg().__name__.replace(".", os.sep), "compat"))
    try:
        csx_mod = importlib.import_module("CSXCAD")
    finally:
        sys.path.pop(0)
    assert csx_mod.CSPrimitives.CSPrimPolyhedronReader is oe.CSPrimPolyhedronReader
    assert hasattr(csx_mod.ContinuousStructure().AddMaterial("x"), "AddPolyhedronReader")


@pytest.mark.parametrize("binary", [True, False])
def test_stl_boxes_build_the_scene_of_the_boxes(oracle_lib, tmp_path, binary):
    oe = pkg("openems_api")
    vox = []
    for stl in (True, False):
        FDTD, port, readers = ph.stl_patch_script(oe, tmp_path, lib=oracle_lib, stl=stl, binary=binary)
        FDTD.Run(str(tmp_path / f"run{int(stl)}"), setup_only=True)
        vox.append(FDTD.sim.vox)
    assert set(np.unique(vox[1].eps_r)) == {1.0, 3.38} and vox[1].pec.sum() > 500
    for f in dataclasses.fields(vox[1]):
        a, b = getattr(vox[0], f.name), getattr(vox[1], f.name)
        if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
            assert np.array_equal(a, b), f.name


def test_thin_mesh_that_marks_no_edge_warns():
    sc = pkg("scene")
    grid = ph.uniform_grid()
    s = ph.scene_of(("metal", "sliver", 0, ph.box_tris((0.2, 0.2, 0.2), (0.7, 0.6, 0.8)), None))
    with pytest.warns(RuntimeWarning, match="metal 'sliver' marks no edge"):
        vs = sc.voxelize(s, grid)
    assert not vs.pec.any()
