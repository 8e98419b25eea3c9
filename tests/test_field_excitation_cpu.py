"""Field excitations on the CPU (field_excitation.py): the list specification on a graded mesh, the weight evaluator, every refusal,
the refusals of the upstream spellings that stay, hard and soft E sources through the oracle, and the known-answer tests on the
oracle plus the numpy statement of include/fdtd_hip_excite.h (excite_cases.py); their records go to profiles/excite/kat.txt."""
import builtins
import json
import os

import numpy as np
import pytest

from conftest import ROOT, pkg
import excite_cases as xc

X = np.cumsum([0] + [1.0, 1.5, 0.5] * 4)           # 13 lines, graded
Y = np.cumsum([0] + [0.8, 1.2] * 5)                # 11
Z = np.cumsum([0] + [1.0, 0.6, 1.4, 1.0] * 3)      # 13
DT = 1e-12


def _grid():
    return pkg("grid").RectGrid(X * 1e-3, Y * 1e-3, Z * 1e-3)


def _lists(excs, pec=None, grid=None):
    fx, sc = pkg("field_excitation"), pkg("scene")
    g = _grid() if grid is None else grid
    pec = np.zeros((3,) + g.shape[::-1], bool) if pec is None else pec
    return fx.lists(g, excs, 1e-3, DT, pec, sc._tol(g)), g


def _entries(l, g):
    """{(comp, i, j, k): [amp, ...]} of one list, amplitudes in list order."""
    nx, ny, _ = g.shape
    out = {}
    for idx, c, a in zip(l[0].tolist(), l[1].tolist(), l[2].tolist()):
        out.setdefault((c, idx % nx, idx // nx % ny, idx // (nx * ny)), []).append(a)
    return out


# ---- the list specification -------------------------------------------------------------------------------------------------------
def test_volume_plane_line_and_point_boxes_on_a_graded_mesh():
    fx = pkg("field_excitation")
    g = _grid()
    f32 = lambda v: float(np.float32(v))
    # a volume of E edges: z edges whose midpoint lies in the box; x, y node coordinates, z the midpoint
    vol = fx.make("vol", 0, [0, 0, 2.0], [X[2], Y[3], Z[4]], [X[4], Y[5], Z[7]], weight=lambda x, y, z: x + 10 * y + 100 * z)
    l, _ = _lists([vol])
    got = _entries(l.soft_e, g)
    want = {(2, i, j, k): [f32(2.0 * (X[i] + 10 * Y[j] + 100 * 0.5 * (Z[k] + Z[k + 1])) * (Z[k + 1] - Z[k]) * 1e-3)]
            for i in (2, 3, 4) for j in (3, 4, 5) for k in (4, 5, 6)}
    assert got == want and l.info[0]["edges"] == 27 and l.info[0]["kind"] == "soft E"
    # a plane of H faces (type 2), normal z on the node plane Z[5]: z faces centred in the plane (x, y midpoints), and — exc_val has an
    # x component too — x faces whose centre (x node, y and z midpoints) lies in it: none, their z is a midpoint
    pl = fx.make("plane", 2, [0, 0, 3.0], [X[1], Y[1], Z[5]], [X[4], Y[3], Z[5]])
    l, _ = _lists([pl])
    got = _entries(l.soft_h, g)
    want = {(2, i, j, 5): [f32(3.0 * g.dd[2][5])] for i in (1, 2, 3) for j in (1, 2)}
    assert got == want and abs(g.dd[2][5] - 0.5 * (Z[6] - Z[4]) * 1e-3) < 1e-18
    # the same plane half a cell up catches the x and y faces (their centres sit on z midpoints) and no z face
    mid = 0.5 * (Z[5] + Z[6])
    l, _ = _lists([fx.make("plane2", 3, [1.0, 0, 5.0], [X[1], Y[1], mid], [X[4], Y[3], mid])])
    got = _entries(l.hard_h, g)
    assert got == {(0, i, j, 5): [f32(1.0 * g.dd[0][i])] for i in (1, 2, 3, 4) for j in (1, 2)} and l.soft_h[0].size == 0
    # a line of y edges along y, and a point that catches exactly one x edge by its midpoint
    ln = fx.make("line", 1, [0, -1.5, 0], [X[6], Y[2], Z[3]], [X[6], Y[7], Z[3]], weight=[None, "y^2", None], delay=3.4e-12)
    pt = fx.make("point", 0, [4.0, 0, 0], [0.5 * (X[7] + X[8]), Y[4], Z[9]], [0.5 * (X[7] + X[8]), Y[4], Z[9]], delay=3.6e-12)
    l, _ = _lists([ln, pt])
    assert _entries(l.hard_e, g) == {(1, 6, j, 3): [f32(-1.5 * (0.5 * (Y[j] + Y[j + 1])) ** 2 * (Y[j + 1] - Y[j]) * 1e-3)] for j in range(2, 7)}
    assert _entries(l.soft_e, g) == {(0, 7, 4, 9): [f32(4.0 * (X[8] - X[7]) * 1e-3)]}
    # the delay: round(delay / dt) timesteps
    assert set(l.hard_e[3].tolist()) == {3} and l.soft_e[3].tolist() == [4] and l.info[0]["delay_steps"] == 3 and l.info[1]["delay_steps"] == 4
    assert l.hard_e[2].dtype == np.float32 and l.hard_e[0].dtype == np.int64 and l.hard_e[1].dtype == np.int8 and l.hard_e[3].dtype == np.int32
    # one callable serves all three components; coordinates arrive in drawing units
    seen = []
    both = fx.make("both", 0, [1, 1, 0], [X[2], Y[2], Z[2]], [X[3], Y[3], Z[2]], weight=lambda x, y, z: seen.append((x.copy(), y.copy(), z.copy())) or 1.0)
    _lists([both])
    assert len(seen) == 2 and np.allclose(seen[0][0], [0.5 * (X[2] + X[3])] * 2) and np.allclose(sorted(seen[1][1]), [0.5 * (Y[2] + Y[3])] * 2)
    assert np.allclose(seen[0][2], Z[2])


def test_priority_and_scene_order():
    fx = pkg("field_excitation")
    g = _grid()
    a = fx.make("a", 0, [0, 0, 1.0], [X[2], Y[2], Z[2]], [X[5], Y[2], Z[3]], priority=0)
    b = fx.make("b", 0, [0, 0, 10.0], [X[4], Y[2], Z[2]], [X[7], Y[2], Z[3]], priority=2)
    c = fx.make("c", 0, [0, 0, 100.0], [X[6], Y[2], Z[2]], [X[8], Y[2], Z[3]], priority=2)
    l, _ = _lists([a, b, c])
    amp = {k: [round(v / ((Z[3] - Z[2]) * 1e-3)) for v in vals] for k, vals in _entries(l.soft_e, g).items()}
    # the higher priority owns an edge; equal priorities both act, in scene order
    assert amp == {(2, 2, 2, 2): [1], (2, 3, 2, 2): [1], (2, 4, 2, 2): [10], (2, 5, 2, 2): [10], (2, 6, 2, 2): [10, 100], (2, 7, 2, 2): [10, 100],
                   (2, 8, 2, 2): [100]}
    assert [q["edges"] for q in l.info] == [2, 4, 3]
    # E edges and H faces do not compete; a hard element is set once
    h = fx.make("h", 2, [0, 0, 1.0], [X[2], Y[2], Z[2]], [X[5], Y[4], Z[2]], priority=9)
    assert _lists([a, h])[0].soft_e[0].size == 4
    hard1 = fx.make("hard1", 1, [0, 0, 1.0], [X[2], Y[2], Z[2]], [X[3], Y[2], Z[3]])
    with pytest.raises(ValueError, match=r"field excitation 'hard1': its hard z edge at node \(2, 2, 2\) is also excited by 'a' with the same priority"):
        _lists([a, hard1])
    hard2 = fx.make("hard2", 1, [0, 0, 1.0], [X[2], Y[2], Z[2]], [X[3], Y[2], Z[3]], priority=1)
    l, _ = _lists([a, hard2])
    assert sorted(_entries(l.hard_e, g)) == [(2, 2, 2, 2), (2, 3, 2, 2)] and sorted(_entries(l.soft_e, g)) == [(2, 4, 2, 2), (2, 5, 2, 2)]


def test_dropped_metal_edges_and_empty_boxes():
    fx = pkg("field_excitation")
    g = _grid()
    pec = np.zeros((3,) + g.shape[::-1], bool)
    pec[2, 2, 2, 3] = pec[2, 2, 2, 4] = True
    soft = fx.make("soft", 0, [0, 0, 1.0], [X[2], Y[2], Z[2]], [X[5], Y[2], Z[3]])
    l, _ = _lists([soft], pec)
    assert sorted(_entries(l.soft_e, g)) == [(2, 2, 2, 2), (2, 5, 2, 2)] and l.dropped == [2] and l.info[0]["dropped_metal_edges"] == 2
    hard = fx.make("hard", 1, [0, 0, 1.0], [X[2], Y[2], Z[2]], [X[5], Y[2], Z[3]])
    with pytest.raises(ValueError, match=r"field excitation 'hard': its hard z edge at node \(3, 2, 2\) lies in metal \(PEC\)"):
        _lists([hard], pec)
    none = fx.make("none", 0, [0, 0, 1.0], [X[2] + 0.1, Y[2], Z[2]], [X[2] + 0.2, Y[2], Z[3]])
    with pytest.raises(ValueError, match=r"field excitation 'none': its box catches no edge of this mesh \(x: \[2.6, 2.7\] — nearest lines 2.5 and 2.5; y: .*z: \[1.6, 3\]"):
        _lists([none])
    with pytest.raises(ValueError, match="its box catches no face"):
        _lists([fx.make("nof", 2, [0, 0, 1.0], [X[2], Y[2], Z[2]], [X[5], Y[2], Z[2]])])       # (a line holds no z-face centre)
    for bad, msg in ((dict(exc_type=4), "exc_type must be 0"), (dict(exc_val=[0, 0, 0]), "at least one of them not zero"), (dict(delay=-1e-12), "delay = -1e-12"),
                     (dict(weight="x"), "a single string is ambiguous"), (dict(weight=["x", "y"]), "three per-component entries, got 2"),
                     (dict(weight=[1, 2, 3]), "weight entry 0 must be a callable or a string")):
        kw = dict(exc_type=0, exc_val=[0, 0, 1.0], start=[0, 0, 0], stop=[1, 1, 1])
        kw.update(bad)
        with pytest.raises(ValueError, match=msg):
            fx.make("bad", **kw)
    with pytest.raises(ValueError, match=r"field excitation 'inf': its weight function is not finite at \(1, 2, 2.3\)"):
        _lists([fx.make("inf", 0, [0, 0, 1.0], [X[1], Y[2], Z[2]], [X[1], Y[2], Z[3]], weight=[None, None, "1/(x-1)"])])


# ---- the refusals of the placement ------------------------------------------------------------------------------------------------
def _sim(add, excs, boundary="PEC", cpml_cells=None, n=(16, 14, 12), **kw):
    sc, sim, grid = pkg("scene"), pkg("simulation"), pkg("grid")
    g = grid.RectGrid(*[np.arange(k) * 1e-3 for k in n])
    s = sc.Scene(unit=1e-3)
    if add is not None:
        add(s)
    for e in excs:
        s.add_field_excitation(*e[:5], **(e[5] if len(e) > 5 else {}))
    return sim.Simulation(g, sc.voxelize(s, g), f0=10e9, fc=6e9, boundary=boundary, cpml_cells=cpml_cells, nr_ts=100, end_criteria=0.0, **kw)


def test_every_refusal_of_the_placement():
    hz = ("hz", 2, [0, 0, 1.0], [4, 4, 5], [7, 7, 5])
    # H faces: on a grid face, magnetic, plane-wave; anything inside a CPML layer; an H type on a decomposed run
    with pytest.raises(ValueError, match=r"field excitation 'edge': its x face at node \(0, 4, 4\) lies on a grid face"):
        _sim(None, [("edge", 3, [1.0, 0, 0], [0, 4, 4.5], [0, 6, 4.5])])
    with pytest.raises(ValueError, match=r"field excitation 'hz': its z face at node \(4, 4, 5\) is a magnetic face"):
        _sim(lambda s: s.add_material("ferrite", mu_r=2.0).add_box([3, 3, 4], [8, 8, 6]), [hz])
    with pytest.raises(ValueError, match=r"field excitation 'hz': its z face at node \(\d, \d, 5\) is a face of the plane wave's list"):
        _sim(lambda s: s.add_plane_wave("pw", (0, 1, 0), (0, 0, 1)).add_box([5, 5, 5], [11, 10, 8]), [hz])
    with pytest.raises(ValueError, match=r"field excitation 'hz': its z face at node \(4, 4, 5\) lies inside the CPML layer z- \(6 cells\)"):
        _sim(None, [hz], boundary=["PEC"] * 4 + ["CPML"] * 2, cpml_cells=6, n=(16, 14, 20))
    with pytest.raises(ValueError, match=r"field excitation 'se': its z edge at node \(4, 4, 15\) lies inside the CPML layer z\+ \(4 cells\)"):
        _sim(None, [("se", 0, [0, 0, 1.0], [4, 4, 15], [4, 4, 16])], boundary=["PEC"] * 4 + ["CPML"] * 2, cpml_cells=4, n=(16, 14, 20))
    s = _sim(None, [hz], n=(16, 14, 24))
    with pytest.raises(ValueError, match=r"field excitation 'hz': H-field excitations need a single slab \(world = 1\)"):
        s.build(None, world=2, rank=0)
    # hard E edges: a lumped port's edge, a lumped element, a sheet, a Debye, a Lorentz and a plane-wave edge
    he = ("he", 1, [0, 0, 1.0], [5, 5, 4], [5, 5, 6])
    cases = [(lambda s: s.add_lumped_port(1, 50.0, [5, 5, 4], [5, 5, 6], "z", 1.0), r"\(5, 5, 4\) is a source or resistor edge of lumped port 1"),
             (lambda s: s.add_lumped_element("load", "z", R=100.0, L=3e-9).add_box([5, 5, 4], [5, 5, 6]), r"\(5, 5, 4\) is an edge of a lumped element"),
             (lambda s: s.add_conducting_sheet("tin", 9.1e6, 5e-6).add_box([5, 3, 3], [5, 8, 8]), r"\(5, 5, 4\) is a conducting-sheet edge"),
             (lambda s: s.add_debye_material("d", 3.0, 0.0, [1.0], [1e-11]).add_box([3, 3, 3], [8, 8, 8]), r"\(5, 5, 4\) is a Debye edge"),
             (lambda s: s.add_lorentz_material("l", 3.0, 0.0, wp=[1e11], w0=[2e11], gamma=[1e10]).add_box([3, 3, 3], [8, 8, 8]), r"\(5, 5, 4\) is a Lorentz edge"),
             (lambda s: s.add_plane_wave("pw", (0, 0, 1), (1, 0, 0)).add_box([5, 3, 3], [10, 9, 8]), r"\(5, 5, 4\) is an edge of the plane wave's list")]
    for add, msg in cases:
        with pytest.raises(ValueError, match=r"field excitation 'he': its hard z edge at node " + msg):
            _sim(add, [he])
    # the same neighbours take a SOFT excitation on the same edges
    for add, _ in cases[:2]:
        assert _sim(add, [("se", 0, [0, 0, 1.0], [5, 5, 4], [5, 5, 6])]).excite_lists.soft_e[0].size == 2
    with pytest.raises(ValueError, match="field excitation 'hz' is defined twice"):
        _sim(None, [hz, hz])


def test_conformal_faces_are_refused():
    fx, grid = pkg("field_excitation"), pkg("grid")
    g = grid.RectGrid(*[np.arange(k) * 1e-3 for k in (10, 10, 10)])
    ex = [fx.make("hz", 3, [0, 0, 1.0], [4, 4, 5], [6, 6, 5])]
    l, _ = _lists(ex, grid=g)

    class Faces:
        idx, comp = np.array([g.flat(5, 4, 5)]), np.array([2], np.int8)
    with pytest.raises(ValueError, match=r"field excitation 'hz': its z face at node \(5, 4, 5\) is a conformal \(cut\) face"):
        fx.check_placement(g, ex, l, conformal=Faces)
    fx.check_placement(g, ex, l)


# ---- the weight evaluator ---------------------------------------------------------------------------------------------------------
EXPRESSIONS = [
    ("x", lambda x, y, z: x), ("-y", lambda x, y, z: -y), ("2.5", lambda x, y, z: 2.5 + 0 * x), ("x + y*z", lambda x, y, z: x + y * z),
    ("(x - y)/(z + 3)", lambda x, y, z: (x - y) / (z + 3)), ("x^2", lambda x, y, z: x ** 2), ("-x^2", lambda x, y, z: -x ** 2), ("2^-x", lambda x, y, z: 2.0 ** -x),
    ("x^2*y^3 + 1", lambda x, y, z: x ** 2 * y ** 3 + 1), ("rho", lambda x, y, z: np.hypot(x, y)), ("a", lambda x, y, z: np.arctan2(y, x)),
    ("r", lambda x, y, z: np.sqrt(x * x + y * y + z * z)), ("t", lambda x, y, z: np.arctan2(np.hypot(x, y), z)),
    ("sin(x)*cos(y) + tan(z/4)", lambda x, y, z: np.sin(x) * np.cos(y) + np.tan(z / 4)),
    ("asin(x/4) + acos(y/4) + atan(z)", lambda x, y, z: np.arcsin(x / 4) + np.arccos(y / 4) + np.arctan(z)),
    ("atan2(y, x)", lambda x, y, z: np.arctan2(y, x)), ("sinh(x) + cosh(y) + tanh(z)", lambda x, y, z: np.sinh(x) + np.cosh(y) + np.tanh(z)),
    ("exp(-rho^2)", lambda x, y, z: np.exp(-np.hypot(x, y) ** 2)), ("log(rho) + log10(r)", lambda x, y, z: np.log(np.hypot(x, y)) + np.log10(np.sqrt(x * x + y * y + z * z))),
    ("sqrt(abs(x))", lambda x, y, z: np.sqrt(np.abs(x))), ("min(x, y) + max(y, z)", lambda x, y, z: np.minimum(x, y) + np.maximum(y, z)),
    ("floor(x) + ceil(y)", lambda x, y, z: np.floor(x) + np.ceil(y)), ("pow(rho, 3)", lambda x, y, z: np.hypot(x, y) ** 3),
    ("if(x > 0, y, z)", lambda x, y, z: np.where(x > 0, y, z)), ("if(x>0 & y>1, 1, -1)", lambda x, y, z: np.where((x > 0) & (y > 1), 1.0, -1.0)),
    ("x > y", lambda x, y, z: (x > y) * 1.0), ("(x >= 0) + (y <= 1) + (z == 0) + (x != y) + (x < z)", lambda x, y, z: 1.0 * (x >= 0) + (y <= 1) + (z == 0) + (x != y) + (x < z)),
    ("x>0 | y>1.5", lambda x, y, z: ((x > 0) | (y > 1.5)) * 1.0), ("(x>0 && y>1) || z<0", lambda x, y, z: (((x > 0) & (y > 1)) | (z < 0)) * 1.0),
    ("pi*x + e", lambda x, y, z: np.pi * x + np.e), ("1e-3*x + 2.E2", lambda x, y, z: 1e-3 * x + 200.0),
    ("x/(x^2+y^2) * (rho>0.7) * (rho<2.5)", lambda x, y, z: x / (x ** 2 + y ** 2) * (np.hypot(x, y) > 0.7) * (np.hypot(x, y) < 2.5)),
    ("y/(x^2+y^2) * (rho>0.7) * (rho<2.5)", lambda x, y, z: y / (x ** 2 + y ** 2) * (np.hypot(x, y) > 0.7) * (np.hypot(x, y) < 2.5)),
]
REJECTED = [("__import__('os')", "the call \"__import__('os')\""), ("x.real", "attribute access 'x.real'"), ("(lambda: 1)()", "the call '(lambda: 1)()'"),
            ("open", "the name 'open'"), ("x[0]", "the subscript 'x[0]'"), ('"s"', "the literal '\"s\"'"), ("q + 1", "the name 'q'"),
            ("eval('1')", "the call"), ("exec('1')", "the call"), ("x if y else z", "the conditional"), ("sin(x, y)", "sin takes 1 argument"),
            ("sin(x=1)", "the call"), ("[x, y]", "the construct"), ("x; y", "cannot be read"), ("x +", "cannot be read"), ("~x", "the operator in '~x'"),
            ("x % 2", "the operator in"), ("x // 2", "the operator in"), ("True", "the literal 'True'"), ("1j", "the literal '1j'"),
            ("().__class__", "attribute access"), ("sin.__call__(x)", "the call")]


def test_weight_expressions_against_numpy(monkeypatch):
    fx = pkg("field_excitation")

    def boom(*a, **k):
        raise AssertionError("eval / exec reached")
    assert len(EXPRESSIONS) >= 30
    rng = np.random.default_rng(0)
    x, y, z = rng.uniform(-3, 3, 200), rng.uniform(0.1, 3, 200), rng.uniform(-2, 2, 200)
    z[:5] = 0
    want = [ref(x, y, z) * np.ones(200) for _, ref in EXPRESSIONS]
    got, refused = [], []
    with monkeypatch.context() as m:          # neither builtin is reachable while the evaluator compiles, evaluates and refuses
        m.setattr(builtins, "eval", boom)
        m.setattr(builtins, "exec", boom)
        for expr, _ in EXPRESSIONS:
            got.append(fx.compile_weight(expr)(x, y, z))
        for expr, _ in REJECTED:
            try:
                fx.compile_weight(expr, "excitation 'w'")
                refused.append(None)
            except ValueError as err:
                refused.append(str(err))
    for (expr, _), g, w in zip(EXPRESSIONS, got, want):
        assert g.shape == (200,) and g.dtype == np.float64
        err = np.max(np.abs(g - w) / np.maximum(np.abs(w), 1.0))
        assert err <= 1e-15, (expr, err)
    for (expr, msg), said in zip(REJECTED, refused):
        assert said is not None and msg in said, (expr, said)
    with pytest.raises(ValueError, match=r"excitation 'w': weight function 'x.real'"):
        fx.compile_weight("x.real", "excitation 'w'")


# ---- the upstream spellings that stay refused -------------------------------------------------------------------------------------
def test_unchanged_refusals():
    import ports_cases as pc
    api = pkg("openems_api")
    CSX = api.ContinuousStructure()
    for t in (0, 1, 2, 3):
        with pytest.raises(ValueError, match=f"exc_type {t} .* is not supported .*AddLumpedPort"):
            CSX.AddExcitation("e", t, [0, 0, 1])
    exc = CSX.AddExcitation("plane_wave", 10, [0, 1, 1])
    with pytest.raises(ValueError, match="SetWeightFunction is not supported"):
        exc.SetWeightFunction(["1", "1", "1"])
    fd, _ = pc.wg(None)
    with pytest.raises(ValueError, match="weight functions given as strings are not supported: pass Python callables"):
        fd.AddWaveGuidePort(3, [0, 0, 12], [16, 8, 24], "z", ["0", "-sin(x)"], ["sin(x)", "0"], 196.0, 1)
    assert not hasattr(api.openEMS, "AddCoaxialPort") and not hasattr(api.openEMS, "AddCircWaveGuidePort")
    # ... beside the new entry point, which logs its call and validates at once
    ex = fd.AddFieldExcitation("feed", 0, [0, 1, 0], [0, 0, 20], [16, 8, 20], weight=["0", "sin(pi*x/16)", "0"], delay=1e-12, priority=3)
    assert fd.calls[-1] == {"op": "AddFieldExcitation", "name": "feed", "exc_type": 0, "exc_val": [0.0, 1.0, 0.0], "start": [0.0, 0.0, 20.0],
                            "stop": [16.0, 8.0, 20.0], "weight": ["0", "sin(pi*x/16)", "0"], "delay": 1e-12, "priority": 3}
    assert ex.priority == 3 and ex.weight[1].expression == "sin(pi*x/16)"
    with pytest.raises(ValueError, match="AddFieldExcitation 'feed' is defined twice"):
        fd.AddFieldExcitation("feed", 0, [0, 1, 0], [0, 0, 20], [16, 8, 20])
    with pytest.raises(ValueError, match=r"field excitation 'w' \(component x\): weight function 'os.system': attribute access 'os.system'"):
        fd.AddFieldExcitation("w", 2, [1, 0, 0], [0, 0, 20], [16, 8, 20], weight=["os.system", "0", "0"])


# ---- E types through the oracle: a hard edge reads exactly amp * sig[n - d] --------------------------------------------------------
def test_hard_and_soft_e_through_the_oracle(oracle_lib):
    capi = pkg("_capi")
    for device_operator in (True, False):
        for classes in (True, False):
            s = _sim(None, [("hard", 1, [0, 0, 2.0], [5, 5, 4], [5, 6, 6], dict(delay=5e-12, weight=[None, None, "1 + y"])),
                            ("soft", 0, [0, 3.0, 0], [8, 5, 6], [8, 7, 6])], use_classes=classes)
            s.device_operator = device_operator
            e = s.build(oracle_lib)
            vv, vi, _, _ = e.get_operator()
            h = s.excite_lists.hard_e
            assert h[0].size == 4 and not vv.reshape(3, -1)[h[1].astype(int), h[0]].any() and not vi.reshape(3, -1)[h[1].astype(int), h[0]].any()
            soft = s.excite_lists.soft_e
            assert vv.reshape(3, -1)[soft[1].astype(int), soft[0]].all()
            pid = [e.add_probe(capi.KIND_V, [g], [c], [1.0]) for g, c in zip(h[0], h[1])]
            e.run(100)
            d = int(h[3][0])
            assert d == round(5e-12 / s.dt) and d > 0
            sig = np.concatenate([np.zeros(d, np.float32), s.signal])[:100]
            for q, p in enumerate(pid):
                assert np.array_equal(e.get_probe(p), (h[2][q] * sig).astype(np.float64))      # fp32(amp * sig[n - d]), 0.0 before
            assert np.abs(e.fields()).max() > 0
            e.close()
    # past the table the hard edge reads 0.0: a table of 40 samples
    s = _sim(None, [("hard", 1, [0, 0, 2.0], [5, 5, 4], [5, 5, 5])])
    s.signal = s.signal[:40].copy()
    e = s.build(oracle_lib)
    p = e.add_probe(capi.KIND_V, s.excite_lists.hard_e[0], [2], [1.0])
    e.run(100)
    got = e.get_probe(p)
    assert np.array_equal(got[:40], (s.excite_lists.hard_e[2][0] * s.signal).astype(np.float64)) and not got[40:].any() and got[:40].any()


# ---- known-answer tests on the oracle plus the statement (records: profiles/excite/kat.txt) ----------------------------------------
C0, ETA0 = 299792458.0, 376.730313668
LAMBDA = 20e-3                                    # the launcher's centre wavelength: f0 = 15 GHz


def launcher_leakage(lib, monkeypatch, cells_per_lambda, whole_steps=False, towards=+1):
    """Backward over forward energy [dB] of the one-directional launcher in a parallel-plate line.

    The line: the z faces of the grid are the plates (PEC, two cells apart), the y faces magnetic walls, CPML of 8 cells at both x
    ends; the TEM wave (E_z, H_y = -+ E_z / eta0 towards +-x) runs along x.  The launcher: a soft-E plane on the node plane i0 and a
    soft-H plane half a cell behind it (at i0 - 1/2), E_z = c dt / dx and H_y = -towards E_z / eta0: the amplitude ratio is the wave
    impedance.  This is the total-field / scattered-field pair of a wave towards +x: the E plane must read the pulse
    dx / (2 c) - dt / 2 ahead of the H plane.  The run takes dt = dx / (2 c), so that this is dt / 2: the E plane reads
    sig[n] = s(n dt), the H plane, one timestep late, sigH[n - 1] = s((n - 1/2) dt) — exactly, and what is left is the grid's
    dispersion.  With sigH taken at whole steps the H plane reads s((n - 1) dt): half a timestep off.  towards = -1 turns the H
    plane round: the wave leaves towards -x instead (the positive control of the probes).
    Probes 20 cells in front of and behind the launcher; the run ends before the echo of the far CPML reaches the rear probe."""
    sc, sim, grid = pkg("scene"), pkg("simulation"), pkg("grid")
    dx = LAMBDA / cells_per_lambda
    q = cells_per_lambda // 20
    nx, i0 = 220 * q, 60 * q
    g = grid.RectGrid(np.arange(nx) * dx, np.arange(5) * dx, np.arange(3) * dx)
    dt = dx / (2 * C0)
    s = sc.Scene(unit=dx)
    S = C0 * dt / dx
    s.add_field_excitation("e", 0, [0, 0, S], [i0, 1, 0], [i0, 3, 2])
    s.add_field_excitation("h", 2, [0, -towards * S / ETA0, 0], [i0 - 0.5, 1, 0], [i0 - 0.5, 3, 2], delay=dt)
    run = sim.Simulation(g, sc.voxelize(s, g), f0=C0 / LAMBDA, fc=0.5 * C0 / LAMBDA, boundary=["CPML", "CPML", "PMC", "PMC", "PEC", "PEC"],
                         cpml_cells=8, nr_ts=600 * q, end_criteria=0.0, dt=dt)
    assert run.excite_lists.soft_e[0].size == 6 and run.excite_lists.soft_h[0].size == 6 and set(run.excite_lists.soft_h[3].tolist()) == {1}
    xc.install(monkeypatch, sig_h=(lambda m: m.signal) if whole_steps else None)
    e = run.build(lib)
    pf = e.add_probe(0, [g.flat(i0 + 20 * q, 2, 0)], [2], [1.0])
    pb = e.add_probe(0, [g.flat(i0 - 20 * q, 2, 0)], [2], [1.0])
    e.run(600 * q)
    f, b = e.get_probe(pf), e.get_probe(pb)
    return 10 * np.log10(np.sum(b * b) / np.sum(f * f))


def test_one_directional_launcher(oracle_lib, monkeypatch):
    """Measured on the oracle plus statement (profiles/excite/kat.txt): -70.4 dB at lambda / 20, -88.7 dB at lambda / 40, -27.9 dB with
    sigH at whole steps.  The bar is 6 dB above the lambda / 20 value: roughly a factor of two in amplitude for mesh and pulse-shape
    variation."""
    BAR = -70.4 + 6.0
    l20 = launcher_leakage(oracle_lib, monkeypatch, 20)
    l40 = launcher_leakage(oracle_lib, monkeypatch, 40)
    mistimed = launcher_leakage(oracle_lib, monkeypatch, 20, whole_steps=True)
    back = launcher_leakage(oracle_lib, monkeypatch, 20, towards=-1)
    print(f"launcher: backward / forward {l20:.1f} dB at lambda/20, {l40:.1f} dB at lambda/40, {mistimed:.1f} dB with sigH at whole steps, "
          f"{back:.1f} dB launched backwards")
    assert l20 <= BAR                           # small ...
    assert l40 < l20                            # ... falls as the cell is halved ...
    assert mistimed >= l20 + 20.0               # ... and rests on the half-step timing of sigH
    assert back > 10.0                          # (the probes tell the two directions apart)


def test_magnetic_dipole(oracle_lib, monkeypatch):
    """One soft H face: a magnetic dipole along the face normal, the dual of test_oracle_kat_cpu.test_hertzian_dipole_directivity, with
    that test's grid and bars: D = 1.5 +- 0.06, a sin^2 pattern, the field E_phi alone, surface flux = far-field power within 2 %."""
    sc, sim, grid, nf = pkg("scene"), pkg("simulation"), pkg("grid"), pkg("nf2ff")
    n, d, f0, c = 52, 2.5e-3, 3e9, 26
    g = grid.RectGrid(*[np.arange(n) * d] * 3)
    s = sc.Scene(unit=d)
    s.add_field_excitation("m", 2, [0, 0, 1.0], [c + 0.5, c + 0.5, c], [c + 0.5, c + 0.5, c])
    run = sim.Simulation(g, sc.voxelize(s, g), f0=f0, fc=1.5e9, boundary="CPML", cpml_cells=8, nr_ts=1400, nf2ff_freqs=[f0], end_criteria=0.0)
    assert run.excite_lists.soft_h[0].tolist() == [g.flat(c, c, c)] and run.excite_lists.soft_h[1].tolist() == [2]
    xc.install(monkeypatch)
    e = run.build(oracle_lib)
    e.run(1400)
    th = np.deg2rad(np.arange(0, 181, 5.0))
    ph = np.deg2rad(np.arange(0, 360, 30.0))
    centre = [g.x[c] + 0.5 * d, g.y[c] + 0.5 * d, g.z[c]]
    res = nf.calc_nf2ff(oracle_lib, run.nf2ff_box, run.nf2ff_boxes(), [f0], th, ph, centre)
    U = res.P_rad[0] / res.P_rad[0].max()
    dth, dph = th[1] - th[0], ph[1] - ph[0]
    P_ff = np.sum(res.P_rad[0] * np.sin(th)[:, None]) * dth * dph
    print(f"magnetic dipole: D = {res.Dmax[0]:.4f}, pattern error {np.max(np.abs(U - np.sin(th)[:, None] ** 2)):.4f}, "
          f"E_theta / E_phi {np.max(np.abs(res.E_theta[0])) / np.max(np.abs(res.E_phi[0])):.4f}, P_ff / P_flux - 1 = {P_ff / res.Prad[0] - 1:+.4f}")
    assert abs(res.Dmax[0] - 1.5) < 0.06, res.Dmax
    assert np.max(np.abs(U - np.sin(th)[:, None] ** 2)) < 0.03
    assert np.max(np.abs(res.E_theta[0])) < 0.02 * np.max(np.abs(res.E_phi[0]))
    assert abs(P_ff - res.Prad[0]) / res.Prad[0] < 0.02


COAX_RI, COAX_RO, COAX_BAND = 1.0, 3.5, (4e9, 12e9)            # mm, mm, Hz: 60 ln(3.5) = 75.17 ohm, TE11 cuts off near 21 GHz


def coax_impedance(lib, h):
    """Re(U / I) over COAX_BAND of an air-filled coaxial line along z, cells of h [mm], drawn with cylinders — no port class: a soft-E
    excitation with the radial weights x / (x^2 + y^2), y / (x^2 + y^2) on the annulus, a voltage probe (type 0) from the inner
    conductor to the shell, two current probes (type 1) round the inner conductor on the dual planes half a cell below and above the
    voltage probe's plane (their mean has the voltage's phase centre), CPML of 8 cells at both ends, the conductors through them."""
    api = pkg("openems_api")
    ri, ro = COAX_RI, COAX_RO
    q = int(round(0.5 / h))
    half = ro + 1.0                                           # the shell is 1 mm thick
    nz = 16 + 30 * q
    fd = api.openEMS(NrTS=900 * q, EndCriteria=0, lib=lib, cpml_cells=8)
    fd.SetGaussExcite(8e9, 6e9)
    fd.SetBoundaryCond(["PEC", "PEC", "PEC", "PEC", "PML_8", "PML_8"])
    csx = api.ContinuousStructure()
    fd.SetCSX(csx)
    mesh = csx.GetGrid()
    mesh.SetDeltaUnit(1e-3)
    xy = np.arange(-round(half / h), round(half / h) + 1) * h
    mesh.AddLine("x", xy)
    mesh.AddLine("y", xy)
    mesh.AddLine("z", np.arange(nz) * h)
    L = (nz - 1) * h
    metal = csx.AddMetal("conductors")
    metal.AddCylinder([0, 0, 0], [0, 0, L], ri)
    metal.AddCylindricalShell([0, 0, 0], [0, 0, L], ro + 0.5, 1.0)
    z0, z1 = (8 + 6 * q) * h, (8 + 22 * q) * h
    cut = f"(rho>{ri}) * (rho<{ro})"
    fd.AddFieldExcitation("feed", 0, [1, 1, 0], [-ro, -ro, z0], [ro, ro, z0], weight=[f"x/(x^2+y^2) * {cut}", f"y/(x^2+y^2) * {cut}", "0"])
    csx.AddProbe("ut", 0).AddBox([ri, 0, z1], [ro, 0, z1])
    rm = ri + 1.0
    csx.AddProbe("it_lo", 1, norm_dir="z").AddBox([-rm, -rm, z1 - 0.25 * h], [rm, rm, z1 - 0.25 * h])
    csx.AddProbe("it_hi", 1, norm_dir="z").AddBox([-rm, -rm, z1 + 0.25 * h], [rm, rm, z1 + 0.25 * h])
    fd.Run(None)
    assert fd.stats.excitations[0]["edges"] > 0 and fd.stats.excitations[0]["dropped_metal_edges"] > 0
    assert fd.stats.probes[1]["dual_plane"] + 1 == fd.stats.probes[2]["dual_plane"] == 8 + 22 * q
    f = np.linspace(*COAX_BAND, 17)
    u, i1, i2 = fd.GetProbe("ut"), fd.GetProbe("it_lo"), fd.GetProbe("it_hi")
    assert np.abs(u["val"][-50:]).max() < 1e-3 * np.abs(u["val"]).max()
    U = api.dft_time2freq(u["t"], u["val"], f)
    I = 0.5 * (api.dft_time2freq(i1["t"], i1["val"], f) + api.dft_time2freq(i2["t"], i2["val"], f))
    return f, U / I


def test_coaxial_line_without_a_port_class(oracle_lib):
    """Measured on the oracle (profiles/excite/kat.txt): max |Re(U / I) / Z0 - 1| over 4 .. 12 GHz = 0.1222 with cells of 0.5 mm (84.2 ..
    84.4 ohm against 75.17) and 0.0889 with cells of 0.25 mm (81.8 ohm): a staircased coax converges slowly.  The bar is 1.5 times the
    deviation measured at the coarser size, and the deviation has to shrink."""
    z0 = 60.0 * np.log(COAX_RO / COAX_RI)
    BAR = 1.5 * 0.1222
    dev = []
    for h in (0.5, 0.25):
        f, z = coax_impedance(oracle_lib, h)
        dev.append(float(np.max(np.abs(z.real / z0 - 1))))
        print(f"coax, cells of {h} mm: Re(U/I) = {z.real.min():.2f} .. {z.real.max():.2f} ohm (Z0 = {z0:.2f}), |Im| <= {np.abs(z.imag).max():.3f}, deviation {dev[-1]:.4f}")
        assert np.all(z.real > 0) and np.abs(z.imag).max() < 0.01 * z0          # a travelling wave towards +z
    assert dev[0] <= BAR and dev[1] <= BAR
    assert dev[1] < dev[0]


# ---- the directed list shapes and the observer scene of test_excite_gpu.py, on the reference alone --------------------------------
def _restated_fields(oracle_lib, lists, n=xc.MAIN_GRID, nsteps=80, seed=4):
    from restatement import Restatement
    r = Restatement(xc.main_sim(n=n), oracle_lib, seed=seed, tables=None if lists is None else {"excite": lists.args()})
    r.run(nsteps)
    return r.e.fields()


def test_directed_lists_are_on_their_side_of_each_threshold():
    """Integer arithmetic on the lists alone: the face counts around k_excite's block of 256, the one face with 300 entries before,
    inside and past the table, the two listings of the 40 faces, and the faces at the grid's extremes."""
    assert xc.PLANE_COUNTS == (1, 255, 256, 257)
    for count in xc.PLANE_COUNTS:
        for hard in (False, True):
            l = xc.plane_lists(count, hard)
            fi, fc = l.faces()
            assert fi.size == count and (count + 255) // 256 == (1 if count <= 256 else 2)
            assert np.all(fi // (xc.MAIN_GRID[0] * xc.MAIN_GRID[1]) == 5)                              # one node plane
            assert all(xc.face_exists(int(c), *_ijk(int(g)), xc.MAIN_GRID) for g, c in zip(fi, fc))
            assert l.hard[0].size == (count if hard else 0) and {0, 3, 57} >= set(l.soft[3].tolist())
    l = xc.many_entries_lists()
    amp, delay = l.soft[2], l.soft[3]
    assert l.faces()[0].size == 1 and amp.size == 300 and (amp > 0).sum() > 100 and (amp < 0).sum() > 100
    assert np.abs(amp).max() / np.abs(amp).min() > 3e5 and np.abs(amp).max() <= 1e-3
    # 80 timesteps, 40 samples: read from the first timestep on; starting inside the run; never reached
    assert (delay == 0).any() and ((delay > 0) & (delay < 40)).sum() > 50 and (delay >= 80).sum() > 50 and ((delay >= 40) & (delay < 80)).sum() > 50
    a, b = xc.forty_faces_lists("face-major"), xc.forty_faces_lists("entry-major")
    assert a.faces()[0].size == 40 and a.soft[0].size == 120 and set(a.faces()[1].tolist()) == {0, 1, 2}
    ka, kb = a.soft[0] * 3 + a.soft[1], b.soft[0] * 3 + b.soft[1]
    assert np.all(ka.reshape(40, 3) == ka.reshape(40, 3)[:, :1]) and np.all(kb.reshape(3, 40) == kb[:40]) and np.unique(kb[:40]).size == 40
    oa, ob = np.argsort(ka, kind="stable"), np.argsort(kb, kind="stable")         # the host's grouping: a stable sort on 3 idx + comp
    for q in range(4):
        assert np.array_equal(a.soft[q][oa], b.soft[q][ob])
    assert np.array_equal(a.rank[oa], b.rank[ob]) and np.array_equal(a.sigH, b.sigH)
    for nx in xc.NX_EXTREMES:
        n = (nx,) + xc.MAIN_GRID[1:]
        faces = xc.extreme_faces(n)
        assert len(set(faces)) == 15 and all(xc.face_exists(*f, n) for f in faces)
        for c in range(3):
            mine = [f for f in faces if f[0] == c]
            assert (c, 0, 0, 0) in mine
            for a_ in range(3):
                assert max(f[1 + a_] for f in mine) == (n[a_] - 1 if a_ == c else n[a_] - 2)
        far = [b_ for f in faces for b_ in xc.beyond(f, n)]
        assert len(far) == 12 and all(0 <= p < n[a_] for b_ in far for a_, p in enumerate(b_[1:])) and not any(xc.face_exists(*b_, n) for b_ in far)
        for hard in (False, True):
            l = xc.extreme_lists(nx, hard)
            assert l.faces()[0].size == 15 and (l.hard[0].size, l.soft[0].size) == ((15, 0) if hard else (0, 18))
    assert {nx % 4 for nx in xc.NX_EXTREMES} == {0, 1, 2, 3}


def _ijk(g, n=xc.MAIN_GRID):
    return g % n[0], g // n[0] % n[1], g // (n[0] * n[1])


def test_directed_lists_on_the_reference(oracle_lib):
    """The reference side of the directed cases: 300 entries on one face in reversed list order give other bits; the 40 faces listed
    face by face and entry by entry give the same bits, and with each face's entries reversed other ones; every face at the grid's
    extremes ends the run with another current than without the set; the held faces read zero."""
    bare = _restated_fields(oracle_lib, None)
    fwd, rev = _restated_fields(oracle_lib, xc.many_entries_lists()), _restated_fields(oracle_lib, xc.many_entries_lists(reverse=True))
    assert np.isfinite(fwd).all() and not np.array_equal(fwd, bare) and not np.array_equal(fwd, rev)
    a, b = xc.forty_faces_lists("face-major"), xc.forty_faces_lists("entry-major")
    fa, fb = _restated_fields(oracle_lib, a), _restated_fields(oracle_lib, b)
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and not np.array_equal(fa, bare)
    flipped = xc.HLists(a.hard, tuple(np.asarray(q).reshape(40, 3)[:, ::-1].ravel() for q in a.soft), a.sigH)
    assert not np.array_equal(_restated_fields(oracle_lib, flipped), fa)
    for nx in xc.NX_EXTREMES:
        n = (nx,) + xc.MAIN_GRID[1:]
        none = _restated_fields(oracle_lib, None, n=n)
        for hard in (False, True):
            f = _restated_fields(oracle_lib, xc.extreme_lists(nx, hard), n=n)
            same = [fc for fc in xc.extreme_faces(n) if f[1, fc[0], fc[3], fc[2], fc[1]] == none[1, fc[0], fc[3], fc[2], fc[1]]]
            assert np.isfinite(f).all() and not same, (nx, hard, same)
    l = xc.held_lists(80)
    f = _restated_fields(oracle_lib, l)
    assert all(f[1, int(c)].reshape(-1)[g] == 0 for g, c in zip(l.hard[0], l.hard[1])) and not np.array_equal(f, bare)


@pytest.mark.parametrize("kind", sorted(xc.OBS_KINDS))
def test_observers_tell_behind_the_excitation_from_in_front_of_it(oracle_lib, kind):
    """The observer scene on the reference alone: the I-probe, the box's running DFT sums and its record, read from the restated I in
    front of `excite` instead of behind it, all change — so a library that samples one of them in front of k_excite cannot pass."""
    sc = xc.observer_scene(kind)
    n = xc.OBS_GRID
    assert max(n[0] - 24, n[1] - 20, n[2] - 16) <= 0
    c, lo, hi = sc["box"]
    inside = lambda f: f[0] == c and all(lo[a] <= f[1 + a] <= hi[a] for a in range(3))
    hk, sk = sc["lists"].hard[0] * 3 + sc["lists"].hard[1], sc["lists"].soft[0] * 3 + sc["lists"].soft[1]
    key = lambda f: xc.node(*f[1:], n) * 3 + f[0]
    assert inside(sc["hard"]) and inside(sc["soft"]) and key(sc["hard"]) in hk and key(sc["hard"]) not in sk and (sk == key(sc["soft"])).sum() == 2
    for probe in (sc["probe"], sc["late"]):
        pk = set((probe[0] * 3 + probe[1]).tolist())
        assert {key(sc["hard"]), key(sc["soft"])} <= pk
    if kind == "mur-near":
        assert sc["hard"][1] == 1 and sc["soft"][2] == n[1] - 2 and sc["source"][0][0] % n[0] == 1      # one node from x-; the last cell row; the plane next to x-
    ref = xc.observed(oracle_lib, kind)
    assert np.isfinite(ref.fields).all() and ref.series.size == xc.OBS_STEPS and ref.late.size == xc.OBS_STEPS - ref.late_at
    assert np.count_nonzero(ref.series != ref.series_front) > xc.OBS_STEPS // 2
    scale = np.abs(ref.acc).max()
    assert np.abs(ref.acc - ref.acc_front).max() > 1e-3 * scale
    at = lambda a, f: a[..., f[3] - lo[2], f[2] - lo[1], f[1] - lo[0]]
    for f in (sc["hard"], sc["soft"]):      # ... on both faces, in the sums and in the record
        assert np.abs(at(ref.acc, f) - at(ref.acc_front, f)).max() > 1e-3 * scale
        assert np.count_nonzero(at(ref.rec, f) != at(ref.rec_front, f)) >= 3
    # the hard face reads the excitation itself
    amp, d = sc["lists"].hard[2][0], int(sc["lists"].hard[3][0])
    sig = np.concatenate([np.zeros(d, np.float32), sc["lists"].sigH, np.zeros(xc.OBS_STEPS, np.float32)])[:xc.OBS_STEPS]
    assert np.array_equal(at(ref.rec, sc["hard"]), (amp * sig)[::xc.OBS_EVERY])
