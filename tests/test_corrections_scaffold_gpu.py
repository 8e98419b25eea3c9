"""What the corrections share (csrc/dense_box.hpp, the edge list of csrc/sheet.hip, the planner's table in csrc/api.hip).

The Lorentz media and the magnetic faces go through the same widen / scatter / crop as the Debye media: their boxes walk the x
alignments test_dispersion_gpu.test_box_alignment_in_x walks (X_ALIGN; test_box_alignment_cases_cover_every_residue there pins what
the list covers), against the restatements of test_lorentz_model_cpu / test_magnetic_model_cpu, bit for bit.  And every refusal that
now comes out of one place keeps its text, for all eight rows of the table (csrc/corrections.hpp); a set that is cleared leaves the
context what it was, and a row's `prime` follows fdtd_set_field."""
import numpy as np
import pytest

from conftest import pkg
from helpers import seeded_fields
from restatement import Restatement
from test_dispersion_gpu import X_ALIGN
from test_lorentz_model_cpu import TWO_PI
from test_sheet_model_cpu import _grid
import test_lorentz_gpu
import test_magnetic_gpu

NY, NZ, NSTEPS = 6, 5, 20
IDS = [f"x{a}-{b}-nx{n}" for a, b, n in X_ALIGN]


def _plain_sim(nx):
    """A PEC box of nx x 6 x 5 nodes filled with a plain dielectric, a port inside (the restatements sample its probes)."""
    sc, sim = pkg("scene"), pkg("simulation")
    g = _grid((nx, NY, NZ))
    x, y, z = (l * 1e3 for l in g.lines)
    s = sc.Scene(unit=1e-3)
    s.add_material("fill", eps_r=2.0).add_box([x[0], y[0], z[0]], [x[-1], y[-1], z[-1]])
    s.add_lumped_port(1, 50.0, [x[2], y[2], z[1]], [x[2], y[2], z[3]], "z", 1.0)
    return sim.Simulation(g, sc.voxelize(s, g), f0=9e9, fc=5e9, boundary="PEC", nr_ts=NSTEPS, end_criteria=0.0)


def _boxes(x0, x1, nx, edges):
    """Per component the box [x0, x1) x [1, 5) x [1, 4) of cells as its edges (`edges`) or faces: one element more along the axes
    the component does not point along (edges) / points along (faces), as far as the grid has them."""
    lo, hi = [], []
    for c in range(3):
        l, h = [x0, 1, 1], [x1, NY - 1, NZ - 1]
        for a, n in enumerate((nx, NY, NZ)):
            if (a != c) == edges:
                h[a] = min(h[a] + 1, n)
        lo.append(tuple(l)); hi.append(tuple(h))
    return lo, hi


@pytest.mark.gpu
@pytest.mark.parametrize("x0,x1,nx", X_ALIGN, ids=IDS)
def test_lorentz_box_alignment_in_x(hip_lib, oracle_lib, x0, x1, nx):
    """Two media of two poles (k_lorentz<true, 2>) over boxes of every x alignment, holes inside, from seeded fields: whole-grid fields
    (the widened columns outside the caller's box keep their bits) and fdtd_lorentz_get's v_prev, states and vi."""
    lor = pkg("lorentz")
    rng = np.random.default_rng(x0 + 100 * x1 + 10000 * nx)
    lo, hi = _boxes(x0, x1, nx, edges=True)
    assert lo[0][0] == x0 and hi[0][0] == x1 and hi[1][0] == hi[2][0] == min(x1 + 1, nx)
    shapes = [(h[2] - l[2], h[1] - l[1], h[0] - l[0]) for l, h in zip(lo, hi)]
    w = [(1e-3 * rng.uniform(0.2, 1.0, s) * (rng.uniform(size=s) > 0.25)).astype(np.float32) for s in shapes]
    med = [rng.integers(0, 2, s).astype(np.uint8) for s in shapes]
    media = [lor.LorentzMedium(1.0, 0.0, TWO_PI * np.array([7e9, 5e9]), TWO_PI * np.array([0.0, 9e9]), np.array([3e9, 1e9])),
             lor.LorentzMedium(1.0, 0.0, TWO_PI * np.array([4e9, 6e9]), TWO_PI * np.array([11e9, 0.0]), np.array([0.0, 8e9]))]
    sim0 = _plain_sim(nx)
    tables = lor.tables(media, sim0.dt, K=2) + (lo, hi, w, med)
    ref = Restatement(sim0, oracle_lib, seed=x0 + 100 * x1, tables={"lorentz": tables})
    ref.run(NSTEPS)
    e = _plain_sim(nx).build(hip_lib)
    seeded_fields(e, x0 + 100 * x1)
    e.set_lorentz(*tables)
    e.run(NSTEPS)
    assert all(np.any(ref.lorentz.w[c] != 0) and np.any(w[c] == 0) for c in range(3))
    assert min(np.abs(x).max() for x in ref.lorentz.x) > 0
    assert np.array_equal(e.fields(), ref.e.fields())
    test_lorentz_gpu._same_state(e, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("x0,x1,nx", X_ALIGN, ids=IDS)
def test_magnetic_box_alignment_in_x(hip_lib, oracle_lib, x0, x1, nx):
    """Two classes and class 0 over boxes of every x alignment, from seeded fields: whole-grid fields and fdtd_magnetic_get's i_prev
    and iv0."""
    rng = np.random.default_rng(x0 + 100 * x1 + 10000 * nx)
    lo, hi = _boxes(x0, x1, nx, edges=False)
    assert lo[0][0] == x0 and hi[0][0] == min(x1 + 1, nx) and hi[1][0] == hi[2][0] == x1
    cls = [rng.integers(0, 3, (h[2] - l[2], h[1] - l[1], h[0] - l[0])).astype(np.uint8) for l, h in zip(lo, hi)]
    for q in cls:
        q.reshape(-1)[:3] = (1, 0, 2)
    tables = (np.array([0.97, 1.0], np.float32), np.array([0.5, 0.25], np.float32), lo, hi, cls)
    ref = Restatement(_plain_sim(nx), oracle_lib, seed=x0 + 100 * x1, tables={"magnetic": tables})
    seed_I = [ref.e.get_field(1, c) for c in range(3)]
    ref.run(NSTEPS)
    e = _plain_sim(nx).build(hip_lib)
    seeded_fields(e, x0 + 100 * x1)
    e.set_magnetic(*tables)
    e.run(NSTEPS)
    assert np.array_equal(e.fields(), ref.e.fields())
    test_magnetic_gpu._same_state(e, ref)
    for c in range(3):
        ip, before = e.magnetic_state(c)[0], seed_I[c][ref.magnetic.sl[c]]
        assert np.array_equal(ip[cls[c] == 0], before[cls[c] == 0]) and np.any(ip[cls[c] != 0] != before[cls[c] != 0])


# ---- the refusals: one context of 8 x 8 x 8 nodes per correction (all eight rows of the planner's table, corrections[] in
# csrc/corrections.hpp), one edge, one face or a box of one cell; CLEAR: the same setters with an empty set ----------------------------
E_PHASE = "their correction runs between the E phase and the H update"
H_PHASE = "their correction runs between the H update and the next E phase"
ONE = [(3, 3, 3)] * 3, [(4, 4, 4)] * 3
EDGE = (np.array([3 * 64 + 3 * 8 + 3], np.int64), np.array([2], np.int8))


def _set_sheet(e):
    e.set_sheets(*EDGE, np.array([0.5], np.float32), np.array([0], np.int32), np.array([[0.9]], np.float32), np.array([[0.1]], np.float32))


def _set_debye(e):
    e.set_debye(np.array([[0.9]]), np.array([[0.1]]), np.array([[0.5]]), *ONE, [np.full((1, 1, 1), 1e-3, np.float32)] * 3)


def _set_lorentz(e):
    e.set_lorentz(np.full((1, 1, 2, 2), 0.5), np.full((1, 1, 2), 0.1), np.full((1, 1, 2), 0.1), *ONE, [np.full((1, 1, 1), 1e-3, np.float32)] * 3)


def _set_lumped(e):
    e.set_lumped(*EDGE, np.array([0.5], np.float32), np.array([0], np.int32), np.full((1, 2, 2), 0.5), np.full((1, 2), 0.1), np.full((1, 2), 0.1))


def _set_magnetic(e):
    e.set_magnetic([0.97], [0.5], *ONE, [np.ones((1, 1, 1), np.uint8)] * 3)


def _set_conformal(e):
    e.set_conformal(EDGE[1], EDGE[0], np.full((1, 4), 0.1, np.float32))


def _set_planewave(e):
    one = (np.array([[1e-3, 0.0]], np.float32), np.zeros((1, 2), np.int32), np.array([[0.5, 0.0]], np.float32))
    e.set_planewave(*EDGE, *one, *EDGE, *one, np.ones(4, np.float32))                # one edge, and the face at the same node


def _set_excite(e):
    e.set_excite(*EDGE, [1.0], [0], [], [], [], [], np.ones(4, np.float32))          # one hard face


NO_BOX = [(0, 0, 0)] * 3, [(0, 0, 0)] * 3, [None] * 3
NO_EDGE = (EDGE[0][:0], EDGE[1][:0], np.zeros(0, np.float32), np.zeros(0, np.int32))
CLEAR = {"fdtd_sheet_set": lambda e: e.set_sheets(*NO_EDGE, np.zeros((0, 1), np.float32), np.zeros((0, 1), np.float32)),
         "fdtd_debye_set": lambda e: e.set_debye(np.zeros((0, 1)), np.zeros((0, 1)), np.zeros((0, 1)), *NO_BOX),
         "fdtd_lorentz_set": lambda e: e.set_lorentz(np.zeros((0, 1, 2, 2)), np.zeros((0, 1, 2)), np.zeros((0, 1, 2)), *NO_BOX),
         "fdtd_lumped_set": lambda e: e.set_lumped(*NO_EDGE, np.zeros(0), np.zeros(0), np.zeros(0)),
         "fdtd_magnetic_set": lambda e: e.set_magnetic([], [], *NO_BOX),
         "fdtd_conformal_set": lambda e: e.set_conformal(EDGE[1][:0], EDGE[0][:0], np.zeros((0, 4), np.float32)),
         "fdtd_planewave_set": lambda e: e.set_planewave(*[[]] * 10, None),
         "fdtd_excite_set": lambda e: e.set_excite(*[[]] * 8, None)}

REFUSALS = [("fdtd_sheet_set", _set_sheet, f"conducting sheets: the two-launch schedule only ({E_PHASE})"),
            ("fdtd_debye_set", _set_debye, f"Debye media: the two-launch schedule only ({E_PHASE})"),
            ("fdtd_lorentz_set", _set_lorentz, f"Lorentz media: the two-launch schedule only ({E_PHASE})"),
            ("fdtd_lumped_set", _set_lumped, f"lumped elements: the two-launch schedule only ({E_PHASE})"),
            ("fdtd_magnetic_set", _set_magnetic, f"magnetic materials: the two-launch schedule only ({H_PHASE})"),
            ("fdtd_conformal_set", _set_conformal, f"conformal boundaries: the two-launch schedule only ({H_PHASE})"),
            ("fdtd_planewave_set", _set_planewave, f"plane-wave excitation: the two-launch schedule only ({H_PHASE})"),
            ("fdtd_excite_set", _set_excite, f"H-field excitations: the two-launch schedule only ({H_PHASE})")]


@pytest.mark.gpu
@pytest.mark.parametrize("who,setter,two_launch", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal_messages_keep_their_text(hip_lib, who, setter, two_launch):
    capi = pkg("_capi")
    from test_lumped_model_cpu import pec_cavity
    sim = pec_cavity(n=(8, 8, 8), nr_ts=4)
    # a forced one-launch or resident schedule: FDTD_E_UNSUPPORTED when the context is asked to step
    for flag in (capi.FLAG_KERNEL_WAVEFRONT, capi.FLAG_KERNEL_RESIDENT):
        e = sim.build(hip_lib, flags=flag)
        setter(e)
        with pytest.raises(capi.FdtdError) as err:
            e.run(1)
        assert str(err.value).endswith(f"(-5): {two_launch}"), str(err.value)
        e.close()
    # after the first timestep, and before the operator: FDTD_E_STATE
    e = sim.build(hip_lib)
    e.run(1)
    with pytest.raises(capi.FdtdError) as err:
        setter(e)
    assert str(err.value).endswith(f"(-2): {who}: before the first timestep"), str(err.value)
    e.close()
    e = capi.Engine(hip_lib, 8, 8, 8, sim.dt)
    with pytest.raises(capi.FdtdError) as err:
        setter(e)
    assert str(err.value).endswith(f"(-2): {who}: set the operator first"), str(err.value)
    e.close()


_NEVER_SET = {}   # the fields of the engine that never had a set, computed by the first case that asks


def _cavity_engine(hip_lib):
    """The 8 x 8 x 8 cavity from seeded fields, and the three I components written once more (what the `prime` rows are asked about)."""
    from test_lumped_model_cpu import pec_cavity
    e = pec_cavity(n=(8, 8, 8), nr_ts=4).build(hip_lib)
    seeded_fields(e, 8)
    rng = np.random.default_rng(88)
    return e, [(1e-3 * rng.standard_normal(e.local_shape)).astype(np.float32) for _ in range(3)]


@pytest.mark.gpu
@pytest.mark.parametrize("who,setter", [r[:2] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_a_cleared_set_leaves_the_context_what_it_was(hip_lib, who, setter):
    """Set one element, clear it with an empty set: the schedule is the plain context's again, and four timesteps end in the bits of an
    engine that never had the set (the row's `active` and `release`).  Magnetic and conformal faces keep i_prev: written through
    fdtd_set_field while the set is live, the I arrays show up in the *_state() (the row's `prime`)."""
    capi = pkg("_capi")
    if not _NEVER_SET:
        r, new_I = _cavity_engine(hip_lib)
        for c in range(3):
            r.set_field(capi.KIND_I, c, new_I[c])
        r.run(4)
        _NEVER_SET["fields"] = r.fields()
        r.close()
    e, new_I = _cavity_engine(hip_lib)
    before = e.schedule_info()
    setter(e)
    assert e.schedule_info()["launches_per_timestep"] == 2
    for c in range(3):
        e.set_field(capi.KIND_I, c, new_I[c])
    if who == "fdtd_magnetic_set":
        for c in range(3):
            assert np.array_equal(e.magnetic_state(c)[0], new_I[c][3:4, 3:4, 3:4])
    if who == "fdtd_conformal_set":
        assert np.array_equal(e.conformal_state(), new_I[2][3, 3, 3:4])
    CLEAR[who](e)
    assert e.schedule_info() == before
    e.run(4)
    assert np.abs(_NEVER_SET["fields"]).max() > 0
    assert np.array_equal(e.fields(), _NEVER_SET["fields"])
    e.close()
