"""The two memory-traffic shortcuts of the update kernels (include/fdtd_hip_traffic.h) against the oracle, which knows neither:

 * inert CPML indices — the ends of the psi slot ranges whose coefficients are the identity — are skipped along y and z
   (fdtd_set_cpml trims them from the tables it is handed; kernel_common.hpp pml_slot_act);
 * the packed class bytes are read as one row offset per (k, j) plus the table of distinct rows (api.hip build_class_rows).

Every case starts from seeded random fields (psi is non-zero from the first timestep on), runs at least 3 x the longest axis in
timesteps in calls of 1 / 7 / the rest, and compares fields with np.array_equal, probe series and energy to 1e-12.  The shapes are
the smallest at which the range logic can go wrong: all faces, one-sided axes and a thickness-1 layer (whose E side has no active
index), rows longer than a wave with nx no multiple of 4, a Mur face beside CPML faces, slabs cut through a z layer.  The oracle
run of a case is computed once and shared by the schedules."""
import numpy as np
import pytest

from conftest import pkg
from helpers import seeded_fields
from opbuild_cases import random_scene

pytestmark = pytest.mark.gpu

#         shape           CPML cells x-, x+, y-, y+, z-, z+   Mur faces
CASES = {
    "all_faces_4": ((22, 19, 17), (4, 4, 4, 4, 4, 4), None),
    "one_sided_and_thickness_1": ((37, 21, 18), (3, 0, 2, 5, 1, 4), None),
    "long_rows_nx_261": ((261, 12, 14), (3, 3, 3, 3, 3, 3), None),
    "mur_face_beside_cpml": ((22, 19, 17), (0, 4, 4, 4, 4, 4), [1, 0, 0, 0, 0, 0]),
}
# schedule -> (flags name, $FDTD_WF_MULTI)
SCHEDULES = {"two_launches": ("FLAG_KERNEL_DIRECT", None), "several_timesteps_per_launch": ("FLAG_KERNEL_WAVEFRONT", "5"),
             "one_timestep_per_launch": ("FLAG_KERNEL_WAVEFRONT", "1")}


def _steps(shape):
    return 3 * max(shape) + 2


def _scene(shape, seed=11):
    grid, eps, kap, pec, _ = random_scene(seed, shape, False, 3, n_lumped=0, pec_frac=0.0)
    return grid, eps, kap, pec


def _cpml_tables(grid, dt, cells):
    cp = pkg("cpml")
    return cp.build_cpml(grid, dt, cp.CPMLSpec(cells=tuple(cells)))


def _expected_skips(tabs, k0, nk):
    """Inert indices at the ends of the two slot ranges per (axis, side), worked out in numpy from the tables of the slab."""
    out = {}
    for a, ax in enumerate("xyz"):
        slot, coef = tabs.slot[a], tabs.coef[a]
        if a == 2:
            slot, coef = slot[k0:k0 + nk], coef[:, :, k0:k0 + nk]
        n = slot.size
        stored = slot >= 0
        lo = 0
        while lo < n and stored[lo]:
            lo += 1
        hi = lo
        while hi < n and not stored[hi]:
            hi += 1
        out[ax] = {}
        for eh, side in enumerate("EH"):
            inert = (coef[eh, 0] == 0) & (coef[eh, 1] == 0) & (coef[eh, 2] == 1)
            skipped = 0
            for b, e in ((0, lo), (hi, n)):
                idx = np.arange(b, e)
                act = idx[~inert[b:e]]
                skipped += idx.size - (0 if act.size == 0 else act[-1] - act[0] + 1)
            out[ax][side] = 0 if a == 0 else int(skipped)
    return out


def _engine(lib, grid, eps, kap, pec, dt, cells, mur, *, flags=0, k0=0, nk=None, rank=0, world=1, nsteps=64, operator="build"):
    capi, eco, const = pkg("_capi"), pkg("ecoperator"), pkg("constants")
    nx, ny, nz = grid.shape
    nk = nz - k0 if nk is None else nk
    e = capi.Engine(lib, nx, ny, nz, dt, k0=k0, nk=nk, rank=rank, world=world, max_steps=nsteps + 8, flags=flags)
    if operator == "build":
        emet, hmet = eco.pack_metric_tables(*eco.metric_lists(grid, dt), grid, k0, nk)
        e.build_operator(grid.d, eps, kap, pec, const.EPS0, eco.lumped_overrides(grid, eps, kap, pec, dt, []), emet, hmet)
    else:
        op = eco.build_operator(grid, eps, kap, pec, dt, [])
        e.set_operator_classes(*op.classes(k0, nk), *op.metric_tables(k0, nk))
    if any(cells):
        e.set_cpml(*_cpml_tables(grid, dt, cells).for_slab(k0, nk))
    if mur is not None:
        coeff = []
        for f in range(6):
            l = grid.lines[f // 2]
            d = (l[-1] - l[-2]) if f % 2 else (l[1] - l[0])
            coeff.append((const.C0 * dt - d) / (const.C0 * dt + d))
        e.set_mur(mur, coeff)
    t = np.arange(nsteps) * dt
    e.set_signal(np.sin(2 * np.pi * 8e9 * t) * np.exp(-((t - 30 * dt) / (12 * dt)) ** 2))
    i, j, k = nx // 2, ny // 2, nz // 2
    cell = (k * ny + j) * nx + i
    e.add_source(np.array([cell], np.int64), np.array([2], np.int8), np.array([1.0], np.float32))
    pv = e.add_probe(capi.KIND_V, np.array([cell + 2, cell + nx], np.int64), np.array([2, 0], np.int8), np.array([-1.0, 0.5], np.float32))
    pi = e.add_probe(capi.KIND_I, np.array([cell - 1, cell - nx * ny], np.int64), np.array([1, 0], np.int8), np.array([1.0, 2.0], np.float32))
    return e, pv, pi


def _seed_global(engs, shape, seed=3):
    """The same seeded global fields, cut to every engine's slab."""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    for kind in (0, 1):
        for comp in range(3):
            g = (1e-3 * rng.standard_normal((nz, ny, nx))).astype(np.float32)
            for e in engs:
                e.set_field(kind, comp, np.ascontiguousarray(g[e.k0:e.k0 + e.nk]))


def _run_cut(e, n):
    for m in (1, 7, n - 8):
        e.run(m)


_oracle = {}


def _oracle_run(oracle_lib, name):
    """(fields, V series, I series, energy) of the case on the oracle — computed once, shared and left unchanged."""
    if name not in _oracle:
        shape, cells, mur = CASES[name]
        grid, eps, kap, pec = _scene(shape)
        dt = grid.courant_dt()
        n = _steps(shape)
        e, pv, pi = _engine(oracle_lib, grid, eps, kap, pec, dt, cells, mur, nsteps=n)
        _seed_global([e], shape)
        _run_cut(e, n)
        f = e.fields()
        assert np.isfinite(f).all() and np.abs(f).max() > 0
        f.setflags(write=False)
        _oracle[name] = (f, e.get_probe(pv), e.get_probe(pi), e.energy())
    return _oracle[name]


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("name", list(CASES))
def test_inert_psi_indices_are_skipped_and_fields_equal_the_oracle(hip_lib, oracle_lib, monkeypatch, name, schedule):
    capi = pkg("_capi")
    shape, cells, mur = CASES[name]
    flag, multi = SCHEDULES[schedule]
    monkeypatch.setenv("FDTD_RESIDENT", "0")
    if multi is not None:
        monkeypatch.setenv("FDTD_WF_MULTI", multi)
    fo, uo, io, wo = _oracle_run(oracle_lib, name)
    grid, eps, kap, pec = _scene(shape)
    dt = grid.courant_dt()
    n = _steps(shape)
    e, pv, pi = _engine(hip_lib, grid, eps, kap, pec, dt, cells, mur, flags=getattr(capi, flag), nsteps=n)
    info = e.traffic_info()
    want = _expected_skips(_cpml_tables(grid, dt, cells), 0, shape[2])
    print(name, schedule, "skipped", info["psi_skipped"], "expected", want, "bytes saved per timestep", info["bytes_saved_per_timestep"])
    assert info["psi_skipped"] == want
    assert sum(want["y"].values()) + sum(want["z"].values()) > 0 and info["bytes_saved_per_timestep"] > 0, "the case skips nothing"
    _seed_global([e], shape)
    _run_cut(e, n)
    sched = e.schedule_info()
    assert not sched["resident"]
    if flag == "FLAG_KERNEL_WAVEFRONT":
        assert sched["launches_per_timestep"] == 1
        assert (sched["timesteps_per_launch_max"] == 1) if multi == "1" else (mur is not None or sched["timesteps_per_launch_max"] > 1)
    else:
        assert sched["launches_per_timestep"] >= 2
    fh = e.fields()
    assert np.array_equal(fh, fo), f"{int((fh != fo).sum())} field values differ from the oracle's"
    assert len(uo) == n and _close(e.get_probe(pv), uo) and _close(e.get_probe(pi), io)
    assert _close(e.energy(), wo)


def test_expected_skips_of_the_cases_are_what_the_layout_implies():
    """The numpy count the GPU cases compare with, against the layout written out by hand: per axis with a low layer the E side loses
    node 0, with a high layer the node where it begins and the last one, the H side the last index; a thickness-1 low layer has no
    active E index at all (its one slot is node 0)."""
    shape, cells, _ = CASES["one_sided_and_thickness_1"]
    grid, *_ = _scene(shape)
    got = _expected_skips(_cpml_tables(grid, grid.courant_dt(), cells), 0, shape[2])
    assert got == {"x": {"E": 0, "H": 0}, "y": {"E": 3, "H": 1}, "z": {"E": 3, "H": 1}}
    shape, cells, _ = CASES["all_faces_4"]
    grid, *_ = _scene(shape)
    tabs = _cpml_tables(grid, grid.courant_dt(), cells)
    assert _expected_skips(tabs, 0, 17) == {"x": {"E": 0, "H": 0}, "y": {"E": 3, "H": 1}, "z": {"E": 3, "H": 1}}
    # slabs cut at plane 14, inside the upper z layer (planes 12 .. 16): the lower one loses node 0 and node 12, the upper one node 16
    assert _expected_skips(tabs, 0, 14)["z"] == {"E": 2, "H": 0} and _expected_skips(tabs, 14, 3)["z"] == {"E": 1, "H": 1}


@pytest.mark.parametrize("transport", ["p2p_two_launches", "p2p_one_launch", "linked"])
def test_slabs_cut_through_a_z_layer_equal_the_single_slab(hip_lib, oracle_lib, monkeypatch, transport):
    """22 x 19 x 17 with 4 cells on all faces as two slabs, planes 0 .. 13 and 14 .. 16: the lower slab owns planes 12 and 13 of the upper
    z layer, and each slab trims ITS z tables.  In-process P2P slabs (mailbox transport inside the update kernels, two launches and one)
    and linked slabs reproduce the single slab — and the oracle — bit for bit."""
    capi = pkg("_capi")
    name = "all_faces_4"
    shape, cells, mur = CASES[name]
    monkeypatch.setenv("FDTD_RESIDENT", "0")
    fo, uo, io, _ = _oracle_run(oracle_lib, name)
    grid, eps, kap, pec = _scene(shape)
    dt = grid.courant_dt()
    n = _steps(shape)
    flags = {"p2p_two_launches": capi.FLAG_KERNEL_DIRECT, "p2p_one_launch": capi.FLAG_KERNEL_WAVEFRONT, "linked": 0}[transport]
    e1, pv1, pi1 = _engine(hip_lib, grid, eps, kap, pec, dt, cells, mur, flags=capi.FLAG_KERNEL_DIRECT, nsteps=n)
    cut = [(0, 14), (14, 3)]
    built = [_engine(hip_lib, grid, eps, kap, pec, dt, cells, mur, flags=flags, k0=k0, nk=nk, rank=r, world=2, nsteps=n)
             for r, (k0, nk) in enumerate(cut)]
    engs = [b[0] for b in built]
    tabs = _cpml_tables(grid, dt, cells)
    for e, (k0, nk) in zip(engs, cut):
        info = e.traffic_info()["psi_skipped"]
        assert info == _expected_skips(tabs, k0, nk), (k0, nk, info)
        assert info["z"]["E"] > 0
    if transport != "linked":
        blobs = [e.p2p_export() for e in engs]
        engs[0].p2p_attach(None, blobs[1])
        engs[1].p2p_attach(blobs[0], None)
    _seed_global([e1] + engs, shape)
    _run_cut(e1, n)
    for m in (1, 7, n - 8):
        capi.run_linked(engs, m)
    f1, f2 = e1.fields(), np.concatenate([e.fields() for e in engs], axis=2)
    assert np.array_equal(f1, fo)
    assert np.array_equal(f2, f1), f"{int((f2 != f1).sum())} field values differ from the single slab's"
    u2 = sum(e.get_probe(b[1]) for e, b in zip(engs, built))
    i2 = sum(e.get_probe(b[2]) for e, b in zip(engs, built))
    assert _close(e1.get_probe(pv1), uo) and _close(u2, uo) and _close(i2, io)


# ---- class rows ---------------------------------------------------------------------------------------------------------------

def _box_and_sheet_scene(shape=(30, 26, 20)):
    """Vacuum with a dielectric box and a PEC sheet on top of it: several distinct class rows, most rows equal."""
    grid_m = pkg("grid")
    nx, ny, nz = shape
    grid = grid_m.RectGrid(*[np.arange(n) * 1e-3 for n in shape])
    eps = np.ones((nz - 1, ny - 1, nx - 1))
    kap = np.zeros_like(eps)
    eps[6:10, 7:18, 8:21] = 4.3
    kap[6:10, 7:18, 8:21] = 2.3e-3
    pec = np.zeros((3, nz, ny, nx), bool)
    pec[0, 10, 9:16, 10:18] = True      # x-directed edges of the sheet in node plane 10
    pec[1, 10, 9:15, 10:19] = True      # y-directed
    return grid, eps, kap, pec


def _numpy_class_rows(grid, eps, kap, pec, dt):
    """Distinct (k, j) rows of the per-edge classes, all three components side by side (a packed byte is a one-to-one code of the triple)."""
    ecls = pkg("ecoperator").build_operator(grid, eps, kap, pec, dt, []).classes()[0]
    nx, ny, nz = grid.shape
    rows = np.ascontiguousarray(np.transpose(ecls, (1, 2, 0, 3))).reshape(nz * ny, 3 * nx)
    return int(np.unique(rows, axis=0).shape[0])


def test_class_rows_equal_the_per_cell_bytes_and_the_oracle(hip_lib, oracle_lib, monkeypatch):
    """Row form and $FDTD_CLASS_ROWS=0, operator from fdtd_build_operator and from fdtd_set_operator_classes: the four runs equal each
    other and the oracle; the info call reports the row count worked out in numpy (0 in the per-cell form); fdtd_get_operator returns
    what it returned."""
    capi = pkg("_capi")
    monkeypatch.setenv("FDTD_RESIDENT", "0")
    shape, cells = (30, 26, 20), (3, 3, 3, 3, 3, 3)
    grid, eps, kap, pec = _box_and_sheet_scene(shape)
    dt = grid.courant_dt()
    n = _steps(shape)
    nrows = _numpy_class_rows(grid, eps, kap, pec, dt)
    assert 3 < nrows < 300
    eo, pvo, pio = _engine(oracle_lib, grid, eps, kap, pec, dt, cells, None, nsteps=n)
    _seed_global([eo], shape)
    _run_cut(eo, n)
    fo, uo, io, wo, opo = eo.fields(), eo.get_probe(pvo), eo.get_probe(pio), eo.energy(), eo.get_operator()
    assert np.abs(fo).max() > 0
    for rows_on in (True, False):
        for operator in ("build", "set_classes"):
            if not rows_on:
                monkeypatch.setenv("FDTD_CLASS_ROWS", "0")
            e, pv, pi = _engine(hip_lib, grid, eps, kap, pec, dt, cells, None, flags=capi.FLAG_KERNEL_WAVEFRONT, nsteps=n, operator=operator)
            monkeypatch.delenv("FDTD_CLASS_ROWS", raising=False)
            assert e.operator_form()[0] == "classes-packed"
            info = e.traffic_info()
            print("rows_on", rows_on, operator, info)
            assert info["class_rows"] == (nrows if rows_on else 0)
            for a, b in zip(e.get_operator(), opo):
                assert np.array_equal(a, b)
            _seed_global([e], shape)
            _run_cut(e, n)
            assert np.array_equal(e.fields(), fo), (rows_on, operator)
            assert _close(e.get_probe(pv), uo) and _close(e.get_probe(pi), io) and _close(e.energy(), wo)


def test_class_rows_that_are_all_distinct_keep_the_per_cell_bytes(hip_lib, oracle_lib, monkeypatch):
    """4096 x 19 x 17 nodes with two classes drawn at random per interior edge: 323 rows of 4096 bytes, of which the 288 away from the
    y and z faces are all distinct (a face row holds no edge to draw on) — 1.125 MiB of patterns, above the 1 MiB the row form is taken
    for.  The context says so (0 rows) and steps with the per-cell bytes, equal to the oracle."""
    capi, eco, grid_m = pkg("_capi"), pkg("ecoperator"), pkg("grid")
    monkeypatch.setenv("FDTD_RESIDENT", "0")
    shape = (4096, 19, 17)
    nx, ny, nz = shape
    grid = grid_m.RectGrid(*[np.arange(m) * 1e-3 for m in shape])
    dt = grid.courant_dt()
    op = eco.build_operator(grid, np.ones((nz - 1, ny - 1, nx - 1)), np.zeros((nz - 1, ny - 1, nx - 1)), np.zeros((3, nz, ny, nx), bool), dt, [])
    ecls, cls_vv, cls_m = op.classes()
    c0 = int(np.bincount(ecls.ravel()).argmax())                  # the vacuum edges; a second class with half their m (a denser medium)
    cls_vv, cls_m = np.append(cls_vv, cls_vv[c0]), np.append(cls_m, np.float32(0.5) * cls_m[c0])
    rng = np.random.default_rng(4)
    ecls = np.where((ecls == c0) & (rng.random(ecls.shape) < 0.5), len(cls_vv) - 1, ecls).astype(np.uint8)
    rows = np.ascontiguousarray(np.transpose(ecls, (1, 2, 0, 3))).reshape(nz * ny, 3 * nx)
    distinct = int(np.unique(rows, axis=0).shape[0])
    assert distinct >= (nz - 2) * (ny - 2) and distinct * nx > (1 << 20)   # (P = nx: patterns beyond 1 MiB)
    out = []
    for lib in (hip_lib, oracle_lib):
        e = capi.Engine(lib, nx, ny, nz, dt, max_steps=16, flags=capi.FLAG_KERNEL_WAVEFRONT if lib is hip_lib else 0)
        e.set_operator_classes(ecls, cls_vv, cls_m, *op.metric_tables())
        e.set_signal(np.zeros(4))
        seeded_fields(e, 8)
        for m in (1, 3):
            e.run(m)
        out.append(e)
    eh, eo = out
    assert eh.operator_form()[0] == "classes-packed"
    info = eh.traffic_info()
    print(info)
    assert info["class_rows"] == 0 and info["bytes_saved_per_timestep"] == 0
    fo = eo.fields()
    assert np.abs(fo).max() > 0 and np.array_equal(eh.fields(), fo)
