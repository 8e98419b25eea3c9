"""Sub-cell averaged dielectric surfaces on the GPU: fdtd_voxel_subcell (csrc/voxel.hip) against subcell.edges_spec, list and bits; a
dielectric sphere beside a lumped port end to end against the oracle under every schedule; the same with conformal metal against the
restated correction and against the equivalent raw operator; the host switch."""
import numpy as np
import pytest

from conftest import pkg
import primitives_cases as pc
import subcell_cases as sc_
from opbuild_cases import same_bits

pytestmark = pytest.mark.gpu
STEPS = 60


def _device(hip_lib, grid, table, nsub, tabs, skip):
    return pkg("_capi").subcell_raw(hip_lib, grid, table, nsub, *tabs, skip)


@pytest.mark.parametrize("nsub", [2, 4, 8])
@pytest.mark.parametrize("kind", sc_.KINDS)
def test_device_list_equals_the_specification_bit_for_bit(hip_lib, kind, nsub):
    grid = pc.grid_of(13, 11, 9)
    table, tabs, skip, want = sc_.spec_of(sc_.one_primitive(kind, grid), grid, nsub)
    got = _device(hip_lib, grid, table, nsub, tabs, skip)
    print(f"{kind} nsub {nsub}: {want.edges()} listed")
    assert len(want) > (20 if kind != "smaller-than-a-cell" else 0)
    assert np.array_equal(got.comp, want.comp) and np.array_equal(got.idx, want.idx)
    assert sc_.same_listed(got, want)


@pytest.mark.parametrize("nsub", [2, 4])
def test_every_pass_spans_several_blocks(hip_lib, nsub):
    sub = pkg("subcell")
    grid, scene = sc_.large_case()
    table, tabs, skip, want = sc_.spec_of(scene, grid, nsub)
    # skip marks: a few live edges carry an override, as a port's would
    rng = np.random.default_rng(5)
    pick = rng.choice(len(want), 40, replace=False)
    skip2 = sub.skip_mask(grid, np.zeros((3,) + grid.shape[::-1], bool), want.idx[pick], want.comp[pick])
    want2 = sub.edges_spec(grid, table, nsub, *tabs, skip2)
    assert len(want) > 10000 and len(want2) == len(want) - 40 and want2.dropped_lumped == 40
    for sk, w in ((skip, want), (skip2, want2)):
        assert sc_.same_listed(_device(hip_lib, grid, table, nsub, tabs, sk), w)


def test_a_dispersive_owner_and_bad_arguments(hip_lib):
    capi, sub, prims = pkg("_capi"), pkg("subcell"), pkg("primitives")
    grid = pc.grid_of(23, 21, 9)
    scene = pc.all_types_scene(grid, sc_.EXT)                       # a Debye shell that ties with a lens, a magnetic rod, metals of every type
    table, tabs, skip, want = sc_.spec_of(scene, grid, 4)
    assert want.dropped_nonplain > 50 and len(want) > 500
    assert sc_.same_listed(_device(hip_lib, grid, table, 4, tabs, skip), want)
    empty = prims.pack_table(pkg("scene").Scene(unit=sc_.UNIT), grid)
    assert len(_device(hip_lib, grid, empty, 4, sub.prop_tables(pkg("scene").Scene()), skip)) == 0
    with pytest.raises(ValueError, match="subcell_samples"):
        _device(hip_lib, grid, table, 3, tabs, skip)
    with pytest.raises(capi.FdtdError, match="has material"):
        _device(hip_lib, grid, table, 4, tuple(t[-2:] for t in tabs), skip)      # fewer materials than the records name
    mapped = prims.Table(table.rec, table.verts, table.tol, [], table.names, np.ones(table.rec.size, np.int32), [])
    with pytest.raises(capi.FdtdError, match="delimits a voxel map"):
        _device(hip_lib, grid, mapped, 4, tabs, skip)


def test_host_switch_gives_the_device_paths_list(hip_lib, monkeypatch):
    capi, sc = pkg("_capi"), pkg("scene")
    grid, scene = sc_.sphere_port_scene()
    monkeypatch.delenv("FDTD_SUBCELL", raising=False)
    dev = capi.default_subcell(hip_lib)
    assert dev is not None
    a = sc.voxelize(scene, grid, subcell=4, device_subcell=dev).subcell
    monkeypatch.setenv("FDTD_SUBCELL", "host")
    assert capi.default_subcell(hip_lib) is None
    b = sc.voxelize(scene, grid, subcell=4, device_subcell=capi.default_subcell(hip_lib)).subcell
    assert len(a) > 100 and sc_.same_listed(a, b)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
_REF = {}


def _oracle_run(oracle_lib):
    if not _REF:
        s = sc_.sphere_port_sim(nr_ts=STEPS)
        e = s.build(oracle_lib)
        op = e.get_operator()
        e.run(STEPS)
        _REF["ref"] = (op, e.fields())
    return _REF["ref"]


# schedule -> (flags name, $FDTD_RESIDENT, $FDTD_WF_MULTI): the five the parity tests of sources and probes tell apart
SCHEDULES = {"auto": ("FLAG_KERNEL_AUTO", None, None), "resident": ("FLAG_KERNEL_RESIDENT", None, None), "two-launch": ("FLAG_KERNEL_DIRECT", "0", None),
             "one-timestep-per-launch": ("FLAG_KERNEL_WAVEFRONT", "0", "1"), "several-timesteps-per-launch": ("FLAG_KERNEL_WAVEFRONT", "0", "5")}


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_sphere_and_port_equal_the_oracle_under_every_schedule(hip_lib, oracle_lib, monkeypatch, schedule):
    capi = pkg("_capi")
    flag, resident, multi = SCHEDULES[schedule]
    flags = getattr(capi, flag)
    for name, val in (("FDTD_RESIDENT", resident), ("FDTD_WF_MULTI", multi)):
        monkeypatch.delenv(name, raising=False)
        if val is not None:
            monkeypatch.setenv(name, val)
    op_o, fields_o = _oracle_run(oracle_lib)
    s = sc_.sphere_port_sim(nr_ts=STEPS, device_subcell=capi.default_subcell(hip_lib))
    plain = sc_.sphere_port_sim(subcell=False, nr_ts=STEPS)
    e = s.build(hip_lib, flags=flags)
    assert e.backend.startswith("hip") and s.operator_build == "device"
    for name, a, b in zip(("vv", "vi", "ii", "iv"), e.get_operator(), op_o):
        assert same_bits(a, b), name
    base = plain.build(hip_lib, flags=flags)
    assert not same_bits(e.get_operator()[0], base.get_operator()[0]) or not same_bits(e.get_operator()[1], base.get_operator()[1])
    info = e.schedule_info()
    print(schedule, info, e.operator_form(), base.operator_form())
    if schedule in ("auto", "resident"):                          # a grid this small: AUTO keeps it resident in registers
        assert info["resident"] and info["launches_per_timestep"] == 1
    elif schedule == "two-launch":
        assert info["launches_per_timestep"] == 2 and not info["resident"]
    else:
        assert info["launches_per_timestep"] == 1 and not info["resident"]
        assert (info["timesteps_per_launch_max"] == 1) if multi == "1" else (info["timesteps_per_launch_max"] > 1)
    stats = s.run(max_steps=STEPS)
    assert np.abs(fields_o).max() > 0 and np.array_equal(e.fields(), fields_o)
    assert stats.subcell["nsub"] == 4 and sum(stats.subcell["edges"]) == len(s.subcell) > 100 and stats.subcell["dropped_lumped"] >= 1
    assert stats.subcell["operator_form"] == s.operator_form


def test_with_conformal_metal(hip_lib, oracle_lib):
    """The same scene with a metal sphere beside the dielectric one, conformal=True: the HIP run equals the restated correction on the
    oracle's half-steps bit for bit, and the equivalent raw operator (conformal.raw_operator over Simulation.op, the sub-cell overrides
    applied) stepped by the oracle to float32 rounding: both forms commit a few roundings of 2^-24 per value and timestep, at most
    4 * 60 * 2^-24 = 1.4e-5 of the field's size after 60 timesteps if every one of them added up — 2e-5 in the l2 norm of the currents
    (the variable both forms share; the raw form's voltages are f V)."""
    from restatement import Restatement
    from test_conformal_model_cpu import build_raw
    from helpers import rel_l2
    capi = pkg("_capi")
    mk = lambda **kw: sc_.sphere_port_sim(conformal=True, nr_ts=STEPS, **kw)
    s = mk(device_subcell=capi.default_subcell(hip_lib))
    assert s.conformal is not None and len(s.conformal) > 20 and len(s.subcell) > 100
    ref = Restatement(mk(), oracle_lib)
    ref.run(STEPS)
    e = s.build(hip_lib)
    e.run(STEPS)
    assert np.abs(ref.e.fields()).max() > 0 and np.array_equal(e.fields(), ref.e.fields())
    raw = build_raw(mk(), oracle_lib)
    raw.run(STEPS)
    err = rel_l2(e.fields()[1], raw.fields()[1])
    print(f"conformal + subcell, currents against the raw operator after {STEPS} steps: {err:.3e}")
    assert err <= 2e-5
