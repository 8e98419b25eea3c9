"""Anisotropic dielectrics on the GPU: fdtd_build_operator_axes (csrc/opbuild.hip) against the operator composed from three isotropic
oracle builds, bit for bit, in all three device forms and on z-slabs; a patch on a uniaxial lossy substrate built on the device, from
host arrays and on the oracle; the scenes that see one axis only; a raw J dump with the per-axis edge conductivities."""
import numpy as np
import pytest

from conftest import pkg
import anisotropic_cases as ac
from opbuild_cases import random_scene, engine_with_built_operator, same_bits

pytestmark = pytest.mark.gpu

# (seed, shape, graded, materials) -> the device form at world = 1, from the numpy counts of distinct pairs / triples (the existing
# seeds of test_operator_build_gpu.py will not do: three palettes multiply the pairs).  Counted on the CPU with
# anisotropic_cases.pair_and_triple_counts: 17 / 135, 212 / 2883, 916 / 4459, 12462 / 7317.
FORM_CASES = [
    (1, (37, 30, 22), False, 2, "classes-packed"),
    (4, (34, 29, 21), False, 5, "classes"),
    (4, (34, 29, 21), False, 8, "raw"),
    (2, (33, 27, 19), True, 8, "raw"),
]
_COMPOSED = {}


def _composed_spec(seed, shape, graded, nmat):
    """The scene and (vv, m) of the specification composed from its three isotropic builds, once per scene."""
    key = (seed, shape, graded, nmat)
    if key not in _COMPOSED:
        eco = pkg("ecoperator")
        grid, eps, kap, pec, lumped = ac.aniso_random_scene(seed, shape, graded, nmat)
        iso = [eco.build_operator(grid, eps[c], kap[c], pec, grid.courant_dt(), lumped) for c in range(3)]
        _COMPOSED[key] = ((grid, eps, kap, pec, lumped), np.stack([iso[c].vv[c] for c in range(3)]), np.stack([iso[c].m[c] for c in range(3)]))
    return _COMPOSED[key]


# ---- 5. fdtd_build_operator_axes against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,shape,graded,nmat,expect", FORM_CASES)
@pytest.mark.parametrize("world,rank", [(1, 0), (3, 0), (3, 1), (3, 2)])
def test_build_operator_axes_matches_three_oracle_builds(hip_lib, oracle_lib, seed, shape, graded, nmat, expect, world, rank):
    capi = pkg("_capi")
    assert capi.has_aniso(hip_lib) and not capi.has_aniso(oracle_lib)
    (grid, eps, kap, pec, lumped), vv, m = _composed_spec(seed, shape, graded, nmat)
    dt = grid.courant_dt()
    eh, k0, nk = ac.engine_with_built_operator_axes(hip_lib, grid, eps, kap, pec, lumped, dt, rank=rank, world=world)
    assert eh.backend.startswith("hip")
    ref = ac.composed_oracle_operator(oracle_lib, grid, eps, kap, pec, lumped, dt, rank=rank, world=world)
    for name, a, b in zip(("vv", "vi", "ii", "iv"), eh.get_operator(), ref):
        assert same_bits(a, b), name
    pairs, triples = ac.pair_and_triple_counts(vv[:, k0:k0 + nk], m[:, k0:k0 + nk])
    form, ncls = eh.operator_form()
    print(f"seed {seed} world {world} rank {rank}: {pairs} pairs, {triples} triples -> {form}, {ncls}")
    assert (form, ncls) == (("raw", 0) if pairs > 256 else ("classes", pairs) if triples > 256 else ("classes-packed", pairs))
    if world == 1:
        assert form == expect


@pytest.mark.parametrize("seed,shape,graded,nmat", [(1, (37, 30, 22), False, 3), (4, (34, 29, 21), False, 8), (2, (33, 27, 19), True, 8)])
@pytest.mark.parametrize("world,rank", [(1, 0), (3, 1)])
def test_three_equal_arrays_give_the_bits_and_form_of_build_operator(hip_lib, seed, shape, graded, nmat, world, rank):
    grid, eps, kap, pec, lumped = random_scene(seed, shape, graded, nmat)
    dt = grid.courant_dt()
    e1, _, _ = engine_with_built_operator(hip_lib, grid, eps, kap, pec, lumped, dt, rank=rank, world=world)
    e3, _, _ = ac.engine_with_built_operator_axes(hip_lib, grid, np.stack([eps] * 3), np.stack([kap] * 3), pec, lumped, dt, rank=rank, world=world)
    for name, a, b in zip(("vv", "vi", "ii", "iv"), e3.get_operator(), e1.get_operator()):
        assert same_bits(a, b), name
    assert e3.operator_form() == e1.operator_form()


def test_build_operator_axes_argument_errors(hip_lib, oracle_lib):
    capi, eco, const = pkg("_capi"), pkg("ecoperator"), pkg("constants")
    grid, eps, kap, pec, lumped = ac.aniso_random_scene(7, (10, 9, 8), False, 2)
    dt = grid.courant_dt()
    with pytest.raises(ValueError, match="per-axis cell arrays"):
        ac.engine_with_built_operator_axes(hip_lib, grid, eps, kap[0], pec, [], dt)
    with pytest.raises(capi.FdtdError, match="does not export fdtd_build_operator_axes"):
        ac.engine_with_built_operator_axes(oracle_lib, grid, eps, kap, pec, [], dt)
    e, _, _ = ac.engine_with_built_operator_axes(hip_lib, grid, eps, kap, pec, [], dt)
    emet, hmet = eco.pack_metric_tables(*eco.metric_lists(grid, dt), grid)
    bad = (np.array([10 ** 9], np.int64), np.array([0], np.int8), np.array([0.5], np.float32), np.array([1.0], np.float32))
    with pytest.raises(capi.FdtdError, match="out of range"):
        e.build_operator_axes(grid.d, eps, kap, pec, const.EPS0, bad, emet, hmet)


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------
_PATCH_REF = {}


def _patch_reference(oracle_lib):
    """The patch from host arrays on the oracle, its sheet and element corrections restated in numpy (restatement.py), once:
    (expanded operator, fields after PATCH_STEPS)."""
    if not _PATCH_REF:
        from restatement import Restatement
        sim = ac.aniso_patch_sim()
        ref = Restatement(sim, oracle_lib)
        assert sim.operator_build == "host" and ref.sheets is not None and ref.elements is not None
        op = ref.e.get_operator()
        ref.run(ac.PATCH_STEPS)
        _PATCH_REF["ref"] = (op, ref.e.fields())
    return _PATCH_REF["ref"]


@pytest.mark.parametrize("schedule", ["default", "two-launch"])
def test_patch_on_a_uniaxial_substrate_three_ways(hip_lib, oracle_lib, schedule):
    capi = pkg("_capi")
    flags = capi.FLAG_KERNEL_AUTO if schedule == "default" else capi.FLAG_KERNEL_DIRECT
    op_o, fields_o = _patch_reference(oracle_lib)
    dev, host = ac.aniso_patch_sim(), ac.aniso_patch_sim()
    host.device_operator = False
    assert dev.anisotropic and len(dev.vox.lumped) > 0 and len(dev.sheets) > 0 and dev.element_stepped.size > 0
    sub = dev.vox.cell_material == dev.vox.material_names.index("substrate")
    assert sub.any() and all(np.all(dev.vox.eps_axes[c][sub] == ac.PATCH_EPS[c]) for c in range(3)) and len(set(dev.vox.kappa_axes[:, sub][:, 0])) == 2
    ed, eh = dev.build(hip_lib, flags=flags), host.build(hip_lib, flags=flags)
    assert dev.operator_build == "device" and host.operator_build == "host"
    for name, a, b, c in zip(("vv", "vi", "ii", "iv"), ed.get_operator(), eh.get_operator(), op_o):
        assert same_bits(a, b) and same_bits(a, c), name
    assert ed.operator_form()[0] == "classes-packed" and eh.operator_form()[0] == "classes-packed"      # as the isotropic patch
    assert ed.operator_form()[1] == eh.operator_form()[1]
    stats = dev.run(max_steps=ac.PATCH_STEPS)
    eh.run(ac.PATCH_STEPS)
    fd, fh = ed.fields(), eh.fields()
    assert np.abs(fields_o).max() > 0 and np.array_equal(fd, fh) and np.array_equal(fd, fields_o)
    assert stats.anisotropic == {"materials": ["substrate"], "cells": int(sub.sum()), "operator_build": "device"}


# ---- 7. the scenes that see one axis only, on the device ----------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_invariant_scene_on_the_device_equals_the_oracles_isotropic_run(hip_lib, oracle_lib, axis):
    eps, kappa = ac.INVARIANT_EPS, ac.INVARIANT_KAPPA
    a1, a2 = (axis + 1) % 3, (axis + 2) % 3
    probe_i, fields_i, _ = ac.invariant_run(oracle_lib, axis, eps[axis], kappa[axis])
    assert not fields_i[0][a1].any() and not fields_i[0][a2].any() and np.abs(fields_i[0][axis]).max() > 1e-3      # the precondition
    probe_a, fields_a, sim = ac.invariant_run(hip_lib, axis, eps, kappa)
    assert sim.anisotropic and sim.operator_build == "device" and sim.engine.backend.startswith("hip")
    assert np.array_equal(probe_a, probe_i) and np.array_equal(fields_a, fields_i)


# ---- 8. a raw J dump over the anisotropic lossy block ----------------------------------------------------------------------------------
def test_raw_current_density_dump_uses_the_per_axis_edge_conductivities(hip_lib, monkeypatch):
    from test_sar_model_cpu import block_scene
    import fields_cases as fc
    sc, sim, eco, fields = pkg("scene"), pkg("simulation"), pkg("ecoperator"), pkg("fields")
    grid, s = block_scene(kappa=(0.8, 1.2, 2.0))
    m = sim.Simulation(grid, sc.voxelize(s, grid), f0=2e9, fc=1e9, boundary="CPML", cpml_cells=4, nr_ts=300, nf2ff_mode="record")
    box = dict(start=(10e-3, 10e-3, 8e-3), stop=(36e-3, 28e-3, 22e-3))
    m.add_field_box("j", kind="J", mode=0, freqs=[2e9], **box)
    m.add_field_box("e", kind="E", mode=0, freqs=[2e9], **box)
    m.build(hip_lib)
    m.run(max_steps=300)
    got = m.field("j")
    assert got.device and np.abs(got.field).max() > 0
    monkeypatch.setenv("FDTD_FIELDS", "host")
    want = m.field("j")
    assert not want.device and fc.same_bits(got.field, want.field)
    # the specification itself, on the edge conductivities of the axes: kap_e of component c averages kappa[c]
    b = m.field_boxes["j"]
    sl = tuple(slice(b["rlo"][a], b["hi"][a] + 1) for a in (2, 1, 0))
    kap = [np.ascontiguousarray(eco._edge_average(m.vox.kappa_axes[c], grid, c)[sl]) for c in range(3)]
    assert all(np.array_equal(k, np.ascontiguousarray(q[sl])) for k, q in zip(kap, m.edge_conductivity()))
    scalar = [np.ascontiguousarray(eco._edge_average(m.vox.kappa, grid, c)[sl]) for c in range(3)]
    assert not np.array_equal(kap[0], scalar[0]) and not np.array_equal(kap[2], scalar[2])
    scale = 2.0 * m.dt * m.dft_every
    tw = pkg("excitation").dft_twiddles(np.array([2e9]), m.dt, m.dft_every, m.dft_nsamples, 0.0)
    V = [m.engine.rec_transform(q, tw)[0][0] * scale for q in m._field_ids["j"]]
    spec = fields.interp_spec("J", 0, grid.lines, b["lo"], b["hi"], V=V, I=None, kappa=kap, sub=b["sub"])
    assert fc.same_bits(got.field, spec)
    assert not fc.same_bits(got.field, fields.interp_spec("J", 0, grid.lines, b["lo"], b["hi"], V=V, I=None, kappa=scalar, sub=b["sub"]))
