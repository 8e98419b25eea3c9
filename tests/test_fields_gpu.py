"""Field dumps on the GPU (csrc/fields.hip): fdtd_field_interp against fields.interp_spec bit for bit on the boxes of
fields_cases.INTERP_CASES — every kind, mode and stride, real samples and complex spectra, twice for identical bits; Simulation.field on
the HIP engine (device interpolation) against the oracle engine (the specification) in record and in dft mode, under the schedule the
planner picks and under the two-launch schedule; a run with an NF2FF box and a SAR box gives the same far field and SAR with and
without field boxes; AddFieldDump / GetFieldDump and the files through the openEMS API mirror."""
import json
import os

import numpy as np
import pytest

from conftest import pkg
import fields_cases as fc


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("name", sorted(fc.INTERP_CASES))
def test_device_interpolation_equals_the_specification_bit_for_bit(hip_lib, name, kind):
    capi = pkg("_capi")
    assert capi.has_fields(hip_lib)
    for cplx in (False, True):
        lines, lo, hi, rec, kap = fc.interp_inputs(name, cplx)
        for mode in fc.MODES:
            for sub in fc.STRIDES:
                want = fc.spec_call(kind, mode, lines, lo, hi, rec, kap, sub)
                got = capi.field_interp_raw(hip_lib, kind, mode, lines, lo, hi, rec, rec, kap if kind == "J" else None, sub)
                assert np.count_nonzero(want) > want.size // 4
                assert fc.same_bits(got, want), (cplx, mode, sub, float(np.abs(got - want).max()))
        again = capi.field_interp_raw(hip_lib, kind, mode, lines, lo, hi, rec, rec, kap if kind == "J" else None, sub)
        assert fc.same_bits(again, got)                             # two calls, identical bits
    if name == "67x5x3-cells":
        assert want.shape[1:] == (2, 3, 23) and np.prod(fc.spec_call(kind, 1, lines, lo, hi, rec, kap, (1, 1, 1)).shape[1:]) > 4 * 256


@pytest.mark.gpu
def test_bad_arguments_and_host_switch(hip_lib, monkeypatch):
    capi = pkg("_capi")
    lines, lo, hi, rec, kap = fc.interp_inputs("the-whole-grid", True)
    n = np.array([l.size for l in lines], np.int32)
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    p = capi._ptr
    out = np.empty((3,) + rec[0].shape, np.complex128)

    def call(kind=0, mode=1, parts=2, lo_=lo, hi_=hi, sub=(1, 1, 1), x=lines[0], k=None):
        a = [i32(n), i32(lo_), i32(hi_), i32(sub)]
        return hip_lib.fdtd_field_interp(0, kind, mode, parts, p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(x), p(lines[1]), p(lines[2]),
                                         p(rec[0]), p(rec[1]), p(rec[2]), k, k, k, p(out))
    assert call() == 0
    for bad, msg in ((dict(kind=4), "bad field_interp argument"), (dict(mode=3), "bad field_interp argument"),
                     (dict(parts=3), "bad field_interp argument"), (dict(kind=2), "bad field_interp argument"),     # J without kappa
                     (dict(hi_=(6, 4, 3)), "does not lie in the grid"), (dict(lo_=(-1, 0, 0)), "does not lie in the grid"),
                     (dict(sub=(1, 0, 1)), "does not lie in the grid"), (dict(mode=2, lo_=(0, 4, 0)), "at least one cell along axis 1"),
                     (dict(x=lines[0][::-1].copy()), "strictly increasing")):
        assert call(**bad) < 0 and msg in hip_lib.fdtd_last_error(None).decode(), bad
    with pytest.raises(ValueError, match="must cover the region"):
        capi.field_interp_raw(hip_lib, "E", 1, lines, lo, hi, [r[1:] for r in rec])
    assert capi.fields_device(hip_lib) is not None
    monkeypatch.setenv("FDTD_FIELDS", "host")
    assert capi.fields_device(hip_lib) is None


# ---- 2. through Simulation -------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle_dumps(oracle_lib, mode):
    """The oracle engine with the specification, once per recording mode: {box: FieldDump at 2 GHz}, and the final fields."""
    if mode not in _ORACLE:
        s = fc.e2e_sim(mode)
        s.build(oracle_lib)
        s.run(max_steps=fc.E2E_STEPS)
        _ORACLE[mode] = ({name: s.field(name) for name in fc.E2E_BOXES}, s.engine.fields())
    return _ORACLE[mode]


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["auto", "two-launch"])
@pytest.mark.parametrize("mode", ["record", "dft"])
def test_simulation_field_device_against_oracle_engine(hip_lib, oracle_lib, mode, schedule, monkeypatch):
    capi = pkg("_capi")
    want, fields_o = _oracle_dumps(oracle_lib, mode)
    s = fc.e2e_sim(mode)
    s.build(hip_lib, flags=capi.FLAG_KERNEL_AUTO if schedule == "auto" else capi.FLAG_KERNEL_DIRECT)
    stats = s.run(max_steps=fc.E2E_STEPS)
    assert s.nf2ff_mode == mode and np.array_equal(s.engine.fields(), fields_o)
    for name, kw in fc.E2E_BOXES.items():
        g, w = s.field(name), want[name]
        assert g.device and not w.device and g.type == kw["kind"] and g.mode == kw["mode"] and g.freq == w.freq == 2e9
        assert g.field.shape == w.field.shape and all(np.array_equal(a, b) for a, b in zip((g.x, g.y, g.z), (w.x, w.y, w.z)))
        top = float(np.abs(w.field).max())
        err = float(np.abs(g.field - w.field).max()) / top
        print(f"{name} ({mode}, {schedule}): largest difference {err:.3e} of the dump's largest magnitude")
        assert top > 0 and err <= 1e-12
        rep = stats.fields[name]
        assert rep["device"] is True and rep["seconds"] > 0 and rep["points"] == list(g.field.shape[:0:-1])
    assert want["h"].field.shape == (3, 2, 9, 7)
    # FDTD_FIELDS=host on the HIP engine: the specification on the same spectra has the device's bits
    monkeypatch.setenv("FDTD_FIELDS", "host")
    for name in fc.E2E_BOXES:
        g = s.field(name)
        monkeypatch.delenv("FDTD_FIELDS")
        d = s.field(name)
        monkeypatch.setenv("FDTD_FIELDS", "host")
        assert not g.device and d.device and fc.same_bits(g.field, d.field)
    if mode == "record":                      # any frequency of the band afterwards
        assert np.abs(s.field("e", 1.6e9).field - s.field("e").field).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["record", "dft"])
def test_field_boxes_leave_far_field_and_sar_alone(hip_lib, mode):
    nf = pkg("nf2ff")
    res = []
    for with_fields in (False, True):
        s = fc.e2e_sim(mode, nf2ff=True, sar=True, fields=with_fields)
        s.build(hip_lib)
        s.run(max_steps=fc.E2E_STEPS)
        boxes = s.nf2ff_boxes()
        ff = nf.calc_nf2ff(hip_lib, s.nf2ff_box, [b[-1:] for b in boxes], [fc.E2E_FREQS[-1]], np.linspace(0, np.pi, 7), np.linspace(0, 2 * np.pi, 9),
                           [23e-3, 19e-3, 15e-3])
        res.append((ff, s.sar("block"), s.field("roth") if with_fields else None))
    (ff0, sar0, _), (ff1, sar1, dump) = res
    assert dump.device and np.abs(dump.field).max() > 0
    for a in ("E_theta", "E_phi", "P_rad"):
        assert np.abs(getattr(ff0, a)[0]).max() > 0 and fc.same_bits(np.asarray(getattr(ff0, a)[0]), np.asarray(getattr(ff1, a)[0])), a
    assert fc.same_bits(np.asarray(ff0.Prad), np.asarray(ff1.Prad)) and fc.same_bits(np.asarray(ff0.Dmax), np.asarray(ff1.Dmax))
    for a in ("sar_local", "sar_avg", "half_side", "status"):
        assert fc.same_bits(getattr(sar0, a), getattr(sar1, a)), a
    assert sar0.P_abs == sar1.P_abs and sar0.peak == sar1.peak and sar0.counts == sar1.counts and sar0.counts["valid"] > 20


# ---- 3. through the openEMS API mirror -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_add_field_dump_through_the_api_mirror(hip_lib, tmp_path):
    from test_fields_cpu import _api_script
    api = pkg("openems_api")
    fd, _ = _api_script(api, hip_lib, nr_ts=fc.E2E_STEPS, nf2ff_mode="record")
    fd.AddFieldDump("Ef", 10, [10, 10, 10], [36, 28, 20], frequency=[2e9], file_type=0)
    fd.AddFieldDump("rotHt", 3, [16, 12, 8], [28, 24, 12], dump_mode=0, timesteps=[150, 290], file_type=1)
    out = str(tmp_path / "run")
    fd.Run(out)
    ef, rt = fd.GetFieldDump("Ef"), fd.GetFieldDump("rotHt", timestep=290)
    assert ef.device and rt.device and rt.field.dtype == np.float64 and np.abs(rt.field).max() > 0
    # the same boxes through Simulation: identical bits
    s = fc.e2e_sim("record", fields=False)
    s.add_field_box("Ef", (10e-3,) * 3, (36e-3, 28e-3, 20e-3), "E", freqs=[2e9])
    s.build(hip_lib)
    s.run(max_steps=fc.E2E_STEPS)
    assert fc.same_bits(s.field("Ef").field, ef.field)
    rep = json.load(open(os.path.join(out, "fdtd_hip_run.json")))["fields"]
    assert rep["Ef"]["device"] is True and rep["Ef"]["points"] == [14, 10, 6] and rep["Ef"]["seconds"] > 0 and rep["rotHt"]["files"] == ["rotHt.npz"]
    x, y, z, vec = fc.read_vtk(os.path.join(out, rep["Ef"]["files"][0]))
    assert np.array_equal(x, ef.x) and np.array_equal(vec["E-field_re"], ef.field.real) and np.array_equal(vec["E-field_im"], ef.field.imag)
    with np.load(os.path.join(out, "rotHt.npz")) as f:
        assert f["timestep"].tolist() == [fd.GetFieldDump("rotHt").timestep, rt.timestep] and np.array_equal(f["field"][1], rt.field)
    assert any(c["op"] == "AddFieldDump" and c["dump_type"] == 3 for c in fd.calls)
