"""The post-processing kernels beyond their first chunk, on the GPU (cases, references and their conditions:
test_postprocessing_edges_cpu.py): k_sar_cube with cubes of more than 64 x cells and more than 64 columns against the
specification and against np.longdouble sums; k_farfield per direction against an np.longdouble reference and the oracle, tail
blocks, fewer directions than a block serves, fewer points than threads, none; k_rec_dft<8> past eight frequencies against the
running DFT, the oracle and single-frequency transforms; the four probe reductions on probes of up to 600 cells in every
strip-plane of the grid under every schedule."""
import numpy as np
import pytest

from conftest import pkg
from helpers import rel_l2, seeded_fields
from test_postprocessing_edges_cpu import (PRB_CALLS, PRB_STEPS, REC_NFREQ, REC_ROWS, REC_STEPS, U, _note_line, add_probes,
                                           check_valid_cubes_in_longdouble, draw_probes, farfield_cases, farfield_ratio, farfield_ref_of,
                                           probe_sim, probe_sum_longdouble, rec_freqs, rec_sim, sar_cases, sar_spec_of,
                                           strip_planes_covered)
from test_sar_gpu import _same_bits, average_matches_the_specification

pytestmark = pytest.mark.gpu


# ---- A. SAR averaging with cubes wider than a wave ---------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["ieee", "simple"])
@pytest.mark.parametrize("name", sorted(sar_cases()))
def test_device_average_of_cubes_wider_than_a_wave(hip_lib, name, method):
    """The comparison of test_sar_gpu.test_device_average_matches_the_specification (its helper) on cubes that take a second and a
    third chunk of x cells, a second chunk of columns, both; the status counts; then every voxel the device calls valid, at the
    device's own half_side, against sums in np.longdouble that do not go through the specification."""
    case = sar_cases()[name]
    spec = sar_spec_of(name, method)
    (g_sa, g_half, g_status, g_counts), near, worst = average_matches_the_specification(hip_lib, case, spec, method)
    assert not near.any() and np.array_equal(g_counts, spec[3])
    ld = check_valid_cubes_in_longdouble(case, g_sa, g_half, g_status)
    line = (f"sar_avg {worst[0]:.2e}, half_side {worst[1]:.2e} off the specification (relative, largest); "
            f"|P/m - sar_avg| / sar_avg against np.longdouble at most {ld:.2e}")
    print(f"{name} / {method}: {line}")
    _note_line("SAR, device against specification and np.longdouble (test_device_average_of_cubes_wider_than_a_wave)", f"{name} / {method}", line)


# ---- B. the far field per direction ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(farfield_cases()))
def test_farfield_per_direction_against_the_longdouble_reference(hip_lib, oracle_lib, name):
    """Every direction and component of a case inside K 2^-53 S_a (test_postprocessing_edges_cpu.farfield_K) of the np.longdouble
    reference: tail blocks of 1, 2 and 3 directions, fewer directions than the four a block serves, fewer points than the block
    has threads, one more, none (exact zeros), the poles; and inside twice the bar of the oracle, per direction."""
    capi = pkg("_capi")
    pos, Js, Ms, kw, th, ph = farfield_cases()[name]
    ref = farfield_ref_of(name)
    K = ref[3]
    got = capi.farfield(hip_lib, pos, Js, Ms, kw, th, ph)
    again = capi.farfield(hip_lib, pos, Js, Ms, kw, th, ph)
    assert all(_same_bits(a, b) for a, b in zip(got, again))
    assert all(g.shape == th.shape for g in got)
    if pos.shape[0] == 0:
        assert all(np.all(g.real == 0) and np.all(g.imag == 0) for g in got)
        return
    ora = capi.farfield(oracle_lib, pos, Js, Ms, kw, th, ph)
    r_dev, r_ora = farfield_ratio(got, ref), farfield_ratio(ora, ref)
    line = f"K = {K:.0f}; largest |err| / (2^-53 S_a): device {r_dev.max():.3f}, oracle {r_ora.max():.3f}"
    print(f"{name}: {line}")
    assert np.all(r_dev <= K), (int(np.argmax(r_dev)), r_dev.max())
    # device against oracle: each within the bar of the reference, so within twice the bar of each other
    both = farfield_ratio(got, (ora[0].astype(np.clongdouble), ora[1].astype(np.clongdouble), ref[2]))
    assert np.all(both <= 2 * K), (int(np.argmax(both)), both.max())
    _note_line("far field, device and oracle against the np.longdouble reference (test_farfield_per_direction_against_the_longdouble_reference)", name, line)


# ---- C. the recorder transform past eight frequencies ------------------------------------------------------------------------------
def test_recorder_transform_past_eight_frequencies(hip_lib, oracle_lib):
    """Recorded once on HIP and once on the oracle, transformed at 1, 8, 9, 16 and 17 frequencies (f0 > 0 and a partial last pass of
    k_rec_dft<8>): at 9 and 17 the same bits as running-DFT runs at those frequencies, per frequency row within 1e-12 of the oracle's
    recorder, and rows 0, 7, 8, 16 of the 17-frequency transform the bits of single-frequency transforms — on all 24 faces, among
    them boxes of 656 .. 3608 points, no multiples of the block."""
    sr, so = rec_sim("record", rec_freqs(17)), rec_sim("record", rec_freqs(17))
    er, eo = sr.build(hip_lib), so.build(oracle_lib)
    for n in (1, 120, 179):
        er.run(n)
    eo.run(REC_STEPS)
    assert er.step == eo.step == REC_STEPS and np.array_equal(er.fields(), eo.fields())
    got = {n: sr.nf2ff_boxes(freqs=rec_freqs(n)) for n in REC_NFREQ}
    assert len(got[17]) == 24 and any(b[0].size % 256 for b in got[17]) and all(b.shape[0] == 17 for b in got[17])
    for n in REC_NFREQ:
        want = so.nf2ff_boxes(freqs=rec_freqs(n))
        assert max(np.abs(b).max() for b in want) > 0
        for a, b in zip(got[n], want):
            assert a.shape == b.shape and a.shape[0] == n
            for q in range(n):
                assert rel_l2(a[q], b[q]) < 1e-12, (n, q, rel_l2(a[q], b[q]))
    for n in (9, 17):
        sd = rec_sim("dft", rec_freqs(n))
        assert (sd.dft_every, sd.dft_nsamples) == (sr.dft_every, sr.dft_nsamples)
        ed = sd.build(hip_lib)
        ed.run(REC_STEPS)
        for a, b in zip(got[n], sd.nf2ff_boxes()):
            assert _same_bits(a, b), n
    for q in REC_ROWS:
        one = sr.nf2ff_boxes(freqs=rec_freqs(17)[q:q + 1])
        for a, b in zip(got[17], one):
            assert _same_bits(np.ascontiguousarray(a[q]), np.ascontiguousarray(b[0])), q


# ---- D. long probes under every schedule -------------------------------------------------------------------------------------------
SCHEDULES = {       # name -> (boundary, build flag, environment, stepping)
    "auto": ("CPML", "AUTO", {}, "run"),
    "several-timesteps-per-launch": ("CPML", "AUTO", {"FDTD_RESIDENT": "0"}, "run"),
    "one-timestep-per-launch": ("CPML", "AUTO", {"FDTD_RESIDENT": "0", "FDTD_WF_MULTI": "1"}, "run"),
    "wavefront": ("CPML", "WAVEFRONT", {}, "run"),
    "direct": ("CPML", "DIRECT", {}, "run"),
    "half-steps": ("CPML", "DIRECT", {}, "half"),
    "resident-cpml": ("CPML", "RESIDENT", {}, "run"),
    "resident-mur": ("MUR", "RESIDENT", {}, "run"),
    "direct-mur": ("MUR", "DIRECT", {}, "run"),
}
_PRB = {}


def _probe_run(lib, boundary, flag="AUTO", stepping="run"):
    """(engine, fields, [series]) of the probe scene after PRB_STEPS timesteps from seeded fields, in calls of PRB_CALLS."""
    capi = pkg("_capi")
    probes = draw_probes(inner=boundary == "MUR")
    e = probe_sim(boundary).build(lib, flags=getattr(capi, "FLAG_KERNEL_" + flag))
    pids = add_probes(e, probes)
    seeded_fields(e, 9)
    if stepping == "half":
        for _ in range(PRB_STEPS):
            e.half_step(0)
            e.half_step(1)
    else:
        for n in PRB_CALLS:
            e.run(n)
    assert e.step == PRB_STEPS
    return e, e.fields(), [e.get_probe(p)[:PRB_STEPS] for p in pids]


def _oracle_probe_run(oracle_lib, boundary):
    if boundary not in _PRB:
        _PRB[boundary] = _probe_run(oracle_lib, boundary)[1:]
    return _PRB[boundary]




def _direct_probe_run(hip_lib, boundary):
    """The series under two launches per timestep (probe_block in k_post's place inside the update kernels), once per process and
    boundary: what every other schedule's series are compared with, bit for bit."""
    if ("direct", boundary) not in _PRB:
        _PRB[("direct", boundary)] = _probe_run(hip_lib, boundary, "DIRECT")[2]
    return _PRB[("direct", boundary)]


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_long_probes_under_every_schedule(hip_lib, oracle_lib, monkeypatch, name):
    """V- and I-probes of 1, 256, 257 and 600 entries (the strided loops of probe_block — in the update kernels and in k_post —,
    of wf_probe_tail plain and MULTI and of k_res_probes take a second and a third turn; the 257- and 600-entry ones have a cell
    in every strip-plane, so wf_probe_tail polls the flag of every one of them and every H strip-plane publishes): fields the
    oracle's bit for bit, every series within 1e-12 of the oracle's and identical in bits to the two-launch schedule's, the last
    sample within (ceil(n / 256) + 9) 2^-53 sum |w F| of the np.longdouble sum over the final fields (n / 256 strided fmas, 8
    tree levels, the conversion of w F is exact).
    NOT covered: k_probes (kernels.hip).  Its only launcher, launch_probes, has no caller — no schedule can reach it, so no test
    can; it states the same loop and tree as probe_block."""
    boundary, flag, env, stepping = SCHEDULES[name]
    direct = _direct_probe_run(hip_lib, boundary)                   # (before the environment of this schedule is set)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    probes = draw_probes(inner=boundary == "MUR")
    e, f, series = _probe_run(hip_lib, boundary, flag, stepping)
    info = e.schedule_info()
    if name == "auto":
        assert info["timesteps_per_launch_max"] > 1
    elif name == "several-timesteps-per-launch":
        assert info["timesteps_per_launch_max"] > 1 and not info["resident"] and info["launches_per_timestep"] == 1
    elif name == "one-timestep-per-launch":
        assert info["timesteps_per_launch_max"] == 1 and not info["resident"] and info["launches_per_timestep"] == 1
    elif name == "wavefront":
        assert not info["resident"] and info["launches_per_timestep"] == 1
    elif name.startswith("resident"):
        assert info["resident"]
    elif name.startswith("direct"):
        assert not info["resident"] and info["launches_per_timestep"] >= 2
    if boundary == "CPML" and not info["resident"]:
        for kind, idx, comp, w in probes:
            if idx.size > 256:
                assert strip_planes_covered(idx, info["rows_per_strip"]), info
    fo, so = _oracle_probe_run(oracle_lib, boundary)
    assert np.abs(fo).max() > 0 and np.array_equal(f, fo)
    worst = 0.0
    for (kind, idx, comp, w), got, want in zip(probes, series, so):
        assert got.size == want.size == PRB_STEPS and np.abs(want).max() > 0
        assert rel_l2(got, want) < 1e-12, (name, kind, idx.size, rel_l2(got, want))
        ref, scale = probe_sum_longdouble(f, kind, idx, comp, w)
        dev = float(abs(np.longdouble(got[-1]) - ref)) / (U * scale)
        worst = max(worst, dev)
        assert dev <= -(-idx.size // 256) + 9, (name, kind, idx.size, dev)
    # identical bits across the HIP schedules of a scene: each against the two-launch schedule's
    for a, b in zip(series, direct):
        assert _same_bits(a, b), name
    line = f"last sample against the np.longdouble sum over the final fields at most {worst:.3f} x 2^-53 sum |w F|"
    print(f"{name}: {line}")
    _note_line("probes of 1 / 256 / 257 / 600 entries (test_long_probes_under_every_schedule)", name, line)
