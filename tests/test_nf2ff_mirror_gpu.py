"""NF2FF mirror planes on the GPU: k_farfield_mirror (fdtd_farfield_mirror) per direction against the np.longdouble reference of the
duplicated point set, its bits against k_farfield's with no plane, the half-space zeros, and one quarter scene end to end through
Simulation on the HIP library.  Cases, references and bars: test_nf2ff_mirror_cpu.py."""
import numpy as np
import pytest

from conftest import pkg
from test_nf2ff_mirror_cpu import (BAR, HALF_CASES, PEC, PMC, _note, half_space_case, half_whole_differences, mirror_cases, mirror_ref_of,
                                   run_scene, symmetric_scene)
from test_postprocessing_edges_cpu import farfield_cases, farfield_ratio
from test_sar_gpu import _same_bits

pytestmark = pytest.mark.gpu


# ---- 6. the kernel against the reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mirror_cases()))
def test_kernel_per_direction_against_the_longdouble_reference(hip_lib, name):
    """Every direction and component inside K 2^-53 S_a (farfield_K of the duplicated set) of the np.longdouble sum over the
    duplicated set: 0, 1, 255, 256, 257, 3000 points, 1, 5, 7 directions and both poles (tail blocks of FF_DIRS = 4), m = 1, 2, 3
    planes of mixed types, a point on a plane; the same bits on a second call; and within twice the bar of the specification."""
    capi, nf = pkg("_capi"), pkg("nf2ff")
    assert capi.has_farfield_mirror(hip_lib)
    pos, Js, Ms, kw, th, ph, mirrors, half = mirror_cases()[name]
    ref = mirror_ref_of(name)
    got = capi.farfield_mirror(hip_lib, pos, Js, Ms, kw, th, ph, mirrors, half)
    again = capi.farfield_mirror(hip_lib, pos, Js, Ms, kw, th, ph, mirrors, half)
    assert all(_same_bits(a, b) for a, b in zip(got, again))
    assert all(g.shape == th.shape for g in got)
    if pos.shape[0] == 0:
        assert all(np.all(g.real == 0) and np.all(g.imag == 0) for g in got)
        return
    spec = nf.farfield_mirror_spec(pos, Js, Ms, kw, th, ph, mirrors, half)
    r_dev, r_spec = farfield_ratio(got, ref), farfield_ratio(spec, ref)
    line = f"K = {ref[3]:.0f}; largest |err| / (2^-53 S_a): device {r_dev.max():.3f}, specification {r_spec.max():.3f}"
    print(f"{name}: {line}")
    _note(f"kernel against np.longdouble, {name}", line)
    assert np.all(r_dev <= ref[3]), (int(np.argmax(r_dev)), r_dev.max())
    both = farfield_ratio(got, (spec[0].astype(np.clongdouble), spec[1].astype(np.clongdouble), ref[2]))
    assert np.all(both <= 2 * ref[3]), (int(np.argmax(both)), both.max())


# ---- 7. no planes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in farfield_cases() if n.startswith("257pts")])
def test_no_planes_is_bit_for_bit_fdtd_farfield(hip_lib, name):
    capi = pkg("_capi")
    pos, Js, Ms, kw, th, ph = farfield_cases()[name]
    plain = capi.farfield(hip_lib, pos, Js, Ms, kw, th, ph)
    got = capi.farfield_mirror(hip_lib, pos, Js, Ms, kw, th, ph, ())
    assert all(_same_bits(a, b) for a, b in zip(got, plain))
    assert np.abs(plain[0]).max() > 0


# ---- 8. the half space --------------------------------------------------------------------------------------------------------------
def test_half_space_zeros_are_exact_and_the_horizon_is_kept(hip_lib):
    capi = pkg("_capi")
    pos, Js, Ms, kw, th, ph, mirrors, half = half_space_case()
    ref = mirror_ref_of("half-space")
    got = capi.farfield_mirror(hip_lib, pos, Js, Ms, kw, th, ph, mirrors, half)
    below = np.cos(th) < 0
    assert below.sum() == 4 and th[2] == th[3] == np.pi / 2 and not below[2]
    for g in got:
        assert np.all(g.real[below] == 0) and np.all(g.imag[below] == 0)
    assert np.all(np.abs(got[0][~below]) + np.abs(got[1][~below]) > 0)
    assert farfield_ratio(got, ref).max() <= ref[3]
    # seen from a ground above the points the other directions are behind, theta = 90 deg still in front
    got_up = capi.farfield_mirror(hip_lib, pos, Js, Ms, kw, th, ph, [(0, PMC, -0.055), (2, PEC, 0.06)], 1)
    above = np.cos(th) > 1e-15
    for g in got_up:
        assert np.all(g[above] == 0)
    assert np.all(np.abs(got_up[0][~above]) + np.abs(got_up[1][~above]) > 0)
    # a whole block of four directions behind the plane (the block skips its points), next to one in front
    th5, ph5 = np.array([2.0, 2.5, 3.0, 1.7, 0.4]), np.array([0.1, 0.2, 0.3, 0.4, 0.5])
    got5 = capi.farfield_mirror(hip_lib, pos, Js, Ms, kw, th5, ph5, mirrors, half)
    one = capi.farfield_mirror(hip_lib, pos, Js, Ms, kw, th5[4:], ph5[4:], mirrors, half)
    assert np.all(got5[0][:4] == 0) and np.all(got5[1][:4] == 0) and _same_bits(got5[0][4:], one[0]) and _same_bits(got5[1][4:], one[1])
    # the argument checks come back as errors
    for bad, kw_bad in ((dict(mirrors=[(2, PEC, 0.0)], half_space=0), "both sides"), (dict(mirrors=mirrors, half_space=0), "PEC plane"),
                        (dict(mirrors=[(2, PEC, 0.0), (2, PMC, 0.1)]), "two mirror planes"), (dict(mirrors=[(3, PEC, 0.0)]), "axis 3"),
                        (dict(mirrors=[(1, 0, 0.0)]), "type 0"), (dict(mirrors=mirrors, half_space=2), "half-space plane 2")):
        with pytest.raises(capi.FdtdError, match=kw_bad):
            capi.farfield_mirror(hip_lib, pos, Js, Ms, kw, th, ph, **bad)


# ---- 9. end to end on the device ----------------------------------------------------------------------------------------------------
def test_quarter_scene_end_to_end_on_the_device(hip_lib, oracle_lib):
    """The quarter scene (PMC x-, PEC z-) of test_half_with_mirrors_equals_the_whole through Simulation on the HIP library, far field
    by k_farfield_mirror: within 1e-11 of max |E| of the same scene on the oracle with the specification (DESIGN's GPU = oracle
    far-field bar), and within the half = whole bar of the whole scene run on the HIP library with its closed box."""
    name = "quarter-pmc-x-pec-z"
    whole, half, centre = symmetric_scene(HALF_CASES[name])
    dt = pkg("grid").RectGrid(*whole["lines"]).courant_dt()
    rd, sd, _ = run_scene(half, hip_lib, dt, centre)
    ro, _, _ = run_scene(half, oracle_lib, dt, centre)
    rw, _, _ = run_scene(whole, hip_lib, dt, centre)
    assert pkg("_capi").has_farfield_mirror(hip_lib) and not pkg("_capi").has_farfield_mirror(oracle_lib) and sd.nf2ff_box.power_factor == 4.0
    dE_o, dP_o, dD_o = half_whole_differences(rd, ro)
    dE_w, dP_w, dD_w = half_whole_differences(rd, rw)
    line = (f"device half against oracle half: E {dE_o:.2e} of max |E|, Prad {dP_o:.2e}, Dmax {dD_o:.2e}; device half against device whole: "
            f"E {dE_w:.2e}, Prad {dP_w:.2e}, Dmax {dD_w:.2e}")
    print(line)
    _note(f"end to end on the device, {name}", line)
    assert dE_o <= 1e-11 and dP_o <= 1e-11 and dD_o <= 1e-11
    assert dE_w <= BAR["E"] and dP_w <= BAR["Prad"] and dD_w <= BAR["Dmax"], (dE_w, dP_w, dD_w)
