"""SAR on the GPU (csrc/sar.hip): fdtd_sar_local against sar.local_spec bit for bit; fdtd_sar_average against sar.average_spec on the
boxes of test_sar_model_cpu.gpu_cases under both methods, and twice for identical bits; Simulation.sar on the HIP engine (device
averaging) against the oracle engine (the specification) in record and in dft mode, and the FDTD_SAR=host switch; AddDump / GetSAR
through the openEMS API mirror against the Simulation path."""
import numpy as np
import pytest

from conftest import pkg
from test_sar_model_cpu import BLOCK_BOX, MARGIN, MAX_EXCLUDED, block_sim, gpu_cases, graded, spec_of

# values and h*: float64 sums of at most a few thousand non-negative terms in another order (<= 1e-12) plus 48 bisection steps
RTOL = 1e-10


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 1. local SAR ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_local_sar_equals_the_specification_bit_for_bit(hip_lib):
    sar, capi = pkg("sar"), pkg("_capi")
    assert capi.has_sar(hip_lib)
    n = (13, 11, 9)
    d = [graded(k, 71 + a) for a, k in enumerate(n)]
    rng = np.random.default_rng(74)
    nodes = tuple(k + 1 for k in n[::-1])
    V = [(rng.standard_normal(nodes) + 1j * rng.standard_normal(nodes)) * 10.0 ** rng.uniform(-6, -2, nodes) for _ in range(3)]
    for v in V:
        v[rng.random(nodes) < 0.15] = 0.0                           # PEC-like edges carry their zero
    V[0][2:5, 3:7, 4:9] = 0.0                                        # ... a whole metal block of them
    sigma = rng.uniform(0.0, 2.0, n[::-1]) * (rng.random(n[::-1]) < 0.8)
    rho = rng.uniform(900.0, 1200.0, n[::-1]) * (rng.random(n[::-1]) < 0.8)     # background cells, with and without sigma
    p, sl = sar.local_spec(*d, *V, sigma, rho)
    gp, gs = capi.sar_local_raw(hip_lib, *d, *V, sigma, rho)
    assert np.count_nonzero(p) > 500 and np.count_nonzero(sl) > 400 and np.count_nonzero((rho == 0) & (p > 0)) > 50
    assert _same_bits(gp, p) and _same_bits(gs, sl)
    with pytest.raises(capi.FdtdError, match="cell sizes"):
        capi.sar_local_raw(hip_lib, d[0] * 0.0, d[1], d[2], *V, sigma, rho)


# ---- 2. the average ----------------------------------------------------------------------------------------------------------------
def average_matches_the_specification(hip_lib, case, spec, method):
    """fdtd_sar_average on `case` against `spec` = average_spec(*case, method, margins=True) — the comparison every device-averaging
    test makes.  Returns (the device's result, the voxels within MARGIN of a threshold, the largest relative deviation of sar_avg
    and of half_side)."""
    capi = pkg("_capi")
    sa, half, status, counts, marg = spec
    got = capi.sar_average_raw(hip_lib, *case, method)
    again = capi.sar_average_raw(hip_lib, *case, method)
    for a, b in zip(got, again):                                    # a fixed reduction order: two calls, identical bits
        assert _same_bits(a, b)
    g_sa, g_half, g_status, g_counts = got
    assert g_status.dtype == np.int8 and g_counts.tolist() == [int((g_status == s).sum()) for s in range(4)]
    # status bytes: identical but at voxels within MARGIN of a threshold, at most MAX_EXCLUDED of the case
    near = (marg < MARGIN) & (status >= 0)
    differ = g_status != status
    assert np.count_nonzero(near) <= MAX_EXCLUDED * status.size
    assert not np.any(differ & ~near), (np.argwhere(differ & ~near)[:5], status[differ & ~near][:5], g_status[differ & ~near][:5])
    same = ~differ & ~near
    assert np.array_equal(np.isnan(g_sa[same]), np.isnan(sa[same])) and np.array_equal(np.isnan(g_half[same]), np.isnan(half[same]))
    worst = []
    for g, w in ((g_sa, sa), (g_half, half)):
        fin = same & np.isfinite(w)
        assert np.all(np.abs(g[fin] - w[fin]) <= RTOL * np.abs(w[fin]))
        nz = fin & (w != 0)
        worst.append(float(np.max(np.abs(g[nz] - w[nz]) / np.abs(w[nz]))) if nz.any() else 0.0)
    bg = status == -1
    assert np.all(g_sa[bg] == 0.0) and np.all(np.isnan(g_half[bg]))
    return got, near, worst


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["ieee", "simple"])
@pytest.mark.parametrize("name", sorted(gpu_cases()))
def test_device_average_matches_the_specification(hip_lib, name, method):
    spec = spec_of(name, method)
    average_matches_the_specification(hip_lib, gpu_cases()[name], spec, method)
    if name == "long-40x9x9":
        assert spec[2].size > 256 * 4        # more voxels than one launch block's threads, many blocks of four voxels


@pytest.mark.gpu
def test_average_bad_arguments_and_host_switch(hip_lib, monkeypatch):
    capi = pkg("_capi")
    dx, dy, dz, rho, p, mass = gpu_cases()["below-a-cell-7x6x5"]
    with pytest.raises(capi.FdtdError, match="bad sar_average argument"):
        capi.sar_average_raw(hip_lib, dx, dy, dz, rho, p, 0.0)
    with pytest.raises(capi.FdtdError, match="finite and >= 0"):
        capi.sar_average_raw(hip_lib, dx, dy, dz, -rho, p, mass)
    with pytest.raises(ValueError, match="method"):
        capi.sar_average_raw(hip_lib, dx, dy, dz, rho, p, mass, "cube")
    assert capi.sar_device(hip_lib) is not None
    monkeypatch.setenv("FDTD_SAR", "host")
    assert capi.sar_device(hip_lib) is None


# ---- 3. through Simulation ---------------------------------------------------------------------------------------------------------
NSTEPS = 300


def _run(lib, mode):
    s = block_sim(nr_ts=NSTEPS, mode=mode, nf2ff_freqs=[1.7e9, 2e9] if mode == "dft" else None, boundary="MUR" if mode == "dft" else "PEC")
    s.add_sar_box("block", *BLOCK_BOX, [2e9], 4000.0 * (6.5e-3) ** 3)
    s.build(lib)
    stats = s.run(max_steps=NSTEPS)
    return s, stats


def _close(a, b, rtol=1e-9):
    assert np.array_equal(np.isnan(a), np.isnan(b))
    fin = np.isfinite(b)
    err = np.abs(a[fin] - b[fin]) / np.where(b[fin] != 0, np.abs(b[fin]), 1.0)
    print(f"largest relative difference {err.max() if err.size else 0.0:.3e}")
    assert np.all(np.abs(a[fin] - b[fin]) <= rtol * np.abs(b[fin]))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["record", "dft"])
def test_simulation_sar_device_against_oracle_engine(hip_lib, oracle_lib, mode, monkeypatch):
    so, _ = _run(oracle_lib, mode)
    sh, stats = _run(hip_lib, mode)
    assert so.nf2ff_mode == sh.nf2ff_mode == mode
    assert np.array_equal(sh.engine.fields(), so.engine.fields())
    ro, rh = so.sar("block"), sh.sar("block")
    assert rh.device and not ro.device
    assert np.array_equal(rh.status, ro.status) and rh.counts == ro.counts
    assert ro.counts["valid"] > 20 and ro.counts["too_small"] > 20 and ro.counts["background"] > 100 and ro.peak > 0
    for f in ("sar_local", "sar_avg", "half_side"):
        _close(getattr(rh, f), getattr(ro, f))
    assert abs(rh.P_abs / ro.P_abs - 1.0) <= 1e-9 and abs(rh.peak / ro.peak - 1.0) <= 1e-9 and rh.peak_cell == ro.peak_cell
    assert rh.mass == ro.mass and rh.freq == 2e9
    rep = stats.sar["block"]
    assert rep["voxels"] == 12 * 11 * 10 and rep["status_counts"] == rh.counts and rep["device"] is True and rep["averaging_seconds"] > 0
    # FDTD_SAR=host on the HIP engine: the specification, on the same spectra — the local values have the device's bits anyway
    monkeypatch.setenv("FDTD_SAR", "host")
    rs = sh.sar("block")
    assert not rs.device and _same_bits(rs.sar_local, rh.sar_local) and np.array_equal(rs.status, rh.status)
    _close(rh.sar_avg, rs.sar_avg, 1e-10)
    if mode == "record":                      # any frequency of the band afterwards
        r2 = sh.sar("block", 1.6e9, normalise_to=2.0)
        monkeypatch.delenv("FDTD_SAR")
        r3 = sh.sar("block", 1.6e9)
        _close(r2.sar_avg * 2.0, r3.sar_avg, 1e-10)
        assert r3.peak != rh.peak


# ---- 4. through the openEMS API mirror ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_adddump_getsar_equal_the_simulation_path(hip_lib):
    api = pkg("openems_api")
    fd = api.openEMS(NrTS=NSTEPS, EndCriteria=0, lib=hip_lib, nf2ff_mode="record")
    fd.SetGaussExcite(2e9, 1e9)
    fd.SetBoundaryCond(["PEC"] * 6)
    csx = api.ContinuousStructure()
    fd.SetCSX(csx)
    g = csx.GetGrid()
    g.SetDeltaUnit(1e-3)
    for a, k in zip("xyz", (24, 20, 16)):
        g.AddLine(a, np.arange(k) * 2.0)
    # block_scene in CSXCAD calls; the density makes 1 g a cube of 6.3 mm
    csx.AddMaterial("tissue", epsilon=20.0, kappa=1.2, density=4000.0).AddBox([12, 10, 6], [32, 28, 22])
    csx.AddMetal("plate").AddBox([12, 10, 6], [32, 28, 6])
    fd.AddLumpedPort(1, 50.0, [22, 18, 0], [22, 18, 6], "z", 1.0)
    csx.AddDump("block", dump_type=21, frequency=[2e9]).AddBox(*[[1e3 * v for v in c] for c in BLOCK_BOX])
    fd.Run("")
    r = fd.GetSAR("block")
    s = block_sim(nr_ts=NSTEPS)
    s.add_sar_box("block", *BLOCK_BOX, [2e9], 1e-3)
    s.build(hip_lib)
    s.run(max_steps=NSTEPS)
    w = s.sar("block")
    assert r.device and w.device and r.counts["valid"] > 20 and r.averaging_mass == 1e-3
    for f in ("sar_local", "sar_avg", "half_side", "status"):
        assert _same_bits(getattr(r, f), getattr(w, f)), f
    assert r.P_abs == w.P_abs and r.peak == w.peak and r.peak_cell == w.peak_cell and r.peak_position == w.peak_position
    assert fd.stats.sar["block"]["status_counts"] == r.counts
    assert any(c["op"] == "AddDump" and c["dump_type"] == 21 for c in fd.calls)
    with pytest.raises(KeyError):
        fd.GetSAR("nope")
