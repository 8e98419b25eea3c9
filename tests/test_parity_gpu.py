"""GPU parity: libfdtd_hip.so vs the CPU oracle through the same C ABI, same inputs.

Bar (tightened): float32 fields IDENTICAL as IEEE values after hundreds of steps — the
HIP kernels and the oracle spell the same fmaf sequence, so every bit agrees except the sign of zero on
never-updated dead boundary edges (0 * out-of-range neighbour, which is the previous row in the dense
host layout and a pad cell in the device layout); probe/DFT/energy reductions (different summation
order) within 1e-12 relative (float64 accumulators)."""
import numpy as np
import pytest

from conftest import pkg
from helpers import patch_sim, seeded_fields, rel_l2


def same_values(a, b):
    """Exact float equality (-0 == +0; any NaN fails)."""
    return np.array_equal(a, b)

pytestmark = pytest.mark.gpu


def _run_both(sim_factory, hip_lib, oracle_lib, steps, seed=None, flags=0):
    import os
    out = []
    for lib in (hip_lib, oracle_lib):
        s = sim_factory()
        e = s.build(lib, flags=flags if lib is hip_lib else 0)
        if seed is not None:
            seeded_fields(e, seed)
        e.run(steps)
        out.append((s, e))
    # Round 4: AUTO steps small grids resident in registers (csrc/resident.hip).  The schedules AUTO took before — several timesteps per launch
    # behind flags, two / three launches — still serve every grid that does not fit the chip: the same case once more with the resident
    # schedule switched off, against the same oracle run.
    if flags == 0 and out[0][1].schedule_info()["resident"]:
        os.environ["FDTD_RESIDENT"] = "0"
        try:
            s = sim_factory()
            e = s.build(hip_lib)
        finally:
            del os.environ["FDTD_RESIDENT"]
        if seed is not None:
            seeded_fields(e, seed)
        e.run(steps)
        assert not e.schedule_info()["resident"]
        assert np.array_equal(e.fields(), out[1][1].fields()), "flag-coupled / multi-launch schedule != oracle"
    return out


@pytest.mark.parametrize("use_classes", [True, False])
@pytest.mark.parametrize("shape", [(64, 60, 36), (53, 47, 31)])
def test_fields_bitexact_cpml(hip_lib, oracle_lib, shape, use_classes):
    """Class-compressed and raw operator, nx a multiple of 4 and not, CPML on all faces."""
    (sh, eh), (so, eo) = _run_both(lambda: patch_sim(*shape, boundary="CPML", cpml_cells=8, nr_ts=300,
                                                     use_classes=use_classes), hip_lib, oracle_lib, 300, seed=1)
    assert eh.backend.startswith("hip") and eo.backend.startswith("oracle")
    fh, fo = eh.fields(), eo.fields()
    assert np.isfinite(fo).all() and np.abs(fo).max() > 0
    assert same_values(fh, fo), f"rel L2 {rel_l2(fh, fo):.3e}"
    nz = fo != 0
    assert np.array_equal(fh[nz].view(np.uint32), fo[nz].view(np.uint32))


@pytest.mark.parametrize("cells", [3, 12])
def test_fields_bitexact_cpml_layer_thickness(hip_lib, oracle_lib, cells):
    """CPML layers thinner than, and a multiple of, the 4-cell groups the kernels work in (the x ranges are aligned
    internally: cells drawn into the aligned range carry identity coefficients)."""
    (sh, eh), (so, eo) = _run_both(lambda: patch_sim(50, 46, 33, boundary="CPML", cpml_cells=cells, nr_ts=200), hip_lib, oracle_lib, 200, seed=4)
    fh, fo = eh.fields(), eo.fields()
    assert np.abs(fo).max() > 0 and same_values(fh, fo), f"rel L2 {rel_l2(fh, fo):.3e}"


def test_fields_bitexact_cpml_thick_x_layers(hip_lib, oracle_lib):
    """x layers of 66 cells on both sides: more aligned x-layer cells than the kernels' LDS coefficient table holds
    (XC_MAX = 128), so the kernels read the x coefficients from global memory; PEC on the other faces."""
    bc = ["CPML", "CPML", "PEC", "PEC", "PEC", "PEC"]
    (sh, eh), (so, eo) = _run_both(lambda: patch_sim(200, 30, 26, boundary=bc, cpml_cells=66, nr_ts=150, nf2ff=False), hip_lib, oracle_lib, 150, seed=6)
    fh, fo = eh.fields(), eo.fields()
    assert np.abs(fo).max() > 0 and same_values(fh, fo), f"rel L2 {rel_l2(fh, fo):.3e}"


@pytest.mark.parametrize("use_classes,shape", [(True, (48, 44, 30)), (False, (48, 44, 30)), (True, (53, 47, 31))])
def test_fields_bitexact_mur(hip_lib, oracle_lib, use_classes, shape):
    """First-order Mur on all six faces (the post pass rides in update_E, the pre pass in update_H): class and raw operator,
    nx a multiple of 4 and not."""
    (sh, eh), (so, eo) = _run_both(lambda: patch_sim(*shape, boundary="MUR", nr_ts=400, use_classes=use_classes), hip_lib, oracle_lib, 400, seed=2)
    fh, fo = eh.fields(), eo.fields()
    assert same_values(fh, fo), f"rel L2 {rel_l2(fh, fo):.3e}"
    nz = fo != 0
    assert np.array_equal(fh[nz].view(np.uint32), fo[nz].view(np.uint32))


def test_fields_bitexact_mixed_boundaries(hip_lib, oracle_lib):
    bc = ["MUR", "CPML", "CPML", "MUR", "PEC", "CPML"]
    (sh, eh), (so, eo) = _run_both(lambda: patch_sim(50, 46, 33, boundary=bc, cpml_cells=6, nr_ts=300), hip_lib, oracle_lib, 300, seed=3)
    fh, fo = eh.fields(), eo.fields()
    assert same_values(fh, fo), f"rel L2 {rel_l2(fh, fo):.3e}"
    nz = fo != 0
    assert np.array_equal(fh[nz].view(np.uint32), fo[nz].view(np.uint32))


def test_port_probes_dft_energy(hip_lib, oracle_lib):
    (sh, eh), (so, eo) = _run_both(lambda: patch_sim(64, 60, 36, nr_ts=1500), hip_lib, oracle_lib, 1500)
    (uh, ih), (uo, io) = sh.port_series()[0], so.port_series()[0]
    assert len(uh) == len(uo) == 1500 and np.abs(uo).max() > 0
    assert rel_l2(uh, uo) < 1e-12 and rel_l2(ih, io) < 1e-12
    bh, bo = sh.nf2ff_boxes(), so.nf2ff_boxes()
    assert len(bh) == len(bo) == 24
    for a, b in zip(bh, bo):
        assert a.shape == b.shape
        assert rel_l2(a, b) < 1e-12
    evh, eih = eh.energy(); evo, eio = eo.energy()
    assert abs(evh - evo) <= 1e-10 * evo and abs(eih - eio) <= 1e-10 * eio


def test_removed_kernel_selection_is_rejected(hip_lib):
    """Flags 2..4 selected the one-pass variants of ABI v1; they were removed: a clean FDTD_E_UNSUPPORTED."""
    capi = pkg("_capi")
    s = patch_sim(40, 40, 30, nr_ts=20, nf2ff=False)
    e = s.build(hip_lib, flags=2)
    with pytest.raises(capi.FdtdError, match="removed"):
        e.run(2)


def test_no_pml_and_odd_sizes(hip_lib, oracle_lib):
    """PEC box (the template path without CPML), nx not a multiple of 4, sources + probes vs the oracle."""
    (sh, eh), (so, eo) = _run_both(lambda: patch_sim(45, 43, 29, boundary="PEC", nr_ts=400, nf2ff=False), hip_lib, oracle_lib, 400)
    assert same_values(eh.fields(), eo.fields()) and np.abs(eo.fields()).max() > 0
    assert rel_l2(sh.port_series()[0][0], so.port_series()[0][0]) < 1e-12


def test_chunked_runs_and_fused_probes(hip_lib, oracle_lib):
    """fdtd_run in uneven chunks (probe flush at every call end, sources injected inside the main kernels)
    must give the same series as the oracle's plain loop."""
    sh, so = patch_sim(48, 44, 32, nr_ts=700), patch_sim(48, 44, 32, nr_ts=700)
    eh = sh.build(hip_lib)
    eo = so.build(oracle_lib)
    for n in (1, 2, 97, 250, 349, 1):
        eh.run(n)
    eo.run(700)
    assert eh.step == eo.step == 700
    (uh, ih), (uo, io) = sh.port_series()[0], so.port_series()[0]
    assert len(uh) == 700 and np.abs(uo).max() > 0 and np.abs(io).max() > 0
    assert rel_l2(uh, uo) < 1e-12 and rel_l2(ih, io) < 1e-12
    assert same_values(eh.fields(), eo.fields())
    for a, b in zip(sh.nf2ff_boxes(), so.nf2ff_boxes()):
        assert rel_l2(a, b) < 1e-12


def test_farfield_matches_oracle(hip_lib, oracle_lib):
    capi = pkg("_capi")
    rng = np.random.default_rng(5)
    npts = 3000
    pos = rng.uniform(-0.05, 0.05, (npts, 3))
    Js = rng.standard_normal((npts, 3)) + 1j * rng.standard_normal((npts, 3))
    Ms = rng.standard_normal((npts, 3)) + 1j * rng.standard_normal((npts, 3))
    th, ph = np.meshgrid(np.deg2rad(np.arange(0, 181, 4.0)), np.deg2rad(np.arange(0, 360, 10.0)), indexing="ij")
    k = 2 * np.pi * 2.45e9 / 299792458.0
    eh = capi.farfield(hip_lib, pos, Js, Ms, k, th.ravel(), ph.ravel())
    eo = capi.farfield(oracle_lib, pos, Js, Ms, k, th.ravel(), ph.ravel())
    assert rel_l2(eh[0], eo[0]) < 1e-11 and rel_l2(eh[1], eo[1]) < 1e-11


def test_two_slabs_equal_one_slab(hip_lib):
    """z-slab decomposition with the external halo transport: two contexts on one device, halos
    copied by the host, must reproduce the single-slab run bit for bit (N-GPU == 1-GPU)."""
    capi = pkg("_capi")
    s1 = patch_sim(56, 52, 34, nr_ts=200)
    e1 = s1.build(hip_lib)
    e1.run(200)
    sa, sb = patch_sim(56, 52, 34, nr_ts=200), patch_sim(56, 52, 34, nr_ts=200)
    ea, eb = sa.build(hip_lib, rank=0, world=2), sb.build(hip_lib, rank=1, world=2)
    for _ in range(200):
        ea.half_step(capi.PHASE_E); eb.half_step(capi.PHASE_E)
        ea.halo_put(capi.HALO_E_DOWN, eb.halo_get(capi.HALO_E_DOWN))
        ea.half_step(capi.PHASE_H); eb.half_step(capi.PHASE_H)
        eb.halo_put(capi.HALO_H_UP, ea.halo_get(capi.HALO_H_UP))
    f1 = e1.fields()
    f2 = np.concatenate([ea.fields(), eb.fields()], axis=2)
    assert np.array_equal(f1.view(np.uint32), f2.view(np.uint32))  # same layout on both sides: every bit
    u1 = s1.port_series()[0][0]
    u2 = sa.port_series()[0][0] + sb.port_series()[0][0]
    assert rel_l2(u2, u1) < 1e-12


@pytest.mark.parametrize("overlap", ["split", "nosplit"])
@pytest.mark.parametrize("world", [2, 3, 5])
def test_linked_slabs_overlapped_schedule(hip_lib, world, overlap):
    """The multi-rank step schedule of the RCCL path (interior planes first, dependent boundary plane after
    the halo event, probes/sources fused into the split launches) driven in-process: `world` slabs on one
    GPU with peer copies instead of ncclSend/ncclRecv must reproduce the single-slab run bit for bit."""
    capi = pkg("_capi")
    s1 = patch_sim(56, 52, 34, nr_ts=260)
    e1 = s1.build(hip_lib)
    sims = [patch_sim(56, 52, 34, nr_ts=260) for _ in range(world)]
    flag = capi.FLAG_OVERLAP_ON if overlap == "split" else capi.FLAG_OVERLAP_OFF
    engs = [s.build(hip_lib, rank=r, world=world, flags=flag) for r, s in enumerate(sims)]
    if world != 3:      # random INITIAL fields (zero ones for world 3): the first exchange happens before the first half-step
        rng = np.random.default_rng(6)
        for kind in (0, 1):
            for comp in range(3):
                g = (1e-3 * rng.standard_normal(e1.local_shape)).astype(np.float32)
                e1.set_field(kind, comp, g)
                for e in engs:
                    e.set_field(kind, comp, np.ascontiguousarray(g[e.k0:e.k0 + e.nk]))
    e1.run(260)
    for n in (1, 100, 159):
        capi.run_linked(engs, n)
    f1, f2 = e1.fields(), np.concatenate([e.fields() for e in engs], axis=2)
    assert np.abs(f1).max() > 0 and np.array_equal(f1, f2)
    differ = f1.view(np.uint32) != f2.view(np.uint32)     # at most the sign of a zero on dead boundary edges (0 * neighbour: seeded runs)
    assert not np.any(f1[differ] != 0) and (world != 3 or not differ.any())
    u1, i1 = s1.port_series()[0]
    u2 = sum(s.port_series()[0][0] for s in sims)
    i2 = sum(s.port_series()[0][1] for s in sims)
    assert rel_l2(u2, u1) < 1e-12 and rel_l2(i2, i1) < 1e-12
    for a, *parts in zip(s1.nf2ff_boxes(), *[s.nf2ff_boxes() for s in sims]):
        assert rel_l2(sum(parts), a) < 1e-12


def test_rccl_single_rank_comm(hip_lib):
    """World of one: the RCCL communicator initialises and the step loop runs through it."""
    capi = pkg("_capi")
    s = patch_sim(40, 40, 30, nr_ts=50, nf2ff=False)
    e = s.build(hip_lib)
    e.comm_init(capi.comm_unique_id(hip_lib))
    e.run(50)
    assert e.step == 50


def test_full_size_properties(hip_lib):
    """BASELINE 'NS' size (300x300x60): size-independent properties instead of an oracle run —
    zero in -> zero out, linearity in the excitation, finite decaying energy."""
    sim_m, wl, sc = pkg("simulation"), pkg("workloads"), pkg("scene")
    w = wl.patch_workload("NS")
    vox = sc.voxelize(w.scene, w.grid)
    res = []
    base_amp = [p.src_amp.copy() for p in vox.ports]
    for amp in (0.0, 1.0, 2.0):
        for p, a0 in zip(vox.ports, base_amp):
            p.src_amp = (amp * a0).astype(np.float32)
        s = sim_m.Simulation(w.grid, vox, f0=w.f0, fc=w.fc, boundary="CPML", cpml_cells=10, nr_ts=600)
        e = s.build(hip_lib)
        e.run(600)
        res.append((e.get_field(0, 2), s.port_series()[0][0]))
    for p, a0 in zip(vox.ports, base_amp):
        p.src_amp = a0
    assert not res[0][0].any() and not res[0][1].any()
    assert np.isfinite(res[1][0]).all() and np.abs(res[1][0]).max() > 0
    assert rel_l2(res[2][0], 2.0 * res[1][0]) < 1e-6
    assert rel_l2(res[2][1], 2.0 * res[1][1]) < 1e-6


def test_plugin_path_s11_and_patterns_gpu_vs_oracle(hip_lib, oracle_lib, tmp_path):
    """North-star parity statement, end to end through the plugin surface: the same PatchAntennaParams
    go through prepare_hip_microstrip_patch_3d / run_prepared_hip once on the GPU library and once on the
    CPU oracle; S11(f) and the E/H-plane patterns must agree to 1e-3 relative L2 (they agree to ~1e-9:
    the time stepping is bit-identical, only fp64 reductions differ)."""
    s = pkg("solver_fdtd_hip")
    sink = pkg("result_sink")
    P = pkg("params").PatchAntennaParams
    p = P.from_user_units(frequency_ghz=5.8, er=4.3, h_mm=1.6, loss_tangent=0.02)
    res = []
    for lib, tag in ((hip_lib, "gpu"), (oracle_lib, "cpu")):
        prep = s.prepare_hip_microstrip_patch_3d(p, feed_direction=s.FeedDirection.NEG_X, boundary="PML_8", theta_step_deg=4.0,
                                                 phi_step_deg=15.0, mesh_quality=1, work_dir=str(tmp_path / tag), lib=lib)
        assert prep.ok, prep.message
        prep.FDTD.NrTS = 2500
        r = s.run_prepared_hip(prep, frequency_hz=5.8e9, verbose=0)
        assert r.ok, r.message
        res.append(r)
    g, c = res
    assert g.intensity.shape == c.intensity.shape == (46, 25)
    assert rel_l2(g.s11, c.s11) < 1e-3 and rel_l2(g.port_u, c.port_u) < 1e-4 and rel_l2(g.port_i, c.port_i) < 1e-4
    _, ge, gh = sink.principal_cuts(g.theta, g.phi, g.intensity)
    _, ce, ch = sink.principal_cuts(c.theta, c.phi, c.intensity)
    lin = lambda d: 10.0 ** (np.asarray(d) / 20.0)
    assert rel_l2(lin(ge), lin(ce)) < 1e-3 and rel_l2(lin(gh), lin(ch)) < 1e-3
    assert abs(g.Dmax - c.Dmax) < 1e-6 * c.Dmax
    assert g.stats["steps"] == c.stats["steps"] and g.stats["grid"] == c.stats["grid"]
    data = sink.write_result(g, str(tmp_path / "result.json"))
    assert data["ok"] and len(data["e_plane_dBi"]) == 46


def test_multi_patch_rotated_two_ports_gpu_vs_oracle(hip_lib, oracle_lib, tmp_path):
    """Two elements, one rotated 90 deg about z and lifted, finite-thickness copper, volumetric lumped ports
    (multi_3d variant = BASELINE config 5's geometry class) through the plugin surface on the HIP library and on
    the oracle: S11 of BOTH ports, both port series and the E/H-plane cuts within 1e-3 relative L2."""
    s = pkg("solver_fdtd_hip")
    sink = pkg("result_sink")
    P = pkg("params").PatchAntennaParams
    p = P.from_user_units(frequency_ghz=5.8, er=4.3, h_mm=1.6, loss_tangent=0.02, metal_thickness_um=200.0)
    arr = [s.PatchInstance("A", p, -0.02, 0.0, 0.0, s.FeedDirection.NEG_X),
           s.PatchInstance("B", p, 0.02, 0.0, 0.002, s.FeedDirection.NEG_Y, rot_z_deg=90.0)]
    out = []
    for lib, tag in ((hip_lib, "gpu"), (oracle_lib, "cpu")):
        prep = s.prepare_hip_microstrip_multi_3d(arr, boundary="PML_8", theta_step_deg=6.0, phi_step_deg=30.0, mesh_quality=1,
                                                 auto_margin_mm=(25.0, 25.0, 30.0), work_dir=str(tmp_path / tag), lib=lib)
        assert prep.ok, prep.message
        prep.FDTD.NrTS = 1500
        r = s.run_prepared_hip(prep, frequency_hz=5.8e9, verbose=0)
        assert r.ok, r.message
        assert np.isfinite(r.intensity).all() and r.intensity.shape == (31, 13)
        series = prep.FDTD.sim.port_series()
        assert len(series) == 2 and all(np.abs(u).max() > 0 and np.abs(i).max() > 0 for u, i in series)
        s11 = [s.s11_from_port(port, prep.sim_path, 5.8e9)[1] for port in prep.ports]
        out.append((r, series, s11))
    (g, sg, s11g), (c, sc_, s11c) = out
    assert g.stats["grid"] == c.stats["grid"] and g.stats["steps"] == c.stats["steps"]
    for q in range(2):
        assert rel_l2(sg[q][0], sc_[q][0]) < 1e-4 and rel_l2(sg[q][1], sc_[q][1]) < 1e-4
        assert rel_l2(s11g[q], s11c[q]) < 1e-3
    _, ge, gh = sink.principal_cuts(g.theta, g.phi, g.intensity)
    _, ce, ch = sink.principal_cuts(c.theta, c.phi, c.intensity)
    lin = lambda d: 10.0 ** (np.asarray(d) / 20.0)
    assert rel_l2(lin(ge), lin(ce)) < 1e-3 and rel_l2(lin(gh), lin(ch)) < 1e-3
    assert abs(g.Dmax - c.Dmax) < 1e-6 * c.Dmax


def test_fixed_scene_mur_end_criterion_gpu_vs_oracle(hip_lib, oracle_lib, tmp_path):
    """The scene the reference's GUI runs by default (prepare_*_patch_fixed: graded mesh, MUR on all faces, lumped port,
    end criterion -40 dB: solver_fdtd_openems_fixed.py:113-342) through the plugin surface on the HIP library and on
    the oracle: both stop at the same step, S11(f), the port series and the two pattern cuts within 1e-3."""
    s = pkg("solver_fdtd_hip")
    P = pkg("params").PatchAntennaParams
    p = P.from_user_units(frequency_ghz=2.45, er=4.3, h_mm=1.6, loss_tangent=0.02)
    res = []
    for lib, tag in ((hip_lib, "gpu"), (oracle_lib, "cpu")):
        prep = s.prepare_hip_patch_fixed(p, work_dir=str(tmp_path / tag), lib=lib)
        assert prep.ok, prep.message
        r = s.run_prepared_hip(prep, frequency_hz=p.frequency_hz, verbose=0)
        assert r.ok, r.message
        res.append(r)
    g, c = res
    assert g.intensity.shape == c.intensity.shape == (90, 2)
    assert g.stats["grid"] == c.stats["grid"] and g.stats["steps"] == c.stats["steps"] < 30000   # stopped by the energy criterion
    assert g.stats["energy_db"] < -40.0
    assert rel_l2(g.port_u, c.port_u) < 1e-4 and rel_l2(g.port_i, c.port_i) < 1e-4
    assert rel_l2(g.s11, c.s11) < 1e-3
    lin = lambda d: 10.0 ** (np.asarray(d) / 20.0)
    assert rel_l2(lin(g.intensity), lin(c.intensity)) < 1e-3
    assert abs(g.Dmax - c.Dmax) < 1e-6 * c.Dmax


def test_northstar_acceptance(hip_lib, oracle_lib):
    """BASELINE north-star grid (300x300x60, CPML-10, lumped port, NF2FF surfaces) stepped on the HIP library and on
    the oracle: port series, S11(f), E/H-plane cuts and Dmax within the north-star's 1e-3 relative-L2 tolerance
    (they are in fact identical to rounding: same fp32 operation order).  3000 of the 12000 steps of the full
    acceptance run (tests/acceptance_northstar.py; its r01 result is committed under profiles/r01/)."""
    import acceptance_northstar
    out = acceptance_northstar.run(steps=3000, workload="NS")
    assert out["gpu"]["backend"].startswith("hip") and out["cpu_oracle"]["backend"].startswith("oracle")
    assert out["tolerance"] == 1e-3
    assert out["pass"], out["rel_l2"]
    assert max(out["rel_l2"].values()) < 1e-6, out["rel_l2"]


@pytest.mark.parametrize("overlap", ["split", "nosplit", "inline"])
def test_rccl_self_loopback_transport(hip_lib, oracle_lib, overlap, monkeypatch):
    """The RCCL calls themselves on one GPU: an interior slab (rank 1 of 3) whose halos go to ITSELF through
    ncclSend/ncclRecv in a communicator of one (FDTD_FLAG_LOOPBACK) — the library's own step loop, communication
    stream, events and overlap split — against the same slab stepped by half-steps with its halo planes copied back
    through the host, on the HIP library and on the oracle.  Interior planes have live coefficients on both faces, so
    a wrong plane, component, count or ordering changes the fields."""
    capi = pkg("_capi")
    flag = capi.FLAG_LOOPBACK | (capi.FLAG_OVERLAP_OFF if overlap == "nosplit" else capi.FLAG_OVERLAP_ON)
    # round 4: a slab this thin exchanges in stream order on the compute stream under AUTO ("inline"); the overlapped schedule (communication
    # stream, events, split sweeps) serves the thick slabs: forced here for the first two cases
    monkeypatch.setenv("FDTD_RCCL_INLINE", "1" if overlap == "inline" else "0")
    n = 120

    def slab(lib, flags):
        s = patch_sim(44, 40, 36, nr_ts=n + 8, nf2ff=False)
        e = s.build(lib, rank=1, world=3, flags=flags)
        seeded_fields(e, 11)
        return s, e

    _, er = slab(hip_lib, flag)
    er.comm_init(capi.comm_unique_id(hip_lib))
    er.run(n)
    outs = [er.fields()]
    for lib in (hip_lib, oracle_lib):
        _, e = slab(lib, 0)
        e.halo_put(capi.HALO_H_UP, e.halo_get(capi.HALO_H_UP))     # the halo of "step -1": the (seeded) initial fields
        for _ in range(n):
            e.half_step(capi.PHASE_E)
            e.halo_put(capi.HALO_E_DOWN, e.halo_get(capi.HALO_E_DOWN))
            e.half_step(capi.PHASE_H)
            e.halo_put(capi.HALO_H_UP, e.halo_get(capi.HALO_H_UP))
        outs.append(e.fields())
    assert er.step == n and np.isfinite(outs[2]).all() and np.abs(outs[2]).max() > 0
    assert same_values(outs[0], outs[1]), f"RCCL loopback vs host loopback (HIP): rel L2 {rel_l2(outs[0], outs[1]):.3e}"
    assert same_values(outs[0], outs[2]), f"RCCL loopback vs oracle: rel L2 {rel_l2(outs[0], outs[2]):.3e}"
    # and the loopback really matters: without any exchange the same slab ends elsewhere
    _, e0 = slab(hip_lib, 0)
    for _ in range(n):
        e0.half_step(capi.PHASE_E)
        e0.half_step(capi.PHASE_H)
    assert not same_values(e0.fields(), outs[0])


def _attach_p2p(engs, selftest=False):
    blobs = [e.p2p_export() for e in engs]
    for r, e in enumerate(engs):
        e.p2p_attach(blobs[r - 1] if r > 0 else None, blobs[r + 1] if r + 1 < len(engs) else None)
    if selftest:
        # the self-test waits for the neighbours' tokens: all ranks must be in it at the same time (one host thread each;
        # ctypes releases the GIL).  It pushes pattern planes through the real data path and restores the zeros after.
        import threading
        errs = []

        def one(e):
            try:
                e.p2p_selftest(0x5E1F0003)
            except Exception as exc:      # noqa: BLE001
                errs.append(exc)
        th = [threading.Thread(target=one, args=(e,)) for e in engs]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs


@pytest.mark.parametrize("schedule", ["two_launches", "one_launch"])
@pytest.mark.parametrize("world", [2, 3, 5])
def test_p2p_mailbox_transport_slabs_equal_one_slab(hip_lib, world, schedule):
    """P2P mailbox transport (halos pushed by the update kernels into the neighbour's mailbox, step-counter flags,
    dependent plane scheduled last): `world` slabs in this process on one GPU — each on its own stream, coupled only
    through the mailboxes — must reproduce the single-slab run bit for bit, over several fdtd_run_linked calls.
    one_launch: every slab steps with ONE launch per timestep (k_step with the mailbox protocol inside: E of plane 0 first,
    H of the top plane last), which AUTO picks for thin slabs."""
    capi = pkg("_capi")
    flags = capi.FLAG_KERNEL_DIRECT if schedule == "two_launches" else capi.FLAG_KERNEL_WAVEFRONT
    s1 = patch_sim(56, 52, 34, nr_ts=260)
    e1 = s1.build(hip_lib, flags=capi.FLAG_KERNEL_DIRECT)
    sims = [patch_sim(56, 52, 34, nr_ts=260) for _ in range(world)]
    engs = [s.build(hip_lib, rank=r, world=world, flags=flags) for r, s in enumerate(sims)]
    _attach_p2p(engs, selftest=(world == 3))
    # random INITIAL fields (world 2 and 5; zero ones for world 3): the halo of "step -1" is pushed before the first launch
    if world != 3:
        rng = np.random.default_rng(5)
        for kind in (0, 1):
            for comp in range(3):
                g = (1e-3 * rng.standard_normal(e1.local_shape)).astype(np.float32)
                e1.set_field(kind, comp, g)
                for e in engs:
                    e.set_field(kind, comp, np.ascontiguousarray(g[e.k0:e.k0 + e.nk]))
    e1.run(260)
    for n in (1, 100, 159):
        capi.run_linked(engs, n)
    f1, f2 = e1.fields(), np.concatenate([e.fields() for e in engs], axis=2)
    assert np.abs(f1).max() > 0 and np.array_equal(f1, f2)
    differ = f1.view(np.uint32) != f2.view(np.uint32)     # at most the sign of a zero on dead boundary edges (0 * neighbour: seeded runs)
    assert not np.any(f1[differ] != 0) and (world != 3 or not differ.any())
    u1, i1 = s1.port_series()[0]
    u2 = sum(s.port_series()[0][0] for s in sims)
    i2 = sum(s.port_series()[0][1] for s in sims)
    assert rel_l2(u2, u1) < 1e-12 and rel_l2(i2, i1) < 1e-12
    for a, *parts in zip(s1.nf2ff_boxes(), *[s.nf2ff_boxes() for s in sims]):
        assert rel_l2(sum(parts), a) < 1e-12


def test_p2p_wait_times_out_instead_of_hanging(hip_lib):
    """A rank whose neighbour never steps: the bounded halo wait gives up (10 s) and fdtd_run reports it."""
    capi = pkg("_capi")
    sims = [patch_sim(40, 36, 24, nr_ts=20, nf2ff=False) for _ in range(2)]
    engs = [s.build(hip_lib, rank=r, world=2) for r, s in enumerate(sims)]
    _attach_p2p(engs)
    with pytest.raises(capi.FdtdError, match="timed out"):
        engs[0].run(1)          # rank 1 is never stepped: rank 0's H half-step waits for an E halo that does not come


@pytest.mark.parametrize("src_i", [1, 9])
def test_mur_with_sources_next_to_and_away_from_a_face(hip_lib, oracle_lib, src_i):
    """Mur scene driven through the C ABI directly: a source edge ON the plane next to the x- Mur face (src_i = 1: the
    order 'Mur post, then source' matters, so the library must take the unfused launch sequence) and in the interior
    (src_i = 9: sources/probes stay fused in the main kernels) — both identical to the oracle, fields and probe series."""
    capi = pkg("_capi")
    from source_probe_cases import raw_engine
    nx, ny, nz = 22, 20, 18
    n = 160
    out = []
    for lib in (hip_lib, oracle_lib):
        e = raw_engine(lib, (21, (nx, ny, nz)), "MUR", max_steps=n + 8)
        dt = e.dt
        t = np.arange(n) * dt
        e.set_signal(np.sin(2 * np.pi * 8e9 * t) * np.exp(-((t - 40 * dt) / (15 * dt)) ** 2))
        j, k = ny // 2, nz // 2
        src = np.array([(k * ny + j) * nx + src_i, (k * ny + j + 1) * nx + src_i], np.int64)
        e.add_source(src, np.array([2, 2], np.int8), np.array([1.0, -0.5], np.float32))
        pv = e.add_probe(capi.KIND_V, np.array([(k * ny + j) * nx + src_i + 3], np.int64), np.array([2], np.int8), np.array([-1.0], np.float32))
        pi = e.add_probe(capi.KIND_I, np.array([(k * ny + j) * nx + src_i + 3], np.int64), np.array([1], np.int8), np.array([1.0], np.float32))
        for m in (1, 70, n - 71):
            e.run(m)
        out.append((e.fields(), e.get_probe(pv), e.get_probe(pi)))
    (fh, uh, ih), (fo, uo, io) = out
    assert np.abs(fo).max() > 0 and len(uo) == n
    assert same_values(fh, fo), f"rel L2 {rel_l2(fh, fo):.3e}"
    assert rel_l2(uh, uo) < 1e-12 and rel_l2(ih, io) < 1e-12


def test_largest_baseline_grid_two_p2p_slabs_equal_one(hip_lib, oracle_lib):
    """BASELINE's largest configuration (C5: 800x800x120, 2x2 array, four lumped ports, 76.8 Mcells) at full size:
    the single-slab HIP run equals the ORACLE on every field value and port series, and two z-slabs coupled by the P2P
    mailbox transport reproduce the single-slab run bit for bit — exercises the index arithmetic, the source lists and
    the mailboxes at the sizes the 8-GPU configuration is quoted on."""
    capi, sim_m, wl, sc = pkg("_capi"), pkg("simulation"), pkg("workloads"), pkg("scene")
    w = wl.baseline_workload("C5")
    vox = sc.voxelize(w.scene, w.grid)
    steps = 36

    def make():
        return sim_m.Simulation(w.grid, vox, f0=w.f0, fc=w.fc, boundary="CPML", cpml_cells=10, nr_ts=steps + 4, nf2ff_freqs=None)

    s1 = make()
    e1 = s1.build(hip_lib)
    e1.run(steps)
    ref = [e1.get_field(kind, comp) for kind in (0, 1) for comp in range(3)]
    u1 = [np.asarray(s1.port_series()[q][0]) for q in range(len(vox.ports))]
    del e1, s1
    so = make()
    eo = so.build(oracle_lib)
    eo.run(steps)
    n = 0
    for kind in (0, 1):
        for comp in range(3):
            assert same_values(ref[n], eo.get_field(kind, comp)), ("HIP vs oracle", kind, comp)
            n += 1
    for q in range(len(vox.ports)):
        assert rel_l2(u1[q], np.asarray(so.port_series()[q][0])) < 1e-12
    del eo, so
    sims = [make(), make()]
    engs = [s.build(hip_lib, rank=r, world=2) for r, s in enumerate(sims)]
    _attach_p2p(engs)
    capi.run_linked(engs, steps)
    n = 0
    for kind in (0, 1):
        for comp in range(3):
            both = np.concatenate([e.get_field(kind, comp) for e in engs], axis=0)
            assert both.shape == ref[n].shape
            assert np.array_equal(both.view(np.uint32), ref[n].view(np.uint32)), (kind, comp)
            n += 1
    assert max(np.abs(r).max() for r in ref) > 0
    for q in range(len(vox.ports)):
        u2 = sum(np.asarray(s.port_series()[q][0]) for s in sims)
        assert rel_l2(u2, u1[q]) < 1e-12


def test_c4_full_size_gpu_equals_oracle(hip_lib, oracle_lib):
    """BASELINE config 4 at full size (512x512x128, 5.8 GHz microstrip-3D geometry, CPML-10): 40 timesteps on the HIP
    library and on the oracle, every field value identical."""
    sim_m, wl, sc = pkg("simulation"), pkg("workloads"), pkg("scene")
    w = wl.baseline_workload("C4")
    vox = sc.voxelize(w.scene, w.grid)
    out = []
    for lib in (hip_lib, oracle_lib):
        s = sim_m.Simulation(w.grid, vox, f0=w.f0, fc=w.fc, boundary="CPML", cpml_cells=10, nr_ts=48, nf2ff_freqs=None)
        e = s.build(lib)
        e.run(40)
        out.append(([e.get_field(kind, comp) for kind in (0, 1) for comp in range(3)], np.asarray(s.port_series()[0][0])))
        del e, s
    (fh, uh), (fo, uo) = out
    assert max(np.abs(a).max() for a in fo) > 0
    for a, b in zip(fh, fo):
        assert same_values(a, b)
    assert rel_l2(uh, uo) < 1e-12


@pytest.mark.parametrize("name,steps", [("C2", 300), ("C3", 90)])
def test_c2_c3_full_size_gpu_equals_oracle(hip_lib, oracle_lib, name, steps):
    """BASELINE configs 2 and 3 at full size (200x200x40 and 400x400x80, fixed scene, CPML-10) WITH the NF2FF surfaces
    recording: every field value identical to the oracle, port series and all 24 DFT boxes to 1e-12."""
    sim_m, wl, sc = pkg("simulation"), pkg("workloads"), pkg("scene")
    w = wl.baseline_workload(name)
    vox = sc.voxelize(w.scene, w.grid)
    out = []
    for lib in (hip_lib, oracle_lib):
        s = sim_m.Simulation(w.grid, vox, f0=w.f0, fc=w.fc, boundary="CPML", cpml_cells=10, nr_ts=steps + 8, nf2ff_freqs=[w.f0])
        e = s.build(lib)
        e.run(steps)
        out.append(([e.get_field(kind, comp) for kind in (0, 1) for comp in range(3)], np.asarray(s.port_series()[0][0]),
                    np.asarray(s.port_series()[0][1]), s.nf2ff_boxes(), s.dft_every))
        del e, s
    (fh, uh, ih, bh, every), (fo, uo, io, bo, _) = out
    assert steps > 2 * every                       # the surfaces took several samples
    assert max(np.abs(a).max() for a in fo) > 0 and np.abs(uo).max() > 0
    for a, b in zip(fh, fo):
        assert same_values(a, b)
    assert rel_l2(uh, uo) < 1e-12 and rel_l2(ih, io) < 1e-12
    assert len(bh) == len(bo) == 24
    for a, b in zip(bh, bo):
        assert a.shape == b.shape and rel_l2(a, b) < 1e-12
    assert max(np.abs(b).max() for b in bo) > 0


@pytest.mark.parametrize("nfreq", [3, 16])
def test_multi_frequency_dft_boxes(hip_lib, oracle_lib, nfreq):
    """Running DFT with nfreq > 1 (the k_dft frequency loop): 3 and 16 frequencies over the reference's S11 band,
    HIP vs oracle 1e-12 on all 24 boxes, and the f0 column equals a single-frequency run bit for bit."""
    f0 = 2.45e9
    freqs = np.linspace(0.7 * f0, 1.3 * f0, nfreq)
    freqs[nfreq // 2] = f0
    (sh, eh), (so, eo) = _run_both(lambda: patch_sim(64, 60, 36, nr_ts=900, nf2ff_freqs=freqs), hip_lib, oracle_lib, 900)
    bh, bo = sh.nf2ff_boxes(), so.nf2ff_boxes()
    assert len(bh) == 24 and bh[0].shape[0] == nfreq
    for a, b in zip(bh, bo):
        assert rel_l2(a, b) < 1e-12
    s1 = patch_sim(64, 60, 36, nr_ts=900)
    s1.dft_every, s1.dft_nsamples = sh.dft_every, sh.dft_nsamples      # same sampling as the multi-frequency run
    e1 = s1.build(hip_lib)
    e1.run(900)
    for a, b in zip(bh, s1.nf2ff_boxes()):
        assert np.array_equal(a[nfreq // 2], b[0])


def test_recorder_equals_running_dft_and_oracle(hip_lib, oracle_lib):
    """Time-domain recording of the NF2FF faces (fdtd_set_recorder / fdtd_rec_transform): transformed afterwards at
    the frequencies a running-DFT run had fixed beforehand it gives the same bits (same float64 fma chain); any other
    frequency afterwards agrees with the oracle's recorder to 1e-12; chunked runs record the same samples."""
    f0 = 2.45e9
    freqs = np.array([0.8 * f0, f0, 1.17 * f0])
    sd = patch_sim(64, 60, 36, nr_ts=900, nf2ff_freqs=freqs)
    ed = sd.build(hip_lib)
    ed.run(900)
    sr = patch_sim(64, 60, 36, nr_ts=900, nf2ff_freqs=freqs, nf2ff_mode="record")
    assert sr.nf2ff_mode == "record" and sr.dft_every == sd.dft_every
    er = sr.build(hip_lib)
    for n in (1, 299, 600):
        er.run(n)
    for a, b in zip(sd.nf2ff_boxes(), sr.nf2ff_boxes()):
        assert np.array_equal(a, b)
    so = patch_sim(64, 60, 36, nr_ts=900, nf2ff_freqs=freqs, nf2ff_mode="record")
    eo = so.build(oracle_lib)
    eo.run(900)
    other = np.array([1.9135e9, 2.2e9])
    bh, bo = sr.nf2ff_boxes(freqs=other), so.nf2ff_boxes(freqs=other)
    assert bh[0].shape[0] == 2 and max(np.abs(b).max() for b in bo) > 0
    for a, b in zip(bh, bo):
        assert rel_l2(a, b) < 1e-12
    with pytest.raises(ValueError, match="above the recorder"):
        sr.nf2ff_boxes(freqs=[9e9])


def test_far_field_taken_at_the_s11_resonance(hip_lib, oracle_lib, tmp_path):
    """Row a13 completed (opt-in: prepared.pattern_at_resonance = True — the reference spells the rule out but never
    reaches it): the microstrip variant picks f_res from S11 and evaluates CalcNF2FF THERE
    (solver_fdtd_openems_microstrip.py:407-433) — possible because the NF2FF faces are recorded in the time domain.
    HIP vs oracle: same f_res, pattern frequency == f_res (the dip is below -10 dB), cuts within 1e-3; and the
    dft-mode fallback (comb) snaps to its nearest recorded frequency and says so in f_pattern."""
    s = pkg("solver_fdtd_hip")
    P = pkg("params").PatchAntennaParams
    p = P.from_user_units(frequency_ghz=2.45, er=4.3, h_mm=1.6, loss_tangent=0.02)
    res = []
    for lib, tag in ((hip_lib, "gpu"), (oracle_lib, "cpu")):
        prep = s.prepare_hip_microstrip_patch(p, feed_direction=s.FeedDirection.NEG_X, boundary="MUR",
                                              work_dir=str(tmp_path / tag), lib=lib)
        assert prep.ok, prep.message
        assert prep.variant == "microstrip"
        prep.FDTD.NrTS = 9000
        prep.pattern_at_resonance = True
        r = s.run_prepared_hip(prep, frequency_hz=p.frequency_hz, verbose=0)
        assert r.ok, r.message
        assert prep.FDTD.sim.nf2ff_mode == "record"
        res.append(r)
    g, c = res
    assert g.s11_dB.min() < -10.0, f"no dip below -10 dB (min {g.s11_dB.min():.1f} dB): the resonance rule cannot be exercised"
    assert g.f_res == c.f_res and g.f_res != p.frequency_hz
    assert g.f_res == g.freq[np.argmin(g.s11_dB)]
    assert g.f_pattern == g.f_res and c.f_pattern == c.f_res
    lin = lambda d: 10.0 ** (np.asarray(d) / 20.0)
    assert rel_l2(lin(g.intensity), lin(c.intensity)) < 1e-3 and rel_l2(g.s11, c.s11) < 1e-3
    # dft-mode fallback: 21-point comb, the far field snaps to the nearest recorded frequency
    prep = s.prepare_hip_microstrip_patch(p, feed_direction=s.FeedDirection.NEG_X, boundary="MUR",
                                          work_dir=str(tmp_path / "comb"), nf2ff_mode="dft")
    prep.FDTD.NrTS = 9000
    prep.pattern_at_resonance = True
    r = s.run_prepared_hip(prep, frequency_hz=p.frequency_hz, verbose=0)
    assert r.ok, r.message
    comb = pkg("openems_api").nf2ff_comb(p.frequency_hz)
    assert prep.FDTD.sim.nf2ff_mode == "dft" and prep.FDTD.sim.nf2ff_freqs.size == comb.size
    assert r.f_res == g.f_res and r.f_pattern in comb and abs(r.f_pattern - r.f_res) <= 0.5 * np.diff(comb).max() * (1 + 1e-9)
    assert rel_l2(lin(r.intensity), lin(g.intensity)) < 0.05


def test_p2p_argument_and_state_checks(hip_lib):
    """Mailbox transport misuse comes back as FDTD_E_* codes, not as device faults: attaching after the first step,
    a neighbour blob that belongs to another grid, a zero self-test token."""
    capi = pkg("_capi")
    sims = [patch_sim(40, 36, 24, nr_ts=20, nf2ff=False) for _ in range(2)]
    engs = [s.build(hip_lib, rank=r, world=2) for r, s in enumerate(sims)]
    blobs = [e.p2p_export() for e in engs]
    other = patch_sim(44, 36, 24, nr_ts=20, nf2ff=False).build(hip_lib, rank=1, world=2)
    with pytest.raises(capi.FdtdError, match="another grid"):
        engs[0].p2p_attach(None, other.p2p_export())
    stepped = patch_sim(40, 36, 24, nr_ts=20, nf2ff=False).build(hip_lib, rank=0, world=2)
    stepped.half_step(capi.PHASE_E); stepped.half_step(capi.PHASE_H)
    with pytest.raises(capi.FdtdError, match="before the first timestep"):
        stepped.p2p_attach(None, blobs[1])
    engs[0].p2p_attach(None, blobs[1])
    engs[1].p2p_attach(blobs[0], None)
    with pytest.raises(capi.FdtdError, match="non-zero"):
        engs[0].p2p_selftest(0)


def test_tutorial_scene_gpu_equals_oracle(hip_lib, oracle_lib, tmp_path):
    """The openEMS tutorial patch that the reference's test_openems.py:19-99 builds (tests/tutorial_scene.py), on the HIP
    library and on the oracle: same stop step, S11(f) and port series to 1e-3 / 1e-4, the same dip inside 2.35-2.60 GHz,
    D within 6-8 dBi, pattern at the dip within 1e-3."""
    import tutorial_scene
    g = tutorial_scene.build_and_run(hip_lib, str(tmp_path / "gpu"))
    c = tutorial_scene.build_and_run(oracle_lib, str(tmp_path / "cpu"))
    assert g["grid"] == c["grid"] and g["steps"] == c["steps"]
    assert rel_l2(g["u"], c["u"]) < 1e-4 and rel_l2(g["i"], c["i"]) < 1e-4 and rel_l2(g["s11"], c["s11"]) < 1e-3
    assert g["f_dip"] == c["f_dip"] and 2.35e9 <= g["f_dip"] <= 2.60e9 and g["dip_dB"] < -10.0
    assert 6.0 <= 10 * np.log10(g["Dmax"]) <= 8.0 and abs(g["Dmax"] - c["Dmax"]) < 1e-6 * c["Dmax"]
    assert rel_l2(g["E_norm"], c["E_norm"]) < 1e-3
    # power balance on the GPU (the CPU twin explains it: tests/test_tutorial_kat_cpu.py): radiated / accepted = 0.95 for this substrate
    assert 0.90 <= g["Prad"] / g["P_acc"] <= 0.985 and abs(g["Prad"] - c["Prad"]) < 1e-6 * c["Prad"] and abs(g["P_acc"] - c["P_acc"]) < 1e-6 * c["P_acc"]


@pytest.mark.parametrize("lag", [0, 1, 3])
@pytest.mark.parametrize("shape,bc,use_classes", [((64, 60, 36), "CPML", True), ((53, 47, 31), "CPML", False),
                                                  ((125, 33, 12), "PEC", True), ((1100, 24, 16), "CPML", True)])
def test_wavefront_schedule_vs_oracle(hip_lib, oracle_lib, shape, bc, use_classes, lag, monkeypatch):
    """One launch per timestep (FDTD_FLAG_KERNEL_WAVEFRONT: E sweep `lag` planes ahead of the H sweep, per-block flags,
    write-through V stores, sc1 V loads) against the oracle: fields bit for bit, port series, NF2FF boxes, chunked runs.
    Shapes: several strips and several blocks per strip, nx not a multiple of 4, rows longer than a block (P4 > 256 threads
    -> the flag set reaches two blocks on), fewer planes than the lag; lag 0 = the library's own choice."""
    capi = pkg("_capi")
    if lag:
        monkeypatch.setenv("FDTD_WF_LAG", str(lag))
    kw = dict(boundary=bc, cpml_cells=4 if shape[2] < 20 else 6, nr_ts=420, use_classes=use_classes, nf2ff=bc == "CPML")
    sh, so = patch_sim(*shape, **kw), patch_sim(*shape, **kw)
    eh = sh.build(hip_lib, flags=capi.FLAG_KERNEL_WAVEFRONT)
    eo = so.build(oracle_lib)
    seeded_fields(eh, 11); seeded_fields(eo, 11)
    for n in (1, 2, 150, 247):
        eh.run(n)
    eo.run(400)
    fh, fo = eh.fields(), eo.fields()
    assert np.isfinite(fo).all() and np.abs(fo).max() > 0
    assert same_values(fh, fo), f"rel L2 {rel_l2(fh, fo):.3e}"
    (uh, ih), (uo, io) = sh.port_series()[0], so.port_series()[0]
    assert len(uh) == 400 and rel_l2(uh, uo) < 1e-12 and rel_l2(ih, io) < 1e-12
    if bc == "CPML":
        for a, b in zip(sh.nf2ff_boxes(), so.nf2ff_boxes()):
            assert rel_l2(a, b) < 1e-12


def test_wavefront_schedule_refuses_what_it_cannot_do(hip_lib):
    """Asked for by name where it cannot run: an error code.  (Mur faces themselves it takes since round 4 — k_step<..., MUR> — but not with a voltage
    probe on a face: the boundary voltages in memory are not final while the launch runs.)"""
    capi = pkg("_capi")
    s = patch_sim(40, 40, 30, boundary="MUR", nr_ts=20, nf2ff=False)
    e = s.build(hip_lib, flags=capi.FLAG_KERNEL_WAVEFRONT)
    e.run(2)
    assert e.schedule_info()["launches_per_timestep"] == 1 and not e.schedule_info()["resident"]
    e = patch_sim(40, 40, 30, boundary="MUR", nr_ts=20, nf2ff=False).build(hip_lib, flags=capi.FLAG_KERNEL_WAVEFRONT)
    e.add_probe(0, np.array([(7 * 40 + 9) * 40 + 0], dtype=np.int64), np.array([1], dtype=np.int8), np.array([1.0], dtype=np.float32))
    with pytest.raises(capi.FdtdError, match="wavefront"):
        e.run(2)


@pytest.mark.parametrize("shape,tys", [((37, 300, 10), 0), ((37, 300, 10), 4), ((64, 60, 36), 40), ((53, 47, 31), 5),
                                       ((1028, 9, 9), 0), ((260, 18, 40), 7), ((16, 9, 12), 0), ((24, 12, 9), 4)])
def test_wavefront_schedule_odd_tilings_equal_two_launches(hip_lib, shape, tys, monkeypatch):
    """The flag sets of the one-launch schedule under unusual tilings — 25 rows per block, one-row strips' worth of blocks,
    strips of 4 / 5 / 7 / 40 rows ($FDTD_TYS), a short last strip, rows longer than a block, more blocks per plane group than
    planes — against the two-launch schedule of the same library (which the rest of the suite pins to the oracle): every
    field value and the port series after 300 steps from seeded random fields."""
    capi = pkg("_capi")
    if tys:
        monkeypatch.setenv("FDTD_TYS", str(tys))
    out = []
    for flags in (capi.FLAG_KERNEL_DIRECT, capi.FLAG_KERNEL_WAVEFRONT):
        s = patch_sim(*shape, boundary="CPML", cpml_cells=3, nr_ts=320, nf2ff=False)
        e = s.build(hip_lib, flags=flags)
        seeded_fields(e, 21)
        e.run(300)
        out.append((s, e))
    (s1, e1), (s2, e2) = out
    f1, f2 = e1.fields(), e2.fields()
    assert np.isfinite(f1).all() and np.abs(f1).max() > 0
    assert same_values(f1, f2), f"rel L2 {rel_l2(f2, f1):.3e}"
    assert rel_l2(s2.port_series()[0][0], s1.port_series()[0][0]) < 1e-12


def test_kernel_schedule_selection(hip_lib, monkeypatch):
    """AUTO: small grids (at most two tiles per CU) resident in registers (round 4: fdtd_profile.fused, one launch holds many timesteps);
    beyond that one launch per timestep on single slabs — all E blocks first on cache-resident grids, H a few planes behind E beyond the
    Infinity Cache — except grids without CPML below 1700 blocks per sweep (two launches, Mur faces included); DIRECT never, WAVEFRONT always."""
    capi = pkg("_capi")
    small = patch_sim(64, 60, 36, nr_ts=40, nf2ff=False)
    assert small.build(hip_lib).schedule_info()["resident"] and small.build(hip_lib).run_profiled(4).fused == 1
    assert small.build(hip_lib, flags=capi.FLAG_KERNEL_DIRECT).run_profiled(4).fused == 0
    mur = patch_sim(64, 60, 36, boundary="MUR", nr_ts=40, nf2ff=False)
    assert mur.build(hip_lib).schedule_info()["resident"]
    assert mur.build(hip_lib, flags=capi.FLAG_KERNEL_DIRECT).run_profiled(4).fused == 0
    monkeypatch.setenv("FDTD_RESIDENT", "0")          # what AUTO takes where the resident schedule does not fit
    assert not small.build(hip_lib).schedule_info()["resident"] and small.build(hip_lib).run_profiled(4).fused == 1
    small_pec = patch_sim(64, 60, 36, boundary="PEC", nr_ts=40, nf2ff=False)
    assert small_pec.build(hip_lib).run_profiled(4).fused == 0
    assert small_pec.build(hip_lib, flags=capi.FLAG_KERNEL_WAVEFRONT).run_profiled(4).fused == 1
    assert mur.build(hip_lib).run_profiled(4).fused == 0
    monkeypatch.delenv("FDTD_RESIDENT")
    big = patch_sim(400, 400, 82, nr_ts=40, nf2ff=False)          # 6 x 84 planes x 640 KB = 323 MB
    assert big.build(hip_lib).run_profiled(4).fused == 1 and not big.build(hip_lib).schedule_info()["resident"]
    assert big.build(hip_lib, flags=capi.FLAG_KERNEL_DIRECT).run_profiled(4).fused == 0
