#!/usr/bin/env python3
"""Headline benchmark: Mcells/s of the 3-D FDTD time-stepping hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--workload NS|C2|C3|C4|C5] [--full] [--dump-outputs DIR]

One bench "step" = `--ts-per-step` (default 500, so the driver's `--steps 20` times BASELINE's 10 000 timesteps) full FDTD timesteps (E half-step + H half-step incl.
CPML, source, port probes and NF2FF running-DFT surfaces) of the named BASELINE workload; default
workload is the north-star 300x300x60 patch-on-FR-4 grid with 10-cell CPML, fp32.  Inputs are
resident in HBM before the timed region.  For N > 1 (launched by torch.distributed.run, one rank
per GPU) the SAME global grid is z-slab decomposed over the ranks (strong scaling, as BASELINE.json
states the target); the halo planes travel inside libfdtd_hip.so — P2P mailboxes written by the update
kernels over xGMI by default, RCCL send/recv on a second stream with `--halo rccl`.

Prints ONE JSON line on rank 0.  A plain run sets up, pre-fills and warms up, times the
K steps and prints the headline (`value`, `ms_per_step`).  With `--full` the line also carries `roofline` (begin-to-end
durations of the dominant kernel, from start / stop events carried by every main launch = the interval a rocprofv3 kernel
trace reports, vs 36 algorithmic bytes per cell per half-step; a profiled pass of its own after the timed steps), at N = 1
`roofline_hbm_resident` (the same measurement on C3, 400x400x80, whose fields do not fit the 256 MiB Infinity Cache), the
side points of the reference's default scenes and `cpu_baseline` (the oracle, test infrastructure, timed on the host cores
as a reported non-target).

`--dump-outputs DIR` writes what the timed path computed by the end of its last step as DIR/<name>.npy (see dump_outputs):
the inputs are fixed by the arguments, so two builds can be compared output for output.
"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = "fdtd-solver-antennas_amd"

SCENES = {"C2": "2.45 GHz patch on FR-4 (fixed scene)", "NS": "2.45 GHz patch on FR-4 (fixed scene)",
          "C3": "2.45 GHz patch on FR-4 (fixed scene)", "C4": "5.8 GHz microstrip-fed patch (microstrip_3d geometry)",
          "C5": "2x2 patch array, 61.2 mm pitch (multi_3d geometry)"}
HBM_PEAK_GBS = 8000.0          # MI355X spec (MI355X_MICROARCH.md: 8 TB/s; 6.29 TB/s measured copy ceiling)
ALGO_BYTES_PER_CELL_HALFSTEP = 36.0   # read 3 + 3 field components, write 3 (fp32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="NS")
    ap.add_argument("--ts-per-step", type=int, default=500)
    ap.add_argument("--cpml-cells", type=int, default=10)
    ap.add_argument("--prefill-seconds", type=float, default=2.5,
                    help="untimed stepping before the warm-up steps, as a number of timesteps fixed by the grid size (seconds x 75 Gcells/s / cells): "
                         "the pulse fills the grid and the GPU leaves its idle clocks (0: only twice the longest axis)")
    ap.add_argument("--halo", default="auto", choices=["auto", "p2p", "rccl", "host"],
                    help="N > 1: halo transport (auto = P2P mailbox, then RCCL, then host copies)")
    ap.add_argument("--partition", default="cost", choices=["cost", "even"],
                    help="N > 1: z-slabs of equal cost (the z-CPML planes weigh 1.4: the end ranks own fewer planes) or of equal plane count")
    ap.add_argument("--raw-operator", action="store_true", help="stream 12 coefficient arrays instead of class bytes")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-hbm-point", action="store_true", help="skip the C3 (HBM-resident) roofline block")
    ap.add_argument("--no-small-grid-point", action="store_true", help="skip the side points: the reference's default GUI scene (resident schedule) and its multi-patch default (MUR, two launches)")
    ap.add_argument("--cpu-steps", type=int, default=0, help="oracle timesteps for the cpu_baseline leg (0 = auto)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: cpu_baseline, the roofline pass, the C3 HBM-resident point and the "
                         "side points of the reference's default scenes (the --no-* options above thin this out)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the fields (a fixed, seeded sample of cells), the port series and the NF2FF surface "
                         "data as DIR/<name>.npy (float32 / float64, < 64 MB in all)")
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("FDTD_BENCH_FORCE_DEVICE") is not None:      # debugging aid: several ranks on one GPU
        local_rank = int(os.environ["FDTD_BENCH_FORCE_DEVICE"])
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node N for --gpus N")
    torch.cuda.set_device(local_rank)
    # launched by torch.distributed.run: bring the process group up also at world 1, so that the one-GPU box exercises the
    # same RCCL ("nccl") bootstrap the N-GPU runs depend on
    use_dist = world > 1 or ("RANK" in os.environ and "MASTER_PORT" in os.environ)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("FDTD_BENCH_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    capi = importlib.import_module(PKG + "._capi")
    wl = importlib.import_module(PKG + ".workloads")
    sc = importlib.import_module(PKG + ".scene")
    simm = importlib.import_module(PKG + ".simulation")
    hip = capi.load_hip_library()           # raises if the HIP library is missing: no fallback

    w = wl.baseline_workload(args.workload)
    vox = sc.voxelize(w.scene, w.grid)
    # The CPU leg FIRST (rank 0, N = 1 only; ~10 s on the host cores), so that everything after it is GPU work and an outside
    # observer sampling the GPU sees the timed region at the end of the run instead of a 10 s CPU phase.
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(capi, simm, w, vox, args)
    # Untimed pre-fill on top of the W warm-up steps: the step time depends on the field VALUES (all-zero fields stream 6-15 %
    # faster, profiles/r02/step_time_vs_field_values.txt), so nothing is timed before the pulse has reached every corner of
    # the grid (<= 0.58 cells per timestep at the Courant limit: twice the longest axis in timesteps)
    # ... and a GPU that has idled (process start, the 10 s CPU leg above) steps up to 10 % slower for its first second or two
    # (profiles/r03/README.md: one default run of this file at 74.9 us per timestep, the same command minutes later at 67.3): the
    # pre-fill lasts ~--prefill-seconds of GPU time, as a timestep count that depends on the grid size only (the same for every N)
    prefill = max(2 * max(w.grid.shape), int(args.prefill_seconds * 75e9 / w.grid.ncells))
    nts_total = (args.steps + args.warmup) * args.ts_per_step * 2 + prefill + 8

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    # N > 1: the halo transport lives inside the library — P2P mailboxes (kernels push the halo planes over xGMI), else RCCL
    # send/recv on a second stream, else host copies; SlabComm.attach falls down that ladder TOGETHER on every rank when one of
    # them cannot set a transport up.  A transport that sets up (and passes its self-test) but fails once timesteps depend on it
    # — every halo wait is bounded and ends in an error, never in a hang — is caught here the same way: the first pre-fill
    # timesteps are the probe, and on an error on any rank all ranks rebuild their slab and take the next transport, so that the
    # run still produces a valid number (and says in `multi_gpu.transports_failed` what happened).
    failed, comm = [], None
    while True:
        sim = simm.Simulation(w.grid, vox, f0=w.f0, fc=w.fc, boundary="CPML", cpml_cells=args.cpml_cells,
                              nr_ts=nts_total, nf2ff_freqs=[w.f0], nf2ff_mode="auto", use_classes=not args.raw_operator)
        eng = sim.build(hip, rank=rank, world=world, device=local_rank, partition=args.partition)
        if world == 1:
            break
        comm = importlib.import_module(PKG + ".distributed").SlabComm(transport=args.halo, skip=[f["transport"] for f in failed])
        comm.attach(sim)
        ok, why = True, ""
        if sim.external_transport is None:
            comm.barrier()                    # every rank starts its first launch now: a halo wait is bounded (10 s), set-up times differ
            try:
                eng.run(min(64, prefill))
            except capi.FdtdError as exc:
                ok, why = False, str(exc)
        if comm._all_agree(ok):
            break
        if args.halo != "auto":
            raise RuntimeError(f"halo transport {comm.transport_used} failed at run time on some rank" + (f": {why}" if why else ""))
        failed.append({"transport": comm.transport_used, "error_on_this_rank": why or None})
        if rank == 0:
            print(f"[bench] halo transport {comm.transport_used} failed at run time; rebuilding with the next one", file=sys.stderr, flush=True)
        comm.barrier()                        # nobody frees a mailbox a neighbour may still write into
        del eng
        sim.engine = None

    def run_steps(n):
        if sim.external_transport is not None:
            sim.external_transport.run_steps(eng, n)
        else:
            eng.run(n)

    tps = args.ts_per_step
    done = int(eng.step)
    while done < prefill:                  # in calls of at most 2000 timesteps (a decomposed grid enqueues two launches per timestep)
        n = min(2000, prefill - done)
        run_steps(n)
        done += n
    for _ in range(args.warmup):
        run_steps(tps)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run_steps(tps)
    barrier()
    elapsed = local_elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    ncells = w.grid.ncells
    timesteps = args.steps * tps
    value = ncells * timesteps / elapsed / 1e6
    if args.dump_outputs:                       # before anything else steps the grid: the state the last timed step left
        dump_outputs(args.dump_outputs, sim, eng, w.grid, world, rank, comm)

    # roofline of the dominant kernel (E half-step == H half-step in algorithmic bytes): a second pass of the same
    # length in which every main launch carries start / stop events (hipExtLaunchKernelGGL) = the dispatch's begin
    # and end timestamps, the interval a rocprofv3 kernel trace reports; nothing is subtracted.
    prof = roofline = None
    if args.full:
        if sim.external_transport is not None:      # host transport: no in-library step loop to profile
            run_steps(min(timesteps, 2000))         # the same second pass, so that every transport ends on the same timestep
            prof = capi.FdtdProfile(ms_total=elapsed * 1e3, ms_update_e=float("nan"), ms_update_h=float("nan"), steps=timesteps)
        else:
            prof = eng.run_profiled(min(timesteps, 2000))
        roofline = roofline_block(args.workload, eng, prof, world, sim.external_transport is not None, elapsed / timesteps * 1e3)
    finite = bool(np.isfinite(eng.get_field(0, 2)).all())
    # L2 norm of the first port's voltage series over every timestep stepped so far (rank-summed): identical for every
    # N and every halo transport, since the decomposed run is bit-identical to the single-slab run
    u0 = sim.port_series(comm.allreduce if world > 1 else None)[0][0]
    port_u_l2 = float(np.sqrt(np.sum(np.asarray(u0, float) ** 2)))

    # N > 1: what shows that the ranks really stepped ONE coupled grid — every rank answers (ranks_seen), the transport
    # they agreed on, the size of the RCCL communicator when that is the transport, each rank's own time per step, and
    # max|V| of every slab (the port sits in one slab: any other slab is non-zero only through its halos)
    coupling = None
    if world > 1:
        seen = comm.allreduce(np.array([1.0]))
        vmax = max(float(np.abs(eng.get_field(0, c)).max()) for c in range(3))
        rec = [None] * world
        zl = simm.plane_costs(w.grid.shape[2], *sim.bc.face_cells()[4:6], w_layer=2.0) > 1.5     # planes inside the z-CPML layers
        sched = eng.schedule_info()
        mine = {"rank": rank, "ms_per_step": round(local_elapsed / args.steps * 1e3, 4),
                "us_per_timestep": round(local_elapsed / timesteps * 1e6, 3),
                "slab_k0": int(eng.k0), "slab_planes": int(eng.nk), "slab_z_cpml_planes": int(zl[eng.k0:eng.k0 + eng.nk].sum()),
                "slab_max_abs_V": vmax, "device": local_rank,
                "launches_per_timestep": sched["launches_per_timestep"], "lag_planes": sched["lag_planes"],
                "us_main_kernels": None if prof is None or not (prof.ms_update_e == prof.ms_update_e) else round((prof.ms_update_e + prof.ms_update_h) * 1e3, 3),
                "ms_halo_host_exchange": round(getattr(comm, "ms_exchange", 0.0) / max(args.steps + args.warmup, 1), 4),
                "rccl_nranks": eng.comm_nranks()}
        if comm.transport_used == "p2p":     # what the runtime says about the way to each neighbour's GPU: xGMI or PCIe, hops
            mine["link_down"] = eng.p2p_link_info(0) if rank > 0 else None
            mine["link_up"] = eng.p2p_link_info(1) if rank + 1 < world else None
            mine["ms_p2p_selftest"] = round(comm.ms_selftest, 3)
        dist.all_gather_object(rec, mine)
        t_rank = [r["us_per_timestep"] for r in rec]
        coupling = {"ranks_seen": int(round(float(seen[0]))), "transport_used": comm.transport_used, "transports_failed": failed,
                    "partition": args.partition, "z_layer_plane_cost": simm.Z_LAYER_PLANE_COST,
                    "rccl_nranks": rec[0]["rccl_nranks"], "per_rank": rec,
                    "rank_time_max_over_mean": round(max(t_rank) / (sum(t_rank) / len(t_rank)), 4),
                    "all_slabs_excited": bool(all(r["slab_max_abs_V"] > 0 for r in rec))}
        # A transport other than the mailbox has a per-timestep floor that does not depend on the slab: say so next to the number it limits.
        # (one MI355X, an interior north-star slab whose halos go to itself: profiles/r04/halo_transport_thin_slab_timing.txt)
        if comm.transport_used == "rccl":
            coupling["transport_note"] = ("fell back to RCCL send/recv: measured floor 43 us per timestep on a 7-plane slab and 52 us on a 17-plane slab "
                                          "(exchange in stream order on the compute stream; 85 us with the overlapped schedule) against 19 / 27 us with the "
                                          "P2P mailbox — thin slabs do not scale on this transport")
        elif comm.transport_used == "host":
            coupling["transport_note"] = "fell back to host-copied halos (fdtd_half_step + torch.distributed send/recv): a debugging transport, milliseconds per timestep"
    operator_form, steps_total = sim.operator_form, int(eng.step)
    hbm_point = None
    if args.full and rank == 0 and world == 1 and not args.no_hbm_point and args.workload != "C3":
        del eng
        sim.engine = None                     # frees the NS context before the C3 one is built
        hbm_point = hbm_resident_point(capi, wl, sc, simm, hip, args)
    small_point = None
    if args.full and rank == 0 and world == 1 and not args.no_small_grid_point:
        try:
            small_point = small_grid_point(capi, simm, hip)
        except Exception as exc:      # the side point never takes the headline number down with it
            small_point = {"error": f"{type(exc).__name__}: {exc}"}
    mur_point = None
    if args.full and rank == 0 and world == 1 and not args.no_small_grid_point:
        try:
            mur_point = mur_scene_point(hip)
        except Exception as exc:
            mur_point = {"error": f"{type(exc).__name__}: {exc}"}
    if world > 1:
        dist.barrier()
    if rank == 0:
        out = {
            "metric": "Mcells/s (Yee cells x steps / s)", "value": round(value, 1), "unit": "Mcells/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{args.workload}: {w.grid.shape[0]}x{w.grid.shape[1]}x{w.grid.shape[2]} "
                                   f"{SCENES.get(args.workload, 'patch')}, CPML-{args.cpml_cells}, "
                                   f"{len(vox.ports)} lumped port(s), NF2FF surfaces ({sim.nf2ff_mode})",
                       "cells": ncells, "timesteps_per_step": tps, "prefill_timesteps": prefill, "operator": operator_form,
                       "parallelism": f"z-slab x{world}, halo transport {comm.transport_used}" if world > 1 else "single GPU",
                       "fields_finite": finite, "port_u_l2": port_u_l2, "timesteps_total": steps_total},
        }
        if roofline is not None:
            out["roofline"] = roofline
        if hbm_point is not None:
            out["roofline_hbm_resident"] = hbm_point
        if small_point is not None:
            out["small_grid_point"] = small_point
        if mur_point is not None:
            out["mur_scene_point"] = mur_point
        if coupling is not None:
            out["multi_gpu"] = coupling
        if cpu is not None:
            out["cpu_baseline"] = cpu
        print(json.dumps(out), flush=True)
    if use_dist:
        if world == 1:
            dist.barrier()
        dist.destroy_process_group()


DUMP_SEED = 20240917
DUMP_FIELD_CELLS = 1 << 20      # cells sampled per field component (float32: 4 MiB each, 24 MiB for the six)
DUMP_SERIES_MAX = 1 << 17       # samples kept per port series (float64: 1 MiB each)
DUMP_NF2FF_MAX = 1 << 20        # complex NF2FF surface values kept (real and imaginary part: 16 MiB)


def _dump_sample(n, cap, salt):
    """Sorted indices of a fixed, seeded sample of `cap` out of `n` (all of them when n <= cap): the same for every run."""
    import numpy as np
    if n <= cap:
        return np.arange(n)
    return np.sort(np.random.default_rng([DUMP_SEED, salt]).choice(n, cap, replace=False))


def dump_outputs(out_dir, sim, eng, grid, world, rank, comm):
    """What a caller of the timed path receives after its last step, as out_dir/<name>.npy:
      V_x V_y V_z I_x I_y I_z  float32  the six field components (E as voltages, H as currents) at a fixed, seeded sample of
                                        cells of the whole grid (all cells when the grid is small), in the order of `cell_index`
      cell_index               float64  flat index k*ny*nx + j*nx + i of every sampled cell
      port<P>_u, port<P>_i     float64  voltage / current series of lumped port P (a fixed sample when longer than 2^17)
      nf2ff_re, nf2ff_im       float64  the NF2FF surface data (all recording boxes, flattened in order; a fixed sample when larger)
    At N > 1 every rank contributes its slab and rank 0 writes."""
    import numpy as np
    import torch.distributed as dist
    allreduce = comm.allreduce if world > 1 else None
    nz, ny, nx = grid.shape[2], grid.shape[1], grid.shape[0]
    idx = _dump_sample(nz * ny * nx, DUMP_FIELD_CELLS, 0)
    lo = int(eng.k0) * ny * nx
    mine = idx[(idx >= lo) & (idx < lo + int(eng.nk) * ny * nx)] - lo
    arrays = {"cell_index": idx.astype(np.float64)}
    for kind, kname in ((0, "V"), (1, "I")):
        for c, cname in enumerate("xyz"):
            vals = eng.get_field(kind, c).reshape(-1)[mine]
            if world > 1:
                parts = [None] * world
                dist.all_gather_object(parts, vals)
                vals = np.concatenate(parts)            # slabs in rank order = ascending k
            assert vals.size == idx.size
            arrays[f"{kname}_{cname}"] = vals.astype(np.float32)
    for p, (u, i) in enumerate(sim.port_series(allreduce)):
        for tag, a in (("u", u), ("i", i)):
            a = np.asarray(a, np.float64)
            arrays[f"port{p}_{tag}"] = a[_dump_sample(a.size, DUMP_SERIES_MAX, 1 + 2 * p + (tag == "i"))]
    if sim.nf2ff_freqs is not None and len(sim.nf2ff_freqs):
        flat = np.concatenate([np.asarray(b, np.complex128).reshape(-1) for b in sim.nf2ff_boxes(allreduce)])
        flat = flat[_dump_sample(flat.size, DUMP_NF2FF_MAX, 1000)]
        arrays["nf2ff_re"], arrays["nf2ff_im"] = flat.real.copy(), flat.imag.copy()
    if rank != 0:
        return
    assert sum(a.nbytes for a in arrays.values()) < 64_000_000
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def working_set_bytes(eng):
    """Six field arrays + class bytes of the slab (what the two sweeps stream every timestep)."""
    return int(eng.nk) * int(eng.ny) * int(eng.nx) * (6 * 4 + 1)


def roofline_block(workload, eng, prof, world, host_transport, ms_timestep):
    own_cells = eng.nk * eng.ny * eng.nx
    algo_bytes = ALGO_BYTES_PER_CELL_HALFSTEP * own_cells
    ms_e, ms_h = prof.ms_update_e, prof.ms_update_h
    one_launch = bool(getattr(prof, "fused", 0))     # wavefront schedule (k_step): E and H half-step of all planes in ONE launch
    if one_launch:
        dom, ms_dom, ms_h = "step", ms_e, 0.0
        algo_bytes *= 2                               # 36 B per cell and half-step, two half-steps per launch
    else:
        dom = "update_E" if ms_e >= ms_h else "update_H"
        ms_dom = max(ms_e, ms_h)
    if host_transport or not (ms_dom == ms_dom and ms_dom > 0):
        # host halo transport: kernels are launched one half-step at a time, nothing to profile
        return {"bound": "hbm", "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None,
                "traffic": None, "kernel": dom, "algorithmic_bytes_per_launch": algo_bytes}
    achieved = algo_bytes / (ms_dom * 1e-3) / 1e9
    ms_ts = prof.ms_total / prof.steps
    # one launch may hold several timesteps (cache-resident single slabs): ms_update_E is the main-launch time PER TIMESTEP
    # (the launches' durations summed, over the timesteps), the bytes are per timestep too; a kernel trace shows the launches
    launches = int(getattr(prof, "launches_e", 0)) or int(prof.steps)
    ts_per_launch = prof.steps / launches if one_launch else 1.0
    traffic, source = pmc_traffic(workload, dom, world)
    ws = working_set_bytes(eng)
    out = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
           "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
           "traffic_source": source, "kernel": dom, "ms_update_E": round(ms_e, 5), "ms_update_H": round(ms_h, 5),
           "algorithmic_bytes_per_launch": algo_bytes * ts_per_launch, "algorithmic_bytes_per_timestep": algo_bytes,
           "timesteps_per_launch": round(ts_per_launch, 2), "ms_per_launch": round(ms_dom * ts_per_launch, 5),
           "schedule": (("k_step: all E blocks, then all H blocks of a timestep; several timesteps per launch (cut where the NF2FF faces are sampled)"
                         if ts_per_launch > 1.0 else
                         "one launch per timestep (k_step: all E blocks, then all H blocks; beyond the Infinity Cache the H sweep a few planes behind the E sweep)")
                        if one_launch else "two launches per timestep"),
           "kernel_timing": "dispatch begin/end timestamps (start/stop events on every main launch), nothing subtracted",
           "ms_per_timestep_profiled": round(ms_ts, 5),
           # the 256 MiB Infinity Cache holds the whole working set of the smaller grids: their 'HBM' rate is a cache rate
           "resident": "infinity-cache" if ws < (240 << 20) else "hbm", "working_set_bytes": ws}
    if world == 1:
        # against the UNPROFILED timestep of the timed region (the profiled pass pays for its events): the two main
        # launches cannot take longer than the timestep; on a grid that fills the chip they leave only the launch gaps
        # and the occasional DFT launch (0.96-0.99 measured; lower on small grids and under a profiler, which slows the
        # dispatches of the timed region).  More than the timestep means the kernel timing is broken.
        ratio = (ms_e + ms_h) / ms_timestep
        out["ms_per_timestep"] = round(ms_timestep, 5)
        out["kernels_over_timestep"] = round(ratio, 4)
        under_profiler = any("rocprof" in os.environ.get(k, "").lower() for k in ("LD_PRELOAD", "HSA_TOOLS_LIB", "ROCP_TOOL_LIBRARIES"))
        if under_profiler:     # a tracing tool stretches the event-carrying dispatches of the profiled pass: no verdict
            out["kernels_over_timestep_note"] = "under a profiler: not checked"
        else:                  # recorded, not asserted: a bench line with a flag beats no bench line
            out["kernel_timing_consistent"] = bool(ratio <= 1.03)
    return out


def hbm_resident_point(capi, wl, sc, simm, hip, args, name="C3", steps=300):
    """The same roofline measurement on C3 (400x400x80): 307 MB of fields do not fit the 256 MiB Infinity Cache, so this
    is the HBM-resident point of the chip for this kernel (the north-star grid is cache-resident)."""
    w = wl.baseline_workload(name)
    vox = sc.voxelize(w.scene, w.grid)
    sim = simm.Simulation(w.grid, vox, f0=w.f0, fc=w.fc, boundary="CPML", cpml_cells=args.cpml_cells,
                          nr_ts=4 * steps + 2 * max(w.grid.shape) + 64, nf2ff_freqs=[w.f0], use_classes=not args.raw_operator)
    eng = sim.build(hip)
    eng.run(max(steps // 2, 2 * max(w.grid.shape)))      # fields non-zero everywhere before anything is timed (see main)
    t0 = time.perf_counter()
    eng.run(steps)
    dt = time.perf_counter() - t0
    prof = eng.run_profiled(steps)
    blk = roofline_block(name, eng, prof, 1, False, dt / steps * 1e3)
    blk["workload"] = f"{name}: {w.grid.shape[0]}x{w.grid.shape[1]}x{w.grid.shape[2]} fixed scene, CPML-{args.cpml_cells}, {steps} timesteps"
    blk["value_mcells_s"] = round(w.grid.ncells * steps / dt / 1e6, 1)
    return blk


def small_grid_point(capi, simm, hip):
    """The grid the reference's GUI runs by default — prepare_*_patch_fixed: 56x55x50 graded mesh, MUR on all faces, to -40 dB
    (solver_fdtd_openems_fixed.py:113-342) — through the plugin path, time stepping only: the resident schedule (csrc/resident.hip).  Not the
    headline metric (latency-bound: 11 MB of algorithmic bytes per timestep); reported because it is what a user of the reference runs first."""
    import tempfile
    import numpy as np
    sol = importlib.import_module(PKG + ".solver_fdtd_hip")
    par = importlib.import_module(PKG + ".params")
    p = par.PatchAntennaParams.from_user_units(frequency_ghz=2.45, er=4.3, h_mm=1.6, loss_tangent=0.02)
    best = None
    with tempfile.TemporaryDirectory() as td:
        for rep in range(2):           # (the first call pays the table set-up of a new context shape)
            prep = sol.prepare_hip_patch_fixed(p, work_dir=os.path.join(td, f"w{rep}"))
            if not prep.ok:
                return {"error": prep.message}
            res = sol.run_prepared_hip(prep, frequency_hz=p.frequency_hz, verbose=0)
            if not res.ok:
                return {"error": res.message}
            st = res.stats
            sched = prep.FDTD.sim.engine.schedule_info()
            rec = {"workload": f"reference default scene (fixed): {st['grid'][0]}x{st['grid'][1]}x{st['grid'][2]} graded mesh, MUR, to -40 dB",
                   "timesteps": st["steps"], "seconds_stepping": round(st["seconds"], 4), "value_mcells_s": round(st["mcells_per_s"], 1),
                   "us_per_timestep": round(st["seconds"] / max(st["steps"], 1) * 1e6, 3), "energy_db": round(st["energy_db"], 2),
                   "schedule": "resident in registers" if sched["resident"] else f"{sched['launches_per_timestep']} launch(es) per timestep",
                   "workgroups": sched["blocks_per_sweep"], "algorithmic_bytes_per_timestep": 72 * st["cells"],
                   "bound": "latency (two device-scope tile-halo hops per timestep)", "Dmax_dBi": round(float(10 * np.log10(res.Dmax)), 3)}
            if best is None or rec["value_mcells_s"] > best["value_mcells_s"]:
                best = rec
    return best


def mur_scene_point(hip):
    """The reference's multi-patch default — prepare_*_microstrip_multi_3d: a 2 x 2 array on a 143x129x89 graded mesh, MUR on all faces
    (solver_fdtd_openems_microstrip_multi_3d.py:102), four lumped ports of 1 350 edges each — through the plugin path, time stepping only: beyond
    the resident schedule, two launches per timestep with no Mur apply pass (kernels.hip: mur_load_V).  A side point like small_grid_point."""
    import tempfile
    import numpy as np
    sol = importlib.import_module(PKG + ".solver_fdtd_hip")
    par = importlib.import_module(PKG + ".params")
    p = par.PatchAntennaParams.from_user_units(frequency_ghz=2.45, er=4.3, h_mm=1.6, loss_tangent=0.02)
    arr = [sol.PatchInstance(f"P{n}", p, (ix - 0.5) * 0.0612, (iy - 0.5) * 0.0612, 0.0, sol.FeedDirection.NEG_X)
           for n, (ix, iy) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)])]
    with tempfile.TemporaryDirectory() as td:
        prep = sol.prepare_hip_microstrip_multi_3d(arr, work_dir=os.path.join(td, "w"), lib=hip)
        if not prep.ok:
            return {"error": prep.message}
        res = sol.run_prepared_hip(prep, frequency_hz=p.frequency_hz, verbose=0)
        if not res.ok:
            return {"error": res.message}
        st = res.stats
        sched = prep.FDTD.sim.engine.schedule_info()
        return {"workload": f"reference multi-patch default (multi_3d 2x2): {st['grid'][0]}x{st['grid'][1]}x{st['grid'][2]} graded mesh, MUR, 4 ports",
                "timesteps": st["steps"], "seconds_stepping": round(st["seconds"], 4), "value_mcells_s": round(st["mcells_per_s"], 1),
                "us_per_timestep": round(st["seconds"] / max(st["steps"], 1) * 1e6, 3), "energy_db": round(st["energy_db"], 2),
                "schedule": "resident in registers" if sched["resident"] else f"{sched['launches_per_timestep']} launch(es) per timestep",
                "algorithmic_bytes_per_timestep": 72 * st["cells"], "Dmax_dBi": round(float(10 * np.log10(res.Dmax)), 3)}


def pmc_traffic(workload, kernel, world):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes (FETCH_SIZE and
    WRITE_SIZE in separate runs, FETCH_SIZE doubled per the gfx950 correction) — profiles/<round>/
    pmc_traffic_<workload>_*.json.  Counters cannot be collected from inside this process, so this is
    null unless a committed measurement exists for this workload at N = 1."""
    import glob
    if world != 1:
        return None, None
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", f"pmc_traffic_{workload}*.json")))
    if not files:
        return None, None
    try:
        data = json.load(open(files[-1]))["per_launch_traffic"]
        want = kernel.replace("update_", "k_update_").replace("step", "k_step")
        # per TIMESTEP, like `achieved`: the launches that hold several timesteps first (their bytes over their timesteps)
        for name, rec in sorted(data.items(), key=lambda kv: "total_bytes_per_timestep" not in kv[1]):
            if want in name:
                return round(rec.get("total_bytes_per_timestep", rec["total_bytes"])), (
                    "committed rocprofv3 --pmc passes (bytes per timestep), not measured in this run: " + os.path.relpath(files[-1], ROOT))
    except (OSError, KeyError, ValueError):
        pass
    return None, None


def usable_cores() -> int:
    """Host cores this process may really use: min(affinity mask, cgroup cpu.max quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def cpu_baseline(capi, simm, w, vox, args):
    """The oracle (plain-C restatement, OpenMP) on a bounded sample of the same workload."""
    import numpy as np
    so = os.path.join(ROOT, "oracle", "libfdtd_oracle.so")
    if not os.path.isfile(so):
        return None
    cores = usable_cores()
    os.environ["OMP_NUM_THREADS"] = str(cores)
    ora = capi.bind(ctypes.CDLL(so))
    ora.fdtd_oracle_set_threads(cores)
    cores = int(ora.fdtd_oracle_get_threads())
    nr_cap = 20000
    sim = simm.Simulation(w.grid, vox, f0=w.f0, fc=w.fc, boundary="CPML", cpml_cells=args.cpml_cells,
                          nr_ts=nr_cap, nf2ff_freqs=[w.f0])
    e = sim.build(ora)
    rng = np.random.default_rng(0)
    for kind in (0, 1):        # non-zero start: avoids x86 denormal stalls of the all-zero initial state
        for c in range(3):
            e.set_field(kind, c, (1e-3 * rng.standard_normal(e.local_shape)).astype(np.float32))
    e.run(8)                   # untimed: first touch of the arrays, thread start-up
    steps, dt, chunk = 0, 0.0, 50
    while dt < 10.0 and steps + chunk < nr_cap - 16:      # bounded sample: ~10 s of CPU work
        t0 = time.perf_counter()
        e.run(chunk)
        dt += time.perf_counter() - t0
        steps += chunk
    if args.cpu_steps:
        t0 = time.perf_counter()
        e.run(args.cpu_steps)
        dt, steps = time.perf_counter() - t0, args.cpu_steps
    return {"value": round(w.grid.ncells * steps / dt / 1e6, 1), "unit": "Mcells/s", "cores": cores,
            "kind": "port",
            "sample": f"{steps} timesteps of the same {w.grid.shape[0]}x{w.grid.shape[1]}x{w.grid.shape[2]} workload "
                      f"(oracle/libfdtd_oracle.so, OpenMP, seeded non-zero fields), {dt:.1f} s"}


if __name__ == "__main__":
    main()
