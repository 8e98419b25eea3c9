#!/usr/bin/env python3
"""Randomised differential run: libfdtd_hip.so against the CPU oracle on grids, boundaries and schedules nobody picked by hand.

Every case draws a grid shape (odd sizes, rows of 2 ... 65 four-cell groups, 12 ... 48 planes), a boundary per face (PEC / MUR / CPML, or
CPML on all six), a layer thickness, the operator form (class bytes / raw arrays), the kernel schedule (AUTO, two launches per timestep,
one launch per timestep forced, resident in registers forced), the tiling ($FDTD_TYS), the timesteps per launch ($FDTD_WF_MULTI), whether the XCD shares are measured
($FDTD_XCD_ADAPT), NF2FF faces as running sums / recorded samples / none, random initial fields, and a list of run() calls of random
length (the launches of several timesteps are cut at calls and at NF2FF sample steps).  The same list goes to both engines through the
same C ABI; compared: all six field components as IEEE values (bit for bit wherever the oracle's value is non-zero), the port series and
the energy to 1e-12, the NF2FF face spectra to 1e-6 of their largest entry (float32 sums in another order).

    python tests/fuzz_parity.py [--cases 60] [--seed 1] [--only N]     # on a GPU box; prints one line per case, exits 1 on a mismatch
    python tests/fuzz_parity.py --slabs ...     # decomposed runs: 2 ... 6 z-slabs of drawn partition and schedules, coupled through their P2P
                                                # mailboxes in one process (fdtd_run_linked), against ONE slab on the oracle ("lag" column: planes per slab)
    python tests/fuzz_parity.py --media ...     # scenes with Debye media and / or conducting sheets (k_debye, k_sheet and their place in the step
                                                # loop) against the oracle's half-steps plus the numpy restatement of the two corrections
                                                # (draw_media_case / run_media_case below); tests/test_media_fuzz_cpu.py guards what the draw covers
    python tests/fuzz_parity.py --corrections ...   # scenes with at least three of the eight corrections of the step loop, often all of them (Debye and
                                                # Lorentz media, sheets, elements, magnetic faces, conformal faces, a plane wave, H-field excitations), against
                                                # tests/restatement.py (draw_corrections_case / run_corrections_case); tests/test_corrections_fuzz_cpu.py guards the draw

Lives under tests/ because it loads the oracle (test infrastructure); tests/test_round3_gpu.py::test_randomised_cases_equal_the_oracle
runs a fixed-seed batch of it in the -m gpu suite.
"""
import argparse
import ctypes
import importlib
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "fdtd-solver-antennas_amd"
ENV_KNOBS = ("FDTD_TYS", "FDTD_WF_MULTI", "FDTD_XCD_ADAPT", "FDTD_WF_LAG", "FDTD_RESIDENT", "FDTD_RES_CHUNK", "FDTD_MUR_APPLY_PASS")


def _mod(name):
    return importlib.import_module(PKG + "." + name)


def draw_case(rng, mur=False):
    """One case as a plain dict (printable, reproducible from --seed / --only)."""
    nx = int(rng.choice([rng.integers(8, 40), rng.integers(40, 141), 4 * rng.integers(3, 30) + 1, 4 * rng.integers(3, 30)]))
    ny = int(rng.choice([rng.integers(8, 30), rng.integers(30, 121)]))
    nz = int(rng.integers(12, 49))
    r = rng.random()
    if r < 0.4:
        kinds = ["CPML"] * 6
    elif r < 0.8:
        kinds = [str(rng.choice(["PEC", "CPML", "CPML"])) for _ in range(6)]
    else:
        kinds = [str(rng.choice(["PEC", "MUR", "CPML"])) for _ in range(6)]
    if rng.random() < 0.12:      # now and then a grid of a few thousand blocks per half-step (several blocks per CU, every XCD share long)
        nx, ny, nz = int(rng.integers(150, 260)), int(rng.integers(120, 220)), int(rng.integers(24, 44))
    if mur:      # --mur: every case has Mur faces (all six, or mixed with PEC / CPML) and mostly runs on the launch-per-half-step schedules
        kinds = ["MUR"] * 6 if rng.random() < 0.5 else [str(rng.choice(["PEC", "MUR", "MUR", "CPML"])) for _ in range(6)]
        if "MUR" not in kinds:
            kinds[int(rng.integers(0, 6))] = "MUR"
    cells_max = max(2, min(12, (min(nx, ny, nz) - 8) // 2))
    cells = int(rng.integers(2, cells_max + 1))
    has_mur = "MUR" in kinds
    sched = str(rng.choice(["auto", "direct", "wavefront", "resident"] if has_mur else ["auto", "direct", "wavefront", "wavefront", "resident"]))
    env = {}
    # round 4: AUTO steps small grids resident in registers; half of the AUTO cases keep the schedules AUTO took before (they still serve
    # every grid that does not fit the chip), and the resident launches are cut short now and then
    if sched == "auto" and rng.random() < 0.5:
        env["FDTD_RESIDENT"] = "0"
    if mur:
        if sched != "resident" and rng.random() < 0.8:
            env["FDTD_RESIDENT"] = "0"
        if rng.random() < 0.25:      # the apply pass as a launch of its own (three launches per timestep) instead of inside update_H (two)
            env["FDTD_MUR_APPLY_PASS"] = "1"
    if rng.random() < 0.3:
        env["FDTD_RES_CHUNK"] = str(int(rng.choice([1, 2, 7, 33])))
    if rng.random() < 0.4:
        env["FDTD_TYS"] = str(int(rng.choice([1, 2, 3, 4, 5, 7, 9, 16, 40])))
    if rng.random() < 0.5:
        env["FDTD_WF_MULTI"] = str(int(rng.choice([1, 2, 3, 5, 64])))
    if rng.random() < 0.3:
        env["FDTD_XCD_ADAPT"] = "0"
    if sched == "wavefront" and rng.random() < 0.3:
        env["FDTD_WF_LAG"] = str(int(rng.choice([0, 1, 2, 3])))
    nf = str(rng.choice(["none", "dft", "record"]))
    ncalls = int(rng.integers(1, 6))
    calls = [int(rng.integers(1, 90)) for _ in range(ncalls)]
    return {"shape": (nx, ny, nz), "kinds": kinds, "cells": cells, "classes": bool(rng.random() < 0.7), "sched": sched, "env": env,
            "nf2ff": nf, "calls": calls, "seed": int(rng.integers(1, 1 << 30))}


def run_case(case, hip, oracle):
    capi, wl, sc, simm = _mod("_capi"), _mod("workloads"), _mod("scene"), _mod("simulation")
    nx, ny, nz = case["shape"]
    w = wl.patch_workload("fuzz", nx=nx, ny=ny, nz=nz)
    vox = sc.voxelize(w.scene, w.grid)
    flags = {"auto": 0, "direct": capi.FLAG_KERNEL_DIRECT, "wavefront": capi.FLAG_KERNEL_WAVEFRONT, "resident": capi.FLAG_KERNEL_RESIDENT}[case["sched"]]
    total = sum(case["calls"])
    saved = {k: os.environ.pop(k, None) for k in ENV_KNOBS}
    os.environ.update(case["env"])
    out = []
    try:
        for lib in (hip, oracle):
            sim = simm.Simulation(w.grid, vox, f0=w.f0, fc=w.fc, boundary=case["kinds"], cpml_cells=case["cells"], nr_ts=total + 8,
                                  nf2ff_freqs=None if case["nf2ff"] == "none" else [w.f0, 1.3 * w.f0], use_classes=case["classes"],
                                  nf2ff_mode="dft" if case["nf2ff"] == "none" else case["nf2ff"])
            eng = sim.build(lib, flags=flags if lib is hip else 0)
            rng = np.random.default_rng(case["seed"])
            for kind in (0, 1):
                for c in range(3):
                    eng.set_field(kind, c, (1e-3 * rng.standard_normal(eng.local_shape)).astype(np.float32))
            for n in case["calls"]:
                eng.run(n)
            out.append((sim, eng))
    finally:
        for k in ENV_KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    (sh, eh), (so, eo) = out
    problems = []
    fh, fo = eh.fields(), eo.fields()
    if not np.isfinite(fo).all() or not np.abs(fo).max() > 0:
        problems.append("oracle fields not finite / all zero")
    if not np.array_equal(fh, fo):
        bad = np.argwhere(fh != fo)
        problems.append(f"fields differ at {len(bad)} of {fo.size} entries, first {tuple(bad[0])}: {fh[tuple(bad[0])]!r} vs {fo[tuple(bad[0])]!r}")
    else:
        nzm = fo != 0
        if not np.array_equal(fh[nzm].view(np.uint32), fo[nzm].view(np.uint32)):
            problems.append("fields equal as values but not as bits where the oracle is non-zero")
    uh, uo = sh.port_series()[0], so.port_series()[0]
    for q, name in ((0, "port voltage"), (1, "port current")):
        a, b = np.asarray(uh[q], float), np.asarray(uo[q], float)
        if a.shape != b.shape or np.linalg.norm(a - b) > 1e-12 * max(np.linalg.norm(b), 1e-300):
            problems.append(f"{name} series differs")
    ea, eb = np.array(eh.energy()), np.array(eo.energy())
    if np.abs(ea - eb).max() > 1e-12 * np.abs(eb).max():
        problems.append(f"energy {ea!r} vs {eb!r}")
    if case["nf2ff"] != "none":
        bh, bo = sh.nf2ff_boxes(), so.nf2ff_boxes()
        worst = max(float(np.abs(np.asarray(a) - np.asarray(b)).max()) / max(float(np.abs(b).max()), 1e-300) for a, b in zip(bh, bo))
        if len(bh) != len(bo) or not worst <= 1e-6:
            problems.append(f"NF2FF face spectra differ ({worst:.2e} of the largest entry)")
    info = eh.schedule_info()
    return problems, info


def draw_slab_case(rng):
    """A decomposed run: 2 ... 6 z-slabs in this process on one GPU, coupled only through their P2P mailboxes (the transport of
    `bench.py --gpus N`), each slab under its own drawn schedule, against ONE slab on the oracle."""
    world = int(rng.integers(2, 7))
    nx = int(rng.choice([rng.integers(12, 60), rng.integers(60, 161), 4 * rng.integers(4, 30) + 1]))
    ny = int(rng.choice([rng.integers(10, 40), rng.integers(40, 141)]))
    nz = int(rng.integers(max(14, 3 * world + 2), 64))
    if rng.random() < 0.15:
        nx, ny = int(rng.integers(160, 300)), int(rng.integers(150, 260))       # slabs of more than one round of resident blocks
    kinds = ["CPML"] * 6 if rng.random() < 0.6 else [str(rng.choice(["PEC", "CPML", "CPML"])) for _ in range(6)]
    cells = int(rng.integers(2, max(2, min(12, (min(nx, ny, nz) - 8) // 2)) + 1))
    env = {}
    if rng.random() < 0.3:
        env["FDTD_TYS"] = str(int(rng.choice([1, 2, 3, 5, 7, 16])))
    sched = [str(rng.choice(["auto", "direct", "wavefront"])) for _ in range(world)]
    # All these slabs share ONE GPU here (AUTO then takes two launches: api.hip, wavefront_active).  Forcing one launch per timestep on some of
    # them keeps blocks resident that spin on a neighbour's halo; with thousands of small blocks per sweep (one-row strips of a 199 x 233
    # plane, six slabs) the spinning blocks of four such kernels held every slot of the chip and the two-launch kernels they waited for
    # never got one — a property of the shared GPU, not of the protocol.  Forced mixtures therefore stay below one round of resident blocks.
    if "wavefront" in sched and any(x != "wavefront" for x in sched):
        env.pop("FDTD_TYS", None)
        nx, ny = min(nx, 120), min(ny, 100)
        cells = min(cells, max(2, (min(nx, ny, nz) - 8) // 2))
    return {"world": world, "shape": (nx, ny, nz), "kinds": kinds, "cells": cells, "classes": bool(rng.random() < 0.7),
            "partition": str(rng.choice(["cost", "even"])), "sched": sched,
            "env": env, "nf2ff": str(rng.choice(["none", "dft"])), "calls": [int(rng.integers(1, 70)) for _ in range(int(rng.integers(1, 5)))],
            "seed": int(rng.integers(1, 1 << 30))}


def run_slab_case(case, hip, oracle):
    capi, wl, sc, simm = _mod("_capi"), _mod("workloads"), _mod("scene"), _mod("simulation")
    nx, ny, nz = case["shape"]
    world = case["world"]
    w = wl.patch_workload("fuzz", nx=nx, ny=ny, nz=nz)
    vox = sc.voxelize(w.scene, w.grid)
    fl = {"auto": 0, "direct": capi.FLAG_KERNEL_DIRECT, "wavefront": capi.FLAG_KERNEL_WAVEFRONT}
    total = sum(case["calls"])

    def make():
        return simm.Simulation(w.grid, vox, f0=w.f0, fc=w.fc, boundary=case["kinds"], cpml_cells=case["cells"], nr_ts=total + 8,
                               nf2ff_freqs=None if case["nf2ff"] == "none" else [w.f0], use_classes=case["classes"])
    saved = {k: os.environ.pop(k, None) for k in ENV_KNOBS}
    os.environ.update(case["env"])
    try:
        so = make()
        eo = so.build(oracle)
        sims = [make() for _ in range(world)]
        engs = [s.build(hip, rank=r, world=world, flags=fl[case["sched"][r]], partition=case["partition"]) for r, s in enumerate(sims)]
        blobs = [e.p2p_export() for e in engs]
        for r, e in enumerate(engs):
            e.p2p_attach(blobs[r - 1] if r > 0 else None, blobs[r + 1] if r + 1 < world else None)
        rng = np.random.default_rng(case["seed"])
        for kind in (0, 1):
            for c in range(3):
                g = (1e-3 * rng.standard_normal(eo.local_shape)).astype(np.float32)
                eo.set_field(kind, c, g)
                for e in engs:
                    e.set_field(kind, c, np.ascontiguousarray(g[e.k0:e.k0 + e.nk]))
        for n in case["calls"]:
            eo.run(n)
            capi.run_linked(engs, n)
    finally:
        for k in ENV_KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    problems = []
    fo, fh = eo.fields(), np.concatenate([e.fields() for e in engs], axis=2)
    if not np.isfinite(fo).all() or not np.abs(fo).max() > 0:
        problems.append("oracle fields not finite / all zero")
    if not np.array_equal(fh, fo):
        bad = np.argwhere(fh != fo)
        problems.append(f"fields differ at {len(bad)} of {fo.size} entries, first {tuple(bad[0])}: {fh[tuple(bad[0])]!r} vs {fo[tuple(bad[0])]!r}")
    uo = so.port_series()[0]
    for q, name in ((0, "port voltage"), (1, "port current")):
        a, b = sum(np.asarray(s.port_series()[0][q], float) for s in sims), np.asarray(uo[q], float)
        if a.shape != b.shape or np.linalg.norm(a - b) > 1e-12 * max(np.linalg.norm(b), 1e-300):
            problems.append(f"{name} series differs")
    if case["nf2ff"] != "none":
        for b, *parts in zip(so.nf2ff_boxes(), *[s.nf2ff_boxes() for s in sims]):
            if np.abs(sum(parts) - b).max() > 1e-6 * max(np.abs(b).max(), 1e-300):
                problems.append("NF2FF face spectra differ")
                break
    info = {"launches_per_timestep": "/".join(str(e.schedule_info()["launches_per_timestep"]) for e in engs),
            "lag_planes": "/".join(str(e.nk) for e in engs), "timesteps_per_launch_max": 1}
    return problems, info


# ---- scenes with Debye media and / or conducting sheets -----------------------------------------------------------------------------
MEDIA_F0, MEDIA_FC, MEDIA_H = 9e9, 5e9, 1e-3
MEDIA_BATCH = (36, 3)        # (cases, seed) of the batch in the -m gpu suite (tests/test_dispersion_gpu.py); test_media_fuzz_cpu.py guards its coverage
MEDIA_BANDS = {3: (5e9, 15e9), 4: (3e9, 20e9), 5: (2e9, 25e9), 8: (0.1e9, 30e9)}     # bands over which K poles hold tan delta within 2 %


def _pick_mod4(rng, lo, hi):
    """A value of lo ... hi (inclusive) whose residue mod 4 is drawn first, so that the residues come out uniform."""
    r = int(rng.integers(0, 4))
    c = [v for v in range(lo, hi + 1) if v % 4 == r] or list(range(lo, hi + 1))
    return int(c[int(rng.integers(0, len(c)))])


def draw_media_case(rng):
    """One scene with 0 ... 8 Debye media and 0 ... 3 conducting sheets (at least one of the two) as a plain dict.  All positions are node
    indices; a medium owns the cells [lo, hi) of its box.  What each item is there for: see the table in docs/HISTORY.md (randomised media)."""
    big = rng.random() < 0.12              # a box of >= 20 blocks of k_debye per component (>= 5 120 groups of four x-edges)
    if big:
        n = [int(rng.integers(62, 91)), int(rng.integers(46, 61)), int(rng.integers(30, 41))]
    else:
        n = [int(rng.choice([rng.integers(14, 40), rng.integers(40, 91)])), int(rng.choice([rng.integers(12, 30), rng.integers(30, 61)])),
             int(rng.integers(12, 41))]
    if rng.random() < 0.3:
        kinds = [str(rng.choice(["PEC", "MUR", "CPML"]))] * 6
    else:
        kinds = [str(rng.choice(["PEC", "MUR", "CPML"])) for _ in range(6)]
    cells = int(rng.integers(2, max(2, min(4 if big else 8, (min(n) - 8) // 2)) + 1))
    layer = [cells if k == "CPML" else 0 for k in kinds]
    L = [layer[2 * a] for a in range(3)]                       # cells [L, H) per axis lie outside the CPML layers
    H = [n[a] - 1 - layer[2 * a + 1] for a in range(3)]
    nmedia = int(rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 8], p=[0.14, 0.28, 0.14, 0.1, 0.05, 0.05, 0.05, 0.05, 0.14]))
    if big:
        nmedia = int(rng.integers(1, 3))
    # the region the media fill: now and then up to a face (never into a CPML layer), else a few cells inside
    touch = [bool(rng.random() < 0.35) and kinds[f] != "CPML" for f in range(6)] if rng.random() < 0.3 else [False] * 6
    rlo, rhi = [], []
    for a in range(3):
        span = H[a] - L[a]
        room = 3 if big else max(3, span // 4)
        lo_min = L[a] if kinds[2 * a] == "CPML" else 1
        hi_max = H[a] if kinds[2 * a + 1] == "CPML" else n[a] - 2
        lo = 0 if touch[2 * a] else _pick_mod4(rng, lo_min, lo_min + room) if a == 0 else int(rng.integers(lo_min, lo_min + room + 1))
        hi = n[a] - 1 if touch[2 * a + 1] else _pick_mod4(rng, hi_max - room, hi_max) if a == 0 else int(rng.integers(hi_max - room, hi_max + 1))
        if hi - lo < 2:
            lo, hi = min(lo, lo_min + 1), max(hi, hi_max - 1)
        rlo.append(int(lo)); rhi.append(int(hi))
    split = int(np.argmax([rhi[a] - rlo[a] for a in range(3)]))       # the media stand behind each other along this axis, a cell apart
    nmedia = min(nmedia, (rhi[split] - rlo[split] + 1) // 2)
    media = []
    if nmedia:
        lens = np.ones(nmedia, int)
        for _ in range(rhi[split] - rlo[split] - (2 * nmedia - 1)):
            lens[int(rng.integers(0, nmedia))] += 1
        pos = rlo[split]
        for q in range(nmedia):
            lo, hi = list(rlo), list(rhi)
            lo[split], hi[split] = pos, pos + int(lens[q])
            pos = hi[split] + 1
            for a in range(3):
                if a != split and q > 0 and rng.random() < 0.6:      # (medium 0 spans the region, so the bounding box is the region)
                    lo[a] = int(rng.integers(rlo[a], rhi[a]))
                    hi[a] = int(rng.integers(lo[a] + 1, rhi[a] + 1))
            K = int(rng.choice([1, 3, 4, 5, 8], p=[0.2, 0.3, 0.15, 0.1, 0.25]))
            kappa = float(rng.choice([0.0, 0.0, round(float(rng.uniform(0.005, 0.05)), 4)]))
            if K == 1:
                par = ("poles", round(float(rng.uniform(1.5, 4.0)), 3), kappa, [round(float(rng.uniform(0.2, 1.5)), 3)],
                       [round(float(rng.uniform(5.0, 40.0)), 2) * 1e-12])
            else:
                par = ("fit", round(float(rng.uniform(2.0, 6.0)), 3), round(float(rng.uniform(0.005, 0.05)), 4), K, kappa)
            hole = None
            if all(hi[a] - lo[a] >= 4 for a in range(3)) and rng.random() < 0.5:      # plain dielectric of higher priority inside: w = 0 groups
                h0 = [int(rng.integers(lo[a] + 1, hi[a] - 2)) for a in range(3)]
                hole = (h0, [int(min(hi[a] - 1, h0[a] + rng.integers(2, 6))) for a in range(3)], round(float(rng.uniform(1.5, 3.0)), 2))
            media.append({"medium": par, "lo": lo, "hi": hi, "hole": hole})
    nf = str(rng.choice(["none", "dft", "record"]))
    nsheets = int(rng.choice([0, 1, 2, 3], p=[0.45, 0.25, 0.2, 0.1])) if nmedia else int(rng.integers(1, 4))

    def sheet_range(with_nf):     # nodes a sheet may use: two planes inside every face, outside the CPML layers, strictly inside the NF2FF box
        lo = [max(2, L[a] + 1, (max(layer[2 * a] + 2, 3) + 1) if with_nf else 0) for a in range(3)]
        hi = [min(n[a] - 3, H[a] - 1, (n[a] - 1 - max(layer[2 * a + 1] + 2, 3) - 1) if with_nf else n[a]) for a in range(3)]
        return lo, hi

    slo, shi = sheet_range(nf != "none")
    if nsheets and any(shi[a] - slo[a] < 2 for a in range(3)):
        nf = "none"
        slo, shi = sheet_range(False)
    # one lumped port along z, half of the time inside a medium
    plo, phi_ = [max(2, L[a] + 1) for a in range(3)], [min(n[a] - 3, H[a] - 1) for a in range(3)]
    port = None
    if media and rng.random() < 0.6:
        m = media[int(rng.integers(0, len(media)))]
        lo = [max(plo[0], m["lo"][0] + 1), max(plo[1], m["lo"][1] + 1), max(plo[2], m["lo"][2])]
        hi = [min(phi_[0], m["hi"][0] - 1), min(phi_[1], m["hi"][1] - 1), min(phi_[2], m["hi"][2])]
        if lo[0] <= hi[0] and lo[1] <= hi[1] and lo[2] < hi[2]:
            z0 = int(rng.integers(lo[2], hi[2]))
            port = (int(rng.integers(lo[0], hi[0] + 1)), int(rng.integers(lo[1], hi[1] + 1)), z0, int(min(hi[2], z0 + rng.integers(1, 5))))
    if port is None:
        z0 = int(rng.integers(plo[2], phi_[2]))
        port = (int(rng.integers(plo[0], phi_[0] + 1)), int(rng.integers(plo[1], phi_[1] + 1)), z0, int(min(phi_[2], z0 + rng.integers(1, 5))))
    sheets = []
    for q in range(nsheets):
        for _ in range(8):
            a = int(rng.integers(0, 3))
            lo = [int(rng.integers(slo[b], shi[b] - 1)) for b in range(3)]
            hi = [int(rng.integers(lo[b] + 2, shi[b] + 1)) for b in range(3)]
            resolved = bool(rng.random() < 0.35)
            if q == 0 and media and rng.random() < 0.6:      # on a medium's face: its edges are dispersive edges too
                m = media[int(rng.integers(0, len(media)))]
                side = m["hi"][a] if rng.random() < 0.5 else m["lo"][a]
                if slo[a] <= side <= shi[a]:
                    lo[a], resolved = int(side), False
                    for b in range(3):
                        if b != a and max(slo[b], m["lo"][b]) + 2 <= min(shi[b], m["hi"][b]):
                            lo[b], hi[b] = max(slo[b], m["lo"][b]), min(shi[b], m["hi"][b])
            hi[a] = min(lo[a] + 2, shi[a]) if resolved else lo[a]
            # (the scene refuses a sheet edge that is a port edge or lies on the port's voltage line: z-edges at the port's x, y)
            zhit = min(hi[2], port[3]) - max(lo[2], port[2]) >= 1
            if lo[0] <= port[0] <= hi[0] and lo[1] <= port[1] <= hi[1] and zhit:
                continue
            sigma = float(rng.choice([5.8e7, 9.1e6, 3e5, 1e5]))
            sheets.append((sigma, 2e-3 if resolved else float(rng.choice([5e-6, 35e-6, 1e-3])), lo, hi))
            break
    if not media and not sheets:      # (eight placements in a row hit the port: a medium instead)
        media.append({"medium": ("fit", 4.3, 0.02, 3, 0.0), "lo": list(rlo), "hi": list(rhi), "hole": None})
    env = {}
    if "MUR" in kinds and rng.random() < 0.4:
        env["FDTD_MUR_APPLY_PASS"] = "1"
    if rng.random() < 0.25:
        env["FDTD_TYS"] = str(int(rng.choice([1, 2, 3, 5, 7, 16])))
    calls = [int(rng.integers(1, 61)) for _ in range(int(rng.integers(1, 6)))]
    if big:
        calls = calls[:3]
    return {"shape": tuple(n), "graded": int(rng.integers(1, 1 << 20)) if rng.random() < 0.6 else 0, "kinds": kinds, "cells": cells,
            "classes": bool(rng.random() < 0.7), "media": media, "sheets": sheets, "port": port, "nf2ff": nf,
            "sched": str(rng.choice(["auto", "direct"])), "env": env, "calls": calls, "seed": int(rng.integers(1, 1 << 30))}


def media_case_medium(par):
    d = _mod("dispersion")
    if par[0] == "poles":
        return d.DebyeMedium(par[1], par[2], par[3], par[4])
    _, eps_r, tan_delta, K, kappa = par
    m = d.fit_constant_loss_tangent(eps_r, tan_delta, MEDIA_F0, *MEDIA_BANDS[K], K=K)
    return m if kappa == 0 else d.DebyeMedium(m.eps_inf, kappa, m.delta_eps, m.tau)


def media_case_sim(case):
    """The Simulation of a drawn case (ValueError: a set-up the host layer refuses)."""
    sc, simm, gr = _mod("scene"), _mod("simulation"), _mod("grid")
    n = case["shape"]
    if case["graded"]:
        g = np.random.default_rng(case["graded"])
        lines = [np.concatenate([[0.0], np.cumsum(MEDIA_H * g.uniform(0.7, 1.4, k - 1))]) for k in n]
    else:
        lines = [np.arange(k) * MEDIA_H for k in n]
    grid = gr.RectGrid(*lines)
    at = lambda p: [float(lines[a][p[a]]) * 1e3 for a in range(3)]
    s = sc.Scene(unit=1e-3)
    for q, m in enumerate(case["media"]):
        med = media_case_medium(m["medium"])
        s.add_debye_material(f"m{q}", med.eps_inf, med.kappa, med.delta_eps, med.tau).add_box(at(m["lo"]), at(m["hi"]), priority=1)
        if m["hole"] is not None:
            s.add_material(f"hole{q}", eps_r=m["hole"][2]).add_box(at(m["hole"][0]), at(m["hole"][1]), priority=2)
    for q, (sigma, t, lo, hi) in enumerate(case["sheets"]):
        s.add_conducting_sheet(f"s{q}", sigma, t).add_box(at(lo), at(hi))
    px, py, z0, z1 = case["port"]
    s.add_lumped_port(1, 50.0, at((px, py, z0)), at((px, py, z1)), "z", 1.0)
    vox = sc.voxelize(s, grid)
    total = sum(case["calls"])
    return simm.Simulation(grid, vox, f0=MEDIA_F0, fc=MEDIA_FC, boundary=case["kinds"], cpml_cells=case["cells"], nr_ts=total + 8,
                           end_criteria=0.0, nf2ff_freqs=None if case["nf2ff"] == "none" else [MEDIA_F0, 1.3 * MEDIA_F0],
                           use_classes=case["classes"], nf2ff_mode="dft" if case["nf2ff"] == "none" else case["nf2ff"])


def _restatement():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    mod = importlib.import_module("restatement")
    assert {"planewave" if name in ("pw_e", "pw_h") else name for name in mod.ORDER} == set(CORRECTION_NAMES)
    return mod


def media_reference_problems(r):
    """What the reference side must show by itself, so that a medium or a sheet the wave never reached cannot pass silently: finite and
    non-zero fields and states, every branch state of every dispersive edge the operator does not hold (w != 0, vi != 0) and the
    branch currents of every sheet edge off zero — at one of the Restatement's checkpoints (the first step, every eighth, the end of a
    run(): a single state update cancels to exactly 0.0f about once in 2^24, which a few of 1e8 final values do)."""
    r.note_moved()
    problems = []
    fo = r.e.fields()
    if not np.isfinite(fo).all() or not np.abs(fo).max() > 0:
        problems.append("reference fields not finite / all zero")
    d = r.debye
    for c in range(3 if d else 0):
        if not d.w[c].size:
            continue
        if not (np.isfinite(d.u[c]).all() and np.isfinite(d.vprev[c]).all()):
            problems.append(f"reference states of component {c} not finite")
        live = (d.w[c] != 0) & (d.vi[c] != 0)
        need = live[None] & (d.tab[c][1] != 0)           # (oma == 0: the padding poles of a shorter medium, which stay at rest)
        if not live.any() or not np.all(d.u_moved[c][need]) or not np.all(d.vprev_moved[c][live]):
            problems.append(f"component {c}: {np.count_nonzero(~d.u_moved[c][need])} branch states of {np.count_nonzero(need)} on dispersive edges never left zero")
        if np.any(d.u[c][:, ~live] != 0) or np.any(d.vprev[c][~live] != 0):
            problems.append(f"component {c}: states of edges that are not dispersive edges moved")
    if r.sheets is not None and not (np.isfinite(r.sheets.ib).all() and np.all(r.sheets.ib_moved.any(axis=0))):
        problems.append("reference: a sheet edge without branch current")
    return problems


def run_media_case(case, hip, oracle):
    """hip = None: the reference side alone (what tests/test_media_fuzz_cpu.py steps without a GPU)."""
    capi = _mod("_capi")
    flags = {"auto": 0, "direct": capi.FLAG_KERNEL_DIRECT}[case["sched"]]
    saved = {k: os.environ.pop(k, None) for k in ENV_KNOBS}
    os.environ.update(case["env"])
    try:
        so = media_case_sim(case)
        ref = _restatement().Restatement(so, oracle, seed=case["seed"])
        sh = eh = None
        if hip is not None:
            sh = media_case_sim(case)
            eh = sh.build(hip, flags=flags)
            rng = np.random.default_rng(case["seed"])
            for kind in (0, 1):
                for c in range(3):
                    eh.set_field(kind, c, (1e-3 * rng.standard_normal(eh.local_shape)).astype(np.float32))
        for nsteps in case["calls"]:
            ref.run(nsteps)
            if eh is not None:
                eh.run(nsteps)
    finally:
        for k in ENV_KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    problems = media_reference_problems(ref)
    if eh is None:
        return problems, {"launches_per_timestep": 0, "lag_planes": 0, "timesteps_per_launch_max": 0}
    fh, fo = eh.fields(), ref.e.fields()
    if not np.array_equal(fh, fo):
        bad = np.argwhere(fh != fo)
        problems.append(f"fields differ at {len(bad)} of {fo.size} entries, first {tuple(bad[0])}: {fh[tuple(bad[0])]!r} vs {fo[tuple(bad[0])]!r}")
    else:
        nzm = fo != 0
        if not np.array_equal(fh[nzm].view(np.uint32), fo[nzm].view(np.uint32)):
            problems.append("fields equal as values but not as bits where the reference is non-zero")
    for c in range(3 if ref.debye else 0):
        hv, hu, hvi = eh.debye_state(c)
        for name, a, b in (("v_prev", hv, ref.debye.vprev[c]), ("u", hu, ref.debye.u[c]), ("vi", hvi, ref.debye.vi[c])):
            if not np.array_equal(a, b):
                bad = np.argwhere(a != b)
                problems.append(f"Debye {name} of component {c} differs at {len(bad)} of {b.size} entries, first {tuple(bad[0])}: "
                                f"{a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}")
    if ref.sheets is not None:
        hv, hib = eh.sheet_state()
        if not np.array_equal(hv, ref.sheets.vprev) or not np.array_equal(hib, ref.sheets.ib):
            problems.append(f"sheet states differ ({np.count_nonzero(hv != ref.sheets.vprev)} v_prev, {np.count_nonzero(hib != ref.sheets.ib)} branch currents)")
    uh, uo = sh.port_series()[0], so.port_series()[0]
    for q, name in ((0, "port voltage"), (1, "port current")):
        a, b = np.asarray(uh[q], float), np.asarray(uo[q], float)
        if a.shape != b.shape or not np.abs(b).max() > 0 or np.linalg.norm(a - b) > 1e-12 * np.linalg.norm(b):
            problems.append(f"{name} series differs")
    ea, eb = np.array(eh.energy()), np.array(ref.e.energy())
    if np.abs(ea - eb).max() > 1e-12 * np.abs(eb).max():
        problems.append(f"energy {ea!r} vs {eb!r}")
    if case["nf2ff"] != "none":
        bh, bo = sh.nf2ff_boxes(), so.nf2ff_boxes()
        worst = max(float(np.abs(np.asarray(a) - np.asarray(b)).max()) / max(float(np.abs(b).max()), 1e-300) for a, b in zip(bh, bo))
        if len(bh) != len(bo) or not worst <= 1e-6:
            problems.append(f"NF2FF face spectra differ ({worst:.2e} of the largest entry)")
    info = eh.schedule_info()
    if info["resident"] or info["launches_per_timestep"] not in (2, 3):
        problems.append(f"schedule {info}: media and sheets step under two or three launches per timestep")
    return problems, info


# ---- all eight corrections in one context ---------------------------------------------------------------------------------------------
CORRECTIONS_BATCH = (24, 2)   # (cases, seed) of the batch in the -m gpu suite (tests/test_corrections_fuzz_gpu.py); test_corrections_fuzz_cpu.py guards its coverage
DRAWN_NAMES = ("debye", "lorentz", "sheets", "elements", "magnetic", "conformal", "planewave")      # (the order the cases are drawn in)
CORRECTION_NAMES = DRAWN_NAMES + ("excite",)      # H-field excitations: drawn last, from a generator of their own (draw_excitations)
TWO_PI = 2 * np.pi


def _line_edges(lo, hi):
    """The edges (comp, i, j, k) with both end nodes in the node box lo..hi (a line: an element or a port; a plane: a sheet)."""
    out = set()
    for c in range(3):
        if hi[c] > lo[c]:
            r = [range(lo[a], hi[a] + (0 if a == c else 1)) for a in range(3)]
            out |= {(c, i, j, k) for i in r[0] for j in r[1] for k in r[2]}
    return out


def _lorentz_poles(rng, K):
    """K poles (wp, w0, gamma) in rad/s, Drude (w0 = 0) and Lorentz ones, loss-free and lossy, rounded so that repr() holds them."""
    wp = [round(float(rng.uniform(2.0, 8.0)), 2) * 1e9 * TWO_PI for _ in range(K)]
    w0 = [0.0 if rng.random() < 0.4 else round(float(rng.uniform(6.0, 20.0)), 2) * 1e9 * TWO_PI for _ in range(K)]
    gamma = [0.0 if rng.random() < 0.3 else round(float(rng.uniform(0.5, 20.0)), 2) * 1e9 for _ in range(K)]
    return wp, w0, gamma


def draw_excitations(case, g):
    """H-field excitations for a drawn case, from the generator `g` alone: one to three hard faces, five to nine soft faces of which the
    first is listed twice (two soft entries on one face), all three components, delays of 0 timesteps, inside the run and past its end
    (such an entry never reads the table: a hard face is then held at zero throughout).  Each is a point box on a face that exists, is
    no grid face, lies in no CPML layer and is no magnetic, conformal or plane-wave face — what field_excitation.check_placement demands,
    asked of the scene without excitations — and that no NF2FF box samples: the reference's NF2FF sums are the oracle's own, taken
    inside its H half-step in front of every H-side correction (boxes and recorder faces ACROSS excited faces: the observer tests of
    test_excite_gpu.py, whose reference samples behind them).  None where that scene is refused or has no such faces."""
    try:
        sim = corrections_case_sim(dict(case, excite=None))
    except ValueError:
        return None
    nx, ny, nz = n = case["shape"]
    ok = np.ones((3, nz, ny, nx), bool)
    cells = sim.bc.face_cells()
    for c in range(3):
        for a in range(3):      # along a: nodes lo <= p < hi (a == c: off the grid faces; else a cell along a; both: outside the layers)
            lo, hi = max(cells[2 * a], 1 if a == c else 0), n[a] - 1 - cells[2 * a + 1]
            p = np.arange(n[a])
            ok[c] &= ((p >= lo) & (p < hi)).reshape([-1 if 2 - a == d else 1 for d in range(3)])
    if sim.magnetic is not None:
        ok &= sim.magnetic.full_classes((nz, ny, nx)) == 0
    flat = ok.reshape(3, -1)
    if sim.conformal is not None:
        flat[np.asarray(sim.conformal.comp, np.int64), np.asarray(sim.conformal.idx, np.int64)] = False
    if sim.plane_wave is not None:
        pwm = _mod("planewave")
        for f, i, j, k, *_ in pwm.terms(sim.grid, sim.plane_wave, 1):
            ok[f, k, j, i] = False
    for r in ([] if sim.nf2ff_box is None else sim.nf2ff_box.requests):
        if r.kind == 1:
            ok[r.comp, r.lo[2]:r.hi[2] + 1, r.lo[1]:r.hi[1] + 1, r.lo[0]:r.hi[0] + 1] = False
    nh, ns = int(g.integers(1, 4)), int(g.integers(5, 10))
    total = sum(case["calls"])
    kinds = {"0": 0, "inside": int(g.integers(1, max(2, total // 2))), "past": total + 8 + int(g.integers(0, 5))}
    out = []
    for q in range(nh + ns):
        c = q % 3 if q >= nh else int(g.integers(0, 3))
        cand = np.argwhere(ok[c])
        if not len(cand):
            return None
        k, j, i = (int(v) for v in cand[int(g.integers(0, len(cand)))])
        ok[c, k, j, i] = False
        how = ("0", "inside", "past")[(q - nh) % 3] if q >= nh else str(g.choice(["0", "inside", "past"]))
        amp = round(float(g.uniform(0.2, 1.0)) * float(g.choice([-1.0, 1.0])), 3)
        out.append({"type": 3 if q < nh else 2, "comp": c, "node": [i, j, k], "val": amp, "delay_steps": kinds[how], "delay": kinds[how] * float(sim.dt)})
    first = out[nh]                  # the repeated face: its second entry 1e-7 of the first, so that the list order shows in float32
    out.append(dict(first, val=round(-1e-7 * first["val"], 10)))
    out.append(dict(first, val=-first["val"]))
    return out


def draw_corrections_case(rng, excite=None):
    """One scene with at least three of the corrections of the step loop (often all of them) as a plain dict: Debye media, Lorentz
    / Drude media, conducting sheets, lumped elements, magnetic materials, a curved metal with conformal faces, a plane wave — drawn from
    `rng` — and H-field excitations: `excite` = (seed, case number) draws them (draw_excitations) from a generator of its own seeded
    with that pair, into every case that holds the seven others and every second of the rest; `rng` is not touched by it, so every other
    quantity of every case is what it is without.  All
    positions are node indices; a box owns the cells [lo, hi).  The media stand behind each other along y or z (the longer of the two
    inside the layers), the curved metal beside them along x, the plane wave's box one cell outside everything and the NF2FF box outside
    that.  What each item is there for: the table in docs/HISTORY.md (randomised corrections)."""
    touchy = False
    if rng.random() < 0.3:
        want = dict.fromkeys(DRAWN_NAMES, True)
    else:
        touchy = bool(rng.random() < 0.4)      # media up to the grid faces along x: no plane wave, no NF2FF box, no CPML there
        while True:
            want = {k: bool(rng.random() < 0.55) for k in DRAWN_NAMES}
            if touchy:
                want["planewave"] = False
            if sum(want.values()) >= 3:
                break
    roomy = want["planewave"] or want["conformal"] or sum(want.values()) >= 6
    n = [int(rng.integers(30, 71)), int(rng.integers(24, 37)), int(rng.integers(20, 29))] if roomy else \
        [int(rng.integers(14, 71)), int(rng.integers(12, 37)), int(rng.integers(12, 29))]
    if rng.random() < 0.3:
        kinds = [str(rng.choice(["PEC", "MUR", "CPML"]))] * 6
    else:
        kinds = [str(rng.choice(["PEC", "MUR", "CPML"])) for _ in range(6)]
    if touchy:
        kinds[0], kinds[1] = str(rng.choice(["PEC", "MUR", "MUR"])), str(rng.choice(["PEC", "MUR", "MUR"]))
    cells = int(rng.integers(2, max(2, min(3 if roomy else 6, (min(n) - 8) // 2)) + 1))
    layer = [cells if k == "CPML" else 0 for k in kinds]
    nf = "none" if touchy else str(rng.choice(["none", "dft", "record"]))
    pw = want["planewave"]

    def margins(nf, pw):      # nodes between a grid face and the region the scene may fill
        out = []
        for f in range(6):
            o, nfp = max(2, layer[f] + 1), max(layer[f] + 2, 3)
            if nf != "none":
                o = max(o, nfp + 1)                     # strictly inside the NF2FF box
            if pw:
                o = max(o, max(layer[f] + 2, nfp + 2 if nf != "none" else 0) + 1)      # a vacuum cell inside the plane wave's box
            out.append(o)
        return out

    need = [12 if want["conformal"] else 6, 5, 5]
    fits = lambda m: all(n[a] - 1 - m[2 * a] - m[2 * a + 1] >= need[a] for a in range(3))
    if not fits(margins(nf, pw)) and fits(margins("none", pw)):
        nf = "none"
    if not fits(margins(nf, pw)):
        pw, need[0] = False, 6
        want["planewave"] = want["conformal"] = False
        if not fits(margins(nf, pw)):
            nf = "none"
    m = margins(nf, pw)
    R0, R1 = [m[2 * a] for a in range(3)], [n[a] - 1 - m[2 * a + 1] for a in range(3)]        # the region, in nodes
    while any(R1[a] - R0[a] < 4 for a in range(3)):      # (a 12-plane grid under six cells of CPML)
        cells -= 1
        layer = [cells if k == "CPML" else 0 for k in kinds]
        m = margins(nf, pw)
        R0, R1 = [m[2 * a] for a in range(3)], [n[a] - 1 - m[2 * a + 1] for a in range(3)]
    # the curved metal: a box of 4 ... 6 cells at one end of the region along x, the media a cell away from it or touching its plane
    metal = None
    M0, M1 = list(R0), list(R1)                          # the media's share of the region
    if want["conformal"] and R1[0] - R0[0] >= 11:
        bw, side, gap = int(rng.integers(4, 7)), int(rng.integers(0, 2)), int(rng.integers(0, 2))
        metal = {"shape": str(rng.choice(["sphere", "sphere", "cylinder"])), "side": side, "gap": gap, "bw": bw}
        if side == 0:
            M0[0] = R0[0] + bw + gap
        else:
            M1[0] = R1[0] - bw - gap
    want["conformal"] = metal is not None
    # media up to a grid face along x (never into a CPML layer, never with a plane wave or an NF2FF box around)
    T0, T1 = list(M0), list(M1)
    if touchy:
        if not (metal and metal["side"] == 0) and rng.random() < 0.7:
            T0[0] = 0
        if not (metal and metal["side"] == 1) and rng.random() < 0.7:
            T1[0] = n[0] - 1
    s = 1 if M1[1] - M0[1] >= M1[2] - M0[2] else 2       # the media stand behind each other along this axis
    t = 3 - s
    nD = int(rng.integers(1, 4)) if want["debye"] else 0
    nL = int(rng.integers(1, 3)) if want["lorentz"] else 0
    nM = int(rng.integers(1, 3)) if want["magnetic"] else 0
    span = M1[s] - M0[s]

    def segments():
        seg = []
        for kind, cnt in (("D", nD), ("L", nL), ("M", nM)):
            for q in range(cnt):
                if kind == "M":      # on the face plane of the dispersive medium in front of it, or a cell away
                    gap_ = 0 if (seg and (seg[-1][0] == "M" or rng.random() < 0.6)) else (1 if seg else 0)
                else:                # two dispersive media never share an edge
                    gap_ = 1 if seg else 0
                seg.append([kind, gap_, 1])
        return seg
    seg = segments()
    while sum(g_ + l_ for _, g_, l_ in seg) > span:
        if nD > 1:
            nD -= 1
        elif nL > 1:
            nL -= 1
        elif nM > 1:
            nM -= 1
        elif nD:
            nD = 0
        else:
            nL = 0
        seg = segments()
    for _ in range(int(rng.integers(0, span - sum(g_ + l_ for _, g_, l_ in seg) + 1)) if seg else 0):
        seg[int(rng.integers(0, len(seg)))][2] += 1
    if rng.random() < 0.5:
        seg = seg[::-1]
        for q in range(len(seg) - 1, 0, -1):
            seg[q][1] = seg[q - 1][1]
        if seg:
            seg[0][1] = 0
    room = max(3, (M1[0] - M0[0]) // 4)
    boxes = []
    pos = M0[s] + (int(rng.integers(0, span - sum(g_ + l_ for _, g_, l_ in seg) + 1)) if seg else 0)
    for q, (kind, gap_, len_) in enumerate(seg):
        pos += gap_
        lo, hi = list(T0), list(T1)
        lo[s], hi[s] = pos, pos + len_
        pos += len_
        first = not any(b["kind"] == kind for b in boxes)
        if kind != "D":       # x0 and x1 with uniform residues mod 4
            if not (T0[0] == 0 and rng.random() < 0.6):
                lo[0] = _pick_mod4(rng, M0[0], M0[0] + room)
            if not (T1[0] == n[0] - 1 and rng.random() < 0.6):
                hi[0] = _pick_mod4(rng, M1[0] - room, M1[0])
            if hi[0] - lo[0] < 2:
                lo[0], hi[0] = M0[0], M1[0]
        if kind == "M" and metal is not None and metal["gap"] == 0:      # magnetic cells stay a cell clear of the curved metal
            if metal["side"] == 0:
                lo[0] = max(lo[0], M0[0] + 1)
            else:
                hi[0] = min(hi[0], M1[0] - 1)
        if not first and rng.random() < 0.5:
            lo[t] = int(rng.integers(M0[t], M1[t] - 1))
            hi[t] = int(rng.integers(lo[t] + 2, M1[t] + 1))
        boxes.append({"kind": kind, "lo": [int(v) for v in lo], "hi": [int(v) for v in hi]})
    debye, lorentz, magnetic = [], [], []
    kmax = int(rng.choice([1, 2, 3, 4]))                 # the poles of the Lorentz media: every k_lorentz<multi, 1 / 2 / 4>
    for b in boxes:
        if b["kind"] == "D":
            K = int(rng.choice([1, 3, 4, 5, 8], p=[0.2, 0.3, 0.15, 0.1, 0.25]))
            kappa = float(rng.choice([0.0, 0.0, round(float(rng.uniform(0.005, 0.05)), 4)]))
            if K == 1:
                par = ("poles", round(float(rng.uniform(1.5, 4.0)), 3), kappa, [round(float(rng.uniform(0.2, 1.5)), 3)],
                       [round(float(rng.uniform(5.0, 40.0)), 2) * 1e-12])
            else:
                par = ("fit", round(float(rng.uniform(2.0, 6.0)), 3), round(float(rng.uniform(0.005, 0.05)), 4), K, kappa)
            debye.append({"medium": par, "lo": b["lo"], "hi": b["hi"]})
        elif b["kind"] == "L":
            K = kmax if not lorentz else int(rng.integers(1, kmax + 1))
            lorentz.append({"medium": (round(float(rng.uniform(1.0, 2.5)), 3), float(rng.choice([0.0, 0.0, 0.01])), *_lorentz_poles(rng, K)),
                            "lo": b["lo"], "hi": b["hi"]})
        else:
            how = str(rng.choice(["mu", "sigma", "both"]))
            magnetic.append({"eps_r": round(float(rng.uniform(1.0, 2.0)), 2), "mu_r": round(float(rng.uniform(1.5, 4.0)), 2) if how != "sigma" else 1.0,
                             "sigma_m": round(float(rng.uniform(50.0, 2000.0)), 1) if how != "mu" else 0.0, "lo": b["lo"], "hi": b["hi"]})
    # what sheets, elements and the port may use: the media's share of the region without the planes on grid faces, a node off the
    # curved metal's plane
    S0, S1 = list(M0), list(M1)
    if metal is not None and metal["gap"] == 0:
        S0[0] += metal["side"] == 0
        S1[0] -= metal["side"] == 1
    clip = lambda b: ([max(b["lo"][a], S0[a]) for a in range(3)], [min(b["hi"][a], S1[a]) for a in range(3)])
    # one lumped port along z: inside a medium (a magnetic one: its current loop runs through magnetic faces) or in the open
    port = None
    if boxes and rng.random() < 0.75:
        lo, hi = clip(boxes[int(rng.integers(0, len(boxes)))])
        inner = [(lo[a] + 1, hi[a] - 1) if hi[a] - lo[a] >= 2 else (lo[a], hi[a]) for a in range(2)]
        if hi[2] > lo[2]:
            z0 = int(rng.integers(lo[2], hi[2]))
            port = (int(rng.integers(inner[0][0], inner[0][1] + 1)), int(rng.integers(inner[1][0], inner[1][1] + 1)), z0,
                    int(min(hi[2], z0 + rng.integers(1, 5))))
    if port is None:
        z0 = int(rng.integers(S0[2], S1[2]))
        port = (int(rng.integers(S0[0] + 1, S1[0])), int(rng.integers(S0[1], S1[1] + 1)), z0, int(min(S1[2], z0 + rng.integers(1, 5))))
    taken = _line_edges([port[0], port[1], port[2]], [port[0], port[1], port[3]])
    # conducting sheets of zero thickness: on a face of a dispersive medium (its edges are dispersive edges too), else anywhere
    sheets = []
    disp = [b for b in boxes if b["kind"] != "M"]
    for q in range(int(rng.integers(1, 4)) if want["sheets"] else 0):
        for _ in range(8):
            if disp and (q == 0 or rng.random() < 0.7):
                b = disp[(q + int(rng.integers(0, 2))) % len(disp)]
                lo, hi = clip(b)
                a = s if rng.random() < 0.7 else int(rng.integers(0, 3))
                lo[a] = hi[a] = lo[a] if rng.random() < 0.5 else hi[a]
            else:
                a = int(rng.integers(0, 3))
                lo, hi = list(S0), list(S1)
                lo[a] = hi[a] = int(rng.integers(S0[a], S1[a] + 1))
            for c in range(3):
                if c != a and hi[c] - lo[c] > 2 and rng.random() < 0.7:
                    lo[c] = int(rng.integers(lo[c], hi[c] - 1))
                    hi[c] = int(rng.integers(lo[c] + 2, min(hi[c], lo[c] + 9) + 1))
            if any(hi[c] <= lo[c] for c in range(3) if c != a):
                continue
            edges = _line_edges(lo, hi)
            if edges & taken:      # (the scene refuses a sheet edge that is a port edge, an element edge or another metal's)
                continue
            taken |= edges
            sheets.append((float(rng.choice([5.8e7, 9.1e6, 3e5, 1e5])), float(rng.choice([5e-6, 35e-6, 1e-3])), [int(v) for v in lo], [int(v) for v in hi]))
            break
    # lumped elements: lines of one to five edges inside a medium of each kind, or next to the curved metal
    elements = []
    for q in range(int(rng.integers(1, 5)) if want["elements"] else 0):
        for _ in range(8):
            d = int(rng.integers(0, 3))
            if metal is not None and metal["gap"] == 1 and rng.random() < 0.3:      # a tangential edge on the plane between metal and media
                d = int(rng.integers(1, 3))
                lo = [M0[0] - 1 if metal["side"] == 0 else M1[0] + 1, int(rng.integers(S0[1], S1[1])), int(rng.integers(S0[2], S1[2]))]
                length = 1
            elif boxes:
                blo, bhi = clip(boxes[(q + int(rng.integers(0, 2))) % len(boxes)])
                if bhi[d] <= blo[d]:
                    continue
                length = int(rng.integers(1, min(5, bhi[d] - blo[d]) + 1))
                lo = [int(rng.integers(blo[a], bhi[a] - length + 1)) if a == d else
                      int(rng.integers(blo[a] + 1, bhi[a])) if bhi[a] - blo[a] >= 2 else int(rng.integers(blo[a], bhi[a] + 1)) for a in range(3)]
            else:
                length = int(rng.integers(1, min(5, S1[d] - S0[d]) + 1))
                lo = [int(rng.integers(S0[a], S1[a] - (length if a == d else 0) + 1)) for a in range(3)]
            hi = list(lo)
            hi[d] += length
            edges = _line_edges(lo, hi)
            if edges & taken:
                continue
            taken |= edges
            kind = str(rng.choice(["parallel", "series"]))
            R = float(rng.choice([1.0, 50.0, 100.0, 1000.0]))
            L = float(rng.choice([1e-9, 3e-9]))
            C = float(rng.choice([0.2e-12, 1e-12]))
            if kind == "parallel":      # the inductor carries the state; R and C fold into the operator
                parts = [(None, L, None), (R, L, None), (None, L, C), (R, L, C)][int(rng.integers(0, 4))]
            else:
                parts = [(R, L, None), (None, L, C), (R, L, C), (R, None, C), (None, L, None)][int(rng.integers(0, 5))]
            elements.append({"dir": d, "kind": kind, "R": parts[0], "L": parts[1], "C": parts[2], "lo": [int(v) for v in lo], "hi": [int(v) for v in hi]})
            break
    if metal is not None:      # the metal's box: bw cells along x at its end of the region, beside a dispersive medium where there is one
        lo, hi = [0, 0, 0], [0, 0, 0]
        lo[0], hi[0] = (R0[0], R0[0] + metal["bw"]) if metal["side"] == 0 else (R1[0] - metal["bw"], R1[0])
        ref_box = disp[0] if disp else boxes[0] if boxes else None
        for a in (1, 2):
            w_ = int(min(metal["bw"], R1[a] - R0[a]))
            mid = (ref_box["lo"][a] + ref_box["hi"][a]) // 2 if ref_box else (R0[a] + R1[a]) // 2
            lo[a] = int(min(max(mid - w_ // 2 + int(rng.integers(-1, 2)), R0[a]), R1[a] - w_))
            hi[a] = lo[a] + w_
        metal = {"shape": metal["shape"], "side": metal["side"], "gap": metal["gap"], "lo": lo, "hi": hi,
                 "shift": [round(float(rng.uniform(-0.3, 0.3)), 2) for _ in range(3)], "tilt": [round(float(rng.uniform(10, 40)), 1), round(float(rng.uniform(10, 40)), 1)]}
    wave = None
    if pw:
        if rng.random() < 0.4:
            k = [0.0, 0.0, 0.0]
            k[int(rng.integers(0, 3))] = float(rng.choice([-1.0, 1.0]))
        else:
            k = [round(float(v), 2) for v in rng.uniform(-1, 1, 3)]
            if max(abs(v) for v in k) < 0.2:
                k[2] = 1.0
        e0 = [round(float(v), 2) for v in np.cross(k, rng.uniform(-1, 1, 3) + [0.1, 0.2, 0.3])]
        if max(abs(v) for v in e0) < 0.05:
            e0 = [round(float(v), 2) for v in np.cross(k, [1.0, 0.0, 0.0] if abs(k[0]) < 0.9 else [0.0, 1.0, 0.0])]
        wave = {"e0": e0, "dir": k, "lo": [R0[a] - 1 for a in range(3)], "hi": [R1[a] + 1 for a in range(3)]}
    env = {}
    if "MUR" in kinds and rng.random() < 0.4:
        env["FDTD_MUR_APPLY_PASS"] = "1"
    if rng.random() < 0.25:
        env["FDTD_TYS"] = str(int(rng.choice([1, 2, 3, 5, 7, 16])))
    calls = [int(rng.integers(1, 61)) for _ in range(int(rng.integers(1, 6)))]
    while sum(calls) > 150:
        q = int(np.argmax(calls))
        calls[q] = max(1, calls[q] - (sum(calls) - 150))
    if wave is not None and sum(calls) < 40:      # (the pulse's first timesteps lie below float32 rounding of the seeded fields)
        calls[-1] += 40 - sum(calls)
    sets = [(int(rng.integers(0, 2)), int(rng.integers(0, 3)), int(rng.integers(1, 1 << 30))) if rng.random() < 0.4 else None for _ in calls[1:]]
    case = {"shape": tuple(n), "graded": int(rng.integers(1, 1 << 20)) if rng.random() < 0.6 else 0, "kinds": kinds, "cells": cells,
            "classes": bool(rng.random() < 0.7), "debye": debye, "lorentz": lorentz, "sheets": sheets, "elements": elements, "magnetic": magnetic,
            "metal": metal, "planewave": wave, "port": port, "nf2ff": nf, "drive": str(rng.choice(["auto", "direct", "half"])), "env": env,
            "calls": calls, "sets": sets, "seed": int(rng.integers(1, 1 << 30)), "excite": None}
    if excite is not None:
        g = np.random.default_rng([int(excite[0]), int(excite[1])])
        everything = bool(debye and lorentz and sheets and elements and magnetic and metal is not None and wave is not None)
        if everything or g.random() < 0.5:
            case["excite"] = draw_excitations(case, g)
    return case


def corrections_batch(ncases=None, seed=None):
    """The drawn cases of a batch (default: CORRECTIONS_BATCH), excitations included."""
    ncases, seed = CORRECTIONS_BATCH if ncases is None else (ncases, seed)
    rng = np.random.default_rng(seed)
    return [draw_corrections_case(rng, excite=(seed, q)) for q in range(ncases)]


def corrections_case_sim(case):
    """The Simulation of a drawn case (ValueError: a set-up the host layer refuses)."""
    sc, simm, gr, lor = _mod("scene"), _mod("simulation"), _mod("grid"), _mod("lorentz")
    n = case["shape"]
    if case["graded"]:
        g = np.random.default_rng(case["graded"])
        lines = [np.concatenate([[0.0], np.cumsum(MEDIA_H * g.uniform(0.7, 1.4, k - 1))]) for k in n]
    else:
        lines = [np.arange(k) * MEDIA_H for k in n]
    grid = gr.RectGrid(*lines)
    at = lambda p: [float(lines[a][p[a]]) * 1e3 for a in range(3)]
    s = sc.Scene(unit=1e-3)
    for q, m in enumerate(case["debye"]):
        med = media_case_medium(m["medium"])
        s.add_debye_material(f"d{q}", med.eps_inf, med.kappa, med.delta_eps, med.tau).add_box(at(m["lo"]), at(m["hi"]), priority=1)
    for q, m in enumerate(case["lorentz"]):
        eps_inf, kappa, wp, w0, gamma = m["medium"]
        s.add_lorentz_material(f"l{q}", eps_inf, kappa, wp, w0, gamma).add_box(at(m["lo"]), at(m["hi"]), priority=1)
    for q, m in enumerate(case["magnetic"]):
        s.add_material(f"f{q}", eps_r=m["eps_r"], mu_r=m["mu_r"], sigma_m=m["sigma_m"]).add_box(at(m["lo"]), at(m["hi"]), priority=1)
    for q, (sigma, t, lo, hi) in enumerate(case["sheets"]):
        s.add_conducting_sheet(f"s{q}", sigma, t).add_box(at(lo), at(hi))
    for q, el in enumerate(case["elements"]):
        s.add_lumped_element(f"e{q}", "xyz"[el["dir"]], R=el["R"], L=el["L"], C=el["C"], kind=el["kind"]).add_box(at(el["lo"]), at(el["hi"]))
    px, py, z0, z1 = case["port"]
    s.add_lumped_port(1, 50.0, at((px, py, z0)), at((px, py, z1)), "z", 1.0)
    mt = case["metal"]
    if mt is not None:      # a ball (or a tilted disc inside that ball) that touches the plane towards the media
        lo, hi = at(mt["lo"]), at(mt["hi"])
        r = 0.47 * min(hi[a] - lo[a] for a in range(3))      # (clear of the far plane of its box: that one may lie next to a Mur face)
        c = [0.5 * (lo[a] + hi[a]) + mt["shift"][a] * (0.5 * (hi[a] - lo[a]) - r) for a in range(3)]
        c[0] = hi[0] - r if mt["side"] == 0 else lo[0] + r
        if mt["shape"] == "sphere":
            s.add_metal("ball").add_sphere(c, r)
        else:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from primitives_cases import rot
            h = 0.8
            d = s.add_metal("dish")
            d.add_cylinder((0.0, 0.0, -h), (0.0, 0.0, h), float(np.sqrt(r * r - h * h)))
            d.boxes[-1].matrix = rot(0, mt["tilt"][0]) @ rot(1, mt["tilt"][1])
            d.boxes[-1].matrix[:3, 3] = c
    pw = case["planewave"]
    if pw is not None:
        s.add_plane_wave("pw", pw["e0"], pw["dir"]).add_box(at(pw["lo"]), at(pw["hi"]))
    for q, x in enumerate(case.get("excite") or []):      # H-field excitations: point boxes at the face centres
        c, p = x["comp"], x["node"]
        centre = [1e3 * (float(lines[a][p[a]]) if a == c else 0.5 * float(lines[a][p[a]] + lines[a][p[a] + 1])) for a in range(3)]
        val = [0.0, 0.0, 0.0]
        val[c] = x["val"]
        s.add_field_excitation(f"x{q}", x["type"], val, centre, centre, delay=x["delay"])
    vox = sc.voxelize(s, grid, conformal=mt is not None)
    total = sum(case["calls"])
    return simm.Simulation(grid, vox, f0=MEDIA_F0, fc=MEDIA_FC, boundary=case["kinds"], cpml_cells=case["cells"], nr_ts=total + 8,
                           end_criteria=0.0, nf2ff_freqs=None if case["nf2ff"] == "none" else [MEDIA_F0, 1.3 * MEDIA_F0],
                           use_classes=case["classes"], nf2ff_mode="dft" if case["nf2ff"] == "none" else case["nf2ff"], conformal=mt is not None)


def corrections_present(sim):
    """Which of the eight corrections the engine steps for this simulation."""
    have = (sim.debye is not None, sim.lorentz is not None, sim.sheets is not None, sim.element_stepped.size > 0, sim.magnetic is not None,
            sim.conformal is not None, sim.plane_wave is not None, sim.excite_h_args is not None)
    return {name for name, h in zip(CORRECTION_NAMES, have) if h}


def watch_plane_wave(ref):
    """Hooks on a Restatement: did the plane wave's two lists change V / I on their elements, and the H-field excitations I on their
    faces?  The returned dict answers per list ("pw_e", "pw_h", "excite")."""
    changed, held = {name: False for name in ("pw_e", "pw_h", "excite") if name in ref.parts}, {}

    def before(name, kind, F):
        if name in changed and not changed[name]:
            held[name] = [a.copy() for a in F]

    def after(name, kind, F):
        if name in held:
            changed[name] = any(np.any(a != b) for a, b in zip(F, held.pop(name)))
    ref.before, ref.after = before, after
    return changed


def corrections_reference_problems(r):
    """media_reference_problems for every correction present: what the reference side must show by itself.  `r.pw_changed`: what
    watch_plane_wave returned for it."""
    problems = media_reference_problems(r)
    if r.lorentz is not None:
        L = r.lorentz
        for c in range(3):
            if not L.w[c].size:
                continue
            live = (L.w[c] != 0) & (L.vi[c] != 0)
            need = live[None] & (L.tab[c][1][:, 0] != 0)      # (gam == 0: the padding poles of a shorter medium, which stay at rest)
            if not np.isfinite(L.x[c]).all():
                problems.append(f"reference Lorentz states of component {c} not finite")
            if live.any() and (not np.all(L.x_moved[c][:, 0][need]) or not np.all(L.vprev[c][live] != 0)):
                problems.append(f"component {c}: {np.count_nonzero(~L.x_moved[c][:, 0][need])} Lorentz branch currents of {np.count_nonzero(need)} never left zero")
            if np.any(L.x[c][:, :, ~live] != 0) or np.any(L.vprev[c][~live] != 0):
                problems.append(f"component {c}: Lorentz states of edges that are not dispersive edges moved")
        if not any(((L.w[c] != 0) & (L.vi[c] != 0)).any() for c in range(3) if L.w[c].size):
            problems.append("reference: Lorentz media without a live edge")
    if r.elements is not None and not (np.isfinite(r.elements.x).all() and np.all(np.any(r.elements.x != 0, axis=0))):
        problems.append("reference: an element edge without branch current")
    if r.magnetic is not None:
        for c in range(3):
            on = r.magnetic.cls[c] != 0
            if on.any() and not (np.isfinite(r.magnetic.iprev[c]).all() and np.all(r.magnetic.iprev[c][on] != 0)):
                problems.append(f"reference: i_prev of {np.count_nonzero(r.magnetic.iprev[c][on] == 0)} magnetic faces of component {c} is zero")
    if r.conformal is not None and not (r.conformal.iprev.size and np.isfinite(r.conformal.iprev).all() and np.all(r.conformal.iprev != 0)):
        problems.append("reference: i_prev of a listed conformal face is zero")
    if r.pw_e is not None and not all(r.pw_changed.values()):
        problems.append(f"reference: the plane wave's lists changed nothing (V: {r.pw_changed['pw_e']}, I: {r.pw_changed['pw_h']})")
    if r.excite is not None:
        if not r.pw_changed["excite"]:
            problems.append("reference: the H-field excitations changed no current")
        l = r.excite.lists
        held = (l.hard[3].astype(np.int64) >= r.nstep) if r.nstep else np.zeros(0, bool)      # hard faces whose entry never read the table: amp * 0.0f
        for g, c in zip(l.hard[0][held], l.hard[1][held]):
            if r.e.get_field(1, int(c)).reshape(-1)[g] != 0:
                problems.append(f"reference: the hard face at node {int(g)}, component {int(c)} is not held at zero")
    return problems


def _differs(name, a, b):
    if a.shape != b.shape:
        return [f"{name}: shape {a.shape} vs {b.shape}"]
    if np.array_equal(a, b):
        return []
    bad = np.argwhere(a != b)
    return [f"{name} differs at {len(bad)} of {b.size} entries, first {tuple(int(v) for v in bad[0])}: {a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}"]


def corrections_state_problems(eh, r):
    """Fields and every state array of the HIP engine against the restatement, bit for bit."""
    problems = []
    fh, fo = eh.fields(), r.e.fields()
    problems += _differs("fields", fh, fo)
    if not problems:
        nzm = fo != 0
        if not np.array_equal(fh[nzm].view(np.uint32), fo[nzm].view(np.uint32)):
            problems.append("fields equal as values but not as bits where the reference is non-zero")
    for c in range(3 if r.debye else 0):
        hv, hu, hvi = eh.debye_state(c)
        for name, a, b in (("v_prev", hv, r.debye.vprev[c]), ("u", hu, r.debye.u[c]), ("vi", hvi, r.debye.vi[c])):
            problems += _differs(f"Debye {name} of component {c}", a, b)
    if r.lorentz is not None:
        for c in range(3):
            for name, a, b in zip(("v_prev", "x", "vi"), eh.lorentz_state(c), (r.lorentz.vprev[c], r.lorentz.x[c], r.lorentz.vi[c])):
                problems += _differs(f"Lorentz {name} of component {c}", a, b)
    if r.sheets is not None:
        hv, hib = eh.sheet_state()
        problems += _differs("sheet v_prev", hv, r.sheets.vprev) + _differs("sheet branch currents", hib, r.sheets.ib)
    if r.elements is not None:
        hv, hx = eh.lumped_state()
        problems += _differs("element v_prev", hv, r.elements.vprev) + _differs("element states", hx, r.elements.x)
    if r.magnetic is not None:
        for c in range(3):
            problems += _differs(f"magnetic i_prev of component {c}", eh.magnetic_state(c)[0], r.magnetic.iprev[c])
    if r.conformal is not None:
        problems += _differs("conformal i_prev", eh.conformal_state(), r.conformal.iprev)
    return problems


def corrections_reference(sim, oracle, seed=None):
    """The Restatement of everything `sim` holds, with the plane wave's lists watched (.pw_changed)."""
    ref = _restatement().Restatement(sim, oracle, seed=seed)
    ref.pw_changed = watch_plane_wave(ref)
    return ref


def run_corrections_case(case, hip, oracle):
    """hip = None: the reference side alone (what tests/test_corrections_fuzz_cpu.py steps without a GPU).  Compared after every call."""
    capi = _mod("_capi")
    flags = {"auto": 0, "direct": capi.FLAG_KERNEL_DIRECT, "half": 0}[case["drive"]]
    saved = {k: os.environ.pop(k, None) for k in ENV_KNOBS}
    os.environ.update(case["env"])
    problems = []
    try:
        so = corrections_case_sim(case)
        ref = corrections_reference(so, oracle, case["seed"])
        sh = eh = None
        if hip is not None:
            sh = corrections_case_sim(case)
            eh = sh.build(hip, flags=flags)
            rng = np.random.default_rng(case["seed"])
            for kind in (0, 1):
                for c in range(3):
                    eh.set_field(kind, c, (1e-3 * rng.standard_normal(eh.local_shape)).astype(np.float32))
        done = 0
        for q, nsteps in enumerate(case["calls"]):
            if q and case["sets"][q - 1] is not None:      # fdtd_set_field between two calls: re-primes i_prev, leaves the E-side states alone
                kind, comp, seed = case["sets"][q - 1]
                a = (1e-3 * np.random.default_rng(seed).standard_normal(ref.e.local_shape)).astype(np.float32)
                ref.set_field(kind, comp, a)
                if eh is not None:
                    eh.set_field(kind, comp, a)
            ref.run(nsteps)
            done += nsteps
            if eh is None:
                continue
            if case["drive"] == "half":
                for _ in range(nsteps):
                    eh.half_step(0)
                    eh.half_step(1)
            else:
                eh.run(nsteps)
            if not problems:      # the first call where something differs names itself; later ones only repeat it
                found = corrections_state_problems(eh, ref)
                for (uid, iid), (ru, ri) in zip(sh._port_probe_ids, so._port_probe_ids):
                    for name, a, b in (("port voltage", eh.get_probe(uid), ref.get_probe(ru)), ("port current", eh.get_probe(iid), ref.get_probe(ri))):
                        if not np.array_equal(np.asarray(a)[:done], np.asarray(b)[:done]):
                            found.append(f"{name} series differs")
                problems += [f"after call {q} ({done} timesteps): {p}" for p in found]
    finally:
        for k in ENV_KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    problems = corrections_reference_problems(ref) + problems
    if eh is None:
        return problems, {"launches_per_timestep": 0, "lag_planes": 0, "timesteps_per_launch_max": 0}
    for (ru, ri) in so._port_probe_ids:
        if not (np.abs(ref.get_probe(ru)).max() > 0 and np.abs(ref.get_probe(ri)).max() > 0):
            problems.append("reference: a port series is all zero")
    if case["nf2ff"] != "none":
        bh, bo = sh.nf2ff_boxes(), so.nf2ff_boxes()
        worst = max(float(np.abs(np.asarray(a) - np.asarray(b)).max()) / max(float(np.abs(b).max()), 1e-300) for a, b in zip(bh, bo))
        if len(bh) != len(bo) or not worst <= 1e-6:
            problems.append(f"NF2FF face spectra differ ({worst:.2e} of the largest entry)")
    info = eh.schedule_info()
    if info["resident"] or info["launches_per_timestep"] not in (2, 3):
        problems.append(f"schedule {info}: a context with corrections steps under two or three launches per timestep")
    eh.close()
    return problems, info


def load_libs():
    capi = _mod("_capi")
    so = os.path.join(ROOT, "oracle", "libfdtd_oracle.so")
    src = os.path.join(ROOT, "oracle", "fdtd_oracle.c")
    if not os.path.isfile(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    import torch  # noqa: F401  (warms the ROCm runtime)
    return capi.load_hip_library(), capi.bind(ctypes.CDLL(so))


def run_batch(ncases, seed, hip, oracle, only=None, log=print, slabs=False, mur=False, media=False, corrections=False):
    rng = np.random.default_rng(seed)
    failed = []
    for n in range(ncases):
        case = draw_corrections_case(rng, excite=(seed, n)) if corrections else draw_media_case(rng) if media else draw_slab_case(rng) if slabs else draw_case(rng, mur)
        if only is not None and n != only:
            continue
        t0 = time.perf_counter()
        try:
            problems, info = (run_corrections_case if corrections else run_media_case if media else run_slab_case if slabs else run_case)(case, hip, oracle)
        except ValueError as exc:      # a drawn set-up the host layer refuses (e.g. layers that leave no room for the NF2FF box)
            log(f"case {n}: skipped ({exc}) {case}")
            continue
        except _mod("_capi").FdtdError as exc:      # an error from the library (a bounded wait that ran out, ...) is a failing case
            if media or corrections:      # ... always with --media / --corrections: no schedule is forced there that the library may refuse
                pass
            elif "(-5): resident schedule" in str(exc) or "(-5): wavefront schedule" in str(exc):    # ... or a grid the schedule asked for by name cannot hold
                log(f"case {n}: refused ({str(exc)[:120]}) {case}")
                continue
            if not (media or corrections) and "not starvation-free" in str(exc):    # ... except a drawn decomposition the library REFUSES: slabs sharing the test GPU that could pin every workgroup slot
                log(f"case {n}: refused ({str(exc)[:150]}...) {case}")
                continue
            log(f"case {n}: FAIL (library error) {case}  -> {exc}")
            failed.append((n, case, [str(exc)]))
            continue
        tag = "ok  " if not problems else "FAIL"
        log(f"case {n}: {tag} {time.perf_counter() - t0:5.1f} s  launches/ts {info['launches_per_timestep']} lag {info['lag_planes']} "
            f"ts/launch {info['timesteps_per_launch_max']}  {case}" + ("  -> " + "; ".join(problems) if problems else ""))
        if problems:
            failed.append((n, case, problems))
    return failed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=60)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--slabs", action="store_true", help="decomposed runs: 2 ... 6 P2P slabs in one process against one slab on the oracle")
    ap.add_argument("--mur", action="store_true", help="every case with Mur faces, mostly on the two / three launches per timestep")
    ap.add_argument("--media", action="store_true", help="scenes with Debye media and / or conducting sheets against the numpy restatement of their corrections")
    ap.add_argument("--corrections", action="store_true", help="scenes with at least three of the eight corrections of the step loop (often all) in one context against tests/restatement.py")
    args = ap.parse_args()
    hip, oracle = load_libs()
    failed = run_batch(args.cases, args.seed, hip, oracle, args.only, log=lambda s: print(s, flush=True), slabs=args.slabs, mur=args.mur, media=args.media,
                       corrections=args.corrections)
    print(f"{len(failed)} failing case(s) of {args.cases} (seed {args.seed})", flush=True)
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
