"""Soft sources and probes through the raw C ABI: the cases of tests/test_sources_probes_cpu.py (oracle against numpy restatements, and
where every case sits relative to the thresholds of the kernels) and tests/test_sources_probes_gpu.py (libfdtd_hip.so under every
schedule against the oracle) — and, cut into z-slabs of one process under every halo transport, of
tests/test_slab_sources_probes_gpu.py (run_slabs, tree_series with planes=, the S cases, the drawn slab batch).  No test functions here.

A node is addressed by its global flat index (k * ny + j) * nx + i, an edge / face by (node, component)."""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
from conftest import pkg
from helpers import seeded_fields

KIND_V, KIND_I = 0, 1
# csrc/fdtd_ctx.h, csrc/kernel_common.hpp, csrc/resident.hip
BLOCK, SRC_SCAN_MAX, RES_MAX_SRC, RES_MAX_PRB, MAX_PROBES = 256, 32, 128, 256, 64
KNOBS = ("FDTD_TYS", "FDTD_WF_MULTI", "FDTD_RESIDENT", "FDTD_RES_CHUNK", "FDTD_WAVEFRONT", "FDTD_MUR_APPLY_PASS")
SCHEDULES = ("DIRECT", "WF1", "WFM", "RESIDENT", "AUTO")   # WF1: WAVEFRONT with FDTD_WF_MULTI=1, WFM: WAVEFRONT with the default


# ---- engines ----------------------------------------------------------------------------------------------------------------------
def raw_engine(lib, grid_case, boundary, flags=0, max_steps=8, *, cpml_cells=3, rank=0, world=1, slab=None, hard=None):
    """An engine on the uniform random-material scene `grid_case` = (seed, (nx, ny, nz)) (opbuild_cases.random_scene without PEC or
    lumped edges), its operator built by the library, `boundary` one kind or six ('PEC' / 'MUR' / 'CPML') set the way
    Simulation.build sets them.  `hard`: (idx, comp) of hard E edges — overrides with vv = m = 0 on every rank, as Simulation._overrides
    makes them (fdtd_build_operator keeps those of its slab).  The engine carries .grid and .dt."""
    capi, eco, const, cp, simm = pkg("_capi"), pkg("ecoperator"), pkg("constants"), pkg("cpml"), pkg("simulation")
    from opbuild_cases import random_scene
    seed, shape = grid_case
    grid, eps, kap, pec, _ = random_scene(seed, shape, False, 3, n_lumped=0, pec_frac=0.0)
    dt = grid.courant_dt()
    nx, ny, nz = grid.shape
    k0, nk = (0, nz) if slab is None else slab
    e = capi.Engine(lib, nx, ny, nz, dt, k0=k0, nk=nk, rank=rank, world=world, max_steps=max_steps, flags=flags)
    emet, hmet = eco.pack_metric_tables(*eco.metric_lists(grid, dt), grid, k0, nk)
    over = eco.lumped_overrides(grid, eps, kap, pec, dt, [])
    if hard is not None:
        z = np.zeros(len(hard[0]), np.float32)
        over = (np.concatenate([over[0], np.asarray(hard[0], np.int64)]), np.concatenate([over[1], np.asarray(hard[1], np.int8)]),
                np.concatenate([over[2], z]), np.concatenate([over[3], z]))
    e.build_operator(grid.d, eps, kap, pec, const.EPS0, over, emet, hmet)
    bc = simm.BoundarySpec.parse(boundary, cpml_cells)
    cells = bc.face_cells()
    if any(cells):
        spec = cp.CPMLSpec(**{**bc.cpml.__dict__, "cells": cells})
        e.set_cpml(*cp.build_cpml(grid, dt, spec).for_slab(k0, nk))
    if "MUR" in bc.kinds:
        coeff = []
        for f in range(6):
            l = grid.lines[f // 2]
            d = (l[-1] - l[-2]) if f % 2 else (l[1] - l[0])
            coeff.append((const.C0 * dt - d) / (const.C0 * dt + d))
        e.set_mur([1 if k == "MUR" else 0 for k in bc.kinds], coeff)
    e.grid, e.dt = grid, dt
    return e


@dataclass
class Case:
    name: str
    shape: tuple                 # (nx, ny, nz)
    boundary: tuple              # six kinds, x- x+ y- y+ z- z+
    cpml_cells: int
    signal: np.ndarray
    sources: list                # add_source calls (idx, comp, amp, delay)
    probes: list                 # (kind, idx, comp, w)
    calls: tuple                 # lengths of the run calls
    later: list = field(default_factory=list)    # (after_call, "source" | "probe", the call): added when that many run calls have returned
    max_steps: int = 0           # 0: eight more than the calls take
    seed: Optional[int] = None   # seeded initial fields (helpers.seeded_fields)
    scene: int = 5               # seed of the materials
    keep_frames: bool = False    # reference() keeps the oracle's fields of every timestep (the cases that are cut into slabs)
    env: dict = field(default_factory=dict)      # knobs read by fdtd_create ($FDTD_TYS ...)
    expect: dict = field(default_factory=dict)   # where the case is meant to sit: keys of regimes(), checked without a GPU
    hard: Optional[tuple] = None                 # hard E edges (idx, comp, amp, delay), each once: operator overrides vv = m = 0 and a source
                                                 # list behind `sources`, as Simulation adds them

    @property
    def nsteps(self):
        return int(sum(self.calls))

    @property
    def cap(self):
        return self.max_steps or self.nsteps + 8

    def all_sources(self):
        """[(first timestep, call)] in the order the engine's list holds them."""
        out = [(0, s) for s in self.sources] + ([(0, self.hard)] if self.hard is not None else [])
        for after, what, call in self.later:
            if what == "source":
                out.append((int(sum(self.calls[:after])), call))
        return out

    def all_probes(self):
        out = [(0, p) for p in self.probes]
        for after, what, call in self.later:
            if what == "probe":
                out.append((int(sum(self.calls[:after])), call))
        return out

    def describe(self):
        return {"name": self.name, "shape": self.shape, "boundary": self.boundary, "cpml_cells": self.cpml_cells, "calls": self.calls,
                "max_steps": self.cap, "seed": self.seed, "env": self.env, "nsig": len(self.signal),
                "sources": [(len(s[0]), int(np.min(s[3])), int(np.max(s[3]))) for _, s in self.all_sources()],
                "probes": [(p[0], len(p[1])) for _, p in self.all_probes()], "later": [(a, w) for a, w, _ in self.later]}


def src(idx, comp, amp, delay):
    return (np.asarray(idx, np.int64), np.asarray(comp, np.int8), np.asarray(amp, np.float32), np.asarray(delay, np.int32))


def prb(kind, idx, comp, w):
    return (int(kind), np.asarray(idx, np.int64), np.asarray(comp, np.int8), np.asarray(w, np.float32))


def seeded_slab_fields(engine, seed, scale=1e-3):
    """helpers.seeded_fields' arrays of the WHOLE grid, the engine's planes of them: a slab starts from its slice of the single slab's
    initial fields."""
    rng = np.random.default_rng(seed)
    for kind in (0, 1):
        for c in range(3):
            g = (scale * rng.standard_normal((engine.nz, engine.ny, engine.nx))).astype(np.float32)
            engine.set_field(kind, c, np.ascontiguousarray(g[engine.k0:engine.k0 + engine.nk]))


def apply(case, engine, without=None):
    """Signal, initial fields, the sources (but call number `without`) and the probes of before the first timestep."""
    engine.set_signal(case.signal)
    if case.seed is not None:
        seeded_slab_fields(engine, case.seed)
    for n, s in enumerate(case.sources + ([case.hard] if case.hard is not None else [])):
        if n != without:
            engine.add_source(*s)
    return [engine.add_probe(*p) for p in case.probes]


def run(case, engine, runner=None, without=None):
    """The run calls, the later additions between them.  `runner(engine, n)` steps n timesteps (default: one fdtd_run)."""
    n_src = len(case.sources) + (case.hard is not None)
    for c, n in enumerate(case.calls):
        (runner or (lambda e, m: e.run(m)))(engine, n)
        for after, what, call in case.later:
            if after != c + 1:
                continue
            if what == "probe":
                engine.add_probe(*call)
            else:
                if n_src != without:
                    engine.add_source(*call)
                n_src += 1


def engine_for(case, lib, flags=0, without=None, **kw):
    e = raw_engine(lib, (case.scene, case.shape), case.boundary, flags, case.cap, cpml_cells=case.cpml_cells,
                   hard=None if (case.hard is None or kw.pop("soft_operator", False)) else case.hard[:2], **kw)
    apply(case, e, without)
    return e


def series_of(case, engine):
    return [engine.get_probe(q) for q in range(len(case.all_probes()))]


# ---- z-slabs in one process -----------------------------------------------------------------------------------------------------------
TRANSPORTS = ("p2p-two", "p2p-one", "linked-split", "linked-nosplit", "half-steps")
# what fdtd_schedule_info reports as the halo transport (linked: once fdtd_run_linked has linked the contexts)
TRANSPORT_REPORTED = {"p2p-two": "p2p", "p2p-one": "p2p", "linked-split": "linked", "linked-nosplit": "linked", "half-steps": "external"}


def transport_flags(transport):
    capi = pkg("_capi")
    return {"p2p-two": capi.FLAG_KERNEL_DIRECT, "p2p-one": capi.FLAG_KERNEL_WAVEFRONT, "linked-split": capi.FLAG_OVERLAP_ON,
            "linked-nosplit": capi.FLAG_OVERLAP_OFF, "half-steps": 0}[transport]


def slab_stepper(engines, transport):
    """step(n): n timesteps of adjacent slabs of one process under `transport`.  The mailbox transports attach here (before the first
    timestep); "half-steps" carries the halos through the host, the H halo of "step -1" (the initial fields) before the first timestep."""
    capi = pkg("_capi")
    if transport.startswith("p2p"):
        blobs = [e.p2p_export() for e in engines]
        for r, e in enumerate(engines):
            e.p2p_attach(blobs[r - 1] if r > 0 else None, blobs[r + 1] if r + 1 < len(engines) else None)
    if transport != "half-steps":
        return lambda n: capi.run_linked(engines, n)
    pairs = list(zip(engines[:-1], engines[1:]))

    def h_up():
        for lo, hi in pairs:
            hi.halo_put(capi.HALO_H_UP, lo.halo_get(capi.HALO_H_UP))

    def step(n):
        if engines[0].step == 0:
            h_up()
        for _ in range(n):
            for e in engines:
                e.half_step(capi.PHASE_E)
            for lo, hi in pairs:
                lo.halo_put(capi.HALO_E_DOWN, hi.halo_get(capi.HALO_E_DOWN))
            for e in engines:
                e.half_step(capi.PHASE_H)
            h_up()
    return step


def run_slabs(case, lib, cuts, transport):
    """The case on the slabs `cuts` = [(k0, nk)] of one process, coupled by `transport`: every rank takes the whole lists (the library
    keeps what it owns), its slice of the seeded fields, and the later additions between the calls.  Returns the engines."""
    world = len(cuts)
    engines = [engine_for(case, lib, transport_flags(transport), rank=r, world=world, slab=tuple(s)) for r, s in enumerate(cuts)]
    step = slab_stepper(engines, transport)
    for c, n in enumerate(case.calls):
        step(n)
        for after, what, call in case.later:
            if after == c + 1:
                for e in engines:
                    (e.add_probe if what == "probe" else e.add_source)(*call)
    return engines


# ---- references -------------------------------------------------------------------------------------------------------------------
def tree_sum(w, f):
    """probe_block's sum (csrc/kernel_common.hpp) in float64: thread t adds its cells t, t + 256, ... in order, s = fma(w, f, s) — the
    product of two float32 values is exact in double, so s + w * f rounds once, as the fma does —, then red[t] += red[t + h] for
    h = 128 ... 1."""
    p = np.asarray(w, np.float32).astype(np.float64) * np.asarray(f, np.float32).astype(np.float64)
    rows = -(-p.size // BLOCK)
    p = np.concatenate([p, np.zeros(rows * BLOCK - p.size)]).reshape(rows, BLOCK)
    s = np.zeros(BLOCK)
    for r in p:
        s = s + r
    h = BLOCK // 2
    while h:
        s[:h] = s[:h] + s[h:2 * h]
        h //= 2
    return float(s[0])


def in_planes(case, idx, planes):
    """Which nodes of `idx` lie in the planes (k0, nk): the entries to_local (csrc/api.hip) keeps of a list on the slab of those planes."""
    k = np.asarray(idx, np.int64) // (case.shape[0] * case.shape[1])
    return (k >= planes[0]) & (k < planes[0] + planes[1])


def clip_to_planes(case, probe, planes):
    """A probe (kind, idx, comp, w) with the entries a slab keeps of it, in list order."""
    keep = in_planes(case, probe[1], planes)
    return (probe[0], probe[1][keep], probe[2][keep], probe[3][keep])


def tree_series(case, fields_per_step, planes=None):
    """Per probe the series of probe_block's sums from `fields_per_step`: per timestep (V, I), float32 [3][nz][ny][nx], V after the E
    half-step (Mur passes and sources applied), I after the H half-step.  Zero before a probe was added and nothing beyond max_steps.
    `planes` = (k0, nk): the series of the rank that owns those planes — every list clipped to them, so that thread t takes the
    entries t, t + 256, ... of the CLIPPED list (all zero where the rank owns no cell)."""
    probes = [(first, p if planes is None else clip_to_planes(case, p, planes)) for first, p in case.all_probes()]
    out = [np.zeros(min(case.nsteps, case.cap)) for _ in probes]
    for step, (V, I) in enumerate(fields_per_step):
        if step >= case.cap:
            break
        for q, (first, (kind, idx, comp, w)) in enumerate(probes):
            if step >= first:
                F = (V if kind == KIND_V else I).reshape(3, -1)
                out[q][step] = tree_sum(w, F[comp.astype(np.int64), idx])
    return out


def half_stepper(frames):
    """A runner for run(): half-steps the engine and keeps (V, I) of every timestep in `frames`."""
    def runner(e, n):
        for _ in range(n):
            e.half_step(0)
            V = np.stack([e.get_field(KIND_V, c) for c in range(3)])
            e.half_step(1)
            frames.append((V, np.stack([e.get_field(KIND_I, c) for c in range(3)])))
    return runner


_REF = {}


def reference(case, oracle_lib):
    """The oracle's run of a case, computed once: final fields, its own (sequential) probe series, tree_series of its fields."""
    if case.name not in _REF:
        e = engine_for(case, oracle_lib)
        frames = []
        run(case, e, half_stepper(frames))
        ref = {"fields": e.fields(), "own": series_of(case, e), "tree": tree_series(case, frames), "step": e.step}
        for a in [ref["fields"]] + ref["own"] + ref["tree"]:
            a.setflags(write=False)
        if case.keep_frames:      # every cut of the case is cut from this one run (slab_trees)
            for V, I in frames:
                V.setflags(write=False), I.setflags(write=False)
            ref["frames"], ref["slab_trees"] = frames, {}
        _REF[case.name] = ref
    return _REF[case.name]


def forget(case):
    """Drop a case's reference (the drawn slab cases keep the fields of every timestep: not for the whole session)."""
    _REF.pop(case.name, None)


def slab_trees(case, oracle_lib, cuts):
    """Per rank of `cuts` = [(k0, nk)] the tree_series of that rank, from the frames of the case's one oracle run."""
    ref = reference(case, oracle_lib)
    key = tuple(cuts)
    if key not in ref["slab_trees"]:
        ref["slab_trees"][key] = [tree_series(case, ref["frames"], planes=s) for s in cuts]
        for t in ref["slab_trees"][key]:
            for a in t:
                a.setflags(write=False)
    return ref["slab_trees"][key]


# ---- where a case sits: the host logic of csrc/ restated (integer arithmetic) -------------------------------------------------------
def default_tys(shape):
    """choose_tiling (csrc/kernels.hip) for grids within the Infinity Cache."""
    nx, ny, _ = shape
    P4 = (nx + 3) // 4
    best, best_cost = 1, 1e30
    for tys in range(4, 41):
        rows = min(tys, ny)
        t = rows * P4
        nbs = -(-t // BLOCK)
        cost = (nbs * BLOCK - t) / (nbs * BLOCK) + 1.0 / tys * 0.15
        if cost < best_cost - 1e-12:
            best_cost, best = cost, rows
    return best


def tys_of(case):
    v = case.env.get("FDTD_TYS")
    return min(int(v), case.shape[1]) if v else default_tys(case.shape)


def res_tiling(shape):
    """res_tiling (csrc/resident.hip): plane bounds kt, row bounds jt, or None."""
    nx, ny, nk = shape
    P4 = (nx + 3) // 4
    if P4 > BLOCK:
        return None
    ZT = 2 if (4 * P4 <= BLOCK and nk >= 4) else 1
    Rmax = min(ny, BLOCK // (ZT * P4))
    nstrips = -(-ny // Rmax)
    jt = [0]
    for s in range(nstrips):
        jt.append(jt[-1] + ny // nstrips + (1 if s < ny % nstrips else 0))
    kt = [0]
    if ZT == 1:
        kt += list(range(1, nk + 1))
    else:
        kt.append(2)
        if nk & 1:
            kt.append(3)
        while kt[-1] < nk:
            kt.append(kt[-1] + 2)
    return kt, jt


def _kji(case, idx):
    nx, ny, _ = case.shape
    idx = np.asarray(idx, np.int64)
    return idx // (nx * ny), (idx // nx) % ny, idx % nx


def regimes(case):
    """The facts the planner and the kernels branch on, with every source and probe of the case added."""
    nx, ny, nz = case.shape
    P4 = (nx + 3) // 4
    tys = tys_of(case)
    nstrips = -(-ny // tys)
    nbs = -(-tys * P4 // BLOCK)
    srcs = [s for _, s in case.all_sources()]
    sidx = np.concatenate([s[0] for s in srcs]) if srcs else np.zeros(0, np.int64)
    scomp = np.concatenate([s[1] for s in srcs]).astype(np.int64) if srcs else np.zeros(0, np.int64)
    k, j, i = _kji(case, sidx)
    sp = np.bincount(k * nstrips + j // tys, minlength=nz * nstrips)
    dup = np.unique(sidx * 4 + scomp).size < sidx.size
    sp_max = int(sp.max()) if sidx.size else 0
    count_ok = not (dup and sp_max > BLOCK)
    mur = [b == "MUR" for b in case.boundary]
    near = False
    if any(mur) and sidx.size:
        pos, n = (i, j, k), (nx, ny, nz)
        for f in range(6):
            a = f // 2
            if a == 2 or mur[f]:      # (a z face may live on another rank: the planner asks every z face once there is a Mur face)
                near |= bool(np.any(pos[a] >= n[a] - 2 if f & 1 else pos[a] <= 1))
    # blocks of a strip-plane the sources of the fullest strip-plane fall into
    t = (j % tys) * P4 + i // 4
    full = (k * nstrips + j // tys) == int(sp.argmax()) if sidx.size else np.zeros(0, bool)
    out = {"tys": tys, "threads_per_strip_plane": min(tys, ny) * P4, "blocks_per_strip_plane": nbs, "strip_planes": nz * nstrips,
           "sp_max": sp_max, "dup": bool(dup), "fusable": bool(count_ok and not near), "near_mur": bool(near),
           "path": "post" if not count_ok else ("none" if sp_max == 0 else "scan" if (sp_max <= SRC_SCAN_MAX or dup) else "dense"),
           "src_blocks": sorted(set((t[full] // BLOCK).tolist())), "src_in_last_group": int(np.sum(i[full] // 4 == P4 - 1)) if sidx.size else 0}
    kt, jt = res_tiling(case.shape)
    nst = len(jt) - 1

    def tile(idx):
        kk, jj, _ = _kji(case, idx)
        return (np.searchsorted(kt, kk, "right") - 1) * nst + np.searchsorted(jt, jj, "right") - 1
    ntiles = (len(kt) - 1) * nst
    out["tile_src_max"] = int(np.bincount(tile(sidx), minlength=ntiles).max()) if sidx.size else 0
    out["tile_src_tiles"] = int(np.unique(tile(sidx)).size) if sidx.size else 0
    probes = [p for _, p in case.all_probes()]
    pidx = np.concatenate([p[1] for p in probes]) if probes else np.zeros(0, np.int64)
    ptile = np.bincount(tile(pidx), minlength=ntiles) if pidx.size else np.zeros(ntiles, np.int64)
    out["tile_prb_max"] = int(ptile.max())
    out["res_tiles"], out["res_strips"] = ntiles, nst
    out["nprobes"] = len(probes)
    out["probe_cells_max"] = max([p[1].size for p in probes], default=0)
    own = []
    for p in probes:      # owner blocks of the one-launch schedule (build_wf_probe_tables)
        kk, jj, ii = _kji(case, p[1])
        own.append(np.unique(((kk * nstrips + jj // tys) * nbs + ((jj % tys) * P4 + ii // 4) // BLOCK)).size)
    out["owner_blocks_max"] = max(own, default=0)
    res_ok = nx >= 6 and ny >= 5 and nz >= 5
    if any(mur):
        res_ok &= not ((mur[2] and jt[1] - jt[0] < 2) or (mur[3] and jt[-1] - jt[-2] < 2))
        res_ok &= not ((mur[4] and kt[1] - kt[0] < 2) or (mur[5] and kt[-1] - kt[-2] < 2))
    out["res_why"] = ("" if res_ok else "tiling") or ("at most 128 source edges per tile" if out["tile_src_max"] > RES_MAX_SRC else
                                                      "at most 256 probe cells per tile" if out["tile_prb_max"] > RES_MAX_PRB else "")
    out["res_possible"] = out["res_why"] == ""
    # Mur faces inside one launch: what mur_direct_possible asks (no V-probe cell on the node plane of a Mur face)
    v_on_face = False
    for p in probes:
        if p[0] == KIND_V and p[1].size:
            kk, jj, ii = _kji(case, p[1])
            pos, n = (ii, jj, kk), (nx, ny, nz)
            for f in range(6):
                if mur[f]:
                    v_on_face |= bool(np.any(pos[f // 2] == (n[f // 2] - 1 if f & 1 else 0)))
    mur_ok = not any(mur) or (out["fusable"] and not v_on_face and nx >= 6 and ny >= 5 and nz >= 5 and 9 * nbs <= BLOCK)
    out["wf_possible"] = bool(mur_ok and nz >= 2 and count_ok)
    return out


def predict(case, sched, env=None):
    """'resident' | 'one' | 'two' | 'refused: <how the message starts>' for a single slab, as plan_schedule (csrc/api.hip) decides."""
    r = regimes(case)
    env = {**case.env, **(env or {})}
    if sched == "RESIDENT":
        if not r["res_possible"]:
            return "refused: resident schedule: " + r["res_why"]
        return "resident" if r["fusable"] else "refused: resident schedule: a source edge lies on or next to a Mur face"
    if sched in ("WF1", "WFM"):
        return "one" if r["wf_possible"] else "refused: wavefront schedule:"
    if sched == "DIRECT":
        return "two"
    if env.get("FDTD_RESIDENT") != "0" and r["fusable"] and r["res_possible"] and r["res_tiles"] <= 512:
        return "resident"
    blocks = r["strip_planes"] * r["blocks_per_strip_plane"]
    return "one" if r["wf_possible"] and ("CPML" in case.boundary or blocks >= 1700) else "two"


# ---- the directed cases -------------------------------------------------------------------------------------------------------------
def signal(n=60):
    t = np.arange(n)
    return (np.sin(2 * np.pi * 0.11 * t) * np.exp(-((t - 24.0) / 11.0) ** 2)).astype(np.float32)


def node(shape, i, j, k):
    return (np.asarray(k, np.int64) * shape[1] + np.asarray(j, np.int64)) * shape[0] + np.asarray(i, np.int64)


def _amps(rng, n):
    return (rng.uniform(0.4, 1.6, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def _weights(rng, n):
    """Weights of one sign per probe."""
    return (rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0])).astype(np.float32)


DIRECTED = {}
RUNS = []      # (case name, schedule, what predict() must say and schedule_info() must show, knobs on top of the case's)


def _add(case, runs):
    assert case.name not in DIRECTED
    DIRECTED[case.name] = case
    for r in runs:
        sched, outcome = r[0], r[1]
        RUNS.append((case.name, sched, outcome, r[2] if len(r) > 2 else {}))


def _d1(n, dup):
    """40 x 24 x 12, CPML-3, strips of 4 rows: n sources in the strip-plane (plane 6, rows 8..11: 4 x 40 x 3 = 480 edges), all distinct
    or with exactly one edge listed twice."""
    shape = (40, 24, 12)
    rng = np.random.default_rng(1000 + n + (500 if dup else 0))
    edges = np.array([(c, j, i) for c in range(3) for j in range(8, 12) for i in range(40)])
    edges = edges[rng.permutation(len(edges))]
    m = n - 1 if dup else n
    c, j, i = edges[:m].T
    idx, comp = node(shape, i, j, 6), c
    amp, delay = _amps(rng, m), rng.integers(-3, 41, m)
    if m >= 8:
        delay[[2, m - 3]] = [500, 81]            # never fire in the 80 timesteps
    if dup:      # one edge again, right behind its first entry (neighbouring threads of k_post's one-thread-per-entry loop): another amplitude, another delay
        at = min(5, m - 1)
        idx, comp = np.insert(idx, at + 1, idx[at]), np.insert(comp, at + 1, comp[at])
        amp, delay = np.insert(amp, at + 1, np.float32(-0.75) * amp[at] + np.float32(0.3)), np.insert(delay, at + 1, delay[at] + 2)
    probes = [prb(KIND_V, node(shape, [19, 20, 21], 9, 6), [2, 2, 2], [1, 1, 1]),
              prb(KIND_I, node(shape, [18, 19, 20, 21], [9, 9, 10, 10], 6), [0, 1, 0, 1], [-1, 1, 1, -1])]
    path = "post" if dup and n > BLOCK else "scan" if (n <= SRC_SCAN_MAX or dup) else "dense"
    case = Case(f"D1-{'dup' if dup else 'n'}{n}", shape, ("CPML",) * 6, 3, signal(), [src(idx, comp, amp, delay)], probes, (80,),
                env={"FDTD_TYS": "4"},
                expect={"tys": 4, "sp_max": n, "dup": dup, "path": path, "fusable": path != "post", "tile_src_max": n, "tile_src_tiles": 1,
                        "threads_per_strip_plane": 40, "blocks_per_strip_plane": 1})
    if path == "post":
        runs = [("DIRECT", "two"), ("AUTO", "two"), ("WF1", "refused: wavefront schedule:"), ("WFM", "refused: wavefront schedule:"),
                ("RESIDENT", "refused: resident schedule: at most 128 source edges per tile")]
    else:
        small = n <= RES_MAX_SRC
        runs = [("DIRECT", "two"), ("WF1", "one"), ("WFM", "one"), ("AUTO", "resident" if small else "one"),
                ("RESIDENT", "resident" if small else "refused: resident schedule: at most 128 source edges per tile")]
    _add(case, runs)


for _n in (1, 32, 33, 255, 256, 257, 480):
    _d1(_n, False)
for _n in (2, 33, 256, 257):
    _d1(_n, True)


def _d2(tys):
    """130 x 17 x 10, PEC: rows of 33 four-cell groups.  40 distinct sources in row 15 — with strips of 8 rows row 7 of its strip
    (threads 231..263: two blocks, i >= 100 in the second), with strips of 3 rows row 0 of a one-block strip — 20 of them at i >= 100,
    two in the last, partial group (i = 128, 129)."""
    shape = (130, 17, 10)
    rng = np.random.default_rng(2000)
    lo = rng.choice(np.arange(2, 100), 20, replace=False)
    hi = np.concatenate([rng.choice(np.arange(100, 128), 18, replace=False), [128, 129]])
    i = rng.permutation(np.concatenate([lo, hi]))
    comp = np.where(i == 129, 2, rng.integers(0, 3, 40))
    idx = node(shape, i, 15, 5)
    probes = [prb(KIND_V, node(shape, np.arange(96, 108), 15, 5), [2] * 12, _weights(rng, 12)),
              prb(KIND_I, node(shape, np.arange(97, 106), 14, 5), [0] * 9, _weights(rng, 9))]
    case = Case(f"D2-tys{tys}", shape, ("PEC",) * 6, 0, signal(), [src(idx, comp, _amps(rng, 40), rng.integers(-3, 30, 40))], probes, (60,),
                env={"FDTD_TYS": str(tys)},
                expect={"tys": tys, "sp_max": 40, "dup": False, "path": "dense", "fusable": True, "src_in_last_group": 2,
                        "threads_per_strip_plane": 33 * tys, "blocks_per_strip_plane": 2 if tys == 8 else 1,
                        "src_blocks": [0, 1] if tys == 8 else [0], "res_strips": 6, "tile_src_max": 40})
    _add(case, [("DIRECT", "two"), ("WF1", "one"), ("WFM", "one"), ("RESIDENT", "resident")])


_d2(8)
_d2(3)

FACES = ("x-", "x+", "y-", "y+", "z-", "z+")


def _d3(f, d):
    """22 x 20 x 18, Mur on all six faces: a source on an existing edge of each component at distance d from face f, a V-probe and an
    I-probe three cells further in."""
    shape = (22, 20, 18)
    a, hi = f // 2, f & 1
    rng = np.random.default_rng(3000 + 10 * f + d)
    mid = [11, 10, 9]

    def at(pos, shift):
        p = [mid[0] + shift, mid[1] - shift, mid[2] + shift]
        p[a] = pos
        return p
    pos = shape[a] - 1 - d if hi else d
    comps = [c for c in range(3) if not (c == a and pos >= shape[a] - 1)]     # (the normal edge does not exist on the high face itself)
    pts = np.array([at(pos, c - 1) for c in comps])
    idx = node(shape, pts[:, 0], pts[:, 1], pts[:, 2])
    inner = pos - 3 if hi else pos + 3
    q = np.array([at(inner, 0), at(inner, 1)])
    pidx = node(shape, q[:, 0], q[:, 1], q[:, 2])
    probes = [prb(KIND_V, pidx, [(a + 1) % 3, (a + 2) % 3], _weights(rng, 2)), prb(KIND_I, pidx, [(a + 2) % 3, (a + 1) % 3], _weights(rng, 2))]
    case = Case(f"D3-{FACES[f]}-d{d}", shape, ("MUR",) * 6, 0, signal(), [src(idx, comps, _amps(rng, len(comps)), [0, -2, 5][:len(comps)])],
                probes, (1, 59), scene=21, expect={"fusable": d == 2, "near_mur": d < 2, "res_possible": True})
    if d == 2:
        runs = [("AUTO", "resident"), ("DIRECT", "two"), ("RESIDENT", "resident"), ("WFM", "one")]
    else:
        runs = [("AUTO", "two"), ("DIRECT", "two"), ("RESIDENT", "refused: resident schedule: a source edge lies on or next to a Mur face"),
                ("WFM", "refused: wavefront schedule:")]
    _add(case, runs)


for _f in range(6):
    for _d in range(3):
        _d3(_f, _d)


def _d3_mixed():
    """Sources one cell from a PEC face (x+) and from a CPML face (y-) of a grid that has Mur faces elsewhere: neither orders anything."""
    shape = (22, 20, 18)
    rng = np.random.default_rng(3900)
    idx = node(shape, [20, 20, 11, 12], [10, 9, 1, 1], [9, 8, 9, 10])
    probes = [prb(KIND_V, node(shape, [17, 11], [10, 4], [9, 9]), [2, 2], _weights(rng, 2)),
              prb(KIND_I, node(shape, [17, 11], [10, 4], [9, 9]), [1, 0], _weights(rng, 2))]
    case = Case("D3-mixed", shape, ("MUR", "PEC", "CPML", "MUR", "MUR", "CPML"), 3, signal(), [src(idx, [1, 2, 0, 2], _amps(rng, 4), [0, 3, -1, 7])],
                probes, (1, 59), scene=21, expect={"fusable": True, "near_mur": False, "res_possible": True})
    _add(case, [("AUTO", "resident"), ("DIRECT", "two"), ("RESIDENT", "resident"), ("WFM", "one")])


_d3_mixed()


def _d4(kind, variant):
    """50 x 23 x 9: resident tiles of planes {0,1} {2} {3,4} {5,6} {7,8} x rows 0..7, 8..15, 16..22.  Source lines across the tiles, one
    tile with exactly 128 source edges; probes of both kinds interleaved in one tile, one tile with 256 probe cells, one probe with a
    cell in every tile.  variant 'src129' / 'prb257': one more in the full tile."""
    shape = (50, 23, 9)
    mur = kind == "MUR"
    rng = np.random.default_rng(4000 + (1 if mur else 0))
    kz = np.arange(2, 7) if mur else np.arange(0, 8)      # (with Mur faces a source stays two nodes off every face, or nothing is fused)
    zline = src(node(shape, 20, 4, kz), [2] * kz.size, _amps(rng, kz.size), rng.integers(-3, 20, kz.size))
    jy = np.arange(5, 19)
    yline = src(node(shape, 30, jy, 5), [1] * jy.size, _amps(rng, jy.size), rng.integers(0, 9, jy.size))
    cells = np.array([(c, k, j, i) for c in range(3) for k in (3, 4) for j in range(8, 16) for i in range(2, 47)])
    cells = cells[rng.permutation(len(cells))]
    n_full = 129 if variant == "src129" else 128
    c, k, j, i = cells[:n_full].T
    full = src(node(shape, i, j, k), c, _amps(rng, n_full), rng.integers(-3, 41, n_full))
    # probes: I before V in the list, their cells alternating in tile (plane 2, rows 16..20)
    pc = np.array([(j, i) for j in range(16, 21) for i in range(5, 41, 5)])
    p_i = prb(KIND_I, node(shape, pc[0::2, 1], pc[0::2, 0], 2), rng.integers(0, 3, len(pc[0::2])), _weights(rng, len(pc[0::2])))
    p_v = prb(KIND_V, node(shape, pc[1::2, 1], pc[1::2, 0], 2), rng.integers(0, 3, len(pc[1::2])), _weights(rng, len(pc[1::2])))
    pcells = np.array([(c, k, j, i) for c in range(3) for k in (5, 6) for j in range(8, 16) for i in range(2, 47)])
    pcells = pcells[rng.permutation(len(pcells))]
    n_big = 256 if variant == "prb257" else 255           # + the cell of the every-tile probe in this tile
    c, k, j, i = pcells[:n_big].T
    p_big = prb(KIND_V, node(shape, i, j, k), c, _weights(rng, n_big))
    ke, je = np.meshgrid([1, 2, 3, 5, 7], [4, 12, 20], indexing="ij")
    p_every = prb(KIND_I, node(shape, 25, je.ravel(), ke.ravel()), rng.integers(0, 3, 15), _weights(rng, 15))
    name = f"D4-{kind.lower()}" + (f"-{variant}" if variant else "")
    exp = {"tile_src_max": n_full, "tile_prb_max": n_big + 1, "res_tiles": 15, "res_strips": 3, "fusable": True,
           "res_possible": variant is None, "tile_src_tiles": (5 if mur else 7) + 1}
    case = Case(name, shape, (kind,) * 6, 3 if kind == "CPML" else 0, signal(), [zline, yline, full], [p_i, p_v, p_big, p_every], (23, 37),
                expect=exp)
    assert res_tiling(shape) == ([0, 2, 3, 5, 7, 9], [0, 8, 16, 23])
    if variant is None:
        runs = [("RESIDENT", "resident", {"FDTD_RES_CHUNK": "1"}), ("RESIDENT", "resident", {"FDTD_RES_CHUNK": "7"}), ("RESIDENT", "resident")]
    else:
        why = "at most 128 source edges per tile" if variant == "src129" else "at most 256 probe cells per tile"
        runs = [("RESIDENT", "refused: resident schedule: " + why), ("AUTO", "two" if mur else "one")]
    _add(case, runs)


for _k in ("MUR", "CPML"):
    for _v in (None, "src129", "prb257"):
        _d4(_k, _v)

D5_SHAPE = (20, 24, 12)


def _d5(reduced):
    """20 x 24 x 12, CPML-3, one-row strips (288 strip-planes), seeded fields and one source: all 64 probes in use.  `reduced`: the large
    probes cut down until every resident tile (two planes, all rows) holds at most 256 probe cells."""
    shape = D5_SHAPE
    nx, ny, nz = shape
    rng = np.random.default_rng(5000)
    every = [(c, k, j, i) for c in range(3) for k in range(nz) for j in range(ny) for i in range(nx)]
    every = np.array(every)[rng.permutation(3 * nx * ny * nz)]

    def cells(n, kind, where=None, repeat=0):
        if where is None:      # inner nodes: every edge there is live (the tangential edges of the outer node planes read 0)
            where = lambda e: np.all((e[:, 1:] >= 1) & (e[:, 1:] <= np.array([nz, ny, nx]) - 2), axis=1)
        e = every[where(every)]
        off = int(rng.integers(0, len(e) - n))
        c, k, j, i = e[off:off + n].T
        idx, comp = node(shape, i, j, k), c
        if repeat:
            pick = rng.integers(0, n, repeat)
            idx, comp = np.concatenate([idx, idx[pick]]), np.concatenate([comp, comp[pick]])
        return prb(kind, idx, comp, _weights(rng, idx.size))
    s_idx = node(shape, [10, 10, 11], [12, 13, 12], [6, 6, 6])
    sources = [src(s_idx, [2, 2, 1], [1.0, -0.5, 0.7], [0, 1, -2])]
    kk, jj = np.meshgrid(np.arange(nz), np.arange(ny), indexing="ij")
    sp_i = rng.integers(0, nx, kk.size)
    probes = [prb(KIND_V, [], [], []),                                                   # 0: no cells
              cells(1, KIND_I)]                                                          # 1: one cell
    if not reduced:
        probes += [cells(255, KIND_V), cells(256, KIND_I), cells(257, KIND_V), cells(400, KIND_I, repeat=200),   # 2..5
                   prb(KIND_V, node(shape, sp_i, jj.ravel(), kk.ravel()), rng.integers(0, 3, kk.size), _weights(rng, kk.size)),    # 6: a cell in every strip-plane
                   prb(KIND_I, node(shape, sp_i[::-1], jj.ravel(), kk.ravel()), rng.integers(0, 3, kk.size), _weights(rng, kk.size))]
    else:   # tiles are plane pairs: 30 + 30 + 30 + 40 cells drawn from one pair each, and a cell in every second row of every plane
        for q, (n, kind, rep) in enumerate([(30, KIND_V, 0), (30, KIND_I, 0), (30, KIND_V, 0), (30, KIND_I, 10)]):
            probes.append(cells(n, kind, where=lambda e, q=q: (e[:, 1] // 2 == q) & (e[:, 2] >= 1) & (e[:, 2] <= ny - 2), repeat=rep))
        sel = (jj.ravel() % 2 == 0)
        probes += [prb(KIND_V, node(shape, sp_i[sel], jj.ravel()[sel], kk.ravel()[sel]), rng.integers(0, 3, int(sel.sum())), _weights(rng, int(sel.sum()))),
                   prb(KIND_I, node(shape, sp_i[::-1][sel], jj.ravel()[sel], kk.ravel()[sel]), rng.integers(0, 3, int(sel.sum())), _weights(rng, int(sel.sum())))]
    shared = node(shape, 7, 8, 4)
    probes += [prb(KIND_V, [shared, node(shape, 8, 8, 4)], [1, 1], [1.0, 0.5]), prb(KIND_V, [node(shape, 7, 9, 4), shared], [1, 1], [-1.0, 2.0]),   # 8, 9 share a cell
               prb(KIND_V, s_idx[:1], [2], [1.0]),                                       # 10: on the source edge itself
               # 11, 12: the first and the last node (dead edges behind the layers: they read 0) and one live cell
               prb(KIND_V, node(shape, [0, 9, nx - 1], [0, 9, ny - 1], [0, 5, nz - 1]), [0, 1, 2], [1.0, 0.5, 1.0]),
               prb(KIND_I, node(shape, [0, 9, nx - 1], [0, 9, ny - 1], [0, 5, nz - 1]), [1, 2, 0], [1.0, 0.5, -1.0])]
    while len(probes) < MAX_PROBES:
        probes.append(cells(int(rng.integers(1, 5 if reduced else 13)), int(rng.integers(0, 2))))
    big = [] if reduced else [255, 256, 257, 600]
    case = Case("D5r" if reduced else "D5", shape, ("CPML",) * 6, 3, signal(), sources, probes, (60,), seed=3,
                env={} if reduced else {"FDTD_TYS": "1"},
                expect={"nprobes": 64, "fusable": True, "res_possible": reduced, **({} if reduced else {
                    "tys": 1, "strip_planes": 288, "blocks_per_strip_plane": 1, "owner_blocks_max": 288, "probe_cells_max": 600})})
    assert len(probes) == MAX_PROBES and all(n in [p[1].size for p in probes] for n in big)
    if reduced:
        runs = [("RESIDENT", "resident"), ("AUTO", "resident")]
    else:
        runs = [("DIRECT", "two"), ("WF1", "one"), ("WFM", "one"),
                ("RESIDENT", "refused: resident schedule: at most 256 probe cells per tile", {"FDTD_TYS": None})]
    _add(case, runs)


_d5(False)
_d5(True)


def _d6():
    """The D5 grid, eight probes, calls of 1, 7, 61 and 30 timesteps with series of 94 entries (the last five timesteps are not
    recorded); after the second call 40 more source edges and a ninth probe."""
    shape = D5_SHAPE
    rng = np.random.default_rng(6000)

    def some(n, kind):
        i, j, k = rng.integers(1, 19, n), rng.integers(1, 23, n), rng.integers(1, 11, n)
        return prb(kind, node(shape, i, j, k), rng.integers(0, 3, n), _weights(rng, n))
    probes = [some(n, q % 2) for q, n in enumerate([1, 3, 9, 17, 40, 64, 5, 2])]
    sources = [src(node(shape, [10, 10], [12, 13], [6, 6]), [2, 2], [1.0, -0.5], [0, 2])]
    i, j = np.meshgrid(np.arange(4, 14), np.arange(9, 13), indexing="ij")
    more = src(node(shape, i.ravel(), j.ravel(), 5), rng.integers(0, 3, 40), _amps(rng, 40), rng.integers(-3, 41, 40))
    case = Case("D6", shape, ("CPML",) * 6, 3, signal(), sources, probes, (1, 7, 61, 30), max_steps=94, seed=4,
                later=[(2, "source", more), (2, "probe", some(33, KIND_V)), (2, "probe", some(21, KIND_I))],
                expect={"fusable": True, "res_possible": True, "nprobes": 10})
    _add(case, [("DIRECT", "two"), ("WF1", "one"), ("WFM", "one"), ("RESIDENT", "resident"), ("AUTO", "resident")])


_d6()


def _d7():
    """40 x 24 x 16, CPML-3, to be cut between planes 7 and 8: a z-directed source line, an I-probe loop round it in planes 7 and 8 and a
    V-probe along it, all on both sides of the cut."""
    shape = (40, 24, 16)
    rng = np.random.default_rng(7000)
    kz = np.arange(5, 11)
    line = src(node(shape, 20, 12, kz), [2] * 6, _amps(rng, 6), [0, 1, 0, 2, -1, 0])
    li, lj = np.array([20, 19, 20, 20] * 2), np.array([12, 12, 12, 11] * 2)      # Iy right / left of the edge (20, 12), Ix above / below it
    loop = prb(KIND_I, node(shape, li, lj, [7] * 4 + [8] * 4), [1, 1, 0, 0] * 2, [1, -1, -1, 1] * 2)
    vline = prb(KIND_V, node(shape, 20, 12, np.arange(6, 10)), [2] * 4, [-1.0] * 4)
    case = Case("D7", shape, ("CPML",) * 6, 3, signal(), [line], [vline, loop], (1, 59), expect={"fusable": True}, keep_frames=True)
    DIRECTED[case.name] = case       # (its runs are the slab tests')


_d7()


# ---- the directed slab cases: D7's grid (40 x 24 x 16), cut at and around planes 7 | 8 ------------------------------------------------
SLAB_SHAPE = (40, 24, 16)
CUT_2 = ((0, 8), (8, 8))
CUT_3 = ((0, 7), (7, 2), (9, 7))              # a two-plane slab: both of its planes wait for a halo
CUT_4 = ((0, 6), (6, 2), (8, 2), (10, 6))
SLAB_RUNS = []     # (case name, cuts, transport, "ok" | "refused: <the library's text>")


def _slab_runs(name, cuts, transports=TRANSPORTS):
    for c in cuts:
        for t in transports:
            SLAB_RUNS.append((name, c, t, "ok"))


def _inner_edges(planes, rows):
    """Every edge (c, k, j, i) of the rows and planes, three cells off the x faces."""
    return np.array([(c, k, j, i) for k in planes for c in range(3) for j in rows for i in range(3, 37)])


def _s1():
    """S1 (and S2: the same lists on thinner slabs): strips of 4 rows; 200 distinct source edges of all three components in rows 8..11
    of plane 8 and 200 in plane 7 (one strip-plane each: the dense LDS image on both sides of the cut 7 | 8), a few of them never
    firing; a V-probe and an I-probe of 300 cells over planes 6..9; a V-probe of 280 cells wholly in plane 8 (the bottom plane of the
    slab above the cut: every cell waits for the H halo) and an I-probe of 270 cells wholly in plane 7 (the top plane of the slab below:
    every cell waits for the E halo), both longer than one block; an I-probe wholly in planes 2..4, of which the upper slabs own
    nothing.  Seeded fields, so that the halo of the initial fields counts."""
    shape = SLAB_SHAPE
    rng = np.random.default_rng(8100)
    sources = []
    for plane in (8, 7):
        e = _inner_edges([plane], range(8, 12))
        c, k, j, i = e[rng.permutation(len(e))[:200]].T
        delay = rng.integers(-3, 41, 200)
        delay[[3, 77, 150]] = [500, 81, 300]        # never fire in the 80 timesteps
        sources.append(src(node(shape, i, j, k), c, _amps(rng, 200), delay))

    def cells(kind, n, planes, rows=range(2, 22)):
        e = _inner_edges(planes, rows)
        c, k, j, i = e[rng.permutation(len(e))[:n]].T
        return prb(kind, node(shape, i, j, k), c, _weights(rng, n))
    probes = [cells(KIND_V, 300, range(6, 10)), cells(KIND_I, 300, range(6, 10)), cells(KIND_V, 280, [8]), cells(KIND_I, 270, [7]),
              cells(KIND_I, 20, range(2, 5))]
    case = Case("S1", shape, ("CPML",) * 6, 3, signal(), sources, probes, (1, 79), seed=11, env={"FDTD_TYS": "4"}, keep_frames=True,
                expect={"tys": 4, "sp_max": 200, "dup": False, "path": "dense", "fusable": True, "blocks_per_strip_plane": 1,
                        "probe_cells_max": 300, "nprobes": 5})
    DIRECTED[case.name] = case
    _slab_runs("S1", [CUT_2, CUT_3, CUT_4])       # (CUT_3, CUT_4: the issue's S2)


_s1()


def _s3():
    """S3: D6's pattern on this grid.  Calls of 1, 7, 40 and 12 timesteps with series of 55 entries (the last five timesteps are not
    recorded); after the second call 40 more source entries on planes 7 and 8 — one edge of plane 8 listed twice, with another amplitude
    and delay (src_dense_ok = 0, the chain of k_post) — and two more probes on planes 7 and 8."""
    shape = SLAB_SHAPE
    rng = np.random.default_rng(8300)

    def some(n, kind, klo=1, khi=15):
        i, j, k = rng.integers(3, 37, n), rng.integers(1, 23, n), rng.integers(klo, khi, n)
        return prb(kind, node(shape, i, j, k), rng.integers(0, 3, n), _weights(rng, n))
    probes = [some(n, q % 2) for q, n in enumerate([1, 3, 9, 17, 40, 64])] + [some(12, KIND_V, 7, 9), some(12, KIND_I, 7, 9)]
    sources = [src(node(shape, [20, 20, 21, 21], [12, 13, 12, 13], [7, 7, 8, 8]), [2, 2, 1, 0], [1.0, -0.5, 0.7, -0.9], [0, 2, 1, -1])]
    e = _inner_edges([7, 8], range(9, 13))
    c, k, j, i = e[rng.permutation(len(e))[:39]].T
    idx, amp, delay = node(shape, i, j, k), _amps(rng, 39), rng.integers(-3, 41, 39)
    at = int(np.flatnonzero(k == 8)[2])           # this edge again, right behind its first entry
    idx, c = np.insert(idx, at + 1, idx[at]), np.insert(c, at + 1, c[at])
    amp, delay = np.insert(amp, at + 1, np.float32(-0.75) * amp[at] + np.float32(0.3)), np.insert(delay, at + 1, delay[at] + 2)
    more = src(idx, c, amp, delay)
    case = Case("S3", shape, ("CPML",) * 6, 3, signal(), sources, probes, (1, 7, 40, 12), max_steps=55, seed=4, keep_frames=True,
                later=[(2, "source", more), (2, "probe", some(33, KIND_V, 7, 9)), (2, "probe", some(21, KIND_I, 7, 9))],
                expect={"dup": True, "path": "scan", "fusable": True, "nprobes": 10})
    DIRECTED[case.name] = case
    _slab_runs("S3", [CUT_2, CUT_3])


_s3()


def _s4(zkind):
    """S4: Mur faces on x and y, the z faces CPML or Mur.  One source edge next to the x-low face in plane 8 and more well inside, in
    planes 7 and 8: the post, apply and source passes are launches of their own; a V-probe with cells ON the x-low node plane (the
    tangential edges the apply pass writes) in planes 7 and 8, and an I-probe round them.  Linked contexts and half-steps only: the mailbox
    transport takes no Mur face."""
    shape = SLAB_SHAPE
    rng = np.random.default_rng(8400)
    sources = [src(node(shape, [1, 20, 20, 21], [12, 12, 13, 12], [8, 8, 7, 7]), [2, 2, 1, 0], [1.0, -0.8, 0.6, 0.9], [0, 1, -2, 3])]
    jj = np.array([5, 9, 12, 12, 16, 20])
    on_face = prb(KIND_V, node(shape, 0, np.concatenate([jj, jj]), [7] * 6 + [8] * 6), [1, 2] * 6, _weights(rng, 12))
    near = prb(KIND_I, node(shape, [0, 1] * 6, np.concatenate([jj, jj]), [7] * 6 + [8] * 6), [2, 1] * 6, _weights(rng, 12))
    inner = prb(KIND_V, node(shape, 20, 12, np.arange(5, 11)), [2] * 6, [-1.0] * 6)
    kinds = ("MUR",) * 4 + (zkind,) * 2
    case = Case(f"S4-z{zkind.lower()}", shape, kinds, 3 if zkind == "CPML" else 0, signal(), sources, [on_face, near, inner], (1, 69), seed=6, scene=21,
                keep_frames=True, expect={"near_mur": True, "fusable": False})
    DIRECTED[case.name] = case
    _slab_runs(case.name, [CUT_2, CUT_3, CUT_4], ("linked-split", "linked-nosplit", "half-steps"))
    SLAB_RUNS.append((case.name, CUT_2, "p2p-two", "refused: fdtd_run_linked: every context must use the p2p transport (no Mur)"))


_s4("CPML")
_s4("MUR")
_slab_runs("D7", [CUT_2])


# ---- E-type field excitations and probes.py lists on the slabs: hard edges (Case.hard) on and next to the cut planes -------------------
HARD_CASES = ("H1-line", "H2-plate", "H2-plate-mur")
HARD_PLANES = {"H1-line": (6, 7, 8, 9), "H2-plate": (7, 8, 9), "H2-plate-mur": (7, 8, 9)}      # the planes each case claims for its hard edges


def _grid_of(case):
    from opbuild_cases import random_scene
    return random_scene(case.scene, case.shape, False, 3, n_lumped=0, pec_frac=0.0)[0]


def _h1():
    """H1: a z-directed hard E line at (20, 12) over the planes 6 ... 9 — for every cut k0 in 7, 8, 9 an edge on plane k0 - 1 (the top
    plane of the rank below: its H update reads the E halo) and one on k0 —, one delay per edge; a V-probe on every hard edge, an I-probe
    on the faces round the line and a V-probe through it, both over planes 5 ... 10."""
    shape = SLAB_SHAPE
    rng = np.random.default_rng(8500)
    ks = np.array(HARD_PLANES["H1-line"])
    hard = src(node(shape, 20, 12, ks), [2] * 4, [1.0, -0.8, 0.6, 0.9], [0, 3, 1, 25])
    on = [prb(KIND_V, [g], [2], [1.0]) for g in hard[0]]
    kk = np.arange(5, 11)
    ring = prb(KIND_I, node(shape, np.tile([19, 20], 6), np.repeat(12, 12), np.repeat(kk, 2)), [1] * 12, _weights(rng, 12))
    through = prb(KIND_V, node(shape, 20, 12, kk), [2] * 6, _weights(rng, 6))
    case = Case("H1-line", shape, ("CPML",) * 6, 3, signal(), [], on + [ring, through], (1, 7, 72), seed=13, keep_frames=True, hard=hard,
                expect={"fusable": True})
    DIRECTED[case.name] = case
    _slab_runs(case.name, [CUT_2, CUT_3])


def _h2(mur):
    """H2: hard E plates of x and y edges IN the planes 7, 8 and 9 (i 18 ... 22, j 10 ... 14): the cut plane k0 belongs to the rank above,
    the rank below reads its voltages as a halo; 40 edges per plane, more than the 32 a strip-plane scans (the dense image), 24 of
    them in rows 12 ... 14.  A V-probe on six of them, an I-probe and a V-probe over planes 6 ... 10 around the plates.  With Mur faces on
    x and y: linked contexts and half-steps, and the mailbox's refusal."""
    shape = SLAB_SHAPE
    rng = np.random.default_rng(8600)
    ex = [(0, k, j, i) for k in HARD_PLANES["H2-plate"] for j in range(10, 15) for i in range(18, 22)]
    ey = [(1, k, j, i) for k in HARD_PLANES["H2-plate"] for j in range(10, 14) for i in range(18, 23)]
    c, k, j, i = np.array(ex + ey).T
    amp = (0.5 + 0.1 * (i - 18) - 0.07 * (j - 10)) * np.where(c == 0, 1.0, -1.0)
    hard = src(node(shape, i, j, k), c, amp, np.where(k == 8, 2, k - 7))
    pick = [0, 21, 47, 60, 88, 119]
    on = [prb(KIND_V, [hard[0][q]], [hard[1][q]], [1.0]) for q in pick]
    n = 60
    pi, pj, pk = rng.integers(16, 25, n), rng.integers(8, 17, n), rng.integers(6, 11, n)
    around_i = prb(KIND_I, node(shape, pi, pj, pk), rng.integers(0, 3, n), _weights(rng, n))
    around_v = prb(KIND_V, node(shape, pi[::-1], pj, pk), rng.integers(0, 3, n), _weights(rng, n))
    kinds = ("MUR",) * 4 + ("CPML",) * 2 if mur else ("CPML",) * 6
    case = Case("H2-plate-mur" if mur else "H2-plate", shape, kinds, 3, signal(), [], on + [around_i, around_v], (1, 7, 72), seed=14,
                scene=21 if mur else 5, keep_frames=True, hard=hard, expect={"fusable": True, "path": "dense"})
    DIRECTED[case.name] = case
    if mur:
        _slab_runs(case.name, [CUT_2, CUT_3], ("linked-split", "linked-nosplit", "half-steps"))
        SLAB_RUNS.append((case.name, CUT_2, "p2p-two", "refused: fdtd_run_linked: every context must use the p2p transport (no Mur)"))
    else:
        _slab_runs(case.name, [CUT_2, CUT_3])


def _h3():
    """H3: a soft E list as a weighted, delayed field excitation makes it — three delays, graded amplitudes, z edges over planes 5 ... 10
    and x edges in planes 7, 8, 9, one edge listed twice — spanning both (all three) slabs; and the four list kinds of probes.py, built
    by probes.lists itself for boxes that straddle the cuts: a voltage line from plane 5 to plane 11, a current loop with normal x
    over planes 6 ... 10, E-field and H-field point probes at nodes of the planes 7 and 8 (a point has one node: one on either side of
    the cut 7 | 8, and the z edge of the one on plane 7 ends on plane 8)."""
    probes_mod = pkg("probes")
    shape = SLAB_SHAPE
    kk = np.repeat(np.arange(5, 11), 3)
    ii = np.tile([14, 15, 16], 6)
    z_idx, z_amp, z_delay = node(shape, ii, 9, kk), 0.2 + 0.1 * (kk - 5) - 0.05 * (ii - 14), np.tile([0, 4, 9], 6)
    xk = np.repeat([7, 8, 9], 4)
    xi = np.tile([13, 14, 15, 16], 3)
    x_idx, x_amp, x_delay = node(shape, xi, 10, xk), -0.3 + 0.08 * (xi - 13) + 0.05 * (xk - 7), np.repeat([9, 0, 4], 4)
    idx = np.concatenate([z_idx, x_idx, z_idx[[10]]])
    comp = np.concatenate([np.full(18, 2), np.full(12, 0), [2]])
    soft = src(idx, comp, np.concatenate([z_amp, x_amp, [-0.45]]), np.concatenate([z_delay, x_delay, [4]]))
    case = Case("H3-soft-and-probes", shape, ("CPML",) * 6, 3, signal(), [soft], [], (1, 7, 72), seed=15, keep_frames=True,
                expect={"fusable": True, "dup": True})
    g = _grid_of(case)
    pec = np.zeros((3, shape[2], shape[1], shape[0]), bool)
    at = lambda i, j, k: (float(g.x[i]), float(g.y[j]), float(g.z[k]))
    mid = lambda a, q: 0.5 * float(g.lines[a][q] + g.lines[a][q + 1])
    specs = []
    for name, t, start, stop, nd in (("ut", 0, at(15, 9, 5), at(15, 9, 11), None),
                                     ("it", 1, (mid(0, 15), float(g.y[8]), float(g.z[6])), (mid(0, 15), float(g.y[11]), float(g.z[10])), 0),
                                     ("et7", 2, at(15, 10, 7), at(15, 10, 7), None), ("et8", 2, at(15, 10, 8), at(15, 10, 8), None),
                                     ("ht7", 3, at(16, 11, 7), at(16, 11, 7), None), ("ht8", 3, at(16, 11, 8), at(16, 11, 8), None)):
        sp = probes_mod.make(name, t, norm_dir=nd)
        sp.start, sp.stop = start, stop
        specs.append(sp)
    case.probe_names = []
    for sp in specs:
        pl = probes_mod.lists(g, pec, sp, 1.0, 1e-9)
        for q in pl.lists:
            case.probes.append(prb(pl.kind, q.idx, q.comp, q.w))
            case.probe_names.append(sp.name)
    DIRECTED[case.name] = case
    _slab_runs(case.name, [CUT_2, CUT_3])


def _h4():
    """H4 (single slab): D2-tys8's grid, 130 x 17 x 10 with strips of 8 rows — 40 hard x and z edges in row 15 of plane 5 (threads
    231 ... 263 of the strip-plane: two blocks), 20 of them at i >= 100, in the second block; a V-probe on six of them."""
    shape = (130, 17, 10)
    rng = np.random.default_rng(8700)
    i = np.concatenate([rng.choice(np.arange(2, 100), 20, replace=False), rng.choice(np.arange(100, 128), 20, replace=False)])
    comp = rng.integers(0, 2, 40) * 2
    hard = src(node(shape, i, 15, 5), comp, _amps(rng, 40), rng.integers(0, 12, 40))
    on = [prb(KIND_V, [hard[0][q]], [hard[1][q]], [1.0]) for q in (0, 7, 19, 20, 31, 39)]
    around = prb(KIND_I, node(shape, np.arange(97, 109), 14, 5), [0] * 12, _weights(rng, 12))
    case = Case("H4-second-block", shape, ("PEC",) * 6, 0, signal(), [], on + [around], (1, 7, 52), seed=16, hard=hard, env={"FDTD_TYS": "8"},
                expect={"tys": 8, "sp_max": 40, "dup": False, "path": "dense", "fusable": True, "blocks_per_strip_plane": 2, "src_blocks": [0, 1]})
    _add(case, [("DIRECT", "two"), ("WF1", "one"), ("RESIDENT", "resident")])


_h1()
_h2(False)
_h2(True)
_h3()
_h4()
# the slab cases once on ONE slab under the resident, the one-launch and the two-launch schedule
for _name in ("H1-line", "H2-plate", "H3-soft-and-probes"):
    for _sched, _outcome in (("RESIDENT", "resident"), ("WF1", "one"), ("DIRECT", "two")):
        RUNS.append((_name, _sched, _outcome, {}))
HARD_CASES = HARD_CASES + ("H4-second-block",)
HARD_PLANES["H4-second-block"] = (5,)


def hard_table(case, q):
    """What hard edge q holds, per recorded timestep: float32(amp * sig[n - delay]) inside the table, 0.0 outside."""
    idx, comp, amp, delay = case.hard
    n = np.arange(min(case.nsteps, case.cap)) - int(delay[q])
    inside = (n >= 0) & (n < len(case.signal))
    s = np.where(inside, case.signal.astype(np.float32)[np.clip(n, 0, len(case.signal) - 1)], np.float32(0.0)).astype(np.float32)
    return (amp[q] * s).astype(np.float64)
SLAB_CASES = sorted({r[0] for r in SLAB_RUNS})


def slab_facts(case, cuts):
    """Where the lists of a case sit on the slabs `cuts`: per rank the source entries of its fullest strip-plane and whether that
    strip-plane takes the dense path on the rank, per rank and probe the cells it owns, and of those the ones in its bottom plane (V: they
    wait for the H halo from below) and in its top plane (I: they wait for the E halo from above)."""
    nx, ny, _ = case.shape
    tys = tys_of(case)
    nstrips = -(-ny // tys)
    out = []
    for r, (k0, nk) in enumerate(cuts):
        sidx = np.concatenate([s[0] for _, s in case.all_sources()])
        scomp = np.concatenate([s[1] for _, s in case.all_sources()]).astype(np.int64)
        own = in_planes(case, sidx, (k0, nk))
        sidx, scomp = sidx[own], scomp[own]
        k, j, _ = _kji(case, sidx)
        sp = np.bincount((k - k0) * nstrips + j // tys, minlength=nk * nstrips)
        dup = np.unique(sidx * 4 + scomp).size < sidx.size
        cells, bottom, top = [], [], []
        for _, p in case.all_probes():
            pk = _kji(case, clip_to_planes(case, p, (k0, nk))[1])[0]
            cells.append(int(pk.size))
            bottom.append(int(np.sum(pk == k0)) if (p[0] == KIND_V and r > 0) else 0)
            top.append(int(np.sum(pk == k0 + nk - 1)) if (p[0] == KIND_I and r + 1 < len(cuts)) else 0)
        out.append({"sp_max": int(sp.max()) if sidx.size else 0, "dense": bool(sidx.size and sp.max() > SRC_SCAN_MAX and not dup), "dup": bool(dup),
                    "sp": sp.reshape(nk, nstrips), "cells": cells, "halo_cells_V": bottom, "halo_cells_I": top})
    return out


# ---- the randomised batch -------------------------------------------------------------------------------------------------------------
def draw(rng):
    """One case of the randomised batch and the flag it runs under ('AUTO' | 'DIRECT')."""
    nx = min(max(int(4 * rng.integers(2, 18) + rng.integers(0, 4)), 10), 70)      # 4m, 4m + 1, 4m + 2, 4m + 3
    ny, nz = int(rng.integers(8, 41)), int(rng.integers(6, 21))
    shape = (nx, ny, nz)
    u = rng.random()
    if u < 0.45:       # one kind all round (else nearly every case would have a Mur face and a CPML layer)
        boundary = (["PEC", "MUR", "CPML", "CPML"][int(rng.integers(0, 4))],) * 6
    else:
        boundary = tuple(["PEC", "MUR", "CPML"][int(v)] for v in rng.integers(0, 3, 6))
    cpml = min(int(rng.integers(2, 4)), (min(shape) - 2) // 2)       # (both layers of an axis fit the grid)
    lim = [(0, nx - 1), (0, ny - 1), (0, nz - 1)]

    def box_points(n, touch):
        lo, hi = [], []
        for a in range(3):
            w = int(rng.integers(2, max(3, lim[a][1] // 2 + 1)))
            s = int(rng.integers(2, max(3, lim[a][1] - w - 1)))
            lo.append(s), hi.append(min(s + w, lim[a][1] - 2))
        if touch:
            a = int(rng.integers(0, 3))
            if rng.random() < 0.5:
                lo[a] = 0
            else:
                hi[a] = lim[a][1]
        return [rng.integers(lo[a], max(hi[a], lo[a]) + 1, n) for a in range(3)]

    def edges(n, touch, clustered):
        i, j, k = box_points(n, touch) if clustered else [rng.integers(2, lim[a][1] - 1, n) for a in range(3)]
        comp = rng.integers(0, 3, n)
        pos = np.stack([i, j, k])
        for c in range(3):      # existing edges only
            sel = (comp == c) & (pos[c] >= lim[c][1])
            pos[c][sel] = lim[c][1] - 1
        return node(shape, *pos), comp

    sources, seen = [], set()
    repeat = rng.random() < 0.3                      # some edges twice, within a call or across calls
    for _ in range(int(rng.integers(1, 5))):
        n = int(rng.integers(1, 301)) if rng.random() < 0.5 else int(rng.integers(1, 40))
        idx, comp = edges(n, rng.random() < 0.3, rng.random() < 0.6)
        keep = []
        for q, key in enumerate((idx * 4 + comp).tolist()):
            if key not in seen:
                seen.add(key), keep.append(q)
        if not keep:
            keep = [0]
        idx, comp = idx[keep], comp[keep]
        if repeat:
            pool = np.array(sorted(seen))
            pick = pool[rng.integers(0, pool.size, int(rng.integers(1, 4)))]
            idx, comp = np.concatenate([idx, pick // 4]), np.concatenate([comp, pick % 4])
        sources.append(src(idx, comp, _amps(rng, idx.size), rng.integers(-3, 41, idx.size)))
    probes = []
    for _ in range(int(rng.integers(1, 9))):
        n = int(rng.integers(1, 401)) if rng.random() < 0.4 else int(rng.integers(1, 30))
        idx, comp = edges(n, rng.random() < 0.2, rng.random() < 0.5)
        probes.append(prb(int(rng.integers(0, 2)), idx, comp, _weights(rng, n)))
    ncalls = int(rng.integers(1, 6))
    calls = tuple(int(v) for v in rng.integers(1, 30, ncalls))
    calls = calls[:-1] + (calls[-1] + max(0, 45 - sum(calls)),)
    env = {}
    tys = [None, 1, 2, 3, 5, 9][int(rng.integers(0, 6))]
    if tys:
        env["FDTD_TYS"] = str(tys)
    wfm = [None, 1, 3][int(rng.integers(0, 3))]
    if wfm:
        env["FDTD_WF_MULTI"] = str(wfm)
    if rng.random() < 0.5:
        env["FDTD_RESIDENT"] = "0"
    flag = "DIRECT" if rng.random() < 0.2 else "AUTO"
    case = Case("random", shape, boundary, cpml, signal(), sources, probes, calls, seed=int(rng.integers(0, 100)) if rng.random() < 0.5 else None,
                scene=int(rng.integers(0, 50)), env=env)
    return case, flag


def drawn(n):
    case, flag = draw(np.random.default_rng(20261019 + n))
    case.name = f"case-{n:02d}"
    return case, flag


N_DRAWN = 24

# ---- the randomised slab batch --------------------------------------------------------------------------------------------------------
N_SLAB_DRAWN = 16
SLAB_SEED = 20268420      # (the first of 20261020, 20261120, ... whose batch meets every floor of test_drawn_slab_batch_covers_what_it_claims)


def draw_slabs(rng):
    """(case, cuts, transport): a case of draw() with at least 8 planes, cut into 2..4 slabs of at least 2 planes — every cut with
    probability 1/2 placed ON a plane that holds a source or probe cell (that plane becomes the bottom plane of the slab above the cut or
    the top plane of the slab below it) — and the transport it runs under, drawn first: a mailbox transport takes the next case without a
    Mur face (and without more than 256 entries with a repeated edge in one strip-plane: it refuses both), so a case with Mur faces runs
    on linked contexts or half-steps."""
    transport = TRANSPORTS[int(rng.integers(0, len(TRANSPORTS)))]
    while True:
        case, _ = draw(rng)
        if case.shape[2] >= 8 and not (transport.startswith("p2p") and ("MUR" in case.boundary or regimes(case)["path"] == "post")):
            break
    nz = case.shape[2]
    nodes = np.concatenate([s[0] for _, s in case.all_sources()] + [p[1] for _, p in case.all_probes()])
    held = np.unique(nodes // (case.shape[0] * case.shape[1]))
    while True:
        world = int(rng.integers(2, 5))
        first = []                 # the first plane of every slab but the lowest
        for _ in range(world - 1):
            if rng.random() < 0.5:
                first.append(int(rng.choice(held)) + int(rng.integers(0, 2)))
            else:
                first.append(int(rng.integers(2, nz - 1)))
        b = [0] + sorted(first) + [nz]
        if all(hi - lo >= 2 for lo, hi in zip(b[:-1], b[1:])):
            break
    cuts = tuple((lo, hi - lo) for lo, hi in zip(b[:-1], b[1:]))
    case.keep_frames = True
    return case, cuts, transport


def drawn_slabs(n):
    case, cuts, transport = draw_slabs(np.random.default_rng(SLAB_SEED + n))
    case.name = f"slabs-{n:02d}"
    return case, cuts, transport


def slab_batch_coverage():
    """What the drawn slab batch reaches, by the arithmetic of slab_facts: the floors tests/test_sources_probes_cpu.py asserts."""
    tally = {"transports": {t: 0 for t in TRANSPORTS}, "two_plane_slabs": 0, "probes_across_a_cut": 0, "rank_probe_pairs_without_cells": 0,
             "slabs_with_a_dense_strip_plane": 0, "mur_cases": 0, "cuts_on_a_held_plane": 0, "cuts": 0}
    for n in range(N_SLAB_DRAWN):
        case, cuts, transport = drawn_slabs(n)
        facts = slab_facts(case, cuts)
        tally["transports"][transport] += 1
        tally["two_plane_slabs"] += sum(nk == 2 for _, nk in cuts)
        tally["mur_cases"] += "MUR" in case.boundary
        tally["slabs_with_a_dense_strip_plane"] += sum(f["dense"] for f in facts)
        for q in range(len(case.all_probes())):
            owners = sum(f["cells"][q] > 0 for f in facts)
            tally["probes_across_a_cut"] += owners >= 2
            tally["rank_probe_pairs_without_cells"] += len(cuts) - owners
        nodes = np.concatenate([s[0] for _, s in case.all_sources()] + [p[1] for _, p in case.all_probes()])
        held = set((nodes // (case.shape[0] * case.shape[1])).tolist())
        for k0, _ in cuts[1:]:
            tally["cuts"] += 1
            tally["cuts_on_a_held_plane"] += (k0 in held) or (k0 - 1 in held)
    return tally
