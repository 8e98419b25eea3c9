"""Child process of test_wait_sets_gpu.py: loads the DIAGNOSTIC build of the library (csrc/_diag, make diag), steps each case twice under
the one-launch schedule and leaves what the device holds in an .npz: the wait sets of every (k, strip, pb, lane) as the device computes
them (fdtd_debug_wait_sets) and the probe tables (fdtd_debug_probe_waits).  One fresh process, so that the product library and the
diagnostic one never share one.

    python tests/wait_sets_diag_child.py OUT.npz
    python tests/wait_sets_diag_child.py delay CASE OUT.json      (the delayed-block runs of one case: delay_runs below)
"""
import ctypes
import os
import sys

import numpy as np

# (name, shape, $FDTD_TYS or None, Mur faces or None, probes: list of (kind, number of cells))
CASES = (
    ("37x300x10_tys4", (37, 300, 10), 4, None, ()),
    ("53x47x31_tys5_probes", (53, 47, 31), 5, None, ((0, 1), (1, 257), (0, 600), (1, 1))),
    ("1028x9x9", (1028, 9, 9), None, None, ((1, 257),)),
    ("1100x24x16", (1100, 24, 16), None, None, ()),
    ("2050x7x6", (2050, 7, 6), None, None, ()),
    ("7700x6x5", (7700, 6, 5), None, None, ()),
    ("30716x5x5", (30716, 5, 5), None, None, ()),
    ("143x129x20_mur_all", (143, 129, 20), None, (1, 1, 1, 1, 1, 1), ()),
    ("143x129x20_mur_y", (143, 129, 20), None, (0, 0, 1, 1, 0, 0), ()),
    ("143x129x20_mur_z", (143, 129, 20), None, (0, 0, 0, 0, 1, 1), ()),
    ("141x129x20_mur_all_x0mod4", (141, 129, 20), None, (1, 1, 1, 1, 1, 1), ()),
    ("142x129x20_mur_all_x1mod4", (142, 129, 20), None, (1, 1, 1, 1, 1, 1), ()),
)


def probe_cells(shape, n, seed):
    """n distinct (global flat node index, component) pairs spread over the grid"""
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.choice(int(np.prod(shape)), size=n, replace=False)).astype(np.int64)
    return idx, rng.integers(0, 3, n).astype(np.int8)


def build_engine(lib, shape, tys, faces, probes, seed=3, wavefront=True):
    from conftest import pkg
    from helpers import seeded_fields
    from opbuild_cases import random_scene
    capi, const, eco = pkg("_capi"), pkg("constants"), pkg("ecoperator")
    for k, v in (("FDTD_RESIDENT", "0"), ("FDTD_TYS", None if tys is None else str(tys))):
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    grid, eps, kap, pec, _ = random_scene(seed, shape, False, 3, n_lumped=0, pec_frac=0.0)
    dt = grid.courant_dt()
    e = capi.Engine(lib, *shape, dt, max_steps=16, flags=capi.FLAG_KERNEL_WAVEFRONT if wavefront else 0)
    emet, hmet = eco.pack_metric_tables(*eco.metric_lists(grid, dt), grid)
    e.build_operator(grid.d, eps, kap, pec, const.EPS0, eco.lumped_overrides(grid, eps, kap, pec, dt, []), emet, hmet)
    if faces is not None:
        coeff = []
        for f in range(6):
            l = grid.lines[f // 2]
            d = (l[-1] - l[-2]) if f % 2 else (l[1] - l[0])
            coeff.append((const.C0 * dt - d) / (const.C0 * dt + d))
        e.set_mur(faces, coeff)
    e.set_signal(np.zeros(4))
    pids = []
    for q, (kind, n) in enumerate(probes):
        idx, comp = probe_cells(shape, n, 100 + q)
        pids.append(e.add_probe(kind, idx, comp, np.ones(n, np.float32)))
    seeded_fields(e, 17)
    return e, pids


def main(out_path):
    from conftest import ROOT, pkg
    capi = pkg("_capi")
    lib = capi.load_hip_library(os.path.join(ROOT, "fdtd-solver-antennas_amd", "csrc", "_diag"))
    I, P = ctypes.c_int, ctypes.c_void_p
    lib.fdtd_debug_wait_sets.restype, lib.fdtd_debug_wait_sets.argtypes = I, [P, P, P]
    lib.fdtd_debug_probe_waits.restype, lib.fdtd_debug_probe_waits.argtypes = I, [P, P, P, P, P, I]
    out = {}
    for name, shape, tys, faces, probes in CASES:
        e, _ = build_engine(lib, shape, tys, faces, probes)
        e.run(2)
        info = e.schedule_info()
        assert info["launches_per_timestep"] == 1 and not info["resident"], (name, info)
        geom = np.zeros(14, np.int32)
        assert lib.fdtd_debug_wait_sets(e._ctx, geom.ctypes.data, None) == 0, name
        n = int(geom[5]) * int(geom[3]) * int(geom[4]) * 256
        dump = np.full((5, n), -7, np.int64)
        assert lib.fdtd_debug_wait_sets(e._ctx, geom.ctypes.data, dump.ctypes.data) == 0, name
        out[name + "/geom"], out[name + "/dump"] = geom, dump
        if probes:
            nsp = int(geom[5]) * int(geom[3])
            sp, spV, rng, blk = np.full(nsp, -7, np.int32), np.full(nsp, -7, np.int32), np.full(128, -7, np.int32), np.full(1 << 16, -7, np.int32)
            nblk = lib.fdtd_debug_probe_waits(e._ctx, sp.ctypes.data, spV.ctypes.data, rng.ctypes.data, blk.ctypes.data, blk.size)
            assert nblk >= 0, (name, nblk)
            out[name + "/sp"], out[name + "/spV"], out[name + "/rng"], out[name + "/blk"] = sp, spV, rng, blk[:nblk]
        e.close()
        print(name, "geom", geom.tolist(), flush=True)
    np.savez_compressed(out_path, **out)


# ---- delayed-block runs --------------------------------------------------------------------------------------------------------------
STEPS = 6
SLOTS = 65536
# schedule -> ($FDTD_WF_LAG, $FDTD_WF_MULTI, timesteps per run() call)
SCHEDULES = {"lag1": ("1", "1", 1), "lag3": ("3", "1", 1), "all_E_then_all_H": (None, "1", 1), "several_timesteps_per_launch": (None, str(STEPS), STEPS)}
MASKS = tuple(f"seed{q}" for q in range(8)) + ("E_only", "H_only")


def block_hash(flag, is_h):
    """a fixed scramble of (block, E / H) to 0 .. 15"""
    h = (np.asarray(flag, np.uint64) * np.uint64(2654435761) + np.uint64(1013 if is_h else 0)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(13)
    return (h & np.uint64(15)).astype(np.int64)


def delay_mask(mask_name, nflags, h_steps):
    """[timestep & 7][E, H][flag] bits: block b spins in timestep s iff (hash(b) + seed + 8 * (s & 1)) % 16 == 0 — one block in 16 per timestep, and
    over the eight seeds and the two parities every block exactly once.  H blocks only in the timesteps h_steps (those in which a block of the same
    launch waits for them)."""
    seed = MASKS.index(mask_name)
    bits = np.zeros((8, 2, SLOTS), bool)
    flag = np.arange(nflags)
    for s in range(STEPS):
        for is_h in (0, 1):
            if (is_h and (mask_name == "E_only" or s not in h_steps)) or (not is_h and mask_name == "H_only"):
                continue
            bits[s & 7, is_h, :nflags] |= ((block_hash(flag, is_h) + seed + 8 * (s & 1)) & 15) == 0
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).ravel().copy()


def waiters_of(ws, geom):
    """From the host build of wait_sets.hpp: for every E flag the H blocks (flags) that poll it, for every H flag the E blocks of the next timestep"""
    from helpers import ws_geom
    P4, ny, tys, nstrips, nbs, nk = (int(v) for v in geom[:6])
    g = ws_geom(ws, P4, ny, tys, nk, [int(v) for v in geom[6:12]])
    nb = nk * nstrips * nbs
    dump = np.full((5, nb * 256), -7, np.int64)
    ws.ws_dump(g, dump.ctypes.data)
    d = dump.reshape(5, nb, 256)
    mur = any(int(v) >= 0 for v in geom[6:12])
    fwd, back = {}, {}
    for w in range(nb):
        polled = d[2, w] if (mur and d[3, w, 0]) else d[0, w]
        for f in polled[polled >= 0]:
            fwd.setdefault(int(f), []).append(w)
        for f in d[1, w][d[1, w] >= 0]:
            back.setdefault(int(f), []).append(w)
    return fwd, back


def delay_runs(case_name, out_path):
    import json
    from conftest import ROOT, pkg
    from helpers import load_wait_sets
    capi = pkg("_capi")
    name, shape, tys, faces, probes = next(c for c in CASES if c[0] == case_name)
    lib = capi.load_hip_library(os.path.join(ROOT, "fdtd-solver-antennas_amd", "csrc", "_diag"))
    ora = capi.bind(ctypes.CDLL(os.path.join(ROOT, "oracle", "libfdtd_oracle.so")))
    ws = load_wait_sets()
    I, P, U64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_ulonglong
    lib.fdtd_debug_wait_sets.restype, lib.fdtd_debug_wait_sets.argtypes = I, [P, P, P]
    lib.fdtd_debug_wf_delay.restype, lib.fdtd_debug_wf_delay.argtypes = I, [P, U64]
    lib.fdtd_debug_wf_stamps.restype, lib.fdtd_debug_wf_stamps.argtypes = I, [P, I, I]
    eo, pids = build_engine(ora, shape, tys, faces, probes, wavefront=False)
    eo.run(STEPS)
    ref_fields, ref_series = eo.fields(), [eo.get_probe(q)[:STEPS] for q in pids]
    assert np.abs(ref_fields).max() > 0
    report = {"case": name, "schedules": {}}
    for sched, (lag, multi, per_call) in SCHEDULES.items():
        if faces is not None and lag is not None:
            continue                                            # Mur faces inside the launch: all E blocks, then all H blocks
        for k, v in (("FDTD_WF_LAG", lag), ("FDTD_WF_MULTI", multi)):
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        h_steps = set(range(STEPS - 1)) if per_call == STEPS else set()
        rec = {"runs": {}}
        ticks, fwd, back = 0, None, None
        evidence = {}                                           # (E / H, flag) of every block delayed under this schedule -> a waiter waited for it at least once
        names = ["none"] + list(MASKS) + ["followup1", "followup2"]
        for mask_name in names:
            if mask_name == "H_only" and not h_steps:
                continue                                        # one timestep per launch: nothing in a launch waits for an H block
            # blocks that no waiter has waited for so far (their waiters were dispatched after they had ended — with one block in 16 late,
            # a timestep lasts about as long as the delay) are delayed once more, alone: a sparse mask, short timesteps
            left = sorted(b for b, ok in evidence.items() if not ok)
            if mask_name.startswith("followup") and not left:
                continue
            e, pids = build_engine(lib, shape, tys, faces, probes)
            geom = np.zeros(14, np.int32)
            assert lib.fdtd_debug_wait_sets(e._ctx, geom.ctypes.data, None) == 0
            nflags = int(geom[5]) * int(geom[3]) * int(geom[4])
            assert nflags <= SLOTS
            if mask_name.startswith("followup"):
                bits = np.zeros((8, 2, SLOTS), bool)
                for h, f in left:
                    for st_ in (sorted(h_steps) if h else range(STEPS)):
                        bits[st_ & 7, h, f] = True
                mask = np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).ravel().copy()
            else:
                mask = None if mask_name == "none" else delay_mask(mask_name, nflags, h_steps)
            assert lib.fdtd_debug_wf_delay(None if mask is None else mask.ctypes.data, ticks) == 0
            stamps = []
            for _ in range(STEPS // per_call):
                e.run(per_call)
                st = np.zeros((SLOTS, 6), np.uint64)
                assert lib.fdtd_debug_wf_stamps(st.ctypes.data, SLOTS, 1) == 0
                stamps.append(st[(st[:, 4] >> np.uint64(42)) & np.uint64(1) == 1].astype(np.int64))
            info = e.schedule_info()
            assert info["launches_per_timestep"] == 1 and not info["resident"], info
            st = np.concatenate(stamps)
            launch = np.concatenate([np.full(len(x), q) for q, x in enumerate(stamps)])
            flag, is_h, delayed, step = st[:, 4] & 0xffffffff, (st[:, 4] >> 40) & 1, (st[:, 4] >> 41) & 1, st[:, 5]
            assert sorted(set(step.tolist())) == list(range(STEPS)) and len(st) == 2 * nflags * STEPS, (sched, mask_name, len(st), nflags)
            fields_ok = bool(np.array_equal(e.fields(), ref_fields))
            series_ok = all(np.array_equal(e.get_probe(q)[:STEPS], r) for q, r in zip(pids, ref_series))
            run = {"fields_equal_oracle": fields_ok, "series_equal_oracle": series_ok, "delayed": int(delayed.sum())}
            if mask_name == "none":
                dur = st[:, 3] - st[:, 0]
                ticks = int(min(20 * int(np.median(dur)), 100000))
                rec["median_block_ticks"], rec["delay_ticks"], rec["lag_planes"] = int(np.median(dur)), ticks, info["lag_planes"]
                rec["blocks_per_sweep"] = nflags
                fwd, back = waiters_of(ws, geom)
                assert delayed.sum() == 0
            else:
                slot = {(int(s), int(h), int(f)): q for q, (s, h, f) in enumerate(zip(step, is_h, flag))}
                lacking = []
                for q in np.flatnonzero(delayed):
                    s, h, f, end = int(step[q]), int(is_h[q]), int(flag[q]), int(st[q, 3])
                    ws_ = [slot.get((s + 1, 0, w)) for w in back.get(f, [])] if h else [slot.get((s, 1, w)) for w in fwd.get(f, [])]
                    ws_ = [w for w in ws_ if w is not None and launch[w] == launch[q]]
                    ok = any(st[w, 1] and st[w, 1] < end < st[w, 2] for w in ws_)
                    evidence[(h, f)] = evidence.get((h, f), False) or ok
                    if not ok:
                        lacking.append([s, h, f, len(ws_)])
                    assert int(st[q, 3] - st[q, 0]) >= ticks
                run["delayed_instances_without_a_waiter_that_waited"] = lacking      # (timestep, E / H, flag, waiters in the launch)
                run["delayed_blocks"] = sorted({(int(h), int(f)) for h, f in zip(is_h[delayed == 1], flag[delayed == 1])})
            rec["runs"][mask_name] = run
            e.close()
            print(sched, mask_name, {k: v for k, v in run.items() if k != "delayed_blocks"}, flush=True)
        seen = set()
        for r in rec["runs"].values():
            seen |= {tuple(x) for x in r.pop("delayed_blocks", [])}
        nfl = rec["blocks_per_sweep"]
        rec["delayed_blocks_no_waiter_ever_waited_for"] = sorted(list(b) for b, ok in evidence.items() if not ok)
        rec["every_E_block_delayed_once"] = {f for h, f in seen if h == 0} == set(range(nfl))
        rec["every_H_block_delayed_once"] = ({f for h, f in seen if h == 1} == set(range(nfl))) if h_steps else None
        report["schedules"][sched] = rec
        print(sched, {k: v for k, v in rec.items() if k != "runs"}, flush=True)
    assert lib.fdtd_debug_wf_delay(None, 0) == 0
    with open(out_path, "w") as f:
        json.dump(report, f)


if __name__ == "__main__":
    if sys.argv[1] == "delay":
        delay_runs(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1])
