"""The wait sets of the one-launch schedule on the device: what the diagnostic build (make -C csrc diag) computes for every
(k, strip, pb, lane) of a context equals, as integers, what the host build of the same header computes — the host build is the one
test_wait_sets_cpu.py proves against the stencil — and the probe tables the device holds are exact: the owner list of a probe is the set
of blocks that own one of its cells by the thread decode, the marked strip-planes are those that hold a cell, nothing else.
The same build delays chosen blocks, so that a wait that is missing would show in the fields (the last test below).
The diagnostic library only ever runs in fresh child processes (wait_sets_diag_child.py), one at a time, which leave their results in files."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import load_wait_sets, ws_geom
from wait_sets_diag_child import CASES, probe_cells

pytestmark = pytest.mark.gpu
B = 256


@pytest.fixture(scope="module")
def device_tables(tmp_path_factory):
    diag = os.path.join(ROOT, "fdtd-solver-antennas_amd", "csrc", "_diag", "libfdtd_hip.so")
    assert os.path.isfile(diag), "the diagnostic build is missing: make -C fdtd-solver-antennas_amd/csrc diag (build() makes it)"
    out = str(tmp_path_factory.mktemp("wait_sets") / "device.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wait_sets_diag_child.py"), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_wait_sets_equal_the_host_build(device_tables, case):
    name, shape, tys, faces, _ = case
    ws = load_wait_sets()
    geom = device_tables[name + "/geom"]
    P4, ny, dtys, nstrips, nbs, nk = (int(v) for v in geom[:6])
    assert (P4, ny, nk, int(geom[12])) == ((shape[0] + 3) // 4, shape[1], shape[2], shape[0])
    if tys is not None:
        assert dtys == min(tys, ny)
    want_b = [-1] * 6 if faces is None else [(((shape[f // 2] - 1) if f % 2 else 0) if faces[f] else -1) for f in range(6)]
    assert geom[6:12].tolist() == want_b
    g = ws_geom(ws, P4, ny, dtys, nk, want_b)
    assert (g.nstrips, g.nbs) == (nstrips, nbs)
    host = np.full((5, nk * nstrips * nbs * B), -7, np.int64)
    ws.ws_dump(g, host.ctypes.data)
    dev = device_tables[name + "/dump"]
    assert dev.shape == host.shape
    for q, what in enumerate(("wf_wait_flag", "wf_wait_back_flag", "wf_wait_mur_flag", "wf_mur_wide", "decode_thread")):
        bad = np.flatnonzero(dev[q] != host[q])
        assert bad.size == 0, f"{what}: {bad.size} words differ, first at (block {bad[0] // B}, lane {bad[0] % B}): device {dev[q][bad[0]]}, host {host[q][bad[0]]}"
    if faces is not None:
        assert dev[3].any() and (9 * nbs <= B)      # the case reaches the wide set
        if faces[1] and (shape[0] - 1) % 4 == 0:
            assert dev[3].all()                      # upper x face on the first cell of a group: every block


@pytest.mark.parametrize("case", [c for c in CASES if c[4]], ids=[c[0] for c in CASES if c[4]])
def test_probe_owner_lists_and_strip_plane_maps_are_exact(device_tables, case):
    name, shape, _, _, probes = case
    nx, ny, nz = shape
    P4, _, tys, nstrips, nbs, nk = (int(v) for v in device_tables[name + "/geom"][:6])
    sp, spV, rng, blk = (device_tables[name + "/" + k] for k in ("sp", "spV", "rng", "blk"))
    dump = device_tables[name + "/dump"]
    # the thread decode of the device, inverted: (row j, group i0 / 4) of plane 0 -> block index within the plane
    dec = dump[4][:nstrips * nbs * B]
    owner = {}
    for e in np.flatnonzero(dec >= 0):
        owner[(int(dec[e]) >> 32, (int(dec[e]) & 0xffffffff) // 4)] = int(e) // B
    assert len(owner) == ny * P4
    want_sp, want_spV = np.zeros(nk * nstrips, np.int32), np.zeros(nk * nstrips, np.int32)
    sizes = set()
    for q, (kind, n) in enumerate(probes):
        idx, _ = probe_cells(shape, n, 100 + q)
        k, j, i = idx // (nx * ny), (idx // nx) % ny, idx % nx
        blocks = sorted({int(kk) * nstrips * nbs + owner[(int(jj), int(ii) // 4)] for kk, jj, ii in zip(k, j, i)})
        got = blk[rng[2 * q]:rng[2 * q + 1]].tolist()
        assert got == blocks, (name, q, sorted(set(blocks) - set(got)), sorted(set(got) - set(blocks)))
        for kk, jj in zip(k, j):
            (want_sp if kind == 1 else want_spV)[int(kk) * nstrips + int(jj) // tys] = 1
        sizes.add(len({(int(kk), int(jj) // tys) for kk, jj in zip(k, j)}))
    assert np.array_equal(sp, want_sp) and np.array_equal(spV, want_spV)
    assert max(sizes) > 1 or max(n for _, n in probes) == 1      # the larger probes spread over several strip-planes
    assert rng[2 * len(probes):].tolist() == [0] * (128 - 2 * len(probes)) and rng[2 * len(probes) - 1] == blk.size


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_delayed_blocks_leave_fields_and_series_equal_to_the_oracle(tmp_path, case):
    """A wait that is missing shows in the fields once the block it should have waited for is late.  The diagnostic build lets chosen blocks
    spin for 20 x the case's median block duration (measured from its own stamps, at most 1 ms; the flag limit is 2 s) right after their
    decode — polls, flags and arithmetic unchanged —, one block in 16 per timestep, every block once over the eight seeds, plus E blocks
    only and H blocks only.  Seeded fields, 6 timesteps, under one launch per timestep with the E sweep 1 and 3 planes ahead, all E then all
    H blocks, and all 6 timesteps in one launch (Mur faces: the last two): fields, and every probe series, equal the oracle's bit for bit.
    That the delay opens the window is asserted from the stamps: for every delayed block some block that polls its flag (by the host build of
    wait_sets.hpp) began polling before the delayed block ended and returned from the poll after it — in at least one of the timesteps in
    which the block was delayed under that schedule (a block is delayed in three of the six; now and then a waiter is dispatched only after
    the delayed block has ended, and that timestep proves nothing for the block; the child's report counts those instances; blocks left
    without such a waiter after the ten masks are delayed once more, alone, in up to two follow-up runs of the same schedule).  H blocks are
    delayed only where a block of the same launch waits for them (several timesteps per launch, all but the last timestep)."""
    import json
    out = str(tmp_path / "delay.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wait_sets_diag_child.py"), "delay", case[0], out], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    rep = json.load(open(out))
    want = {"all_E_then_all_H", "several_timesteps_per_launch"} | (set() if case[3] is not None else {"lag1", "lag3"})
    assert set(rep["schedules"]) == want
    for sched, rec in rep["schedules"].items():
        assert 0 < rec["delay_ticks"] <= 100000 and rec["delay_ticks"] == min(20 * rec["median_block_ticks"], 100000)
        assert rec["every_E_block_delayed_once"] and rec["every_H_block_delayed_once"] in (True, None), (sched, rec)
        assert (rec["every_H_block_delayed_once"] is True) == (sched == "several_timesteps_per_launch")
        for mask, run in rec["runs"].items():
            assert run["fields_equal_oracle"] and run["series_equal_oracle"], (sched, mask)
            if mask != "none":
                assert run["delayed"] > 0, (sched, mask)
        assert rec["delayed_blocks_no_waiter_ever_waited_for"] == [], (sched, rec["delayed_blocks_no_waiter_ever_waited_for"][:10])
