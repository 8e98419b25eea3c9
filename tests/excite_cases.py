"""Shared cases of the field-excitation tests, and the numpy statement of include/fdtd_hip_excite.h, operation for operation in float32.

The oracle knows nothing of H-field excitations, so the reference is the oracle's half-steps with `HLists.apply` behind the H half-step,
last of the H-side corrections: `ExciteRestatement` is restatement.Restatement with that one more part."""
import numpy as np

import restatement
from conftest import pkg
from restatement import Restatement

MAIN_GRID = (21, 14, 12)     # nx odd: rows of P = 24 floats


class HLists:
    """The hard list and the soft list of fdtd_excite_set — each (idx int64 [n], comp int8 [n], amp float32 [n], delay int32 [n]) — and
    sigH.  apply(I, n) is the header's statement at timestep n on the three current arrays [nz][ny][nx], in place:

        the face's hard entry first:            I = amp * s              (s = 0.0f outside the table: the face is held at zero)
        then its soft entries, in list order:   t = amp * s; I = I + t   (outside the table: nothing, I keeps its bits)

    Entries of one face are applied one after the other (the q-th entries of all faces together: a face appears once among them)."""

    def __init__(self, hard, soft, sigH):
        cast = lambda l: (np.asarray(l[0], np.int64).ravel(), np.asarray(l[1], np.int8).ravel(), np.asarray(l[2], np.float32).ravel(),
                          np.asarray(l[3], np.int32).ravel())
        self.hard, self.soft, self.sigH = cast(hard), cast(soft), np.asarray(sigH, np.float32).ravel()
        key = self.soft[0] * 3 + self.soft[1]
        self.rank = np.zeros(key.size, np.int64)        # the position of an entry among the entries of its face
        seen = {}
        for e, k in enumerate(key.tolist()):
            self.rank[e] = seen.get(k, 0)
            seen[k] = self.rank[e] + 1
        hk = self.hard[0] * 3 + self.hard[1]
        assert np.unique(hk).size == hk.size, "a face twice in the hard list"

    def args(self):
        return (*self.hard, *self.soft, self.sigH)

    def faces(self):
        """The distinct (idx, comp) pairs of both lists."""
        k = np.unique(np.concatenate([self.hard[0] * 3 + self.hard[1], self.soft[0] * 3 + self.soft[1]]))
        return k // 3, (k % 3).astype(np.int8)

    def _sig(self, delay, n):
        p = n - delay.astype(np.int64)
        inside = (p >= 0) & (p < self.sigH.size)
        s = np.where(inside, self.sigH[np.clip(p, 0, max(self.sigH.size - 1, 0))], np.float32(0.0)).astype(np.float32)
        return s, inside

    def apply(self, I, n):
        assert all(a.dtype == np.float32 and a.flags.c_contiguous for a in I)
        flat = [a.reshape(-1) for a in I]
        idx, comp, amp, delay = self.hard
        s, _ = self._sig(delay, n)
        v = amp * s
        for c in range(3):
            q = comp == c
            flat[c][idx[q]] = v[q]
        idx, comp, amp, delay = self.soft
        s, inside = self._sig(delay, n)
        for r in range(int(self.rank.max()) + 1 if self.rank.size else 0):
            for c in range(3):
                q = np.nonzero((self.rank == r) & (comp == c) & inside)[0]
                if q.size:
                    t = amp[q] * s[q]
                    flat[c][idx[q]] = flat[c][idx[q]] + t


class _Part:
    def __init__(self, lists):
        self.lists = lists

    def apply(self, F, r):
        self.lists.apply(F, r.n)


class ExciteRestatement(Restatement):
    """Restatement with the H-field excitations `lists` (HLists) applied behind the H half-step, behind the plane wave's face list."""

    def __init__(self, sim, lib, lists, **kw):
        super().__init__(sim, lib, **kw)
        self.excite = _Part(lists)
        self.parts["excite"] = self.excite

    def get_probe(self, pid):
        if pid in self.i_probes:
            return np.array(self.i_series.get(pid, []), np.float64)
        return self.e.get_probe(pid)

    def step(self):
        e = self.e
        e.half_step(0)
        self.n = int(e.step)
        if any(name in self.parts for name in restatement.E_SIDE + ("conformal",)):      # (conformal faces read the voltages)
            self.V = [self.get(0, c) for c in range(3)]
            self._apply(restatement.E_SIDE, 0, self.V)
        e.half_step(1)
        self.I = [self.get(1, c) for c in range(3)]
        self._apply(restatement.H_SIDE + ("excite",), 1, self.I)
        for pid, (idx, comp, w) in self.i_probes.items():      # (the oracle sampled its I-probes in front of the corrections)
            s = 0.0
            for g, c, wq in zip(idx, comp, w):
                s = float(wq) * float(self.I[c].reshape(-1)[g]) + s
            self.i_series.setdefault(pid, []).append(s)
        self.nstep += 1
        if self.nstep == 1 or self.nstep % 8 == 0:
            self.note_moved()


def node(i, j, k, n=MAIN_GRID):
    return (k * n[1] + j) * n[0] + i


def main_sim(add=None, *, n=MAIN_GRID, nr_ts=100, boundary=("PEC", "PEC", "PEC", "PEC", "CPML", "CPML"), cpml_cells=4, use_classes=True):
    """The main parity grid: 21 x 14 x 12 nodes of 1 mm, CPML of 4 cells on z, PEC elsewhere; `add(scene)` draws into it."""
    sc, sim, grid = pkg("scene"), pkg("simulation"), pkg("grid")
    g = grid.RectGrid(*[np.arange(k) * 1e-3 for k in n])
    s = sc.Scene(unit=1e-3)
    if add is not None:
        add(s)
    return sim.Simulation(g, sc.voxelize(s, g), f0=10e9, fc=4e9, boundary=list(boundary), cpml_cells=cpml_cells, nr_ts=nr_ts, end_criteria=0.0,
                          use_classes=use_classes)


def main_lists(seed=1, nsig=40, rows=(0, 13), n=MAIN_GRID):
    """The H lists of the main parity case on MAIN_GRID, faces with rows(0) <= j < rows(1) only:
      * 300 soft faces on the node plane k = 5 (more than one block of 256): every z-face of the rows, then x-faces, then y-faces;
      * 5 faces with three soft entries each, amplitudes 1, 1e-7, -1 (times a common scale): the list order shows in float32;
      * 4 hard faces, two of which also carry soft entries;
      * delays 0, 3 and 57: an entry before, inside and past the 40-sample table within 100 timesteps;
      * faces in the first (i = 0..3) and the last (i = 16..20) four-cell group of a row; all three components."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = n
    j0, j1 = rows[0], min(rows[1], ny - 1)
    zf = [(node(i, j, 5, n), 2) for j in range(j0, j1) for i in range(nx - 1)]
    xf = [(node(i, j, 5, n), 0) for j in range(j0, j1) for i in range(nx)]
    yf = [(node(i, j, 5, n), 1) for j in range(j0, j1) for i in range(nx - 1)]
    plane = (zf + xf + yf)[:300]
    assert len(plane) == 300 and any(c == 0 for _, c in plane) and any(c == 2 for _, c in plane)
    soft = [(g, c, 1e-3 * rng.standard_normal(), (0, 3, 57)[q % 3]) for q, (g, c) in enumerate(plane)]
    triple = [(node(1, j0, 7, n), 1), (node(18, j0, 7, n), 1), (node(0, j0 + 1, 6, n), 2), (node(19, j0 + 1, 6, n), 2), (node(nx - 1, j0, 8, n), 0)]
    for q, (g, c) in enumerate(triple):
        for a in (1.0, 1e-7, -1.0):
            soft.append((g, c, 0.37 * a, (0, 3, 0, 3, 57)[q]))
    hard_faces = [(node(2, j0, 2, n), 1), (node(17, j0 + 1, 9, n), 0), plane[7], triple[1]]     # the last two carry soft entries too
    hard = [(g, c, 1e-3 * rng.standard_normal(), (3, 57, 0, 3)[q]) for q, (g, c) in enumerate(hard_faces)]
    cols = lambda l: ([e[0] for e in l], [e[1] for e in l], [e[2] for e in l], [e[3] for e in l])
    sigH = rng.standard_normal(nsig).astype(np.float32)
    return HLists(cols(hard), cols(soft), sigH)


def install(monkeypatch, sig_h=None):
    """Simulation.build -> an ExciteRestatement's engine when the simulation holds H-field excitations and the library lacks
    fdtd_excite_set (the oracle), the real build otherwise: the checker of the API-level tests.  The restatement is sim.restated.
    `sig_h(sim)`: another pulse table for the statement than the simulation's own (the negative control of the half-step timing)."""
    Sim = pkg("simulation").Simulation
    orig = Sim.build

    def build(self, lib, **kw):
        args = self.excite_h_args
        if args is None or pkg("_capi").has_excite(lib):
            return orig(self, lib, **kw)
        lists = HLists(args[0:4], args[4:8], args[8] if sig_h is None else sig_h(self))
        self.excite_h_args = None
        try:
            r = ExciteRestatement(self, lib, lists, flags=kw.get("flags", 0))
        finally:
            self.excite_h_args = args
        for name, pl in self.probes.items():          # the stand-alone current probes: sampled behind the excitations, as on the device
            if pl.kind == 1:
                for pid, q in zip(self._probe_ids[name], pl.lists):
                    r.i_probes[pid] = (np.asarray(q.idx, np.int64), np.asarray(q.comp, np.int64), np.asarray(q.w, np.float32))
        self.engine, self.lib = r.engine, lib
        self.rank, self.world, self.device, self._build_flags = 0, 1, 0, 0
        self.restated = r
        return r.engine
    monkeypatch.setattr(Sim, "build", build)
