"""Shared cases of the field-excitation tests, and the numpy statement of include/fdtd_hip_excite.h, operation for operation in float32.

The oracle knows nothing of H-field excitations, so the reference is the oracle's half-steps with `HLists.apply` behind the H half-step,
last of the H-side corrections: restatement.Restatement's eighth part ("excite" of restatement.ORDER)."""
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


def ExciteRestatement(sim, lib, lists, **kw):
    """restatement.Restatement of `sim` with the H-field excitations `lists` (HLists) as its eighth correction."""
    return Restatement(sim, lib, tables=dict(kw.pop("tables", None) or {}, excite=lists.args()), **kw)


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
    """restatement.install: Simulation.build -> the restatement's engine when the simulation holds H-field excitations and the library
    lacks fdtd_excite_set (the oracle), the real build otherwise: the checker of the API-level tests.  The restatement is sim.restated.
    `sig_h(sim)`: another pulse table for the statement than the simulation's own (the negative control of the half-step timing)."""
    tables = None if sig_h is None else (lambda sim: {} if sim.excite_h_args is None else {"excite": (*sim.excite_h_args[:8], sig_h(sim))})
    restatement.install(monkeypatch, tables=tables)


# ---- directed list shapes of fdtd_excite_set / k_excite (test_excite_gpu.py; their CPU side: test_field_excitation_cpu.py) ------------
NX_EXTREMES = (20, 21, 22, 23)          # every nx mod 4
PLANE_COUNTS = (1, 255, 256, 257)       # distinct faces around k_excite's block of 256 threads
_cols = lambda l: ([e[0] for e in l], [e[1] for e in l], [e[2] for e in l], [e[3] for e in l])


def face_exists(comp, i, j, k, n):
    """Integer arithmetic: the node is in the grid and the face of component `comp` there has a cell along both transverse axes."""
    p = (i, j, k)
    return all(0 <= p[a] < n[a] for a in range(3)) and all(p[a] < n[a] - 1 for a in range(3) if a != comp)


def plane_faces(count, n=MAIN_GRID):
    """`count` distinct faces (comp, i, j, k) of the node plane k = 5: z-faces row by row, then x-faces."""
    nx, ny, nz = n
    out = [(2, i, j, 5) for j in range(ny - 1) for i in range(nx - 1)] + [(0, i, j, 5) for j in range(ny - 1) for i in range(nx)]
    assert len(out) >= count
    return out[:count]


def plane_lists(count, hard, seed=3, nsig=40, n=MAIN_GRID):
    """`count` distinct faces on one node plane, each with one soft entry (delays 0, 3, 57); `hard`: a hard entry on every face as well
    (delays 3, 0, 57), so that every thread takes the hard branch and then adds its soft entry."""
    rng = np.random.default_rng(seed + count)
    faces = plane_faces(count, n)
    soft = [(node(i, j, k, n), c, 1e-3 * rng.standard_normal(), (0, 3, 57)[q % 3]) for q, (c, i, j, k) in enumerate(faces)]
    hard_l = [(node(i, j, k, n), c, 1e-3 * rng.standard_normal(), (3, 0, 57)[q % 3]) for q, (c, i, j, k) in enumerate(faces)] if hard else []
    return HLists(_cols(hard_l), _cols(soft), rng.standard_normal(nsig).astype(np.float32))


def many_entries_lists(nentries=300, seed=9, nsig=40, reverse=False, n=MAIN_GRID):
    """ONE face with `nentries` soft entries: amplitudes over six decades with both signs, delays 0 ... 139 against a table of 40 samples
    and runs of 80 timesteps — entries in front of the table's start, inside it and never reached.  `reverse`: the same entries in
    the reversed list order (another float32 sum)."""
    rng = np.random.default_rng(seed)
    amp = (1e-3 * rng.choice([-1.0, 1.0], nentries) * 10.0 ** rng.uniform(-6.0, 0.0, nentries)).astype(np.float32)
    delay = rng.integers(0, 140, nentries).astype(np.int32)
    delay[:3] = (0, 20, 139)
    o = slice(None, None, -1) if reverse else slice(None)
    soft = (np.full(nentries, node(9, 6, 6, n), np.int64), np.full(nentries, 1, np.int8), amp[o], delay[o])
    return HLists(_cols([]), soft, rng.standard_normal(nsig).astype(np.float32))


def forty_faces_lists(order, seed=12, nsig=40, n=MAIN_GRID):
    """40 faces (all three components, nodes spread over the grid) with 3 soft entries each — 1, 1e-7, -1 times a common scale: their
    order shows in float32 — listed "face-major" (a face's three entries one after the other) or "entry-major" (the first entries of
    all faces, then the second ones, ...: a face's entries are scattered through the list, 40 apart).  Both keep each face's entries
    in the same order, so the host's stable grouping reaches the same set."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = n
    faces = [(q % 3, 1 + (7 * q) % (nx - 2), 1 + (5 * q) % (ny - 2), 2 + (3 * q) % (nz - 4)) for q in range(40)]
    assert len(set(faces)) == 40 and all(face_exists(*f, n) for f in faces)
    scale = 0.2 * rng.uniform(0.5, 1.5, 40)
    entry = lambda f, r: (node(*faces[f][1:], n), faces[f][0], scale[f] * (1.0, 1e-7, -1.0)[r], (0, 3, 11)[(f + r) % 3])
    pairs = [(f, r) for f in range(40) for r in range(3)] if order == "face-major" else [(f, r) for r in range(3) for f in range(40)]
    assert order in ("face-major", "entry-major")
    return HLists(_cols([]), _cols([entry(f, r) for f, r in pairs]), rng.standard_normal(nsig).astype(np.float32))


def extreme_faces(n):
    """The faces at the grid's extremes, (comp, i, j, k): per component the face at the origin, the last existing face along each axis
    (the others mid-grid) and the last one along all three at once — along the component's own axis the last node plane n - 1, along a
    transverse axis the last cell n - 2."""
    last = lambda c: [n[a] - 1 if a == c else n[a] - 2 for a in range(3)]
    mid = [n[a] // 2 for a in range(3)]
    out = []
    for c in range(3):
        out.append((c, 0, 0, 0))
        for a in range(3):
            p = list(mid)
            p[a] = last(c)[a]
            out.append((c, *p))
        out.append((c, *last(c)))
    return out


def beyond(face, n):
    """The neighbours of a face one step further along each transverse axis on which it is the last: nodes of the grid without that face."""
    c, *p = face
    out = []
    for a in range(3):
        if a != c and p[a] == n[a] - 2:
            q = list(p)
            q[a] += 1
            out.append((c, *q))
    return out


def extreme_lists(nx, hard, seed=21, nsig=40):
    """extreme_faces of the grid nx x 14 x 12 as a soft list (each face once, the corner faces twice) or as a hard list."""
    n = (nx,) + MAIN_GRID[1:]
    rng = np.random.default_rng(seed + nx)
    faces = extreme_faces(n)
    entries = [(node(i, j, k, n), c, 1e-3 * rng.standard_normal(), (0, 3, 57)[q % 3]) for q, (c, i, j, k) in enumerate(faces)]
    if not hard:
        entries += [(g, c, -0.5 * a, 3) for g, c, a, _ in entries[4::5]]
    empty = _cols([])
    return HLists(_cols(entries) if hard else empty, empty if hard else _cols(entries), rng.standard_normal(nsig).astype(np.float32))


def held_lists(nsteps=80, seed=17, nsig=40, n=MAIN_GRID):
    """Two hard faces that the excitation holds at zero: one with amp = +0.0 (inside the table 0.0f * s: a zero with the sign of s), one
    with amp = 0.7 whose delay lies past the run (0.7f * 0.0f = +0.0 in every timestep); and a soft entry on each, past the run too
    (it adds nothing, not even a zero)."""
    rng = np.random.default_rng(seed)
    faces = [(node(5, 4, 6, n), 0), (node(12, 8, 4, n), 2)]
    hard = [(faces[0][0], faces[0][1], 0.0, 2), (faces[1][0], faces[1][1], 0.7, nsteps + 5)]
    soft = [(g, c, 0.3, nsteps + 9) for g, c in faces]
    return HLists(_cols(hard), _cols(soft), rng.standard_normal(nsig).astype(np.float32))


# ---- what samples I behind the excitation: one small scene with an I-probe, an I-DFT box and a recorder face -------------------------
OBS_GRID = (20, 16, 12)
OBS_STEPS, OBS_EVERY, OBS_FREQS = 80, 5, np.array([8e9, 11e9])
OBS_KINDS = {"pec": ["PEC"] * 6, "mur": ["MUR"] * 6, "mur-near": ["MUR"] * 6}


def observer_scene(kind):
    """The scene of test_excite_gpu's observer tests on OBS_GRID with PEC faces ("pec") or six Mur faces ("mur", "mur-near"), as a dict:
    `lists`   HLists with a hard z-face `hard` and a soft z-face `soft` (two entries) among a dozen other excited faces of all components;
    `probe`   (idx, comp, w) of an I-probe over the hard face, the soft face and a bare face;
    `box`     (comp, lo, hi) in nodes, inclusive: a one-plane box over the hard and the soft face — the I-DFT box of the `dft` mode and
              the recorder face of the `record` mode;
    `late`    (idx, comp, w): a second I-probe over the same two faces, for adding between two calls;
    `source`  None, or (idx, comp, amp) of a soft voltage source.
    "mur-near": the hard face is the z-face at i = 1, one node from the Mur face plane x-, the soft one the z-face of the last cell
    row j = ny - 2, and a soft voltage source sits on the plane next to the face x-: the library then takes its sources and probes out
    of the update launches (sources_fusable in csrc/api.hip), so the I-probes are sampled by k_post instead of the probe blocks."""
    n = OBS_GRID
    rng = np.random.default_rng(31 + len(kind))
    if kind == "mur-near":
        hard, soft, bare, lo, hi = (2, 1, 7, 6), (2, 4, n[1] - 2, 6), (2, 3, 8, 6), (1, 6, 6), (5, n[1] - 2, 6)
        source = (np.array([node(1, 5, 5, n)], np.int64), np.array([2], np.int8), np.array([0.01], np.float32))
    else:
        hard, soft, bare, lo, hi = (2, 8, 7, 6), (2, 10, 8, 6), (2, 9, 9, 6), (7, 6, 6), (11, 9, 6)
        source = None
    others = [(q % 3, 2 + (5 * q) % 15, 2 + (3 * q) % 11, 3 + q % 6) for q in range(12)]
    assert len({hard, soft, bare, *others}) == 15 and all(face_exists(*f, n) for f in (hard, soft, bare, *others))
    g = lambda f: node(*f[1:], n)
    hard_l = [(g(hard), 2, 1.5e-3, 2), (g(others[0]), others[0][0], -1e-3, 0), (g(others[1]), others[1][0], 2e-3, 30)]
    soft_l = [(g(soft), 2, 1e-3, 0), (g(soft), 2, -3e-4, 7)] + [(g(f), f[0], 1e-3 * rng.standard_normal(), (0, 3, 57)[q % 3]) for q, f in enumerate(others[1:])]
    lists = HLists(_cols(hard_l), _cols(soft_l), rng.standard_normal(60).astype(np.float32))
    idx = np.array([g(hard), g(soft), g(bare)], np.int64)
    comp = np.array([2, 2, 2], np.int8)
    return {"kind": kind, "lists": lists, "hard": hard, "soft": soft, "probe": (idx, comp, np.array([1.0, -2.0, 0.5], np.float32)),
            "late": (idx[:2], comp[:2], np.array([0.25, 4.0], np.float32)), "box": (2, lo, hi), "source": source}


def observer_sim(kind):
    return main_sim(n=OBS_GRID, nr_ts=OBS_STEPS, boundary=OBS_KINDS[kind], cpml_cells=0)


def observer_twiddles(dt):
    """(tw_v, tw_i) of set_dft, and the identity table of rec_transform: "frequency" f picks sample f, so the record itself comes back."""
    exc = pkg("excitation")
    nsamp = OBS_STEPS // OBS_EVERY + 1
    ident = np.zeros((nsamp, nsamp, 2))
    ident[np.arange(nsamp), np.arange(nsamp), 0] = 1.0
    return exc.dft_twiddles(OBS_FREQS, dt, OBS_EVERY, nsamp, 0.0), exc.dft_twiddles(OBS_FREQS, dt, OBS_EVERY, nsamp, 0.5), ident


class Observed:
    """The observer scene on the restatement: after run(), behind the excitation (what the library must give) and, for the CPU proof,
    in front of it (`*_front`: the same observer reading the current the plane wave's launch would have left):
      .series / .series_front     the I-probe [OBS_STEPS], double, the probe's fma chain;
      .late                       the second I-probe, added in front of timestep `late_at`: its samples from there on;
      .acc / .acc_front           the box's running DFT sums, complex128 [2] + box shape;
      .rec / .rec_front           the box's record, float32 [samples] + box shape (timesteps 0, OBS_EVERY, ...);
      .fields."""

    def __init__(self, lib, kind, late_at=8):
        sc = self.scene = observer_scene(kind)
        self.sim = observer_sim(kind)
        r = self.r = Restatement(self.sim, lib, seed=5, tables={"excite": sc["lists"].args()})
        if sc["source"] is not None:
            r.e.add_source(*sc["source"])
        self.pid = r.add_probe(1, *sc["probe"])
        self.late_at, self.late_pid = late_at, None
        c, lo, hi = sc["box"]
        self.comp, self.sl = c, (slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1), slice(lo[0], hi[0] + 1))

    def run(self):
        r, sc = self.r, self.scene
        tw = observer_twiddles(self.sim.dt)[1]
        seen = r.record("excite")
        shape = tuple(s.stop - s.start for s in self.sl)
        self.acc, self.acc_front = np.zeros((2,) + shape, np.complex128), np.zeros((2,) + shape, np.complex128)
        self.series_front, rec, rec_front = [], [], []
        idx, comp, w = sc["probe"]
        for n in range(OBS_STEPS):
            if n == self.late_at:
                self.late_pid = r.add_probe(1, *sc["late"])
            r.step()
            assert r.n == n
            front = seen["excite"][0]
            s = 0.0
            for g, c, wq in zip(idx, comp, w):
                s = float(wq) * float(front[c].reshape(-1)[g]) + s
            self.series_front.append(s)
            if n % OBS_EVERY == 0:
                t = tw[n // OBS_EVERY, :, 0] + 1j * tw[n // OBS_EVERY, :, 1]
                self.acc += t[:, None, None, None] * r.I[self.comp][self.sl].astype(np.float64)[None]
                self.acc_front += t[:, None, None, None] * front[self.comp][self.sl].astype(np.float64)[None]
                rec.append(r.I[self.comp][self.sl].copy())
                rec_front.append(front[self.comp][self.sl].copy())
        self.series, self.series_front = r.get_probe(self.pid), np.array(self.series_front)
        self.late = r.get_probe(self.late_pid)
        self.rec, self.rec_front = np.stack(rec), np.stack(rec_front)
        self.fields = r.e.fields()
        return self


_OBSERVED = {}


def observed(oracle_lib, kind):
    """The finished reference run of the observer scene, once per session, left unchanged."""
    if kind not in _OBSERVED:
        _OBSERVED[kind] = Observed(oracle_lib, kind).run()
    return _OBSERVED[kind]
