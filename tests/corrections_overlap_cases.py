"""Overlapping lists through the raw C ABI (CPU: the reference side alone, test_corrections_fuzz_cpu.py; GPU: HIP against it,
test_corrections_fuzz_gpu.py).  The scene layer keeps every correction off every other's elements; the setters take any existing edge
or face, and the headers say "the order above holds for any edge set this call accepts".  The tables here are made by hand on a grid
of 12 x 10 x 9 nodes with PEC faces (and again with a Mur face at x+, far from the elements, so that both Mur schedules run):

  edge A  z-directed at node (6, 5, 4): inside a Debye box (w != 0), a sheet edge, an element edge and on the plane wave's E list;
  edge B  x-directed at node (6, 6, 3): the same inside a Lorentz box;
          each under a V-probe of its own and inside a V-DFT box;
  face F  y-normal at node (6, 5, 4) (edge A is one of its four): magnetic class 1, a listed conformal face and on the plane wave's
          H list, under an I-probe and inside an I-DFT box; it also carries two soft entries of fdtd_excite_set, 1 and 1e-7 of a common
          scale, whose order shows in float32;
  face G  y-normal at node (7, 5, 4): magnetic class 2, on the plane wave's H list, and a hard entry of fdtd_excite_set: whatever the
          other lists did, its current is amp * sigH[n - delay], under an I-probe and inside an I-DFT box of its own;
  and a few more elements per list that overlap in pairs or not at all (include/fdtd_hip_excite.h leaves the placement to the caller:
  the C ABI accepts an excited face that is a magnetic, conformal or plane-wave face, and the launch order decides the bits there).

The reference is restatement.Restatement with these raw tables: the headers' statement lists in the headers' order on the oracle's
half-steps: Debye, Lorentz, sheets, elements, plane wave (E list) between the E phase and the H update, magnetic, conformal, plane wave
(H list), H-field excitations behind the H update.  V-probes and V-DFT boxes read in front of every E-side correction (the oracle's own E phase samples
them there), I-probes and I-DFT boxes behind every H-side one (kept here: the oracle samples I inside its H half-step)."""
import numpy as np

from conftest import pkg
from restatement import E_SIDE, ORDER, Restatement

N = (12, 10, 9)
STEPS, CALLS, SEED = 60, (25, 35), 11
EVERY, FREQS = 5, np.array([8e9, 11e9])
NAMES = ORDER[:-1] + ("excite_soft", "excite_hard")                   # what `dropped` can take out: the excitations' two lists singly
A, B, F, G = (2, 6, 5, 4), (0, 6, 6, 3), (1, 6, 5, 4), (1, 7, 5, 4)
V_PROBES = [([A], [1.0]), ([B], [-0.5])]
I_PROBES = [([F], [1.0]), ([F, (2, 6, 5, 4)], [2.0, -1.0]), ([G], [1.0])]
V_BOXES = [(2, (5, 4, 3), (7, 6, 5)), (0, (5, 5, 2), (7, 7, 4))]      # (component, lo, hi) in nodes, inclusive: over A / over B
I_BOXES = [(1, (5, 4, 3), (7, 6, 5)), (1, (7, 4, 4), (7, 6, 4))]      # over F (and G) / over G alone
NSIG_H, HARD_G = 40, (2.5, 2)                                         # sigH's samples; (amplitude, delay) of the hard entry on G


def flat(i, j, k):
    return (k * N[1] + j) * N[0] + i


def overlap_sim(mur=False, nr_ts=STEPS):
    sc, sim = pkg("scene"), pkg("simulation")
    g = pkg("grid").RectGrid(*[np.arange(k) * 1e-3 for k in N])
    s = sc.Scene(unit=1e-3)
    s.add_lumped_port(1, 50.0, [3, 3, 2], [3, 3, 4], "z", 1.0)
    boundary = ["PEC", "MUR" if mur else "PEC", "PEC", "PEC", "PEC", "PEC"]
    return sim.Simulation(g, sc.voxelize(s, g), f0=10e9, fc=4e9, boundary=boundary, nr_ts=nr_ts, end_criteria=0.0)


def _list(elems):
    return np.array([flat(i, j, k) for _, i, j, k in elems], np.int64), np.array([c for c, _, _, _ in elems], np.int8)


def _at(arr, elems):
    """arr [3][nz][ny][nx] at the elements."""
    return np.array([arr[c][k, j, i] for c, i, j, k in elems], np.float32)


def _box(rng, lo, hi, draw):
    shape = (hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0])
    return draw(rng, shape)


def hand_tables(op, dt, seed=5):
    """The argument tuples of the eight setters, keyed by ORDER's sets ("pw" holds both lists, "excite" both of its).  op: Engine.get_operator() of the scene."""
    disp, lor, lum, pwm = pkg("dispersion"), pkg("lorentz"), pkg("lumped"), pkg("planewave")
    rng = np.random.default_rng(seed)
    vi, iv = op[1], op[3]
    empty = ((0, 0, 0), (0, 0, 0))
    T = {}
    # Debye: one box of z-edges around A, about a third of the weights zero
    dlo, dhi = (5, 4, 3), (8, 7, 6)
    w = _box(rng, dlo, dhi, lambda r, s: (1e-3 * r.uniform(0.2, 1.0, s) * (r.uniform(size=s) > 0.3)).astype(np.float32))
    w[A[3] - dlo[2], A[2] - dlo[1], A[1] - dlo[0]] = 7e-4
    z3 = np.zeros((0, 0, 0), np.float32)
    med = [disp.DebyeMedium(2.5, 0.0, [0.8, 0.3], [2e-11, 6e-12])]
    T["debye"] = disp.tables(med, dt) + ([empty[0], empty[0], dlo], [empty[1], empty[1], dhi], [z3, z3, w], None)
    # Lorentz: one box of x-edges around B, two media
    llo, lhi = (5, 5, 2), (8, 8, 5)
    w = _box(rng, llo, lhi, lambda r, s: (1e-3 * r.uniform(0.2, 1.0, s) * (r.uniform(size=s) > 0.3)).astype(np.float32))
    w[B[3] - llo[2], B[2] - llo[1], B[1] - llo[0]] = 6e-4
    m = _box(rng, llo, lhi, lambda r, s: r.integers(0, 2, s).astype(np.uint8))
    two_pi = 2 * np.pi
    media = [lor.LorentzMedium(1.0, 0.0, two_pi * np.array([7e9, 5e9]), two_pi * np.array([0.0, 9e9]), np.array([3e9, 1e9])),
             lor.LorentzMedium(1.0, 0.0, two_pi * np.array([4e9, 6e9]), two_pi * np.array([11e9, 0.0]), np.array([0.0, 8e9]))]
    z8 = np.zeros((0, 0, 0), np.uint8)
    T["lorentz"] = lor.tables(media, dt, K=2) + ([llo, empty[0], empty[0]], [lhi, empty[1], empty[1]], [w, z3, z3], [m, z8, z8])
    # sheets: A, B, a y-edge at A's node, a z-edge elsewhere; two classes of two branches
    el = [A, B, (1, 6, 5, 4), (2, 4, 4, 4)]
    idx, comp = _list(el)
    T["sheets"] = (idx, comp, _at(vi, el), np.array([0, 1, 1, 0], np.int32), np.array([[0.6, 0.95], [0.8, 0.5]], np.float32),
                   np.array([[3e-4, 1e-4], [2e-4, 4e-4]], np.float32))
    # elements: A, B and one more edge; a series R-L and a parallel L-C
    el = [A, B, (0, 4, 6, 5)]
    idx, comp = _list(el)
    parts = [lum.Element("series-rl", 50.0, 1e-9, None, "series"), lum.Element("parallel-lc", None, 2e-9, 0.5e-12, "parallel")]
    T["elements"] = (idx, comp, _at(vi, el)) + lum.tables(parts, np.array([0, 1, 0]), dt)
    # magnetic: a box of y-normal faces around F and a box of x-normal ones, classes 0 ... 2
    mlo, mhi = (5, 4, 3), (8, 7, 6)
    cy = _box(rng, mlo, mhi, lambda r, s: r.integers(0, 3, s).astype(np.uint8))
    cy[F[3] - mlo[2], F[2] - mlo[1], F[1] - mlo[0]] = 1
    cy[G[3] - mlo[2], G[2] - mlo[1], G[1] - mlo[0]] = 2
    xlo, xhi = (4, 4, 4), (6, 6, 6)
    cx = _box(rng, xlo, xhi, lambda r, s: r.integers(0, 3, s).astype(np.uint8))
    T["magnetic"] = (np.array([0.97, 0.9], np.float32), np.array([0.6, 0.85], np.float32), [xlo, mlo, empty[0]], [xhi, mhi, empty[1]], [cx, cy, z8])
    # conformal: F, another face of the magnetic box, two faces outside it
    fc = [F, (1, 5, 6, 3), (0, 6, 4, 3), (2, 5, 5, 5)]
    idx, comp = _list(fc)
    T["conformal"] = (comp, idx, (_at(iv, fc)[:, None].astype(np.float64) * rng.uniform(0.5, 2.0, (len(fc), 4))).astype(np.float32))
    # the plane wave: A, B and three more edges; F and three more faces
    def hand(elems):
        n = len(elems)
        i_, c_ = _list(elems)
        coef = (1e-3 * rng.standard_normal((n, 2))).astype(np.float32)
        coef[::4, 1] = 0
        w_ = rng.uniform(0, 1, (n, 2)).astype(np.float32)
        w_[w_ >= 1] = 0
        return i_, c_, coef, rng.integers(0, 41, (n, 2)).astype(np.int32), w_
    T["pw"] = pwm.Tables(hand([A, B, (1, 5, 5, 5), (2, 7, 5, 4), (0, 5, 6, 3)]), hand([F, (2, 6, 5, 4), (0, 5, 5, 5), (1, 7, 5, 4)]),
                         pwm.signal2(10e9, 4e9, 18e-12, 40))
    # the H-field excitations (a generator of their own: the tables above are what they were): hard on G and on a face no other list has;
    # soft twice on F — in float32 (I + t) + 1e-7 t is not (I + 1e-7 t) + t — and once on two other faces, one of them conformal
    rx = np.random.default_rng(seed + 1000)
    hard, soft = [G, (2, 3, 6, 5)], [F, (0, 6, 4, 3), F, (2, 4, 3, 6)]
    hi_, hc_ = _list(hard)
    si_, sc_ = _list(soft)
    T["excite"] = (hi_, hc_, np.array([HARD_G[0], -0.8], np.float32), np.array([HARD_G[1], 0], np.int32),
                   si_, sc_, np.array([0.9, 0.4, 0.9e-7, -0.6], np.float32), np.array([0, 3, 0, 30], np.int32),
                   (1e-3 * rx.standard_normal(NSIG_H)).astype(np.float32))
    return T


def dropped(T, name):
    """The tables without one correction (the plane wave's two lists count singly)."""
    pwm = pkg("planewave")
    out = {k: v for k, v in T.items() if k != name}
    if name in ("excite_soft", "excite_hard"):
        x = T["excite"]
        out["excite"] = tuple(a[:0] for a in x[:4]) + x[4:] if name == "excite_hard" else x[:4] + tuple(a[:0] for a in x[4:8]) + x[8:]
    if name in ("pw_e", "pw_h"):
        none = tuple(a[:0] for a in T["pw"].E)
        out["pw"] = pwm.Tables(none if name == "pw_e" else T["pw"].E, none if name == "pw_h" else T["pw"].H, T["pw"].sig2)
    return out


def set_tables(e, T):
    """The setters of the C ABI, in the order Simulation.build calls them."""
    for name, fn in (("debye", e.set_debye), ("lorentz", e.set_lorentz), ("sheets", e.set_sheets), ("elements", e.set_lumped),
                     ("magnetic", e.set_magnetic), ("conformal", e.set_conformal)):
        if name in T:
            fn(*T[name])
    if "pw" in T:
        e.set_planewave(*T["pw"].args())
    if "excite" in T:
        e.set_excite(*T["excite"])


def twiddles(dt):
    exc = pkg("excitation")
    nsamp = STEPS // EVERY + 1
    return exc.dft_twiddles(FREQS, dt, EVERY, nsamp, 0.0), exc.dft_twiddles(FREQS, dt, EVERY, nsamp, 0.5)


def add_probes_and_boxes(e, dt):
    """The probes and DFT boxes on an engine: (V-probe ids, I-probe ids, V-box ids, I-box ids)."""
    e.set_dft(EVERY, *twiddles(dt))
    vp = [e.add_probe(0, *_list(el), np.array(w, np.float32)) for el, w in V_PROBES]
    ip = [e.add_probe(1, *_list(el), np.array(w, np.float32)) for el, w in I_PROBES]
    return vp, ip, [e.add_dft_box(0, c, lo, hi) for c, lo, hi in V_BOXES], [e.add_dft_box(1, c, lo, hi) for c, lo, hi in I_BOXES]


def _slices(lo, hi, inclusive=False):
    q = 1 if inclusive else 0
    return (slice(lo[2], hi[2] + q), slice(lo[1], hi[1] + q), slice(lo[0], hi[0] + q))


class Ordered:
    """The hand tables stepped by restatement.Restatement (the headers' statement lists in the headers' order on the oracle's
    half-steps), with the probes and DFT sums kept here.  After run(): .fields, .state (the arrays the getters of the C ABI return,
    keyed as `hip_state`), .v_series / .i_series [probe][step] (double), .v_acc / .i_acc the DFT sums of the boxes (complex128
    [2 frequencies] + box shape)."""

    def __init__(self, lib, T, mur=False):
        sim = overlap_sim(mur)
        self.sim, self.T = sim, T
        r = self.r = Restatement(sim, lib, seed=SEED, tables=T, before=self._before)
        e = self.e = r.e
        self.own_v = [e.add_probe(0, *_list(el), np.array(w, np.float32)) for el, w in V_PROBES]
        self.first = next(name for name in E_SIDE if name in r.parts)
        self.tw = twiddles(sim.dt)
        self.v_series = [[] for _ in V_PROBES]
        self.i_series = [[] for _ in I_PROBES]
        self.v_acc = [np.zeros((2,) + tuple(h - l + 1 for l, h in zip(lo[::-1], hi[::-1])), np.complex128) for _, lo, hi in V_BOXES]
        self.i_acc = [np.zeros((2,) + tuple(h - l + 1 for l, h in zip(lo[::-1], hi[::-1])), np.complex128) for _, lo, hi in I_BOXES]

    def _sample(self, kind, Fs):
        series, acc, probes, boxes = ((self.v_series, self.v_acc, V_PROBES, V_BOXES) if kind == 0 else (self.i_series, self.i_acc, I_PROBES, I_BOXES))
        n = self.r.n
        for q, (el, w) in enumerate(probes):
            s = 0.0
            for (c, i, j, k), wq in zip(el, w):
                s = float(np.float32(wq)) * float(Fs[c][k, j, i]) + s
            series[q].append(s)
        if n % EVERY == 0:
            t = self.tw[kind][n // EVERY, :, 0] + 1j * self.tw[kind][n // EVERY, :, 1]
            for q, (c, lo, hi) in enumerate(boxes):
                acc[q] += t[:, None, None, None] * Fs[c][_slices(lo, hi, True)].astype(np.float64)[None]

    def _before(self, name, kind, Fs):
        if name == self.first:
            self._sample(0, Fs)                               # V-probes and V-DFT boxes: in front of every E-side correction

    def step(self):
        self.r.step()
        self._sample(1, self.r.I)                             # I-probes and I-DFT boxes: behind every H-side one

    def run(self, n=STEPS):
        for _ in range(n):
            self.step()
        self.fields = self.e.fields()
        return self

    @property
    def state(self):
        r, out = self.r, {}
        if "debye" in self.T:
            out["debye"] = (r.debye.vprev[2], r.debye.u[2])
        if "lorentz" in self.T:
            out["lorentz"] = (r.lorentz.vprev[0], r.lorentz.x[0])
        if "sheets" in self.T:
            out["sheets"] = (r.sheets.vprev, r.sheets.ib)
        if "elements" in self.T:
            out["elements"] = (r.elements.vprev, r.elements.x)
        if "magnetic" in self.T:
            out["magnetic"] = (r.magnetic.iprev[0], r.magnetic.iprev[1])
        if "conformal" in self.T:
            out["conformal"] = (r.conformal.iprev,)
        return out


def hip_state(e, T):
    """The same arrays through the getters of the C ABI."""
    out = {}
    if "debye" in T:
        out["debye"] = e.debye_state(2)[:2]
    if "lorentz" in T:
        out["lorentz"] = e.lorentz_state(0)[:2]
    if "sheets" in T:
        out["sheets"] = e.sheet_state()
    if "elements" in T:
        out["elements"] = e.lumped_state()
    if "magnetic" in T:
        out["magnetic"] = (e.magnetic_state(0)[0], e.magnetic_state(1)[0])
    if "conformal" in T:
        out["conformal"] = (e.conformal_state(),)
    return out


def compared(r):
    """Everything the GPU test compares, of a finished Ordered run, as one flat list of arrays."""
    out = [r.fields] + [a for k in sorted(r.state) for a in r.state[k]]
    return out + [np.array(s) for s in r.v_series + r.i_series] + r.v_acc + r.i_acc


_REFS = {}


def reference(oracle_lib, mur=False, drop=None):
    """The finished reference run, once per session per (mur, dropped correction), left unchanged."""
    key = (mur, drop)
    if key not in _REFS:
        sim = overlap_sim(mur)
        T = hand_tables(sim.build(oracle_lib).get_operator(), sim.dt)
        _REFS[key] = Ordered(oracle_lib, T if drop is None else dropped(T, drop), mur).run()
    return _REFS[key]
