"""Cases for the plane wave's place in the timestep (CPU: the reference side alone, test_planewave_order_cpu.py; GPU: HIP against it,
test_planewave_order_gpu.py).  fdtd_planewave_set takes any existing edge or face; the scene layer keeps the lists off every probe,
box and grid face, so the cases are hand tables in the style of test_planewave_gpu._hand_tables whose elements are chosen here:

  order scene  test_lumped_model_cpu.pec_cavity(None): about 40 edges and 40 faces inside the nodes [3..10] x [3..9] x [3..8], three
               V-probes / I-probes of one cell and weight 1.0 on listed elements, one V-DFT / I-DFT box over listed and unlisted ones;
  Mur scene    test_sheet_model_cpu.cavity_sim(..., sheet=False, boundary="MUR"): tangential edges on the node plane of each of the six
               faces and on the plane next to it, faces touching those planes, and a handful of both in the middle.

The reference is restatement.Restatement on the oracle from seeded fields, run once per session and left unchanged."""
import numpy as np

from conftest import pkg
from helpers import seeded_fields
from restatement import Restatement
from test_lumped_model_cpu import pec_cavity
from test_sheet_model_cpu import cavity_sim

N = (14, 13, 12)
NSIG2 = 80
ORDER_STEPS, ORDER_SEED, ORDER_BLOCK = 150, 4, ((3, 3, 3), (10, 9, 8))
ORDER_CORNER = ((8, 7, 6), (10, 9, 8))      # the corner of the block farthest from the port, where the port's own field is weakest
EVERY, FREQS = 5, np.array([8e9, 11e9])
MUR_STEPS, MUR_SEED = 120, 6
PORT_CLEAR = ((4, 4, 3), (6, 6, 5))         # the nodes around the port's edge (5, 5, 4): its source and V-probe edge, its I-probe faces


def order_sim():
    return pec_cavity(None, nr_ts=ORDER_STEPS)


def mur_sim():
    return cavity_sim(1.0, 1.0, sheet=False, boundary="MUR", nr_ts=MUR_STEPS)


def flat(i, j, k):
    return (k * N[1] + j) * N[0] + i


def near_port(i, j, k):
    return all(lo <= p <= hi for p, lo, hi in zip((i, j, k), *PORT_CLEAR))


def hand_list(elems, rng):
    """One list of fdtd_planewave_set for the elements [(comp, i, j, k)]: random coefficients of order 1e-3, delays of 0..40 half-steps
    in both terms, fractions in [0, 1), every fourth entry without a second term."""
    n = len(elems)
    idx = np.array([flat(i, j, k) for _, i, j, k in elems], np.int64)
    comp = np.array([c for c, _, _, _ in elems], np.int8)
    coef = (1e-3 * rng.standard_normal((n, 2))).astype(np.float32)
    coef[::4, 1] = 0
    m0 = rng.integers(0, 41, (n, 2)).astype(np.int32)
    w = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    w[w >= 1] = 0
    return idx, comp, coef, m0, w


def _tables(E, H, seed):
    pwm = pkg("planewave")
    rng = np.random.default_rng(seed)
    # the pulse table holds the WHOLE pulse (9 ps per entry; 2 ps, as in test_planewave_gpu, would hold its first 1e-5 only): the
    # additions are then of the order of the coefficients, and whoever samples on the wrong side of a list reads something else
    return pwm.Tables(hand_list(E, rng), hand_list(H, rng), pwm.signal2(10e9, 4e9, 18e-12, NSIG2 // 2))


def subset(tab, keepE=None, keepH=None):
    """The tables with the E / H entries of the boolean masks alone (every kept entry keeps its numbers)."""
    pick = lambda l, keep: l if keep is None else tuple(a[keep] for a in l)
    return pkg("planewave").Tables(pick(tab.E, keepE), pick(tab.H, keepH), tab.sig2)


def elements(l):
    """[(comp, i, j, k)] of a list."""
    k, r = np.divmod(l[0], N[0] * N[1])
    j, i = np.divmod(r, N[0])
    return [(int(c), int(a), int(b), int(d)) for c, a, b, d in zip(l[1], i, j, k)]


# ---- the order scene -------------------------------------------------------------------------------------------------------------------
def order_elements(seed=22, n=40):
    """n edges and n faces drawn from the 81 of the block's far corner, so that a box of a few nodes holds several listed elements.
    (The port drives voltages of 0.5 ... 1 throughout the cavity, the additions are of the order 1e-3: the draw is one whose V box
    changes by more than test_planewave_order_cpu's 1e-3 of its scale across the list; about half of the draws do.)"""
    rng = np.random.default_rng(seed)
    (i0, j0, k0), (i1, j1, k1) = ORDER_CORNER
    every = [(c, i, j, k) for k in range(k0, k1 + 1) for j in range(j0, j1 + 1) for i in range(i0, i1 + 1) for c in range(3) if not near_port(i, j, k)]
    return [sorted(every[q] for q in rng.choice(len(every), n, replace=False)) for _ in range(2)]


def order_tables():
    E, H = order_elements()
    return _tables(E, H, seed=3)


class Order:
    """What the two order tests need of the scene: the tables, per kind (0: V, 1: I) the three probe cells — per component the listed
    element with the largest first coefficient — and the box (component, lo, hi: the nodes around the second probe cell, inside the
    block) with the mask of its listed elements."""

    def __init__(self):
        self.tables = order_tables()
        self.dt = order_sim().dt
        nsamp = ORDER_STEPS // EVERY + 1
        exc = pkg("excitation")
        self.tw = [exc.dft_twiddles(FREQS, self.dt, EVERY, nsamp, 0.0), exc.dft_twiddles(FREQS, self.dt, EVERY, nsamp, 0.5)]
        self.cells, self.box, self.listed = [], [], []
        for l in (self.tables.E, self.tables.H):
            el = elements(l)
            cells = [el[max((q for q in range(len(el)) if el[q][0] == c), key=lambda q: abs(float(l[2][q, 0])))] for c in range(3)]
            c, i, j, k = cells[1]
            lo = tuple(max(p - 1, b) for p, b in zip((i, j, k), ORDER_BLOCK[0]))
            hi = tuple(min(p + 1, b) for p, b in zip((i, j, k), ORDER_BLOCK[1]))
            mask = np.zeros(N[::-1], bool)
            for cc, a, b, d in el:
                if cc == c:
                    mask[d, b, a] = True
            self.cells.append(cells)
            self.box.append((c, lo, hi))
            self.listed.append(mask[self.slices(len(self.box) - 1)])

    def slices(self, kind):
        _, lo, hi = self.box[kind]
        return (slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1), slice(lo[0], hi[0] + 1))

    def probe_args(self, kind):
        """[(idx, comp, w)] of the three one-cell probes."""
        return [(np.array([flat(i, j, k)], np.int64), np.array([c], np.int8), np.array([1.0], np.float32)) for c, i, j, k in self.cells[kind]]


_ORDER_RUN = {}


def order_reference(oracle_lib):
    """The order scene restated on the oracle from seeded fields, once per session.  Per kind: `series[kind][q]` the probed elements'
    values in front of (q = 0) and behind (q = 1) the list, [ORDER_STEPS][3] float32; `acc[kind][q]` the DFT sums of the box from
    those values, complex128 [2 frequencies] + box shape; `own[kind]` the oracle's own probes' series (V: sampled in front of the E
    list; I: in front of the H list); `fields` the final fields."""
    if "run" not in _ORDER_RUN:
        o = Order()
        ref = Restatement(order_sim(), oracle_lib, tables={"pw": o.tables})
        seen = ref.record("pw_e", "pw_h")      # the fields in front of and behind each list of the last timestep
        pids = [[ref.e.add_probe(kind, *a) for a in o.probe_args(kind)] for kind in (0, 1)]
        seeded_fields(ref.e, ORDER_SEED)
        series = [[np.zeros((ORDER_STEPS, 3), np.float32) for _ in range(2)] for _ in range(2)]
        acc = [[np.zeros((2,) + o.listed[kind].shape, np.complex128) for _ in range(2)] for kind in range(2)]
        for n in range(ORDER_STEPS):
            ref.step()
            for kind in (0, 1):
                for q in range(2):
                    F = seen[("pw_e", "pw_h")[kind]][q]
                    series[kind][q][n] = [F[c][k, j, i] for c, i, j, k in o.cells[kind]]
                    if n % EVERY == 0:
                        t = o.tw[kind][n // EVERY, :, 0] + 1j * o.tw[kind][n // EVERY, :, 1]
                        acc[kind][q] += t[:, None, None, None] * F[o.box[kind][0]][o.slices(kind)].astype(np.float64)[None]
        o.series, o.acc = series, acc
        o.own = [np.stack([ref.e.get_probe(p)[:ORDER_STEPS] for p in pids[kind]], axis=1) for kind in (0, 1)]
        o.fields = ref.e.fields()
        _ORDER_RUN["run"] = o
    return _ORDER_RUN["run"]


# ---- the Mur scene ---------------------------------------------------------------------------------------------------------------------
MUR_MIDDLE = ((7, 6, 6), (9, 8, 7))


def mur_elements(seed=12, per=8):
    """(edges, faces): per grid face and per plane — the face's node plane (0 or n - 1) and the plane next to it (1 or n - 2) — `per`
    draws of each tangential edge component on it, the transverse coordinates of the first two anywhere (some land on a second face's
    plane: the grid's own edges);
    faces of every component touching those planes; and the edges and faces of the middle block."""
    rng = np.random.default_rng(seed)
    E, H = set(), set()
    for a in range(3):
        for plane in (0, 1, N[a] - 2, N[a] - 1):
            for c in range(3):
                for d in range(per):
                    # an edge spans one cell along its own axis, a face one cell along both transverse axes; the first two draws
                    # anywhere, the others off the outermost nodes
                    m = 0 if d < 2 else 1
                    pe = [int(rng.integers(m, N[q] - (1 if q == c else 0) - m)) for q in range(3)]
                    pf = [int(rng.integers(m, N[q] - (1 if q != c else 0) - m)) for q in range(3)]
                    pe[a] = plane
                    # a face of the normal component lies in the plane; another one touches it from the node it starts at or one below
                    pf[a] = plane if (c == a or plane <= 1) else plane - 1
                    if c != a:
                        E.add((c, *pe))
                    H.add((c, *pf))
    (i0, j0, k0), (i1, j1, k1) = MUR_MIDDLE
    mid = [(c, i, j, k) for k in range(k0, k1 + 1) for j in range(j0, j1 + 1) for i in range(i0, i1 + 1) for c in range(3)]
    E.update(e for e in mid if sum(e) % 2 == 0)
    H.update(e for e in mid if sum(e) % 2 == 1)
    return sorted(E), sorted(H)


def on_face_plane(el):
    """Per element: does its node lie on the node plane of a grid face (the planner's question of an edge list)?"""
    return np.array([any(p == 0 or p == n - 1 for p, n in zip(e[1:], N)) for e in el], bool)


def in_middle(el):
    return np.array([all(lo <= p <= hi for p, lo, hi in zip(e[1:], *MUR_MIDDLE)) for e in el], bool)


def mur_tables(which="full"):
    """`full`: every element; `middle`: the middle block's alone; `off-face`: the full lists less the EDGES on a face's node plane."""
    E, H = mur_elements()
    full = _tables(E, H, seed=5)
    if which == "full":
        return full
    if which == "middle":
        return subset(full, in_middle(E), in_middle(H))
    assert which == "off-face", which
    return subset(full, ~on_face_plane(E), None)


_MUR_RUNS = {}


def mur_reference(oracle_lib, which="full"):
    """The Mur scene restated on the oracle from seeded fields, MUR_STEPS timesteps, once per session per table set: the final fields."""
    if which not in _MUR_RUNS:
        ref = Restatement(mur_sim(), oracle_lib, tables={"pw": mur_tables(which)})
        seeded_fields(ref.e, MUR_SEED)
        ref.run(MUR_STEPS)
        f = ref.e.fields()
        f.setflags(write=False)
        _MUR_RUNS[which] = f
        ref.e.close()
    return _MUR_RUNS[which]
