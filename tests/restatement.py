"""The reference for the eight step-loop corrections: Debye media, Lorentz / Drude media, conducting sheets, lumped elements, magnetic
faces, conformal faces, the plane wave and the H-field excitations.  oracle/fdtd_oracle.c has none of them, so the parity tests compare
the HIP library, bit for bit, with the oracle's half-steps and the float32 statement lists of dispersion.py, lorentz.py, sheet.py,
lumped.py, magnetic.py, conformal.py, planewave.py and excite_cases.HLists (the numpy statement of include/fdtd_hip_excite.h) applied in
numpy between them, in the order include/fdtd_hip_*.h give.  That order is ORDER, stated here
once; Restatement.step reads top to bottom as the headers do:

    half_step(E)        (the oracle samples its V-probes and V boxes here, in front of every E-side correction)
    read V
    Debye -> Lorentz -> sheets -> elements -> plane wave (edge list)
    write V back
    half_step(H)
    read I
    magnetic -> conformal (reads the V just written) -> plane wave (face list) -> H-field excitations
    write I back; sample the kept I-probes

It holds for any tables the setters of the C ABI accept, overlapping ones included (corrections_overlap_cases.py)."""
import contextlib
import ctypes

import numpy as np

from conftest import pkg
from helpers import seeded_fields

ORDER = ("debye", "lorentz", "sheets", "elements", "pw_e", "magnetic", "conformal", "pw_h", "excite")
E_SIDE, H_SIDE = ORDER[:5], ORDER[5:]
# what a Simulation holds of each correction, and the _capi question whether a library can step it
HELD = {"debye": lambda s: s.debye is not None, "lorentz": lambda s: s.lorentz is not None, "sheets": lambda s: s.sheets is not None,
        "elements": lambda s: s.element_stepped.size > 0, "magnetic": lambda s: s.magnetic is not None,
        "conformal": lambda s: s.conformal is not None, "pw": lambda s: s.plane_wave is not None,
        "excite": lambda s: s.excite_h_args is not None}
HAS = {"debye": "has_dispersion", "lorentz": "has_lorentz", "sheets": "has_sheets", "elements": "has_lumped", "magnetic": "has_magnetic",
       "conformal": "has_conformal", "pw": "has_planewave", "excite": "has_excite"}


@contextlib.contextmanager
def corrections_hidden(sim):
    """`sim` without its eight corrections, so that sim.build makes the folded / base operator alone: the oracle has no setter for any.
    (The E side of a field excitation is source lists and operator overrides, which the oracle has: it stays.)"""
    saved = {k: getattr(sim, k) for k in ("debye", "lorentz", "sheets", "element_stepped", "magnetic", "conformal", "plane_wave", "excite_h_args")}
    for k in saved:
        setattr(sim, k, np.zeros(0, np.int64) if k == "element_stepped" else None)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(sim, k, v)


def _slices(lo, hi):
    return (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))


# ---- the corrections: tables in the layout the numpy statement functions take, states, apply (and reprime for i_prev) ---------------
class _Boxes:
    """A dense E-side correction: per component a box of edges with their vi, weights w, medium rows `tab`, v_prev and branch states x.
    `rows`: the per-medium tables [medium] + row shape; edges the operator holds at zero (vi == 0: grid faces, metal) get w = 0, as
    in the setters."""

    def __init__(self, r, rows, lo, hi, w, med):
        ty, vi_all = r.ty, r.vi()
        rows = [np.asarray(t) for t in rows]
        self.sl, self.vi, self.w, self.tab, self.x, self.vprev = [], [], [], [], [], []
        for c in range(3):
            sl = _slices(lo[c], hi[c])
            shape = tuple(max(s.stop - s.start, 0) for s in sl)
            empty = 0 in shape
            vi = np.zeros(shape, ty) if empty else vi_all[c][sl].astype(ty)
            m = np.zeros(shape, np.int64) if (empty or med is None) else np.asarray(med[c], np.int64).reshape(shape)
            self.sl.append(sl)
            self.vi.append(vi)
            self.w.append(np.zeros(shape, ty) if empty else np.where(vi == 0, ty(0), np.asarray(w[c], ty).reshape(shape)))
            self.tab.append(tuple(np.moveaxis(t[m], tuple(range(1 - t.ndim, 0)), tuple(range(t.ndim - 1))).astype(ty, order="C") for t in rows))   # row shape + box shape
            self.x.append(np.zeros(rows[1].shape[1:] + shape, ty))
            self.vprev.append(np.zeros(shape, ty))
        # which states have been off zero at a checkpoint (Restatement.note_moved): "the wave reached this edge".  Asked at checkpoints and
        # not of the final values alone because a + b of a state update cancels to exactly 0.0f about once in 2^24 state updates — twice
        # in 800 drawn cases of ~5e7 states (one step earlier and later the state was ~5e-6).
        self.x_moved = [np.zeros(x.shape, bool) for x in self.x]
        self.vprev_moved = [np.zeros(v.shape, bool) for v in self.vprev]

    def apply(self, F, r):
        for c in range(3):
            if self.w[c].size:
                F[c][self.sl[c]] = self.statements(F[c][self.sl[c]], self.vi[c], self.w[c], self.vprev[c], self.x[c], *self.tab[c])

    def note_moved(self):
        for c in range(3):
            self.x_moved[c] |= self.x[c] != 0
            self.vprev_moved[c] |= self.vprev[c] != 0


class Debye(_Boxes):
    """(alpha, oma, beta, lo, hi, w, med) of fdtd_debye_set; the branch states are .u (= .x) [K] + box shape."""

    def __init__(self, r, alpha, oma, beta, lo, hi, w, med=None):
        super().__init__(r, (alpha, oma, beta), lo, hi, w, med)
        self.statements, self.u, self.u_moved = pkg("dispersion").correction, self.x, self.x_moved


class Lorentz(_Boxes):
    """(phi, gam, h, lo, hi, w, med) of fdtd_lorentz_set; the branch states are .x [K][2] + box shape."""

    def __init__(self, r, phi, gam, h, lo, hi, w, med=None):
        super().__init__(r, (phi, gam, h), lo, hi, w, med)
        self.statements, self.K = pkg("lorentz").correction, np.asarray(phi).shape[1]


class _Listed:
    """A listed E-side correction: edges (idx, comp) with their vi and v_prev."""

    def __init__(self, idx, comp, vi):
        self.idx, self.comp, self.vi = np.asarray(idx, np.int64), np.asarray(comp, np.int8), np.asarray(vi, np.float32)
        self.by_c = [np.nonzero(self.comp == c)[0] for c in range(3)]
        self.vprev = np.zeros(self.idx.size, np.float32)

    def apply(self, F, r):
        V = np.empty(self.idx.size, np.float32)
        for c in range(3):
            V[self.by_c[c]] = F[c].reshape(-1)[self.idx[self.by_c[c]]]
        v = self.vprev = self.statements(V)
        for c in range(3):
            F[c].reshape(-1)[self.idx[self.by_c[c]]] = v[self.by_c[c]]


class Sheets(_Listed):
    """(idx, comp, vi, cls, alpha, b) of fdtd_sheet_set; the branch currents are .ib [K][n]."""

    def __init__(self, r, idx, comp, vi, cls, alpha, b):
        super().__init__(idx, comp, vi)
        cls = np.asarray(cls, np.int64)
        self.al, self.b = np.asarray(alpha, np.float32)[cls].T.copy(), np.asarray(b, np.float32)[cls].T.copy()
        self.ib = np.zeros((self.al.shape[0], self.idx.size), np.float32)
        self.ib_moved = np.zeros(self.ib.shape, bool)

    def statements(self, V):
        return pkg("sheet").correction(V, self.vi, self.vprev, self.ib, self.al, self.b)

    def note_moved(self):
        self.ib_moved |= self.ib != 0


class Elements(_Listed):
    """(idx, comp, vi, cls, phi, gam, h) of fdtd_lumped_set; the branch states are .x [2][n]."""

    def __init__(self, r, idx, comp, vi, cls, phi, gam, h):
        super().__init__(idx, comp, vi)
        cls = np.asarray(cls, np.int64)
        self.phi = np.moveaxis(np.asarray(phi, np.float32)[cls], 0, -1).copy()
        self.gam, self.h = np.asarray(gam, np.float32)[cls].T.copy(), np.asarray(h, np.float32)[cls].T.copy()
        self.x = np.zeros((2, self.idx.size), np.float32)

    def statements(self, V):
        return pkg("lumped").correction(V, self.vi, self.vprev, self.x, self.phi, self.gam, self.h)


class Magnetic:
    """(a, b, lo, hi, cls) of fdtd_magnetic_set.  i_prev is loaded from the I arrays when the set is made and again by set_field(1, ...),
    as include/fdtd_hip_magnetic.h promises."""

    def __init__(self, r, ta, tb, lo, hi, cls):
        self.ta, self.tb = np.asarray(ta, np.float32), np.asarray(tb, np.float32)
        self.sl = [_slices(lo[c], hi[c]) for c in range(3)]
        self.cls = [np.asarray(cls[c], np.uint8).reshape([s.stop - s.start for s in self.sl[c]]) for c in range(3)]
        self.iprev = [None] * 3
        for c in range(3):
            self.reprime(c, r.e.get_field(1, c))

    def reprime(self, comp, a):
        self.iprev[comp] = np.asarray(a, np.float32)[self.sl[comp]].copy()

    def apply(self, F, r):
        for c in range(3):
            if self.cls[c].size:
                F[c][self.sl[c]] = pkg("magnetic").correction(F[c][self.sl[c]], self.iprev[c], self.cls[c], self.ta, self.tb)


class Conformal:
    """(comp, idx, coef) of fdtd_conformal_set; i_prev [n] as for the magnetic faces.  Reads the voltages written back in front of the H
    half-step, i.e. behind every E-side correction."""

    def __init__(self, r, comp, idx, coef):
        self.comp, self.idx = np.asarray(comp, np.int64), np.asarray(idx, np.int64)
        self.coef = np.asarray(coef, np.float32).reshape(-1, 4)
        self.iprev = np.zeros(self.idx.size, np.float32)
        for c in range(3):
            self.reprime(c, r.e.get_field(1, c))

    def reprime(self, comp, a):
        q = self.comp == comp
        self.iprev[q] = np.asarray(a, np.float32).reshape(-1)[self.idx[q]]

    def apply(self, F, r):
        new = pkg("conformal").correction(np.stack(r.V), self.iprev, self.comp, self.idx, self.coef)
        for c in range(3):
            q = self.comp == c
            if q.any():
                F[c].reshape(-1)[self.idx[q]] = new[q]


class PlaneWaveList:
    """One of the two lists of planewave.Tables (kind 0: the edge list, 1: the face list) at timestep r.n."""

    def __init__(self, tables, kind):
        self.tables, self.kind = tables, kind

    def apply(self, F, r):
        pkg("planewave").apply(F, self.tables, r.n, self.kind)


class Excite:
    """The nine arguments of fdtd_excite_set (the hard list, the soft list, sigH) at timestep r.n; .lists is the excite_cases.HLists whose
    apply is the numpy statement of include/fdtd_hip_excite.h.  No state."""

    def __init__(self, r, *args):
        from excite_cases import HLists
        assert len(args) == 9
        self.lists = HLists(args[0:4], args[4:8], args[8])

    def apply(self, F, r):
        self.lists.apply(F, r.n)


# ---- the stepper ----------------------------------------------------------------------------------------------------------------------
class Restatement:
    """An engine of `lib` (the oracle: no correction entry points needed) built from `sim` with its corrections hidden and stepped by
    half-steps, with the corrections applied in numpy in ORDER.  Each is an object above, None where absent: .debye, .lorentz, .sheets,
    .elements, .magnetic, .conformal, .excite, and .pw_e / .pw_h for the plane wave's two lists.
    `tables`: {name: the argument tuple of the C ABI setter} for "debye", "lorentz", "sheets", "elements", "magnetic", "conformal",
    "excite", and "pw": planewave.Tables.  A correction not named there takes the simulation's own tables, if the simulation holds it.
    `seed`: seeded noise in all six field components (helpers.seeded_fields) in front of priming i_prev; the other states start at zero.
    `before`, `after`: hooks called with (name, kind, fields) in front of and behind each correction held; `fields` are the three live
    arrays of that kind (0: V, 1: I) — copy what you keep (record() does).  After a step .V and, with an H-side correction, .I hold the
    fields as written back.
    The oracle samples its I-probes inside the H half-step, in front of the H-side corrections, so with magnetic or conformal faces or
    H-field excitations the I-probe series are kept here — sum_e w_e I_e in double in the probe's edge order: the products are exact in double, so this is the
    oracle's fma chain — and get_probe returns them; otherwise it returns the oracle's own.
    `f64`: the double-precision oracle library when `lib` is that one — fields and vi go through its double entry points and the
    correction runs in float64, on the simulation's float32-rounded tables (`round32`) or on the float64 ones; Lorentz media only."""

    def __init__(self, sim, lib, *, flags=0, seed=None, tables=None, before=None, after=None, f64=None, round32=True):
        self.sim, self.f64, self.before, self.after = sim, f64, before, after
        self.ty = np.float32 if f64 is None else np.float64
        with corrections_hidden(sim):
            e = self.e = sim.build(lib, flags=flags)
        if f64 is not None:
            assert lib is f64
            for fn in (f64.fdtd_oracle_get_field_f64, f64.fdtd_oracle_set_field_f64):
                fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
            f64.fdtd_oracle_get_operator_f64.restype, f64.fdtd_oracle_get_operator_f64.argtypes = ctypes.c_int, [ctypes.c_void_p] * 5
        if seed is not None:
            seeded_fields(e, seed)
        own = {"debye": sim.debye_tables, "lorentz": sim.lorentz_tables, "sheets": sim.sheet_tables, "elements": sim.lumped_tables,
               "magnetic": lambda: sim.magnetic.tables(), "conformal": sim.conformal_tables, "pw": self._planewave_tables,
               "excite": lambda: sim.excite_h_args}
        if f64 is not None and not round32:
            d = sim.lorentz
            own["lorentz"] = lambda: pkg("lorentz").tables(d.media, sim.dt, dtype=np.float64) + (d.lo, d.hi, d.w, d.med)
        given = dict(tables or {})
        T = {k: given[k] if k in given else own[k]() for k in own if k in given or HELD[k](sim)}
        assert f64 is None or set(T) <= {"lorentz"}
        make = {"debye": Debye, "lorentz": Lorentz, "sheets": Sheets, "elements": Elements, "magnetic": Magnetic, "conformal": Conformal,
                "excite": Excite}
        self.parts = {}
        for name in ORDER:
            key = "pw" if name in ("pw_e", "pw_h") else name
            part = None
            if key in T:
                part = PlaneWaveList(T["pw"], int(name == "pw_h")) if key == "pw" else make[name](self, *T[name])
                self.parts[name] = part
            setattr(self, name, part)
        if self.debye and self.lorentz and "debye" not in given and "lorentz" not in given:      # the scene layer refuses a shared edge
            for c in range(3):
                both = np.zeros(e.local_shape, bool)
                both[self.debye.sl[c]] = self.debye.w[c] != 0
                assert not np.any(both[self.lorentz.sl[c]] & (self.lorentz.w[c] != 0))
        self.i_probes, self.i_series = {}, {}
        for p, (_, iid) in zip(sim.vox.ports, sim._port_probe_ids):
            self.i_probes[iid] = (np.asarray(p.i_idx, np.int64), np.asarray(p.i_comp, np.int64), np.asarray(p.i_w, np.float32))
        self.nstep = 0
        self.engine = _Engine(self)

    def _planewave_tables(self):
        op = self.e.get_operator()
        return pkg("planewave").tables(self.sim.grid, self.sim.plane_wave, self.sim.dt, op[1], op[3], self.sim.signal2)

    # -- fields and vi in the restatement's precision
    def get(self, kind, c):
        if self.f64 is None:
            return self.e.get_field(kind, c)
        out = np.zeros(self.e.local_shape, np.float64)
        assert self.f64.fdtd_oracle_get_field_f64(self.e._ctx, kind, c, out.ctypes.data) == 0
        return out

    def put(self, kind, c, a):
        if self.f64 is None:
            return self.e.set_field(kind, c, a)
        a = np.ascontiguousarray(a, np.float64)
        assert self.f64.fdtd_oracle_set_field_f64(self.e._ctx, kind, c, a.ctypes.data) == 0

    def vi(self):
        if self.f64 is None:
            return self.e.get_operator()[1]
        out = [np.zeros((3,) + self.e.local_shape, np.float64) for _ in range(4)]
        assert self.f64.fdtd_oracle_get_operator_f64(self.e._ctx, *[a.ctypes.data for a in out]) == 0
        return out[1]

    # -- what the C ABI offers and the corrections change
    def set_field(self, kind, comp, a):
        """fdtd_set_field, with the re-priming of i_prev the headers promise for FDTD_KIND_I."""
        self.e.set_field(kind, comp, a)
        if kind == 1:
            for part in (self.magnetic, self.conformal):
                if part is not None:
                    part.reprime(comp, a)

    def add_probe(self, kind, idx, comp, w):
        pid = self.e.add_probe(kind, idx, comp, w)
        if kind == 1:
            self.i_probes[pid] = (np.asarray(idx, np.int64), np.asarray(comp, np.int64), np.asarray(w, np.float32))
        return pid

    def get_probe(self, pid):
        if pid in self.i_probes and (self.magnetic or self.conformal or self.excite):
            return np.array(self.i_series.get(pid, []), np.float64)
        return self.e.get_probe(pid)

    def record(self, *names):
        """Hooks that keep copies of the fields around the named corrections: the returned dict holds name -> [fields in front of it,
        fields behind it] of the last step."""
        seen = {}

        def before(name, kind, F):
            if name in names:
                seen[name] = [[a.copy() for a in F], None]

        def after(name, kind, F):
            if name in names:
                seen[name][1] = [a.copy() for a in F]
        self.before, self.after = before, after
        return seen

    def _apply(self, names, kind, F):
        held = [name for name in names if name in self.parts]
        for name in held:
            if self.before is not None:
                self.before(name, kind, F)
            self.parts[name].apply(F, self)
            if self.after is not None:
                self.after(name, kind, F)
        for c in range(3 if held else 0):
            self.put(kind, c, F[c])

    def step(self):
        e = self.e
        e.half_step(0)
        self.n = int(e.step)
        self.V = [self.get(0, c) for c in range(3)]
        self._apply(E_SIDE, 0, self.V)
        e.half_step(1)
        if any(name in self.parts for name in H_SIDE):
            self.I = [self.get(1, c) for c in range(3)]
            self._apply(H_SIDE, 1, self.I)
        if self.magnetic or self.conformal or self.excite:      # behind every H-side correction, the excitations included
            for pid, (idx, comp, w) in self.i_probes.items():
                s = 0.0
                for g, c, wq in zip(idx, comp, w):
                    s = float(wq) * float(self.I[c].reshape(-1)[g]) + s
                self.i_series.setdefault(pid, []).append(s)
        self.nstep += 1
        if self.nstep == 1 or self.nstep % 8 == 0:
            self.note_moved()

    def run(self, n):
        for _ in range(int(n)):
            self.step()
        self.note_moved()

    def note_moved(self):
        """The checkpoints of the *_moved masks: after the first step, every eighth, the end of every run()."""
        for part in self.parts.values():
            if hasattr(part, "note_moved"):
                part.note_moved()


class _Engine:
    """What a Simulation keeps as its engine (install): the oracle's engine, with run, set_field and the probes going through the
    restatement."""

    def __init__(self, r):
        self._r = r
        self.run, self.set_field, self.add_probe, self.get_probe = r.run, r.set_field, r.add_probe, r.get_probe

    def __getattr__(self, name):
        return getattr(self._r.e, name)


def install(monkeypatch, tables=None):
    """Simulation.build -> the restatement's engine when the simulation holds a correction whose entry points the library lacks (the
    oracle), the real build otherwise: the checker of the plugin-level tests.  The restatement is sim.restated.
    `tables(sim)`: raw tables that replace the simulation's own (Restatement's `tables`)."""
    Sim = pkg("simulation").Simulation
    orig = Sim.build

    def build(self, lib, **kw):
        capi = pkg("_capi")
        if not any(held(self) and not getattr(capi, HAS[name])(lib) for name, held in HELD.items()):
            return orig(self, lib, **kw)
        r = Restatement(self, lib, flags=kw.get("flags", 0), tables=None if tables is None else tables(self))
        for name, pl in self.probes.items():          # the stand-alone current probes: kept like the ports' (sampled behind the H side)
            if pl.kind == 1:
                for pid, q in zip(self._probe_ids[name], pl.lists):
                    r.i_probes[pid] = (np.asarray(q.idx, np.int64), np.asarray(q.comp, np.int64), np.asarray(q.w, np.float32))
        self.engine, self.lib = r.engine, lib
        self.rank, self.world, self.device, self._build_flags = 0, 1, 0, 0
        if r.pw_e is not None:
            self.planewave_tables = r.pw_e.tables
        self.restated = r
        return r.engine
    monkeypatch.setattr(Sim, "build", build)
