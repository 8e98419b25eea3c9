"""Lumped R-L-C elements (lumped.py, scene.add_lumped_element): the discretisation's algebra, the admittance an element presents to
the engine's edge, stability and passivity, what folds into the operator alone, the voxeliser's geometry and refusals, and the API
mirror.  The per-timestep correction is restated in numpy (lumped.correction) on top of the oracle's half-steps — the oracle knows
nothing of elements — behind the corrections of the Debye media and the sheets (restatement.Restatement), which is also what the GPU
tests compare the HIP path with, bit for bit."""
import os

import numpy as np
import pytest

from conftest import ROOT, pkg
from restatement import Restatement
from test_dispersion_model_cpu import _discrete_energy, _edge_CL
from test_sheet_model_cpu import _grid

EPS0 = pkg("constants").EPS0


def _lumped():
    return pkg("lumped")


# ---- discretisation algebra ----------------------------------------------------------------------------------------------------
def _case_table(rng):
    E = _lumped().Element
    u = lambda lo, hi: float(np.exp(rng.uniform(np.log(lo), np.log(hi))))
    cases = []
    for _ in range(3):
        R, L, C = u(1, 1e3), u(1e-10, 1e-8), u(1e-14, 1e-11)
        cases += [("par R", E("e", R=R)), ("par C", E("e", C=C)), ("par L", E("e", L=L)), ("par RLC", E("e", R=R, L=L, C=C)),
                  ("par LC", E("e", L=L, C=C)), ("ser RLC", E("e", R=R, L=L, C=C, kind="series")),
                  ("ser LC", E("e", L=L, C=C, kind="series")), ("ser RL", E("e", R=R, L=L, kind="series")),
                  ("ser L", E("e", L=L, kind=1)), ("ser RC", E("e", R=R, C=C, kind="series")), ("ser R", E("e", R=R, kind="series")),
                  ("ser C", E("e", C=C, kind="series")), ("ser RLC split", E("e", R=R, L=L, C=C, kind="series", n_ser=3, n_par=4))]
    cases += [("ser LC stiff", E("e", L=1e-13, C=1e-16, kind="series")), ("par LC stiff", E("e", L=1e-13, C=1e-16)),
              ("ser RLC high Q", E("e", R=0.5, L=2e-9, C=1e-12, kind="series"))]
    return cases


def test_discretisation_equals_the_warped_admittance():
    lm = _lumped()
    dt = 1.9e-12
    wdt = np.linspace(0.01, 0.3, 30)
    f = wdt / (2 * np.pi * dt)
    nstates = {"par R": 0, "par C": 0, "par L": 1, "par RLC": 1, "par LC": 1, "ser RLC": 2, "ser LC": 2, "ser RL": 1, "ser L": 1, "ser RC": 1,
               "ser R": 0, "ser C": 0, "ser RLC split": 2, "ser LC stiff": 2, "par LC stiff": 1, "ser RLC high Q": 2}
    for name, el in _case_table(np.random.default_rng(11)):
        Phi, Gam, h, g0, G, C = el.discretise(dt)
        assert el.nstates == nstates[name], name
        assert g0 >= 0 and G >= 0 and C >= 0, name
        assert np.max(np.abs(np.linalg.eigvals(Phi))) <= 1 + 1e-12, name
        if el.nstates < 2:
            assert not Phi[1].any() and not Phi[:, 1].any() and Gam[1] == 0 and h[1] == 0, name
        s_d = 1j * (2 / dt) * np.tan(0.5 * wdt)
        got = lm.transfer(Phi, Gam, h, g0, f, dt) + G + s_d * C
        want = el.admittance_discrete(f, dt)
        assert np.max(np.abs(got - want) / np.abs(want)) <= 1e-12, (name, np.max(np.abs(got - want) / np.abs(want)))
        # the warped frequency tends to the true one: Y(s_d) -> Y(jw) as w dt -> 0
        lo = 1e-4 / (2 * np.pi * dt)
        assert abs(el.admittance_discrete(lo, dt)[0] / el.admittance(lo)[0] - 1) < 1e-6, name
    e = lm.Element("lc", L=2e-9, C=1e-12, kind="series", n_ser=2, n_par=3)
    assert abs(e.resonance() - 1 / (2 * np.pi * np.sqrt(2e-21))) < 1 and e.resonance(dt) < e.resonance()
    fr = e.resonance(dt)             # the stepped branch resonates there: its susceptance changes sign
    assert e.admittance_discrete(0.999 * fr, dt)[0].imag > 0 > e.admittance_discrete(1.001 * fr, dt)[0].imag


def test_refused_values():
    E = _lumped().Element
    for kw in (dict(R=-1.0), dict(L=float("inf")), dict(C=-1e-12), dict(), dict(R=0.0), dict(L=0.0), dict(kind="series"),
               dict(kind="series", R=0.0), dict(kind="series", R=5.0, C=0.0), dict(kind="delta", R=1.0), dict(R=1.0, n_ser=0)):
        with pytest.raises(ValueError, match="'bad'"):
            E("bad", **kw)
    assert E("ok", R=float("nan"), C=1e-12).R is None


# ---- the float64 line: the algebra of lumped.correction ------------------------------------------------------------------------
def _line_admittance(el, steps=40000, N=200):
    """A 1-D leapfrog line (50 ohm, 0.99 of its Courant limit) in float64, fed through 50 ohm at one end and terminated by the element
    through lumped.correction: the admittance measured at the last node minus the edge's own s_d C + G, against Y(s_d)."""
    lm = _lumped()
    L0, C0 = 2.5e-10, 1e-13
    dt = 0.99 * np.sqrt(L0 * C0)
    Phi, Gam, h, g0, Gf, Cf = el.discretise(dt)
    V, I = np.zeros(N), np.zeros(N + 1)
    Ce, G = np.full(N, C0), np.zeros(N)
    e = N - 1
    Ce[e] += Cf; G[e] += Gf + g0; G[0] += 1 / 50.0
    x_ = 0.5 * dt * G / Ce
    vv, vi = (1 - x_) / (1 + x_), dt / (Ce * (1 + x_))
    f0, fc = 3e9, 2e9
    t = np.arange(steps) * dt
    sig = np.exp(-((t - 4 / fc) * fc * 1.5) ** 2) * np.cos(2 * np.pi * f0 * t)
    x, vprev = np.zeros((2, 1)), np.zeros(1)
    phi, gam, hh = Phi.reshape(2, 2, 1), Gam.reshape(2, 1), h.reshape(2, 1)
    Vm, Ic = np.zeros(steps), np.zeros(steps)
    for s in range(steps):
        curl = I[:-1] - I[1:]
        V = vv * V + vi * curl
        V[0] += vi[0] * sig[s] / 50.0
        v = lm.correction(V[e:e + 1], vi[e:e + 1], vprev, x, phi, gam, hh)
        Vm[s], Ic[s] = 0.5 * (v[0] + vprev[0]), curl[e]
        V[e], vprev = v[0], v
        I[1:-1] += (dt / L0) * (V[:-1] - V[1:])
    assert abs(Vm[-1]) < 1e-9 * np.abs(Vm).max()
    fs = np.linspace(1.5e9, 4.5e9, 7)
    n = np.arange(steps)
    F = lambda a: np.array([np.sum(a * np.exp(-2j * np.pi * f * dt * n)) for f in fs])
    s_d = 1j * (2 / dt) * np.tan(np.pi * fs * dt)
    return F(Ic) / F(Vm) - (s_d * C0), el.admittance_discrete(fs, dt)


def test_correction_in_float64_presents_the_warped_admittance():
    E = _lumped().Element
    for el in (E("a", R=300.0, L=3e-9, C=1e-12), E("b", R=5.0, L=2e-9, C=1e-12, kind="series"), E("c", R=30.0, C=2e-12, kind="series")):
        got, want = _line_admittance(el)
        err = float(np.max(np.abs(got - want) / np.abs(want)))
        print(f"float64 line, {el.kind} R={el.R} L={el.L} C={el.C}: |Y - Y(s_d)| / |Y(s_d)| <= {err:.2e}")
        assert err <= 1e-9


# ---- admittance identity on the engine -----------------------------------------------------------------------------------------
IDENTITY_CASES = [("parallel R||L||C", dict(R=200.0, L=2e-9, C=0.3e-12, kind="parallel")),
                  ("series R-L-C underdamped", dict(R=10.0, L=3e-9, C=0.2e-12, kind="series")),
                  ("series R-C", dict(R=50.0, C=0.5e-12, kind="series"))]
# the bar: ten times the worst case measured once on the CPU oracle (profiles/lumped/admittance_identity.txt) — rounding of a
# fp32 recursion of a few thousand timesteps varies by about that between scenes
IDENTITY_WORST_MEASURED = 2.25e-5
IDENTITY_BAR = 10 * IDENTITY_WORST_MEASURED


def _identity_sim(element, nr_ts=6000):
    sc, sim = pkg("scene"), pkg("simulation")
    g = _grid((20, 18, 16))
    s = sc.Scene(unit=1e-3)
    s.add_lumped_port(1, 50.0, [7, 9, 7], [7, 9, 9], "z", 1.0)
    if element is not None:
        s.add_lumped_element("el", "z", **element).add_box([10, 9, 8], [10, 9, 9])
    return sim.Simulation(g, sc.voxelize(s, g), f0=6e9, fc=4e9, boundary="CPML", cpml_cells=4, nr_ts=nr_ts, end_criteria=0.0)


def measure_identity(lib, element):
    """(frequencies, measured F(curl)/F(Vm) - (s_d C0 + G0), Y(s_d), Y(jw), timesteps) at the element edge (10, 9, 8) z."""
    i, j, k = 10, 9, 8
    bare = _identity_sim(None)
    op = bare.op
    vv0, vi0 = float(op.vv[2][k, j, i]), float(op.raw()[1][2][k, j, i])
    run = _identity_sim(element)
    dt = run.dt
    C0 = dt * (1 + vv0) / (2 * vi0)
    G0 = 2 * C0 * (1 - vv0) / (1 + vv0) / dt
    r = Restatement(run, lib)
    assert r.elements is not None and r.elements.idx.size == 1
    curl, vm, up = [], [], []
    vold, peak = 0.0, 0.0
    for n in range(run.nr_ts):
        Ix, Iy = r.e.get_field(1, 0), r.e.get_field(1, 1)
        curl.append((float(Iy[k, j, i]) - float(Iy[k, j, i - 1])) - (float(Ix[k, j, i]) - float(Ix[k, j - 1, i])))
        r.step()
        v = float(r.V[2][k, j, i])
        vm.append(0.5 * (v + vold))
        vold = v
        u = abs(sum(float(r.V[2][kk, 9, 7]) for kk in (7, 8)))        # the port voltage (its probe line)
        up.append(u)
        peak = max(peak, u)
        # ... and the element's own ringing 100 dB below ITS peak: what is cut off leaks into the transforms
        if n > len(run.signal) and n % 50 == 0 and max(up[-50:]) < 1e-3 * peak and \
                np.abs(vm[-50:]).max() < 1e-5 * np.abs(vm).max() and np.abs(curl[-50:]).max() < 1e-5 * np.abs(curl).max():
            break
    assert max(up[-50:]) < 1e-3 * peak, "the port voltage has not fallen 60 dB below its peak"
    curl, vm = np.array(curl), np.array(vm)
    assert np.abs(vm[-50:]).max() < 1e-5 * np.abs(vm).max() and np.abs(curl[-50:]).max() < 1e-5 * np.abs(curl).max()
    fs = np.linspace(run.f0 - 0.75 * run.fc, run.f0 + 0.75 * run.fc, 7)
    t = np.arange(curl.size)
    F = lambda a: np.array([np.sum(a * np.exp(-2j * np.pi * f * dt * t)) for f in fs])
    s_d = 1j * (2 / dt) * np.tan(np.pi * fs * dt)
    el = run.elements.elements[0]
    return fs, F(curl) / F(vm) - (s_d * C0 + G0), el.admittance_discrete(fs, dt), el.admittance(fs), curl.size


@pytest.mark.parametrize("name,element", IDENTITY_CASES, ids=[c[0] for c in IDENTITY_CASES])
def test_admittance_identity_on_the_engine(oracle_lib, name, element):
    fs, got, want, cont, steps = measure_identity(oracle_lib, element)
    err = np.abs(got - want) / np.abs(want)
    print(f"{name}: {steps} timesteps; |Y_measured - Y(s_d)| / |Y(s_d)| per frequency {np.array2string(err, precision=2)}; "
          f"against the continuous Y(jw) {np.array2string(np.abs(got - cont) / np.abs(cont), precision=2)}")
    assert float(err.max()) <= IDENTITY_BAR, (name, float(err.max()))


# ---- stability -----------------------------------------------------------------------------------------------------------------
def pec_cavity(add=None, *, n=(14, 13, 12), nr_ts=20000, f0=10e9, fc=4e9, boundary="PEC", use_classes=True):
    """The PEC cavity of test_sheet_model_cpu.cavity_sim without sheets (metal walls one cell inside the grid faces, a 0-ohm soft
    source inside); `add(scene)` draws the elements.  The excitation is the Gauss pulse under a Hann window, less the multiple of that
    window that makes it sum to zero.  As it comes, the truncated pulse sums to 1e-3 of its peak and ends in steps of 1e-4: the 0-ohm
    source would leave a static charge behind, whose field no series capacitor lets through, and ring the grid-scale modes of the cavity,
    which no edge in its middle couples to — below the cavity's cut-off those two would be most of what it holds."""
    sc, sim = pkg("scene"), pkg("simulation")
    g = _grid(n)
    s = sc.Scene(unit=1e-3)
    lo, hi = (2, 2, 2), (n[0] - 3, n[1] - 3, n[2] - 3)
    for a in range(3):
        for side in (lo[a], hi[a]):
            st, sp = list(lo), list(hi)
            st[a] = sp[a] = side
            s.add_metal(f"w{a}{side}").add_box(st, sp)
    s.add_lumped_port(1, 0.0, [5, 5, 4], [5, 5, 5], "z", 1.0)
    if add is not None:
        add(s)
    run = sim.Simulation(g, sc.voxelize(s, g), f0=f0, fc=fc, boundary=boundary, nr_ts=nr_ts, end_criteria=0.0, use_classes=use_classes)
    win = np.hanning(len(run.signal) + 2)[1:-1]
    sig = run.signal.astype(np.float64) * win
    run.signal = (sig - sig.sum() * win / win.sum()).astype(np.float32)
    return run


def _one_element(kind, L, C, R=None):
    return lambda s: s.add_lumped_element("el", "z", R=R, L=L, C=C, kind=kind).add_box([7, 6, 5], [7, 6, 6])


def _energy_series(run, lib, nsteps, every=10):
    """(energies, element energies, restatement): the conserved leapfrog energy 1/2 V C V + 1/2 I^{n+1/2} L I^{n-1/2} (C with the folded
    capacitors: 1/2 C_fold V^2) plus the elements' stored energy, every `every` timesteps from the end of the source on."""
    lm = _lumped()
    C, L = _edge_CL(run.grid, run.vox.eps_r)
    weights = None
    if run.elements is not None:
        el = run.elements
        for le in run.element_lumped:
            C[le.comp, le.k, le.j, le.i] += le.C
        weights = np.stack([el.elements[m].energy_weights() for m in el.elem[run.element_stepped]], axis=1)
    r = Restatement(run, lib)
    stop = len(run.signal) + 1
    r.run(stop)
    en, en_el = [], []
    for n in range(stop, nsteps):
        before = np.stack([r.e.get_field(1, c) for c in range(3)]) if (n + 1) % every == 0 else None
        r.step()
        if before is not None:
            now = np.stack([r.e.get_field(1, c) for c in range(3)])
            en_el.append(lm.stored_energy(weights, r.elements.x) if weights is not None else 0.0)
            en.append(_discrete_energy(C, L, np.stack(r.V), now, before) + en_el[-1])
    return np.array(en), np.array(en_el), r


STABILITY = [(kind, name, L, C) for kind in ("parallel", "series") for name, L, C in (("ordinary", 10e-9, 1e-12), ("stiff", 1e-13, 1e-16))]


@pytest.mark.parametrize("kind,name,L,C", STABILITY, ids=[f"{c[0]}-{c[1]}" for c in STABILITY])
def test_loss_free_element_never_gains_energy(oracle_lib, kind, name, L, C):
    """A loss-free parallel L||C or series L-C on one edge of the PEC cavity, 20 000 timesteps: once the source has ended, field energy
    + stored_energy + 1/2 C_fold V^2 never grows.  In exact arithmetic the sum is constant: per step the fields hand the branch
    dt Vm ibar and the trapezoidal rule stores exactly that (with the field energy in its conserved leapfrog form).  In float32 every
    stored value — voltages, currents, states, and once the class tables — is rounded a few times per timestep: at most four roundings
    of relative size 2^-24 each is 8 * 2^-24 of the (quadratic) energy per timestep if all of them push the same way, which the
    tables' rounding does.  That linear worst case is the bound: between the maxima of consecutive 200-timestep windows (at most 400
    timesteps apart) and, over the whole run, above the start.  (A time-level error — the branch driven by V' instead of Vm, a state
    read after its update — makes the branch non-passive: its energy grows by a fraction of (w dt)^2 per timestep, e-folding within a
    few hundred timesteps.)"""
    run = pec_cavity(_one_element(kind, L, C))
    assert run.element_stepped.size == 1 and run.dt == run.grid.courant_dt()
    nsteps = 20000
    en, en_el, r = _energy_series(run, oracle_lib, nsteps)
    assert np.all(np.isfinite(en)) and en[0] > 0 and np.abs(r.elements.x).max() > 0
    w = en[:en.size // 20 * 20].reshape(-1, 20).max(axis=1)
    rise = float(np.max(np.diff(w)) / w[0])
    above = float(np.max(w) / w[0] - 1)
    per_step = 8 * 2.0 ** -24
    print(f"{kind} {name}: energy {en[0]:.3e} -> {en[-1]:.3e} (the element holds up to {en_el.max() / w[0]:.2e} of it); largest rise between "
          f"window maxima {rise:.2e} (bound {400 * per_step:.2e}), most above the start {above:.2e} (bound {(nsteps - len(run.signal)) * per_step:.2e})")
    assert rise <= 400 * per_step and above <= (nsteps - len(run.signal)) * per_step


def test_series_resistance_dissipates(oracle_lib):
    """R = 5 ohm in the series element: the energy never grows between window maxima and falls by three decades."""
    run = pec_cavity(_one_element("series", 10e-9, 1e-12, R=5.0))
    en, en_el, _ = _energy_series(run, oracle_lib, 20000)
    w = en[:en.size // 20 * 20].reshape(-1, 20).max(axis=1)
    print(f"R = 5 ohm: energy {w[0]:.3e} -> {w[-1]:.3e}; the element's {en_el[:20].max():.3e} -> {en_el[-20:].max():.3e}")
    assert np.all(np.isfinite(en)) and np.all(np.diff(w) <= 0), "energy grew after the source ended"
    assert w[-1] < 1e-3 * w[0]


# ---- equivalences --------------------------------------------------------------------------------------------------------------
def _open_sim(add, nr_ts=300):
    sc, sim = pkg("scene"), pkg("simulation")
    g = _grid((16, 15, 14))
    s = sc.Scene(unit=1e-3)
    s.add_metal("gnd").add_box([3, 3, 4], [12, 11, 4])
    s.add_lumped_port(1, 50.0, [6, 7, 4], [6, 7, 6], "z", 1.0)
    add(s)
    return sim.Simulation(g, sc.voxelize(s, g), f0=6e9, fc=4e9, boundary="PEC", nr_ts=nr_ts, end_criteria=0.0)


def test_resistor_only_element_is_a_port_resistor(oracle_lib):
    box = ([9, 6, 4], [10, 7, 7])
    as_port = _open_sim(lambda s: s.add_lumped_port(2, 75.0, box[0], box[1], "z", 0.0))
    as_elem = _open_sim(lambda s: s.add_lumped_element("r", "z", R=75.0, caps=False).add_box(*box))
    assert as_elem.element_stepped.size == 0 and len(as_elem.elements) == 12
    fields = []
    for run in (as_port, as_elem):
        e = run.build(oracle_lib)                       # the oracle has no lumped entry points: no set is made
        e.run(300)
        fields.append(e.fields())
    assert np.abs(fields[0]).max() > 0 and np.array_equal(fields[0], fields[1])
    rc = _open_sim(lambda s: s.add_lumped_element("rc", "z", R=75.0, C=1e-12, caps=False).add_box(*box))
    assert rc.element_stepped.size == 0
    e = rc.build(oracle_lib)
    e.run(300)
    assert not np.array_equal(e.fields(), fields[0])
    # the capacitor is in the operator: vi of an element edge is dt / ((C0 + C_e)(1 + dt G / 2 (C0 + C_e)))
    le = rc.element_lumped[0]
    C_e, G_e = 1e-12 * 3 / 4, 3 / (75.0 * 4)
    assert le.C == C_e and le.G == G_e
    Ctot = EPS0 * 1e-3 + C_e
    vi = float(rc.op.raw()[1][2][le.k, le.j, le.i])
    assert abs(vi / (rc.dt / (Ctot * (1 + 0.5 * rc.dt * G_e / Ctot))) - 1) < 1e-6


def test_split_rule_3_series_2x2_parallel():
    run = _open_sim(lambda s: s.add_lumped_element("t", "z", R=10.0, L=4e-9, C=2e-12, kind="series", caps=False).add_box([9, 6, 4], [10, 7, 7]))
    el = run.elements
    assert len(el) == 12 and len(el.elements) == 1 and run.element_stepped.size == 12
    m = el.elements[0]
    assert (m.n_ser, m.n_par) == (3, 4)
    assert m.R_edge == 10.0 * 4 / 3 and m.L_edge == 4e-9 * 4 / 3 and m.C_edge == 2e-12 * 3 / 4
    # 3 in series x 4 in parallel of the per-edge admittance is the element's
    f = np.array([1e9, 3e9, 7e9])
    assert np.allclose(m.admittance(f) * 4 / 3, 1 / (10.0 + 2j * np.pi * f * 4e-9 + 1 / (2j * np.pi * f * 2e-12)), rtol=1e-13)
    nx, ny, _ = run.grid.shape
    k, r = np.divmod(el.idx, nx * ny)
    assert sorted(set(k)) == [4, 5, 6] and sorted(set(r % nx)) == [9, 10] and sorted(set(r // nx)) == [6, 7] and np.all(el.comp == 2)
    idx, comp, vi, cls, phi, gam, h = run.lumped_tables()
    assert phi.shape == (1, 2, 2) and np.all(cls == 0)
    assert np.array_equal(vi, run.op.raw()[1].reshape(3, -1)[comp.astype(np.int64), idx])
    info = run.lumped_info()[0]
    assert info["edges"] == 12 and info["n_ser"] == 3 and info["n_par"] == 4 and info["kind"] == "series"
    assert abs(info["resonance_hz"] - 1 / (2 * np.pi * np.sqrt(8e-21))) < 1 and info["resonance_warped_hz"] < info["resonance_hz"]


# ---- scene and API -------------------------------------------------------------------------------------------------------------
def test_add_lumped_element_through_openems_api():
    oa = pkg("openems_api")
    csx = oa.ContinuousStructure()
    csx.GetGrid().SetDeltaUnit(1e-3)
    for a, l in zip("xyz", ([0, 11], [0, 11], [0, 9])):
        csx.GetGrid().AddLine(a, np.arange(l[0], l[1] + 1, 1.0))
    csx.AddLumpedElement("trap", "z", caps=False, R=2.0, C=1.5e-12, L=3e-9, LEtype=1).AddBox([4, 5, 3], [4, 5, 5])
    f = oa.openEMS(NrTS=10)
    f.SetGaussExcite(2e9, 1e9)
    f.SetCSX(csx)
    assert f.calls[-2] == {"op": "AddLumpedElement", "name": "trap", "ny": 2, "caps": False, "R": 2.0, "C": 1.5e-12, "L": 3e-9, "LEtype": 1}
    assert f.calls[-1] == {"op": "AddBox", "prop": "trap", "priority": 0, "start": [4, 5, 3], "stop": [4, 5, 5]}
    grid, scene = f._build_scene()
    el = scene.elements[0]
    assert (el.name, el.direction, el.caps, el.spec.kind, el.spec.R, el.spec.L, el.spec.C) == ("trap", 2, False, "series", 2.0, 3e-9, 1.5e-12)
    v = pkg("scene").voxelize(scene, grid)
    assert len(v.elements) == 2 and v.elements.elements[0].n_ser == 2
    with pytest.raises(ValueError, match="'neg'"):
        csx.AddLumpedElement("neg", "x", R=-5.0)
    import importlib, sys
    sys.path.insert(0, os.path.join(ROOT, "fdtd-solver-antennas_amd", "compat"))
    try:
        assert hasattr(importlib.import_module("CSXCAD").ContinuousStructure, "AddLumpedElement")
    finally:
        sys.path.pop(0)


def test_voxeliser_refusals_name_the_element_and_the_node():
    sc = pkg("scene")
    g = _grid((12, 12, 10))

    def scene():
        s = sc.Scene(unit=1e-3)
        s.add_metal("strip").add_box([2, 5, 3], [9, 5, 3])
        s.add_lumped_port(1, 50.0, [3, 7, 2], [3, 7, 4], "z", 1.0)
        return s
    cases = [(lambda s: s.add_lumped_element("e1", "x", L=1e-9).add_box([4, 5, 3], [6, 5, 3]), r"'e1'.*\(4, 5, 3\).*PEC"),
             (lambda s: s.add_lumped_element("e2", "z", L=1e-9).add_box([3, 7, 3], [3, 7, 4]), r"'e2'.*\(3, 7, 3\).*lumped port 1"),
             (lambda s: (s.add_lumped_element("e3", "y", L=1e-9).add_box([6, 7, 6], [6, 9, 6]),
                         s.add_lumped_element("e4", "y", R=5.0).add_box([6, 8, 6], [6, 9, 6])), r"'e3'.*\(6, 8, 6\).*'e4'.*two elements"),
             (lambda s: s.add_lumped_element("e5", "z", L=1e-9).add_box([6, 7, 6], [8, 7, 6]), r"'e5'.*\(6, 7, 6\).*zero length"),
             # the caps of one element short the edges of another
             (lambda s: (s.add_lumped_element("e6", "z", R=5.0).add_box([6, 7, 5], [8, 9, 7]),
                         s.add_lumped_element("e7", "x", L=1e-9, caps=False).add_box([6, 8, 7], [7, 8, 7])), r"'e7'.*\(6, 8, 7\).*PEC")]
    for add, msg in cases:
        s = scene()
        add(s)
        with pytest.raises(ValueError, match=msg):
            sc.voxelize(s, g)
    # a port's source edges that are not on its probe line, and a sheet edge
    s = scene()
    s.ports[0].start, s.ports[0].stop = (3.0, 6.0, 2.0), (3.0, 8.0, 4.0)
    s.add_lumped_element("e8", "z", L=1e-9).add_box([3, 8, 2], [3, 8, 3])
    with pytest.raises(ValueError, match=r"'e8'.*\(3, 8, 2\).*source edge of lumped port 1"):
        sc.voxelize(s, g)
    s = scene()
    s.add_conducting_sheet("cu", 5.8e7, 35e-6).add_box([2, 8, 6], [9, 10, 6])
    s.add_lumped_element("e9", "x", L=1e-9).add_box([4, 9, 6], [5, 9, 6])
    with pytest.raises(ValueError, match=r"'e9'.*\(4, 9, 6\).*conducting-sheet edge"):
        sc.voxelize(s, g)


def test_caps_short_exactly_the_end_plane_edges():
    sc = pkg("scene")
    g = _grid((12, 12, 10))

    def vox(caps, start, stop):
        s = sc.Scene(unit=1e-3)
        s.add_lumped_element("e", "z", R=50.0, caps=caps).add_box(start, stop)
        return sc.voxelize(s, g)
    assert not vox(True, [5, 5, 3], [5, 5, 6]).pec.any()                # a line element has no cap edges
    assert not vox(False, [4, 5, 3], [6, 7, 6]).pec.any()
    v = vox(True, [4, 5, 3], [6, 7, 6])
    want = np.zeros_like(v.pec)
    for k in (3, 6):
        want[0, k, 5:8, 4:6] = True          # x edges (4..5) on the three y lines
        want[1, k, 5:7, 4:7] = True          # y edges (5..6) on the three x lines
    assert np.array_equal(v.pec, want)
    assert len(v.elements) == 27 and v.elements.elements[0].n_ser == 3 and v.elements.elements[0].n_par == 9


def _sheet_strips(caps):
    """Two conducting-sheet strips on a substrate, the gap between them bridged by a series R-L-C with a cross-section."""
    sc, sim = pkg("scene"), pkg("simulation")
    g = _grid((26, 24, 22))
    s = sc.Scene(unit=1e-3)
    s.add_material("sub", eps_r=3.0).add_box([5, 5, 8], [20, 18, 10])
    s.add_metal("gnd").add_box([5, 5, 8], [20, 18, 8])
    s.add_conducting_sheet("strip", 5.8e7, 35e-6).add_box([8, 11, 10], [12, 12, 10])
    s.add_conducting_sheet("strip2", 5.8e7, 35e-6).add_box([14, 11, 10], [18, 12, 10])
    s.add_lumped_element("trap", "x", R=5.0, L=2e-9, C=0.3e-12, kind="series", caps=caps).add_box([12, 11, 10], [14, 12, 10])
    s.add_lumped_port(1, 50.0, [8, 11, 8], [8, 12, 10], "z", 1.0)
    v = sc.voxelize(s, g)
    return v, sim.Simulation(g, v, f0=6e9, fc=4e9, boundary="CPML", cpml_cells=4, nr_ts=300, end_criteria=0.0)


def test_caps_on_conducting_sheet_edges_are_metal_not_sheet(oracle_lib):
    """An element with caps between two conducting-sheet strips: the two cap edges are the strips' end edges.  They become PEC and leave
    the sheet set; every remaining sheet edge and every element edge takes its vi from the operator, and the scene steps."""
    v0, run0 = _sheet_strips(False)
    v1, run1 = _sheet_strips(True)
    nx, ny, _ = run1.grid.shape
    caps = {((10 * ny + 11) * nx + 12) * 3 + 1, ((10 * ny + 11) * nx + 14) * 3 + 1}       # the y edges (12 | 14, 11..12, 10)
    k0, k1 = set((v0.sheets.idx * 3 + v0.sheets.comp).tolist()), set((v1.sheets.idx * 3 + v1.sheets.comp).tolist())
    assert caps <= k0 and k1 == k0 - caps and len(v1.sheets) == len(v0.sheets) - 2
    assert v1.pec[1, 10, 11, 12] and v1.pec[1, 10, 11, 14] and not v0.pec[1, 10, 11, 12]
    for run in (run0, run1):
        vi_op = run.op.raw()[1].reshape(3, -1)
        assert np.array_equal(run.sheet_vi(), vi_op[run.sheets.comp.astype(np.int64), run.sheets.idx])
        idx, comp = run.lumped_tables()[:2]
        assert idx.size == 4 and np.array_equal(run.lumped_vi(), vi_op[comp.astype(np.int64), idx]) and np.all(run.lumped_vi() != 0)
    r = Restatement(run1, oracle_lib)
    r.run(300)
    assert np.all(np.isfinite(r.e.fields())) and np.abs(r.elements.x).max() > 0 and np.abs(r.sheets.ib).max() > 0


def test_caps_that_would_short_a_port_are_refused():
    sc = pkg("scene")
    g = _grid((12, 12, 10))
    # a port on the z edges (3, 6..8, 2..3), probe line at y = 7; x-directed elements whose end plane x = 3 holds some of those edges
    for start, stop, node, what in (([3, 8, 2], [5, 9, 4], r"\(3, 8, [23]\)", "source edge"), ([3, 6, 2], [5, 8, 4], r"\(3, 7, [23]\)", "voltage-probe line")):
        s = sc.Scene(unit=1e-3)
        s.add_lumped_port(1, 50.0, [3, 6, 2], [3, 8, 4], "z", 1.0)
        s.add_lumped_element("e", "x", R=50.0).add_box(start, stop)
        with pytest.raises(ValueError, match=rf"'e'.*cap edge.*{node}.*{what} of lumped port 1"):
            sc.voxelize(s, g)
        s.elements[0].caps = False
        sc.voxelize(s, g)
