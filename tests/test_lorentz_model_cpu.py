"""Lorentz and Drude media (lorentz.py, scene.add_lorentz_material, CSX.AddLorentzMaterial): the admittance the discretised poles
present, the resonances of a filled cavity against their closed forms, passivity, the float32 budget of the correction, the fold into
the operator, the voxeliser's refusals and the API mirror.  The per-timestep correction is restated in numpy (lorentz.correction) on
top of the oracle's half-steps — the oracle knows nothing of dispersion — behind the Debye media's correction and in front of the
sheets' (restatement.Restatement), which is also what the GPU tests compare the HIP path with, bit for bit."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, pkg
from helpers import load_oracle_f64, rel_l2, stage_f64_tables
from restatement import Restatement, install
from test_dispersion_model_cpu import _discrete_energy, _edge_CL, _fr4, _graded, _grid
from test_lumped_model_cpu import pec_cavity
from test_oracle_kat_cpu import _peak

C0 = 299792458.0
EPS0 = pkg("constants").EPS0
TWO_PI = 2 * np.pi

# test 4: rel. L2 of the float32 restatement against the float64 one, over the same quantity of the scene with the media replaced by
# plain materials of their eps_inf.  The cap is the one the magnetic budget test holds its F to.
FP32_BUDGET_CAP = 10.0


def _lor():
    return pkg("lorentz")


def lorentz_cavity(add, *, n=(14, 13, 12), nr_ts=400, boundary="PEC", use_classes=True, f0=10e9, fc=4e9):
    """The PEC cavity of test_lumped_model_cpu.pec_cavity; `add(scene)` draws the media."""
    return pec_cavity(add, n=n, nr_ts=nr_ts, boundary=boundary, use_classes=use_classes, f0=f0, fc=fc)


# ---- 1. admittance identity ---------------------------------------------------------------------------------------------------
POLES = {"drude": dict(wp=[TWO_PI * 7e9], w0=[0.0], gamma=[0.0]),
         "drude lossy": dict(wp=[TWO_PI * 7e9], w0=[0.0], gamma=[3e10]),
         "lorentz": dict(wp=[TWO_PI * 5e9], w0=[TWO_PI * 9e9], gamma=[0.0]),
         "lorentz lossy": dict(wp=[TWO_PI * 5e9], w0=[TWO_PI * 9e9], gamma=[8e9]),
         "four mixed": dict(wp=TWO_PI * np.array([3e9, 5e9, 2e9, 8e9]), w0=TWO_PI * np.array([0.0, 6e9, 12e9, 20e9]),
                            gamma=[1e9, 0.0, 4e9, 2e10])}


@pytest.mark.parametrize("name", sorted(POLES))
def test_discrete_admittance_is_the_warped_continuous_one(name):
    lo, lm = _lor(), pkg("lumped")
    med = lo.LorentzMedium(2.2, 0.03, **POLES[name])
    dt = 1.9e-12
    wdt = np.linspace(0.01, 0.3, 30)
    f = wdt / (TWO_PI * dt)
    Phi, Gam, h, g0 = med.discretise(dt)
    s_d = 1j * (2 / dt) * np.tan(0.5 * wdt)
    y_cont = np.zeros(f.size, np.complex128)
    for k, br in enumerate(med.branches()):
        l = 1 / (EPS0 * med.eps_inf * med.wp[k] ** 2)
        assert br.L == l and br.R == med.gamma[k] * l and (br.C is None) == (med.w0[k] == 0)
        if med.w0[k]:
            assert abs(br.C * l * med.w0[k] ** 2 - 1) < 1e-14
        else:
            assert not Phi[k][1].any() and not Phi[k][:, 1].any() and Gam[k][1] == 0 and h[k][1] == 0
        assert g0[k] > 0 and np.max(np.abs(np.linalg.eigvals(Phi[k]))) <= 1 + 1e-12
        got = lm.transfer(Phi[k], Gam[k], h[k], g0[k], f, dt)
        want = 1.0 / (br.R + s_d * l + (0 if br.C is None else 1.0 / (s_d * br.C)))
        err = float(np.max(np.abs(got - want) / np.abs(want)))
        print(f"{name} pole {k}: discrete admittance against Y(s_d): {err:.2e}")
        assert err <= 1e-12
        y_cont += br.admittance(f)
    # eps(w) from the branch values is the medium's
    w = TWO_PI * f
    rebuilt = med.eps_inf + y_cont / (1j * w * EPS0) - 1j * med.kappa / (w * EPS0)
    assert np.max(np.abs(rebuilt - med.eps(f)) / np.abs(med.eps(f))) <= 1e-12
    assert np.all(med.eps(f).imag <= 0)
    # the fold
    assert med.folded(dt) == (2.2, 0.03 + float(np.sum(g0)))
    phi32, gam32, h32 = lo.tables([med, lo.LorentzMedium(1.0, 0.0, [1e10])], dt)
    assert phi32.shape == (2, med.K, 2, 2) and phi32.dtype == np.float32 and np.array_equal(phi32[0], Phi.astype(np.float32))
    assert np.array_equal(gam32[0], Gam.astype(np.float32)) and np.array_equal(h32[0], h.astype(np.float32))
    assert not phi32[1, 1:].any() and not gam32[1, 1:].any() and not h32[1, 1:].any()       # padding poles carry nothing


def test_refused_media():
    lo = _lor()
    for bad in (dict(eps_inf=0.9, kappa=0, wp=[1e10]), dict(eps_inf=1, kappa=-1, wp=[1e10]), dict(eps_inf=1, kappa=0, wp=[0.0]),
                dict(eps_inf=1, kappa=0, wp=[1e10], w0=[-1.0]), dict(eps_inf=1, kappa=0, wp=[1e10], gamma=[-1.0]),
                dict(eps_inf=1, kappa=0, wp=[1e10] * 5), dict(eps_inf=1, kappa=0, wp=[]), dict(eps_inf=1, kappa=0, wp=[1e10], w0=[1e10, 2e10]),
                dict(eps_inf=1, kappa=0, wp=[float("nan")])):
        with pytest.raises(ValueError, match="Lorentz medium"):
            lo.LorentzMedium(**{"w0": (), "gamma": (), **bad})
    m = lo.LorentzMedium(1.0, 0.0, [1e10], (), ())
    assert m.K == 1 and m.w0[0] == 0 and m.gamma[0] == 0


# ---- 2. cavity resonances -----------------------------------------------------------------------------------------------------
def _kat_cavity(medium, nsteps, *, lines=(41, 25, 33)):
    """The PEC cavity of test_oracle_kat_cpu.test_pec_cavity_te101 (0.10 x 0.06 x 0.08 m, its source and probe), filled completely."""
    sc, sim = pkg("scene"), pkg("simulation")
    a, b, d = 0.10, 0.06, 0.08
    g = pkg("grid").RectGrid(np.linspace(0, a, lines[0]), np.linspace(0, b, lines[1]), np.linspace(0, d, lines[2]))
    s = sc.Scene(unit=1.0)
    if medium is not None:
        s.add_lorentz_material("fill", medium.eps_inf, medium.kappa, medium.wp, medium.w0, medium.gamma).add_box([-1.0] * 3, [1.0] * 3)
    return sim.Simulation(g, sc.voxelize(s, g), f0=2.5e9, fc=1.5e9, boundary="PEC", nr_ts=nsteps, end_criteria=0.0), g


def _kat_series(run, g, lib, nsteps):
    r = Restatement(run, lib)
    assert g.shape == (41, 25, 33)                      # the KAT's mesh: its source and probe nodes
    r.e.add_source([g.flat(13, 10, 9)], [1], [1.0])
    pid = r.e.add_probe(0, [g.flat(25, 12, 20)], [1], [1.0])
    r.run(nsteps)
    return r, r.e.get_probe(pid)[:nsteps]


def test_filled_cavity_resonances_against_closed_forms(oracle_lib):
    """TE101 of the KAT cavity, filled with a loss-free Drude medium (eps_inf = 1): sqrt(f_c^2 + f_p^2); filled with a loss-free
    Lorentz medium: both roots of eps_inf w^2 (1 + wp^2 / (w0^2 - w^2)) = w_c^2.  Bar: 2e-3, the bar the KAT holds the empty cavity
    to on this mesh; the empty cavity's error by the same estimator is recorded next to them."""
    lo = _lor()
    a, d = 0.10, 0.08
    fc = C0 / 2 * np.sqrt(1 / a ** 2 + 1 / d ** 2)
    nsteps = 6000
    fp, f0, einf = 2.0e9, 3.0e9, 1.5
    assert all(fc / 2 <= v <= 2 * fc for v in (fp, f0))
    lines = []
    run, g = _kat_cavity(None, nsteps)
    dt = run.dt
    _, v = _kat_series(run, g, oracle_lib, nsteps)
    e_empty = abs(_peak(v, dt, 0.9 * fc, 1.1 * fc, pad=64) / fc - 1)
    lines.append(f"cavity 0.10 x 0.06 x 0.08 m on 40 x 24 x 32 cells, dt = {dt:.4e} s (the Courant limit), {nsteps} timesteps, f_c = {fc / 1e9:.5f} GHz")
    lines.append(f"empty: TE101 relative error {e_empty:.2e}")
    # Drude
    drude = lo.LorentzMedium(1.0, 0.0, [TWO_PI * fp])
    run, g = _kat_cavity(drude, nsteps)
    assert run.dt == dt and run.lorentz is not None and run.kappa_cells.min() > 0
    r, v = _kat_series(run, g, oracle_lib, nsteps)
    want = np.sqrt(fc ** 2 + fp ** 2)
    e_drude = abs(_peak(v, dt, 0.9 * want, 1.1 * want, pad=64) / want - 1)
    assert max(np.abs(x).max() for x in r.lorentz.x) > 0
    lines.append(f"Drude f_p = {fp / 1e9:.2f} GHz, eps_inf = 1: sqrt(f_c^2 + f_p^2) = {want / 1e9:.5f} GHz, relative error {e_drude:.2e}")
    # Lorentz: x = w^2 solves x^2 - x (w0^2 + wp^2 + wc^2 / eps_inf) + w0^2 wc^2 / eps_inf = 0
    lor = lo.LorentzMedium(einf, 0.0, [TWO_PI * fp], [TWO_PI * f0])
    S, P = f0 ** 2 + fp ** 2 + fc ** 2 / einf, f0 ** 2 * fc ** 2 / einf
    roots = [np.sqrt(0.5 * (S - np.sqrt(S * S - 4 * P))), np.sqrt(0.5 * (S + np.sqrt(S * S - 4 * P)))]
    for fr in roots:
        e = lor.eps([fr])[0]
        assert abs(e.real * fr ** 2 / fc ** 2 - 1) < 1e-12 and e.imag == 0
    run, g = _kat_cavity(lor, nsteps)
    r, v = _kat_series(run, g, oracle_lib, nsteps)
    e_lor = [abs(_peak(v, dt, 0.965 * fr, 1.035 * fr, pad=64) / fr - 1) for fr in roots]
    lines.append(f"Lorentz f_p = {fp / 1e9:.2f} GHz, f_0 = {f0 / 1e9:.2f} GHz, eps_inf = {einf}: lower branch {roots[0] / 1e9:.5f} GHz, relative error "
                 f"{e_lor[0]:.2e}; upper branch {roots[1] / 1e9:.5f} GHz, relative error {e_lor[1]:.2e}")
    lines.append("bar: 2e-3 (tests/test_oracle_kat_cpu.py::test_pec_cavity_te101)")
    print("\n".join(lines))
    if os.environ.get("FDTD_WRITE_RECORDS") == "1":      # the committed record is rewritten on request only
        out = os.path.join(ROOT, "profiles", "lorentz")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "kat.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
    assert e_empty < 2e-3
    assert e_drude < 2e-3 and e_lor[0] < 2e-3 and e_lor[1] < 2e-3, (e_drude, e_lor)


# ---- 3. passivity -------------------------------------------------------------------------------------------------------------
def _f64_fields(e, lib64):
    from test_magnetic_model_cpu import fields_f64
    return fields_f64(e, lib64)


def _energy_run(medium, nsteps, lib64, seed=5):
    """Discrete energy (test_oracle_invariants_cpu's form: 1/2 V C V + 1/2 I^{n+1/2} L I^{n-1/2}, plus the branches' 1/2 w_e (l j^2 +
    c u^2)) after each of nsteps timesteps of the KAT cavity on a 20 x 12 x 16-cell mesh from seeded fields, everything in double."""
    run, g = _kat_cavity(medium, nsteps, lines=(21, 13, 17))
    stage_f64_tables(run, lib64)
    r = Restatement(run, lib64, f64=lib64, round32=False)
    e = r.e
    op = [np.zeros((3,) + e.local_shape, np.float64) for _ in range(4)]
    lib64.fdtd_oracle_get_operator_f64.restype = ctypes.c_int
    lib64.fdtd_oracle_get_operator_f64.argtypes = [ctypes.c_void_p] * 5
    assert lib64.fdtd_oracle_get_operator_f64(e._ctx, *[a.ctypes.data for a in op]) == 0
    rng = np.random.default_rng(seed)
    for kind, live in ((0, op[1] != 0), (1, op[3] != 0)):      # seeded noise on the live unknowns; the walls stay at zero
        for c in range(3):
            e.set_field(kind, c, (1e-3 * rng.standard_normal(e.local_shape) * live[c]).astype(np.float32))
    eps_cells = np.full(run.vox.eps_r.shape, 1.0 if medium is None else medium.eps_inf)
    C, L = _edge_CL(g, eps_cells)
    C, L = C * (op[1] != 0), L * (op[3] != 0)
    I_prev = _f64_fields(e, lib64)[1]
    step = r.step if medium is not None else (lambda: (e.half_step(0), e.half_step(1)))
    en = []
    for _ in range(nsteps):
        step()
        F = _f64_fields(e, lib64)
        q = 0.5 * float(np.sum(C * F[0] ** 2)) + 0.5 * float(np.sum(L * F[1] * I_prev))
        if medium is not None:
            q += _lor().branch_energy(run.lorentz, r.lorentz.x)
        en.append(q)
        I_prev = F[1]
    return np.array(en), r


def test_passivity_in_double(oracle_lib):
    lo = _lor()
    lib64 = load_oracle_f64()
    nsteps = 400
    en0, _ = _energy_run(None, nsteps, lib64)
    drift = float(np.max(np.abs(en0 / en0[0] - 1)))
    print(f"empty cavity, double: conserved-energy drift over {nsteps} timesteps {drift:.2e}")
    assert 0 < drift < 1e-10
    bound = 10 * drift                         # one order of magnitude for the extra state arithmetic
    free = lo.LorentzMedium(1.5, 0.0, TWO_PI * np.array([2e9, 3e9]), TWO_PI * np.array([0.0, 3e9]), [0.0, 0.0])
    en, r = _energy_run(free, nsteps, lib64)
    got = float(np.max(np.abs(en / en[0] - 1)))
    branch = lo.branch_energy(r.sim.lorentz, r.lorentz.x)
    print(f"loss-free Drude + Lorentz poles: drift {got:.2e} (bound {bound:.2e}); branches hold {branch / en[-1]:.3f} of the energy")
    assert branch > 0.01 * en[-1]
    assert got <= bound
    lossy = lo.LorentzMedium(1.5, 0.0, TWO_PI * np.array([2e9, 3e9]), TWO_PI * np.array([0.0, 3e9]), [2e9, 5e8])
    en, _ = _energy_run(lossy, nsteps, lib64)
    rise = float(np.max(np.diff(en)) / en[0])
    print(f"lossy poles: energy {en[0]:.3e} -> {en[-1]:.3e}; largest rise from one timestep to the next {rise:.2e} of the start")
    assert rise <= bound and en[-1] < 0.95 * en[0]          # never up beyond round-off, and the resistors did take energy


# ---- 4. fp32 budget -----------------------------------------------------------------------------------------------------------
def budget_media(s, plain=False):
    lo = _lor()
    a = lo.LorentzMedium(2.0, 0.0, TWO_PI * np.array([6e9, 9e9]), TWO_PI * np.array([11e9, 0.0]), [1e9, 5e9])
    b = lo.LorentzMedium(1.0, 0.0, [TWO_PI * 8e9], [0.0], [0.0])
    for name, m, box in (("block", a, ([4, 4, 3], [9, 8, 8])), ("tile", b, ([10, 4, 3], [11, 8, 6]))):
        if plain:
            s.add_material(name, eps_r=m.eps_inf, kappa=m.kappa).add_box(*box)
        else:
            s.add_lorentz_material(name, m.eps_inf, m.kappa, m.wp, m.w0, m.gamma).add_box(*box)


def budget_sim(n, plain=False):
    """Both builds of the oracle take the same float32 coefficients: the raw operator of the host build."""
    run = lorentz_cavity(lambda s: budget_media(s, plain), nr_ts=n)
    run.device_operator, run.use_classes = False, False
    return run


def budget_reference(lib32, lib64, seed, nsteps):
    """(fields of the float64 restatement on the float32-rounded tables, e_plain: rel. L2 of the float32 oracle against the float64
    oracle on the plain scene), from the same seeded fields."""
    from helpers import seeded_fields
    ref = Restatement(budget_sim(nsteps), lib64, seed=seed, f64=lib64)
    ref.run(nsteps)
    want = _f64_fields(ref.e, lib64)
    plain = []
    for lib in (lib64, lib32):
        e = budget_sim(nsteps, plain=True).build(lib)
        seeded_fields(e, seed)
        e.run(nsteps)
        plain.append(_f64_fields(e, lib64) if lib is lib64 else e.fields().astype(np.float64))
        e.close()
    return want, rel_l2(plain[1], plain[0])


def test_fp32_budget_of_the_correction(oracle_lib):
    lib64 = load_oracle_f64()
    nsteps, lines, worst = 300, [], 0.0
    for seed in (1, 2, 3):
        want, e_plain = budget_reference(oracle_lib, lib64, seed, nsteps)
        r = Restatement(budget_sim(nsteps), oracle_lib, seed=seed)
        r.run(nsteps)
        e_lor = rel_l2(r.e.fields().astype(np.float64), want)
        lines.append(f"seed {seed}: float32 restatement against float64 {e_lor:.3e}; plain materials of eps_inf {e_plain:.3e}; ratio {e_lor / e_plain:.2f}")
        assert 0 < e_plain < 1e-4 and max(np.abs(x).max() for x in r.lorentz.x) > 0
        worst = max(worst, e_lor / e_plain)
    lines.append(f"largest ratio {worst:.2f}; cap {FP32_BUDGET_CAP:g}")
    print("\n".join(lines))
    if os.environ.get("FDTD_WRITE_RECORDS") == "1":
        out = os.path.join(ROOT, "profiles", "lorentz")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "fp32_budget.txt"), "w") as fh:
            fh.write("PEC cavity 14 x 13 x 12 with a two-pole Lorentz / Drude block and a loss-free Drude tile, 300 timesteps from seeded fields;\n"
                     "rel. L2 over all six field components, both precisions on the same float32 operator and tables\n" + "\n".join(lines) + "\n")
    assert worst <= FP32_BUDGET_CAP, worst


# ---- 5. host rules ------------------------------------------------------------------------------------------------------------
def _filled(g, med, lo, hi, name="plasma", unit=1e-3):
    s = pkg("scene").Scene(unit=unit)
    s.add_lorentz_material(name, med.eps_inf, med.kappa, med.wp, med.w0, med.gamma).add_box(lo, hi)
    return s


def test_fold_merge_and_refusals():
    lo, sc, sim, eo = _lor(), pkg("scene"), pkg("simulation"), pkg("ecoperator")
    g = _graded((11, 10, 9))
    x, y, z = (l * 1e3 for l in g.lines)
    m = lo.LorentzMedium(1.8, 0.01, TWO_PI * np.array([4e9, 7e9]), TWO_PI * np.array([0.0, 9e9]), [2e9, 0.0])
    s = _filled(g, m, [x[3], y[2], z[2]], [x[8], y[7], z[5]])
    s.add_material("air_gap", eps_r=1.0).add_box([x[4], y[3], z[2]], [x[6], y[5], z[5]], priority=1)
    v = sc.voxelize(s, g)
    assert v.debye is None and len(v.lorentz.media) == 1 and v.lorentz.names == [["plasma"]]
    run = sim.Simulation(g, v, f0=6e9, fc=3e9, boundary="PEC", nr_ts=10)
    on = v.lorentz.cell_medium == 0
    assert on.any() and not on.all() and np.all(v.eps_r[on] == 1.8) and np.all(v.kappa[on] == 0.01) and np.all(v.kappa[~on] == 0)
    kc = 0.01 + float(np.sum(m.discretise(run.dt)[3]))
    assert np.all(run.kappa_cells[on] == kc) and np.all(run.kappa_cells[~on] == 0) and kc > 0.01
    # the weights are dispersion.edge_weights of the medium's indicator, the boxes tight
    full = pkg("dispersion").edge_weights(g, v.lorentz.cell_medium, 1)
    for c in range(3):
        (i0, j0, k0), (i1, j1, k1) = v.lorentz.lo[c], v.lorentz.hi[c]
        assert np.array_equal(v.lorentz.w[c], full[c][0][k0:k1, j0:j1, i0:i1]) and np.count_nonzero(v.lorentz.w[c]) == np.count_nonzero(full[c][0])
    # the class count grows by the medium's own classes only: a plain material of the folded values gives the same operator
    s2 = sc.Scene(unit=1e-3)
    s2.add_material("plain", eps_r=1.8, kappa=kc).add_box([x[3], y[2], z[2]], [x[8], y[7], z[5]])
    s2.add_material("air_gap", eps_r=1.0).add_box([x[4], y[3], z[2]], [x[6], y[5], z[5]], priority=1)
    v2 = sc.voxelize(s2, g)
    op, op2 = run.op, eo.build_operator(g, v2.eps_r, v2.kappa, v2.pec, run.dt)
    assert np.array_equal(op.vv, op2.vv) and np.array_equal(op.m, op2.m)
    info = run.lorentz_info()
    assert info["K"] == 2 and info["poles"] == 2 and info["edges"] == [int(np.count_nonzero(w)) for w in v.lorentz.w] and sum(info["edges"]) == len(v.lorentz)
    assert info["media"][0]["names"] == ["plasma"] and info["media"][0]["kappa_cell"] == kc
    assert np.allclose(info["media"][0]["plasma_hz"], [4e9, 7e9]) and np.allclose(info["media"][0]["pole_hz"], [0.0, 9e9])
    # identical media merge; different media on one edge are refused; apart they are two media
    s4 = _filled(g, m, [x[1], y[1], z[1]], [x[4], y[8], z[6]], name="a")
    s4.add_lorentz_material("b", m.eps_inf, m.kappa, m.wp.copy(), m.w0.copy(), m.gamma.copy()).add_box([x[4], y[1], z[1]], [x[9], y[8], z[6]])
    v4 = sc.voxelize(s4, g)
    assert len(v4.lorentz.media) == 1 and v4.lorentz.names == [["a", "b"]] and np.count_nonzero(v4.lorentz.cell_medium == 0) == 8 * 7 * 5
    other = lo.LorentzMedium(1.0, 0.0, [TWO_PI * 5e9])
    s5 = _filled(g, m, [x[1], y[1], z[1]], [x[4], y[8], z[6]], name="a")
    s5.add_lorentz_material("c", 1.0, 0.0, other.wp).add_box([x[4], y[1], z[1]], [x[9], y[8], z[6]])
    with pytest.raises(ValueError, match=r"edge at node \(4, \d, \d\) is shared by two different Lorentz media \('a' and 'c'\)"):
        sc.voxelize(s5, g)
    s6 = _filled(g, m, [x[1], y[1], z[1]], [x[4], y[8], z[6]], name="a")
    s6.add_lorentz_material("c", 1.0, 0.0, other.wp).add_box([x[5], y[1], z[1]], [x[9], y[8], z[6]])
    v6 = sc.voxelize(s6, g)
    assert len(v6.lorentz.media) == 2 and v6.lorentz.K == 2 and set(np.unique(v6.lorentz.med[0])) == {0, 1}
    r6 = sim.Simulation(g, v6, f0=6e9, fc=3e9, boundary="PEC", nr_ts=10)
    assert len(set(np.unique(r6.kappa_cells))) == 3 and r6.lorentz_tables()[0].shape == (2, 2, 2, 2)
    # a Lorentz and a Debye medium on one edge are refused, apart they live together
    fr4 = _fr4()
    s7 = _filled(g, m, [x[1], y[1], z[1]], [x[4], y[8], z[6]], name="a")
    s7.add_debye_material("sub", fr4.eps_inf, fr4.kappa, fr4.delta_eps, fr4.tau).add_box([x[4], y[1], z[1]], [x[9], y[8], z[6]])
    with pytest.raises(ValueError, match=r"edge at node \(4, \d, \d\) is shared by the Lorentz medium 'a' and the Debye medium 'sub'"):
        sc.voxelize(s7, g)
    s8 = _filled(g, m, [x[1], y[1], z[1]], [x[4], y[8], z[6]], name="a")
    s8.add_debye_material("sub", fr4.eps_inf, fr4.kappa, fr4.delta_eps, fr4.tau).add_box([x[5], y[1], z[1]], [x[9], y[8], z[6]])
    v8 = sc.voxelize(s8, g)
    r8 = sim.Simulation(g, v8, f0=6e9, fc=3e9, boundary="PEC", nr_ts=10)
    assert v8.debye is not None and v8.lorentz is not None and r8.debye is not None and r8.lorentz is not None
    assert np.all(r8.kappa_cells[v8.lorentz.cell_medium == 0] == kc) and np.all(r8.kappa_cells[v8.debye.cell_medium == 0] == fr4.folded(r8.dt)[1])
    # nine different media are one too many
    s9 = sc.Scene(unit=1e-3)
    for q in range(9):
        s9.add_lorentz_material(f"m{q}", 1.0, 0.0, [TWO_PI * (1 + q) * 1e9]).add_box([x[q], y[1], z[1]], [x[q + 1], y[2], z[2]])
    with pytest.raises(ValueError, match="9 different Lorentz media: at most 8"):
        sc.voxelize(s9, g)
    # media in CPML layers are refused (8 cells on a 24-cell grid), outside them and with Mur faces accepted
    g2 = _grid((24, 24, 24))
    sim.Simulation(g2, sc.voxelize(_filled(g2, m, [9, 9, 9], [14, 14, 14]), g2), f0=6e9, fc=3e9, boundary="CPML", cpml_cells=8, nr_ts=10)
    into = sc.voxelize(_filled(g2, m, [9, 9, 9], [14, 14, 17]), g2)
    with pytest.raises(ValueError, match="Lorentz medium 'plasma' reaches into the CPML layer z\\+ \\(8 cells\\): dispersive cells inside absorbing layers"):
        sim.Simulation(g2, into, f0=6e9, fc=3e9, boundary="CPML", cpml_cells=8, nr_ts=10)
    r_mur = sim.Simulation(g2, into, f0=6e9, fc=3e9, boundary="MUR", nr_ts=10)
    # a decomposed run is refused before any engine exists
    with pytest.raises(pkg("_capi").FdtdError, match="Lorentz media need a single slab"):
        r_mur.build(object(), world=2, rank=0)


def test_add_lorentz_material_to_engine_calls():
    """CSX.AddLorentzMaterial -> scene -> Simulation -> the engine call sequence (a recording stand-in for the library's Engine)."""
    oa, sim, lo = pkg("openems_api"), pkg("simulation"), _lor()
    CS = oa.ContinuousStructure
    fd = oa.openEMS(NrTS=50, EndCriteria=1e-4)
    fd.SetGaussExcite(6e9, 3e9)
    fd.SetBoundaryCond(["PEC"] * 6)
    csx = CS()
    fd.SetCSX(csx)
    mesh = csx.GetGrid()
    mesh.SetDeltaUnit(1e-3)
    for ax, nn in zip("xyz", (13, 12, 11)):
        mesh.AddLine(ax, np.arange(nn, dtype=float))
    p = csx.AddLorentzMaterial("meta", order=2, epsilon=1.5, kappa=0.02, eps_plasma=[4e9, 7e9], eps_pole_freq=[0.0, 9e9], eps_relax=[5e-10, 0.0])
    p.AddBox([2, 2, 2], [10, 9, 8])
    assert p.params == dict(order=2, epsilon=1.5, kappa=0.02, eps_plasma=[4e9, 7e9], eps_pole_freq=[0.0, 9e9], eps_relax=[5e-10, 0.0])
    # the first pole bare, further poles numbered from 1: the same property
    q = CS().AddLorentzMaterial("x", epsilon=1.5, kappa=0.02, eps_plasma=4e9, eps_plasma_1=7e9, eps_pole_freq=0.0, eps_pole_freq_1=9e9,
                                eps_relax=5e-10, eps_relax_1=0.0)
    assert q.params == p.params
    # a plain Drude plasma: order, pole frequency and relaxation time left out
    d = CS().AddLorentzMaterial("plasma", eps_plasma=3e9)
    assert d.params == dict(order=1, epsilon=1.0, kappa=0.0, eps_plasma=[3e9], eps_pole_freq=[0.0], eps_relax=[0.0])
    assert CS().AddLorentzMaterial("ok", eps_plasma=3e9, mue=1.0).params == d.params
    with pytest.raises(ValueError, match="order 2 needs 2 plasma frequencies"):
        CS().AddLorentzMaterial("x", order=2, eps_plasma=[1e9])
    with pytest.raises(ValueError, match="order 1 needs"):
        CS().AddLorentzMaterial("x", eps_plasma=[1e9], eps_pole_freq=[1e9, 2e9])
    with pytest.raises(ValueError, match="1..4 poles"):
        CS().AddLorentzMaterial("x", eps_plasma=[1e9] * 5)
    with pytest.raises(ValueError, match="order 0"):
        CS().AddLorentzMaterial("x", epsilon=2.0)
    with pytest.raises(ValueError, match="eps_relax must be >= 0"):
        CS().AddLorentzMaterial("x", eps_plasma=1e9, eps_relax=-1e-9)
    with pytest.raises(TypeError, match=r"unknown keyword\(s\) \['eps_delta'\]"):
        CS().AddLorentzMaterial("x", eps_plasma=1e9, eps_delta=1.0)
    for kw, word in ((dict(mue_plasma=1e9), "mue_plasma"), (dict(mue_pole_freq_1=1e9), "mue_pole_freq_1"), (dict(mue_relax=1e-9), "mue_relax")):
        with pytest.raises(ValueError, match=f"magnetic poles \\({word}\\) are not supported"):
            CS().AddLorentzMaterial("x", eps_plasma=1e9, **kw)
    for mue in (2.0, [1.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match="mue = .* is not supported"):
            CS().AddLorentzMaterial("x", eps_plasma=1e9, mue=mue)
    assert hasattr(pkg("compat.CSXCAD").ContinuousStructure, "AddLorentzMaterial")
    grid, scene = fd._build_scene()
    mat = scene.materials[0]
    want = lo.LorentzMedium(1.5, 0.02, TWO_PI * np.array([4e9, 7e9]), TWO_PI * np.array([0.0, 9e9]), [1.0 / 5e-10, 0.0])
    assert type(mat).__name__ == "LorentzMaterial" and mat.medium.key() == want.key() and mat.boxes[0].start == (2, 2, 2)
    v = pkg("scene").voxelize(scene, grid)
    run = sim.Simulation(grid, v, f0=6e9, fc=3e9, boundary="PEC", nr_ts=50)
    calls = []

    class Rec:
        def __init__(self, lib, nx, ny, nz, dt, **kw):
            calls.append(("Engine", nx, ny, nz))
            self.step = 0

        def operator_form(self):
            return ("classes", 0)

        def __getattr__(self, name):
            def f(*a, **k):
                calls.append((name,) + tuple(a))
                return 0
            return f

    orig = sim.Engine
    sim.Engine = Rec
    try:
        run.build(object())
    finally:
        sim.Engine = orig
    names = [c[0] for c in calls]
    assert names[:3] == ["Engine", "build_operator", "set_lorentz"] and "set_debye" not in names
    bo = calls[1]
    assert np.array_equal(bo[2], v.eps_r) and np.array_equal(bo[3], run.kappa_cells) and bo[3].max() > 0.02
    phi, gam, h, lo_, hi_, w, med = calls[2][1:]
    P, G, H, g0 = want.discretise(run.dt)
    assert np.array_equal(phi, P.astype(np.float32)[None]) and np.array_equal(gam, G.astype(np.float32)[None]) and np.array_equal(h, H.astype(np.float32)[None])
    assert lo_[0] == (2, 2, 2) and hi_[0] == (10, 10, 9) and w[0].dtype == np.float32 and w[0].shape == (7, 8, 8)
    assert run.lorentz_info()["poles"] == 2 and run.dispersion_info() is None


# ---- 6. through openems_api ---------------------------------------------------------------------------------------------------
def lorentz_patch(lib, nr_ts=1500):
    """A small patch over a ground plane on an eps_r = 2 substrate under a two-pole (Drude + Lorentz) superstrate, fed by a lumped port."""
    oa = pkg("openems_api")
    csx = oa.ContinuousStructure()
    csx.GetGrid().SetDeltaUnit(1e-3)
    for a, l in zip("xyz", (25, 23, 21)):
        csx.GetGrid().AddLine(a, np.arange(0.0, l + 1, 1.0))
    csx.AddMaterial("sub", epsilon=2.0).AddBox([5, 5, 8], [20, 18, 10])
    csx.AddLorentzMaterial("super", order=2, epsilon=1.2, eps_plasma=[3e9, 5e9], eps_pole_freq=[0.0, 8e9], eps_relax=[2e-10, 1e-9]).AddBox([5, 5, 10], [20, 18, 12])
    csx.AddMetal("gnd").AddBox([5, 5, 8], [20, 18, 8])
    csx.AddMetal("patch").AddBox([8, 8, 10], [17, 15, 10])
    f = oa.openEMS(NrTS=nr_ts, EndCriteria=0, lib=lib, cpml_cells=4)
    f.SetGaussExcite(6e9, 4e9)
    f.SetBoundaryCond(["PML_4"] * 6)
    f.SetCSX(csx)
    port = f.AddLumpedPort(1, 50.0, [10, 11, 8], [10, 11, 10], "z", 1.0)
    return f, port


def test_lorentz_superstrate_reaches_the_simulation(oracle_lib, tmp_path, monkeypatch):
    install(monkeypatch)
    f, port = lorentz_patch(oracle_lib, nr_ts=200)
    f.Run(str(tmp_path / "l"), verbose=0)
    d = f.sim.lorentz
    assert d is not None and np.all(f.sim.vox.eps_r[10:12, 5:18, 5:20] == 1.2) and np.all(d.cell_medium[10:12, 5:18, 5:20] == 0)
    st = f.stats.lorentz
    assert st["K"] == 2 and st["poles"] == 2 and st["edges"] == [int(np.count_nonzero(w)) for w in d.w] and sum(st["edges"]) == len(d) > 0
    assert st["media"][0]["names"] == ["super"] and np.allclose(st["media"][0]["plasma_hz"], [3e9, 5e9]) and np.allclose(st["media"][0]["gamma"], [5e9, 1e9])
    assert max(np.abs(x).max() for x in f.sim.restated.lorentz.x) > 0
    # a scene without a Lorentz material reports none
    from test_magnetic_model_cpu import magnetic_patch
    f2, _ = magnetic_patch(oracle_lib, nr_ts=20, mue=1.0)
    f2.Run(str(tmp_path / "p"), verbose=0)
    assert f2.sim.lorentz is None and f2.stats.lorentz is None
