"""Magnetic materials (magnetic.py, Scene.add_material(mu_r=, sigma_m=)) and PMC walls: the face coefficients, known answers on the
oracle stepping the RAW operator magnetic.raw_ii_iv expands (the oracle knows nothing of magnetic media: I = fma(ii, I, iv * curl) is
an independent reference), the numpy restatement of the engine's correction on top of the oracle's half-steps — what the GPU tests
compare the HIP path with, bit for bit — and magnetic-wall symmetry on the double-precision oracle."""
import numpy as np
import pytest

from conftest import pkg
from helpers import rel_l2
from restatement import Restatement, install
from test_dispersion_model_cpu import _discrete_energy, _edge_CL, _graded
from test_oracle_kat_cpu import _peak

C0 = 299792458.0
EPS0 = pkg("constants").EPS0
MU0 = pkg("constants").MU0
ETA0 = float(np.sqrt(MU0 / EPS0))

# GPU test 2 / model test 6: the engine's correction against the oracle's raw operator, both in float32, both measured against the
# double-precision oracle on the same float32 coefficients: e_hip <= FP32_BUDGET_F * e_ref.  F is twice the largest ratio measured
# over the seeds of the test (profiles/magnetic/fp32_budget.txt; the restatement is the engine's arithmetic bit for bit, so the ratio
# is the same on the CPU); the issue's condition is F <= 10 — a wrong formula shows as a ratio of 100 or more.
FP32_BUDGET_F = 2.1
BUDGET_SEEDS = (1, 2, 3)


def _mag():
    return pkg("magnetic")


def _grid(n, h=1e-3):
    return pkg("grid").RectGrid(*[np.arange(k) * h for k in n])


# ---- the two checkers ---------------------------------------------------------------------------------------------------------
def build_raw(sim, lib, magnetic="own"):
    """sim.build(lib) with the operator in raw form and the magnetic faces IN it (ii = a, iv = b iv0): the independent reference.
    `magnetic`: the MagneticFaces to expand (default the simulation's own; None: the base operator)."""
    mag = sim.magnetic if isinstance(magnetic, str) else magnetic
    op = sim.op

    class _Raw:
        def classes(self, *a):
            return None

        def raw(self, k0=0, nk=None):
            vv, vi, _, _ = op.raw(k0, nk)
            ii, iv = _mag().raw_ii_iv(op, mag, k0, nk)
            return vv, vi, ii, iv

    saved = sim.magnetic, sim.device_operator, sim.use_classes
    sim.magnetic, sim.device_operator, sim.use_classes, sim._op = None, False, False, _Raw()
    try:
        return sim.build(lib)
    finally:
        sim.magnetic, sim.device_operator, sim.use_classes = saved
        sim._op = op


def magnetic_cavity(add, *, n=(14, 13, 12), nr_ts=400, boundary="PEC", use_classes=True, f0=10e9, fc=4e9):
    """The PEC cavity of test_lumped_model_cpu.pec_cavity (metal walls one cell inside the grid faces, a 0-ohm soft source); `add(scene)`
    draws the magnetic materials."""
    from test_lumped_model_cpu import pec_cavity
    return pec_cavity(add, n=n, nr_ts=nr_ts, boundary=boundary, use_classes=use_classes, f0=f0, fc=fc)


# ---- 1. coefficients -------------------------------------------------------------------------------------------------------------
def test_coefficients_uniform_interface_and_none():
    mg = _mag()
    g = _graded()
    nx, ny, nz = g.shape
    cells = (nz - 1, ny - 1, nx - 1)
    dt = g.courant_dt()
    for mu in (4.0, 2.5, 7.0):
        a, b, s = mg.face_coefficients(g, np.full(cells, mu), np.zeros(cells), dt)
        for c in range(3):
            live = np.ones((nz, ny, nx), bool)
            for t in ((c + 1) % 3, (c + 2) % 3):
                idx = [slice(None)] * 3; idx[2 - t] = -1
                live[tuple(idx)] = False
            assert np.all(b[c][live] == 1.0 / mu) and np.all(a[c] == 1.0) and np.all(b[c][~live] == 1.0)
    # a two-cell interface along z on the graded mesh: the series (harmonic) value, weighted with the two half cells
    mu = np.ones(cells); mu[6:] = 4.0
    sg = np.zeros(cells); sg[6:] = 300.0
    a, b, s = mg.face_coefficients(g, mu, sg, dt)
    l1, l2 = 0.5 * g.d[2][5], 0.5 * g.d[2][6]
    s_want = (l1 / 1.0 + l2 / 4.0) / (l1 + l2)
    x_want = 0.5 * dt * (l2 * 300.0 / (MU0 * 4.0)) / (l1 + l2)
    assert l1 != l2
    assert np.allclose(s[2][6, :-1, :-1], s_want, rtol=1e-14) and np.allclose(b[2][6, :-1, :-1], s_want / (1 + x_want), rtol=1e-14)
    assert np.allclose(a[2][6, :-1, :-1], (1 - x_want) / (1 + x_want), rtol=1e-14)
    assert np.all(b[2][5, :-1, :-1] == 1.0) and np.allclose(b[2][7, :-1, :-1], 0.25 / (1 + 0.5 * dt * 300.0 / (4 * MU0)), rtol=1e-14)
    # the transverse components see one cell each: no mixing across the interface
    assert np.all(b[0][5, :-1, 1:-1] == 1.0) and np.allclose(s[0][6, :-1, 1:-1], 0.25, rtol=1e-15)
    # L = mu0 A / (l~ s)
    L = mg.inductance(g, s)
    assert np.isclose(L[2][6, 3, 4], MU0 * g.d[0][4] * g.d[1][3] / (g.dd[2][6] * s_want), rtol=1e-14)
    # a non-magnetic scene has no faces at all
    assert mg.make_faces(g, np.ones(cells), np.zeros(cells), dt) is None
    sc, sim = pkg("scene"), pkg("simulation")
    s0 = sc.Scene(unit=1e-3)
    s0.add_material("plain", eps_r=3.0, kappa=0.1).add_box([-100] * 3, [100] * 3)
    v0 = sc.voxelize(s0, g)
    assert np.all(v0.mu_r == 1.0) and np.all(v0.sigma_m == 0.0)
    assert sim.Simulation(g, v0, f0=5e9, fc=3e9, boundary="PEC", nr_ts=10).magnetic is None
    # classes and boxes: the interface scene has three live (a, b) pairs along z times the graded lines
    f = mg.make_faces(g, mu, sg, dt)
    assert f.ncls <= mg.MAX_CLASSES and len(f) == sum(f.faces()) and f.lo[2][2] == 6 and f.lo[0][2] == 6 and f.hi[2][2] == nz
    full = f.full_classes((nz, ny, nx))
    ta = np.concatenate([[np.float32(1)], f.tab_a]); tb = np.concatenate([[np.float32(1)], f.tab_b])
    assert np.array_equal(ta[full], a.astype(np.float32)) and np.array_equal(tb[full], b.astype(np.float32))


def test_priority_rule_and_refusals():
    mg, sc, sim = _mag(), pkg("scene"), pkg("simulation")
    g = _grid((14, 13, 12))
    s = sc.Scene(unit=1e-3)
    s.add_material("ferrite", eps_r=2.0, mu_r=5.0, sigma_m=40.0).add_box([2, 2, 2], [9, 9, 9])
    s.add_material("hole", eps_r=1.0).add_box([4, 4, 2], [6, 6, 9], priority=1)
    v = sc.voxelize(s, g)
    assert v.mu_r[5, 3, 3] == 5.0 and v.sigma_m[5, 3, 3] == 40.0 and v.eps_r[5, 3, 3] == 2.0
    assert v.mu_r[5, 4, 4] == 1.0 and v.sigma_m[5, 4, 4] == 0.0 and v.mu_r[0, 0, 0] == 1.0
    assert v.material_names[v.cell_material[5, 3, 3]] == "ferrite"
    for kw, what in ((dict(mu_r=0.5), "mu_r"), (dict(mu_r=float("nan")), "mu_r"), (dict(sigma_m=-1.0), "sigma_m"),
                     (dict(mu_r=float("inf")), "mu_r"), (dict(mu_r=(2.0, 2.0, 3.0)), "anisotropic"), (dict(sigma_m=[1.0, 2.0, 3.0]), "anisotropic")):
        with pytest.raises(ValueError, match=f"(?s)'bad'.*{what}|{what}.*'bad'"):
            sc.Scene().add_material("bad", **kw)
    # per-cell values (a VoxelScene put together by hand): the material and the node of the cell are named
    cells = v.mu_r.shape
    for mu_bad, sg_bad in ((0.9, 0.0), (float("nan"), 0.0), (2.0, -3.0)):
        mu = v.mu_r.copy(); sgm = v.sigma_m.copy()
        mu[5, 3, 7] = mu_bad; sgm[5, 3, 7] = sg_bad
        with pytest.raises(ValueError, match=r"(?s)'ferrite'.*\(7, 3, 5\)"):
            mg.check_cells(g, mu, sgm, (0,) * 6, v.cell_material, v.material_names)
    with pytest.raises(ValueError, match=r"(?s)'ferrite'.*CPML layer x-.*\(2, 2, 2\)"):
        sim.Simulation(g, v, f0=5e9, fc=3e9, boundary="CPML", cpml_cells=3, nr_ts=10)
    with pytest.raises(ValueError, match=r"'ferrite'.*CPML layer z\+"):
        sim.Simulation(g, v, f0=5e9, fc=3e9, boundary=["PEC"] * 5 + ["PML_3"], nr_ts=10)
    ok = sim.Simulation(g, v, f0=5e9, fc=3e9, boundary="CPML", cpml_cells=2, nr_ts=10)       # the layers end in front of the block
    assert ok.magnetic is not None and ok.magnetic.media == ["ferrite"]
    with pytest.raises(pkg("_capi").FdtdError, match="single slab"):
        ok.build(None, world=2, rank=0)
    # more than 255 classes: refused with the count
    gg = _graded((40, 9, 9))
    big = (8, 8, 39)
    mu = np.ones(big)
    mu[:, :, 2:37] = 1.0 + np.arange(35)[None, None, :] * 0.37 + np.arange(8)[None, :, None] * 0.011
    with pytest.raises(ValueError, match=r"\d+ distinct \(a, b\) face classes"):
        mg.make_faces(gg, mu, np.zeros(big), gg.courant_dt())


# ---- 2. filled PEC cavity ---------------------------------------------------------------------------------------------------------
def test_filled_cavity_resonates_at_half_the_frequency(oracle_lib):
    """The uniform-mesh TE101 cavity of test_oracle_kat_cpu filled with mu_r = 4: the wave speed halves, TE101 sits at f101 / 2
    (tolerance 2e-3, the bar of that test), drawn through Scene.add_material and stepped on the oracle's raw operator."""
    sc, sim = pkg("scene"), pkg("simulation")
    a, b, d = 0.10, 0.06, 0.08
    g = pkg("grid").RectGrid(np.linspace(0, a, 41), np.linspace(0, b, 25), np.linspace(0, d, 33))
    s = sc.Scene(unit=1.0)
    s.add_material("fill", mu_r=4.0).add_box([-1, -1, -1], [1, 1, 1])
    nsteps = 12000
    run = sim.Simulation(g, sc.voxelize(s, g), f0=1.25e9, fc=0.75e9, boundary="PEC", nr_ts=nsteps, end_criteria=0.0)
    assert run.dt == g.courant_dt() and run.magnetic is not None and run.magnetic.ncls == 1
    assert run.magnetic.tab_b[0] == np.float32(0.25) and run.magnetic.tab_a[0] == 1.0
    e = build_raw(run, oracle_lib)
    assert np.all(e.get_operator()[2][run.magnetic.full_classes(e.local_shape) != 0] == 1.0)      # ii = a = 1: loss-free
    e.add_source([g.flat(13, 10, 9)], [1], [1.0])
    pid = e.add_probe(0, [g.flat(25, 12, 20)], [1], [1.0])
    e.run(nsteps)
    f101 = C0 / 2 * np.sqrt(1 / a ** 2 + 1 / d ** 2)
    got = _peak(e.get_probe(pid), run.dt, 0.3 * f101, 0.8 * f101)
    print(f"TE101 of the mu_r = 4 cavity: {got / 1e9:.5f} GHz, f101 / 2 = {f101 / 2e9:.5f} GHz")
    assert abs(got - f101 / 2) / (f101 / 2) < 2e-3


# ---- 3. / 4. a TEM line ------------------------------------------------------------------------------------------------------------
NZ_LINE, K_SRC, K_PRB, K_IFC = 2000, 700, 1000, 1300


def _tem_line(lib, fill, steps, probes, k_end=None):
    """The parallel-plate line of test_host_layer_kat_cpu._plate_line (PEC plates normal to y two cells apart: Ey, Hx, Hz), four node
    lines wide with magnetic side walls, so the TEM wave along z is the 1-D plane wave; PEC at both ends, too far away to echo within
    the window.  `fill`: (eps_r, kappa, mu_r, sigma_m) of the cells K_IFC <= k < k_end (None: to the end).  1 mm cells: 33 cells per
    shortest wavelength of the pulse (9 GHz)."""
    d = 1e-3
    nx, nz = 4, NZ_LINE
    g = pkg("grid").RectGrid(np.arange(nx) * d, np.arange(3) * d, np.arange(nz) * d)
    shape = (nz - 1, 2, nx - 1)
    eps, kap, mu, sgm = np.ones(shape), np.zeros(shape), np.ones(shape), np.zeros(shape)
    if fill is not None:
        sl = slice(K_IFC, k_end)
        eps[sl], kap[sl], mu[sl], sgm[sl] = fill
    vox = pkg("scene").VoxelScene(eps, kap, np.zeros((3, nz, 3, nx), bool), [], mu_r=mu, sigma_m=sgm)
    s = pkg("simulation").Simulation(g, vox, f0=5e9, fc=4e9, boundary=["PMC", "PMC", "PEC", "PEC", "PEC", "PEC"], nr_ts=steps, end_criteria=0.0)
    assert C0 / 9e9 / d >= 30
    e = build_raw(s, lib)
    src = [g.flat(i, j, K_SRC) for i in (1, 2) for j in (0, 1)]
    e.add_source(src, [1] * 4, [1.0] * 4)
    pids = [e.add_probe(0, [g.flat(1, 1, k)], [1], [1.0]) for k in probes]
    e.run(steps)
    out = [e.get_probe(p) for p in pids]
    # the wave is uniform across the line: the two live columns carry the same field
    Ey = e.get_field(0, 1)
    assert np.abs(Ey).max() > 0 and np.array_equal(Ey[:, :2, 1], Ey[:, :2, 2])
    return out, s


def _signed_ratio(x, ref):
    """Amplitude of x in units of ref, signed, at the lag where they overlap best."""
    cc = np.correlate(x, ref, mode="full")
    return float(cc[np.argmax(np.abs(cc))] / np.dot(ref, ref))


def test_interface_polarity_magnetic_against_dielectric(oracle_lib):
    """Air -> mu_r = 4 (eta doubles): reflection +1/3, the reflected pulse has the sign of the incident one; air -> eps_r = 4 (eta
    halves): -1/3.  Within 5 %.  Measured on the oracle: +0.3353 and -0.3313."""
    steps = 2100
    (inc,), _ = _tem_line(oracle_lib, None, steps, [K_PRB])
    got = {}
    for name, fill in (("mu", (1.0, 0.0, 4.0, 0.0)), ("eps", (4.0, 0.0, 1.0, 0.0))):
        (tot,), s = _tem_line(oracle_lib, fill, steps, [K_PRB])
        assert (s.magnetic is not None) == (name == "mu")
        got[name] = _signed_ratio(tot - inc, inc)
    print(f"reflection air -> mu_r 4: {got['mu']:+.4f}; air -> eps_r 4: {got['eps']:+.4f} (+-1/3)")
    assert got["mu"] > 0 and abs(got["mu"] - 1 / 3) < 0.05 / 3
    assert got["eps"] < 0 and abs(got["eps"] + 1 / 3) < 0.05 / 3


def test_matched_lossy_slab(oracle_lib):
    """eps_r = mu_r = 1 with kappa and sigma* = kappa mu0 / eps0: the medium keeps eta0 — no reflection, and a plane wave decays as
    exp(-kappa eta0 z) whatever its frequency.  A slab of 100 cells with kappa eta0 L = 1: the transmitted amplitude is 1/e within 2 %,
    and its reflection lies below that of the kappa-only twin.  Measured on the oracle: transmitted 0.36752 (1/e = 0.36788), reflected
    1.2e-4 of the incident peak; the kappa-only twin transmits 0.607 and reflects 2.6e-2."""
    steps, L = 2600, 0.1
    kappa = 1.0 / (ETA0 * L)
    k_end, k_out = K_IFC + 100, K_IFC + 250
    (inc_r, inc_t), _ = _tem_line(oracle_lib, None, steps, [K_PRB, k_out])
    (r_m, t_m), s = _tem_line(oracle_lib, (1.0, kappa, 1.0, kappa * MU0 / EPS0), steps, [K_PRB, k_out], k_end)
    (r_u, t_u), _ = _tem_line(oracle_lib, (1.0, kappa, 1.0, 0.0), steps, [K_PRB, k_out], k_end)
    assert s.magnetic is not None and np.all(s.magnetic.tab_a < 1.0)
    trans = _signed_ratio(t_m, inc_t)
    refl_m = float(np.abs(r_m - inc_r).max() / np.abs(inc_r).max())
    refl_u = float(np.abs(r_u - inc_r).max() / np.abs(inc_r).max())
    print(f"matched slab: transmitted {trans:.5f} (exp(-1) = {np.exp(-1):.5f}), reflected {refl_m:.2e}; kappa-only twin: transmitted "
          f"{_signed_ratio(t_u, inc_t):.5f}, reflected {refl_u:.2e}")
    assert abs(trans / np.exp(-kappa * ETA0 * L) - 1) < 0.02
    assert refl_m < refl_u


# ---- 5. energy ---------------------------------------------------------------------------------------------------------------------
def _block(mu_r, sigma_m=0.0):
    return lambda s: s.add_material("block", eps_r=2.0, mu_r=mu_r, sigma_m=sigma_m).add_box([4, 4, 3], [9, 8, 8])


def _energy_windows(run, lib, nsteps, every=10):
    C, _ = _edge_CL(run.grid, run.vox.eps_r)
    L = _mag().inductance(run.grid, run.magnetic.s)
    r = Restatement(run, lib)
    stop = len(run.signal) + 1
    r.run(stop)
    en = []
    for n in range(stop, nsteps):
        before = np.stack(r.I) if (n + 1) % every == 0 else None
        r.step()
        if before is not None:
            en.append(_discrete_energy(C, L, np.stack(r.V), np.stack(r.I), before))
    en = np.array(en)
    return en, en[:en.size // 20 * 20].reshape(-1, 20).max(axis=1), r


def test_loss_free_block_never_gains_energy(oracle_lib):
    """A loss-free mu_r = 3 block in the PEC cavity, stepped by the restatement (the engine's arithmetic): once the source has ended
    the conserved leapfrog energy 1/2 V C V + 1/2 I^{n+1/2} L I^{n-1/2}, L = mu0 A / (l~ s), never grows.  In exact arithmetic it is
    constant; in float32 a magnetic face's current is rounded five times per timestep (the H update and four statements of the
    correction), a voltage twice, and the class table once: eight roundings of 2^-24 each, all pushing the same way, are 16 * 2^-24 of
    the (quadratic) energy per timestep.  That linear worst case is the bound, as for the lumped elements: between the maxima of
    consecutive 200-timestep windows and, over the whole run, above the start.  (A wrong L or a correction applied at the wrong time
    level makes the sum oscillate or grow by percents.)"""
    nsteps = 8000
    run = magnetic_cavity(_block(3.0), nr_ts=nsteps)
    assert run.dt == run.grid.courant_dt() and run.magnetic is not None
    en, w, r = _energy_windows(run, oracle_lib, nsteps)
    per_step = 16 * 2.0 ** -24
    rise, above = float(np.max(np.diff(w)) / w[0]), float(np.max(w) / w[0] - 1)
    print(f"loss-free block: energy {en[0]:.4e} -> {en[-1]:.4e}; largest rise between window maxima {rise:.2e} (bound {400 * per_step:.2e}), "
          f"most above the start {above:.2e} (bound {(nsteps - len(run.signal)) * per_step:.2e}); spread {np.ptp(en) / en[0]:.2e}")
    assert np.all(np.isfinite(en)) and en[0] > 0 and max(np.abs(p).max() for p in r.magnetic.iprev) > 0
    assert rise <= 400 * per_step and above <= (nsteps - len(run.signal)) * per_step
    # ... and it is CONSTANT within the same accumulated rounding, sample by sample: with another L (mu0 A / l~ without s) the sum
    # swings with the field between the block and the air around it
    assert np.ptp(en) / en[0] <= (nsteps - len(run.signal)) * per_step
    L0 = _edge_CL(run.grid, run.vox.eps_r)[1]
    assert not np.allclose(L0[:, :-1, :-1, :-1], _mag().inductance(run.grid, run.magnetic.s)[:, :-1, :-1, :-1], rtol=1e-6, atol=0.0)


def test_magnetic_loss_dissipates(oracle_lib):
    nsteps = 8000
    run = magnetic_cavity(_block(3.0, 2000.0), nr_ts=nsteps)
    en, w, _ = _energy_windows(run, oracle_lib, nsteps)
    print(f"sigma* = 2000 ohm/m: energy {w[0]:.3e} -> {w[-1]:.3e}")
    assert np.all(np.isfinite(en)) and np.all(np.diff(w) <= 0), "energy grew after the source ended"
    assert w[-1] < 0.5 * w[0]


def fields_f64(e, lib64):
    """All six components of an engine of the double-precision oracle, in double: [2][3][nz][ny][nx]."""
    import ctypes
    out = np.zeros((2, 3) + e.local_shape, np.float64)
    lib64.fdtd_oracle_get_field_f64.restype = ctypes.c_int
    lib64.fdtd_oracle_get_field_f64.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    for kind in (0, 1):
        for c in range(3):
            assert lib64.fdtd_oracle_get_field_f64(e._ctx, kind, c, out[kind, c].ctypes.data) == 0
    return out


# ---- 6. the restatement against the raw operator -----------------------------------------------------------------------------------
def budget_case(make, lib32, lib64, seed, nsteps, stepper):
    """(e_x, e_ref): relative L2 error of the fields `stepper(sim, seed, nsteps)` returns, and of the float32 oracle on the raw
    operator, against the double-precision oracle on the same float32 raw coefficients, all three from the same seeded fields."""
    from helpers import seeded_fields
    fields = []
    for lib in (lib64, lib32):
        e = build_raw(make(nsteps), lib)
        seeded_fields(e, seed)
        e.run(nsteps)
        fields.append(fields_f64(e, lib64) if lib is lib64 else e.fields().astype(np.float64))
        e.close()
    got = stepper(make(nsteps), seed, nsteps).astype(np.float64)
    return rel_l2(got, fields[0]), rel_l2(fields[1], fields[0])


def budget_sim(n):
    return magnetic_cavity(lambda s: (s.add_material("block", eps_r=2.0, mu_r=3.0, sigma_m=500.0).add_box([4, 4, 3], [9, 8, 8]),
                                      s.add_material("tile", mu_r=1.5).add_box([9, 4, 3], [11, 8, 5])), nr_ts=n)


def test_restatement_agrees_with_the_raw_operator(oracle_lib):
    from helpers import load_oracle_f64
    lib64 = load_oracle_f64()

    def stepper(sim, seed, nsteps):
        r = Restatement(sim, oracle_lib, seed=seed)
        r.run(nsteps)
        return r.e.fields()
    worst = 0.0
    for seed in BUDGET_SEEDS:
        e_x, e_ref = budget_case(budget_sim, oracle_lib, lib64, seed, 300, stepper)
        print(f"seed {seed}: restatement {e_x:.3e}, float32 oracle on the raw operator {e_ref:.3e}, ratio {e_x / e_ref:.2f}")
        assert 0 < e_ref < 1e-4
        worst = max(worst, e_x / e_ref)
    assert FP32_BUDGET_F <= 10 and worst <= FP32_BUDGET_F, worst


# ---- 7. through openems_api ---------------------------------------------------------------------------------------------------------
def magnetic_patch(lib, nr_ts=1500, mue=2.0, sigma=0.0):
    """A small patch over a ground plane on a mu_r = 2, eps_r = 2 substrate, fed by a lumped port."""
    oa = pkg("openems_api")
    csx = oa.ContinuousStructure()
    csx.GetGrid().SetDeltaUnit(1e-3)
    for a, l in zip("xyz", (25, 23, 21)):
        csx.GetGrid().AddLine(a, np.arange(0.0, l + 1, 1.0))
    csx.AddMaterial("sub", epsilon=2.0, mue=mue, sigma=sigma).AddBox([5, 5, 8], [20, 18, 10])
    csx.AddMetal("gnd").AddBox([5, 5, 8], [20, 18, 8])
    csx.AddMetal("patch").AddBox([8, 8, 10], [17, 15, 10])
    f = oa.openEMS(NrTS=nr_ts, EndCriteria=0, lib=lib, cpml_cells=4)
    f.SetGaussExcite(6e9, 4e9)
    f.SetBoundaryCond(["PML_4"] * 6)
    f.SetCSX(csx)
    port = f.AddLumpedPort(1, 50.0, [10, 11, 8], [10, 11, 10], "z", 1.0)
    return f, port


def test_mue_and_sigma_reach_the_simulation(oracle_lib, tmp_path, monkeypatch):
    install(monkeypatch)
    f, port = magnetic_patch(oracle_lib, nr_ts=200, mue=2.0, sigma=150.0)
    f.Run(str(tmp_path / "m"), verbose=0)
    m = f.sim.magnetic
    assert m is not None and np.all(f.sim.vox.mu_r[8:10, 5:18, 5:20] == 2.0) and np.all(f.sim.vox.sigma_m[8:10, 5:18, 5:20] == 150.0)
    st = f.stats.magnetic
    assert st["media"] == ["sub"] and st["classes"] == m.ncls >= 2 and st["faces"] == m.faces() and sum(st["faces"]) == len(m) > 0
    assert st["lo"][2] == [5, 5, 8] and st["hi"][2] == [20, 18, 11] and st["lo"][0] == [5, 5, 8] and st["hi"][0] == [21, 18, 10]
    assert f.sim.restated.magnetic is not None and max(np.abs(p).max() for p in f.sim.restated.magnetic.iprev) > 0
    # unknown keywords stay as tolerant as they were, and a plain material stays plain
    f2, _ = magnetic_patch(oracle_lib, nr_ts=20, mue=1.0)
    f2.GetCSX().AddMaterial("odd", epsilon=1.0, density=3.0).AddBox([1, 1, 1], [2, 2, 2])
    f2.Run(str(tmp_path / "p"), verbose=0)
    assert f2.sim.magnetic is None and f2.stats.magnetic is None


# ---- 8. PMC walls ------------------------------------------------------------------------------------------------------------------
def _dyadic_lines(cells):
    """Node lines from cell sizes in units of 2^-10 m: every coordinate and every difference is exact, so a mirrored mesh has
    bit-identical metric tables."""
    return np.concatenate([[0.0], np.cumsum(np.asarray(cells, np.float64))]) * 2.0 ** -10


def _symmetric_case(axis, side, others):
    """(whole, half): grids, per-cell eps_r, PEC edges, sources and boundaries of a scene that is mirror-symmetric about the plane
    midway between its two middle node lines along `axis`, and of its half with a PMC wall on that plane (`side` 0: the upper half,
    wall on the low face; 1: the lower half, wall on the high face).  `others`: the kind of the five other faces."""
    rng = np.random.default_rng(11 + axis)
    half_cells = [rng.integers(2, 5, 7).astype(float) for _ in range(3)]           # graded, 2..4 units
    n_other = 13
    cells, lines = [], []
    for a in range(3):
        if a == axis:
            c = np.concatenate([half_cells[a][::-1], [3.0], half_cells[a]])         # 15 cells, 16 lines, symmetric; the plane halves cell 7
        else:
            c = rng.integers(2, 5, n_other - 1).astype(float)
        cells.append(c); lines.append(_dyadic_lines(c))
    n = [l.size for l in lines]
    eps = np.ones((n[2] - 1, n[1] - 1, n[0] - 1))
    pec = np.zeros((3, n[2], n[1], n[0]), bool)

    def put(lo, hi, what):                      # a box in node indices, mirrored along `axis`
        for mirror in (False, True):
            l, h = list(lo), list(hi)
            if mirror:
                l[axis], h[axis] = n[axis] - 1 - hi[axis], n[axis] - 1 - lo[axis]
            what(l, h)
    put((3, 3, 3), (6, 7, 6), lambda l, h: eps.__setitem__((slice(l[2], h[2]), slice(l[1], h[1]), slice(l[0], h[0])), 3.5))
    t1 = (axis + 1) % 3

    def plate(l, h):                            # a metal plate normal to axis + 2: edges along axis and axis + 1
        for c in (axis, t1):
            hh = list(h); hh[c] -= 1
            pec[c][l[2]:hh[2] + 1, l[1]:hh[1] + 1, l[0]:hh[0] + 1] = True
    lo_p, hi_p = [4, 4, 4], [8, 8, 8]
    lo_p[(axis + 2) % 3] = hi_p[(axis + 2) % 3] = 8
    lo_p[axis], hi_p[axis] = 5, 10             # across the symmetry plane (nodes 7 | 8), symmetric: 5 .. 10
    plate(lo_p, hi_p)
    # an even source: edges tangential to the plane, on both sides of it
    src = []
    for q in (6, 9):
        pos = [5, 5, 5]; pos[axis] = q
        src.append((t1, tuple(pos)))
    kinds = [others] * 6
    whole = dict(lines=lines, eps=eps, pec=pec, src=src, bc=list(kinds), off=0)
    # the half: node lines 7 .. 15 (side 0) or 0 .. 8 (side 1); the wall lies between its first (last) two lines
    cut = slice(7, None) if side == 0 else slice(0, 9)
    ccut = slice(7, None) if side == 0 else slice(0, 8)
    hl = [l[cut] - l[cut][0] if a == axis else l for a, l in enumerate(lines)]
    sl_c = [slice(None)] * 3; sl_c[2 - axis] = ccut
    sl_n = [slice(None)] * 4; sl_n[3 - axis] = cut
    hk = list(kinds); hk[2 * axis + side] = "PMC"
    off = 7 if side == 0 else 0
    c_keep, p_keep = src[1] if side == 0 else src[0]                 # the source on this half's side of the plane
    hsrc = [(c_keep, tuple(p_keep[a] - (off if a == axis else 0) for a in range(3)))]
    half = dict(lines=hl, eps=eps[tuple(sl_c)].copy(), pec=pec[tuple(sl_n)].copy(), src=hsrc, bc=hk, off=off)
    return whole, half


def _run_f64(case, lib64, nsteps, cpml_cells):
    from helpers import build_f64
    g = pkg("grid").RectGrid(*case["lines"])
    vox = pkg("scene").VoxelScene(case["eps"], np.zeros_like(case["eps"]), case["pec"], [])
    s = pkg("simulation").Simulation(g, vox, f0=8e9, fc=6e9, boundary=case["bc"], cpml_cells=cpml_cells, nr_ts=nsteps, end_criteria=0.0,
                                     dt=case["dt"])
    e = build_f64(s, lib64, double_tables=False)     # the float32 tables of the ABI in double arithmetic: the wall is in hmet
    e.add_source([g.flat(*p) for _, p in case["src"]], [c for c, _ in case["src"]], [1.0] * len(case["src"]))
    e.run(nsteps)
    out = fields_f64(e, lib64)
    e.close()
    return out


@pytest.mark.parametrize("axis,side,others", [(0, 0, "PEC"), (1, 1, "PEC"), (0, 0, "PML_3"), (1, 1, "PML_3")],
                         ids=["x-minus", "y-plus", "x-minus-cpml", "y-plus-cpml"])
def test_pmc_wall_is_the_symmetry_plane(axis, side, others):
    """A mirror-symmetric scene with an even source, whole, against its half behind a PMC wall, on the double-precision oracle: every
    field value of the half equals the whole's to 1e-9 of the largest value (symmetry in exact arithmetic; float64 leaves only
    rounding).  The wall sits on the first dual plane inside the face: the half keeps one node line beyond it, whose tangential
    edges are dead (the whole's are not: they are left out of the comparison, as is the normal current on that outer plane)."""
    from helpers import load_oracle_f64
    lib64 = load_oracle_f64()
    whole, half = _symmetric_case(axis, side, others)
    assert len(half["src"]) == 1 and len(whole["src"]) == 2
    gw = pkg("grid").RectGrid(*whole["lines"])
    whole["dt"] = half["dt"] = gw.courant_dt()
    nsteps = 260
    Fw = _run_f64(whole, lib64, nsteps, 3)
    Fh = _run_f64(half, lib64, nsteps, 3)
    nh = Fh.shape[4 - axis]
    cut = [slice(None)] * 5
    cut[4 - axis] = slice(half["off"], half["off"] + nh)
    Fw = Fw[tuple(cut)]
    keep = [slice(None)] * 5
    keep[4 - axis] = slice(1, None) if side == 0 else slice(0, nh - 1)      # without the outer node plane behind the wall
    a, b = Fh[tuple(keep)], Fw[tuple(keep)]
    for kind in (0, 1):
        scale = np.abs(b[kind]).max()
        assert scale > 0
        err = np.abs(a[kind] - b[kind]).max() / scale
        print(f"{'VI'[kind]}: largest difference half - whole {err:.2e} of the largest value")
        assert err <= 1e-9
    # on the wall: the tangential currents of the half are exactly zero, and so is the normal voltage
    wall = [slice(None)] * 3
    wall[2 - axis] = 0 if side == 0 else nh - 2
    for c in range(3):
        if c != axis:
            assert not Fh[1][c][tuple(wall)].any()
    assert not Fh[0][axis][tuple(wall)].any()


def test_pmc_parse_and_nf2ff_refusal():
    sim, sc = pkg("simulation"), pkg("scene")
    bc = sim.BoundarySpec.parse(["PMC", 1, "1", "PEC", "MUR", "PML_8"])
    assert bc.kinds == ("PMC", "PMC", "PMC", "PEC", "MUR", "CPML") and bc.face_cells() == (0, 0, 0, 0, 0, 8)
    assert bc.pmc_faces() == (True, True, True, False, False, False) and sim.BoundarySpec.parse("PEC").pmc_faces() is None
    g = _grid((30, 30, 30))
    n = g.shape
    vox = sc.VoxelScene(np.ones((29, 29, 29)), np.zeros((29, 29, 29)), np.zeros((3, 30, 30, 30), bool), [])
    with pytest.raises(ValueError, match="NF2FF.*PMC"):
        sim.Simulation(g, vox, f0=5e9, fc=3e9, boundary=["PMC"] + ["PML_4"] * 5, nr_ts=10, nf2ff_freqs=[5e9])
    s = sim.Simulation(g, vox, f0=5e9, fc=3e9, boundary=["PMC", "PEC", "PEC", "PMC", "MUR", "PML_4"], nr_ts=10)
    assert list(s.mur_enable) == [0, 0, 0, 0, 1, 0]
    eco = pkg("ecoperator")
    emet, hmet = eco.metric_lists(g, s.dt, pmc=s.pmc)
    e0, h0 = eco.metric_lists(g, s.dt)
    for c in range(3):
        for a in range(3):
            assert np.array_equal(emet[c][a], e0[c][a])
            want = h0[c][a].copy()
            if a != c and a == 0:
                want[0] = 0
            if a != c and a == 1:
                want[-2] = 0
            assert np.array_equal(hmet[c][a], want)
