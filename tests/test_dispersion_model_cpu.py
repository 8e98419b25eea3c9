"""Debye media (dispersion.py, scene.add_debye_material): the constant-loss-tangent fit, the discretisation and its fold into the
operator, voxeliser geometry, stability and passivity of the scheme, the Q of a filled cavity at two modes, and the API mirror.
The per-timestep correction is restated in numpy (dispersion.correction) on top of the oracle's half-steps — the oracle itself
knows nothing of dispersion — which is also what the GPU tests compare the HIP path with, bit for bit."""
import os

import numpy as np
import pytest

from conftest import ROOT, pkg
from restatement import Restatement
from test_plugin_surface_cpu import _load, _params, _same

EPS0 = pkg("constants").EPS0
MU0 = pkg("constants").MU0
FR4 = dict(eps_r=4.3, tan_delta=0.02)


def _disp():
    return pkg("dispersion")


def _grid(n=(12, 12, 10), h=1e-3):
    return pkg("grid").RectGrid(*[np.arange(k) * h for k in n])


def _graded(n=(15, 13, 14), h=1e-3, seed=3):
    """Node lines with cells between 0.7 h and 1.4 h."""
    rng = np.random.default_rng(seed)
    return pkg("grid").RectGrid(*[np.concatenate([[0.0], np.cumsum(h * rng.uniform(0.7, 1.4, k - 1))]) for k in n])


# ---- fit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [None, 3, 4])
def test_fit_conditions(K):
    d = _disp()
    f_lo, f_hi = 1.2e9, 3.7e9
    assert f_hi / f_lo <= 3.1
    m = d.fit_constant_loss_tangent(FR4["eps_r"], FR4["tan_delta"], 2.45e9, f_lo, f_hi, K=K)
    assert m.K <= 4 and (K is None or m.K == K)
    assert np.all(m.delta_eps >= 0) and np.all(m.tau > 0) and m.eps_inf >= 1 and m.kappa == 0
    f = np.linspace(f_lo, f_hi, 1001)
    e = m.eps(f)
    # closed form, written out
    w = 2 * np.pi * f
    ref = m.eps_inf + sum(de / (1 + 1j * w * t) for de, t in zip(m.delta_eps, m.tau))
    assert np.allclose(e, ref, rtol=1e-14)
    tan = -e.imag / e.real
    err_t, err_e = np.max(np.abs(tan / FR4["tan_delta"] - 1)), np.max(np.abs(e.real / FR4["eps_r"] - 1))
    print(f"K = {m.K}: tan delta within {100 * err_t:.3f} %, Re eps within {100 * err_e:.3f} %")
    assert err_t <= 0.02 and err_e <= 0.01
    assert abs(m.eps([2.45e9])[0].real - FR4["eps_r"]) <= 1e-12 * FR4["eps_r"]
    assert m.fit_info["tan_delta_error"] <= 0.02
    # relaxation frequencies log-spaced over about [f_lo / 3, 3 f_hi]
    fr = np.sort(1 / (2 * np.pi * m.tau))
    assert f_lo / 5.01 <= fr[0] <= f_lo / 1.99 and 1.99 * f_hi <= fr[-1] <= 5.01 * f_hi
    assert np.allclose(np.diff(np.log(fr)), np.diff(np.log(fr))[0])
    # kappa term of the closed form
    mk = d.DebyeMedium(m.eps_inf, 0.01, m.delta_eps, m.tau)
    assert np.allclose(mk.eps(f), ref - 1j * 0.01 / (w * EPS0), rtol=1e-14)


def test_fit_refuses_too_few_poles_and_escalates_on_wide_bands():
    d = _disp()
    with pytest.raises(ValueError, match="K = 2 cannot hold tan delta within 2 %"):
        d.fit_constant_loss_tangent(4.3, 0.02, 2.45e9, 1.2e9, 3.7e9, K=2)
    narrow = d.fit_constant_loss_tangent(4.3, 0.02, 2.45e9, 1.2e9, 3.7e9)
    wide = d.fit_constant_loss_tangent(4.3, 0.02, 2.45e9, 0.1e9, 30e9)           # 300 : 1
    assert narrow.K == 3 and narrow.K < wide.K <= 8
    f = np.geomspace(0.1e9, 30e9, 2001)
    assert np.max(np.abs(wide.tan_delta(f) / 0.02 - 1)) <= 0.02
    assert np.all(wide.delta_eps >= 0) and wide.eps_inf >= 1
    with pytest.raises(ValueError, match="K = 3 cannot"):
        d.fit_constant_loss_tangent(4.3, 0.02, 2.45e9, 0.1e9, 30e9, K=3)
    with pytest.raises(ValueError, match="K up to 8 cannot"):
        d.fit_constant_loss_tangent(4.3, 0.02, 2.45e9, 1e5, 1e13)
    for bad in (dict(eps_inf=0.9, kappa=0, delta_eps=[1], tau=[1e-10]), dict(eps_inf=2, kappa=0, delta_eps=[-1], tau=[1e-10]),
                dict(eps_inf=2, kappa=0, delta_eps=[1], tau=[0.0]), dict(eps_inf=2, kappa=0, delta_eps=[1] * 9, tau=[1e-10] * 9)):
        with pytest.raises(ValueError):
            d.DebyeMedium(**bad)


# ---- discretisation and fold -------------------------------------------------------------------------------------------------
def _fr4(f_ref=2.45e9, f_lo=1.2e9, f_hi=3.7e9, K=3):
    return _disp().fit_constant_loss_tangent(FR4["eps_r"], FR4["tan_delta"], f_ref, f_lo, f_hi, K=K)


def _filled_scene(g, med, lo, hi, unit=1e-3, name="fr4"):
    sc = pkg("scene")
    s = sc.Scene(unit=unit)
    s.add_debye_material(name, med.eps_inf, med.kappa, med.delta_eps, med.tau).add_box(lo, hi)
    return s


def test_discretise_and_fold(monkeypatch):
    d, sc, sim = _disp(), pkg("scene"), pkg("simulation")
    m = _fr4()
    dt = 0.8e-12
    alpha, beta = m.discretise(dt)
    assert np.allclose(alpha, np.exp(-dt / m.tau), rtol=1e-15)
    assert np.allclose(beta, EPS0 * m.delta_eps * (1 - np.exp(-dt / m.tau)) / dt, rtol=1e-12)
    assert np.allclose(m.one_minus_alpha(dt), 1 - alpha, rtol=1e-12)
    # dt -> 0: sum beta_k -> eps0 sum deps_k / tau_k (the high-frequency conductivity of the poles)
    assert np.allclose(m.discretise(1e-18)[1], EPS0 * m.delta_eps / m.tau, rtol=1e-6)
    a32, o32, b32 = d.tables([m, d.DebyeMedium(2.0, 0.0, [0.5], [1e-11])], dt)
    assert a32.shape == (2, 3) and a32.dtype == np.float32 and np.array_equal(a32[0], alpha.astype(np.float32))
    assert np.array_equal(o32[0], m.one_minus_alpha(dt).astype(np.float32)) and np.array_equal(b32[0], beta.astype(np.float32))
    assert np.all(b32[1, 1:] == 0) and np.all(o32[1, 1:] == 0)          # the shorter medium's padding poles carry nothing
    # the fold: exactly eps_inf and kappa + sum beta_k per cell of the medium, untouched elsewhere
    g = _graded()
    s = _filled_scene(g, m, [2, 2, 2], [9, 8, 7])
    s.add_material("air_gap", eps_r=1.0).add_box([4, 4, 2], [6, 6, 7], priority=1)
    v = sc.voxelize(s, g)
    run = sim.Simulation(g, v, f0=2.45e9, fc=1.2e9, boundary="PEC", nr_ts=10)
    on = v.debye.cell_medium == 0
    assert on.any() and not on.all()
    assert np.all(v.eps_r[on] == m.eps_inf) and np.all(v.eps_r[~on] == 1.0) and np.all(v.kappa == 0)
    kc = m.kappa + float(np.sum(m.discretise(run.dt)[1]))
    assert np.all(run.kappa_cells[on] == kc) and np.all(run.kappa_cells[~on] == 0)
    assert abs(kc - EPS0 * np.sum(m.delta_eps * (1 - np.exp(-run.dt / m.tau))) / run.dt) <= 1e-12 * kc
    seen = {}
    eo = pkg("ecoperator")
    orig = eo.build_operator

    def spy(grid, eps_r, kappa, pec, dt, lumped=()):
        seen["eps"], seen["kappa"] = eps_r, kappa
        return orig(grid, eps_r, kappa, pec, dt, lumped)

    monkeypatch.setattr(sim, "build_operator", spy)
    op = run.op
    assert seen["eps"] is v.eps_r and np.array_equal(seen["kappa"], run.kappa_cells)
    # the class count grows by the medium's own classes only: the same scene with a plain material of the folded values has as many
    s2 = sc.Scene(unit=1e-3)
    s2.add_material("plain", eps_r=m.eps_inf, kappa=kc).add_box([2, 2, 2], [9, 8, 7])
    s2.add_material("air_gap", eps_r=1.0).add_box([4, 4, 2], [6, 6, 7], priority=1)
    op2 = orig(g, *(lambda q: (q.eps_r, q.kappa, q.pec))(sc.voxelize(s2, g)), run.dt)
    assert np.array_equal(op.vv, op2.vv) and np.array_equal(op.m, op2.m)


# ---- voxeliser ---------------------------------------------------------------------------------------------------------------
def _brute_weights(g, cell_medium, m):
    nx, ny, nz = g.shape
    out = [np.zeros((nz, ny, nx)) for _ in range(3)]
    dx = [np.diff(l) for l in g.lines]
    for c in range(3):
        a1, a2 = (c + 1) % 3, (c + 2) % 3
        n = (nx, ny, nz)
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    pos = [i, j, k]
                    if pos[c] >= n[c] - 1:
                        continue
                    num = den = 0.0
                    for o1 in (-1, 0):
                        for o2 in (-1, 0):
                            q = list(pos)
                            q[a1] += o1
                            q[a2] += o2
                            if not (0 <= q[a1] < n[a1] - 1 and 0 <= q[a2] < n[a2] - 1):
                                continue
                            a = dx[a1][q[a1]] * dx[a2][q[a2]]
                            den += a
                            num += a * (cell_medium[q[2], q[1], q[0]] == m)
                    out[c][k, j, i] = num / den * g.dd[a1][pos[a1]] * g.dd[a2][pos[a2]] / g.d[c][pos[c]]
    return out


def test_voxeliser_weights_boxes_rotation_priority_merge_refusals():
    d, sc, sim = _disp(), pkg("scene"), pkg("simulation")
    g = _graded((11, 10, 9))
    m = _fr4()
    x, y, z = (l * 1e3 for l in g.lines)
    s = _filled_scene(g, m, [x[3], y[2], z[2]], [x[8], y[7], z[5]])
    v = sc.voxelize(s, g)
    dis = v.debye
    assert len(dis.media) == 1 and dis.names == [["fr4"]]
    cm = dis.cell_medium
    assert cm.shape == (8, 9, 10) and np.all(cm[2:5, 2:7, 3:8] == 0) and np.count_nonzero(cm == 0) == 3 * 5 * 5
    brute = _brute_weights(g, cm, 0)
    full = d.edge_weights(g, cm, 1)
    for c in range(3):
        assert np.allclose(full[c][0], brute[c], rtol=1e-13, atol=0)
        assert np.array_equal(full[c][0] != 0, brute[c] != 0)
        # tight boxes: every outer slab of the box holds a dispersive edge, and nothing outside it does
        (i0, j0, k0), (i1, j1, k1) = dis.lo[c], dis.hi[c]
        w = dis.w[c]
        assert w.shape == (k1 - k0, j1 - j0, i1 - i0) and np.array_equal(w, full[c][0][k0:k1, j0:j1, i0:i1])
        assert np.count_nonzero(w) == np.count_nonzero(full[c][0])
        for ax in range(3):
            assert np.any(np.take(w, 0, axis=ax)) and np.any(np.take(w, -1, axis=ax))
    # x-edges: cells 3..7 in x -> edges 3..7; y, z: nodes 2..7 and 2..5 (edges on the medium's faces get part of their area)
    assert dis.lo[0] == (3, 2, 2) and dis.hi[0] == (8, 8, 6)
    assert dis.lo[2] == (3, 2, 2) and dis.hi[2] == (9, 8, 5)
    assert len(dis) == sum(np.count_nonzero(b) for b in brute)
    # an interior edge carries the full A~/l, a face edge about half, an edge of the box's rim about a quarter
    a_l = g.dd[1][4] * g.dd[2][3] / g.d[0][5]
    assert abs(full[0][0][3, 4, 5] - a_l) <= 1e-13 * a_l
    assert 0.2 * a_l < full[0][0][2, 2, 5] / (g.dd[1][2] * g.dd[2][2] / g.d[0][5]) * a_l < 0.35 * a_l
    # priority: a plain material of higher priority owns its cells; of lower priority it does not
    for prio, owned in ((1, False), (-1, True)):
        s2 = _filled_scene(g, m, [x[3], y[2], z[2]], [x[8], y[7], z[5]])
        s2.add_material("hole", eps_r=2.0).add_box([x[4], y[3], z[2]], [x[6], y[5], z[5]], priority=prio)
        v2 = sc.voxelize(s2, g)
        assert np.all((v2.debye.cell_medium[2:5, 3:5, 4:6] == 0) == owned)
        assert np.all(v2.eps_r[2:5, 3:5, 4:6] == (m.eps_inf if owned else 2.0))
    # a rotated box: 45 degrees about z — the owned cells are those whose centres lie in the rotated box
    s3 = sc.Scene(unit=1e-3)
    mat = s3.add_debye_material("rot", m.eps_inf, 0.0, m.delta_eps, m.tau)
    ang = np.pi / 4
    M = np.eye(4)
    M[:2, :2] = [[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]
    M[:3, 3] = [x[5], y[5], 0.0]
    mat.boxes.append(sc.Box((-3.0, -1.2, z[2]), (3.0, 1.2, z[5]), 0, M))
    v3 = sc.voxelize(s3, g)
    cx, cy = g.centers(0) * 1e3 - x[5], g.centers(1) * 1e3 - y[5]
    X, Y = np.meshgrid(cx, cy)
    u_, v_ = np.cos(ang) * X + np.sin(ang) * Y, -np.sin(ang) * X + np.cos(ang) * Y
    want = (np.abs(u_) < 3.0) & (np.abs(v_) < 1.2)
    assert want.sum() >= 6 and np.array_equal(v3.debye.cell_medium[3] == 0, want) and np.all(v3.debye.cell_medium[0] == -1)
    # identical media merge; different media on one edge are refused; apart they are two media
    s4 = _filled_scene(g, m, [x[1], y[1], z[1]], [x[4], y[8], z[6]], name="a")
    s4.add_debye_material("b", m.eps_inf, m.kappa, m.delta_eps.copy(), m.tau.copy()).add_box([x[4], y[1], z[1]], [x[9], y[8], z[6]])
    v4 = sc.voxelize(s4, g)
    assert len(v4.debye.media) == 1 and v4.debye.names == [["a", "b"]] and np.count_nonzero(v4.debye.cell_medium == 0) == 8 * 7 * 5
    other = d.DebyeMedium(3.0, 0.0, [0.2], [5e-11])
    s5 = _filled_scene(g, m, [x[1], y[1], z[1]], [x[4], y[8], z[6]], name="a")
    s5.add_debye_material("c", other.eps_inf, 0.0, other.delta_eps, other.tau).add_box([x[4], y[1], z[1]], [x[9], y[8], z[6]])
    with pytest.raises(ValueError, match=r"edge at node \(4, \d, \d\) is shared by two different Debye media \('a' and 'c'\)"):
        sc.voxelize(s5, g)
    s6 = _filled_scene(g, m, [x[1], y[1], z[1]], [x[4], y[8], z[6]], name="a")
    s6.add_debye_material("c", other.eps_inf, 0.0, other.delta_eps, other.tau).add_box([x[5], y[1], z[1]], [x[9], y[8], z[6]])
    v6 = sc.voxelize(s6, g)
    assert len(v6.debye.media) == 2 and v6.debye.K == 3 and set(np.unique(v6.debye.med[0])) == {0, 1}
    # media in CPML layers are refused (8 cells on a 20-cell grid), outside them accepted
    g2 = _grid((24, 24, 24))
    inside = sc.voxelize(_filled_scene(g2, m, [9, 9, 9], [14, 14, 14]), g2)
    sim.Simulation(g2, inside, f0=2.45e9, fc=1.2e9, boundary="CPML", cpml_cells=8, nr_ts=10)
    into = sc.voxelize(_filled_scene(g2, m, [9, 9, 9], [14, 14, 17]), g2)
    with pytest.raises(ValueError, match="Debye medium 'fr4' reaches into the CPML layer z\\+"):
        sim.Simulation(g2, into, f0=2.45e9, fc=1.2e9, boundary="CPML", cpml_cells=8, nr_ts=10)
    sim.Simulation(g2, into, f0=2.45e9, fc=1.2e9, boundary="MUR", nr_ts=10)


# ---- the restatement on the oracle: port edge, stability, Q ------------------------------------------------------------------
def _edge_CL(g, eps_cells):
    """Edge capacitances C [3][nz][ny][nx] (eps_eff A~/l) and loop inductances L (mu0 A/l~) of the EC operator."""
    ea = pkg("ecoperator")._edge_average
    nx, ny, nz = g.shape

    def along(a, arr):
        s = [1, 1, 1]
        s[2 - a] = arr.size
        return arr.reshape(s)

    C, L = [], []
    for c in range(3):
        a1, a2 = (c + 1) % 3, (c + 2) % 3
        C.append(EPS0 * ea(eps_cells, g, c) * along(a1, g.dd[a1]) * along(a2, g.dd[a2]) / along(c, g.d[c]))
        L.append(MU0 * along(a1, g.d[a1]) * along(a2, g.d[a2]) / along(c, g.dd[c]) * np.ones((nz, ny, nx)))
    return np.array(C), np.array(L)


def test_port_edge_inside_medium_equals_restatement(oracle_lib):
    """A lumped port whose edges lie inside the medium: the port's conductance is part of vi_e, the correction uses that vi_e, and the
    edge's implicit equation C (V'-V)/dt + (G_port + w sum beta) (V'+V)/2 - w sum beta_k u_k = curl I holds to float32 round-off."""
    d, sc, sim = _disp(), pkg("scene"), pkg("simulation")
    g = _graded((13, 12, 11))
    m = _fr4(9e9, 5e9, 15e9)
    x, y, z = (l * 1e3 for l in g.lines)
    s = _filled_scene(g, m, [x[2], y[2], z[2]], [x[10], y[9], z[8]])
    s.add_lumped_port(1, 50.0, [x[6], y[5], z[3]], [x[6], y[5], z[6]], "z", 1.0)
    v = sc.voxelize(s, g)
    run = sim.Simulation(g, v, f0=9e9, fc=5e9, boundary="PEC", nr_ts=400, end_criteria=0.0)
    r = Restatement(run, oracle_lib)
    le = v.lumped[0]
    k, j, i = le.k, le.j, le.i
    (i0, j0, k0) = v.debye.lo[2]
    b = (k - k0, j - j0, i - i0)
    w_e = v.debye.w[2][b]
    A_l = g.dd[0][i] * g.dd[1][j] / g.d[2][k]
    assert abs(w_e - A_l) <= 1e-12 * A_l                                     # fully inside the medium
    # vi of the port edge = dt / (C (1 + dt G / 2C)) with G = kappa_cell A~/l + 1/R
    C = EPS0 * m.eps_inf * A_l
    G = run.kappa_cells[k, j, i] * A_l + le.G
    vi_want = run.dt / (C * (1 + 0.5 * run.dt * G / C))
    assert le.G > 0 and abs(r.debye.vi[2][b] / vi_want - 1) < 1e-6
    alpha, beta = m.discretise(run.dt)
    resid, scale = [], []
    for n in range(400):
        Vold = r.e.get_field(0, 2)[k, j, i] if n else np.float32(0)
        Is = [r.e.get_field(1, c) for c in range(3)]
        u_old = r.debye.u[2][(slice(None),) + b].astype(np.float64)
        r.step()
        Vnew = float(r.V[2][k, j, i])
        curl = (Is[1][k, j, i] - Is[1][k, j, i - 1]) - (Is[0][k, j, i] - Is[0][k, j - 1, i])
        src = float(run.signal[n]) * float(v.ports[0].src_amp[list(v.ports[0].src_idx).index(g.flat(i, j, k))]) if n < len(run.signal) else 0.0
        lhs = C * (Vnew - float(Vold)) / run.dt + G * 0.5 * (Vnew + float(Vold)) - w_e * float(np.sum(beta * u_old))
        resid.append(lhs - float(curl) - src * C * (1 + 0.5 * run.dt * G / C) / run.dt)
        scale.append(abs(float(curl)) + abs(C * Vnew / run.dt))
    assert max(scale) > 0 and np.abs(r.debye.u[2]).max() > 0
    assert np.max(np.abs(resid)) <= 2e-5 * max(scale), (np.max(np.abs(resid)), max(scale))


def _cavity(g, med=None, eps_plain=None, port=True, f0=9e9, fc=5e9, nr_ts=20000):
    sc, sim = pkg("scene"), pkg("simulation")
    s = sc.Scene(unit=1e-3)
    big = [-1e3] * 3, [1e3] * 3
    if med is not None:
        s.add_debye_material("fill", med.eps_inf, med.kappa, med.delta_eps, med.tau).add_box(*big)
    else:
        s.add_material("fill", eps_r=eps_plain[0], kappa=eps_plain[1]).add_box(*big)
    if port:
        x, y, z = (l * 1e3 for l in g.lines)
        s.add_lumped_port(1, 0.0, [x[5], y[4], z[4]], [x[5], y[4], z[6]], "z", 1.0)
    v = sc.voxelize(s, g)
    return sim.Simulation(g, v, f0=f0, fc=fc, boundary="PEC", nr_ts=nr_ts, end_criteria=0.0), v


def _discrete_energy(C, L, V, I_now, I_before):
    """1/2 V^n C V^n + 1/2 I^{n+1/2} L I^{n-1/2}: the quantity the loss-free leapfrog conserves exactly."""
    return 0.5 * float(np.sum(C * V.astype(np.float64) ** 2)) + 0.5 * float(np.sum(L * I_now.astype(np.float64) * I_before.astype(np.float64)))


def test_stability_and_passivity_graded_cavity(oracle_lib):
    """A closed PEC cavity on a graded mesh filled with the K = 3 FR-4 medium, at the Courant-limit dt grid.py gives, 20 000
    timesteps: after the source has stopped the discrete energy — field energy in its conserved leapfrog form plus the branch
    capacitors' 1/2 sum C_k u_k^2 — never exceeds its value at that moment, nor rises above ANY earlier value, by more than the
    relative drift the SAME cavity shows loss-free (plain eps_inf, the parent's path) over the same timesteps, times that starting
    energy; and it ends below 1e-3 of its start.  (In exact arithmetic the sum cannot grow at all: per step the fields lose
    dt G Vm^2 and each branch takes V_m C_k (u' - u) of which it stores 1/2 C_k (u'^2 - u^2), the difference
    C_k (1 - alpha)(1 + alpha)/2 (Vm - u)^2 >= 0 being the heat in its resistor.  What is left at the end is the static field of the
    charge the soft source deposited — kappa = 0 lets it stand — on which float32 rounding walks by parts in 1e5 of ITS energy.)"""
    d = _disp()
    g = _graded((13, 12, 11))
    med = _fr4(9e9, 5e9, 15e9)
    nsteps = 20000
    # loss-free yardstick: relative drift of the conserved energy, source off
    free, _ = _cavity(g, eps_plain=(med.eps_inf, 0.0), nr_ts=nsteps)
    assert free.dt == g.courant_dt()
    C, L = _edge_CL(g, np.full(free.vox.eps_r.shape, med.eps_inf))
    e = free.build(oracle_lib)
    stop = len(free.signal) + 1
    e.run(stop)
    I_prev = e.fields()[1]
    en0 = []
    for n in range(stop, nsteps):
        e.run(1)
        F = e.fields()
        en0.append(_discrete_energy(C, L, F[0], F[1], I_prev))
        I_prev = F[1]
    en0 = np.array(en0)
    drift = float(np.max(np.abs(en0 / en0[0] - 1)))
    print(f"loss-free cavity: conserved-energy drift over {nsteps - stop} timesteps {drift:.2e}")
    assert 0 < drift < 1e-3
    run, v = _cavity(g, med=med, nr_ts=nsteps)
    assert run.dt == free.dt and len(v.debye) > 0
    r = Restatement(run, oracle_lib)
    r.run(stop)
    I_prev = r.e.fields()[1]
    en = []
    for n in range(stop, nsteps):
        r.step()
        I_now = np.stack([r.e.get_field(1, c) for c in range(3)])
        en.append(_discrete_energy(C, L, np.stack(r.V), I_now, I_prev) + d.branch_energy(v.debye, r.debye.u))
        I_prev = I_now
    en = np.array(en)
    assert np.all(np.isfinite(en)) and en[0] > 0
    runmin = np.minimum.accumulate(en)
    over_start = float(np.max(en / en[0] - 1))
    worst = float(np.max(en[1:] - runmin[:-1]) / en[0])
    print(f"Debye cavity: energy {en[0]:.3e} -> {en[-1]:.3e}; most above the start {over_start:.2e}, largest rise over any earlier "
          f"value {worst:.2e} of the start (bound {drift:.2e})")
    assert over_start <= drift
    assert worst <= drift
    assert en[-1] < 1e-3 * en[0]


def _ring_down(stepper, probe, nsteps):
    """The probe voltage after each of nsteps timesteps."""
    out = np.empty(nsteps)
    for n in range(nsteps):
        stepper()
        out[n] = probe()
    return out


def _freq_and_q(sig, dt, skip):
    """Frequency from the zero crossings (exactly periodic for a decaying sinusoid) and Q = w / (2 decay rate of the amplitude) from
    the magnitudes of the extrema between them."""
    s = sig[skip:]
    zc = np.nonzero(np.signbit(s[:-1]) != np.signbit(s[1:]))[0]
    tz = zc + s[zc] / (s[zc] - s[zc + 1])
    f = (tz.size - 1) / (2.0 * (tz[-1] - tz[0]) * dt)
    pk, tp = [], []
    for a, b in zip(zc[:-1], zc[1:]):
        q = a + 1 + int(np.argmax(np.abs(s[a + 1:b + 1])))
        # parabola through the extremum and its neighbours
        y0, y1, y2 = np.abs(s[q - 1]), np.abs(s[q]), np.abs(s[q + 1])
        den = y0 - 2 * y1 + y2
        off = 0.5 * (y0 - y2) / den if den != 0 else 0.0
        pk.append(y1 - 0.25 * (y0 - y2) * off)
        tp.append(q + off)
    rate = -np.polyfit(np.array(tp) * dt, np.log(np.array(pk)), 1)[0]
    return f, 2 * np.pi * f / (2 * rate)


def test_cavity_q_flat_with_debye_and_falling_with_kappa(oracle_lib):
    """TE101 and TE103 of a 74 x 2 x 96-cell cavity filled with FR-4, each started from its own mode shape and left to ring down.
    kappa model (the parent's behaviour, the yardstick): Q = w eps / kappa, Q2 / Q1 = f2 / f1.  Debye medium: Q = Re eps / -Im eps of
    the fitted poles at the measured frequency, the same at both modes."""
    d, sc, sim = _disp(), pkg("scene"), pkg("simulation")
    na, nd = 74, 96
    n = (na + 1, 3, nd + 1)
    f1_t = 2.45e9
    # cell size so that TE101 sits at f1_t in eps_r = 4.3
    h = 299792458.0 / (2 * np.sqrt(FR4["eps_r"]) * f1_t) * np.sqrt(1 / na ** 2 + 1 / nd ** 2)
    g = _grid(n, h)
    f2_t = f1_t * np.sqrt(1 / na ** 2 + 9 / nd ** 2) / np.sqrt(1 / na ** 2 + 1 / nd ** 2)
    assert f2_t / f1_t >= 1.6
    med = d.fit_constant_loss_tangent(FR4["eps_r"], FR4["tan_delta"], f1_t, f1_t / 1.25, f2_t * 1.25)
    assert med.K <= 4
    kappa = 2 * np.pi * f1_t * EPS0 * FR4["eps_r"] * FR4["tan_delta"]
    X = np.sin(np.pi * np.arange(na + 1) / na)
    res = {}
    for model in ("kappa", "debye"):
        for mode, p in (("TE101", 1), ("TE103", 3)):
            if model == "kappa":
                run, v = _cavity(g, eps_plain=(FR4["eps_r"], kappa), port=False, f0=f1_t, fc=f1_t / 2, nr_ts=10)
                e = run.build(oracle_lib)
                stepper = lambda: e.run(1)
            else:
                run, v = _cavity(g, med=med, port=False, f0=f1_t, fc=f1_t / 2, nr_ts=10)
                r = Restatement(run, oracle_lib)
                e = r.e
                stepper = r.step
            wdt = 2 * np.pi * f2_t * run.dt
            assert wdt <= 0.03, wdt
            Vy = np.zeros((n[2], n[1], n[0]), np.float32)
            Vy[:, :2, :] = (np.sin(p * np.pi * np.arange(nd + 1) / nd)[:, None, None] * X[None, None, :]).astype(np.float32)
            e.set_field(0, 1, Vy)
            f_t = f1_t if p == 1 else f2_t
            period = 1.0 / (f_t * run.dt)
            nsteps = int(14 * period)
            sig = _ring_down(stepper, lambda: float(e.get_field(0, 1)[nd // (2 * p), 0, na // 2]), nsteps)
            res[model, mode] = _freq_and_q(sig, run.dt, int(3 * period))
    (f1k, q1k), (f2k, q2k) = res["kappa", "TE101"], res["kappa", "TE103"]
    (f1d, q1d), (f2d, q2d) = res["debye", "TE101"], res["debye", "TE103"]
    cf = lambda f: 2 * np.pi * f * EPS0 * FR4["eps_r"] / kappa
    e0 = max(abs(q1k / cf(f1k) - 1), abs(q2k / cf(f2k) - 1))
    cfd = lambda f: float(1.0 / med.tan_delta([f])[0])
    lines = [f"cavity {na} x 2 x {nd} cells of {h * 1e3:.4f} mm, FR-4 (eps_r 4.3, tan delta 0.02), w dt at TE103 {wdt:.4f}",
             f"kappa model: TE101 {f1k / 1e9:.4f} GHz Q {q1k:.2f} (closed form w eps / kappa {cf(f1k):.2f}); "
             f"TE103 {f2k / 1e9:.4f} GHz Q {q2k:.2f} ({cf(f2k):.2f}); e0 = {e0:.2e}; Q2 / Q1 = {q2k / q1k:.4f}, f2 / f1 = {f2k / f1k:.4f}",
             f"Debye K = {med.K}: TE101 {f1d / 1e9:.4f} GHz Q {q1d:.2f} (fitted poles' Re eps / -Im eps {cfd(f1d):.2f}); "
             f"TE103 {f2d / 1e9:.4f} GHz Q {q2d:.2f} ({cfd(f2d):.2f}); Q2 / Q1 = {q2d / q1d:.4f}; 1 / tan delta = {1 / FR4['tan_delta']:.1f}"]
    print("\n".join(lines))
    out = os.path.join(ROOT, "profiles", "dispersion")
    if os.environ.get("FDTD_WRITE_RECORDS") == "1":      # the committed record is rewritten on request only
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "cavity_q.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
    assert f2k / f1k >= 1.6 and f2d / f1d >= 1.6
    bar = 2 * e0 + 0.02
    assert abs(q1d / cfd(f1d) - 1) <= bar and abs(q2d / cfd(f2d) - 1) <= bar, (q1d, cfd(f1d), q2d, cfd(f2d), bar)
    assert abs(q1d * FR4["tan_delta"] - 1) <= bar and abs(q2d * FR4["tan_delta"] - 1) <= bar
    assert abs(q2d / q1d - 1) < 0.05
    assert abs((q2k / q1k) / (f2k / f1k) - 1) < 0.05


# ---- API mirror ---------------------------------------------------------------------------------------------------------------
def test_add_debye_material_to_engine_calls():
    """CSX.AddDebyeMaterial -> scene -> Simulation -> the engine call sequence (a recording stand-in for the library's Engine)."""
    oa, sim = pkg("openems_api"), pkg("simulation")
    m = _fr4()
    fd = oa.openEMS(NrTS=50, EndCriteria=1e-4)
    fd.SetGaussExcite(2.45e9, 1.2e9)
    fd.SetBoundaryCond(["PEC"] * 6)
    csx = oa.ContinuousStructure()
    fd.SetCSX(csx)
    mesh = csx.GetGrid()
    mesh.SetDeltaUnit(1e-3)
    for ax, nn in zip("xyz", (13, 12, 11)):
        mesh.AddLine(ax, np.arange(nn, dtype=float))
    p = csx.AddDebyeMaterial("fr4", order=3, epsilon=m.eps_inf, kappa=0.0, eps_delta=m.delta_eps.tolist(), eps_relax_time=m.tau.tolist())
    p.AddBox([2, 2, 2], [10, 9, 8])
    # the numbered spelling and the aliases give the same property
    q = oa.ContinuousStructure().AddDebyeMaterial("x", eps_inf=m.eps_inf, **{f"eps_delta_{k + 1}": v for k, v in enumerate(m.delta_eps)},
                                                  **{f"eps_relaxtime_{k + 1}": v for k, v in enumerate(m.tau)})
    assert q.params == p.params
    with pytest.raises(ValueError, match="order 2 needs 2"):
        oa.ContinuousStructure().AddDebyeMaterial("x", order=2, epsilon=2.0, eps_delta=[1.0], eps_relax_time=[1e-10])
    with pytest.raises(TypeError, match="unknown keyword"):
        oa.ContinuousStructure().AddDebyeMaterial("x", epsilon=2.0, eps_delta=[1.0], tau=[1e-10], plasma=1)
    assert hasattr(pkg("compat.CSXCAD").ContinuousStructure, "AddDebyeMaterial")
    grid, scene = fd._build_scene()
    mat = scene.materials[0]
    assert type(mat).__name__ == "DebyeMaterial" and mat.medium.key() == m.key() and mat.boxes[0].start == (2, 2, 2)
    v = pkg("scene").voxelize(scene, grid)
    run = sim.Simulation(grid, v, f0=2.45e9, fc=1.2e9, boundary="PEC", nr_ts=50)
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
    assert names[:3] == ["Engine", "build_operator", "set_debye"] and "set_sheets" not in names
    bo = calls[1]
    assert np.array_equal(bo[2], v.eps_r) and np.array_equal(bo[3], run.kappa_cells) and bo[3].max() > 0
    alpha, oma, beta, lo, hi, w, med = calls[2][1:]
    a64, b64 = m.discretise(run.dt)
    assert np.array_equal(alpha, a64.astype(np.float32)[None]) and np.array_equal(beta, b64.astype(np.float32)[None])
    assert lo[0] == (2, 2, 2) and hi[0] == (10, 10, 9) and w[0].dtype == np.float32 and w[0].shape == (7, 8, 8)
    assert run.dispersion_info()["edges"] == len(v.debye) and run.dispersion_info()["K"] == 3


def _plugin_cases(s, **kw):
    FD, PI = s.FeedDirection, s.PatchInstance
    pitch = 0.0612
    arr = [PI(name=f"P{n}", params=_params(), center_x_m=(ix - 0.5) * pitch, center_y_m=(iy - 0.5) * pitch, center_z_m=0.0,
              feed_direction=FD.NEG_X) for n, (ix, iy) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)])]
    return {
        "fixed_2g45": lambda: s.prepare_hip_patch_fixed(_params(), **kw),
        "microstrip_negx": lambda: s.prepare_hip_microstrip_patch(_params(), feed_direction=FD.NEG_X, boundary="MUR", theta_step_deg=2.0, **kw),
        "microstrip3d_5g8_pml_q3": lambda: s.prepare_hip_microstrip_patch_3d(_params(5.8e9), feed_direction=FD.NEG_X, boundary="PML_8",
                                                                           theta_step_deg=2.0, phi_step_deg=5.0, mesh_quality=3, **kw),
        "multi_2x2": lambda: s.prepare_hip_microstrip_multi_3d(arr, boundary="PML_8", theta_step_deg=2.0, phi_step_deg=5.0, mesh_quality=3, **kw),
        "legacy_2g45": lambda: s.prepare_hip_patch(_params(), **kw),
    }


@pytest.mark.parametrize("name", ["fixed_2g45", "microstrip_negx", "microstrip3d_5g8_pml_q3", "multi_2x2", "legacy_2g45"])
def test_plugin_calls_default_off_and_on(name):
    """substrate_dispersion=False: the call log is the committed golden one, call for call.  True: the same log except that every
    substrate is an AddDebyeMaterial whose poles give the tan delta the USER typed over the excitation band (so no 1e-3 quirk in the
    fixed variant), with Re eps(f0) = eps_r; a loss tangent of 0 gives a plain loss-free material."""
    s = pkg("solver_fdtd_hip")
    gold = _load("scene_calls.json")[name]["calls"]
    off = _plugin_cases(s, substrate_dispersion=False)[name]()
    assert off.ok, off.message
    _same(off.FDTD.calls, gold, name)
    on = _plugin_cases(s, substrate_dispersion=True)[name]()
    assert on.ok, on.message
    calls = on.FDTD.calls
    assert len(calls) == len(gold)
    diff = [(a, b) for a, b in zip(off.FDTD.calls, calls) if a != b]
    assert len(diff) == (4 if name == "multi_2x2" else 1), diff
    f0 = 5.8e9 if "5g8" in name else 2.45e9
    for a, b in diff:
        assert a["op"] == "AddMaterial" and b["op"] == "AddDebyeMaterial" and a["name"] == b["name"] and a["name"].startswith("substrate")
        med = _disp().DebyeMedium(b["epsilon"], b["kappa"], b["eps_delta"], b["eps_relax_time"])
        assert b["order"] == med.K == 3 and b["kappa"] == 0.0
        assert abs(med.eps([f0])[0].real / 4.3 - 1) < 1e-12
        f = np.linspace(*_disp().substrate_band(f0, 0.5 * f0), 101)
        assert f[0] == 0.5 * f0 and f[-1] == 1.5 * f0
        assert np.max(np.abs(med.tan_delta(f) / 0.02 - 1)) <= 0.02
    if name == "fixed_2g45":      # the quirk is in the plain material only
        assert abs(diff[0][0]["kappa"] / (1e-3 * 2 * np.pi * f0 * EPS0 * 4.3 * 0.02) - 1) < 1e-9
        P = pkg("params").PatchAntennaParams
        p0 = P.from_user_units(frequency_ghz=2.45, er=4.3, h_mm=1.6, loss_tangent=0.0)
        c0 = s.prepare_hip_patch_fixed(p0, substrate_dispersion=True).FDTD.calls
        assert not any(c["op"] == "AddDebyeMaterial" for c in c0)
        assert [c for c in c0 if c["op"] == "AddMaterial"] == [{"op": "AddMaterial", "name": "substrate", "epsilon": 4.3, "kappa": 0.0}]
        both = s.prepare_hip_patch_fixed(_params(), substrate_dispersion=True, metal_loss=True).FDTD.calls
        assert any(c["op"] == "AddDebyeMaterial" for c in both) and any(c["op"] == "AddConductingSheet" for c in both)
