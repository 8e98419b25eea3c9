"""Conformal (Dey-Mittra) PEC boundaries (conformal.py, Simulation(conformal=True)): the cut edges' fractions on known geometry, the
area rules, the spectral bound behind dt = courant_dt / sqrt(R), the engine's correction (restated in numpy on top of the oracle's
half-steps — what the GPU tests compare the HIP path with, bit for bit) against the equivalent raw operator the oracle steps as it
is, TM010 of a cylindrical cavity against the staircase, the energy of a long run, the refusals and the off switch."""
import os

import numpy as np
import pytest

from conftest import ROOT, pkg
from helpers import rel_l2
from restatement import Restatement, install

C0 = 299792458.0
KAT = os.path.join(ROOT, "profiles", "conformal", "kat.txt")
RATIOS = (1.0, 2.0, 4.0)
RADII = (20.0, 20.25, 20.5, 20.75)


def _cf():
    return pkg("conformal")


def _uniform(n, h=1e-3):
    return pkg("grid").RectGrid(*[np.arange(k) * h for k in n])


def _graded16(seed=5, n=(17, 16, 15), h=1e-3):
    """About 16^3 nodes, cells between 0.75 h and 1.3 h."""
    rng = np.random.default_rng(seed)
    return pkg("grid").RectGrid(*[np.concatenate([[0.0], np.cumsum(h * rng.uniform(0.75, 1.3, k - 1))]) for k in n])


def _note(tag, lines):
    """Replace the block `tag` of profiles/conformal/kat.txt when FDTD_WRITE_KAT is set (the committed record of the measured values)."""
    if not os.environ.get("FDTD_WRITE_KAT"):
        return
    os.makedirs(os.path.dirname(KAT), exist_ok=True)
    old = open(KAT).read().split("\n") if os.path.isfile(KAT) else []
    keep, skip = [], False
    for l in old:
        if l.startswith("## "):
            skip = l == f"## {tag}"
        if not skip and l != "":
            keep.append(l)
    with open(KAT, "w") as fh:
        fh.write("\n".join(keep + [f"## {tag}"] + list(lines)) + "\n")


# ---- scenes shared with test_conformal_gpu.py ----------------------------------------------------------------------------------
def sphere_scene(centre=(12.4, 10.7, 5.2), radius=5.3, tilted_disc=False):
    sc = pkg("scene")
    s = sc.Scene(unit=1e-3)
    s.add_metal("ball").add_sphere(centre, radius)
    if tilted_disc:
        # a disc 1.6 cells thick (a tilted disc of zero thickness holds no node of the mesh), tilted about x and y
        from primitives_cases import rot
        m = s.add_metal("dish")
        m.add_cylinder((0.0, 0.0, -0.8), (0.0, 0.0, 0.8), 4.1)
        m.boxes[-1].matrix = rot(0, 27.0) @ rot(1, 19.0)
        m.boxes[-1].matrix[:3, 3] = (19.3, 15.6, 5.4)
    return s


def sphere_sim(n=(26, 23, 11), nr_ts=200, boundary="PEC", cpml_cells=None, ratio=2.0, conformal=True, grid=None, **kw):
    sc, sim = pkg("scene"), pkg("simulation")
    g = _uniform(n) if grid is None else grid
    s = sphere_scene(**kw)
    vox = sc.voxelize(s, g, conformal=True)
    return sim.Simulation(g, vox, f0=12e9, fc=6e9, boundary=boundary, cpml_cells=cpml_cells, nr_ts=nr_ts, end_criteria=0.0,
                          conformal=conformal, conformal_ratio=ratio)


def build_raw(sim, lib, conformal="own"):
    """An engine of `lib` on the equivalent raw operator (conformal.raw_operator): the independent reference."""
    conf = sim.conformal if isinstance(conformal, str) else conformal
    op = sim.op

    class _Raw:
        def classes(self, *a):
            return None

        def raw(self, k0=0, nk=None):
            return _cf().raw_operator(op, conf, k0, nk)
    saved = sim.conformal, sim.device_operator, sim.use_classes
    sim.conformal, sim.device_operator, sim.use_classes, sim._op = None, False, False, _Raw()
    try:
        return sim.build(lib)
    finally:
        sim.conformal, sim.device_operator, sim.use_classes = saved
        sim._op = op


def circular_patch_script(oe, lib=None, device=0, conformal=True, nr_ts=400):
    """primitives_cases.probe_patch_script (a coax-probe-fed circular patch) with conformal boundaries."""
    FDTD = oe.openEMS(NrTS=nr_ts, EndCriteria=0, lib=lib, device=device, cpml_cells=4, conformal=conformal)
    FDTD.SetGaussExcite(6e9, 3e9)
    FDTD.SetBoundaryCond(["PML_4"] * 6)
    CSX = oe.ContinuousStructure()
    FDTD.SetCSX(CSX)
    mesh = CSX.GetGrid()
    mesh.SetDeltaUnit(1e-3)
    mesh.AddLine("x", np.arange(25) - 12.0)
    mesh.AddLine("y", np.arange(25) - 12.0)
    mesh.AddLine("z", np.arange(17) - 6.0)
    CSX.AddMetal("gnd").AddBox([-6, -6, 0], [6, 6, 0], priority=10)
    CSX.AddMaterial("substrate", epsilon=3.38, kappa=1e-3).AddCylinder([0, 0, 0], [0, 0, 3], 6.0, priority=1)
    CSX.AddMetal("patch").AddCylinder([0.2, -0.1, 3], [0.2, -0.1, 3], 4.53, priority=10)
    CSX.AddMetal("pin").AddCylinder([2, 0, 1], [2, 0, 3], 1.43, priority=10)
    port = FDTD.AddLumpedPort(1, 50, [2, 0, 0], [2, 0, 1], "z", 1.0, priority=5)
    return FDTD, port


# ---- 1. fractions on known geometry ---------------------------------------------------------------------------------------------
def _edge_geometry(g, fr):
    """(pos [3][n], inside coordinate, outside coordinate along the edge) of the cut edges of a Fractions."""
    nx, ny, nz = g.shape
    k, r = np.divmod(fr.idx, nx * ny)
    j, i = np.divmod(r, nx)
    pos = np.stack([i, j, k])
    c = fr.comp.astype(np.int64)
    ar = np.arange(fr.idx.size)
    lo = np.stack([g.lines[a][pos[a]] for a in range(3)])[c, ar]
    p1 = pos.copy(); p1[c, ar] += 1
    hi = np.stack([g.lines[a][p1[a]] for a in range(3)])[c, ar]
    inside_hi = fr.node_in.reshape(-1)[g.flat(p1[0], p1[1], p1[2])]
    return pos, np.where(inside_hi, hi, lo), np.where(inside_hi, lo, hi)


def test_fractions_of_a_disc_and_a_sphere_against_the_closed_form():
    """The crossing of an x-edge with a disc / a sphere is at cx +- sqrt(re^2 - dy^2 (- dz^2)), re = r + tol (metals hold what is
    within tol of their surface): f_e to the bisection's resolution 2^-32 (twice that: the crossing lies between t_a and t_b)."""
    cf, sc = _cf(), pkg("scene")
    g = _graded16()
    L = [l[-1] * 1e3 for l in g.lines]
    zd = float(g.z[6]) * 1e3
    for what in ("disc", "sphere"):
        s = sc.Scene(unit=1e-3)
        m = s.add_metal("m")
        c = (0.47 * L[0], 0.52 * L[1], zd if what == "disc" else 0.45 * L[2])
        r = 0.31 * min(L)
        (m.add_cylinder(c, c, r) if what == "disc" else m.add_sphere(c, r))
        fr = cf.fractions(s, g)
        tol = fr.table.tol
        pos, x_in, x_out = _edge_geometry(g, fr)
        q = np.flatnonzero(fr.comp == 0)
        assert q.size >= 8
        y, z = g.y[pos[1][q]], g.z[pos[2][q]]
        re = r * 1e-3 + tol
        dz2 = 0.0 if what == "disc" else (z - c[2] * 1e-3) ** 2
        half = np.sqrt(re ** 2 - (y - c[1] * 1e-3) ** 2 - dz2)
        xc = c[0] * 1e-3 + np.where(x_out[q] > x_in[q], half, -half)
        want = 1.0 - (xc - x_in[q]) / (x_out[q] - x_in[q])
        assert np.all((fr.f[q] > 0) & (fr.f[q] <= 1))
        free = fr.f[q] != 1.0                                      # (not snapped)
        assert free.sum() >= 8
        err = np.abs(fr.f[q] - want)[free].max()
        print(f"{what}: {q.size} cut x-edges, largest |f - closed form| = {err:.2e} (resolution {2.0 ** -31:.2e})")
        assert err <= 2.0 ** -31 + 1e-12
        if what == "disc":                                         # the edges that leave the disc's plane are free over their whole length
            assert np.all(fr.f[fr.comp == 2] == 1.0) and np.count_nonzero(fr.comp == 2) > 0


def test_fractions_of_a_rotated_box_end_on_its_surface():
    """A box rotated by 31.7 degrees about z and 12 degrees about x: every crossing x_in + (1 - f) d lies on the (grown) surface to
    the bisection's resolution — the largest of the box's six signed local distances is zero there."""
    from primitives_cases import rot
    cf, sc = _cf(), pkg("scene")
    g = _graded16()
    s = sc.Scene(unit=1e-3)
    m = s.add_metal("slab")
    lo, hi = np.array([-4.1, -2.7, -1.9]), np.array([3.9, 3.1, 2.3])
    m.add_box(lo, hi)
    M = rot(2, 31.7) @ rot(0, 12.0)
    M[:3, 3] = (8.3, 7.4, 6.9)
    m.boxes[-1].matrix = M
    fr = cf.fractions(s, g)
    assert fr.idx.size > 50 and np.all((fr.f > 0) & (fr.f <= 1)) and set(np.unique(fr.comp)) == {0, 1, 2}
    pos, x_in, x_out = _edge_geometry(g, fr)
    P = np.stack([g.lines[a][pos[a]] for a in range(3)])
    P[fr.comp.astype(np.int64), np.arange(fr.idx.size)] = x_in + (1.0 - fr.f) * (x_out - x_in)
    Mm = M.copy(); Mm[:3, 3] *= 1e-3
    loc = np.linalg.inv(Mm)[:3] @ np.vstack([P, np.ones(P.shape[1])])
    tol = fr.table.tol
    out = np.maximum((lo * 1e-3 - tol)[:, None] - loc, loc - (hi * 1e-3 + tol)[:, None]).max(axis=0)     # signed distance, > 0 outside
    free = fr.f != 1.0
    err = np.abs(out[free] / np.abs(x_out - x_in)[free]).max()
    print(f"rotated box: {fr.idx.size} cut edges, crossings off the surface by at most {err:.2e} of the edge")
    assert free.sum() > 50 and err <= 2.0 ** -31 + 1e-9


def test_boxes_on_mesh_lines_cut_nothing_and_area_rules():
    cf, sc = _cf(), pkg("scene")
    g = _graded16()
    x, y, z = (l * 1e3 for l in g.lines)
    s = sc.Scene(unit=1e-3)
    s.add_metal("block").add_box([x[3], y[4], z[2]], [x[9], y[11], z[7]])
    s.add_metal("plate").add_box([x[2], y[2], z[10]], [x[13], y[12], z[10]])
    vox = sc.voxelize(s, g, conformal=True)
    fr = vox.fractions
    assert fr.idx.size > 0 and np.all(fr.f == 1.0)                 # every crossing is within the snap distance of the inside node
    assert cf.make_faces(g, fr, vox.pec) is None
    run = pkg("simulation").Simulation(g, vox, f0=9e9, fc=5e9, boundary="PEC", nr_ts=10, conformal=True)
    assert run.conformal is None and run.dt == g.courant_dt() and run.conformal_info() is None
    # the area rules on hand cases: corners (00, 10, 01, 11), edges e0: 00-01, e1: 10-11, e2: 00-10, e3: 01-11
    T, F = np.array([True]), np.array([False])
    one = lambda v: np.array([v])

    def area(corners, f, cut):
        return float(cf.area_fraction([T if c else F for c in corners], [one(v) for v in f], [T if c else F for c in cut])[0])
    assert area((0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0)) == 1.0
    assert area((1, 1, 1, 1), (1, 1, 1, 1), (0, 0, 0, 0)) == 1.0
    # one corner (00) inside: the edges at it are e0 and e2
    assert area((1, 0, 0, 0), (0.75, 1, 0.5, 1), (1, 0, 1, 0)) == 1 - 0.5 * 0.25 * 0.5
    assert area((0, 0, 0, 1), (1, 0.25, 1, 0.5), (0, 1, 0, 1)) == 1 - 0.5 * 0.75 * 0.5
    # two adjacent (00, 10): e2 lies in the metal, e0 and e1 are cut
    assert area((1, 1, 0, 0), (0.25, 0.5, 1, 1), (1, 1, 0, 0)) == 0.5 * (0.25 + 0.5)
    assert area((0, 1, 0, 1), (1, 1, 0.75, 0.125), (0, 0, 1, 1)) == 0.5 * (0.75 + 0.125)
    # three inside (all but 11): e1 and e3 are cut
    assert area((1, 1, 1, 0), (1, 0.5, 1, 0.25), (0, 1, 0, 1)) == 0.5 * 0.5 * 0.25
    assert area((0, 1, 1, 1), (0.5, 1, 0.75, 1), (1, 0, 1, 0)) == 0.5 * 0.5 * 0.75
    # two diagonal (00, 11): all four cut
    assert area((1, 0, 0, 1), (0.75, 0.5, 0.25, 0.5), (1, 1, 1, 1)) == 1 - 0.5 * 0.25 * 0.75 - 0.5 * 0.5 * 0.5
    assert area((0, 1, 1, 0), (0.75, 0.5, 0.25, 0.5), (1, 1, 1, 1)) == 1 - 0.5 * 0.5 * 0.75 - 0.5 * 0.25 * 0.5
    # the clamp: every g_e of every listed face is at most R, equal to f_e / a_f, and a_f is never below the geometric value
    for R in RATIOS:
        conf = sphere_sim(ratio=R, grid=g, centre=(7.1, 6.8, 6.3), radius=5.3).conformal
        assert len(conf) > 100 and np.all(conf.g <= R * (1 + 1e-15)) and np.all(conf.a >= conf.a_geo) and np.all(conf.a_geo > 0)
        assert (conf.clamped > 0) and conf.dt_factor == 1 / np.sqrt(R)
    with pytest.raises(ValueError, match="conformal_ratio"):
        sphere_sim(ratio=0.5)


# ---- 2. the spectral bound ------------------------------------------------------------------------------------------------------
def _curl_matrix(shape):
    """C [3 N x 3 N] of the H update: (C V)(n, p) = V_a2(p) - V_a2(p + e_a1) - V_a1(p) + V_a1(p + e_a2) on the faces that exist."""
    import scipy.sparse as sp
    nx, ny, nz = shape
    N = nx * ny * nz
    st = (1, nx, nx * ny)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    pos = (i.ravel(), j.ravel(), k.ravel())
    p = np.arange(N)
    rows, cols, vals = [], [], []
    for n in range(3):
        a1, a2 = (n + 1) % 3, (n + 2) % 3
        ok = (pos[a1] < shape[a1] - 1) & (pos[a2] < shape[a2] - 1)
        for (c, off), sgn in zip(_cf().face_edges(n), (1.0, -1.0, -1.0, 1.0)):
            rows.append(n * N + p[ok]); cols.append(c * N + p[ok] + (0 if off is None else st[off])); vals.append(np.full(ok.sum(), sgn))
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(3 * N, 3 * N))


def test_spectral_bound_of_the_clamped_operator():
    """lambda_max of the symmetric factor (F P)^1/2 C^T D C (F P)^1/2 = B^T B, B = diag(iv')^1/2 C diag(vi')^1/2: the leapfrog is
    stable iff lambda_max <= 4 (vi iv carries dt^2).  At dt = courant_dt / sqrt(R), with every g_e <= R, for R = 1, 2 and 4 — the
    analytic bound of conformal.py, asserted as it stands."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import svds
    g = _graded16()
    C = _curl_matrix(g.shape)
    out = []
    for R in RATIOS:
        run = sphere_sim(ratio=R, grid=g, centre=(7.1, 6.8, 6.3), radius=5.3)
        assert run.conformal is not None and run.dt == g.courant_dt() / np.sqrt(R)
        _, vi, _, iv = _cf().raw_operator(run.op, run.conformal)
        assert vi.min() >= 0 and iv.min() >= 0
        B = sp.diags(np.sqrt(iv.astype(np.float64).ravel())) @ C @ sp.diags(np.sqrt(vi.astype(np.float64).ravel()))
        lam = float(svds(B, k=1, return_singular_vectors=False, tol=1e-10)[0]) ** 2
        _, vi0, _, iv0 = run.op.raw()
        B0 = sp.diags(np.sqrt(iv0.astype(np.float64).ravel())) @ C @ sp.diags(np.sqrt(vi0.astype(np.float64).ravel()))
        lam0 = float(svds(B0, k=1, return_singular_vectors=False, tol=1e-10)[0]) ** 2
        out.append(f"R = {R:g}: lambda_max = {lam:.4f} (staircase at the same dt: {lam0:.4f}; bound 4), {len(run.conformal)} faces, {run.conformal.clamped} clamped")
        print(out[-1])
        assert lam <= 4.0
    _note("spectral bound (sphere r = 5.3 cells, graded 17 x 16 x 15)", out)


# ---- 3. the two forms agree ------------------------------------------------------------------------------------------------------
def test_correction_form_agrees_with_the_raw_operator(oracle_lib):
    """A: the oracle's half-steps plus conformal.correction (the engine's arithmetic).  B: the oracle on raw_operator in one run.
    300 steps from the same seeded fields (V' = f V).  The I fields and f V against V' agree within 4 times the float32 floor: the
    relative L2 difference between the float32 and the double oracle on run B, a number that does not depend on the correction."""
    from helpers import load_oracle_f64
    from test_magnetic_model_cpu import fields_f64
    lib64 = load_oracle_f64()
    nsteps, seed = 300, 3
    g = _graded16()
    mk = lambda: sphere_sim(nr_ts=nsteps, grid=g, centre=(7.1, 6.8, 6.3), radius=5.3)
    a = Restatement(mk(), oracle_lib, seed=seed)
    f = a.sim.conformal.frac.dense()
    start = a.e.fields()
    a.run(nsteps)
    A = a.e.fields().astype(np.float64)
    A[0] *= f
    res = []
    for lib in (oracle_lib, lib64):
        e = build_raw(mk(), lib)
        for c in range(3):
            e.set_field(0, c, (start[0][c].astype(np.float64) * f[c]).astype(np.float32))
            e.set_field(1, c, start[1][c])
        e.run(nsteps)
        res.append(fields_f64(e, lib64) if lib is lib64 else e.fields().astype(np.float64))
        e.close()
    floor = max(rel_l2(res[0][k], res[1][k]) for k in (0, 1))
    err = max(rel_l2(A[k], res[1][k]) for k in (0, 1))
    line = f"correction form against the raw operator in double, 300 steps: {err:.3e}; float32 floor of the raw form {floor:.3e}; ratio {err / floor:.2f} (allowed 4)"
    print(line)
    _note("two forms (sphere r = 5.3 cells, graded 17 x 16 x 15, seed 3)", [line])
    assert 0 < floor < 1e-4 and np.abs(res[1]).max() > 0
    assert err <= 4 * floor


# ---- 4. TM010 ---------------------------------------------------------------------------------------------------------------------
def peak_frequency(v, dt, f_lo, f_hi):
    """The peak of |DTFT| of the Hann-windowed series inside (f_lo, f_hi): the bin of the 8x zero-padded FFT, then a golden-section
    search between its neighbours — resolved far below 1e-4 relative (40 steps shrink the bracket by 0.618^40)."""
    n = len(v)
    w = v * np.hanning(n)
    F = np.abs(np.fft.rfft(w, 8 * n))
    f = np.fft.rfftfreq(8 * n, dt)
    band = np.flatnonzero((f > f_lo) & (f < f_hi))
    q = int(band[np.argmax(F[band])])
    t = np.arange(n) * dt
    mag = lambda fr: -abs(np.sum(w * np.exp(-2j * np.pi * fr * t)))
    a, b = f[q - 1], f[q + 1]
    gr = (np.sqrt(5) - 1) / 2
    c, d = b - gr * (b - a), a + gr * (b - a)
    for _ in range(40):
        if mag(c) < mag(d):
            b = d
        else:
            a = c
        c, d = b - gr * (b - a), a + gr * (b - a)
    return 0.5 * (a + b)


def _tm010_error(lib, na, conformal, ratio=2.0, periods=8000):
    """Relative error of TM010 of the cavity of test_primitives_cpu.test_cylindrical_cavity_tm010_on_the_oracle at an inner radius of
    `na` cells, on the oracle through raw_operator (one fdtd_run): staircased or conformal.  The run covers the same physical time
    whatever dt."""
    sc, capi, cf = pkg("scene"), pkg("_capi"), _cf()
    d = 1e-3
    a = na * d
    n = 2 * (20 + 4) + 1
    grid = pkg("grid").RectGrid((np.arange(n) - (n - 1) / 2) * d, (np.arange(n) - (n - 1) / 2) * d, np.arange(7) * d)
    s = sc.Scene(unit=1e-3)
    wall = s.add_metal("wall")
    wall.add_cylindrical_shell((0, 0, 1), (0, 0, 5), na + 1.0, 2.0)
    wall.add_box((-24, -24, 1), (24, 24, 1))
    wall.add_box((-24, -24, 5), (24, 24, 5))
    vox = sc.voxelize(s, grid, conformal=conformal)
    conf = cf.make_faces(grid, vox.fractions, vox.pec, ratio) if conformal else None
    factor = 1.0 if conf is None else conf.dt_factor
    dt = grid.courant_dt() * factor
    steps = int(round(periods / factor))
    op = pkg("ecoperator").build_operator(grid, vox.eps_r, vox.kappa, vox.pec, dt, ())
    e = capi.Engine(lib, *grid.shape, dt, max_steps=steps)
    e.set_operator_raw(*cf.raw_operator(op, conf))
    f010 = 2.405 * C0 / (2 * np.pi * a)
    e.set_signal(pkg("excitation").gauss_pulse(f010, 0.35 * f010, dt))
    ic = (n - 1) // 2
    e.add_source([grid.flat(ic + 3, ic + 2, 2)], [2], [1.0])
    pid = e.add_probe(0, [grid.flat(ic - 4, ic + 1, 3)], [2], [1.0])
    e.run(steps)
    v = e.get_probe(pid)
    e.close()
    assert np.all(np.isfinite(v)) and np.abs(v).max() > 0
    return (peak_frequency(v, dt, 0.8 * f010, 1.2 * f010) - f010) / f010


def test_tm010_conformal_against_the_staircase(oracle_lib):
    """TM010 = 2.405 c / (2 pi a) of a PEC cylindrical cavity at inner radii of 20, 20.25, 20.5 and 20.75 cells: the conformal error
    is below the staircase's at every radius, and the worst conformal error is at most half the worst staircased one (the staircase,
    the parent's behaviour, is the yardstick; R = 2, the default).  Measured (profiles/conformal/kat.txt): staircase -1.42e-2,
    -2.41e-2, -1.53e-2, -1.82e-2; conformal R = 2 +1.8e-3, -5.6e-3, +9e-4, -9e-4.  TM010 has E along the axis only, so no cut edge
    carries a voltage: what corrects the frequency is the area fraction a_f alone, and R = 1 (a_f clamped back to 1 wherever a face
    has a whole free edge) leaves the staircase's value."""
    stair = [_tm010_error(oracle_lib, na, False) for na in RADII]
    conf = {R: [_tm010_error(oracle_lib, na, True, R) for na in RADII] for R in ((2.0,) if not os.environ.get("FDTD_WRITE_KAT") else RATIOS)}
    lines = ["inner radius [cells]: " + ", ".join(f"{na:g}" for na in RADII),
             "staircase:           " + ", ".join(f"{e:+.3e}" for e in stair)]
    lines += [f"conformal R = {R:g}:     " + ", ".join(f"{e:+.3e}" for e in conf[R]) for R in conf]
    print("\n".join(lines))
    _note("TM010 of a PEC cylindrical cavity, relative frequency error (1 mm cells, 8000 Courant steps of physical time)", lines)
    for es, ec in zip(stair, conf[2.0]):
        assert abs(ec) < abs(es)
    assert max(map(abs, conf[2.0])) <= 0.5 * max(map(abs, stair))


# ---- 5. energy -------------------------------------------------------------------------------------------------------------------
def test_energy_does_not_grow_over_20000_steps(oracle_lib):
    """The sphere scene in a closed PEC box on the graded mesh, stepped on raw_operator at dt = courant_dt / sqrt(2): 20 000 steps
    after the pulse has ended the conserved leapfrog energy sum V'^2 / vi' + sum I^{n+1/2} I^{n-1/2} / iv' (constant in exact
    arithmetic whenever the scheme is stable) has not grown.  In float32 each V' and each I is rounded once per timestep (one fma
    each), 2^-24 relative, the energy is quadratic: 4 * 2^-24 per timestep in the linear worst case is the bound, over the whole run
    and between the maxima of consecutive 2000-step windows."""
    nsteps, every = 20000, 100
    g = _graded16()
    run = sphere_sim(nr_ts=10 ** 6, grid=g, centre=(7.1, 6.8, 6.3), radius=5.3)
    e = build_raw(run, oracle_lib)
    _, vi, _, iv = _cf().raw_operator(run.op, run.conformal)
    e.set_signal(run.signal)
    e.add_source([g.flat(14, 12, 3)], [2], [1.0])
    wv = np.where(vi > 0, 1.0 / np.where(vi > 0, vi, 1).astype(np.float64), 0.0)
    wi = np.where(iv > 0, 1.0 / np.where(iv > 0, iv, 1).astype(np.float64), 0.0)
    e.run(len(run.signal) + 1)
    en = []
    for _ in range(nsteps // every):
        e.run(every - 1)
        before = np.stack([e.get_field(1, c) for c in range(3)]).astype(np.float64)
        e.run(1)
        F = e.fields().astype(np.float64)
        en.append(float(np.sum(wv * F[0] ** 2) + np.sum(wi * F[1] * before)))
    en = np.array(en)
    w = en.reshape(-1, 20).max(axis=1)
    per_step = 4 * 2.0 ** -24
    rise, above = float(np.max(np.diff(w)) / w[0]), float(np.max(en) / en[0] - 1)
    line = (f"energy over {nsteps} steps at R = 2: {en[0]:.6e} -> {en[-1]:.6e}; most above the start {above:+.2e} (bound {nsteps * per_step:.2e}); "
            f"largest rise between window maxima {rise:+.2e} (bound {2 * 2000 * per_step:.2e}); spread {np.ptp(en) / en[0]:.2e}")
    print(line)
    _note("energy (sphere r = 5.3 cells, graded 17 x 16 x 15, closed PEC box)", [line])
    assert np.all(np.isfinite(en)) and en[0] > 0
    assert above <= nsteps * per_step and rise <= 2 * 2000 * per_step


# ---- 6. refusals and the off switch ----------------------------------------------------------------------------------------------
def test_refusals_name_the_metal_and_the_node():
    sc, sim = pkg("scene"), pkg("simulation")
    with pytest.raises(ValueError, match=r"(?s)'ball'.*node \(\d+, \d+, \d+\).*CPML layer"):
        sphere_sim(boundary="CPML", cpml_cells=4)
    with pytest.raises(ValueError, match=r"(?s)'ball'.*node \(\d+, \d+, \d+\).*Mur face z"):
        sphere_sim(boundary=["PEC"] * 4 + ["MUR", "PEC"])
    ok = sphere_sim(n=(30, 28, 24), boundary="CPML", cpml_cells=4, centre=(14.4, 13.7, 11.3), radius=4.3)
    assert ok.conformal is not None and len(ok.conformal) > 50
    g = _uniform((26, 23, 15))
    s = sphere_scene(centre=(12.4, 10.7, 7.2), radius=4.3)
    s.add_material("ferrite", eps_r=2.0, mu_r=3.0).add_box([5, 5, 2], [20, 18, 12])
    with pytest.raises(ValueError, match=r"(?s)'ball'.*node \(\d+, \d+, \d+\).*magnetic face"):
        sim.Simulation(g, sc.voxelize(s, g, conformal=True), f0=9e9, fc=5e9, boundary="PEC", nr_ts=10, conformal=True)
    with pytest.raises(ValueError, match="conformal=True needs the fractions"):
        sim.Simulation(g, sc.voxelize(s, g), f0=9e9, fc=5e9, boundary="PEC", nr_ts=10, conformal=True)
    with pytest.raises(pkg("_capi").FdtdError, match="single slab"):
        sphere_sim(n=(26, 23, 15), centre=(12.4, 10.7, 7.2), radius=4.3).build(None, world=2, rank=0)
    # conducting sheets do not count: a sheet sphere cuts nothing
    s2 = sc.Scene(unit=1e-3)
    s2.add_conducting_sheet("tin", 9.1e6, 5e-6).add_sphere((12.4, 10.7, 7.2), 4.3)
    assert sc.voxelize(s2, g, conformal=True).fractions.idx.size == 0


def test_the_off_switch_changes_nothing():
    """With conformal=False (the default) dt, the operator and every table of the Simulation are what they are without the fractions;
    and asking voxelize for the fractions changes no other field of the VoxelScene."""
    sc, sim = pkg("scene"), pkg("simulation")
    g = _uniform((26, 23, 11))
    s = sphere_scene(tilted_disc=True)
    s.add_material("sub", eps_r=3.3, kappa=0.01).add_box([2, 2, 1], [22, 20, 3])
    s.add_lumped_port(1, 50.0, [21, 19, 1], [21, 19, 3], "z", 1.0)
    v0, v1 = sc.voxelize(s, g), sc.voxelize(s, g, conformal=True)
    assert v0.fractions is None and v1.fractions is not None and v1.fractions.idx.size > 0
    for name in ("eps_r", "kappa", "pec", "mu_r", "sigma_m", "cell_material"):
        assert np.array_equal(getattr(v0, name), getattr(v1, name)), name
    kw = dict(f0=9e9, fc=5e9, boundary="PEC", nr_ts=50)
    a, b, on = sim.Simulation(g, v0, **kw), sim.Simulation(g, v1, **kw), sim.Simulation(g, v1, conformal=True, **kw)
    assert a.conformal is None and b.conformal is None and on.conformal is not None
    assert a.dt == b.dt == g.courant_dt() and on.dt == g.courant_dt() / np.sqrt(2.0)
    assert np.array_equal(a.signal, b.signal)
    for x, y in zip(a.op.raw(), b.op.raw()):
        assert np.array_equal(x, y)
    assert a.conformal_info() is None and b.conformal_info() is None
    info = on.conformal_info()
    assert info["ratio"] == 2.0 and info["dt_factor"] == 1 / np.sqrt(2.0) and sum(info["faces"]) == len(on.conformal) and info["clamped"] >= 0
    assert info["cut_edges"] == v1.fractions.idx.size
    oe = pkg("openems_api")
    assert oe.openEMS(NrTS=10)._conformal is False and oe.openEMS(NrTS=10, conformal=True, conformal_ratio=4)._conformal_ratio == 4.0


def test_conformal_reaches_the_simulation_through_the_api(oracle_lib, tmp_path, monkeypatch):
    install(monkeypatch)
    oe = pkg("openems_api")
    f, port = circular_patch_script(oe, oracle_lib, nr_ts=60)
    f.Run(str(tmp_path / "c"), verbose=0)
    st = f.stats.conformal
    assert f.sim.conformal is not None and sum(st["faces"]) == len(f.sim.conformal) > 0 and st["ratio"] == 2.0
    assert st["dt_factor"] == 1 / np.sqrt(2.0) and f.sim.dt == f.sim.grid.courant_dt() / np.sqrt(2.0) and hasattr(f.sim, "restated")
    f2, _ = circular_patch_script(oe, oracle_lib, conformal=False, nr_ts=20)
    f2.Run(str(tmp_path / "p"), verbose=0)
    assert f2.sim.conformal is None and f2.stats.conformal is None and f2.sim.vox.fractions is None and f2.sim.dt == f2.sim.grid.courant_dt()
