"""The scenes of tests/test_ports_cpu.py and tests/test_ports_gpu.py, small on purpose, drawn through the public API.  No test functions.

WG        uniform 1 mm cells, 16 x 8 x 64; PEC on x and y, PML_8 on both z ends; a = 16 mm, b = 8 mm: TE10 cuts off at 9.37 GHz, TE20 and
          TE01 at 18.7 GHz; Gauss pulse f0 = 14 GHz, fc = 3 GHz.  Port 1 runs z = 12 -> 24 (excited), port 2 z = 52 -> 40 (passive);
          excite=(0, 1) drives port 2 instead.  WG-slab: eps_r = 4 fills z = 30..38.  WG-odd (engine-parity runs only): the measurement
          planes on z = 25 and 39.
MSL       40 (x = t) x 100 (y = prop) x 24 (z = exc) cells of 0.2 mm; PEC at z-, PML_8 elsewhere; substrate eps_r = 3.38, 4 cells high;
          the strip 8 cells wide; two ports facing each other, each starting on the inner edge of the PML, 30 cells long; Gauss pulse
          f0 = 6 GHz, fc = 5 GHz; beyond either port the strip goes on through the PML to the grid face (a line that ended on the PML's
          edge would be open-ended there).  MSL-open: the strip ends 20 cells beyond port 1's measurement line, no port 2.  MSL-feedR: port 1
          starts 12 cells inside the domain (at cell 20) with Feed_R = 50.
"""
import numpy as np
from conftest import pkg

C0 = 299792458.0
WG_A, WG_B, WG_CELL = 16e-3, 8e-3, 1e-3
WG_F0, WG_FC, WG_BAND = 14e9, 3e9, (11e9, 17e9)
WG_NRTS = 6000
WG_DIST = 16e-3                       # port 1's plane (z = 24) to port 2's (z = 40)
WG_SLAB = (30.0, 38.0, 4.0)           # z range [mm], eps_r
MSL_CELL, MSL_EPS, MSL_H, MSL_W = 0.2, 3.38, 4, 8
MSL_F0, MSL_FC, MSL_BAND = 6e9, 5e9, (2e9, 10e9)
MSL_NRTS = 5000
MSL_OPEN_BEYOND = 20                  # cells from port 1's measurement line to the open end


def wg_freqs(n=25):
    return np.linspace(*WG_BAND, n)


def msl_freqs(n=17):
    return np.linspace(*MSL_BAND, n)


def wg(lib, slab=False, excite=(1.0, 0.0), nr_ts=WG_NRTS, mode="TE10", planes=(24, 40)):
    """(fdtd, [port 1, port 2]) of the WG scene, not yet run.  `planes`: the measurement planes of the two ports."""
    api = pkg("openems_api")
    fd = api.openEMS(NrTS=nr_ts, EndCriteria=0, lib=lib)
    fd.SetGaussExcite(WG_F0, WG_FC)
    fd.SetBoundaryCond(["PEC", "PEC", "PEC", "PEC", "PML_8", "PML_8"])
    csx = api.ContinuousStructure()
    fd.SetCSX(csx)
    mesh = csx.GetGrid()
    mesh.SetDeltaUnit(1e-3)
    mesh.AddLine("x", np.arange(17.0))
    mesh.AddLine("y", np.arange(9.0))
    mesh.AddLine("z", np.arange(65.0))
    if slab:
        csx.AddMaterial("slab", epsilon=WG_SLAB[2]).AddBox([0, 0, WG_SLAB[0]], [16, 8, WG_SLAB[1]])
    p1 = fd.AddRectWaveGuidePort(1, [0, 0, 12], [16, 8, planes[0]], "z", WG_A, WG_B, mode, excite[0])
    p2 = fd.AddRectWaveGuidePort(2, [0, 0, 52], [16, 8, planes[1]], "z", WG_A, WG_B, mode, excite[1])
    return fd, [p1, p2]


def msl(lib, variant=None, nr_ts=MSL_NRTS):
    """(fdtd, ports) of the MSL scene (variant None, 'open' or 'feedR'), not yet run.  Coordinates in cells of 0.2 mm."""
    api = pkg("openems_api")
    fd = api.openEMS(NrTS=nr_ts, EndCriteria=0, lib=lib)
    fd.SetGaussExcite(MSL_F0, MSL_FC)
    fd.SetBoundaryCond(["PML_8", "PML_8", "PML_8", "PML_8", "PEC", "PML_8"])
    csx = api.ContinuousStructure()
    fd.SetCSX(csx)
    mesh = csx.GetGrid()
    mesh.SetDeltaUnit(MSL_CELL * 1e-3)
    mesh.AddLine("x", np.arange(41.0))
    mesh.AddLine("y", np.arange(101.0))
    mesh.AddLine("z", np.arange(25.0))
    csx.AddMaterial("substrate", epsilon=MSL_EPS).AddBox([0, 0, 0], [40, 100, MSL_H])
    strip = csx.AddMetal("strip")
    x0, x1 = 20 - MSL_W // 2, 20 + MSL_W // 2
    y_start = 20 if variant == "feedR" else 8
    kw = {"Feed_R": 50.0} if variant == "feedR" else {}
    p1 = fd.AddMSLPort(1, strip, [x0, y_start, 0], [x1, y_start + 30, MSL_H], "y", "z", 1.0, priority=10, **kw)
    ports = [p1]
    if variant != "feedR":     # the line goes on through the PML to the grid face: it would be open-ended at the PML's edge otherwise
        strip.AddBox([x0, 0, MSL_H], [x1, y_start, MSL_H], priority=10)
    if variant == "open":
        strip.AddBox([x0, y_start + 30, MSL_H], [x1, y_start + 15 + MSL_OPEN_BEYOND, MSL_H], priority=10)
    else:
        strip.AddBox([x0, y_start + 30, MSL_H], [x1, 62, MSL_H], priority=10)
        strip.AddBox([x0, 92, MSL_H], [x1, 100, MSL_H], priority=10)
        ports.append(fd.AddMSLPort(2, strip, [x0, 92, 0], [x1, 62, MSL_H], "y", "z", 0.0, priority=10))
    return fd, ports


_RUNS = {}


def ran(lib, key, make):
    """The scene make(lib) -> (fdtd, ports), run once per library and key and shared among the tests; treat it as read-only."""
    k = (id(lib), key)
    if k not in _RUNS:
        fd, ports = make(lib)
        fd.Run(None)
        _RUNS[k] = (fd, ports)
    return _RUNS[k]


def s_params(p_in, p_out, freqs, **kw):
    """(S11, S21) of a run that excites p_in: uf_ref / uf_inc at p_in, and the wave LEAVING the structure at p_out — its uf_ref, a port
    looks into the structure — over uf_inc at p_in (equal reference impedances)."""
    a = p_in.CalcPort(None, freqs, **kw)
    inc, s11 = a.uf_inc.copy(), a.uf_ref / a.uf_inc
    if p_out is None:
        return s11, None
    b = p_out.CalcPort(None, freqs)
    return s11, b.uf_ref / inc


# ---- references ---------------------------------------------------------------------------------------------------------------------
def yee_beta_te10(freqs, dt, cell=WG_CELL, a=WG_A, eps_r=1.0):
    """beta_d of the discrete TE10 mode on the uniform mesh, from the Yee dispersion relation
    sin^2(w dt / 2) / (c dt)^2 = sin^2(beta_d D / 2) / D^2 + sin^2(pi D / (2 a)) / D^2 (the discrete sine across the guide is an exact
    eigenmode of the difference operator)."""
    w = 2 * np.pi * np.asarray(freqs, float)
    c = C0 / np.sqrt(eps_r)
    rhs = (np.sin(w * dt / 2) / (c * dt)) ** 2 - (np.sin(np.pi * cell / (2 * a)) / cell) ** 2
    return 2.0 / cell * np.arcsin(cell * np.sqrt(rhs))


def slab_line(freqs, length=8e-3, eps_r=4.0, a=WG_A, d_in=6e-3, d_out=2e-3):
    """(S11, S21) of the three-section transmission line vacuum | slab | vacuum with the analytic beta and ZL of TE10 in each section,
    referred to planes d_in before and d_out behind the slab, reference impedance ZL of the vacuum guide."""
    ports = pkg("ports")
    kc = np.pi / a
    b0, z0 = ports.waveguide_beta_zl(freqs, kc, 1.0)
    b1, z1 = ports.waveguide_beta_zl(freqs, kc, eps_r)
    g = (z1 - z0) / (z1 + z0)
    ph = np.exp(-1j * b1 * length)
    den = 1 - g * g * ph * ph
    s11 = g * (1 - ph * ph) / den
    s21 = (1 - g * g) * ph / den
    return s11 * np.exp(-2j * b0 * d_in), s21 * np.exp(-1j * b0 * (d_in + d_out))


def hammerstad_jensen(w_over_h, eps_r):
    """(Z0, eps_eff) of a zero-thickness microstrip line (Hammerstad and Jensen 1980), quasi-static."""
    u = float(w_over_h)
    fu = 6 + (2 * np.pi - 6) * np.exp(-(30.666 / u) ** 0.7528)
    z01 = 376.730313668 / (2 * np.pi) * np.log(fu / u + np.sqrt(1 + (2 / u) ** 2))
    a = 1 + np.log((u ** 4 + (u / 52) ** 2) / (u ** 4 + 0.432)) / 49 + np.log(1 + (u / 18.1) ** 3) / 18.7
    b = 0.564 * ((eps_r - 0.9) / (eps_r + 3)) ** 0.053
    ee = (eps_r + 1) / 2 + (eps_r - 1) / 2 * (1 + 10 / u) ** (-a * b)
    return z01 / np.sqrt(ee), ee


# ---- the raw lists, for the engine-parity tests -------------------------------------------------------------------------------------
def simulation(make, nr_ts=600):
    """A Simulation of the scene make(None) -> (fdtd, ports) with its port lists, not yet built."""
    fd, _ = make(None)
    grid, sc = fd._build_scene()
    vox = pkg("scene").voxelize(sc, grid)
    bc = pkg("simulation").BoundarySpec.parse(fd._bc, None)
    return pkg("simulation").Simulation(grid, vox, f0=fd._f0, fc=fd._fc, boundary=bc, nr_ts=nr_ts, end_criteria=0)


RAW = {"WG": lambda lib: wg(lib), "WG-slab": lambda lib: wg(lib, slab=True), "MSL": lambda lib: msl(lib),
       "WG-odd": lambda lib: wg(lib, planes=(25, 39))}
RAW_STEPS = 600
# (scene, schedule, what source_probe_cases.predict must say and fdtd_schedule_info must show): every schedule for every scene.  The
# guide's planes hold 120 source edges (one strip-plane: the dense source path), 120 V-probe edges and, in the two half-planes of one
# resident tile, 240 I-probe faces: 360 probe cells in a tile, which the resident schedule refuses by name.  WG-odd moves the
# measurement planes to z = 25 and 39, where the two half-planes fall into two tiles (120 and 240 cells): the resident schedule takes it.
RAW_RUNS = [(n, s, o) for n in ("WG", "WG-slab") for s, o in (
    ("DIRECT", "two"), ("WF1", "one"), ("WFM", "one"), ("AUTO", "one"), ("RESIDENT", "refused: resident schedule: at most 256 probe cells per tile"))]
RAW_RUNS += [("WG-odd", "RESIDENT", "resident"), ("WG-odd", "AUTO", "resident")]
RAW_RUNS += [("MSL", s, o) for s, o in (("DIRECT", "two"), ("WF1", "one"), ("WFM", "one"), ("AUTO", "resident"), ("RESIDENT", "resident"))]
_RAW = {}


def raw(name):
    """(Simulation, source_probe_cases.Case of its lists) of a RAW scene: the case restates the lists the way the schedule arithmetic of
    source_probe_cases reads them (regimes, predict); probes in the order Simulation.build adds them."""
    import source_probe_cases as spc
    if name not in _RAW:
        sim = simulation(RAW[name], RAW_STEPS)
        sources = [spc.src(p.src_idx, p.src_comp, p.src_amp, np.full(p.src_idx.size, p.port.delay_steps)) for p in sim.vox.ports if p.port.excite != 0]
        probes = []
        for p in sim.vox.ports:
            probes += [spc.prb(spc.KIND_V, *q) for q in p.v_probes] + [spc.prb(spc.KIND_I, *q) for q in p.i_probes]
        case = spc.Case(name, sim.grid.shape, tuple(sim.bc.kinds), sim.bc.cpml_cells, sim.signal, sources, probes, (RAW_STEPS,))
        _RAW[name] = (sim, case)
    return _RAW[name]


def raw_engine(name, lib, flags=0):
    """A fresh engine of a RAW scene on `lib` with the port lists added by Simulation.build, and the probe ids in list order."""
    sim, _ = raw(name)
    e = sim.build(lib, flags=flags)
    ids = [q for uids, iids in sim._port_probe_lists for q in uids + iids]
    return e, ids


# The guide (65 node planes) as z-slabs of one process.  Cut at plane 24: port 1's source plane and V-plane become the bottom plane of
# the slab above the cut (every cell waits for the H halo) and its I half-planes, 23 and 24, straddle the cut; the second cut at 40
# does the same to port 2's V-plane.
WG_CUTS = {"2slabs": ((0, 24), (24, 41)), "3slabs": ((0, 24), (24, 16), (40, 25))}
WG_SLAB_TRANSPORTS = ("p2p-two", "p2p-one", "linked-split")


def slab_engines(name, lib, cuts, flags=0):
    """([engine of every rank], probe ids in list order) of a RAW scene on the slabs `cuts` = [(k0, nk)], every rank built by
    Simulation.build with the port lists unchanged (the library keeps what the rank owns)."""
    sim, _ = raw(name)
    sim.slabs = lambda world, partition="cost": list(cuts)      # (Simulation.slabs cuts by cost or evenly: these cuts are the test's)
    try:
        engines = [sim.build(lib, rank=r, world=len(cuts), flags=flags) for r in range(len(cuts))]
    finally:
        del sim.slabs
    assert [(e.k0, e.nk) for e in engines] == [tuple(s) for s in cuts]
    return engines, [q for uids, iids in sim._port_probe_lists for q in uids + iids]


def s_from_series(name, series, freqs):
    """(S11, S21) of a RAW guide scene from probe series in list order, through the ports' own post-processing (CalcPort)."""
    sim, _ = raw(name)
    fd, (p1, p2) = RAW[name](None)
    fd.sim, fd._u_i_all, at = sim, [], 0
    for p in sim.vox.ports:
        nu, ni = len(p.v_probes), len(p.i_probes)
        fd._u_i_all.append((list(series[at:at + nu]), list(series[at + nu:at + nu + ni])))
        at += nu + ni
    assert at == len(series)
    return s_params(p1, p2, freqs)


_RAW_REF = {}


def raw_reference(name, oracle_lib):
    """The oracle's run of a RAW scene, computed once: final fields, its own probe series, and per probe the series of probe_block's
    sums (source_probe_cases.tree_sum) over the oracle's fields, taken half-step by half-step.  WG: likewise per rank of every cut of
    WG_CUTS, every list clipped to the rank's planes ("slab_trees": {cut name: [rank][probe]})."""
    import source_probe_cases as spc
    if name not in _RAW_REF:
        _, case = raw(name)
        e, ids = raw_engine(name, oracle_lib)
        tree = [np.zeros(RAW_STEPS) for _ in case.probes]
        slabs = {cut: [[(np.zeros(RAW_STEPS), spc.clip_to_planes(case, p, s)) for p in case.probes] for s in cuts]
                 for cut, cuts in (WG_CUTS.items() if name == "WG" else ())}
        for step in range(RAW_STEPS):
            for phase, kind in ((0, spc.KIND_V), (1, spc.KIND_I)):
                e.half_step(phase)
                F = np.stack([e.get_field(kind, c) for c in range(3)]).reshape(3, -1)
                for q, (k, idx, comp, w) in enumerate(case.probes):
                    if k == kind:
                        tree[q][step] = spc.tree_sum(w, F[comp.astype(np.int64), idx])
                for ranks in slabs.values():
                    for probes in ranks:
                        for out, (k, idx, comp, w) in probes:
                            if k == kind:
                                out[step] = spc.tree_sum(w, F[comp.astype(np.int64), idx])
        ref = {"fields": e.fields(), "own": [e.get_probe(q) for q in ids], "tree": tree, "step": e.step,
               "slab_trees": {cut: [[out for out, _ in probes] for probes in ranks] for cut, ranks in slabs.items()}}
        for a in [ref["fields"]] + ref["own"] + ref["tree"] + [t for ranks in ref["slab_trees"].values() for probes in ranks for t in probes]:
            a.setflags(write=False)
        _RAW_REF[name] = ref
    return _RAW_REF[name]


# ---- the measured quantities: what profiles/ports/kat.txt records and tests/test_ports_cpu.py bounds -------------------------------
def _wrapped(phase):
    return np.abs(np.angle(np.exp(1j * np.asarray(phase))))


def wg_measures(lib):
    """WG and WG-slab, worst case over the band 11-17 GHz."""
    f = wg_freqs()
    fd, (p1, p2) = ran(lib, "wg", wg)
    s11, s21 = s_params(p1, p2, f)
    _, (q1, q2) = ran(lib, "wg-back", lambda l: wg(l, excite=(0.0, 1.0)))
    _, s12 = s_params(q2, q1, f)
    bd = yee_beta_te10(f, fd.sim.dt)
    _, (r1, r2) = ran(lib, "wg-slab", lambda l: wg(l, slab=True))
    t11, t21 = s_params(r1, r2, f)
    a11, a21 = slab_line(f)
    return {"wg_phase_rad": float(_wrapped(np.angle(s21) + bd * WG_DIST).max()), "wg_s11": float(np.abs(s11).max()),
            "wg_s21": float(np.abs(np.abs(s21) - 1).max()), "wg_reciprocity": float(np.abs(s21 - s12).max()),
            "slab_s11": float(np.abs(t11 - a11).max()), "slab_s21": float(np.abs(t21 - a21).max())}


def msl_measures(lib):
    """MSL, MSL-open and MSL-feedR, worst case over the band 2-10 GHz."""
    f = msl_freqs()
    _, (p1, p2) = ran(lib, "msl", msl)
    s11, s21 = s_params(p1, p2, f)
    zl = p1.ZL.copy()
    _, (o1,) = ran(lib, "msl-open", lambda l: msl(l, "open"))
    o11, _ = s_params(o1, None, f)
    o11s, _ = s_params(o1, None, f, ref_plane_shift=MSL_OPEN_BEYOND)
    _, (r1, r2) = ran(lib, "msl-feedR", lambda l: msl(l, "feedR"))
    r11, _ = s_params(r1, r2, f)
    z_hj, e_hj = hammerstad_jensen(MSL_W / MSL_H, MSL_EPS)
    return {"msl_margin": float(max(0.0, (np.abs(s11) ** 2 + np.abs(s21) ** 2 - 1).max())), "open_s11": float(np.abs(np.abs(o11) - 1).max()),
            "feedR_s11": float(np.abs(r11).max()), "shift_s11": float(np.abs(np.abs(o11s) - np.abs(o11)).max()),
            "open_phase_rad": float(np.abs(np.angle(o11s)).max()),
            # recorded, not asserted: the 0.2 mm staircase of an 8-cell strip decides them
            "zl_over_hammerstad_jensen_min": float(np.real(zl).min() / z_hj), "zl_over_hammerstad_jensen_max": float(np.real(zl).max() / z_hj)}
