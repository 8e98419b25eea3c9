"""Waveguide and microstrip-line ports without a GPU (scenes: tests/ports_cases.py; every run goes through the float32 oracle).

The lists against cases written out by hand; the orthogonality of the mode weights; the sign of the incident power on every scene; the
guide against closed forms (the Yee dispersion relation for TE10, the three-section line for the slab); the line against bounds that can
be derived; the refusals.  The bounds of the physical checks are NOT tuned here: profiles/ports/kat.txt records the worst case of each
quantity over the band from one run through the double-precision oracle (python tests/ports_kat.py), and the tests assert at twice that
value; PML reflection, grid dispersion and — for the slab, whose reference uses the analytic beta and ZL — the staircase of the mode
impedance set the values, the float32 step loop (budget 1.7e-5) does not."""
import os
import types

import numpy as np
import pytest

import ports_cases as pc
from conftest import ROOT, pkg

PEC_PML = ["PEC", "PEC", "PEC", "PEC", "PML_8", "PML_8"]


def _kat():
    out = {}
    with open(os.path.join(ROOT, "profiles", "ports", "kat.txt")) as fh:
        for line in fh:
            if "=" in line and not line.startswith("#"):
                k, v = line.split("=")
                out[k.strip()] = float(v)
    return out


KAT = _kat()


def _as_dict(grid, probe):
    """{(comp, i, j, k): weight} of a list; an entry listed twice fails."""
    nx, ny, _ = grid.shape
    out = {}
    for g, c, w in zip(probe.idx.tolist(), probe.comp.tolist(), probe.w.tolist()):
        k, r = divmod(g, nx * ny)
        key = (c, r % nx, r // nx, k)
        assert key not in out, key
        out[key] = w
    return out


def _close(got, want):
    assert set(got) == set(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-6, abs=0), (k, got[k], want[k])     # (float32 lists)


# ---- 1. the lists, by hand -----------------------------------------------------------------------------------------------------------
def test_waveguide_lists_of_a_4_by_2_cell_guide():
    """4 x 2 cells of 1 mm, TE10, z = 1 -> 4: e_y = -(1/a) sin(pi x / a) on the y edges of the node lines i = 1, 2, 3 (i = 0 and 4 are
    the walls: weight zero, not listed), no x edge (e_x = 0); h_x = (1/a) sin(pi x / a) on the x faces of the same lines.
    N_e = N_h = 250^2 * 1e-6 * (1/2 + 1 + 1/2) * 2 = 0.25."""
    ports, grid_m = pkg("ports"), pkg("grid")
    grid = grid_m.RectGrid(np.arange(5) * 1e-3, np.arange(3) * 1e-3, np.arange(7) * 1e-3)
    e, h, kc = ports.rect_te_mode(4e-3, 2e-3, "TE10")
    assert kc == pytest.approx(np.pi / 4e-3)
    pl = ports.waveguide_lists(grid, np.zeros((3, 7, 3, 5), bool), ports.WaveguidePort(1, (0, 0, 1), (4, 2, 4), 2, e, h, kc, excite=2.0), 1e-3)
    s = {1: np.sqrt(0.5), 2: 1.0, 3: np.sqrt(0.5)}
    _close(_as_dict(grid, pl.src), {(1, i, j, 1): -2.0 * 250 * s[i] * 1e-3 for i in s for j in (0, 1)})
    _close(_as_dict(grid, pl.v_probes[0]), {(1, i, j, 4): -250 * s[i] * 1e-3 / 0.5 for i in s for j in (0, 1)})
    _close(_as_dict(grid, pl.i_probes[0]), {(0, i, j, k): 0.5 * 250 * s[i] * 1e-3 / 0.5 for i in s for j in (0, 1) for k in (3, 4)})
    assert len(pl.v_probes) == len(pl.i_probes) == 1 and not pl.lumped
    assert (pl.info["source_plane"], pl.info["probe_plane"], pl.info["sign"]) == (1, 4, 1)
    # the same box walked the other way: source and probe planes swap, the current changes sign; metal edges leave the lists
    pec = np.zeros((3, 7, 3, 5), bool)
    pec[1, 1, 0, 2] = True
    back = ports.waveguide_lists(grid, pec, ports.WaveguidePort(1, (0, 0, 4), (4, 2, 1), 2, e, h, kc, excite=0.0), 1e-3)
    assert back.src.idx.size == 0 and (back.info["source_plane"], back.info["probe_plane"], back.info["sign"]) == (4, 1, -1)
    n_e = 0.25 - 250 ** 2 * 1e-6
    _close(_as_dict(grid, back.v_probes[0]), {(1, i, j, 1): -250 * s[i] * 1e-3 / np.sqrt(n_e) for i in s for j in (0, 1) if (i, j) != (2, 0)})
    _close(_as_dict(grid, back.i_probes[0]), {(0, i, j, k): -0.5 * 250 * s[i] * 1e-3 / 0.5 for i in s for j in (0, 1) for k in (0, 1)})


@pytest.mark.parametrize("feed_R", [np.inf, 50.0, 0.0])
def test_msl_lists_of_a_strip_two_nodes_wide(feed_R):
    """Cells of 1 mm, t = x, prop = y, exc = z; box (2, 1, 0) -> (3, 7, 2): strip nodes i = 2, 3 on the plane k = 2, measurement lines
    j = 3, 4, 5, the V path on i = 2 (the line nearest the centre 2.5; a tie goes to the lower line), loops at j = 3 and 4
    (between the lines 3|4 and 4|5), feed and resistor on j = 1."""
    ports, grid_m, scene = pkg("ports"), pkg("grid"), pkg("scene")
    grid = grid_m.RectGrid(np.arange(6) * 1e-3, np.arange(9) * 1e-3, np.arange(5) * 1e-3)
    port = ports.MSLPort(1, scene.Metal("strip"), (2, 1, 0), (3, 7, 2), 1, 2, excite=1.0, feed_R=feed_R)
    assert ports.msl_strip_box(port) == ((2.0, 1.0, 2.0), (3.0, 7.0, 2.0))
    pl = ports.msl_lists(grid, np.zeros((3, 5, 9, 6), bool), port, 1e-3)
    _close(_as_dict(grid, pl.src), {(2, i, 1, k): 0.5 for i in (2, 3) for k in (0, 1)})
    for q, j in enumerate((3, 4, 5)):
        _close(_as_dict(grid, pl.v_probes[q]), {(2, 2, j, k): -1.0 for k in (0, 1)})
    for q, j in enumerate((3, 4)):      # H_x above (+) and below (-) the strip over its nodes, H_z left (+) and right (-) of its rims
        _close(_as_dict(grid, pl.i_probes[q]), {(0, 2, j, 2): 1.0, (0, 3, j, 2): 1.0, (0, 2, j, 1): -1.0, (0, 3, j, 1): -1.0,
                                                (2, 1, j, 2): 1.0, (2, 3, j, 2): -1.0})
    under = {(2, i, 1, k) for i in (2, 3) for k in (0, 1)}
    if feed_R == 50.0:       # two in series, two in parallel: each edge carries n_ser / (R n_par)
        assert {(le.comp, le.i, le.j, le.k) for le in pl.lumped} == under and all(le.G == pytest.approx(2 / (50.0 * 2)) for le in pl.lumped)
    else:
        assert not pl.lumped
    nx, ny, _ = grid.shape
    assert {(int(c), int(g) % nx, int(g) // nx % ny, int(g) // (nx * ny)) for g, c in zip(*pl.pec)} == (under if feed_R == 0 else set())
    assert pl.info["dist_AC"] == pytest.approx(2e-3) and pl.info["dist_loops"] == pytest.approx(1e-3)
    # walked the other way, strip on the lower plane: the voltage keeps its meaning (strip over the other plane), the loops change sign
    back = ports.msl_lists(grid, np.zeros((3, 5, 9, 6), bool), ports.MSLPort(1, scene.Metal("strip"), (2, 7, 3), (3, 1, 1), 1, 2, excite=1.0), 1e-3)
    assert all(np.all(q.w == 1.0) for q in back.v_probes) and [int(q.idx[0]) // 6 % 9 for q in back.v_probes] == [5, 4, 3]
    _close(_as_dict(grid, back.i_probes[0]), {(0, 2, 4, 1): -1.0, (0, 3, 4, 1): -1.0, (0, 2, 4, 0): 1.0, (0, 3, 4, 0): 1.0,
                                              (2, 1, 4, 1): -1.0, (2, 3, 4, 1): 1.0})


def test_voxelize_carries_the_lists_and_build_hands_them_over(oracle_lib):
    """VoxelScene.ports holds lumped, waveguide and MSL ports alike, in the order they were added; Simulation.build adds one source list
    and every probe of each in the one loop, and an MSL port's strip and shorted feed are metal."""
    fd, _ = pc.msl(oracle_lib, None, nr_ts=4)
    fd.AddLumpedPort(3, 50.0, [30, 50, 0], [30, 50, 4], "z", 0.0)
    fd.Run(None)
    vox, sim = fd.sim.vox, fd.sim
    assert [type(p.port).__name__ for p in vox.ports] == ["MSLPort", "MSLPort", "LumpedPort"]
    assert [(len(p.v_probes), len(p.i_probes)) for p in vox.ports] == [(3, 2), (3, 2), (1, 1)]
    assert sim._port_probe_lists == [([0, 1, 2], [3, 4]), ([5, 6, 7], [8, 9]), ([10], [11])] and sim._port_probe_ids == [(0, 3), (5, 8), (10, 11)]
    assert vox.pec[1, 4, 8:38, 16:25].all() and vox.pec[0, 4, 8:39, 16:24].all() and not vox.pec[2].any()
    assert vox.ports[2].info is None and vox.ports[2].v_idx is vox.ports[2].v_probes[0].idx
    assert [c["op"] for c in fd.calls if c["op"].startswith("AddMSL")] == ["AddMSLPort", "AddMSLPort"]
    us, is_, dt = fd._port_all_series(2)
    assert len(us) == 3 and len(is_) == 2 and all(len(u) == 4 for u in us + is_) and dt == sim.dt


# ---- 2. mode weights -------------------------------------------------------------------------------------------------------------------
def test_te10_probe_is_blind_to_the_other_modes_sources():
    """On the uniform WG mesh the TE10 V-probe applied to the source amplitudes of TE20, TE01 and TE11 gives less than 1e-12 of its
    response to TE10's: exact by symmetry (the discrete sines are orthogonal), only rounding remains — read from the float64 lists."""
    ports, grid_m = pkg("ports"), pkg("grid")
    grid = grid_m.RectGrid(np.arange(17) * 1e-3, np.arange(9) * 1e-3, np.arange(65) * 1e-3)
    pec = np.zeros((3, 65, 9, 17), bool)

    def lists(mode):
        e, h, kc = ports.rect_te_mode(pc.WG_A, pc.WG_B, mode)
        return ports.waveguide_lists(grid, pec, ports.WaveguidePort(1, (0, 0, 12), (16, 8, 12.6), 2, e, h, kc, excite=1.0), 1e-3, dtype=np.float64)
    te10 = lists("TE10")
    assert te10.info["source_plane"] == 12 and te10.info["probe_plane"] == 13 and te10.v_probes[0].w.dtype == np.float64
    plane = 17 * 9
    w = {(c, g % plane): v for g, c, v in zip(te10.v_probes[0].idx.tolist(), te10.v_probes[0].comp.tolist(), te10.v_probes[0].w.tolist())}

    def response(pl):
        return sum(w.get((c, g % plane), 0.0) * a for g, c, a in zip(pl.src.idx.tolist(), pl.src.comp.tolist(), pl.src.w.tolist()))
    own = response(te10)
    assert own == pytest.approx(np.sqrt(pc.WG_A * pc.WG_B / 2) / pc.WG_A, rel=1e-12)       # sqrt(N_e), N_e = (1 / a)^2 a b / 2 exactly on this mesh
    for mode in ("TE20", "TE01", "TE11"):
        other = lists(mode)
        assert other.src.idx.size > 0
        assert abs(response(other)) < 1e-12 * abs(own), (mode, response(other), own)


# ---- 3. signs ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["wg", "wg-back", "wg-slab", "msl", "msl-open", "msl-feedR"])
def test_incident_power_is_positive_on_the_excited_port(oracle_lib, key):
    """A wave along the port's direction gives Re(U conj I) > 0: P_inc > 0 across the band on the excited port, and the wave that
    arrives at the passive port is its REFLECTED wave (it looks into the structure)."""
    make = {"wg": pc.wg, "wg-back": lambda l: pc.wg(l, excite=(0.0, 1.0)), "wg-slab": lambda l: pc.wg(l, slab=True), "msl": pc.msl,
            "msl-open": lambda l: pc.msl(l, "open"), "msl-feedR": lambda l: pc.msl(l, "feedR")}[key]
    _, ports = pc.ran(oracle_lib, key, make)
    f = pc.wg_freqs() if key.startswith("wg") else pc.msl_freqs()
    driven = [p for p in ports if p.excite != 0]
    assert len(driven) == 1
    r = driven[0].CalcPort(None, f)
    assert np.all(r.P_inc > 0) and np.all(np.isfinite(r.P_inc))
    for name in ("uf_tot", "if_tot", "uf_inc", "uf_ref", "if_inc", "if_ref", "P_inc", "P_ref", "P_acc", "beta", "ZL", "Z_ref", "u_data", "i_data"):
        assert hasattr(r, name), name
    assert r.uf_tot == pytest.approx(r.uf_inc + r.uf_ref) and r.if_tot == pytest.approx(r.if_inc - r.if_ref)
    for p in ports:
        if p.excite == 0 and key != "wg-slab":
            q = p.CalcPort(None, f)
            assert np.all(q.P_ref > 100 * q.P_inc) and np.all(q.P_acc < 0)


# ---- 4-6. the guide against closed forms ---------------------------------------------------------------------------------------------
def test_waveguide_against_the_yee_dispersion_relation_and_the_slab_line(oracle_lib):
    """Phase of the transmitted wave (port 2's uf_ref over port 1's uf_inc: the wave travels 16 mm from plane to plane) against
    -beta_d 16 mm, beta_d from the Yee dispersion relation; |S11|, |S21| and S21 - S12 of the empty guide; S11 and S21 of the slab
    against the three-section line.  Every bound: twice profiles/ports/kat.txt."""
    got = pc.wg_measures(oracle_lib)
    print({k: (got[k], KAT[k]) for k in got})
    for k in ("wg_phase_rad", "wg_s11", "wg_s21", "wg_reciprocity", "slab_s11", "slab_s21"):
        assert got[k] <= 2 * KAT[k], (k, got[k], KAT[k])
    fd, (p1, _) = pc.ran(oracle_lib, "wg", pc.wg)
    f = pc.wg_freqs()
    r = p1.CalcPort(None, f)
    k = 2 * np.pi * f / pc.C0
    assert r.beta == pytest.approx(np.sqrt(k * k - (np.pi / pc.WG_A) ** 2)) and r.ZL == pytest.approx(2 * np.pi * f * 4e-7 * np.pi / r.beta, rel=1e-6)
    below = p1.CalcPort(None, [5e9])
    assert below.beta[0].real == 0 and below.beta[0].imag < 0                 # evanescent below the 9.37 GHz cut-off: beta = -j alpha
    assert p1.CalcPort(None, f, ref_impedance=100.0).Z_ref == 100.0
    # the discrete beta is itself within 2 % of the analytic one over the band (the mesh resolves the guide): the two references agree
    assert np.abs(pc.yee_beta_te10(f, fd.sim.dt) / r.beta.real - 1).max() < 0.02


# ---- 7-10. the line ---------------------------------------------------------------------------------------------------------------------
def test_msl_line_constants_and_power_balance(oracle_lib):
    """1 < (Re beta / k0)^2 < eps_r (the field is partly in air, partly in the substrate), Re ZL > 0, |S11|^2 + |S21|^2 <= 1 + margin."""
    f = pc.msl_freqs()
    _, (p1, p2) = pc.ran(oracle_lib, "msl", pc.msl)
    s11, s21 = pc.s_params(p1, p2, f)
    eps_eff = (p1.beta.real / (2 * np.pi * f / pc.C0)) ** 2
    print("eps_eff", eps_eff, "ZL", p1.ZL, "Hammerstad-Jensen", pc.hammerstad_jensen(pc.MSL_W / pc.MSL_H, pc.MSL_EPS))
    assert np.all(eps_eff > 1) and np.all(eps_eff < pc.MSL_EPS)
    assert np.all(p1.ZL.real > 0)
    assert np.all(np.abs(s11) ** 2 + np.abs(s21) ** 2 <= 1 + 2 * KAT["msl_margin"])


def test_msl_open_end_feed_resistor_and_reference_plane_shift(oracle_lib):
    got = pc.msl_measures(oracle_lib)
    print({k: (got[k], KAT[k]) for k in got})
    for k in ("open_s11", "feedR_s11", "shift_s11", "open_phase_rad"):
        assert got[k] <= 2 * KAT[k], (k, got[k], KAT[k])
    # the shift is along the port's direction, in drawing units: by s and back is the identity, the totals follow the shifted waves
    _, (o1,) = pc.ran(oracle_lib, "msl-open", lambda l: pc.msl(l, "open"))
    f = pc.msl_freqs()
    a = o1.CalcPort(None, f)
    inc, ref, beta = a.uf_inc.copy(), a.uf_ref.copy(), a.beta.copy()
    b = o1.CalcPort(None, f, ref_plane_shift=7.0)
    assert b.uf_inc == pytest.approx(inc * np.exp(-1j * beta.real * 7.0 * 0.2e-3)) and b.uf_ref == pytest.approx(ref * np.exp(1j * beta.real * 7.0 * 0.2e-3))
    assert b.uf_tot == pytest.approx(b.uf_inc + b.uf_ref) and b.if_tot == pytest.approx(b.if_inc - b.if_ref)


def test_run_summary_names_the_ports(oracle_lib, tmp_path):
    import json
    fd, _ = pc.wg(oracle_lib, nr_ts=4)
    fd.Run(str(tmp_path))
    got = json.load(open(tmp_path / "fdtd_hip_run.json"))["ports"]
    assert [(p["number"], p["kind"], p["direction"], p["sign"], p["source_plane"], p["probe_plane"], p["source_edges"], p["v_probe_edges"],
             p["i_probe_faces"]) for p in got] == [(1, "rect_waveguide", "z", 1, 12, 24, 120, [120], [240]), (2, "rect_waveguide", "z", -1, 52, 40, 0, [120], [240])]


def test_compat_module_exports_the_port_classes():
    import importlib
    import sys
    sys.path.insert(0, os.path.join(ROOT, "fdtd-solver-antennas_amd", "compat"))
    try:
        m = importlib.import_module("openEMS.ports")
    finally:
        sys.path.pop(0)
    api = pkg("openems_api")
    assert (m.LumpedPort, m.MSLPort, m.WaveguidePort, m.RectWGPort) == (api.LumpedPort, api.MSLPort, api.WaveguidePort, api.RectWGPort)
    assert issubclass(m.RectWGPort, m.WaveguidePort)


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------------------
def _guide(extra=None, box=((0, 0, 12), (16, 8, 24)), boundary=PEC_PML, port=None):
    """The WG mesh through the Scene interface, one port, up to the Simulation (no engine)."""
    scene, grid_m, sim = pkg("scene"), pkg("grid"), pkg("simulation")
    grid = grid_m.RectGrid(np.arange(17) * 1e-3, np.arange(9) * 1e-3, np.arange(65) * 1e-3)
    sc = scene.Scene(unit=1e-3)
    if extra:
        extra(sc)
    (port or (lambda s: s.add_rect_waveguide_port(1, box[0], box[1], "z", pc.WG_A, pc.WG_B, "TE10", 1.0)))(sc)
    return sim.Simulation(grid, scene.voxelize(sc, grid), f0=pc.WG_F0, fc=pc.WG_FC, boundary=boundary, nr_ts=600)


def test_a_guide_that_fits_is_accepted():
    s = _guide()
    assert s.vox.ports[0].info["source_edges"] == 120
    # walls drawn as metal, one cell inside the mesh, a box one cell wider than the guide: still from wall to wall
    def walls(sc):
        m = sc.add_metal("walls")
        for a, b in (((1, 0, 0), (1, 8, 64)), ((15, 0, 0), (15, 8, 64))):
            m.add_box(a, b)
    assert _guide(walls, boundary=["MUR", "MUR", "PEC", "PEC", "PML_8", "PML_8"]).vox.ports[0].info["source_edges"] > 0


def test_tm_modes_are_refused():
    with pytest.raises(ValueError, match="TM modes are not supported"):
        _guide(port=lambda s: s.add_rect_waveguide_port(1, (0, 0, 12), (16, 8, 24), "z", pc.WG_A, pc.WG_B, "TM11", 1.0))
    api = pkg("openems_api")
    fd, _ = pc.wg(None)
    with pytest.raises(ValueError, match="TM modes are not supported"):
        fd.AddRectWaveGuidePort(3, [0, 0, 12], [16, 8, 24], "z", pc.WG_A, pc.WG_B, "TM11", 1)
    assert api.RectWGPort is not None


def test_te00_is_refused():
    with pytest.raises(ValueError, match=r"TE00 does not exist \(m = n = 0\)"):
        _guide(port=lambda s: s.add_rect_waveguide_port(1, (0, 0, 12), (16, 8, 24), "z", pc.WG_A, pc.WG_B, "TE00", 1.0))


def test_a_port_without_direction_is_refused():
    with pytest.raises(ValueError, match=r"waveguide port 1: start and stop coincide along z: the port has no direction \(d = 0\)"):
        _guide(box=((0, 0, 12), (16, 8, 12)))
    fd, _ = pc.wg(None)
    with pytest.raises(ValueError, match=r"d = 0"):
        fd.AddRectWaveGuidePort(3, [0, 0, 12], [16, 8, 12], "z", pc.WG_A, pc.WG_B, "TE10", 1)


def test_string_weight_functions_are_refused():
    fd, _ = pc.wg(None)
    with pytest.raises(ValueError, match="weight functions given as strings are not supported: pass Python callables"):
        fd.AddWaveGuidePort(3, [0, 0, 12], [16, 8, 24], "z", ["0", "-sin(x)"], ["sin(x)", "0"], 196.0, 1)
    with pytest.raises(ValueError, match="given as strings are not supported"):
        fd.AddWaveGuidePort(3, [0, 0, 12], [16, 8, 24], "z", "sin(x)", "sin(x)", 196.0, 1)


def test_field_excitations_stay_refused():
    """The ports do not open CSX.AddExcitation: its field types and SetWeightFunction are refused as before."""
    api = pkg("openems_api")
    csx = api.ContinuousStructure()
    with pytest.raises(ValueError):
        csx.AddExcitation("e", 0, [0, 1, 0])
    assert not hasattr(api.openEMS, "AddCoaxialPort") and not hasattr(api.openEMS, "AddCircWaveGuidePort")


def test_a_box_that_does_not_span_the_guide_is_refused():
    with pytest.raises(ValueError, match=r"waveguide port 1: the rim edge y-directed at node \(3, 0, 12\) of its box \(nodes \(3, 0, 12\)\.\.\(13, 8, 24\)\) is "
                                         r"neither metal \(PEC\) nor on a PEC / PMC grid face.*from wall to wall along x"):
        _guide(box=((3, 0, 12), (13, 8, 24)))
    # an absorbing face is no wall
    with pytest.raises(ValueError, match=r"the rim edge x-directed at node \(0, 0, 12\).*wall to wall along y"):
        _guide(boundary=["PEC", "PEC", "MUR", "MUR", "PML_8", "PML_8"])


def test_a_measurement_plane_on_a_grid_face_is_refused():
    with pytest.raises(ValueError, match=r"measurement plane \(node 64 along z\) lies on a grid face"):
        _guide(box=((0, 0, 40), (16, 8, 64)))


OWNERS = {
    "Debye": (lambda sc: sc.add_debye_material("water", 4.0, 0.0, [2.0], [1e-11]).add_box((0, 0, 10), (16, 8, 14)),
              r"waveguide port 1: its source edge y-directed at node \(1, 0, 12\) is an edge of the Debye medium 'water'"),
    "Lorentz": (lambda sc: sc.add_lorentz_material("gold", 1.0, 0.0, wp=[2e11], w0=[0.0], gamma=[1e10]).add_box((0, 0, 22), (16, 8, 26)),
                r"waveguide port 1: its voltage-probe edge y-directed at node \(1, 0, 24\) is an edge of the Lorentz medium 'gold'"),
    "sheet": (lambda sc: sc.add_conducting_sheet("foil", 5.8e7, 35e-6).add_box((4, 2, 12), (8, 6, 12)),
              r"(waveguide port 1.*conducting-sheet edge of 'foil'|conducting sheet 'foil'.*waveguide port 1)"),
    "element": (lambda sc: sc.add_lumped_element("R1", "y", R=50.0, caps=False).add_box((8, 2, 24), (8, 4, 24)),
                r"(waveguide port 1.*lumped-element edge of 'R1'|lumped element 'R1'.*waveguide port 1)"),
    "plane wave": (lambda sc: sc.add_plane_wave("pw", (0.0, 1.0, 0.0), (0, 0, 1)).add_box((5, 3, 24), (11, 5, 30)),
                   r"(waveguide port 1.*plane-wave box 'pw'|plane wave 'pw'.*)"),
}


@pytest.mark.parametrize("owner", sorted(OWNERS))
def test_a_port_plane_on_a_correction_list_is_refused(owner):
    extra, text = OWNERS[owner]
    with pytest.raises(ValueError, match=text):
        _guide(extra)


def test_a_port_plane_on_a_conformal_cut_face_is_refused():
    """The cut faces and cut edges of a conformal run, handed to check_placement as Simulation does."""
    ports = pkg("ports")
    s = _guide()
    p = s.vox.ports[0]
    lists = dict(src=ports.Probe(p.src_idx, p.src_comp, p.src_amp), v_probes=p.v_probes, i_probes=p.i_probes)
    none = types.SimpleNamespace(idx=np.zeros(0, np.int64), comp=np.zeros(0, np.int8))
    face = types.SimpleNamespace(idx=p.i_probes[0].idx[5:6], comp=p.i_probes[0].comp[5:6], frac=none)
    with pytest.raises(ValueError, match=r"waveguide port 1: its current-probe face x-directed at node \(\d+, \d+, 23\) is a conformal \(cut\) face"):
        ports.check_placement(s.grid, p.port, p.info, pec=s.vox.pec, kinds=s.bc.kinds, conformal=face, **lists)
    edge = types.SimpleNamespace(idx=none.idx, comp=none.comp, frac=types.SimpleNamespace(idx=p.src_idx[7:8], comp=p.src_comp[7:8]))
    with pytest.raises(ValueError, match=r"waveguide port 1: its source edge y-directed at node \(\d+, \d+, 12\) is cut by a conformal metal surface"):
        ports.check_placement(s.grid, p.port, p.info, pec=s.vox.pec, kinds=s.bc.kinds, conformal=edge, **lists)


def test_msl_refusals():
    scene, grid_m, ports = pkg("scene"), pkg("grid"), pkg("ports")
    grid = grid_m.RectGrid(np.arange(41) * 0.2e-3, np.arange(101) * 0.2e-3, np.arange(25) * 0.2e-3)

    def port(start, stop, **kw):
        sc = scene.Scene(unit=0.2e-3)
        sc.add_msl_port(1, sc.add_metal("strip"), start, stop, "y", "z", 1.0, **kw)
        return scene.voxelize(sc, grid)
    for a, stop in enumerate(((16, 38, 4), (24, 8, 4), (24, 38, 0))):
        with pytest.raises(ValueError, match=f"MSL port 1: its box has zero extent along {'xyz'[a]}"):
            port((16, 8, 0), stop)
    with pytest.raises(ValueError, match=r"MSL port 1: the measurement lines 37, 38, 39 along y do not all lie inside its box \(nodes 8\.\.38\)"):
        port((16, 8, 0), (24, 38, 4), meas_plane_shift=30)
    with pytest.raises(ValueError, match=r"MSL port 1: the propagation and the excitation direction are both y"):
        sc = scene.Scene(unit=0.2e-3)
        sc.add_msl_port(1, sc.add_metal("strip"), (16, 8, 0), (24, 38, 4), "y", "y", 1.0)
    with pytest.raises(ValueError, match=r"MSL port 1: Feed_R = -5.0 must be >= 0"):
        port((16, 8, 0), (24, 38, 4), feed_R=-5.0)
    assert port((16, 8, 0), (24, 38, 4), meas_plane_shift=29).ports[0].info["probe_planes"] == [36, 37, 38]
    assert ports.label(port((16, 8, 0), (24, 38, 4)).ports[0].port) == "MSL port 1"
    fd, _ = pc.msl(None)
    with pytest.raises(ValueError, match="MSL port 3: metal_prop must be a metal of the structure"):
        fd.AddMSLPort(3, fd.GetCSX().AddMaterial("fr4", epsilon=4.4), [16, 8, 0], [24, 38, 4], "y", "z", 1)


@pytest.mark.parametrize("cut", sorted(pc.WG_CUTS))
def test_the_guide_on_oracle_slabs_is_the_guide_on_one_slab(oracle_lib, cut):
    """WG cut at plane 24 (port 1's source and V-plane the bottom plane of the upper slab, its I half-planes on both sides of the cut) and
    at planes 24 and 40, the oracle half-stepped with the halos carried by the host: the single slab's fields (every value, and the bits
    of every non-zero one: the sign of a zero on a dead edge depends on what lies below plane 0, tests/test_sources_probes_cpu.py); every
    rank's series the sums of the cells it owns; the ranks' series added up and handed to the ports' post-processing give the single
    slab's S11 and S21 over the band to 1e-12 relative."""
    import source_probe_cases as spc
    from helpers import rel_l2
    cuts = pc.WG_CUTS[cut]
    _, case = pc.raw("WG")
    ref = pc.raw_reference("WG", oracle_lib)
    engs, ids = pc.slab_engines("WG", oracle_lib, cuts)
    spc.slab_stepper(engs, "half-steps")(pc.RAW_STEPS)
    got, want = np.concatenate([e.fields() for e in engs], axis=2), ref["fields"]
    assert np.array_equal(got, want) and np.array_equal(got[want != 0].view(np.uint32), want[want != 0].view(np.uint32))
    trees = ref["slab_trees"][cut]
    owners = []
    for q, pid in enumerate(ids):
        parts = [e.get_probe(pid) for e in engs]
        for r, part in enumerate(parts):
            assert len(part) == pc.RAW_STEPS and part.any() == trees[r][q].any() and rel_l2(part, trees[r][q]) < 1e-12, (cut, r, q)
        owners.append([bool(p.any()) for p in parts])
        assert rel_l2(sum(parts), ref["own"][q]) < 1e-12, (cut, q)
    # port 1: V (120 cells, plane 24) the upper slab's alone, I (240 faces, planes 23 and 24) on both sides of the cut
    assert [p[1].size for p in case.probes[:2]] == [120, 240] and owners[0][:2] == [False, True] and owners[1][:2] == [True, True], owners
    f = pc.wg_freqs()
    summed = pc.s_from_series("WG", [sum(e.get_probe(pid) for e in engs) for pid in ids], f)
    single = pc.s_from_series("WG", ref["own"], f)
    for a, b in zip(summed, single):
        assert np.abs(b).min() > 0 and np.all(np.abs(a - b) <= 1e-12 * np.abs(b)), (cut, np.abs((a - b) / b).max())
