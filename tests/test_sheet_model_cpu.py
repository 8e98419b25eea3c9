"""Conducting sheets (sheet.py, scene.add_conducting_sheet): surface-impedance model, rational fit, voxeliser geometry, the
plugin's call sequence, and the per-timestep correction restated in numpy on top of the oracle's half-steps."""
import numpy as np
import pytest

from conftest import pkg
from restatement import Restatement
from test_plugin_surface_cpu import _load, _params, _same

MU0 = 4e-7 * np.pi


def _sheet():
    return pkg("sheet")


# ---- model --------------------------------------------------------------------------------------------------
def test_surface_impedance_limits():
    sh = _sheet()
    sigma, t = 5.8e7, 35e-6
    assert abs(sh.Z_s([0.0], sigma, t)[0] - 1 / (sigma * t)) < 1e-15
    assert abs(sh.Z_s([1.0], sigma, t)[0].real * sigma * t - 1) < 1e-6           # quasi-DC: delta >> t
    f = 2.45e9
    delta = np.sqrt(2 / (2 * np.pi * f * MU0 * sigma))
    Rs = np.sqrt(2 * np.pi * f * MU0 / (2 * sigma))
    z = sh.Z_s([f], sigma, 30 * delta)[0]
    assert abs(z - (1 + 1j) * Rs) < 1e-9 * Rs
    # t ~ delta: coth(gamma t) differs from 1 noticeably, and both limits are wrong there
    for s_, t_ in ((4.1e7, 2e-6), (9.1e6, 5e-6)):
        d = np.sqrt(2 / (2 * np.pi * f * MU0 * s_))
        assert 0.5 < t_ / d < 2
        z = sh.Z_s([f], s_, t_)[0]
        thick = (1 + 1j) * np.sqrt(2 * np.pi * f * MU0 / (2 * s_))
        g = (1 + 1j) / d
        assert abs(z - g / s_ / np.tanh(g * t_)) < 1e-9 * abs(z)
        assert abs(z - thick) > 0.02 * abs(thick) and abs(z - 1 / (s_ * t_)) > 0.02 * abs(z)
    assert np.all(np.isfinite(sh.Z_s(np.geomspace(1, 1e12, 50), 1e12, 1e-3)))


@pytest.mark.parametrize("band", [(1.225e9, 3.675e9), (2.9e9, 8.7e9), (5e9, 15e9)])
def test_fit_accuracy_passivity_and_discretisation(band):
    sh, P = _sheet(), pkg("params")
    for m in P.metal_defaults.values():
        ft = sh.fit(m.conductivity_s_per_m, m.thickness_m, *band)
        f = np.linspace(*band, 301)
        err = np.max(np.abs(ft.Y(f) - sh.Y_s(f, m.conductivity_s_per_m, m.thickness_m)) / np.abs(sh.Y_s(f, m.conductivity_s_per_m, m.thickness_m)))
        assert err <= 0.01 and ft.band_error <= 0.01, (m.name, band, err)
        dense = np.concatenate([[0.0], np.geomspace(1.0, 100 * band[1], 4000)])
        assert np.all(ft.Y(dense).real >= 0)
        assert ft.G0 >= 0 and np.all(ft.c >= 0) and ft.poles.size <= 8
        alpha, b = ft.discretise(1e-12)
        assert np.all((alpha > 0) & (alpha < 1)) and np.all(b >= 0)


# ---- voxeliser ----------------------------------------------------------------------------------------------
def _grid(n=(12, 12, 10), h=1e-3):
    return pkg("grid").RectGrid(*[np.arange(k) * h for k in n])


def test_infinite_sheet_and_rim():
    sc, g = pkg("scene"), _grid()
    s = sc.Scene(unit=1e-3)
    s.add_conducting_sheet("s", 5.8e7, 35e-6).add_box([-5, -5, 4], [50, 50, 4])    # through the whole grid at z = 4
    v = sc.voxelize(s, g)
    sh = v.sheets
    nx, ny, _ = g.shape
    k, r = np.divmod(sh.idx, nx * ny)
    j, i = np.divmod(r, nx)
    assert np.all(k == 4) and set(sh.comp.tolist()) == {0, 1}
    assert not v.pec[:2, 4, 1:-1, 1:-1].any() and not v.pec[2].any()       # the sheet's edges are no longer PEC (outer rows stay PEC)
    # all interior in-plane edges, w = dual width (1 mm) over l = 1 mm
    assert len(sh) == 2 * (nx - 1) * (ny - 2)
    assert np.allclose(sh.scale, 1.0)
    # a finite sheet: its rim edges carry half the dual width
    s2 = sc.Scene(unit=1e-3)
    s2.add_conducting_sheet("s", 5.8e7, 35e-6).add_box([3, 3, 4], [8, 8, 4])
    sh2 = sc.voxelize(s2, g).sheets
    k, r = np.divmod(sh2.idx, nx * ny)
    j, i = np.divmod(r, nx)
    x_edges = sh2.comp == 0
    rim = x_edges & ((j == 3) | (j == 8))
    inner = x_edges & (j > 3) & (j < 8)
    assert rim.sum() == 10 and inner.sum() == 20
    assert np.allclose(sh2.scale[rim], 0.5) and np.allclose(sh2.scale[inner], 1.0)
    # no edge of the sheet stays PEC (all are surface edges), nothing outside it is metal
    assert not sc.voxelize(s2, g).pec.any()


def test_resolved_layer_gives_surface_edges_only():
    sc, g = pkg("scene"), _grid()
    s = sc.Scene(unit=1e-3)
    s.add_conducting_sheet("cu", 5.8e7, 2e-3).add_box([3, 3, 3], [8, 8, 5])          # two cells thick
    v = sc.voxelize(s, g)
    nx, ny, _ = g.shape
    k, r = np.divmod(v.sheets.idx, nx * ny)
    j, i = np.divmod(r, nx)
    # the middle plane's interior edges stay PEC; the top / bottom faces and the sides are sheet edges
    assert v.pec[0, 4, 4:8, 3:8].all() and v.pec[2, 3, 4:8, 4:8].all()
    mid = (k == 4) & (v.sheets.comp != 2) & (i > 3) & (i < 8) & (j > 3) & (j < 8)
    assert not mid.any()
    assert ((k == 3) & (v.sheets.comp == 0)).sum() == 5 * 6 and ((k == 5) & (v.sheets.comp == 0)).sum() == 5 * 6
    side_z = (v.sheets.comp == 2) & (i == 3) & (j > 3) & (j < 8)
    assert side_z.sum() == 2 * 4 and np.allclose(v.sheets.scale[side_z], 1.0)
    # a corner edge of the box: two faces, half a dual width each
    corner = (v.sheets.comp == 2) & (i == 3) & (j == 3)
    assert corner.sum() == 2 and np.allclose(v.sheets.scale[corner], 1.0)


def test_priority_between_metals():
    sc, g = pkg("scene"), _grid()
    s = sc.Scene(unit=1e-3)
    s.add_conducting_sheet("s", 5.8e7, 35e-6).add_box([2, 2, 4], [9, 9, 4], priority=1)
    s.add_metal("pec").add_box([2, 2, 4], [5, 9, 4], priority=5)
    v = sc.voxelize(s, g)
    nx, ny, _ = g.shape
    r = v.sheets.idx % (nx * ny)
    assert np.all(r % nx >= 5)                       # the PEC box owns x < 5
    assert v.pec[0, 4, 3, 2:5].all()


def test_forbidden_overlaps_refused():
    sc, g, sim = pkg("scene"), _grid(), pkg("simulation")
    # a port three edges wide in x (z-directed, centre line x = 5): the plane y = 5 holds its voltage line, the plane x = 4 a port
    # edge beside that line
    for box, what in ((([2, 5, 2], [9, 5, 8]), "voltage-probe line"), (([4, 2, 2], [4, 9, 8]), "port edge")):
        s = sc.Scene(unit=1e-3)
        s.add_conducting_sheet("s", 5.8e7, 35e-6).add_box(*box)
        s.add_lumped_port(1, 50, [4, 5, 4], [6, 5, 5], "z")
        with pytest.raises(ValueError, match=what):
            sc.voxelize(s, g)
    s = sc.Scene(unit=1e-3)
    s.add_conducting_sheet("s", 5.8e7, 35e-6).add_box([3, 3, 1], [8, 8, 1])
    v = sc.voxelize(s, g)
    with pytest.raises(ValueError, match="Mur"):
        sim.Simulation(g, v, f0=2e9, fc=1e9, boundary="MUR", nr_ts=10)
    s = sc.Scene(unit=1e-3)
    s.add_conducting_sheet("s", 5.8e7, 35e-6).add_box([0, 0, 3], [11, 11, 3])
    v = sc.voxelize(s, g)
    with pytest.raises(ValueError, match="NF2FF"):
        sim.Simulation(g, v, f0=2e9, fc=1e9, boundary="PEC", nr_ts=10, nf2ff_freqs=[2e9])


def test_junction_of_two_sheets_of_one_metal_is_no_rim():
    """A patch and its feed line drawn as two sheets of the same metal, edge to edge: the junction line is inside one conductor (full
    dual width).  Two different metals meeting there: each sees its own rim (half)."""
    sc, g = pkg("scene"), _grid()
    nx, ny, _ = g.shape
    for feed_sigma, want in ((5.8e7, 1.0), (9.1e6, 0.5)):
        s = sc.Scene(unit=1e-3)
        s.add_conducting_sheet("patch", 5.8e7, 35e-6).add_box([2, 2, 4], [6, 9, 4])
        s.add_conducting_sheet("feed", feed_sigma, 35e-6).add_box([6, 4, 4], [10, 7, 4])
        sh = sc.voxelize(s, g).sheets
        r = sh.idx % (nx * ny)
        i, j = r % nx, r // nx
        junction = (sh.comp == 1) & (i == 6) & (j >= 4) & (j < 7)
        assert junction.sum() == 3 and np.allclose(sh.scale[junction], want), (feed_sigma, sh.scale[junction])


def test_sheet_vi_is_the_operators(oracle_lib):
    """Simulation.sheet_vi evaluates the sheet edges' vi on the host; it must be what the engine's operator holds, in either form."""
    for classes in (True, False):
        s = cavity_sim(3e5, 1e-3, nr_ts=10)
        s.use_classes = classes
        saved, s.sheets = s.sheets, None
        e = s.build(oracle_lib)
        s.sheets = saved
        vi = e.get_operator()[1].reshape(3, -1)[s.sheets.comp.astype(np.int64), s.sheets.idx]
        assert np.array_equal(s.sheet_vi(), vi) and np.all(vi > 0)


# ---- plugin call sequence ------------------------------------------------------------------------------------
def test_metal_loss_call_sequence():
    s = pkg("solver_fdtd_hip")
    p = _params()
    prep = s.prepare_hip_patch_fixed(p, metal_loss=True)
    assert prep.ok, prep.message
    sheets = [c for c in prep.FDTD.calls if c["op"] == "AddConductingSheet"]
    assert [c["name"] for c in sheets] == ["patch", "gnd"]
    for c in sheets:
        assert c["conductivity"] == p.metal.conductivity_s_per_m and c["thickness"] == p.metal.thickness_m
    assert not any(c["op"] == "AddMetal" for c in prep.FDTD.calls)
    gold = _load("scene_calls.json")["fixed_2g45"]
    _same(s.prepare_hip_patch_fixed(p, metal_loss=False).FDTD.calls, gold["calls"], "fixed_2g45")
    for fn in (s.prepare_hip_microstrip_patch, s.prepare_hip_microstrip_patch_3d):
        calls = fn(p, metal_loss=True).FDTD.calls
        assert any(c["op"] == "AddConductingSheet" for c in calls) and not any(c["op"] == "AddMetal" for c in calls)
    # the legacy variant's ground plane crosses its NF2FF box: refused when prepared, with the reason
    prep = s.prepare_hip_patch(p, metal_loss=True)
    assert not prep.ok and "NF2FF" in prep.message
    assert s.prepare_hip_patch(p).ok
    inst = s.PatchInstance(name="A", params=p, center_x_m=0.0, center_y_m=0.0, center_z_m=0.0, feed_direction=s.FeedDirection.NEG_X)
    calls = s.prepare_hip_microstrip_multi_3d([inst], mesh_quality=2, metal_loss=True).FDTD.calls
    assert sorted(c["name"] for c in calls if c["op"] == "AddConductingSheet") == ["feed_1", "ground_1", "patch_1"]


def test_conducting_sheet_scene_through_openems_api():
    oa = pkg("openems_api")
    csx = oa.ContinuousStructure()
    csx.GetGrid().SetDeltaUnit(1e-3)
    for a, l in zip("xyz", ([0, 11], [0, 11], [0, 9])):
        csx.GetGrid().AddLine(a, np.arange(l[0], l[1] + 1, 1.0))
    csx.AddConductingSheet("s", conductivity=9.1e6, thickness=5e-6).AddBox([3, 3, 4], [8, 8, 4]).AddTransform("Translate", [1, 0, 0])
    f = oa.openEMS(NrTS=10)
    f.SetGaussExcite(2e9, 1e9)
    f.SetCSX(csx)
    assert f.calls[-2] == {"op": "AddConductingSheet", "name": "s", "conductivity": 9.1e6, "thickness": 5e-6}
    assert f.calls[-1] == {"op": "AddBox", "prop": "s", "priority": 0, "start": [3, 3, 4], "stop": [8, 8, 4],
                           "transforms": [["Translate", [1, 0, 0]]]}
    grid, scene = f._build_scene()
    v = pkg("scene").voxelize(scene, grid)
    assert len(v.sheets) == 60 and v.sheets.metals[0].conductivity == 9.1e6
    nx, ny, _ = grid.shape
    assert (v.sheets.idx % nx).min() == 4           # translated by +1 mm


# ---- restatement on the oracle --------------------------------------------------------------------------------
def cavity_sim(sigma, t, *, n=(14, 13, 12), boundary="PEC", nr_ts=2000, sheet=True, f0=6e9, fc=4e9):
    """A box walled by six zero-thickness sheets (one cell inside the grid faces), a soft source inside."""
    sc, sim = pkg("scene"), pkg("simulation")
    g = _grid(n)
    s = sc.Scene(unit=1e-3)
    nx, ny, nz = n
    lo, hi = (2, 2, 2), (nx - 3, ny - 3, nz - 3)
    mk = (lambda nm: s.add_conducting_sheet(nm, sigma, t)) if sheet else s.add_metal
    for a in range(3):
        for side in (lo[a], hi[a]):
            st, sp = list(lo), list(hi)
            st[a] = sp[a] = side
            mk(f"w{a}{side}").add_box(st, sp)
    s.add_lumped_port(1, 0.0, [5, 5, 4], [5, 5, 5], "z", 1.0)
    v = sc.voxelize(s, g)
    return sim.Simulation(g, v, f0=f0, fc=fc, boundary=boundary, nr_ts=nr_ts, end_criteria=0.0)


def test_high_conductivity_matches_pec(oracle_lib):
    nsteps = 600
    pec = cavity_sim(1.0, 1.0, sheet=False, nr_ts=nsteps)
    e = pec.build(oracle_lib)
    e.run(nsteps)
    ref = e.fields()
    s = cavity_sim(1e12, 1e-3, nr_ts=nsteps)
    assert len(s.sheets) > 0
    r = Restatement(s, oracle_lib)
    r.run(nsteps)
    got = r.e.fields()
    assert np.abs(ref).max() > 0
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()


def test_lossy_cavity_energy_decays(oracle_lib):
    """sigma = 1e5 S/m walls, 20 000 timesteps: once the source has ended the stored energy never grows (maxima over 200-step
    windows: the leapfrog energy of a single instant oscillates within a period) and it falls by decades."""
    s = cavity_sim(1e5, 1e-3, nr_ts=20000, f0=20e9, fc=10e9)
    tail = len(s.signal)
    r, en = Restatement(s, oracle_lib), []
    for n in range(20000):
        r.step()
        if (n + 1) % 10 == 0:
            sv, si = r.e.energy()
            en.append(8.854187817e-12 * sv + MU0 * si)
    ib, en = r.sheets.ib, np.array(en)
    after = en[(tail + 9) // 10:]
    assert after[0] > 0 and np.all(np.isfinite(after))
    w = after[:after.size // 20 * 20].reshape(-1, 20).max(axis=1)
    assert np.all(np.diff(w) <= 0), "energy grew after the source ended"
    assert w[-1] < 1e-3 * w[0] and np.abs(ib).max() > 0


# ---- efficiency and gain of the plugin result ------------------------------------------------------------------
def _two_dipoles(lib, tmp, excite2):
    """Two short dipoles in free space, each fed by a 50-ohm lumped port; the second port excited or not."""
    oa, s = pkg("openems_api"), pkg("solver_fdtd_hip")
    fdtd = oa.openEMS(NrTS=6000, EndCriteria=1e-5, lib=lib)
    fdtd.SetGaussExcite(3e9, 1.5e9)
    fdtd.SetBoundaryCond(["MUR"] * 6)
    csx = oa.ContinuousStructure()
    fdtd.SetCSX(csx)
    mesh = csx.GetGrid()
    mesh.SetDeltaUnit(1e-3)
    for a in "xyz":
        mesh.AddLine(a, np.arange(-48.0, 48.1, 4.0))
    ports = []
    for n, (x, ex) in enumerate(((-12.0, 1.0), (12.0, excite2))):
        w = csx.AddMetal(f"wire{n}")
        w.AddBox([x, 0, 4], [x, 0, 16])
        w.AddBox([x, 0, -16], [x, 0, -4])
        ports.append(fdtd.AddLumpedPort(n + 1, 50, [x, 0, -4], [x, 0, 4], "z", ex))
    nf = fdtd.CreateNF2FFBox()
    prep = s.FDTDPrepared(True, "two dipoles", FDTD=fdtd, nf=nf, sim_path=str(tmp), theta=np.arange(0.0, 181.0, 10.0),
                          phi=np.array([0.0, 90.0]), nf_center=np.zeros(3), port=ports[0], ports=ports, variant="fixed")
    res = s.run_prepared_hip(prep, frequency_hz=3e9, verbose=0)
    assert res.ok, res.message
    return prep, res


@pytest.mark.parametrize("excite2", [1.0, 0.0])
def test_efficiency_and_gain_sum_every_excited_port(oracle_lib, tmp_path, excite2):
    """radiation_efficiency = Prad / (P_acc summed over the EXCITED ports), recomputed here from the ports and the NF2FF result at
    f_pattern; realised gain = Dmax Prad / sum P_inc.  Two driven dipoles must not read twice the efficiency of one."""
    prep, res = _two_dipoles(oracle_lib, tmp_path, excite2)
    f = res.f_pattern
    nfr = prep.nf.CalcNF2FF(prep.sim_path, [f], np.arange(0.0, 181.0, 10.0), np.array([0.0, 90.0]), center=[0, 0, 0])
    prad = float(np.asarray(nfr.Prad)[0])
    driven = prep.ports if excite2 else prep.ports[:1]
    acc = sum(float(p.CalcPort(prep.sim_path, np.array([f])).P_acc[0]) for p in driven)
    inc = sum(float(p.CalcPort(prep.sim_path, np.array([f])).P_inc[0]) for p in driven)
    assert acc > 0 and prad > 0
    assert abs(res.radiation_efficiency - prad / acc) <= 1e-9 * (prad / acc)
    assert abs(res.gain_dBi - 10 * np.log10(res.Dmax * prad / acc)) < 1e-9
    assert abs(res.realized_gain_dBi - 10 * np.log10(res.Dmax * prad / inc)) < 1e-9
    # loss-free wires in free space: what the driven ports accept leaves through the box (the passive port's load takes a little)
    assert 0.5 < res.radiation_efficiency <= 1.05, res.radiation_efficiency
