"""Stand-alone probes (CSX.AddProbe, probes.py) on the CPU oracle: the voltage and current probes on a lumped port's own boxes against
that port's series, the field probes against fdtd_get_field, the mode-matching probes against the rectangular waveguide port's, the
probe files of Run, and the limit of 64 device probes."""
import json
import os

import numpy as np
import pytest

from conftest import pkg
import ports_cases as pc


def _scene(lib, nr_ts=150, bc=("MUR",) * 6):
    api = pkg("openems_api")
    fd = api.openEMS(NrTS=nr_ts, EndCriteria=0, lib=lib)
    fd.SetGaussExcite(8e9, 6e9)
    fd.SetBoundaryCond(list(bc))
    csx = api.ContinuousStructure()
    fd.SetCSX(csx)
    mesh = csx.GetGrid()
    mesh.SetDeltaUnit(1e-3)
    mesh.AddLine("x", np.cumsum([0] + [1.0, 1.2, 0.9] * 5))       # a graded mesh: every length differs from its neighbour's
    mesh.AddLine("y", np.cumsum([0] + [1.1, 0.8] * 7))
    mesh.AddLine("z", np.cumsum([0] + [0.7, 1.0, 1.3] * 4))
    csx.AddMaterial("sub", epsilon=3.0).AddBox([2, 2, 2], [12, 10, 5])
    return fd, csx, [np.asarray(mesh.GetLines(a)) for a in "xyz"]


def test_voltage_and_current_probes_on_a_lumped_ports_own_boxes(oracle_lib):
    for sign in (1, -1):
        fd, csx, (x, y, z) = _scene(oracle_lib)
        start, stop = [x[5], y[5], z[3]], [x[7], y[6], z[6]]
        if sign < 0:
            start[2], stop[2] = stop[2], start[2]
        port = fd.AddLumpedPort(1, 50.0, start, stop, "z", 1.0)
        mid = [0.5 * (start[a] + stop[a]) for a in range(3)]
        # upstream's LumpedPort: the voltage along the centre line from start to stop with weight -1; the current through the
        # cross-section at mid-length, weight = the port's direction
        csx.AddProbe("ut", 0, weight=-1).AddBox([mid[0], mid[1], start[2]], [mid[0], mid[1], stop[2]])
        csx.AddProbe("it", 1, weight=sign, norm_dir="z").AddBox([start[0], start[1], mid[2]], [stop[0], stop[1], mid[2]])
        fd.Run(None)
        u, i = fd.sim.port_series()[0]
        pu, pi = fd.GetProbe("ut"), fd.GetProbe("it")
        assert np.abs(u).max() > 0 and np.abs(i).max() > 0
        assert np.array_equal(pu["val"], u) and np.array_equal(pi["val"], i)
        assert np.array_equal(pu["t"], np.arange(u.size) * fd.sim.dt) and np.array_equal(pi["t"], (np.arange(i.size) + 0.5) * fd.sim.dt)
        # a box with one zero extent names the normal by itself
        fd2, csx2, _ = _scene(oracle_lib)
        fd2.AddLumpedPort(1, 50.0, start, stop, "z", 1.0)
        csx2.AddProbe("it", 1, weight=sign).AddBox([start[0], start[1], mid[2]], [stop[0], stop[1], mid[2]])
        fd2.Run(None)
        assert np.array_equal(fd2.GetProbe("it")["val"], i)


def test_a_voltage_probe_walks_x_then_y_then_z():
    pr, grid = pkg("probes"), pkg("grid")
    g = grid.RectGrid(np.arange(6.0), np.arange(5.0), np.arange(4.0))
    idx, comp, sign = pr.voltage_path(g, (4, 1, 0), (2, 3, 2))
    want = [((2, 1, 0), 0, -1), ((3, 1, 0), 0, -1), ((2, 1, 0), 1, 1), ((2, 2, 0), 1, 1), ((2, 3, 0), 2, 1), ((2, 3, 1), 2, 1)]
    assert idx.tolist() == [int(g.flat(*p)) for p, _, _ in want] and comp.tolist() == [c for _, c, _ in want] and sign.tolist() == [s for _, _, s in want]
    assert pr.dual_plane(g, 2, 1.0, 1e-9) == 0 and pr.dual_plane(g, 2, 1.5, 1e-9) == 1 and pr.dual_plane(g, 2, 1.6, 1e-9) == 1


def test_field_probes_equal_get_field_over_the_lengths(oracle_lib):
    fd, csx, (x, y, z) = _scene(oracle_lib, nr_ts=60)
    fd.AddLumpedPort(1, 50.0, [x[5], y[5], z[3]], [x[7], y[6], z[6]], "z", 1.0)
    node = (6, 4, 5)
    at = [x[node[0]] + 0.3, y[node[1]] - 0.2, z[node[2]] + 0.1]          # the node nearest to start
    csx.AddProbe("et", 2).AddBox(at, at)
    csx.AddProbe("ht", 3).AddBox(at, [x[9], y[9], z[9]])
    fd.Run(None, setup_only=True)
    sim, e = fd.sim, fd.sim.engine
    g = sim.grid
    V, I = [], []
    for _ in range(60):
        e.run(1)
        V.append([float(e.get_field(0, c)[node[2], node[1], node[0]]) for c in range(3)])
        I.append([float(e.get_field(1, c)[node[2], node[1], node[0]]) for c in range(3)])
    et, ht = sim.probe_series("et"), sim.probe_series("ht")
    assert et["val"].shape == (3, 60) and ht["val"].shape == (3, 60) and np.abs(et["val"]).max() > 0 and np.abs(ht["val"]).min(axis=1).max() > 0
    for c in range(3):
        assert len({float(g.d[c][node[c]]), float(g.dd[c][node[c]])}) == 2
        assert np.array_equal(et["val"][c], np.array(V)[:, c] / g.d[c][node[c]])
        assert np.array_equal(ht["val"][c], np.array(I)[:, c] / g.dd[c][node[c]])
    assert np.array_equal(ht["t"], (np.arange(60) + 0.5) * sim.dt)
    with pytest.raises(ValueError, match=r"probe 'edge': the x edge at node \(15, 4, 5\) does not exist"):
        sim2 = _scene(oracle_lib)
        sim2[1].AddProbe("edge", 2).AddBox([x[15], y[4], z[5]], [x[15], y[4], z[5]])
        sim2[0].AddLumpedPort(1, 50.0, [x[5], y[5], z[3]], [x[7], y[6], z[6]], "z", 1.0)
        sim2[0].Run(None, setup_only=True)


def test_mode_probes_equal_the_rectangular_waveguide_ports(oracle_lib):
    fd, ports = pc.wg(oracle_lib, nr_ts=500)
    csx = fd.GetCSX()
    a = pc.WG_A
    e_te10 = ["0", "-sin(pi*x/16)/0.016", "0"]                                        # x in mm; e_PP = -(1/a) sin(pi x / a)
    h_te10 = [lambda x, y, z: np.sin(np.pi * (x * 1e-3) / a) / a, lambda x, y, z: 0 * x, "0"]
    csx.AddProbe("mode_u", 10, mode_function=e_te10).AddBox([0, 0, 24], [16, 8, 24])
    csx.AddProbe("mode_i", 11, mode_function=h_te10, norm_dir="z").AddBox([0, 0, 24], [16, 8, 24])
    csx.AddProbe("mode_i2", 11, weight=-1, mode_function=h_te10).AddBox([0, 0, 40], [16, 8, 40])    # port 2 looks along -z
    fd.Run(None)
    (u1, i1), (u2, i2) = fd.sim.port_series()
    for got, want in ((fd.GetProbe("mode_u")["val"], u1), (fd.GetProbe("mode_i")["val"], i1), (fd.GetProbe("mode_i2")["val"], i2)):
        assert np.abs(want).max() > 0
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"mode probe against the port's series: {err:.3e}")
        assert err <= 1e-12
    pl, port = fd.sim.probes["mode_u"].lists[0], fd.sim.vox.ports[0]
    assert np.array_equal(pl.idx, port.v_probes[0].idx)                               # the same routine: the same edges
    with pytest.raises(ValueError, match="mode_function = three per-component entries"):
        csx.AddProbe("bad", 10, mode_function="sin(x)")
    with pytest.raises(ValueError, match=r"probe 'bad' \(component y\): weight function 'x.imag': attribute access 'x.imag' is not allowed"):
        csx.AddProbe("bad", 10, mode_function=["0", "x.imag", "0"])


def test_probe_files_and_run_record(oracle_lib, tmp_path):
    fd, csx, (x, y, z) = _scene(oracle_lib, nr_ts=80)
    fd.AddLumpedPort(1, 50.0, [x[5], y[5], z[3]], [x[7], y[6], z[6]], "z", 1.0)
    csx.AddProbe("ut1", 0).AddBox([x[3], y[3], z[2]], [x[8], y[6], z[4]])
    csx.AddProbe("it1", 1, norm_dir="x").AddBox([x[6], y[4], z[3]], [x[6], y[7], z[5]])
    csx.AddProbe("ht1", 3).AddBox([x[6], y[6], z[6]], [x[6], y[6], z[6]])
    fd.Run(str(tmp_path))
    for name in ("ut1", "it1", "ht1"):
        got, r = np.loadtxt(os.path.join(str(tmp_path), name)), fd.GetProbe(name)
        assert np.array_equal(got[:, 0], r["t"]) and np.array_equal(got[:, 1:].T, np.atleast_2d(r["val"])) and np.abs(r["val"]).max() > 0
    rec = json.load(open(os.path.join(str(tmp_path), "fdtd_hip_run.json")))["probes"]
    assert [(p["name"], p["type"], p["kind"], p["file"], p["samples"], p["entries"]) for p in rec] == \
        [("ut1", 0, "voltage", "ut1", 80, [10]), ("it1", 1, "current", "it1", 80, [14]), ("ht1", 3, "H field", "ht1", 80, [1, 1, 1])]
    assert fd.stats.probes[1]["normal"] == "x" and fd.stats.probes[1]["dual_plane"] == 5
    ops = [c["op"] for c in fd.calls]
    assert ops.count("AddProbe") == 3
    with pytest.raises(KeyError, match="no probe 'nope'"):
        fd.GetProbe("nope")


def test_the_65th_device_probe_is_refused(oracle_lib):
    fd, csx, (x, y, z) = _scene(oracle_lib, nr_ts=10)
    fd.AddLumpedPort(1, 50.0, [x[5], y[5], z[3]], [x[7], y[6], z[6]], "z", 1.0)          # two device probes
    for q in range(20):
        csx.AddProbe(f"e{q}", 2).AddBox([x[3], y[3], z[3 + q % 4]], [x[3], y[3], z[3]])   # 60 more
    csx.AddProbe("u62", 0).AddBox([x[3], y[3], z[2]], [x[3], y[3], z[4]])
    csx.AddProbe("u63", 0).AddBox([x[3], y[3], z[2]], [x[3], y[3], z[4]])                # the 64th
    fd.Run(None, setup_only=True)
    assert sum(len(v) for v in fd.sim._probe_ids.values()) == 62
    fd.sim.engine.close()
    csx.AddProbe("u64", 0).AddBox([x[3], y[3], z[2]], [x[3], y[3], z[4]])
    with pytest.raises(ValueError, match=r"probe 'u64': its 1 device probe\(s\) would make 65 probes, a context takes 64 \(FDTD_MAX_PROBES\), the ports' 2 included"):
        fd.Run(None, setup_only=True)
    with pytest.raises(ValueError, match="AddProbe 'u64' is defined twice"):
        csx.AddProbe("u64", 0)
    with pytest.raises(ValueError, match=r"p_type must be one of 0 \(voltage\), 1 \(current\).*got 4"):
        csx.AddProbe("p", 4)
