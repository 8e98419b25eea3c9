"""SAR (sar.py, Simulation.add_sar_box / sar, AddDump / GetSAR): the numpy specification on cases with known answers — a uniform field
in a homogeneous block, a linear loss density, a mass below one cell's, a tissue half-space under air with the "ieee" validity rule
and second pass against a brute-force restatement, a hand-computed 2 x 2 x 2 local case —, the plumbing of `density`, every refusal,
and the whole chain on the oracle: the power absorbed in a lossy block against the power the port accepted, at two cell sizes.
The cases of test_sar_gpu.py are built here, and the share of their voxels that sits on a status threshold is bounded here."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg

KAT = os.path.join(ROOT, "profiles", "sar", "kat.txt")
MARGIN = 1e-9            # a voxel whose margin to a status threshold is below this may take either status on the device
MAX_EXCLUDED = 0.01      # ... and at most this share of a case's voxels may be such


def _sar():
    return pkg("sar")


def _note(tag, lines):
    """Replace the block `tag` of profiles/sar/kat.txt when FDTD_WRITE_KAT is set (the committed record of the measured values)."""
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


def graded(n, seed, h=1e-3):
    """n cell sizes between 0.75 h and 1.3 h."""
    return h * np.random.default_rng(seed).uniform(0.75, 1.3, n)


def uniform_field_voltages(d, E):
    """Edge voltages [ncz+1][ncy+1][ncx+1] of the uniform complex field E = (Ex, Ey, Ez): V = E * delta (the last, unused entry of
    an axis repeats the last cell)."""
    shape = tuple(a.size + 1 for a in d[::-1])
    out = []
    for c in range(3):
        shp = [1, 1, 1]
        shp[2 - c] = d[c].size + 1
        out.append(np.broadcast_to((E[c] * np.append(d[c], d[c][-1])).reshape(shp), shape).copy())
    return out


# ---- 1. uniform field, homogeneous block -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["uniform", "graded"])
@pytest.mark.parametrize("method", ["ieee", "simple"])
def test_uniform_field_in_a_homogeneous_block(mesh, method):
    sar = _sar()
    n = (9, 8, 7)
    d = [np.full(k, 1e-3) for k in n] if mesh == "uniform" else [graded(k, 11 + a) for a, k in enumerate(n)]
    E = (3.0 - 1.0j, 0.5 + 2.0j, -1.5 + 0.25j)
    sigma, rho0 = 0.8, 1050.0
    shape = n[::-1]
    p, sl = sar.local_spec(*d, *uniform_field_voltages(d, E), np.full(shape, sigma), np.full(shape, rho0))
    want = 0.5 * sigma * sum(abs(e) ** 2 for e in E) / rho0
    assert np.allclose(sl, want, rtol=1e-13, atol=0)
    M = rho0 * (3.1e-3) ** 3                       # cubes 3.1 mm wide
    sa, half, status, counts = sar.average_spec(*d, np.full(shape, rho0), p, M, method)
    ok = status == 0
    assert ok.any() and (status == 3).any() and not np.any((status == 1) | (status == 2) | (status == -1))
    assert np.max(np.abs(sa[ok] / sl[ok] - 1.0)) <= 1e-12
    assert np.all(np.isnan(sa[status == 3])) and np.all(np.isnan(half[status == 3]))
    assert counts.tolist() == [int(ok.sum()), 0, 0, int((status == 3).sum())]
    # the cube holds the mass: m(h*) within 2^-40 of M, and h* is the half-side geometry gives
    box = sar._Box([np.asarray(a, float) for a in d], np.full(shape, rho0), p)
    for k, j, i in zip(*np.nonzero(ok)):
        m = box.sums((i, j, k), half[k, j, i], [box.rho])[0]
        assert m >= M and (m - M) / M <= 2.0 ** -40
    assert np.allclose(half[ok], 1.55e-3, rtol=1e-12, atol=0)
    # the status map: a voxel whose 3.1 mm cube leaves the box is 3
    lines = [sar.node_lines(np.asarray(a, float)) for a in d]
    for k in range(n[2]):
        for j in range(n[1]):
            for i in range(n[0]):
                c = [lines[a][1][q] for a, q in enumerate((i, j, k))]
                room = min(min(c[a], lines[a][0][-1] - c[a]) for a in range(3))
                if abs(room - 1.55e-3) > 1e-9:
                    assert status[k, j, i] == (0 if room > 1.55e-3 else 3), (i, j, k)


# ---- 2. p linear in x --------------------------------------------------------------------------------------------------------------
def test_linear_loss_density_averages_to_the_local_value():
    sar = _sar()
    n = (11, 7, 7)
    d = [np.full(k, 1e-3) for k in n]
    rho = np.full(n[::-1], 1000.0)
    xc = (np.arange(n[0]) + 0.5) * 1e-3
    p = np.broadcast_to(2.0 + 300.0 * xc, n[::-1]).copy()
    sa, half, status, _ = sar.average_spec(*d, rho, p, 1000.0 * (2.6e-3) ** 3, "ieee")
    ok = status == 0
    assert ok.sum() > 50
    assert np.max(np.abs(sa[ok] / (p[ok] / rho[ok]) - 1.0)) <= 1e-12


# ---- 3. a mass below one cell's ----------------------------------------------------------------------------------------------------
def test_mass_below_one_cells_mass_stays_inside_the_cell():
    sar = _sar()
    n = (6, 5, 4)
    d = [graded(k, 3 + a) for a, k in enumerate(n)]
    rng = np.random.default_rng(8)
    rho = rng.uniform(900.0, 1100.0, n[::-1])
    p = rng.uniform(0.5, 2.0, n[::-1])
    vol = d[2][:, None, None] * d[1][None, :, None] * d[0][None, None, :]
    M = 0.05 * float(np.min(rho * vol))
    sa, half, status, counts = sar.average_spec(*d, rho, p, M, "ieee")
    assert np.all(status == 0) and counts.tolist() == [rho.size, 0, 0, 0]
    hmin = 0.5 * np.minimum(np.minimum(d[2][:, None, None], d[1][None, :, None]), d[0][None, None, :])
    assert np.all(half < hmin)
    assert np.max(np.abs(sa / (p / rho) - 1.0)) <= 1e-12
    assert np.max(np.abs(rho * (2 * half) ** 3 / M - 1.0)) <= 1e-12


# ---- 4. half-space under air -------------------------------------------------------------------------------------------------------
def half_space(seed=4):
    """11 x 11 x 12 cells of 1 mm: tissue below z = 6 mm, air above, and one tissue cell afloat in the air (cell (2, 2, 7)); the mass
    of 8.5 cells gives cubes about 2.04 cells wide in the bulk."""
    n = (11, 11, 12)
    d = [np.full(k, 1e-3) for k in n]
    rho = np.zeros(n[::-1])
    rho[:6] = 1000.0
    rho[7, 2, 2] = 1000.0
    p = np.random.default_rng(seed).uniform(1.0, 3.0, n[::-1]) * (rho > 0)
    return d, rho, p, 8.5e-6


def brute_second_pass(d, sa, half, status):
    """The second pass restated: plain loops, centres from plain sums."""
    ctr = [np.cumsum(a) - 0.5 * a for a in d]
    out, st = sa.copy(), status.copy()
    valid = [(i, j, k) for k, j, i in zip(*np.nonzero(status == 0))]
    for k, j, i in zip(*np.nonzero(status == 1)):
        best = None
        for (i0, j0, k0) in valid:
            h0 = half[k0, j0, i0]
            if abs(ctr[0][i] - ctr[0][i0]) <= h0 and abs(ctr[1][j] - ctr[1][j0]) <= h0 and abs(ctr[2][k] - ctr[2][k0]) <= h0:
                best = sa[k0, j0, i0] if best is None else max(best, sa[k0, j0, i0])
        if best is None:
            out[k, j, i], st[k, j, i] = np.nan, 2
        else:
            out[k, j, i] = best
    return out, st


def test_half_space_under_air_validity_rule_and_second_pass():
    sar = _sar()
    d, rho, p, M = half_space()
    first = sar.average_spec(*d, rho, p, M, "simple")
    sa, half, status, counts = sar.average_spec(*d, rho, p, M, "ieee")
    # "simple": status 0 wherever a cube fits, and the same cubes as "ieee" finds
    assert np.array_equal(first[2] == 3, status == 3) and np.array_equal(first[2] == -1, rho == 0)
    assert np.all(first[2][(rho > 0) & (first[2] != 3)] == 0)
    assert np.array_equal(first[1], half, equal_nan=True)
    # the top tissue layer, away from the box's side faces: cubes reach into the air, status 1, value from the enclosing valid cubes
    top = status[5, 3:8, 3:8]
    assert np.all(top == 1) and np.all(status[3, 3:8, 3:8] == 0)
    # restated: the validity rule from the first pass's cubes, then the second pass by brute force
    box = sar._Box([np.asarray(a, float) for a in d], rho, p)
    st1 = first[2].copy()
    for k, j, i in zip(*np.nonzero(first[2] == 0)):
        vbg = box.sums((i, j, k), half[k, j, i], [box.bg])[0]
        if vbg > 0.1 * (2 * half[k, j, i]) ** 3:
            st1[k, j, i] = 1
    want, want_st = brute_second_pass(d, first[0], half, st1)
    assert np.array_equal(status, want_st)
    assert np.array_equal(sa, want, equal_nan=True)
    used = status == 1
    assert used.sum() > 25 and np.all(sa[used] != first[0][used])
    # the cell afloat in the air: its cube holds the mass but is mostly air, and no valid cube reaches it
    assert first[2][7, 2, 2] == 0 and status[7, 2, 2] == 2 and np.isnan(sa[7, 2, 2]) and np.isfinite(half[7, 2, 2])
    assert counts[2] == 1 and counts.tolist() == [int((status == s).sum()) for s in range(4)]


# ---- 5. local SAR by hand ----------------------------------------------------------------------------------------------------------
def test_local_sar_of_a_hand_computed_2x2x2_box():
    sar = _sar()
    dx, dy, dz = np.array([1e-3, 2e-3]), np.array([1e-3, 1e-3]), np.array([2e-3, 1e-3])
    Vx = np.zeros((3, 3, 3), complex); Vy = np.zeros((3, 3, 3), complex); Vz = np.zeros((3, 3, 3), complex)
    # cell (0, 0, 0): x edges at nodes (0,0,0), (0,1,0), (0,0,1), (0,1,1) [k][j][i]; the one at (0,1,1) is PEC and carries 0
    Vx[0, 0, 0], Vx[0, 1, 0], Vx[1, 0, 0], Vx[1, 1, 0] = 4e-3, 2e-3j, 2e-3 + 2e-3j, 0.0
    # y edges at (0,0,0), (1,0,0), (0,0,1), (1,0,1)
    Vy[0, 0, 0], Vy[0, 0, 1], Vy[1, 0, 0], Vy[1, 0, 1] = 1e-3, 1e-3, 1e-3, 1e-3
    # z edges at (0,0,0), (1,0,0), (0,1,0), (1,1,0)
    Vz[0, 0, 0], Vz[0, 0, 1], Vz[0, 1, 0], Vz[0, 1, 1] = 8e-3j, 0.0, 0.0, 0.0
    sigma = np.zeros((2, 2, 2)); rho = np.zeros((2, 2, 2))
    sigma[0, 0, 0], rho[0, 0, 0] = 2.0, 1000.0
    sigma[1, 1, 1], rho[1, 1, 1] = 1.0, 0.0               # a lossy background cell: p but no SAR
    Vz[1, 1, 1] = Vz[1, 1, 2] = Vz[1, 2, 1] = Vz[1, 2, 2] = 3e-3        # cell (1, 1, 1): Ez = 3 V/m
    p, sl = sar.local_spec(dx, dy, dz, Vx, Vy, Vz, sigma, rho)
    # Ex = ((4 + 2j + 2 + 2j + 0) / 4) mV / 1 mm = 1.5 + 1j; Ey = 1 mV / 1 mm = 1; Ez = (8j / 4) mV / 2 mm = 1j
    want_p = 0.5 * 2.0 * ((1.5 ** 2 + 1.0 ** 2) + 1.0 + 1.0)
    assert abs(p[0, 0, 0] / want_p - 1.0) < 1e-15 and abs(sl[0, 0, 0] / (want_p / 1000.0) - 1.0) < 1e-15
    assert abs(p[1, 1, 1] / (0.5 * 1.0 * 9.0) - 1.0) < 1e-15 and sl[1, 1, 1] == 0.0
    others = np.ones((2, 2, 2), bool)
    others[0, 0, 0] = others[1, 1, 1] = False
    assert np.all(p[others] == 0.0) and np.all(sl[others] == 0.0)
    with pytest.raises(ValueError, match="node box"):
        sar.local_spec(dx, dy, dz, Vx[:2], Vy, Vz, sigma, rho)
    with pytest.raises(ValueError, match="method"):
        sar.average_spec(dx, dy, dz, rho, p, 1e-6, "ieee-3")


# ---- 6. the cases of test_sar_gpu.py -----------------------------------------------------------------------------------------------
def _pockets(shape, seed, share=0.06):
    rng = np.random.default_rng(seed)
    rho = rng.uniform(900.0, 1150.0, shape)
    rho[rng.random(shape) < share] = 0.0
    return rho, rng.uniform(0.2, 3.0, shape) * (rng.random(shape) < 0.97)


def gpu_cases():
    """name -> (dx, dy, dz, rho, p, mass): the boxes test_sar_gpu.py runs fdtd_sar_average on, under both methods."""
    out = {}
    d = [graded(13, 21), graded(11, 22), graded(9, 23)]
    rho, p = _pockets((9, 11, 13), 24)
    rho[3:5, 4:6, 5:8] = 0.0                                         # an air pocket of 12 cells
    out["graded-13x11x9"] = (*d, rho, p, 1000.0 * (3.6e-3) ** 3)     # cubes 3 to 5 cells wide
    for name, n in (("line-1x1x17", (1, 1, 17)), ("line-17x1x1", (17, 1, 1))):
        d = [graded(k, 31 + a) if k > 1 else np.array([1.2e-3]) for a, k in enumerate(n)]      # 1.2 mm across, graded along
        rho, p = _pockets(n[::-1], 33, share=0.15)
        out[name] = (*d, rho, p, 1000.0 * (1.18e-3) ** 3)           # a cube almost as wide as the line: fits where the tissue is dense
    d = [graded(40, 41), graded(9, 42), graded(9, 43)]
    rho, p = _pockets((9, 9, 40), 44)
    out["long-40x9x9"] = (*d, rho, p, 1000.0 * (2.7e-3) ** 3)
    d = [graded(7, 51), graded(6, 52), graded(5, 53)]
    rho, p = _pockets((5, 6, 7), 54)
    out["below-a-cell-7x6x5"] = (*d, rho, p, 0.05 * 900.0 * (0.75e-3) ** 3)
    d = [graded(5, 61), graded(5, 62), graded(5, 63)]
    rho, p = _pockets((5, 5, 5), 64)
    out["no-cube-fits-5x5x5"] = (*d, rho, p, 1.0)
    return out


_SPEC = {}


def spec_of(name, method):
    """average_spec(..., margins=True) of a GPU case, computed once per process."""
    if (name, method) not in _SPEC:
        _SPEC[(name, method)] = _sar().average_spec(*gpu_cases()[name], method, margins=True)
    return _SPEC[(name, method)]


@pytest.mark.parametrize("method", ["ieee", "simple"])
@pytest.mark.parametrize("name", sorted(gpu_cases()))
def test_gpu_cases_keep_clear_of_the_status_thresholds(name, method):
    """The device sums in another order: a voxel within MARGIN of a threshold may come out with the other status there and is left out
    of the comparison of status bytes — at most MAX_EXCLUDED of a case, a condition on the seeds, checked on the specification alone."""
    sa, half, status, counts, marg = spec_of(name, method)
    tissue = status >= 0
    assert tissue.any()
    assert np.count_nonzero(marg[tissue] < MARGIN) <= MAX_EXCLUDED * status.size
    if name == "no-cube-fits-5x5x5":
        assert np.all(status[tissue] == 3)
    elif name == "below-a-cell-7x6x5":
        assert np.all(status[tissue] == 0)
    elif name == "graded-13x11x9":
        width = 2 * half[status == 0] / 1e-3
        assert width.min() > 2.7 and width.max() < 5.2 and (status == 0).sum() > 100
        assert method == "simple" or ((status == 1).sum() > 5)
    else:
        assert (status == 0).any() and (status == 3).any()


# ---- 7. plumbing and refusals ------------------------------------------------------------------------------------------------------
def block_scene(n=(24, 20, 16), u=2.0, density=4000.0, kappa=1.2, debye=False, lorentz=False):
    """A lossy block of tissue on a plate over the floor of the box, the plate fed by a z port from the floor; cells of u mm (the
    lines are those of the same AddLine calls: drawing units times the unit)."""
    sc = pkg("scene")
    grid = pkg("grid").RectGrid(*[(np.arange(k) * u) * 1e-3 for k in n])
    s = sc.Scene(unit=1e-3)
    s.add_material("tissue", 20.0, kappa, density=density).add_box((6 * u, 5 * u, 3 * u), (16 * u, 14 * u, 11 * u))
    if debye:
        s.add_debye_material("wet", 4.0, 0.0, [2.0], [8e-12], density=900.0).add_box((6 * u, 5 * u, 9 * u), (16 * u, 14 * u, 11 * u), priority=2)
    if lorentz:
        s.add_lorentz_material("res", 2.0, 0.0, wp=[2e10], w0=[4e10], gamma=[1e9], density=900.0).add_box((6 * u, 5 * u, 3 * u), (16 * u, 14 * u, 5 * u), priority=2)
    s.add_metal("plate").add_box((6 * u, 5 * u, 3 * u), (16 * u, 14 * u, 3 * u))
    s.add_lumped_port(1, 50.0, (11 * u, 9 * u, 0.0), (11 * u, 9 * u, 3 * u), "z", 1.0)
    return grid, s


BLOCK_BOX = ((10e-3, 8e-3, 4e-3), (34e-3, 30e-3, 24e-3))     # nodes (5, 4, 2) .. (17, 15, 12) of block_scene


def block_sim(nr_ts=300, boundary="PEC", cpml_cells=None, mode="record", nf2ff_freqs=None, **scene_kw):
    sc, sim = pkg("scene"), pkg("simulation")
    grid, s = block_scene(**scene_kw)
    return sim.Simulation(grid, sc.voxelize(s, grid), f0=2e9, fc=1e9, boundary=boundary, cpml_cells=cpml_cells, nr_ts=nr_ts,
                          nf2ff_mode=mode, nf2ff_freqs=nf2ff_freqs)


def test_density_reaches_the_voxel_scene(oracle_lib, monkeypatch):
    sc, api = pkg("scene"), pkg("openems_api")
    grid, s = block_scene()
    vox = sc.voxelize(s, grid)
    assert vox.density.shape == vox.kappa.shape and set(np.unique(vox.density)) == {0.0, 4000.0}
    assert np.array_equal(vox.density > 0, vox.kappa > 0) and int((vox.density > 0).sum()) == 10 * 9 * 8
    w = pkg("workloads").patch_workload("t", nx=24, ny=20, nz=16)
    assert sc.voxelize(w.scene, w.grid).density is None
    for bad in (-1.0, float("nan"), float("inf"), (1.0, 2.0)):
        with pytest.raises(ValueError, match="density"):
            sc.Scene().add_material("m", density=bad)

    def script(mod_csx, mod_ems):
        fd = mod_ems(NrTS=50, lib=oracle_lib)
        fd.SetGaussExcite(2e9, 1e9)
        fd.SetBoundaryCond(["PEC"] * 6)
        csx = mod_csx()
        fd.SetCSX(csx)
        g = csx.GetGrid()
        g.SetDeltaUnit(1e-3)
        for a, k in zip("xyz", (24, 20, 16)):
            g.AddLine(a, np.arange(k) * 2.0)
        csx.AddMaterial("tissue", epsilon=20.0, kappa=1.2, density=4000.0).AddBox([12, 10, 6], [32, 28, 22])
        # a sphere sends the scene through the owner arrays (voxelize_owners)
        csx.AddMaterial("fat", epsilon=5.0, kappa=0.1, density=900.0).AddSphere([22, 19, 14], 4.1, priority=3)
        fd.AddLumpedPort(1, 50, [22, 18, 0], [22, 18, 6], "z", 1.0)
        fd.Run("", setup_only=True)
        return fd
    fd = script(api.ContinuousStructure, api.openEMS)
    rho = fd.sim.vox.density
    assert set(np.unique(rho)) == {0.0, 900.0, 4000.0} and rho[7, 9, 11] == 900.0 and rho[4, 6, 7] == 4000.0
    assert {"op": "AddMaterial", "name": "tissue", "epsilon": 20.0, "kappa": 1.2, "density": 4000.0} in fd.calls
    # ... and under the upstream module names
    monkeypatch.syspath_prepend(os.path.join(ROOT, "fdtd-solver-antennas_amd", "compat"))
    for m in [k for k in sys.modules if k.split(".")[0] in ("openEMS", "CSXCAD")]:
        monkeypatch.delitem(sys.modules, m)
    import CSXCAD
    import openEMS
    fd2 = script(CSXCAD.ContinuousStructure, openEMS.openEMS)
    assert np.array_equal(fd2.sim.vox.density, rho)


def test_sar_box_refusals(oracle_lib):
    capi, api = pkg("_capi"), pkg("openems_api")
    f = [2e9]
    s = block_sim()
    s.add_sar_box("ok", *BLOCK_BOX, f, 1e-3)
    assert s.sar_boxes["ok"]["lo"] == (5, 4, 2) and s.sar_boxes["ok"]["hi"] == (17, 15, 12)
    with pytest.raises(ValueError, match="defined twice"):
        s.add_sar_box("ok", *BLOCK_BOX, f, 1e-3)
    with pytest.raises(ValueError, match="no whole cell along y"):
        s.add_sar_box("flat", (10e-3, 8e-3, 4e-3), (34e-3, 8.4e-3, 24e-3), f, 1e-3)
    with pytest.raises(ValueError, match="no cell of a material with density > 0"):
        s.add_sar_box("air", (36e-3, 8e-3, 4e-3), (44e-3, 30e-3, 24e-3), f, 1e-3)
    with pytest.raises(ValueError, match="above the recorder's band"):
        s.add_sar_box("high", *BLOCK_BOX, [3.5e9], 1e-3)
    with pytest.raises(ValueError, match="method"):
        s.add_sar_box("m", *BLOCK_BOX, f, 1e-3, method="cube")
    with pytest.raises(capi.FdtdError, match=r"SAR boxes need a single slab \(world = 1\)"):
        s.build(oracle_lib, rank=0, world=2)
    s.build(oracle_lib)
    with pytest.raises(ValueError, match="comes before build"):
        s.add_sar_box("late", *BLOCK_BOX, f, 1e-3)
    with pytest.raises(KeyError, match="no SAR box 'nope'"):
        s.sar("nope")
    # a scene without any density
    grid, sc = block_scene(density=0.0)
    s = pkg("simulation").Simulation(grid, pkg("scene").voxelize(sc, grid), f0=2e9, fc=1e9, boundary="PEC", nr_ts=100)
    with pytest.raises(ValueError, match="no cell of a material with density > 0"):
        s.add_sar_box("b", *BLOCK_BOX, f, 1e-3)
    # CPML layers: 4 cells of 2 mm; the box starts at node 2 in z
    s = block_sim(boundary="CPML", cpml_cells=4)
    with pytest.raises(ValueError, match=r"reaches into the CPML layer z- \(4 cells\)"):
        s.add_sar_box("b", *BLOCK_BOX, f, 1e-3)
    s.add_sar_box("b", (12e-3, 10e-3, 8e-3), (32e-3, 28e-3, 22e-3), f, 1e-3)
    # dispersive cells inside the box
    with pytest.raises(ValueError, match="holds cells of the Debye medium 'wet'"):
        block_sim(debye=True).add_sar_box("b", *BLOCK_BOX, f, 1e-3)
    with pytest.raises(ValueError, match="holds cells of the Lorentz medium 'res'"):
        block_sim(lorentz=True).add_sar_box("b", *BLOCK_BOX, f, 1e-3)
    block_sim(lorentz=True).add_sar_box("above", (10e-3, 8e-3, 10e-3), (34e-3, 30e-3, 24e-3), f, 1e-3)
    # the running DFT accumulates nf2ff_freqs only
    s = block_sim(mode="dft", nf2ff_freqs=[1.8e9, 2e9], boundary="MUR")
    s.add_sar_box("b", *BLOCK_BOX, [2e9], 1e-3)
    with pytest.raises(ValueError, match="2.2e\\+09 Hz is not among nf2ff_freqs"):
        s.add_sar_box("c", *BLOCK_BOX, [2.2e9], 1e-3)
    # FDTD_MAX_BOXES: 24 NF2FF requests + 3 per SAR box
    assert capi.MAX_BOXES == 64 and len(s.nf2ff_box.requests) == 24
    for q in range(12):
        s.add_sar_box(f"n{q}", *BLOCK_BOX, [2e9], 1e-3)
    with pytest.raises(ValueError, match=r"would make 66 recording boxes, a context takes 64 \(FDTD_MAX_BOXES\)"):
        s.add_sar_box("one-too-many", *BLOCK_BOX, [2e9], 1e-3)
    s.build(oracle_lib)                                              # 63 boxes: the engine takes them
    s = block_sim()
    for q in range(21):
        s.add_sar_box(f"n{q}", *BLOCK_BOX, f, 0.0)
    with pytest.raises(ValueError, match="FDTD_MAX_BOXES"):
        s.add_sar_box("n21", *BLOCK_BOX, f, 0.0)
    # AddDump: the SAR dump types only
    csx = api.ContinuousStructure()
    for t in (0, 1, 2, 3, 10, 11, 29):
        with pytest.raises(ValueError, match="field dumps are not supported"):
            csx.AddDump("Et", dump_type=t)
    with pytest.raises(ValueError, match="field dumps are not supported"):
        csx.AddDump("Et")
    with pytest.raises(ValueError, match="needs frequency"):
        csx.AddDump("sar", dump_type=21)
    d = csx.AddDump("sar", dump_type=22, frequency=[2e9], dump_mode=2)
    d.AddBox([0, 0, 0], [1, 1, 1])
    assert csx._log.calls[-2] == {"op": "AddDump", "name": "sar", "dump_type": 22, "frequency": [2e9], "sar_method": "ieee", "dump_mode": 2}
    assert csx._log.calls[-1]["op"] == "AddBox" and csx._log.calls[-1]["prop"] == "sar"
    # density is accepted on the dispersive materials (so that the refusal above can name them), nothing else new is
    csx.AddDebyeMaterial("wet", epsilon=4.0, eps_delta=[2.0], eps_relax_time=[8e-12], density=900.0)
    csx.AddLorentzMaterial("res", epsilon=2.0, eps_plasma=3e9, eps_pole_freq=6e9, density=900.0)
    with pytest.raises(TypeError, match="unknown keyword"):
        csx.AddDebyeMaterial("wet2", epsilon=4.0, eps_delta=[2.0], eps_relax_time=[8e-12], rho=900.0)


# ---- 8. end to end on the oracle: absorbed against accepted power ------------------------------------------------------------------
def cavity_script(api, lib, h, nr_ts=40000, dump_type=21, **kw):
    """A closed PEC box of 30 mm; a 12 mm block of tissue on a plate fed against the floor by a 50 ohm port: whatever the port
    accepts is absorbed in the block.  The SAR box is the block and one more cell of air (h = 1.5: on every side)."""
    fd = api.openEMS(NrTS=nr_ts, EndCriteria=1e-5, lib=lib, nf2ff_mode="record", **kw)
    fd.SetGaussExcite(2e9, 1e9)
    fd.SetBoundaryCond(["PEC"] * 6)
    csx = api.ContinuousStructure()
    fd.SetCSX(csx)
    g = csx.GetGrid()
    g.SetDeltaUnit(1e-3)
    for a in "xyz":
        g.AddLine(a, np.arange(int(round(30 / h)) + 1) * h)
    csx.AddMaterial("tissue", epsilon=20.0, kappa=1.0, density=1000.0).AddBox([9, 9, 3], [21, 21, 15])
    csx.AddMetal("plate").AddBox([9, 9, 3], [21, 21, 3])
    port = fd.AddLumpedPort(1, 50, [15, 15, 0], [15, 15, 3], "z", 1.0)
    csx.AddDump("sar", dump_type=dump_type, frequency=[2e9]).AddBox([7.5, 7.5, 1.5], [22.5, 22.5, 16.5])
    return fd, port


def edgewise_power(sim, name, f):
    """0.5 * sum G_e |V_e|^2 over the edges of SAR box `name`, G_e = kappa_e * dual area / length with the area-weighted kappa of
    ecoperator (the conductance the engine steps), from the same spectra Simulation.sar reads."""
    eco, exc = pkg("ecoperator"), pkg("excitation")
    b, g = sim.sar_boxes[name], sim.grid
    tw = exc.dft_twiddles(np.array([f]), sim.dt, sim.dft_every, sim.dft_nsamples, 0.0)
    total = 0.0
    for c in range(3):
        V = sim.engine.rec_transform(sim._sar_ids[name][c], tw)[0][0] * (2.0 * sim.dt * sim.dft_every)
        a1, a2 = (c + 1) % 3, (c + 2) % 3
        shp = lambda a, v: v.reshape([-1 if 2 - a == q else 1 for q in range(3)])
        G = eco._edge_average(sim.vox.kappa, g, c) * shp(a1, g.dd[a1]) * shp(a2, g.dd[a2]) / shp(c, g.d[c])
        hi = list(b["hi"])
        hi[c] -= 1                                                   # the edges inside the box
        sl = tuple(slice(b["lo"][a], hi[a] + 1) for a in (2, 1, 0))
        vs = tuple(slice(0, hi[a] - b["lo"][a] + 1) for a in (2, 1, 0))
        total += 0.5 * float(np.sum(G[sl] * np.abs(V[vs]) ** 2))
    return total


def test_absorbed_power_equals_accepted_power_on_the_oracle(oracle_lib):
    """P_abs of the SAR box against CalcPort's accepted power at the port's best-matched frequency, less nothing: the box is closed
    and loss-free but for the block.  Both are single-sided pulse spectra of one scale; a one-sided against a two-sided spectrum,
    a missing `every`, peak against rms would show as a factor 2 or 4.  The bar of 10 % at h = 1.5 mm is a condition; h / 2 must
    not be worse.  Measured (profiles/sar/kat.txt): ratio 0.9925 at h = 1.5 mm, 0.9966 at h = 0.75 mm."""
    api = pkg("openems_api")
    lines, err = [], []
    for h in (1.5, 0.75):
        fd, port = cavity_script(api, oracle_lib, h)
        fd.Run("")
        assert fd.stats.stopped_by_energy and fd.sim.nf2ff_mode == "record"
        band = np.linspace(1e9, 3e9, 81)
        port.CalcPort("", band)
        fb = float(band[np.argmin(np.abs(port.uf_ref / port.uf_inc))])
        port.CalcPort("", [fb])
        r = fd.GetSAR("sar", fb)
        ratio = r.P_abs / float(port.P_acc[0])
        edge = edgewise_power(fd.sim, "sar", fb)
        err.append(abs(ratio - 1.0))
        lines.append(f"h = {h} mm ({fd.sim.grid.shape[0]}^3 nodes, {fd.stats.steps} timesteps), best match at {fb / 1e9:.3f} GHz: "
                     f"P_abs / P_acc = {ratio:.5f}, cell-centred P_abs / edge-wise 0.5 sum G |V|^2 = {r.P_abs / edge:.5f}")
        print(lines[-1])
        # the edge-wise sum is the engine's own loss: it meets the accepted power closer than the 10 % bar by far
        assert abs(edge / float(port.P_acc[0]) - 1.0) <= 0.10
        # normalised to the accepted power: SAR per watt; the whole block's SAR is P_abs / mass
        rn = fd.GetSAR("sar", fb, normalise_to=float(port.P_acc[0]))
        assert abs(rn.P_abs - ratio) <= 1e-12 * ratio and np.allclose(rn.sar_local * port.P_acc[0], r.sar_local, rtol=1e-12, atol=0)
        assert abs(r.mass / (1000.0 * 12e-3 ** 3) - 1.0) < 1e-12
        rep = fd.stats.sar["sar"]
        assert rep["voxels"] == r.status.size and rep["status_counts"] == r.counts and rep["averaging_seconds"] >= 0 and rep["device"] is False
        assert sum(r.counts.values()) == r.status.size and r.counts["valid"] > 0
        k, j, i = np.unravel_index(np.nanargmax(r.sar_avg), r.sar_avg.shape)
        assert r.peak == r.sar_avg[k, j, i] and r.peak_cell == (i, j, k) and r.peak_position == (r.x[i], r.y[j], r.z[k])
    _note("absorbed against accepted power, closed PEC box (test_absorbed_power_equals_accepted_power_on_the_oracle)", lines)
    assert err[0] <= 0.10
    assert err[1] <= err[0]
