"""Shared cases of the anisotropic-dielectric tests (test_anisotropic_cpu.py, test_anisotropic_gpu.py).

The reference of every operator test is the composition identity ecoperator.build_operator states: component c of the anisotropic
operator is component c of the ISOTROPIC operator built from (eps_r[c], kappa[c]).  The oracle builds isotropic operators only, so
the reference is three oracle builds with one component taken from each (composed_oracle_operator)."""
import numpy as np

from conftest import pkg
from opbuild_cases import random_scene, engine_with_built_operator

_EPS_PAL = np.array([1.0, 4.3, 2.2, 9.8, 3.38, 6.15, 10.2, 1.5])      # random_scene's permittivities, all distinct: they name the material


def aniso_random_scene(seed, shape, graded, nmat, n_lumped=3, pec_frac=0.05):
    """random_scene's mesh, material map, PEC edges and lumped edges, with an independent random palette per axis:
    (grid, eps_axes [3][nz-1][ny-1][nx-1], kappa_axes, pec, lumped).  Material 0 stays vacuum on every axis."""
    grid, eps, kap, pec, lumped = random_scene(seed, shape, graded, nmat, n_lumped=n_lumped, pec_frac=pec_frac)
    mat = np.argmin(np.abs(eps[..., None] - _EPS_PAL[:nmat]), axis=-1)
    assert np.array_equal(_EPS_PAL[mat], eps)
    rng = np.random.default_rng(7000 + seed)
    pal_e = np.round(rng.uniform(1.5, 12.0, (3, nmat)), 2)
    pal_k = np.round(rng.uniform(0.0, 0.2, (3, nmat)), 4) * (rng.random((3, nmat)) < 0.7)
    pal_e[:, 0], pal_k[:, 0] = 1.0, 0.0
    return grid, np.stack([pal_e[c][mat] for c in range(3)]), np.stack([pal_k[c][mat] for c in range(3)]), pec, lumped


def engine_with_built_operator_axes(lib, grid, eps_axes, kap_axes, pec, lumped, dt, *, rank=0, world=1, prefer_classes=True):
    """opbuild_cases.engine_with_built_operator through fdtd_build_operator_axes."""
    capi, eco, simm, const = pkg("_capi"), pkg("ecoperator"), pkg("simulation"), pkg("constants")
    nx, ny, nz = grid.shape
    k0, nk = simm.slab_range(nz, world, rank)
    e = capi.Engine(lib, nx, ny, nz, dt, k0=k0, nk=nk, rank=rank, world=world, max_steps=8)
    emet, hmet = eco.pack_metric_tables(*eco.metric_lists(grid, dt), grid, k0, nk)
    e.build_operator_axes(grid.d, eps_axes, kap_axes, pec, const.EPS0, eco.lumped_overrides(grid, eps_axes, kap_axes, pec, dt, lumped),
                          emet, hmet, prefer_classes=prefer_classes)
    return e, k0, nk


def composed_oracle_operator(oracle_lib, grid, eps_axes, kap_axes, pec, lumped, dt, *, rank=0, world=1):
    """(vv, vi, ii, iv) [3][nk][ny][nx]: component c of the oracle's fdtd_build_operator for (eps_axes[c], kap_axes[c])."""
    out = None
    for c in range(3):
        e, _, _ = engine_with_built_operator(oracle_lib, grid, np.ascontiguousarray(eps_axes[c]), np.ascontiguousarray(kap_axes[c]), pec,
                                             lumped, dt, rank=rank, world=world)
        op = e.get_operator()
        if out is None:
            out = [np.empty_like(a) for a in op]
        for a, b in zip(out, op):
            a[c] = b[c]
    return tuple(out)


def pair_and_triple_counts(vv, vi_or_m):
    """(distinct (vv, m) pairs over all three components, distinct per-node class triples) of two float32 arrays [3][nk][ny][nx], with
    numpy.unique — what decides the device form: pairs > 256 raw, else triples > 256 one byte per edge, else one byte per cell."""
    key = (np.ascontiguousarray(vv).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.ascontiguousarray(vi_or_m).view(np.uint32).astype(np.uint64)
    uniq, inv = np.unique(key.ravel(), return_inverse=True)
    inv = inv.reshape(3, -1).astype(np.uint64)
    triples = np.unique(inv[0] | (inv[1] << np.uint64(16)) | (inv[2] << np.uint64(32))).size
    return int(uniq.size), int(triples)


# ---- scenes that see one axis only --------------------------------------------------------------------------------------------------
# A dielectric block through the whole extent along `axis`, closed there by the grid's PEC planes, driven by equal soft sources on every
# axis-directed edge of one column: the fields do not depend on the coordinate along `axis`, the two transverse E components stay
# exactly 0.0, and only eps[axis] / kappa[axis] of the block matter.
INVARIANT_EPS = (2.2, 3.4, 4.6)
INVARIANT_KAPPA = (0.02, 0.05, 0.11)
INVARIANT_STEPS = 200


def invariant_run(lib, axis, eps, kappa, nsteps=INVARIANT_STEPS):
    """The scene along `axis` with a block of (eps, kappa) — each one value or three — stepped on `lib`:
    (probe series, fields [2][3][nz][ny][nx], the Simulation)."""
    sc, sim, capi, grid_m = pkg("scene"), pkg("simulation"), pkg("_capi"), pkg("grid")
    a1, a2 = (axis + 1) % 3, (axis + 2) % 3
    n = [0, 0, 0]
    n[axis], n[a1], n[a2] = 8, 24, 20
    grid = grid_m.RectGrid(*[np.arange(k) * 1e-3 for k in n])
    lo, hi = [0.0] * 3, [0.0] * 3
    lo[axis], hi[axis] = -1.0, 8.0
    lo[a1], hi[a1] = 6.0, 15.0
    lo[a2], hi[a2] = 5.0, 12.0
    s = sc.Scene(unit=1e-3)
    s.add_material("block", eps, kappa).add_box(lo, hi)
    m = sim.Simulation(grid, sc.voxelize(s, grid), f0=8e9, fc=6e9, boundary="PEC", nr_ts=nsteps, end_criteria=0.0)
    e = m.build(lib)

    def column(p1, p2, ks):
        pos = np.zeros((len(ks), 3), np.int64)
        pos[:, axis], pos[:, a1], pos[:, a2] = ks, p1, p2
        return np.array([grid.flat(*p) for p in pos], np.int64)
    src = column(4, 4, range(n[axis] - 1))
    e.add_source(src, np.full(src.size, axis, np.int8), np.ones(src.size, np.float32), np.zeros(src.size, np.int32))
    idx = column(10, 8, [3])
    pid = e.add_probe(capi.KIND_V, idx, np.full(1, axis, np.int8), np.ones(1, np.float32))
    e.run(nsteps)
    return e.get_probe(pid), e.fields(), m


# ---- a closed cavity partly filled with a uniaxial block ------------------------------------------------------------------------------
CAVITY_STEPS = 6000


def cavity_lowest_resonance(lib, eps, nsteps=CAVITY_STEPS):
    """(frequency of the lowest resonance [Hz], DFT bin width [Hz]) of a loss-free PEC cavity of 40 x 32 x 24 mm whose corner region
    0..26 x 0..20 x 0..14 mm holds a block of `eps` (one value or three), driven and probed on z edges off every symmetry plane.  One
    Hann-windowed DFT of the one probe series; the lowest resonance is the lowest local maximum of at least a tenth of the largest."""
    sc, sim, capi, grid_m = pkg("scene"), pkg("simulation"), pkg("_capi"), pkg("grid")
    grid = grid_m.RectGrid(np.arange(21) * 2e-3, np.arange(17) * 2e-3, np.arange(13) * 2e-3)
    s = sc.Scene(unit=1e-3)
    s.add_material("block", eps, 0.0).add_box([-1, -1, -1], [26, 20, 14])
    m = sim.Simulation(grid, sc.voxelize(s, grid), f0=4.5e9, fc=3.5e9, boundary="PEC", nr_ts=nsteps, end_criteria=0.0)
    e = m.build(lib)
    one = lambda i, j, k: np.array([grid.flat(i, j, k)], np.int64)
    z8, w1 = np.full(1, 2, np.int8), np.ones(1, np.float32)
    e.add_source(one(6, 5, 3), z8, w1, np.zeros(1, np.int32))
    pid = e.add_probe(capi.KIND_V, one(13, 10, 8), z8, w1)
    e.run(nsteps)
    u = np.asarray(e.get_probe(pid), np.float64)
    assert u.size == nsteps and np.all(np.isfinite(u))
    spec = np.abs(np.fft.rfft(u * np.hanning(u.size)))
    df = 1.0 / (nsteps * m.dt)
    peaks = [q for q in range(2, spec.size - 1) if spec[q] > spec[q - 1] and spec[q] >= spec[q + 1] and spec[q] >= 0.1 * spec.max()]
    return peaks[0] * df, df


# ---- the end-to-end patch: uniaxial lossy substrate, sheet patch, port, element --------------------------------------------------------
PATCH_EPS = (4.8, 4.8, 4.3)
PATCH_STEPS = 300


def aniso_patch_sim(nr_ts=PATCH_STEPS, eps=PATCH_EPS):
    """The patch scene of workloads.patch_workload on its 52 x 44 x 30 grid with a uniaxial lossy substrate, the patch a conducting
    sheet (sheet edges), the lumped port through the substrate and a series R-L element through it under the patch."""
    wl, sc, sim, pd, const = pkg("workloads"), pkg("scene"), pkg("simulation"), pkg("patch_design"), pkg("constants")
    w = wl.patch_workload("test", nx=52, ny=44, nz=30)
    h = 1.6e-3
    L, W, _ = pd.design_patch_for_frequency(w.f0, 4.3, h)
    pw, pl, hh = W / 1e-3, L / 1e-3, h / 1e-3
    tand = (0.004, 0.004, 0.02)
    kappa = tuple(2 * np.pi * w.f0 * const.EPS0 * e * t for e, t in zip(eps, tand)) if np.ndim(eps) else 2 * np.pi * w.f0 * const.EPS0 * eps * 0.02
    s = sc.Scene(unit=1e-3)
    s.add_conducting_sheet("patch", 5.8e7, 35e-6).add_box([-pw / 2, -pl / 2, hh], [pw / 2, pl / 2, hh], priority=10)
    s.add_material("substrate", eps, kappa).add_box([-30, -30, 0], [30, 30, hh], priority=0)
    s.add_metal("gnd").add_box([-30, -30, 0], [30, 30, 0], priority=10)
    s.add_lumped_port(1, 50.0, [-6, 0, 0], [-6, 0, hh], "z", 1.0, priority=5)
    s.add_lumped_element("load", "z", R=150.0, L=2e-9, kind="series").add_box([8, 5, 0], [8, 5, hh])
    return sim.Simulation(w.grid, sc.voxelize(s, w.grid), f0=w.f0, fc=w.fc, boundary="CPML", cpml_cells=8, nr_ts=nr_ts, nf2ff_freqs=[w.f0])
