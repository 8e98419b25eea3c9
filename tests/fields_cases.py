"""Shared cases of the field-dump tests (test_fields_cpu.py, test_fields_gpu.py): the boxes and random inputs fdtd_field_interp is
compared on, the small scenes the end-to-end tests run, and the reader of the two file formats."""
import numpy as np

from conftest import pkg

KINDS = ("E", "H", "J", "rotH")
MODES = (0, 1, 2)
STRIDES = ((1, 1, 1), (2, 3, 1), (3, 2, 2))

# name -> (nodes of the grid, lo, hi of the dump box in nodes); every mesh is graded (graded_lines)
INTERP_CASES = {
    "5x3x2-cells-inside": ((9, 8, 7), (2, 3, 2), (7, 6, 4)),
    "67x5x3-cells": ((72, 9, 8), (3, 2, 2), (70, 7, 5)),            # more points than one block of 256 threads, an odd count along x
    "one-cell-thick-x": ((9, 8, 7), (3, 1, 1), (4, 6, 5)),
    "one-cell-thick-y": ((9, 8, 7), (1, 4, 1), (7, 5, 5)),
    "one-cell-thick-z": ((9, 8, 7), (1, 1, 2), (7, 6, 3)),
    "touches-the-low-faces": ((9, 8, 7), (0, 0, 0), (4, 3, 2)),
    "touches-the-high-faces": ((9, 8, 7), (4, 4, 4), (8, 7, 6)),
    "the-whole-grid": ((6, 5, 4), (0, 0, 0), (5, 4, 3)),
}


def graded_lines(n, seed, h=1e-3):
    """n node lines whose cells grow and shrink by up to 1.4 from one to the next."""
    rng = np.random.default_rng(seed)
    d = h * np.cumprod(rng.uniform(1 / 1.4, 1.4, n - 1))
    return np.concatenate([[0.0], np.cumsum(d)])


def interp_inputs(name, cplx, seed=0):
    """(lines, lo, hi, recorded arrays [3], edge conductivities [3]) of INTERP_CASES[name]: values over six decades, one in seven an
    exact zero (a PEC edge), kappa zero in a third of the region."""
    fields = pkg("fields")
    n, lo, hi = INTERP_CASES[name]
    lines = [graded_lines(k, 100 * seed + 11 + a) for a, k in enumerate(n)]
    rlo, _ = fields.region(lo, hi)
    shape = tuple(hi[a] - rlo[a] + 1 for a in (2, 1, 0))
    rng = np.random.default_rng(1000 + seed + sum(map(ord, name)))
    rec = []
    for _ in range(3):
        a = rng.standard_normal(shape) * 10.0 ** rng.uniform(-6, 0, shape)
        if cplx:
            a = a + 1j * rng.standard_normal(shape) * 10.0 ** rng.uniform(-6, 0, shape)
        a[rng.random(shape) < 1 / 7] = 0.0
        rec.append(a)
    kap = [rng.uniform(0.0, 3.0, shape) * (rng.random(shape) < 2 / 3) for _ in range(3)]
    return lines, lo, hi, rec, kap


def spec_call(kind, mode, lines, lo, hi, rec, kap, sub):
    fields = pkg("fields")
    return fields.interp_spec(kind, mode, lines, lo, hi, V=rec, I=rec, kappa=kap if kind == "J" else None, sub=sub)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the 24 x 20 x 16 scene of the end-to-end tests: port, lossy block, CPML-4 -----------------------------------------------------------
E2E_STEPS = 300
E2E_FREQS = [1.7e9, 2e9]
# node boxes inside the CPML-4 layers' inner faces; the E box is thin, the rot-H box crosses the port, the H box is sub-sampled
E2E_BOXES = {
    "e": dict(start=(10e-3, 10e-3, 10e-3), stop=(36e-3, 28e-3, 20e-3), kind="E", mode=1),
    "h": dict(start=(10e-3, 10e-3, 10e-3), stop=(36e-3, 28e-3, 22e-3), kind="H", mode=2, sub_sampling=(2, 1, 3)),
    "roth": dict(start=(16e-3, 12e-3, 8e-3), stop=(28e-3, 24e-3, 12e-3), kind="rotH", mode=0),
}


def e2e_sim(mode, nf2ff=False, sar=False, fields=True, nr_ts=E2E_STEPS):
    """block_scene of the SAR tests (a lossy block on a plate, a z port from the floor) under CPML-4."""
    from test_sar_model_cpu import block_scene
    sc, sim = pkg("scene"), pkg("simulation")
    grid, s = block_scene()
    nf = E2E_FREQS if (nf2ff or mode == "dft") else None
    m = sim.Simulation(grid, sc.voxelize(s, grid), f0=2e9, fc=1e9, boundary="CPML", cpml_cells=4, nr_ts=nr_ts, nf2ff_mode=mode, nf2ff_freqs=nf)
    if sar:
        m.add_sar_box("block", (12e-3, 10e-3, 8e-3), (32e-3, 28e-3, 22e-3), [2e9], 4000.0 * (6.5e-3) ** 3)
    if fields:
        for name, kw in E2E_BOXES.items():
            m.add_field_box(name, freqs=[2e9], **kw)
    return m


# ---- the reader of the two file formats ---------------------------------------------------------------------------------------------
def read_vtk(path):
    """(x, y, z, {vector name: [3][nz][ny][nx]}) of an ASCII legacy-VTK rectilinear grid as fields.write_vtk writes it."""
    rows = open(path).read().split("\n")
    assert rows[0].startswith("# vtk DataFile") and rows[2] == "ASCII" and rows[3] == "DATASET RECTILINEAR_GRID"
    nx, ny, nz = (int(v) for v in rows[4].split()[1:])
    x, y, z = (np.array(rows[6 + 2 * a].split(), float) for a in range(3))
    npts, out, r = int(rows[11].split()[1]), {}, 12
    while r < len(rows) and rows[r].startswith("VECTORS"):
        vec = np.array([row.split() for row in rows[r + 1:r + 1 + npts]], float)
        out[rows[r].split()[1]] = np.moveaxis(vec.reshape(nz, ny, nx, 3), -1, 0)
        r += 1 + npts
    return x, y, z, out
