"""Specific absorption rate: local and 1 g / 10 g mass-averaged (numpy, float64) — the specification of csrc/sar.hip.

What openEMS's SAR dumps (dump types 20 / 21 / 22) deliver after a run, from the frequency-domain edge voltages of a volume box
(Simulation.add_sar_box registers the three voltage boxes, Simulation.sar collects them).  A box has ncx x ncy x ncz cells; cell
(i, j, k) spans nodes i..i+1 on each axis.  Arrays are [z][y][x] like every other per-cell array of the package.

Local SAR (``local_spec`` = fdtd_sar_local, bit for bit): the cell-centre field along c is the complex mean of the cell's four
c-directed edges, each V / delta_c (a PEC edge carries its zero).  With the four edges a0..a3 in the order (0,0), (+1 on the first
transverse axis, 0), (0, +1 on the second), (+1, +1) — for x the nodes (i,j,k), (i,j+1,k), (i,j,k+1), (i,j+1,k+1); for y the first
transverse axis is x, the second z; for z they are x and y — separately for the real and the imaginary part:

    s = (a0 + a1) + (a2 + a3);  e = (0.25 * s) / delta_c;  q_c = e_re * e_re + e_im * e_im
    p = (0.5 * sigma) * ((q_x + q_y) + q_z)           [W/m^3]
    sar_local = p / rho  where rho > 0, else 0        [W/kg]

in exactly this association (the library is built with -ffp-contract=off).

Averaging (``average_spec``; fdtd_sar_average agrees to rounding, its sums run in another order): for target mass M and every cell
with rho > 0 a cube of half-side h centred on the cell centre c.  With the node coordinates e[0] = 0, e[i+1] = e[i] + d[i] and the
centres c[i] = 0.5 * (e[i] + e[i+1]), the overlap of [c - h, c + h] with cell i' is w[i'] = max(0, min(e[i'+1], c + h) -
max(e[i'], c - h)), per axis, and

    m(h) = sum rho wx wy wz,   P(h) = sum p wx wy wz,   Vbg(h) = sum over rho == 0 of wx wy wz.

h_max = the smallest distance from c to a face of the box.  m(h_max) < M: status 3 (box too small), NaN.  Otherwise 48 bisection
steps on [0, h_max] keeping the upper end (m(h*) >= M), sar_avg = P(h*) / m(h*).  Method "simple": status 0.  Method "ieee": status 0
only if Vbg(h*) <= 0.1 * (2 h*)^3, else 1 (unused); in a second pass a status-1 voxel takes the largest sar_avg of the status-0 cubes
that contain its cell centre (|c - c0| <= h0 on every axis), and becomes status 2 (NaN) if there is none.  The standard's third
stage (surface-attached cubes for those) is left out; their number is reported.  Background cells: status -1, value 0.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

N_BISECT = 48
BG_FRACTION = 0.1
METHODS = {"ieee": 0, "simple": 1}
STATUS_BACKGROUND, STATUS_VALID, STATUS_USED, STATUS_NO_CUBE, STATUS_TOO_SMALL = -1, 0, 1, 2, 3


def _cells(dx, dy, dz, *arrs):
    d = [np.ascontiguousarray(a, np.float64).ravel() for a in (dx, dy, dz)]
    shape = (d[2].size, d[1].size, d[0].size)
    if min(shape) < 1 or not all(np.all(np.isfinite(a)) and np.all(a > 0) for a in d):
        raise ValueError("SAR: the box needs at least one cell per axis and finite cell sizes > 0")
    out = []
    for a in arrs:
        a = np.ascontiguousarray(a, np.float64)
        if a.shape != shape:
            raise ValueError(f"SAR: per-cell arrays must be [ncz][ncy][ncx] = {shape}, got {a.shape}")
        if not (np.all(np.isfinite(a)) and np.all(a >= 0)):
            raise ValueError("SAR: per-cell values must be finite and >= 0")
        out.append(a)
    return d, shape, out


def centre_field_sq(V, c, d):
    """q_c of the module text: |cell-centre field along c|^2 from the edge voltages V complex [ncz+1][ncy+1][ncx+1]."""
    nz, ny, nx = (n - 1 for n in V.shape)
    X, Y, Z = slice(0, nx), slice(0, ny), slice(0, nz)
    X1, Y1, Z1 = slice(1, nx + 1), slice(1, ny + 1), slice(1, nz + 1)
    a = {0: (V[Z, Y, X], V[Z, Y1, X], V[Z1, Y, X], V[Z1, Y1, X]),
         1: (V[Z, Y, X], V[Z, Y, X1], V[Z1, Y, X], V[Z1, Y, X1]),
         2: (V[Z, Y, X], V[Z, Y, X1], V[Z, Y1, X], V[Z, Y1, X1])}[c]
    shp = [1, 1, 1]
    shp[2 - c] = d.size
    dd = d.reshape(shp)
    parts = []
    for part in (np.real, np.imag):
        s = (part(a[0]) + part(a[1])) + (part(a[2]) + part(a[3]))
        e = (0.25 * s) / dd
        parts.append(e * e)
    return parts[0] + parts[1]


def local_spec(dx, dy, dz, Vx, Vy, Vz, sigma, rho) -> Tuple[np.ndarray, np.ndarray]:
    """(p [W/m^3], sar_local [W/kg]) per cell, float64 [ncz][ncy][ncx]."""
    d, shape, (sigma, rho) = _cells(dx, dy, dz, sigma, rho)
    V = [np.ascontiguousarray(v, np.complex128) for v in (Vx, Vy, Vz)]
    for v in V:
        if v.shape != tuple(n + 1 for n in shape):
            raise ValueError(f"SAR: edge voltages must cover the node box {tuple(n + 1 for n in shape)}, got {v.shape}")
    q = [centre_field_sq(V[c], c, d[c]) for c in range(3)]
    p = (0.5 * sigma) * ((q[0] + q[1]) + q[2])
    sar = np.zeros(shape)
    on = rho > 0
    sar[on] = p[on] / rho[on]
    return p, sar


def node_lines(d):
    """(e, c): node coordinates e[0] = 0, e[i+1] = e[i] + d[i] (summed in order) and the cell centres."""
    e = np.zeros(d.size + 1)
    for i in range(d.size):
        e[i + 1] = e[i] + d[i]
    return e, 0.5 * (e[:-1] + e[1:])


def overlap(e, c, h):
    """(first cell, weights) of the cells of one axis that [c - h, c + h] can overlap."""
    lo, hi = c - h, c + h
    n = e.size - 1
    a = min(max(int(np.searchsorted(e, lo, side="right")) - 1, 0), n - 1)
    b = min(max(int(np.searchsorted(e, hi, side="left")) - 1, a), n - 1)
    w = np.maximum(0.0, np.minimum(e[a + 1:b + 2], hi) - np.maximum(e[a:b + 1], lo))
    return a, w


class _Box:
    def __init__(self, d, rho, p):
        self.lines = [node_lines(a) for a in d]
        self.rho, self.p, self.bg = rho, p, (rho == 0).astype(np.float64)

    def sums(self, cell, h, what):
        """The sums `what` (arrays [z][y][x]) over the cube of half-side h about cell (i, j, k)."""
        rng = [overlap(self.lines[a][0], self.lines[a][1][cell[a]], h) for a in range(3)]
        sl = tuple(slice(rng[a][0], rng[a][0] + rng[a][1].size) for a in (2, 1, 0))
        wx, wy, wz = rng[0][1], rng[1][1], rng[2][1]
        return [float(((arr[sl] @ wx) @ wy) @ wz) for arr in what]


def average_spec(dx, dy, dz, rho, p, mass, method="ieee", margins=False):
    """(sar_avg, half_side float64 [ncz][ncy][ncx], status int8, counts int64 [4]: voxels of status 0..3).  `margins`: also the
    smallest relative margin of each tissue voxel to a threshold that decides its status (|m(h_max) - M| / M and, method "ieee",
    |Vbg - 10 %| / 10 % of the cube) — where it is tiny another summation order may decide otherwise."""
    if method not in METHODS:
        raise ValueError(f"SAR: averaging method must be one of {sorted(METHODS)}, got {method!r}")
    mass = float(mass)
    if not (np.isfinite(mass) and mass > 0):
        raise ValueError("SAR: the averaging mass must be finite and > 0")
    d, shape, (rho, p) = _cells(dx, dy, dz, rho, p)
    box = _Box(d, rho, p)
    sar = np.zeros(shape)
    half = np.full(shape, np.nan)
    status = np.full(shape, STATUS_BACKGROUND, np.int8)
    marg = np.full(shape, np.inf)
    ext = [box.lines[a][0][-1] for a in range(3)]
    for k, j, i in zip(*np.nonzero(rho > 0)):
        cell = (i, j, k)
        c = [box.lines[a][1][cell[a]] for a in range(3)]
        h_max = min(min(c[a], ext[a] - c[a]) for a in range(3))
        m_max = box.sums(cell, h_max, [rho])[0]
        marg[k, j, i] = abs(m_max - mass) / mass
        if m_max < mass:
            status[k, j, i], sar[k, j, i] = STATUS_TOO_SMALL, np.nan
            continue
        lo, hi = 0.0, h_max
        for _ in range(N_BISECT):
            mid = 0.5 * (lo + hi)
            if box.sums(cell, mid, [rho])[0] >= mass:
                hi = mid
            else:
                lo = mid
        m, P, vbg = box.sums(cell, hi, [rho, p, box.bg])
        sar[k, j, i], half[k, j, i] = P / m, hi
        status[k, j, i] = STATUS_VALID
        if method == "ieee":
            side = 2.0 * hi
            lim = BG_FRACTION * ((side * side) * side)
            marg[k, j, i] = min(marg[k, j, i], abs(vbg - lim) / lim)
            if not vbg <= lim:
                status[k, j, i] = STATUS_USED
    if method == "ieee":
        sar, half, status = second_pass(box.lines, sar, half, status)
    counts = np.array([int(np.count_nonzero(status == s)) for s in range(4)], np.int64)
    return (sar, half, status, counts, marg) if margins else (sar, half, status, counts)


def second_pass(lines, sar, half, status):
    """A status-1 voxel takes the largest sar_avg of the status-0 cubes that contain its cell centre; none: status 2, NaN."""
    sar, status = sar.copy(), status.copy()
    cx, cy, cz = (l[1] for l in lines)
    k0, j0, i0 = np.nonzero(status == STATUS_VALID)
    h0, v0 = half[k0, j0, i0], sar[k0, j0, i0]
    for k, j, i in zip(*np.nonzero(status == STATUS_USED)):
        inside = (np.abs(cx[i] - cx[i0]) <= h0) & (np.abs(cy[j] - cy[j0]) <= h0) & (np.abs(cz[k] - cz[k0]) <= h0)
        if inside.any():
            sar[k, j, i] = float(np.max(v0[inside]))
        else:
            sar[k, j, i], status[k, j, i] = np.nan, STATUS_NO_CUBE
    return sar, half, status


@dataclass
class SARResult:
    """What Simulation.sar returns.  Per-cell arrays are [ncz][ncy][ncx]; x, y, z are the cell-centre coordinates in metres."""
    name: str
    freq: float
    averaging_mass: float       # [kg]; 0: local SAR only (sar_avg is sar_local, status 0 in tissue)
    method: str
    sar_local: np.ndarray
    sar_avg: np.ndarray
    status: np.ndarray
    half_side: np.ndarray
    peak: float
    peak_cell: Tuple[int, int, int]          # (i, j, k) inside the box
    peak_position: Tuple[float, float, float]
    P_abs: float                # sum p * vol over the box [W]
    mass: float                 # of the box [kg]
    counts: dict                # voxels per status: valid, used, no_cube, too_small, background
    x: np.ndarray
    y: np.ndarray
    z: np.ndarray
    device: bool = False        # the averaging ran in csrc/sar.hip
    seconds: float = 0.0        # time spent in the averaging
    normalised_to: Optional[float] = None


def evaluate(dx, dy, dz, Vx, Vy, Vz, sigma, rho, mass, method="ieee", device_calls=None):
    """(p, sar_local, sar_avg, half_side, status, counts, seconds in the averaging): the specification, or `device_calls`
    (_capi.sar_device: the pair (local, average) of csrc/sar.hip)."""
    import time
    local, average = (local_spec, average_spec) if device_calls is None else device_calls
    p, sl = local(dx, dy, dz, Vx, Vy, Vz, sigma, rho)
    rho = np.ascontiguousarray(rho, np.float64)
    t0 = time.perf_counter()
    if mass > 0:
        sa, half, status, counts = average(dx, dy, dz, rho, p, mass, method)
    else:
        sa, half = sl.copy(), np.full(sl.shape, np.nan)
        status = np.where(rho > 0, STATUS_VALID, STATUS_BACKGROUND).astype(np.int8)
        counts = np.array([int(np.count_nonzero(rho > 0)), 0, 0, 0], np.int64)
    return p, sl, sa, half, status, counts, time.perf_counter() - t0
