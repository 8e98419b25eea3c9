"""Field dumps: E, H, J and rot-H of a box on a point lattice (numpy, float64) — the specification of csrc/fields.hip.

What openEMS's field dumps (dump types 0..3 in the time domain, 10..13 in the frequency domain) deliver, from the recorded edge
voltages V_c or face currents I_c of a volume box (Simulation.add_field_box registers the three boxes, Simulation.field collects
them).  Every array is [z][y][x]; a complex spectrum is treated as two real arrays (re, im), each by the same real arithmetic.

Indices.  The grid has n_a node lines l_a per axis.  d_a[i] = l_a[i+1] - l_a[i] is the primal edge length (d_a[n_a-1] = d_a[n_a-2]:
the mirror of the last cell, as grid.RectGrid.d); where a rule below asks for d_a[-1] it is d_a[0].  dd_a[i] is the dual edge length
(grid.RectGrid.dd: 0.5 * (l_a[i+1] - l_a[i-1]) inside, the whole adjacent cell on the two outer lines).  For component c the
transverse axes are a1 = (c + 1) mod 3 and a2 = (c + 2) mod 3.  Edge c at node g runs from g to g + e_c; it exists when g lies in the
grid and g_c < n_c - 1.  Face c at node g has its normal along c, spans the cell g_a1..g_a1+1 x g_a2..g_a2+1 and exists when g
lies in the grid, g_a1 < n_a1 - 1 and g_a2 < n_a2 - 1.  An edge or face that does not exist counts as 0, whatever the arrays hold.

The dump box is the nodes lo..hi.  The recorded arrays cover the REGION max(lo - 1, 0)..hi: the box grown by one node on each low
side, clipped to the grid, because the node rules reach one index down.

Raw fields (dump_mode 0), at node index g of the box:

    E_c    = V_c[g] / d_c[g_c]                                                        at the edge's midpoint
    H_c    = I_c[g] / dd_c[g_c]                                                       at the face's centre
    J_c    = kappa_c[g] * (V_c[g] / d_c[g_c])                                         at the edge's midpoint
    Jtot_c = (((I_a2[g] - I_a2[g - e_a1]) - I_a1[g]) + I_a1[g - e_a2]) / (dd_a1[g_a1] * dd_a2[g_a2])     at the edge's midpoint

kappa_c is the operator's edge conductivity (ecoperator._edge_average of the cells' kappa: the kap_e of fdtd_build_operator; lumped
overrides do not enter).  The loop of Jtot is the current loop of scene._port_on_grid, so Jtot_c times the dual face area is the
current through the edge's dual face; it is taken at the time of H (half a step after E).

Node interpolation (dump_mode 1), at node g, F the raw field:

    E, J, Jtot:  (F_c[g - e_c] * dp + F_c[g] * dm) / (dm + dp)       dm = d_c[g_c - 1], dp = d_c[g_c]
    H:           0.25 * ((F_c[g] + F_c[g - e_a1]) + (F_c[g - e_a2] + F_c[g - e_a1 - e_a2]))

A missing neighbour is a zero field on a cell of the mirrored size (d_c[-1] = d_c[0], d_c[n_c-1] = d_c[n_c-2]).

Cell interpolation (dump_mode 2), at the centre of cell g (lo <= g < hi on every axis):

    E, J, Jtot:  0.25 * ((F_c[g] + F_c[g + e_a1]) + (F_c[g + e_a2] + F_c[g + e_a1 + e_a2]))
    H:           0.5 * (F_c[g] + F_c[g + e_c])

Sub-sampling (sx, sy, sz) keeps the points lo + q * s of every axis.  All of it in exactly this association (the library is built
with -ffp-contract=off): fdtd_field_interp gives ``interp_spec`` bit for bit.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from .grid import _primal, _dual

KINDS = {"E": 0, "H": 1, "J": 2, "rotH": 3}
KIND_NAMES = {v: k for k, v in KINDS.items()}
MODE_RAW, MODE_NODE, MODE_CELL = 0, 1, 2
H_TIME = {"E": False, "H": True, "J": False, "rotH": True}      # sampled half a step after E
NEEDS_I = {"E": False, "H": True, "J": False, "rotH": True}      # the recorded boxes are face currents (else edge voltages)
# upstream's dump types: time domain 0..3, frequency domain 10..13
DUMP_TYPES = {0: ("E", False), 1: ("H", False), 2: ("J", False), 3: ("rotH", False),
              10: ("E", True), 11: ("H", True), 12: ("J", True), 13: ("rotH", True)}
DUMP_TYPE_NAMES = {0: "Et", 1: "Ht", 2: "Jt", 3: "rotHt", 10: "Ef", 11: "Hf", 12: "Jf", 13: "rotHf"}


def region(lo, hi) -> Tuple[tuple, tuple]:
    """(lo, hi) of the recorded node box of dump box lo..hi."""
    return tuple(max(int(v) - 1, 0) for v in lo), tuple(int(v) for v in hi)


def out_counts(mode, lo, hi, sub=(1, 1, 1)) -> tuple:
    """(nx, ny, nz) output points."""
    ext = [int(hi[a]) - int(lo[a]) + (0 if mode == MODE_CELL else 1) for a in range(3)]
    return tuple((ext[a] - 1) // int(sub[a]) + 1 for a in range(3))


def check_args(kind, mode, lines, lo, hi, sub):
    if kind not in KINDS:
        raise ValueError(f"field dump: kind must be one of {sorted(KINDS)}, got {kind!r}")
    if mode not in (MODE_RAW, MODE_NODE, MODE_CELL):
        raise ValueError(f"field dump: dump_mode must be 0 (raw), 1 (node) or 2 (cell), got {mode!r}")
    lines = [np.ascontiguousarray(l, np.float64).ravel() for l in lines]
    for a, l in enumerate(lines):
        if l.size < 2 or not np.all(np.isfinite(l)) or not np.all(np.diff(l) > 0):
            raise ValueError(f"field dump: the {'xyz'[a]} lines must be finite, >= 2 and strictly increasing")
    lo, hi, sub = [int(v) for v in lo], [int(v) for v in hi], [int(v) for v in sub]
    for a in range(3):
        if not 0 <= lo[a] <= hi[a] <= lines[a].size - 1:
            raise ValueError(f"field dump: the box {lo[a]}..{hi[a]} along {'xyz'[a]} does not lie in the grid (0..{lines[a].size - 1})")
        if mode == MODE_CELL and hi[a] == lo[a]:
            raise ValueError(f"field dump: cell interpolation needs at least one cell along {'xyz'[a]}")
        if sub[a] < 1:
            raise ValueError("field dump: sub_sampling must be >= 1")
    return lines, lo, hi, sub


def _parts(a, shape, what):
    a = np.ascontiguousarray(a)
    if a.shape != shape:
        raise ValueError(f"field dump: {what} must cover the region [nz][ny][nx] = {shape}, got {a.shape}")
    if np.iscomplexobj(a):
        return np.stack([a.real, a.imag], axis=-1).astype(np.float64), True
    return a.astype(np.float64)[..., None], False


def interp_spec(kind, mode, lines, lo, hi, V=None, I=None, kappa=None, sub=(1, 1, 1)) -> np.ndarray:
    """field[3][nz][ny][nx] of the module text: complex128 for spectra, float64 for samples.  `lines`: the grid's three node-line
    arrays; lo, hi: the dump box in nodes; V / I: the three recorded arrays over region(lo, hi) (V for E and J, I for H and rotH);
    kappa: the three edge conductivities over the region (J)."""
    lines, lo, hi, sub = check_args(kind, mode, lines, lo, hi, sub)
    n = [l.size for l in lines]
    d, dd = [_primal(l) for l in lines], [_dual(l) for l in lines]
    rlo, _ = region(lo, hi)
    rshape = tuple(hi[a] - rlo[a] + 1 for a in (2, 1, 0))
    src = I if NEEDS_I[kind] else V
    if src is None or len(src) != 3:
        raise ValueError(f"field dump: kind {kind} needs the three recorded {'face currents I' if NEEDS_I[kind] else 'edge voltages V'}")
    got = [_parts(a, rshape, "a recorded array") for a in src]
    if len({c for _, c in got}) != 1:
        raise ValueError("field dump: the three recorded arrays must be all real or all complex")
    cplx, P = got[0][1], got[0][0].shape[-1]
    kap = None
    if kind == "J":
        if kappa is None or len(kappa) != 3:
            raise ValueError("field dump: kind J needs the three edge conductivities")
        kap = [_parts(np.asarray(k, np.float64), rshape, "an edge conductivity")[0] for k in kappa]

    # the extended index space lo - 2 .. hi of every axis; the window W = lo - 1 .. hi holds the raw fields
    g = [np.arange(lo[a] - 2, hi[a] + 1) for a in range(3)]
    inn = [(g[a] >= 0) & (g[a] <= n[a] - 1) for a in range(3)]
    cel = [(g[a] >= 0) & (g[a] < n[a] - 1) for a in range(3)]
    eshape = tuple(g[a].size for a in (2, 1, 0))

    def ax(a, v):
        shp = [1, 1, 1, 1]
        shp[2 - a] = -1
        return np.asarray(v).reshape(shp)

    def exists(c, face):
        a1, a2 = (c + 1) % 3, (c + 2) % 3
        return (ax(c, inn[c]) & ax(a1, cel[a1]) & ax(a2, cel[a2])) if face else (ax(c, cel[c]) & ax(a1, inn[a1]) & ax(a2, inn[a2]))

    def ext(A, c, face):
        X = np.zeros(eshape + (A.shape[-1],))
        X[tuple(slice(rlo[a] - (lo[a] - 2), None) for a in (2, 1, 0))] = A
        return np.where(exists(c, face), X, 0.0)

    def win(X, base, trim, shift=(0, 0, 0)):
        """X[first + shift .. last - trim + shift] on every axis."""
        return X[tuple(slice(base + shift[a], X.shape[2 - a] - trim + shift[a]) for a in (2, 1, 0))]

    def unit(a, s=1):
        e = [0, 0, 0]
        e[a] = s
        return tuple(e)

    def met(tab, a, idx):
        return ax(a, tab[a][np.clip(idx, 0, n[a] - 1)])

    gw = [g[a][1:] for a in range(3)]
    F = []
    for c in range(3):
        a1, a2 = (c + 1) % 3, (c + 2) % 3
        if kind in ("E", "J"):
            f = win(ext(got[c][0], c, False), 1, 0) / met(d, c, gw[c])
            if kind == "J":
                f = win(ext(kap[c], c, False), 1, 0) * f
        elif kind == "H":
            f = win(ext(got[c][0], c, True), 1, 0) / met(dd, c, gw[c])
        else:
            X1, X2 = ext(got[a1][0], a1, True), ext(got[a2][0], a2, True)
            cur = ((win(X2, 1, 0) - win(X2, 1, 0, unit(a1, -1))) - win(X1, 1, 0)) + win(X1, 1, 0, unit(a2, -1))
            f = cur / (met(dd, a1, gw[a1]) * met(dd, a2, gw[a2]))
        F.append(np.where(win(np.broadcast_to(exists(c, kind == "H"), eshape + (1,)), 1, 0), f, 0.0))

    out = []
    for c in range(3):
        a1, a2 = (c + 1) % 3, (c + 2) % 3
        if mode == MODE_RAW:
            v = win(F[c], 1, 0)
        elif mode == MODE_NODE:
            if kind == "H":
                m1, m2 = unit(a1, -1), unit(a2, -1)
                m12 = tuple(m1[a] + m2[a] for a in range(3))
                v = 0.25 * ((win(F[c], 1, 0) + win(F[c], 1, 0, m1)) + (win(F[c], 1, 0, m2) + win(F[c], 1, 0, m12)))
            else:
                gn = g[c][2:]
                dm, dp = met(d, c, gn - 1), met(d, c, gn)
                v = (win(F[c], 1, 0, unit(c, -1)) * dp + win(F[c], 1, 0) * dm) / (dm + dp)
        else:
            if kind == "H":
                v = 0.5 * (win(F[c], 1, 1) + win(F[c], 1, 1, unit(c)))
            else:
                p1, p2 = unit(a1), unit(a2)
                p12 = tuple(p1[a] + p2[a] for a in range(3))
                v = 0.25 * ((win(F[c], 1, 1) + win(F[c], 1, 1, p1)) + (win(F[c], 1, 1, p2) + win(F[c], 1, 1, p12)))
        out.append(v[::sub[2], ::sub[1], ::sub[0]])
    res = np.stack(out)
    # (re, im) pairs reinterpreted, not re + 1j * im: that sum would turn a real part of -0.0 into +0.0
    return np.ascontiguousarray(res).view(np.complex128)[..., 0] if cplx else np.ascontiguousarray(res[..., 0])


def offsets(kind, mode) -> Optional[np.ndarray]:
    """Raw mode: offsets[c][a] in cells (0 or 0.5) of component c's samples from the node along axis a; else None."""
    if mode != MODE_RAW:
        return None
    o = np.zeros((3, 3))
    for c in range(3):
        for a in range(3):
            o[c, a] = 0.5 if (a == c) != (kind == "H") else 0.0
    return o


def points(mode, lines, lo, hi, sub=(1, 1, 1)):
    """(x, y, z) of the output points: the nodes lo..hi (raw: the nodes the samples are indexed by), or the cell centres."""
    out = []
    for a in range(3):
        l = np.asarray(lines[a], np.float64)
        p = 0.5 * (l[lo[a]:hi[a]] + l[lo[a] + 1:hi[a] + 1]) if mode == MODE_CELL else l[lo[a]:hi[a] + 1]
        out.append(p[::int(sub[a])].copy())
    return tuple(out)


@dataclass
class FieldDump:
    """What Simulation.field returns.  field is [3][nz][ny][nx]: complex128 at `freq` (single-sided spectrum, as the port spectra),
    float64 at recorder sample `timestep` (taken at `time` seconds: H-time kinds half a step after the E-time ones)."""
    name: str
    type: str                   # "E", "H", "J", "rotH"
    mode: int                   # 0 raw, 1 node-interpolated, 2 cell-interpolated
    x: np.ndarray
    y: np.ndarray
    z: np.ndarray
    field: np.ndarray
    freq: Optional[float] = None
    timestep: Optional[int] = None
    time: Optional[float] = None
    offsets: Optional[np.ndarray] = None      # raw mode only: see offsets()
    device: bool = False        # the interpolation ran in csrc/fields.hip
    seconds: float = 0.0        # time spent in the interpolation


def evaluate(kind, mode, lines, lo, hi, V=None, I=None, kappa=None, sub=(1, 1, 1), device_call=None):
    """(field, seconds): the specification, or `device_call` (_capi.fields_device: fdtd_field_interp of csrc/fields.hip)."""
    import time
    t0 = time.perf_counter()
    f = (interp_spec if device_call is None else device_call)(kind, mode, lines, lo, hi, V, I, kappa, sub)
    return f, time.perf_counter() - t0


# ---- writers (no library: an ASCII legacy-VTK rectilinear grid, or one .npz) ---------------------------------------------------------
def _label(d: FieldDump) -> str:
    return f"{d.freq:.9g}Hz" if d.freq is not None else f"ts{int(d.timestep):010d}"


def write_vtk(path: str, d: FieldDump) -> str:
    """One dump as an ASCII VTK rectilinear grid (legacy format): a spectrum as the two vector fields <type>-field_re / _im, a snapshot
    as <type>-field.  Raw dumps go out on their index nodes (the per-component offsets are in the header line)."""
    nz, ny, nx = d.field.shape[1:]
    head = f"{d.name} {d.type} dump_mode={d.mode} " + (f"freq={d.freq!r}" if d.freq is not None else f"timestep={d.timestep} time={d.time!r}")
    if d.offsets is not None:
        head += " offsets=" + ",".join(f"{v:g}" for v in d.offsets.ravel())
    rows = ["# vtk DataFile Version 3.0", head, "ASCII", "DATASET RECTILINEAR_GRID", f"DIMENSIONS {nx} {ny} {nz}"]
    for a, v in zip("XYZ", (d.x, d.y, d.z)):
        rows += [f"{a}_COORDINATES {v.size} double", " ".join(repr(float(t)) for t in v)]
    rows.append(f"POINT_DATA {nx * ny * nz}")
    sets = [("_re", d.field.real), ("_im", d.field.imag)] if np.iscomplexobj(d.field) else [("", d.field)]
    for tag, f in sets:
        rows.append(f"VECTORS {d.type}-field{tag} double")
        vec = np.ascontiguousarray(np.moveaxis(f, 0, -1)).reshape(-1, 3)
        rows += [f"{float(a)!r} {float(b)!r} {float(c)!r}" for a, b, c in vec]
    with open(path, "w") as fh:
        fh.write("\n".join(rows) + "\n")
    return path


def write_npz(path: str, dumps: Sequence[FieldDump]) -> str:
    """All dumps of one box in one .npz: field [n][3][nz][ny][nx] with freq [n], or timestep [n] and time [n]."""
    d0 = dumps[0]
    arrs = {"name": np.array(d0.name), "type": np.array(d0.type), "mode": np.array(d0.mode), "x": d0.x, "y": d0.y, "z": d0.z,
            "field": np.stack([d.field for d in dumps])}
    if d0.freq is not None:
        arrs["freq"] = np.array([d.freq for d in dumps], np.float64)
    else:
        arrs["timestep"] = np.array([d.timestep for d in dumps], np.int64)
        arrs["time"] = np.array([d.time for d in dumps], np.float64)
    if d0.offsets is not None:
        arrs["offsets"] = d0.offsets
    with open(path, "wb") as fh:
        np.savez(fh, **arrs)
    return path


def write(sim_path: str, dumps: Sequence[FieldDump], file_type: int = 0) -> list:
    """The files of one box under sim_path: file_type 0 one <name>_<frequency or timestep>.vtk per dump, 1 one <name>.npz."""
    if file_type == 1:
        return [write_npz(os.path.join(sim_path, f"{dumps[0].name}.npz"), dumps)]
    if file_type != 0:
        raise ValueError(f"field dump: file_type must be 0 (vtk) or 1 (npz), got {file_type!r}")
    return [write_vtk(os.path.join(sim_path, f"{d.name}_{_label(d)}.vtk"), d) for d in dumps]
