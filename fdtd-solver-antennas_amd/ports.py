"""Waveguide and microstrip-line ports: plain data and the numpy specification of their lists.

A port is, for the engine, nothing new: optional resistor edges (folded into the operator), ONE soft-source list (fdtd_add_source:
V_e += amp_e * signal[n]), a list of V-probes and a list of I-probes (fdtd_add_probe: sum_e w_e V_e after the E half-step, sum_f w_f I_f
after the H half-step).  V_e is an edge voltage (E times the edge length), I_f a face current (H times the dual length of the face's
component).  The face current (c, i, j, k) sits on the node line of axis c and half a cell up along the two other axes.  This module
computes these lists; scene.voxelize carries them in VoxelScene.ports and Simulation.build hands them over in the loop that serves the
lumped port.  Port boxes are in drawing units; every coordinate snaps to the nearest mesh line (grid.snap).  Entries whose weight is
zero (|f| <= 1e-12 of the largest mode value: the tangential E of a TE mode on its walls) are not listed.

Rectangular waveguide port (number, start, stop, p_dir, a, b, mode, excite, eps_r = 1)
    a, b [m] along the axes P = (p + 1) % 3 and PP = (p + 2) % 3; mode 'TEmn' (TM modes and m = n = 0 are refused by name);
    d = sign(stop[p] - start[p]) (d = 0 is refused); x, y are measured from the box's minimum corner along P and PP.
        e_P  =  (n / b) cos(m pi x / a) sin(n pi y / b)        h_P  = (m / a) sin(m pi x / a) cos(n pi y / b)
        e_PP = -(m / a) sin(m pi x / a) cos(n pi y / b)        h_PP = (n / b) cos(m pi x / a) sin(n pi y / b)
        kc^2 = (m pi / a)^2 + (n pi / b)^2
    The general waveguide port takes e = (e_P, e_PP), h = (h_P, h_PP) as callables of (x, y) and kc; the rectangular one is built on it.
    source   on the node plane of start[p]: every tangential edge inside the box that is not PEC, amp = excite e_c(edge midpoint) len_e
             (excite = 0: no source list).
    V-probe  on the node plane of stop[p]: U = sum_e V_e e_c(mid_e) w_e / sqrt(N_e); w_e the dual width across the edge within the
             plane (half the sum of the two adjoining cell widths, clipped to the box); N_e = sum_e e_c(mid_e)^2 len_e w_e.
    I-probe  the tangential face currents of the two half-planes adjoining that node plane (indices s - 1 and s along p), 1/2 each:
             I = d sum_f 1/2 I_f h_c(mid_f) len_f / sqrt(N_h); len_f the primal length transverse to the component at the face's
             in-plane position; N_h = sum_f h_c(mid_f)^2 len_f dual_f over ONE plane, dual_f the dual length of the component clipped
             to the box.  E_P x H_PP and -E_PP x H_P point along +p for the functions above, so a wave along d gives Re(U conj I) > 0
             (checked by tests/test_ports_cpu.py on every scene, not assumed).
    placement (check_placement): on the source and the probe plane every rim edge of the box must be PEC, or lie on a PEC / PMC grid
             face, itself or its neighbour one cell inwards or outwards; the first uncovered rim edge is named.  A source or probe edge
             (or probe face) that belongs to a correction list — Debye, Lorentz, conducting sheet, lumped element, plane-wave surface,
             conformal cut face — is refused with the edge and its owner.

Microstrip-line port (number, metal, start, stop, prop_dir, exc_dir, excite, feed_shift = 0, meas_plane_shift = None, feed_R = inf,
priority = 0)
    t is the third axis, d = sign(stop[prop] - start[prop]); zero extent along any of the three axes is refused.
    strip    a zero-thickness box on the plane stop[exc] over the full box, added to `metal` with `priority`.
    line m   the mesh line nearest start[prop] + d meas_plane_shift (default: half the length); m - d, m, m + d must lie inside the box.
    V-probes A, B, C on the lines m - d, m, m + d: the exc-directed edges from start[exc] to stop[exc] on the line of axis t nearest the
             strip centre, weight -sign(stop[exc] - start[exc]) (the lumped port's v_w): U = potential of the strip over the other plane.
    I-probes two, on the dual positions between A|B and B|C: the closed loop of face currents round the strip — the t-directed faces just
             below and just above the strip plane over the strip's nodes, the exc-directed faces just outside either rim —, weights
             +-1 (the right-handed loop about +prop, times d), so that a wave along d gives Re(U_B conj I) > 0.
    source   on the line nearest start[prop] + d feed_shift: the exc-directed edges under the strip, amp = excite len_e / sum(len) of
             one column.
    feed_R   finite and > 0: a resistor on the exc edges under the strip at the line of start[prop], split in series / parallel as the
             lumped port's; 0: those edges become PEC; inf: nothing.

Out of scope: coaxial, circular-waveguide, CPW, stripline and curve ports, TM modes, weight functions given as strings.  The lists use
global node indices and reach the ranks of a decomposed run through the same calls as a lumped port's; world > 1 is tested on the
waveguide scene cut at its ports' planes (2 and 3 slabs of one process: mailbox transport with two launches and with one launch per
timestep, linked contexts), not on the microstrip ports.
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from typing import Callable, List, NamedTuple, Optional, Tuple
import numpy as np

from .grid import RectGrid
from .ecoperator import LumpedEdge

AX = "xyz"
ZERO_WEIGHT = 1e-12


class Probe(NamedTuple):
    """One fdtd_add_probe call: global flat node indices, components, weights."""
    idx: np.ndarray
    comp: np.ndarray
    w: np.ndarray


@dataclass
class WaveguidePort:
    """AddWaveGuidePort / AddRectWaveGuidePort as plain data: e_func, h_func (x, y) -> (c_P, c_PP) in metres from the minimum corner."""
    number: int
    start: Tuple[float, float, float]
    stop: Tuple[float, float, float]
    direction: int
    e_func: Callable = None
    h_func: Callable = None
    kc: float = 0.0
    excite: float = 0.0
    eps_r: float = 1.0
    delay_steps: int = 0
    mode: Optional[str] = None       # 'TEmn' of a rectangular port
    kind: str = "waveguide"


@dataclass
class MSLPort:
    """AddMSLPort as plain data; `metal` is the scene.Metal the strip was added to."""
    number: int
    metal: object
    start: Tuple[float, float, float]
    stop: Tuple[float, float, float]
    prop: int
    exc: int
    excite: float = 0.0
    feed_shift: float = 0.0
    meas_plane_shift: Optional[float] = None
    feed_R: float = float("inf")
    priority: int = 0
    delay_steps: int = 0
    kind: str = "msl"


@dataclass
class PortLists:
    """What a port is on the grid: resistor edges, one source list, V-probes, I-probes, edges made PEC, and a summary (`info`: kind,
    direction, plane indices, edge counts — what fdtd_hip_run.json reports, and what check_placement and CalcPort read)."""
    lumped: List[LumpedEdge]
    src: Probe                       # (idx, comp, amp)
    v_probes: List[Probe]
    i_probes: List[Probe]
    pec: Tuple[np.ndarray, np.ndarray] = (np.zeros(0, np.int64), np.zeros(0, np.int8))
    info: dict = field(default_factory=dict)


def label(port) -> str:
    """'lumped port 1', 'waveguide port 2', 'MSL port 3': how a refusal names a port."""
    return f"{ {'waveguide': 'waveguide', 'msl': 'MSL'}.get(getattr(port, 'kind', None), 'lumped') } port {port.number}"


def check_funcs(who: str, *funcs) -> None:
    """Refuse weight functions given as strings (upstream's form: one string, or a list of two) and anything else not callable."""
    for f in funcs:
        if isinstance(f, str) or (isinstance(f, (list, tuple)) and any(isinstance(q, str) for q in f)):
            raise ValueError(f"{who}: weight functions given as strings are not supported: pass Python callables (x, y) -> (c_P, c_PP)")
        if not callable(f):
            raise ValueError(f"{who}: E_func and H_func must be callables (x, y) -> (c_P, c_PP)")


def _axis(v, who):
    a = {"x": 0, "y": 1, "z": 2}.get(v, v)
    if a not in (0, 1, 2):
        raise ValueError(f"{who}: a direction must be 0..2 or 'x', 'y', 'z', got {v!r}")
    return int(a)


def _probe(idx, comp, w, dtype=np.float32) -> Probe:
    return Probe(np.asarray(idx, np.int64).reshape(-1), np.asarray(comp, np.int8).reshape(-1), np.asarray(w, dtype).reshape(-1))


# ---- the rectangular guide's modes ---------------------------------------------------------------------------------------------
def rect_te_mode(a: float, b: float, mode: str, who: str = "rectangular waveguide port"):
    """(e_func, h_func, kc) of mode 'TEmn' in an a x b guide."""
    s = str(mode).upper()
    if s.startswith("TM"):
        raise ValueError(f"{who}: mode {mode!r}: TM modes are not supported (TE modes only)")
    got = re.fullmatch(r"TE(\d)(\d)", s)
    if not got:
        raise ValueError(f"{who}: mode {mode!r} is not of the form 'TEmn' with one digit each")
    m, n = int(got.group(1)), int(got.group(2))
    if m == 0 and n == 0:
        raise ValueError(f"{who}: mode TE00 does not exist (m = n = 0)")
    a, b = float(a), float(b)
    if not (a > 0 and b > 0):
        raise ValueError(f"{who}: a = {a!r} and b = {b!r} must be > 0 [m]")

    def e_func(x, y):
        return (n / b) * np.cos(m * np.pi * x / a) * np.sin(n * np.pi * y / b), -(m / a) * np.sin(m * np.pi * x / a) * np.cos(n * np.pi * y / b)

    def h_func(x, y):
        return (m / a) * np.sin(m * np.pi * x / a) * np.cos(n * np.pi * y / b), (n / b) * np.cos(m * np.pi * x / a) * np.sin(n * np.pi * y / b)
    return e_func, h_func, float(np.sqrt((m * np.pi / a) ** 2 + (n * np.pi / b) ** 2))


# ---- waveguide lists ---------------------------------------------------------------------------------------------------------------
def _clipped_dual(lines: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """Dual width of the node lines lo..hi: half the sum of the two adjoining cell widths, cells outside lo..hi left out."""
    w = np.zeros(hi - lo + 1)
    cell = np.diff(lines[lo:hi + 1])
    w[:-1] += 0.5 * cell
    w[1:] += 0.5 * cell
    return w


def _plane_items(grid: RectGrid, lo, hi, cell_ax: int, line_ax: int):
    """The items of a box cross-section that sit on the cells of `cell_ax` and on the node lines of `line_ax` (edges along cell_ax;
    faces of component line_ax), line index outer, cell index inner: (cell index, line index, cell position, line position, primal
    length along cell_ax, clipped dual width along line_ax)."""
    ic = np.arange(lo[cell_ax], hi[cell_ax])
    il = np.arange(lo[line_ax], hi[line_ax] + 1)
    L, C = np.meshgrid(il, ic, indexing="ij")
    L, C = L.reshape(-1), C.reshape(-1)
    dual = _clipped_dual(grid.lines[line_ax], lo[line_ax], hi[line_ax])[L - lo[line_ax]]
    return C, L, grid.centers(cell_ax)[C], grid.lines[line_ax][L], grid.d[cell_ax][C], dual


def _flat(grid: RectGrid, p: int, s: int, ax_a: int, ia, ax_b: int, ib):
    pos = [None, None, None]
    pos[p], pos[ax_a], pos[ax_b] = np.full(np.shape(ia), s), ia, ib
    return grid.flat(pos[0], pos[1], pos[2])


def _mode_items(grid: RectGrid, lo, hi, p: int, func, faces: bool):
    """Per tangential edge (faces=False) or face (faces=True) of the cross-section lo..hi: (comp, cell-axis index, line-axis index,
    cell axis, line axis, mode value of the component at the midpoint, primal length, clipped dual width), component P first."""
    P, PP = (p + 1) % 3, (p + 2) % 3
    x0, y0 = grid.lines[P][lo[P]], grid.lines[PP][lo[PP]]
    out = []
    for which, c in enumerate((P, PP)):
        o = PP if c == P else P
        cell_ax, line_ax = (o, c) if faces else (c, o)
        C, L, pc, pl, ln, dual = _plane_items(grid, lo, hi, cell_ax, line_ax)
        x, y = (pc - x0, pl - y0) if cell_ax == P else (pl - x0, pc - y0)
        val = np.asarray(func(x, y)[which], float) * np.ones_like(x)
        out.append((c, C, L, cell_ax, line_ax, val, ln, dual))
    return out


def mode_lists(grid: RectGrid, pec: np.ndarray, lo, hi, p: int, who: str, *, e_func=None, h_func=None, s_src=None, excite=0.0, s_prb=None,
               d: int = 1, dtype=np.float32):
    """The mode-matching lists over the cross-section lo..hi of the planes along axis p — what a waveguide port's source and probes
    are, and a stand-alone mode-matching probe (probes.py): (source list on node plane s_src, V-probe on node plane s_prb, I-probe on
    the two half-planes adjoining s_prb), each a Probe or None where its function or plane is not given.  e_func, h_func: (x, y) ->
    (c_P, c_PP), metres from the box's minimum corner."""
    src = v = i = None
    if e_func is not None:
        e_items = _mode_items(grid, lo, hi, p, e_func, False)
        e_max = max(float(np.max(np.abs(it[5]))) for it in e_items)
    if h_func is not None:
        h_items = _mode_items(grid, lo, hi, p, h_func, True)
        h_max = max(float(np.max(np.abs(it[5]))) for it in h_items)
    if not ((e_func is None or (e_max > 0 and np.isfinite(e_max))) and (h_func is None or (h_max > 0 and np.isfinite(h_max)))):
        raise ValueError(f"{who}: its mode functions are zero (or not finite) on every edge of the cross-section")
    pec_flat = pec.reshape(3, -1)

    def edges(s):
        """(idx, comp, e, len, w) of the live edges of node plane s."""
        parts = []
        for c, C, L, cell_ax, line_ax, val, ln, dual in e_items:
            idx = _flat(grid, p, s, cell_ax, C, line_ax, L)
            keep = (np.abs(val) > ZERO_WEIGHT * e_max) & ~pec_flat[c][idx]
            parts.append((idx[keep], np.full(int(keep.sum()), c, np.int8), val[keep], ln[keep], dual[keep]))
        return [np.concatenate([q[t] for q in parts]) for t in range(5)]
    if e_func is not None and s_src is not None:
        idx, comp, e, ln, w = edges(s_src)
        src = _probe(idx, comp, excite * e * ln, dtype)
    if e_func is not None and s_prb is not None:
        idx, comp, e, ln, w = edges(s_prb)
        n_e = float(np.sum(e * e * ln * w))
        if not n_e > 0:
            raise ValueError(f"{who}: every edge of its measurement plane (node {s_prb} along {AX[p]}) is metal (PEC)")
        v = _probe(idx, comp, e * w / np.sqrt(n_e), dtype)
    if h_func is not None and s_prb is not None:
        parts, n_h = [], 0.0
        for c, C, L, cell_ax, line_ax, val, ln, dual in h_items:
            keep = np.abs(val) > ZERO_WEIGHT * h_max
            n_h += float(np.sum(val[keep] ** 2 * ln[keep] * dual[keep]))
            for s in (s_prb - 1, s_prb):
                parts.append((_flat(grid, p, s, cell_ax, C, line_ax, L)[keep], np.full(int(keep.sum()), c, np.int8), 0.5 * d * val[keep] * ln[keep]))
        i = _probe(np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts]), np.concatenate([q[2] for q in parts]) / np.sqrt(n_h), dtype)
    return src, v, i


def waveguide_lists(grid: RectGrid, pec: np.ndarray, port: WaveguidePort, u: float, dtype=np.float32) -> PortLists:
    """The lists of a waveguide port; `dtype`: float32 is what the engine takes, float64 keeps the weights as computed (the tests of
    the mode functions' orthogonality read those)."""
    who = f"waveguide port {port.number}"
    p = _axis(port.direction, who)
    P, PP = (p + 1) % 3, (p + 2) % 3
    check_funcs(who, port.e_func, port.h_func)
    if port.stop[p] == port.start[p]:
        raise ValueError(f"{who}: start and stop coincide along {AX[p]}: the port has no direction (d = 0)")
    d = 1 if port.stop[p] > port.start[p] else -1
    lo = [grid.snap(a, min(port.start[a], port.stop[a]) * u) for a in range(3)]
    hi = [grid.snap(a, max(port.start[a], port.stop[a]) * u) for a in range(3)]
    for a in (P, PP):
        if hi[a] <= lo[a]:
            raise ValueError(f"{who}: its box has no cross-section along {AX[a]} on this mesh (nodes {lo[a]}..{hi[a]})")
    s_src, s_prb = grid.snap(p, port.start[p] * u), grid.snap(p, port.stop[p] * u)
    if s_src == s_prb:
        raise ValueError(f"{who}: start and stop snap to the same mesh line along {AX[p]} (node {s_src}): the port has no length on this mesh")
    if s_prb < 1 or s_prb > grid.shape[p] - 2:
        raise ValueError(f"{who}: its measurement plane (node {s_prb} along {AX[p]}) lies on a grid face: the current probe needs a half-plane on either side")
    src, v, i = mode_lists(grid, pec, lo, hi, p, who, e_func=port.e_func, h_func=port.h_func, s_src=s_src if port.excite != 0 else None,
                           excite=port.excite, s_prb=s_prb, d=d, dtype=dtype)
    if src is None:
        src = _probe([], [], [], dtype)
    info = {"kind": "waveguide" if port.mode is None else "rect_waveguide", "mode": port.mode, "direction": AX[p], "sign": d,
            "lo": [int(q) for q in lo], "hi": [int(q) for q in hi], "source_plane": int(s_src), "probe_plane": int(s_prb),
            "source_edges": int(src.idx.size), "v_probe_edges": [int(v.idx.size)], "i_probe_faces": [int(i.idx.size)], "resistor_edges": 0}
    return PortLists([], src, [v], [i], info=info)


# ---- microstrip-line lists ---------------------------------------------------------------------------------------------------------
def msl_geometry(grid: RectGrid, port: MSLPort, u: float) -> dict:
    """The snapped indices of an MSL port: box, direction signs, the lines of the source, the resistor and the probes."""
    who = f"MSL port {port.number}"
    prop, exc = _axis(port.prop, who), _axis(port.exc, who)
    if prop == exc:
        raise ValueError(f"{who}: the propagation and the excitation direction are both {AX[prop]}")
    t = 3 - prop - exc
    for a in range(3):
        if port.start[a] == port.stop[a]:
            raise ValueError(f"{who}: its box has zero extent along {AX[a]}")
    lo = [grid.snap(a, min(port.start[a], port.stop[a]) * u) for a in range(3)]
    hi = [grid.snap(a, max(port.start[a], port.stop[a]) * u) for a in range(3)]
    for a in range(3):
        if hi[a] <= lo[a]:
            raise ValueError(f"{who}: its box has zero extent along {AX[a]} on this mesh (node {lo[a]})")
    d = 1 if port.stop[prop] > port.start[prop] else -1
    sign_exc = 1 if port.stop[exc] > port.start[exc] else -1
    shift = 0.5 * abs(port.stop[prop] - port.start[prop]) if port.meas_plane_shift is None else float(port.meas_plane_shift)
    m = grid.snap(prop, (port.start[prop] + d * shift) * u)
    if not (lo[prop] <= m - 1 and m + 1 <= hi[prop]):
        raise ValueError(f"{who}: the measurement lines {m - 1}, {m}, {m + 1} along {AX[prop]} do not all lie inside its box (nodes {lo[prop]}..{hi[prop]}): "
                         f"move the measurement plane (MeasPlaneShift) or lengthen the port")
    feed = grid.snap(prop, (port.start[prop] + d * float(port.feed_shift)) * u)
    if not lo[prop] <= feed <= hi[prop]:
        raise ValueError(f"{who}: the feed line (node {feed} along {AX[prop]}) lies outside its box (nodes {lo[prop]}..{hi[prop]})")
    return {"prop": prop, "exc": exc, "t": t, "lo": lo, "hi": hi, "d": d, "sign_exc": sign_exc, "m": m, "feed": feed,
            "start_line": grid.snap(prop, port.start[prop] * u), "strip_plane": grid.snap(exc, port.stop[exc] * u),
            "t_centre": grid.snap(t, 0.5 * (port.start[t] + port.stop[t]) * u)}


def msl_lists(grid: RectGrid, pec: np.ndarray, port: MSLPort, u: float) -> PortLists:
    who = f"MSL port {port.number}"
    g = msl_geometry(grid, port, u)
    prop, exc, t, lo, hi, d = g["prop"], g["exc"], g["t"], g["lo"], g["hi"], g["d"]
    n = grid.shape
    es = g["strip_plane"]
    if es < 1 or es > n[exc] - 2 or lo[t] < 1 or hi[t] > n[t] - 2:
        raise ValueError(f"{who}: the strip touches a grid face: the current loop needs a cell on every side of it")
    ie = np.arange(lo[exc], hi[exc])                      # the exc-directed edges from one plane to the other
    it = np.arange(lo[t], hi[t] + 1)                      # the strip's nodes along t

    def flat(q_prop, q_exc, q_t):
        pos = [None, None, None]
        q_prop, q_exc, q_t = np.broadcast_arrays(q_prop, q_exc, q_t)
        pos[prop], pos[exc], pos[t] = q_prop, q_exc, q_t
        return grid.flat(pos[0], pos[1], pos[2]).reshape(-1)
    v_probes = [_probe(flat(q, ie, g["t_centre"]), np.full(ie.size, exc), np.full(ie.size, -g["sign_exc"])) for q in (g["m"] - d, g["m"], g["m"] + d)]
    # the right-handed loop about +prop round the strip's nodes (scene._port_on_grid's loop, summed over the nodes of the cross-section)
    a1, a2 = (prop + 1) % 3, (prop + 2) % 3
    i_probes = []
    for q in (min(g["m"] - d, g["m"]), min(g["m"], g["m"] + d)):      # the face currents of index q sit between the lines q and q + 1
        acc = {}
        for tn in it:
            pos = [0, 0, 0]
            pos[prop], pos[exc], pos[t] = q, es, int(tn)
            pm1 = list(pos); pm1[a1] -= 1
            pm2 = list(pos); pm2[a2] -= 1
            for comp, at, w in ((a2, pos, 1.0), (a2, pm1, -1.0), (a1, pos, -1.0), (a1, pm2, 1.0)):
                key = (comp, tuple(at))
                acc[key] = acc.get(key, 0.0) + w
        items = [(k, w) for k, w in acc.items() if w != 0.0]
        i_probes.append(_probe([grid.flat(*k[1]) for k, _ in items], [k[0] for k, _ in items], [d * w for _, w in items]))
    T, E = np.meshgrid(it, ie, indexing="ij")
    under = flat(g["feed"], E.reshape(-1), T.reshape(-1))
    length = float(np.sum(grid.d[exc][ie]))
    src = _probe(under, np.full(under.size, exc), port.excite * grid.d[exc][E.reshape(-1)] / length) if port.excite != 0 else _probe([], [], [])
    lumped, pec_edges = [], (np.zeros(0, np.int64), np.zeros(0, np.int8))
    R = float(port.feed_R)
    if R < 0 or np.isnan(R):
        raise ValueError(f"{who}: Feed_R = {port.feed_R!r} must be >= 0 (0: short, inf: open)")
    if R == 0:
        at = flat(g["start_line"], E.reshape(-1), T.reshape(-1))
        pec_edges = (at.astype(np.int64), np.full(at.size, exc, np.int8))
    elif np.isfinite(R):
        n_ser, n_par = ie.size, it.size
        for tn in it:
            for q in ie:
                pos = [0, 0, 0]
                pos[prop], pos[exc], pos[t] = g["start_line"], int(q), int(tn)
                lumped.append(LumpedEdge(exc, pos[0], pos[1], pos[2], n_ser / (R * n_par)))
    pl = grid.lines[prop]
    info = {"kind": "msl", "direction": AX[prop], "exc_direction": AX[exc], "sign": d, "lo": [int(q) for q in lo], "hi": [int(q) for q in hi],
            "source_plane": int(g["feed"]), "probe_planes": [int(g["m"] - d), int(g["m"]), int(g["m"] + d)], "strip_plane": int(es),
            "source_edges": int(src.idx.size), "v_probe_edges": [int(q.idx.size) for q in v_probes],
            "i_probe_faces": [int(q.idx.size) for q in i_probes], "resistor_edges": len(lumped) + int(pec_edges[0].size),
            # metres along the port's direction: A..C, and between the two loops (the midpoints of A|B and B|C)
            "dist_AC": float(abs(pl[g["m"] + 1] - pl[g["m"] - 1])), "dist_loops": float(0.5 * abs(pl[g["m"] + 1] - pl[g["m"] - 1])),
            "meas_pos": float(pl[g["m"]])}
    return PortLists(lumped, src, v_probes, i_probes, pec_edges, info)


def msl_strip_box(port: MSLPort):
    """(start, stop) in drawing units of the strip: the port's box flattened onto the plane stop[exc]."""
    start, stop = list(map(float, port.start)), list(map(float, port.stop))
    e = _axis(port.exc, f"MSL port {port.number}")
    start[e] = stop[e]
    return tuple(start), tuple(stop)


def lists(grid: RectGrid, pec: np.ndarray, port, u: float) -> PortLists:
    return msl_lists(grid, pec, port, u) if isinstance(port, MSLPort) else waveguide_lists(grid, pec, port, u)


# ---- placement ---------------------------------------------------------------------------------------------------------------------
def _at(grid: RectGrid, c: int, g: int) -> str:
    nx, ny, _ = grid.shape
    k, r = divmod(int(g), nx * ny)
    j, i = divmod(r, nx)
    return f"{AX[c]}-directed at node ({i}, {j}, {k})"


def check_placement(grid: RectGrid, port, info: dict, src: Probe, v_probes, i_probes, *, pec: np.ndarray, kinds=("PEC",) * 6,
                    debye=None, lorentz=None, sheets=None, elements=None, conformal=None, plane_wave=None) -> None:
    """Refuse (ValueError) a waveguide or MSL port the lists cannot serve (the rules: this module's docstring).  debye / lorentz:
    dispersion.DebyeEdges; sheets / elements: objects with idx, comp; conformal: conformal.ConformalFaces; plane_wave:
    planewave.PlaneWave (snapped)."""
    who = label(port)
    n = grid.shape
    if info["kind"] != "msl":
        p = AX.index(info["direction"])
        lo, hi = info["lo"], info["hi"]
        pec_flat = pec.reshape(3, -1)

        def covered(c, pos, o):
            for step in (0, -1, 1):
                q = list(pos)
                q[o] += step
                if not 0 <= q[o] <= n[o] - 1:
                    continue
                if pec_flat[c][grid.flat(*q)]:
                    return True
                if q[o] in (0, n[o] - 1) and kinds[2 * o + (1 if q[o] else 0)] in ("PEC", "PMC"):
                    return True
            return False
        for s in (info["source_plane"], info["probe_plane"]):
            for c in ((p + 1) % 3, (p + 2) % 3):
                o = 3 - p - c
                for rim in (lo[o], hi[o]):
                    for q in range(lo[c], hi[c]):
                        pos = [0, 0, 0]
                        pos[p], pos[c], pos[o] = s, q, rim
                        if not covered(c, pos, o):
                            raise ValueError(f"{who}: the rim edge {_at(grid, c, grid.flat(*pos))} of its box (nodes {tuple(lo)}..{tuple(hi)}) is neither "
                                             f"metal (PEC) nor on a PEC / PMC grid face, nor is its neighbour one cell away: the box must span the guide "
                                             f"from wall to wall along {AX[o]}")
    mine = [("source edge", src.comp, src.idx, False)] + [("voltage-probe edge", q.comp, q.idx, False) for q in v_probes] \
        + [("current-probe face", q.comp, q.idx, True) for q in i_probes]

    def refuse(what, c, g, owner):
        raise ValueError(f"{who}: its {what} {_at(grid, c, g)} {owner}: keep the port's planes clear of the correction lists (they are "
                         f"applied after the probes sample and would not see the source)")
    for kind, med in (("Debye", debye), ("Lorentz", lorentz)):
        if med is None:
            continue
        for what, comp, idx, is_face in mine:
            if is_face:
                continue
            k, r = np.divmod(idx, n[0] * n[1])
            j, i = np.divmod(r, n[0])
            for c in range(3):
                if c >= len(med.w) or med.w[c].size == 0:
                    continue
                blo, bhi = med.lo[c], med.hi[c]
                sel = (comp == c) & (i >= blo[0]) & (i < bhi[0]) & (j >= blo[1]) & (j < bhi[1]) & (k >= blo[2]) & (k < bhi[2])
                hit = np.flatnonzero(sel)
                hit = hit[med.w[c][k[hit] - blo[2], j[hit] - blo[1], i[hit] - blo[0]] != 0]
                if hit.size:
                    q = int(hit[0])
                    name = " / ".join(med.names[int(med.med[c][k[q] - blo[2], j[q] - blo[1], i[q] - blo[0]])])
                    refuse(what, c, idx[q], f"is an edge of the {kind} medium '{name}'")
    surf = (set(), set())
    if plane_wave is not None:
        from . import planewave as _planewave
        surf = _planewave.surface_keys(grid, plane_wave)
    for what, comp, idx, is_face in mine:
        key = idx * 3 + comp.astype(np.int64)
        if not is_face:
            for owner, lst in (("is a conducting-sheet edge", sheets), ("is a lumped-element edge", elements),
                               ("is cut by a conformal metal surface", None if conformal is None else conformal.frac)):
                if lst is not None and len(lst.idx):
                    hit = np.isin(key, np.asarray(lst.idx, np.int64) * 3 + np.asarray(lst.comp, np.int64))
                    if hit.any():
                        q = int(np.argmax(hit))
                        if owner.startswith("is a conducting") and hasattr(lst, "metals"):
                            e = int(np.flatnonzero((np.asarray(lst.idx) == idx[q]) & (np.asarray(lst.comp) == comp[q]))[0])
                            owner += f" of '{lst.metals[lst.metal[e]].name}'"
                        elif owner.startswith("is a lumped") and hasattr(lst, "elements"):
                            e = int(np.flatnonzero((np.asarray(lst.idx) == idx[q]) & (np.asarray(lst.comp) == comp[q]))[0])
                            owner += f" of '{lst.elements[lst.elem[e]].name}'"
                        refuse(what, int(comp[q]), idx[q], owner)
        elif conformal is not None and len(conformal.idx):
            hit = np.isin(key, np.asarray(conformal.idx, np.int64) * 3 + np.asarray(conformal.comp, np.int64))
            if hit.any():
                q = int(np.argmax(hit))
                refuse(what, int(comp[q]), idx[q], "is a conformal (cut) face")
        keys = surf[1 if is_face else 0]
        if keys:
            for c, g in zip(comp.tolist(), idx.tolist()):
                if (int(c), int(g)) in keys:
                    refuse(what, int(c), g, f"lies on the surface of the plane-wave box '{plane_wave.name}'")


# ---- post-processing ---------------------------------------------------------------------------------------------------------------
def waves(uf_tot, if_tot, Z_ref, beta=None, shift_m=None):
    """The lumped port's incident / reflected split with Z_ref, then the reference-plane shift: inc *= exp(-j Re(beta) s),
    ref *= exp(+j Re(beta) s), s [m] positive along the port's direction, the totals recomputed from the shifted waves."""
    uf_inc = 0.5 * (uf_tot + if_tot * Z_ref)
    if_inc = 0.5 * (if_tot + uf_tot / Z_ref)
    uf_ref = uf_tot - uf_inc
    if_ref = if_inc - if_tot
    if shift_m is not None:
        ph = np.exp(-1j * np.real(beta) * shift_m)
        uf_inc, if_inc, uf_ref, if_ref = uf_inc * ph, if_inc * ph, uf_ref / ph, if_ref / ph
        uf_tot, if_tot = uf_inc + uf_ref, if_inc - if_ref
    return uf_tot, if_tot, uf_inc, if_inc, uf_ref, if_ref


def waveguide_beta_zl(freq, kc: float, eps_r: float = 1.0):
    """beta = sqrt(k^2 - kc^2), -j sqrt(kc^2 - k^2) below cut-off, k = 2 pi f sqrt(eps_r) / c; ZL = 2 pi f mu0 / beta."""
    from .constants import C0, MU0
    f = np.atleast_1d(np.asarray(freq, float))
    k = 2 * np.pi * f * np.sqrt(eps_r) / C0
    beta = np.where(k >= kc, np.sqrt(np.maximum(k * k - kc * kc, 0.0)) + 0j, -1j * np.sqrt(np.maximum(kc * kc - k * k, 0.0)))
    with np.errstate(divide="ignore", invalid="ignore"):
        return beta, 2 * np.pi * f * MU0 / beta


def msl_beta_zl(uA, uB, uC, i1, i2, dist_AC: float, dist_loops: float):
    """Et = U_B, Ht = (I_1 + I_2) / 2, dEt = (U_C - U_A) / dist_AC, dHt = (I_2 - I_1) / dist_loops;
    beta = sqrt(-dEt dHt / (Ht Et)) with its sign flipped where Re beta < 0; ZL = sqrt(Et dEt / (Ht dHt))."""
    Et, Ht = uB, 0.5 * (i1 + i2)
    dEt, dHt = (uC - uA) / dist_AC, (i2 - i1) / dist_loops
    beta = np.sqrt(-dEt * dHt / (Ht * Et))
    beta = np.where(np.real(beta) < 0, -beta, beta)
    return Et, Ht, beta, np.sqrt(Et * dEt / (Ht * dHt))
