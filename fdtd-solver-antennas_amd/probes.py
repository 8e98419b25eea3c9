"""Stand-alone probes (CSX.AddProbe): plain data and the numpy specification of their lists.  Every probe is one or three
fdtd_add_probe lists (ports.Probe) — sum_e w_e V_e after the E half-step, sum_f w_f I_f after the H half-step; no kernel work.

    type 0   voltage       weight * sum of the edge voltages along the staircase path from start to stop: along x, then y, then z
                           between the nodes nearest to start and stop, every edge with the sign of the walk (`voltage_path`, the
                           rule of the lumped port's voltage line, whose probe is this one with weight -1)
    type 1   current       the box has one zero extent, or norm_dir names the axis: weight * the closed loop of face currents round the
                           nodes of the box's cross-section, right-handed about +norm_dir, on the dual plane nearest the box's
                           position along norm_dir, the lower one of two equally near (`current_loop`, the lumped port's loop)
    type 2   E field       at the node nearest start: three series V_c / l_c (the edge that starts at the node, its primal length)
    type 3   H field       likewise I_c / l~_c (the face at the node, the dual length of its component)
    type 10  mode voltage  over a plane (norm_dir or the zero extent of the box): sum_e V_e f_c(mid_e) w_e / sqrt(N_e), the V-probe of a
    type 11  mode current  waveguide port (ports.mode_lists) resp. its I-probe, times weight; mode_function: three per-component entries,
                           callables (x, y, z) or strings (field_excitation.compile_weight), coordinates in drawing units

Current-type probes (1, 3, 11) are sampled half a step after the voltage types.  A context takes 64 device probes (FDTD_MAX_PROBES),
the ports' included; a field probe takes three."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple
import numpy as np

from .grid import RectGrid

AX = "xyz"
TYPES = {0: "voltage", 1: "current", 2: "E field", 3: "H field", 10: "mode voltage", 11: "mode current"}
CURRENT_TYPES = (1, 3, 11)
MAX_PROBES = 64        # FDTD_MAX_PROBES (csrc/fdtd_ctx.h)


def voltage_path(grid: RectGrid, p0, p1):
    """The edges of the staircase path from node p0 to node p1 — along x, then y, then z; the edges of one leg in ascending order —
    as (idx int64, comp int8, sign float64): +1 for an edge walked upwards, -1 downwards."""
    cur = [int(v) for v in p0]
    idx, comp, sign = [], [], []
    for a in range(3):
        lo, hi = sorted((cur[a], int(p1[a])))
        s = 1.0 if int(p1[a]) >= cur[a] else -1.0
        for q in range(lo, hi):
            pos = list(cur)
            pos[a] = q
            idx.append(int(grid.flat(*pos))); comp.append(a); sign.append(s)
        cur[a] = int(p1[a])
    return np.array(idx, np.int64), np.array(comp, np.int8), np.array(sign, np.float64)


def current_loop(grid: RectGrid, lo, hi, d: int, q: int):
    """The closed loop of face currents round the nodes lo..hi of the cross-section normal to d, on the dual plane of index q (the faces
    between the node planes q and q + 1), right-handed about +d: (idx int64, comp int8, w float64), inner faces cancelled."""
    a1, a2 = (d + 1) % 3, (d + 2) % 3
    acc = {}

    def add(comp, pos, w):
        key = (comp, tuple(pos))
        acc[key] = acc.get(key, 0.0) + w

    for p1 in range(lo[a1], hi[a1] + 1):
        for p2 in range(lo[a2], hi[a2] + 1):
            pos = [0, 0, 0]
            pos[d], pos[a1], pos[a2] = q, p1, p2
            pm1 = list(pos); pm1[a1] -= 1
            pm2 = list(pos); pm2[a2] -= 1
            add(a2, pos, +1.0); add(a2, pm1, -1.0)
            add(a1, pos, -1.0); add(a1, pm2, +1.0)
    items = [(k, w) for k, w in acc.items() if abs(w) > 0]
    return (np.array([grid.flat(*k[1]) for k, _ in items], np.int64), np.array([k[0] for k, _ in items], np.int8),
            np.array([w for _, w in items], np.float64))


def dual_plane(grid: RectGrid, a: int, coord: float, tol: float) -> int:
    """The index of the dual plane (cell centre) along axis a nearest to coord [m]; of two equally near the lower."""
    dist = np.abs(grid.centers(a) - coord)
    return int(np.nonzero(dist <= dist.min() + tol)[0][0])


@dataclass
class ProbeSpec:
    """AddProbe(name, p_type, weight, norm_dir, mode_function) + AddBox(start, stop) as plain data (drawing units)."""
    name: str
    p_type: int
    weight: float = 1.0
    norm_dir: Optional[int] = None
    mode_function: Optional[list] = None
    start: Optional[Tuple[float, float, float]] = None
    stop: Optional[Tuple[float, float, float]] = None


@dataclass
class ProbeLists:
    """A probe on the grid: kind (0: V, 1: I), its one or three lists (ports.Probe), per list the divisor of its series (the length of
    a field probe's element, else 1) and what fdtd_hip_run.json reports."""
    name: str
    p_type: int
    kind: int
    lists: list
    scale: List[float]
    info: dict = field(default_factory=dict)


def make(name, p_type, weight=1, norm_dir=None, mode_function=None) -> ProbeSpec:
    from . import field_excitation as _fexc
    who = f"probe '{name}'"
    if isinstance(p_type, bool) or p_type not in TYPES:
        raise ValueError(f"{who}: p_type must be one of " + ", ".join(f"{t} ({n})" for t, n in sorted(TYPES.items())) + f", got {p_type!r}")
    if not (np.ndim(weight) == 0 and np.isfinite(float(weight))):
        raise ValueError(f"{who}: weight = {weight!r} must be one finite value")
    nd = None
    if norm_dir is not None:
        nd = {"x": 0, "y": 1, "z": 2}.get(norm_dir, norm_dir)
        if nd not in (0, 1, 2):
            raise ValueError(f"{who}: norm_dir must be 0..2 or 'x', 'y', 'z', got {norm_dir!r}")
    funcs = None
    if p_type in (10, 11):
        if mode_function is None or isinstance(mode_function, str) or callable(mode_function) or len(mode_function) != 3:
            raise ValueError(f"{who}: a mode-matching probe needs mode_function = three per-component entries (callables or strings)")
        funcs = _fexc.parse_weight(list(mode_function), who)
    elif mode_function is not None:
        raise ValueError(f"{who}: mode_function belongs to the mode-matching types 10 and 11")
    return ProbeSpec(str(name), int(p_type), float(weight), None if nd is None else int(nd), funcs)


def lists(grid: RectGrid, pec: np.ndarray, spec: ProbeSpec, u: float, tol: float) -> ProbeLists:
    from .ports import Probe, mode_lists
    who = f"probe '{spec.name}'"
    if spec.start is None:
        raise ValueError(f"{who} has no box: AddBox(start, stop) places it")
    n = grid.shape
    t = spec.p_type
    a0 = [grid.snap(a, spec.start[a] * u) for a in range(3)]
    a1 = [grid.snap(a, spec.stop[a] * u) for a in range(3)]
    lo, hi = [min(p, q) for p, q in zip(a0, a1)], [max(p, q) for p, q in zip(a0, a1)]
    f32 = lambda w: np.asarray(w, np.float64).astype(np.float32)
    info = {"name": spec.name, "type": t, "kind": TYPES[t], "weight": spec.weight}
    if t == 0:
        idx, comp, sign = voltage_path(grid, a0, a1)
        if idx.size == 0:
            raise ValueError(f"{who}: start and stop snap to the same node {tuple(a0)}: the voltage path has no edge on this mesh")
        info.update(entries=[int(idx.size)], start_node=a0, stop_node=a1)
        return ProbeLists(spec.name, t, 0, [Probe(idx, comp, f32(spec.weight * sign))], [1.0], info)
    if t in (2, 3):
        out = []
        for c in range(3):
            exists = (a0[c] < n[c] - 1) if t == 2 else (a0[(c + 1) % 3] < n[(c + 1) % 3] - 1 and a0[(c + 2) % 3] < n[(c + 2) % 3] - 1)
            if not exists:
                raise ValueError(f"{who}: the {AX[c]} {'edge' if t == 2 else 'face'} at node {tuple(a0)} does not exist (the node lies on the "
                                 f"upper grid face): move the probe one cell inwards")
            out.append(Probe(np.array([grid.flat(*a0)], np.int64), np.array([c], np.int8), np.array([1.0], np.float32)))
        scale = [float((grid.d if t == 2 else grid.dd)[c][a0[c]]) for c in range(3)]
        info.update(entries=[1, 1, 1], node=a0)
        return ProbeLists(spec.name, t, 0 if t == 2 else 1, out, scale, info)
    # the types over a cross-section: the normal axis
    flat_axes = [a for a in range(3) if spec.start[a] == spec.stop[a]]
    d = spec.norm_dir if spec.norm_dir is not None else (flat_axes[0] if len(flat_axes) == 1 else None)
    if d is None:
        raise ValueError(f"{who}: its box needs exactly one zero extent, or norm_dir: the normal of its plane is not known")
    if t == 1:
        q = dual_plane(grid, d, 0.5 * (spec.start[d] + spec.stop[d]) * u, tol)
        for a in ((d + 1) % 3, (d + 2) % 3):
            if lo[a] < 1 or hi[a] > n[a] - 2:
                raise ValueError(f"{who}: its cross-section touches a grid face along {AX[a]}: the loop needs a cell on every side of it")
        idx, comp, w = current_loop(grid, lo, hi, d, q)
        info.update(entries=[int(idx.size)], normal=AX[d], dual_plane=q, lo=lo, hi=hi)
        return ProbeLists(spec.name, t, 1, [Probe(idx, comp, f32(spec.weight * w))], [1.0], info)
    P, PP = (d + 1) % 3, (d + 2) % 3
    for a in (P, PP):
        if hi[a] <= lo[a]:
            raise ValueError(f"{who}: its box has no cross-section along {AX[a]} on this mesh (nodes {lo[a]}..{hi[a]})")
    s = a0[d]
    if t == 11 and (s < 1 or s > n[d] - 2):
        raise ValueError(f"{who}: its plane (node {s} along {AX[d]}) lies on a grid face: the current probe needs a half-plane on either side")
    x0, y0, zc = grid.lines[P][lo[P]], grid.lines[PP][lo[PP]], grid.lines[d][s]

    def func(x, y):
        """The mode function in the waveguide port's form: (x, y) metres from the minimum corner -> (c_P, c_PP)."""
        pos = [None, None, None]
        pos[P], pos[PP], pos[d] = (x + x0) / u, (y + y0) / u, np.full(np.shape(x), zc / u)
        one = np.ones(np.shape(x))
        return tuple(one if spec.mode_function[c] is None else np.asarray(spec.mode_function[c](pos[0], pos[1], pos[2]), np.float64) * one for c in (P, PP))
    if t == 10:
        _, v, _ = mode_lists(grid, pec, lo, hi, d, who, e_func=func, s_prb=s, dtype=np.float64)
        pl, kind = v, 0
    else:
        _, _, i = mode_lists(grid, pec, lo, hi, d, who, h_func=func, s_prb=s, d=1, dtype=np.float64)
        pl, kind = i, 1
    info.update(entries=[int(pl.idx.size)], normal=AX[d], plane=s, lo=lo, hi=hi)
    return ProbeLists(spec.name, t, kind, [Probe(pl.idx, pl.comp, f32(spec.weight * pl.w))], [1.0], info)
