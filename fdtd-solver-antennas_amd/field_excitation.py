"""Field excitations: E- and H-field sources over a box, a plane, a line or a point — plain data and the numpy specification of
their lists, in the role ports.py has for ports.

    type 0  soft E   V_e += amp_e sig[n - d]          one fdtd_add_source list
    type 1  hard E   V_e  = amp_e sig[n - d]          the same list on edges whose operator entries vv and vi are zero (the overrides
                                                      the lumped elements use): the fused source leaves amp sig while the pulse lasts,
                                                      0 before and after
    type 2  soft H   I_f += amp_f sigH[n - d]         the soft list of fdtd_excite_set (include/fdtd_hip_excite.h, csrc/excite.hip)
    type 3  hard H   I_f  = amp_f sigH[n - d]         its hard list; sigH[m] = s((m + 1/2) dt)

Which elements a box catches (start, stop in drawing units, closed, within the scene's tolerance): an E edge of component c whose
midpoint — node coordinates, the midpoint along c — lies in the box; an H face of component c whose centre — the node coordinate
along c, midpoints along the two other axes — lies in it.  Only components with exc_val[c] != 0 are used.  A box that catches
nothing is refused with the nearest mesh lines.  Where boxes overlap, the higher priority owns the element; with equal priority and
the same type both act, in scene order (an element of a hard list is then refused: it can be set once).

    amp = exc_val[c] * weight_c(x, y, z) * l       float64, rounded to float32; l the primal edge length (E types), the dual edge
                                                    length of the face's component (H types); x, y, z in DRAWING units, as upstream
    delay [s] -> round(delay / dt) timesteps

weight: None, one callable (x, y, z) -> value for every component, or three per-component entries, each a vectorised callable or a
string.  Strings go through `compile_weight`, a whitelist evaluator on the ast of the expression (never eval or exec): the variables
x y z rho a r t (rho = sqrt(x^2 + y^2), a = atan2(y, x), r = sqrt(x^2 + y^2 + z^2), t = atan2(rho, z): upstream's cylindrical
and spherical coordinates of a Cartesian point), numbers, + - * /, ^ as power, unary minus, comparisons (0 / 1), & and |,
the functions of FUNCTIONS and if(c, a, b), the constants pi and e.

Refused (check_placement), each with the excitation and the node: a hard E edge in metal (soft lists drop metal edges and count
them), an H face on a grid face, an H face that is a magnetic, conformal or plane-wave face (k_magnetic and k_conformal restart from
an i_prev of their own), a hard E edge shared with a lumped port's source or resistor edge, a lumped element, a sheet, a Debye, a
Lorentz or a plane-wave edge, any element inside a CPML layer, and any H type on a decomposed run.

Out of scope: other signal shapes than the run's Gauss pulse, excitations on curves or primitives other than boxes, H types inside
the one-launch or resident schedules and on decomposed grids.
"""
from __future__ import annotations

import ast
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple
import numpy as np

from .grid import RectGrid

AX = "xyz"
TYPES = {0: "soft E", 1: "hard E", 2: "soft H", 3: "hard H"}


# ---- the weight evaluator --------------------------------------------------------------------------------------------------------
def _if(c, a, b):
    return np.where(np.asarray(c) != 0, a, b)


FUNCTIONS = {"sin": np.sin, "cos": np.cos, "tan": np.tan, "asin": np.arcsin, "acos": np.arccos, "atan": np.arctan, "atan2": np.arctan2,
             "sinh": np.sinh, "cosh": np.cosh, "tanh": np.tanh, "exp": np.exp, "log": np.log, "log10": np.log10, "sqrt": np.sqrt,
             "abs": np.abs, "min": np.minimum, "max": np.maximum, "floor": np.floor, "ceil": np.ceil, "pow": np.power, "if": _if}
NARGS = {"atan2": 2, "min": 2, "max": 2, "pow": 2, "if": 3}
CONSTANTS = {"pi": float(np.pi), "e": float(np.e)}
VARIABLES = ("x", "y", "z", "rho", "a", "r", "t")
_BIN = {ast.Add: np.add, ast.Sub: np.subtract, ast.Mult: np.multiply, ast.Div: np.divide, ast.Pow: np.power}
_CMP = {ast.Lt: np.less, ast.LtE: np.less_equal, ast.Gt: np.greater, ast.GtE: np.greater_equal, ast.Eq: np.equal, ast.NotEq: np.not_equal}


def _token(expr: str, node) -> str:
    seg = ast.get_source_segment(expr, node)
    return seg if seg else type(node).__name__


def _check(expr: str, node, who: str) -> None:
    """Walk the tree once, refusing the first node outside the whitelist by its source text."""
    bad = lambda what: ValueError(f"{who}: weight function {expr!r}: {what} {_token(expr, node)!r} is not allowed")
    if isinstance(node, ast.Expression):
        return _check(expr, node.body, who)
    if isinstance(node, ast.Constant):
        if isinstance(node.value, bool) or not isinstance(node.value, (int, float)):
            raise bad("the literal")
        return
    if isinstance(node, ast.Name):
        if node.id not in VARIABLES and node.id not in CONSTANTS:
            raise bad("the name")
        return
    if isinstance(node, ast.UnaryOp):
        if not isinstance(node.op, (ast.USub, ast.UAdd)):
            raise bad("the operator in")
        return _check(expr, node.operand, who)
    if isinstance(node, ast.BinOp):
        if type(node.op) not in _BIN:
            raise bad("the operator in")
        _check(expr, node.left, who)
        return _check(expr, node.right, who)
    if isinstance(node, ast.BoolOp):             # (& and | arrive as `and` / `or`: _prepare)
        for q in node.values:
            _check(expr, q, who)
        return
    if isinstance(node, ast.Compare):
        if any(type(op) not in _CMP for op in node.ops):
            raise bad("the comparison")
        for q in [node.left] + list(node.comparators):
            _check(expr, q, who)
        return
    if isinstance(node, ast.Call):
        if not isinstance(node.func, ast.Name) or node.func.id not in FUNCTIONS or node.keywords:
            raise bad("the call")
        if len(node.args) != NARGS.get(node.func.id, 1):
            raise ValueError(f"{who}: weight function {expr!r}: {node.func.id} takes {NARGS.get(node.func.id, 1)} argument(s), got {len(node.args)}")
        for q in node.args:
            _check(expr, q, who)
        return
    kind = {ast.Attribute: "attribute access", ast.Subscript: "the subscript", ast.Lambda: "the lambda",
            ast.IfExp: "the conditional (use if(c, a, b))"}.get(type(node), "the construct")
    raise bad(kind)


def _eval(node, env):
    if isinstance(node, ast.Constant):
        return float(node.value)
    if isinstance(node, ast.Name):
        return env[node.id]
    if isinstance(node, ast.UnaryOp):
        v = _eval(node.operand, env)
        return np.negative(v) if isinstance(node.op, ast.USub) else v
    if isinstance(node, ast.BinOp):
        return _BIN[type(node.op)](_eval(node.left, env), _eval(node.right, env))
    if isinstance(node, ast.BoolOp):
        vals = [np.asarray(_eval(q, env)) != 0 for q in node.values]
        out = vals[0]
        for v in vals[1:]:
            out = (out & v) if isinstance(node.op, ast.And) else (out | v)
        return np.asarray(out).astype(np.float64)
    if isinstance(node, ast.Compare):
        out, l = None, _eval(node.left, env)
        for op, q in zip(node.ops, node.comparators):
            r = _eval(q, env)
            c = _CMP[type(op)](l, r)
            out, l = c if out is None else (out & c), r
        return np.asarray(out).astype(np.float64)
    return FUNCTIONS[node.func.id](*[_eval(q, env) for q in node.args])      # ast.Call: nothing else passed _check


def _prepare(expr: str) -> str:
    """Upstream's spellings in Python's grammar, with upstream's precedences: ^ becomes ** (Python's ^ binds more loosely than * and
    +), & and | (also && and ||) become `and` and `or` (Python's & and | bind more tightly than the comparisons), if( ... ) becomes a
    call of a plain name."""
    out, i = [], 0
    s = expr.replace("&&", "&").replace("||", "|").replace("^", "**").replace("&", " and ").replace("|", " or ")
    while i < len(s):
        if s.startswith("if", i) and (i == 0 or not (s[i - 1].isalnum() or s[i - 1] == "_")) and s[i + 2:].lstrip().startswith("("):
            out.append("if_")
            i += 2
        else:
            out.append(s[i])
            i += 1
    return "".join(out)


def compile_weight(expr: str, who: str = "field excitation") -> Callable:
    """(x, y, z) -> float64 array for a weight string; ValueError naming the offending token for anything outside the whitelist."""
    if not isinstance(expr, str) or not expr.strip():
        raise ValueError(f"{who}: a weight function must be a non-empty string or a callable, got {expr!r}")
    src = _prepare(expr.strip())
    try:
        tree = ast.parse(src, mode="eval")
    except SyntaxError as err:
        raise ValueError(f"{who}: weight function {expr!r}: cannot be read ({err.msg} at {str(err.text or '').strip()!r})") from None
    for n in ast.walk(tree):                 # (if_ is the spelling of `if` that Python's grammar takes)
        if isinstance(n, ast.Name) and n.id == "if_":
            n.id = "if"
        elif isinstance(n, ast.Name) and n.id == "if":
            raise ValueError(f"{who}: weight function {expr!r}: the name 'if' is not allowed")
    _check(src, tree, who)

    def f(x, y, z):
        x, y, z = (np.asarray(v, np.float64) for v in (x, y, z))
        rho = np.sqrt(x * x + y * y)
        with np.errstate(all="ignore"):
            env = {"x": x, "y": y, "z": z, "rho": rho, "a": np.arctan2(y, x), "r": np.sqrt(x * x + y * y + z * z), "t": np.arctan2(rho, z), **CONSTANTS}
            return np.asarray(_eval(tree.body, env), np.float64) * np.ones(np.broadcast(x, y, z).shape)
    f.expression = expr
    return f


def parse_weight(weight, who: str) -> List[Optional[Callable]]:
    """Three per-component callables (None: weight 1) from None, one callable, or three entries (callable, string or None)."""
    if weight is None:
        return [None, None, None]
    if callable(weight):
        return [weight] * 3
    if isinstance(weight, str):
        raise ValueError(f"{who}: weight must be None, one callable or three per-component entries; a single string is ambiguous — give three")
    w = list(weight)
    if len(w) != 3:
        raise ValueError(f"{who}: weight needs three per-component entries, got {len(w)}")
    out = []
    for c, q in enumerate(w):
        if q is None or callable(q):
            out.append(q)
        elif isinstance(q, str):
            out.append(compile_weight(q, f"{who} (component {AX[c]})"))
        else:
            raise ValueError(f"{who}: weight entry {c} must be a callable or a string, got {q!r}")
    return out


# ---- plain data ------------------------------------------------------------------------------------------------------------------
@dataclass
class FieldExcitation:
    """add_field_excitation(name, exc_type, exc_val, start, stop, weight, delay, priority) as plain data."""
    name: str
    exc_type: int
    exc_val: Tuple[float, float, float]
    start: Tuple[float, float, float]
    stop: Tuple[float, float, float]
    weight: List[Optional[Callable]] = field(default_factory=lambda: [None, None, None])
    delay: float = 0.0
    priority: int = 0


def make(name, exc_type, exc_val, start, stop, weight=None, delay=0.0, priority=0) -> FieldExcitation:
    who = f"field excitation '{name}'"
    if isinstance(exc_type, bool) or exc_type not in TYPES:
        raise ValueError(f"{who}: exc_type must be 0 (soft E), 1 (hard E), 2 (soft H) or 3 (hard H), got {exc_type!r}")
    v = np.asarray(exc_val, float).reshape(-1)
    if v.size != 3 or not np.all(np.isfinite(v)) or not np.any(v != 0):
        raise ValueError(f"{who}: exc_val must be three finite values, at least one of them not zero, got {exc_val!r}")
    if len(start) != 3 or len(stop) != 3 or not np.all(np.isfinite(np.asarray(list(start) + list(stop), float))):
        raise ValueError(f"{who}: start and stop must be three finite coordinates each")
    if not (np.ndim(delay) == 0 and np.isfinite(float(delay)) and float(delay) >= 0):
        raise ValueError(f"{who}: delay = {delay!r} must be one finite value >= 0 [s]")
    return FieldExcitation(str(name), int(exc_type), tuple(map(float, v)), tuple(map(float, start)), tuple(map(float, stop)),
                           parse_weight(weight, who), float(delay), int(priority))


@dataclass
class ExcitationLists:
    """What the excitations of a scene are on the grid.  soft_e, hard_e, soft_h, hard_h: (idx int64, comp int8, amp float32, delay
    int32, owner int32 — the position of the excitation in the scene); dropped: metal edges left out per excitation; info: per
    excitation what fdtd_hip_run.json reports."""
    soft_e: tuple
    hard_e: tuple
    soft_h: tuple
    hard_h: tuple
    dropped: List[int]
    info: List[dict]

    def h_args(self, sigH):
        """The arguments of Engine.set_excite."""
        return (*self.hard_h[:4], *self.soft_h[:4], sigH)

    def any_h(self) -> bool:
        return bool(self.soft_h[0].size or self.hard_h[0].size)


def signal_h(f0: float, fc: float, dt: float, nsig: int) -> np.ndarray:
    """The run's pulse at the times the face currents live: float32 [nsig], sigH[m] = s((m + 1/2) dt) — the odd samples of
    planewave.signal2."""
    from .excitation import gauss_pulse
    return np.ascontiguousarray(gauss_pulse(f0, fc, 0.5 * dt, 2 * int(nsig))[1::2])


def _empty():
    return (np.zeros(0, np.int64), np.zeros(0, np.int8), np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32))


def _nearest(grid: RectGrid, ex: FieldExcitation, u: float) -> str:
    parts = []
    for a in range(3):
        lo, hi = sorted((ex.start[a] * u, ex.stop[a] * u))
        parts.append(f"{AX[a]}: [{lo / u:g}, {hi / u:g}] — nearest lines {grid.lines[a][grid.snap(a, lo)] / u:g} and {grid.lines[a][grid.snap(a, hi)] / u:g}")
    return "; ".join(parts)


def caught(grid: RectGrid, ex: FieldExcitation, u: float, tol: float, comp: int):
    """(i, j, k) index arrays of the elements of component `comp` the box of `ex` catches."""
    faces = ex.exc_type >= 2
    sel = []
    for a in range(3):
        lo, hi = sorted((ex.start[a] * u, ex.stop[a] * u))
        mid = (a == comp) != faces           # an edge: midpoint along its own axis; a face: midpoints along the two others
        pos = grid.centers(a) if mid else grid.lines[a]
        sel.append(np.nonzero((pos >= lo - tol) & (pos <= hi + tol))[0])
    K, J, I = np.meshgrid(sel[2], sel[1], sel[0], indexing="ij")
    return I.reshape(-1), J.reshape(-1), K.reshape(-1)


def lists(grid: RectGrid, excitations: Sequence[FieldExcitation], u: float, dt: float, pec: np.ndarray, tol: float) -> ExcitationLists:
    """The four lists of a scene's excitations.  pec: bool [3][nz][ny][nx]."""
    nx, ny, nz = grid.shape
    raw = []                                 # per excitation and component: (q, c, idx, amp)
    dropped = [0] * len(excitations)
    for q, ex in enumerate(excitations):
        who = f"field excitation '{ex.name}'"
        faces = ex.exc_type >= 2
        n_all = 0
        for c in range(3):
            if ex.exc_val[c] == 0:
                continue
            i, j, k = caught(grid, ex, u, tol, c)
            n_all += i.size
            if i.size == 0:
                continue
            pos = [grid.lines[0][i], grid.lines[1][j], grid.lines[2][k]]
            ijk = (i, j, k)
            for a in range(3):
                if (a == c) != faces:
                    pos[a] = grid.centers(a)[ijk[a]]
            w = np.ones(i.size) if ex.weight[c] is None else np.asarray(ex.weight[c](pos[0] / u, pos[1] / u, pos[2] / u), np.float64) * np.ones(i.size)
            if not np.all(np.isfinite(w)):
                b = int(np.nonzero(~np.isfinite(w))[0][0])
                raise ValueError(f"{who}: its weight function is not finite at ({pos[0][b] / u:g}, {pos[1][b] / u:g}, {pos[2][b] / u:g}) "
                                 f"(component {AX[c]}, node ({i[b]}, {j[b]}, {k[b]}))")
            ln = (grid.dd if faces else grid.d)[c][ijk[c]]
            amp = ex.exc_val[c] * w * ln
            idx = grid.flat(i, j, k)
            if not faces:
                metal = pec[c].reshape(-1)[idx]
                if ex.exc_type == 1 and metal.any():
                    b = int(np.nonzero(metal)[0][0])
                    raise ValueError(f"{who}: its hard {AX[c]} edge at node ({i[b]}, {j[b]}, {k[b]}) lies in metal (PEC): a hard source on a metal edge "
                                     f"would replace the conductor — end the box at the metal")
                dropped[q] += int(metal.sum())
                idx, amp = idx[~metal], amp[~metal]
            raw.append((q, c, idx, amp))
        if n_all == 0:
            raise ValueError(f"{who}: its box catches no {'face' if faces else 'edge'} of this mesh ({_nearest(grid, ex, u)})")
    # priority: the highest priority that lists an element owns it, per family (E edges, H faces)
    prio = {}
    for q, c, idx, amp in raw:
        fam = excitations[q].exc_type >= 2
        for g in (idx * 3 + c).tolist():
            key = (fam, g)
            if key not in prio or excitations[q].priority > prio[key]:
                prio[key] = excitations[q].priority
    out = {t: [[], [], [], [], []] for t in TYPES}
    counts = [0] * len(excitations)
    for q, c, idx, amp in raw:
        ex = excitations[q]
        fam = ex.exc_type >= 2
        keep = np.array([prio[(fam, g)] == ex.priority for g in (idx * 3 + c).tolist()], bool) if idx.size else np.zeros(0, bool)
        n = int(keep.sum())
        counts[q] += n
        o = out[ex.exc_type]
        o[0].append(idx[keep]); o[1].append(np.full(n, c, np.int8)); o[2].append(amp[keep].astype(np.float32))
        o[3].append(np.full(n, int(round(ex.delay / dt)), np.int32)); o[4].append(np.full(n, q, np.int32))
    cat = lambda o: tuple(np.concatenate(a).astype(d) if a else e for a, d, e in zip(o, (np.int64, np.int8, np.float32, np.int32, np.int32), _empty()))
    res = {t: cat(out[t]) for t in TYPES}
    # an element with equal priority under a soft and a hard list, or twice under a hard list: it can be set once
    for fam, (soft, hard) in enumerate(((res[0], res[1]), (res[2], res[3]))):
        hk = hard[0] * 3 + hard[1]
        uq, first, cnt = np.unique(hk, return_index=True, return_counts=True)
        clash = None
        if np.any(cnt > 1):
            b = uq[cnt > 1][0]
            e = np.nonzero(hk == b)[0]
            clash = (int(e[0]), int(hard[4][e[0]]), int(hard[4][e[1]]))
        else:
            both = np.nonzero(np.isin(soft[0] * 3 + soft[1], hk))[0]
            if both.size:
                e = int(np.nonzero(hk == (soft[0] * 3 + soft[1])[both[0]])[0][0])
                clash = (e, int(hard[4][e]), int(soft[4][both[0]]))
        if clash is not None:
            e, qa, qb = clash
            g, c = int(hard[0][e]), int(hard[1][e])
            raise ValueError(f"field excitation '{excitations[qa].name}': its hard {AX[c]} {'face' if fam else 'edge'} at node "
                             f"({g % nx}, {g // nx % ny}, {g // (nx * ny)}) is also excited by '{excitations[qb].name}' with the same priority: "
                             f"a hard element is set by one excitation — give one of them the higher priority")
    info = [{"name": ex.name, "type": ex.exc_type, "kind": TYPES[ex.exc_type], ("faces" if ex.exc_type >= 2 else "edges"): counts[q],
             "dropped_metal_edges": dropped[q], "delay_steps": int(round(ex.delay / dt)), "priority": ex.priority}
            for q, ex in enumerate(excitations)]
    return ExcitationLists(res[0], res[1], res[2], res[3], dropped, info)


# ---- placement -------------------------------------------------------------------------------------------------------------------
def _ijk(g: int, shape):
    nx, ny, _ = shape
    return g % nx, g // nx % ny, g // (nx * ny)


def check_placement(grid: RectGrid, excitations: Sequence[FieldExcitation], ls: ExcitationLists, *, cpml_cells: Sequence[int] = (0,) * 6,
                    magnetic_classes=None, conformal=None, plane_wave_elems=None, ports=(), elements=None, sheets=None, debye=None,
                    lorentz=None, world: int = 1) -> None:
    """Refuse (ValueError, naming the excitation and the node) what the lists cannot serve; the rules are the module's docstring.
    magnetic_classes: uint8 [3][nz][ny][nx] (magnetic.MagneticFaces.full_classes); conformal: an object with idx, comp;
    plane_wave_elems: (edge keys, face keys) as 3 * idx + comp; ports: scene.PortOnGrid; elements / sheets: objects with idx, comp;
    debye / lorentz: objects with lo, hi, w per component."""
    n = grid.shape
    nx, ny, nz = n
    name = lambda q: f"field excitation '{excitations[int(q)].name}'"

    def first(l, mask):
        e = int(np.nonzero(mask)[0][0])
        return int(l[4][e]), int(l[1][e]), _ijk(int(l[0][e]), n)

    if world > 1 and ls.any_h():
        l = ls.hard_h if ls.hard_h[0].size else ls.soft_h
        raise ValueError(f"{name(l[4][0])}: H-field excitations need a single slab (world = 1): a decomposed run with an H-type excitation is not supported")
    for l, faces in ((ls.soft_e, False), (ls.hard_e, False), (ls.soft_h, True), (ls.hard_h, True)):
        if not l[0].size:
            continue
        pos = np.stack(_ijk(l[0], n))                      # [3][entries]
        what = "face" if faces else "edge"
        # inside a CPML layer: the planes that carry psi (node and cell indices 0 .. cells - 1 and n - 1 - cells .. n - 1, cpml.py)
        for a in range(3):
            for side, cells in ((0, cpml_cells[2 * a]), (1, cpml_cells[2 * a + 1])):
                if not cells:
                    continue
                bad = (pos[a] < cells) if side == 0 else (pos[a] >= n[a] - 1 - cells)
                if bad.any():
                    q, c, p = first(l, bad)
                    raise ValueError(f"{name(q)}: its {AX[c]} {what} at node {p} lies inside the CPML layer {AX[a]}{'+' if side else '-'} ({cells} cells): "
                                     f"excitations inside absorbing layers are not supported — end the box before the layer")
        if faces:
            bad = np.zeros(l[0].size, bool)
            for a in range(3):
                on = np.array([a == c for c in l[1]])
                bad |= on & ((pos[a] == 0) | (pos[a] == n[a] - 1))
            if bad.any():
                q, c, p = first(l, bad)
                raise ValueError(f"{name(q)}: its {AX[c]} face at node {p} lies on a grid face: the face current there belongs to the boundary")
            key = l[0] * 3 + l[1]
            owners = []
            if magnetic_classes is not None:
                owners.append(("a magnetic face", magnetic_classes.reshape(3, -1)[l[1].astype(np.int64), l[0]] != 0))
            if conformal is not None and len(conformal.idx):
                owners.append(("a conformal (cut) face", np.isin(key, np.asarray(conformal.idx, np.int64) * 3 + np.asarray(conformal.comp, np.int64))))
            if plane_wave_elems is not None:
                owners.append(("a face of the plane wave's list", np.isin(key, plane_wave_elems[1])))
            for owner, bad in owners:
                if bad.any():
                    q, c, p = first(l, bad)
                    raise ValueError(f"{name(q)}: its {AX[c]} face at node {p} is {owner}: that correction restarts from its own output and would "
                                     f"lose the excitation — keep the box off it")
    l = ls.hard_e
    if l[0].size:
        key = l[0] * 3 + l[1]
        owners = []
        for p in ports:
            from .ports import label
            pk = [np.asarray(p.src_idx, np.int64) * 3 + np.asarray(p.src_comp, np.int64)]
            pk += [np.array([grid.flat(le.i, le.j, le.k) * 3 + le.comp for le in p.lumped], np.int64).reshape(-1)]
            owners.append((f"a source or resistor edge of {label(p.port)}", np.isin(key, np.concatenate(pk))))
        for what, obj in (("an edge of a lumped element", elements), ("a conducting-sheet edge", sheets)):
            if obj is not None and len(obj.idx):
                owners.append((what, np.isin(key, np.asarray(obj.idx, np.int64) * 3 + np.asarray(obj.comp, np.int64))))
        for what, obj in (("a Debye edge", debye), ("a Lorentz edge", lorentz)):
            if obj is not None:
                full = np.zeros((3, nz, ny, nx), bool)
                for c in range(3):
                    if obj.w[c].size:
                        (i0, j0, k0), (i1, j1, k1) = obj.lo[c], obj.hi[c]
                        full[c, k0:k1, j0:j1, i0:i1] = obj.w[c] != 0
                owners.append((what, full.reshape(3, -1)[l[1].astype(np.int64), l[0]]))
        if plane_wave_elems is not None:
            owners.append(("an edge of the plane wave's list", np.isin(key, plane_wave_elems[0])))
        for owner, bad in owners:
            if bad.any():
                q, c, p = first(l, bad)
                raise ValueError(f"{name(q)}: its hard {AX[c]} edge at node {p} is {owner}: a hard source zeroes the edge's operator entries, "
                                 f"which that owner needs — keep the box off it")
