"""Plane-wave excitation on a total-field / scattered-field box (openEMS users know it as ``CSX.AddExcitation(name, 10, E0)`` with
``SetPropagationDir``).

Model.  A box of whole nodes lo..hi (inclusive on every axis).  Inside the box and on its surface the grid holds the TOTAL field,
outside it the SCATTERED field; the incident field is analytic,

    E_inc(r, t) = E0 s(t - k.(r - r0)/c0),      H_inc = k x E_inc / Z0,      |k| = 1, E0 perpendicular to k,

with s the run's excitation pulse.  The update kernels know nothing of this: across the box surface they difference a total against
a scattered quantity.  Two sparse corrections per timestep add what each such difference missed (include/fdtd_hip_planewave.h,
csrc/planewave.hip; ``apply`` below restates them in numpy, operation for operation):

    E list  after the E phase of step n: every total-field edge whose update read a scattered-field current — the tangential edges
            on the six box faces — takes  +-vi_e I_inc  of the outer face it read, I_inc = H_inc l~ at the face centre, at time
            (n - 1/2) dt;
    H list  after the H update of step n: every scattered-field face just outside the box whose update read a total-field voltage
            takes  -+iv_f V_inc  of that surface edge, V_inc = E_inc l at the edge midpoint, at time n dt.

The signs are those of the differences in update_E / update_H of oracle/fdtd_oracle.c (component n, a1 = n + 1, a2 = n + 2 mod 3):

    V_n(p) += vi ((I_a2(p) - I_a2(p - e_a1)) - (I_a1(p) - I_a1(p - e_a2)))
    I_n(p) += iv ((V_a2(p) - V_a2(p + e_a1)) - (V_a1(p) - V_a1(p + e_a2)))

An edge on a box EDGE reads two outer faces, one from each of the two box faces that meet there: its two terms are merged into one
entry, so no element appears twice in a launch.  An entry whose second term is absent carries coefficient 0 there.

Time.  V after the E phase of step n is at n dt, I after the H update of step n at (n + 1/2) dt, and a soft source adds sig[n] at
step n (excitation.dft_twiddles, post_E of the oracle).  The plane wave reads the same pulse tabulated at HALF-step resolution,
sig2[m] = s(m dt/2) in float64 rounded to float32 — sig2[2 n] is bit for bit what a port gets at step n — so port-driven and
wave-driven runs of one scene share a time axis and a spectrum.  Per term the delay in half-steps D = k.(r - r0)/(c0 dt/2) is split
into m0 = floor(D) and w = D - m0 (float32), and the pulse is interpolated linearly at p = base - m0 (base = 2 n for the H list,
2 n - 1 for the E list), zero outside the table.

r0.  The corner, of the box WIDENED BY ONE CELL on every side, that the wave reaches first: the H list's incident edges lie on the
box, but the E list's incident faces are centred half a cell outside it, and with the plain box corner the first of them would need
a negative delay.  Every delay is >= 0 this way, and the incident field at r0 is s(t) itself.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence, Tuple
import numpy as np

from .constants import C0, ETA0
from .grid import RectGrid
from .excitation import gauss_pulse

MIN_CELLS = 2        # cells the box holds per axis at least
CLEARANCE = 2        # cells between the box and a CPML layer, a Mur face or a PMC wall (and any grid face)


@dataclass
class PlaneWave:
    """One plane wave: e0 [V/m] (projected perpendicular to the direction), the propagation direction (normalised) and its box in
    whole nodes, inclusive."""
    name: str
    e0: Sequence[float]
    direction: Sequence[float]
    lo: Tuple[int, int, int] = (0, 0, 0)
    hi: Tuple[int, int, int] = (0, 0, 0)

    def __post_init__(self):
        k = np.asarray(self.direction, np.float64).reshape(-1)
        e = np.asarray(self.e0, np.float64).reshape(-1)
        if k.size != 3 or e.size != 3 or not (np.all(np.isfinite(k)) and np.all(np.isfinite(e))):
            raise ValueError(f"plane wave '{self.name}': e0 and the propagation direction must be three finite values each")
        if not np.linalg.norm(k) > 0:
            raise ValueError(f"plane wave '{self.name}': the propagation direction is zero")
        if not np.linalg.norm(e) > 0:
            raise ValueError(f"plane wave '{self.name}': e0 is zero")
        k = k / np.linalg.norm(k)
        ep = e - k * float(e @ k)
        if np.linalg.norm(ep) <= 1e-9 * np.linalg.norm(e):
            raise ValueError(f"plane wave '{self.name}': the polarisation e0 = {tuple(e)} is parallel to the propagation direction "
                             f"{tuple(k)}: a plane wave is transverse")
        self.direction, self.e0 = k, ep
        self.lo, self.hi = tuple(int(v) for v in self.lo), tuple(int(v) for v in self.hi)

    @property
    def h0(self) -> np.ndarray:
        """H0 = k x E0 / Z0 [A/m]."""
        return np.cross(self.direction, self.e0) / ETA0

    def r0(self, grid: RectGrid) -> np.ndarray:
        """The corner of the box widened by one cell that the wave reaches first (the module text)."""
        return np.array([grid.lines[a][self.lo[a] - 1] if self.direction[a] >= 0 else grid.lines[a][self.hi[a] + 1] for a in range(3)])

    def far_delay(self, grid: RectGrid) -> float:
        """Seconds the front needs from r0 to the opposite corner of the widened box."""
        far = np.array([grid.lines[a][self.hi[a] + 1] if self.direction[a] >= 0 else grid.lines[a][self.lo[a] - 1] for a in range(3)])
        return float(self.direction @ (far - self.r0(grid)) / C0)


def signal2(f0: float, fc: float, dt: float, nsig: int) -> np.ndarray:
    """The pulse of a run whose port signal has nsig samples, at half-step resolution: float32 [2 nsig], sig2[2 n] == signal[n]."""
    return gauss_pulse(f0, fc, 0.5 * dt, 2 * int(nsig))


def incident_spectrum(freqs, sig2: np.ndarray, dt: float) -> np.ndarray:
    """s^(f) of the incident pulse at r0, single-sided and scaled by 2 dt like CalcPort and Simulation.nf2ff_boxes:
    2 dt sum_n sig2[2 n] exp(-j 2 pi f n dt).  E_inc^(f) at r is E0 s^(f) exp(-j 2 pi f k.(r - r0)/c0)."""
    f = np.atleast_1d(np.asarray(freqs, np.float64))
    s = np.asarray(sig2, np.float64)[::2]
    t = np.arange(s.size) * dt
    return 2.0 * dt * (np.exp(-2j * np.pi * np.outer(f, t)) @ s)


# ---- which elements, which terms ---------------------------------------------------------------------------------------------
def _box_mask(shape, lo, hi):
    """bool [nz][ny][nx], True for lo[a] <= index[a] <= hi[a]."""
    m = np.zeros(shape[::-1], bool)
    if all(hi[a] >= lo[a] for a in range(3)):
        m[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    return m


def total_masks(shape, lo, hi):
    """(totE, totH): per component the elements that hold the total field.  An edge of direction c spans the nodes p, p + e_c: total
    when both lie in the box; a face of normal c spans one cell along both other axes: total when its four nodes lie in the box."""
    totE, totH = [], []
    for c in range(3):
        h = list(hi); h[c] -= 1
        totE.append(_box_mask(shape, lo, h))
        h = [v - 1 for v in hi]; h[c] = hi[c]
        totH.append(_box_mask(shape, lo, h))
    return totE, totH


def _reads(n: int):
    """The four reads of the update of component n, E and H alike: (component read, axis of the shift or None, sign in the difference);
    the shift is -1 along the axis for the E update, +1 for the H update."""
    a1, a2 = (n + 1) % 3, (n + 2) % 3
    return [(a2, None, 1.0), (a2, a1, -1.0), (a1, None, -1.0), (a1, a2, 1.0)]


def _shifted(mask, axis, step):
    """mask at p + step e_axis (the box stays clear of the grid faces, so nothing wraps that matters)."""
    return mask if axis is None else np.roll(mask, -step, axis=2 - axis)


def terms(grid: RectGrid, pw: PlaneWave, phase: int):
    """Every single term of one list, unmerged: (comp, i, j, k of the corrected element; component and i, j, k of the incident
    element it stands for; sign of that read in the update's difference)."""
    totE, totH = total_masks(grid.shape, pw.lo, pw.hi)
    out = []
    for n in range(3):
        for fc, axis, sign in _reads(n):
            step = -1 if phase == 0 else 1
            if phase == 0:      # a total edge that read a scattered face
                hit = totE[n] & ~_shifted(totH[fc], axis, step)
            else:               # a scattered face that read a total edge
                hit = ~totH[n] & _shifted(totE[fc], axis, step)
            k, j, i = np.nonzero(hit)
            q = [i.copy(), j.copy(), k.copy()]
            if axis is not None:
                q[axis] += step
            for t in range(i.size):
                out.append((n, int(i[t]), int(j[t]), int(k[t]), fc, int(q[0][t]), int(q[1][t]), int(q[2][t]), sign))
    return out


def _position(grid: RectGrid, phase: int, comp: int, ijk) -> np.ndarray:
    """Where the incident element is taken: a face (E list) at its centre — on the node plane along its normal, mid-cell along both
    other axes; an edge (H list) at its midpoint."""
    r = np.empty(3)
    for a in range(3):
        l = grid.lines[a]
        mid = (a != comp) if phase == 0 else (a == comp)
        r[a] = 0.5 * (l[ijk[a]] + l[ijk[a] + 1]) if mid else l[ijk[a]]
    return r


@dataclass
class Tables:
    """What fdtd_planewave_set takes: per list idx int64 [n], comp int8 [n], coef float32 [n][2], m0 int32 [n][2], w float32 [n][2];
    sig2 float32.  coef64 / delay64: the float64 values before rounding / splitting (tests)."""
    E: tuple
    H: tuple
    sig2: np.ndarray
    coef64: tuple = ()
    delay64: tuple = ()

    def args(self):
        return (*self.E, *self.H, self.sig2)


def tables(grid: RectGrid, pw: PlaneWave, dt: float, vi: np.ndarray, iv: np.ndarray, sig2: np.ndarray, dtype=np.float32) -> Tables:
    """The two entry lists.  vi, iv: [3][nz][ny][nx], the operator's own values (Engine.get_operator()[1] and [3]).  dtype: what
    coef, w and sig2 are rounded to (float32: what the engine takes; float64 for a restatement on the double oracle)."""
    nx, ny, _ = grid.shape
    r0, kdir = pw.r0(grid), pw.direction
    amp = (pw.h0, pw.e0)
    lists, c64, d64 = [], [], []
    for phase in (0, 1):
        op = vi if phase == 0 else iv
        by_key = {}
        for n, i, j, k, fc, qi, qj, qk, sign in terms(grid, pw, phase):
            if phase == 0:
                coef = sign * float(op[n][k, j, i]) * amp[0][fc] * grid.dd[fc][(qi, qj, qk)[fc]]
            else:
                coef = -sign * float(op[n][k, j, i]) * amp[1][fc] * grid.d[fc][(qi, qj, qk)[fc]]
            D = float(kdir @ (_position(grid, phase, fc, (qi, qj, qk)) - r0)) / (C0 * 0.5 * dt)
            by_key.setdefault((n, (k * ny + j) * nx + i), []).append((coef, D))
        keys = sorted(by_key)
        n_e = len(keys)
        idx = np.array([g for _, g in keys], np.int64).reshape(n_e)
        comp = np.array([c for c, _ in keys], np.int8).reshape(n_e)
        coef = np.zeros((n_e, 2), np.float64)
        D = np.zeros((n_e, 2), np.float64)
        for e, key in enumerate(keys):
            ts = by_key[key]
            assert len(ts) <= 2, "an element of the box surface takes at most two terms"
            for q, (cf, dl) in enumerate(ts):
                coef[e, q], D[e, q] = cf, dl
        assert np.all(D > -1e-9), "a delay before the wave reaches r0"
        D = np.maximum(D, 0.0)
        m0 = np.floor(D).astype(np.int64)
        w = (D - m0).astype(dtype)
        up = w >= 1.0                # (the fraction rounded up to 1: the next whole half-step)
        m0[up] += 1
        w[up] = 0.0
        lists.append((idx, comp, coef.astype(dtype), m0.astype(np.int32), w))
        c64.append(coef); d64.append(D)
    return Tables(lists[0], lists[1], np.ascontiguousarray(sig2, dtype), tuple(c64), tuple(d64))


def apply(fields, tab: Tables, n: int, phase: int) -> None:
    """The correction of include/fdtd_hip_planewave.h, statement for statement, in the fields' own precision (float32 to restate the
    kernel).  fields: the three voltage arrays (phase 0, after the E phase of step n) or current arrays (phase 1, after the H update
    of step n), [nz][ny][nx] each, changed in place."""
    idx, comp, coef, m0, w = tab.E if phase == 0 else tab.H
    if idx.size == 0:
        return
    ft = fields[0].dtype.type
    sig2 = tab.sig2.astype(fields[0].dtype)
    base = 2 * int(n) - (1 if phase == 0 else 0)

    def sig(p):
        ok = (p >= 0) & (p < sig2.size)
        return np.where(ok, sig2[np.clip(p, 0, sig2.size - 1)], ft(0))

    def term(q):
        p = base - m0[:, q].astype(np.int64)
        hi = sig(p)
        a = sig(p - 1) - hi
        b = w[:, q].astype(hi.dtype) * a
        s = hi + b
        return coef[:, q].astype(hi.dtype) * s
    t0, t1 = term(0), term(1)
    for c in range(3):
        sel = np.nonzero(comp == c)[0]
        if sel.size:
            F = fields[c].reshape(-1)
            g = F[idx[sel]] + t0[sel]
            F[idx[sel]] = g + t1[sel]


def incident_fields(grid: RectGrid, pw: PlaneWave, s, t_v: float, t_i: float):
    """(V [3][nz][ny][nx], I likewise) float64 of the incident wave alone on every edge and face of the grid: s a callable of time,
    V at time t_v, I at t_i (tests: the analytic wave the grid is compared with)."""
    nx, ny, nz = grid.shape
    r0 = pw.r0(grid)
    ext = [np.append(l, 2 * l[-1] - l[-2]) for l in grid.lines]
    node = [l.copy() for l in grid.lines]
    mid = [0.5 * (e[:-1] + e[1:]) for e in ext]
    V, I = np.empty((3, nz, ny, nx)), np.empty((3, nz, ny, nx))
    for c in range(3):
        for phase, out, t, a0, ln in ((1, V, t_v, pw.e0, grid.d), (0, I, t_i, pw.h0, grid.dd)):
            ax = [(mid[a] if ((a != c) if phase == 0 else (a == c)) else node[a]) - r0[a] for a in range(3)]
            tau = (pw.direction[0] * ax[0][None, None, :] + pw.direction[1] * ax[1][None, :, None] + pw.direction[2] * ax[2][:, None, None]) / C0
            shp = [1, 1, 1]; shp[2 - c] = ln[c].size
            out[c] = a0[c] * ln[c].reshape(shp) * s(t - tau)
    return V, I


# ---- placement --------------------------------------------------------------------------------------------------------------
def surface_keys(grid: RectGrid, pw: PlaneWave):
    """(edges, faces): the sets of (comp, flat node index) of the surface edges (the E list's elements: every tangential edge on the
    six box faces) and of the adjacent outer faces (the H list's elements)."""
    nx, ny, _ = grid.shape
    out = []
    for phase in (0, 1):
        out.append({(n, (k * ny + j) * nx + i) for n, i, j, k, *_ in terms(grid, pw, phase)})
    return out[0], out[1]


def check_box(grid: RectGrid, pw: PlaneWave, cpml_cells: Sequence[int] = (0,) * 6, kinds: Sequence[str] = ("PEC",) * 6) -> None:
    """The box itself: cells per axis, clearance to the layers / faces / walls."""
    n = grid.shape
    for a in range(3):
        if pw.hi[a] - pw.lo[a] < MIN_CELLS:
            raise ValueError(f"plane wave '{pw.name}': its box holds {max(pw.hi[a] - pw.lo[a], 0)} cells along {'xyz'[a]} on this mesh "
                             f"(nodes {pw.lo[a]}..{pw.hi[a]}): at least {MIN_CELLS} are needed")
        for side in (0, 1):
            f = 2 * a + side
            room = (pw.lo[a] - cpml_cells[f]) if side == 0 else (n[a] - 1 - cpml_cells[f] - pw.hi[a])
            if room < CLEARANCE:
                what = {"CPML": f"CPML layer ({cpml_cells[f]} cells)", "MUR": "Mur face", "PMC": "PMC wall"}.get(kinds[f], "grid face")
                raise ValueError(f"plane wave '{pw.name}': its box (nodes {pw.lo[a]}..{pw.hi[a]} along {'xyz'[a]}) comes within {max(room, 0)} "
                                 f"cells of the {what} {'xyz'[a]}{'+' if side else '-'}: keep it at least {CLEARANCE} cells clear")


def check_placement(grid: RectGrid, pw: PlaneWave, *, cpml_cells: Sequence[int] = (0,) * 6, kinds: Sequence[str] = ("PEC",) * 6,
                    eps_r=None, kappa=None, mu_r=None, sigma_m=None, pec=None, sheets=None, elements=None, debye=None, lorentz=None,
                    conformal=None, ports=(), dft_boxes=(), sar_boxes=None, field_boxes=None) -> None:
    """Refuse (ValueError) a box the corrections cannot serve: see the rules in DESIGN.  eps_r ... sigma_m: per cell
    [nz-1][ny-1][nx-1]; pec: bool [3][nz][ny][nx]; sheets / elements: objects with idx, comp; debye / lorentz: with cell_medium and
    names; conformal: conformal.ConformalFaces; ports: scene.PortOnGrid; dft_boxes: (kind, comp, lo, hi) of the recording requests;
    sar_boxes: {name: {"lo", "hi"}}; field_boxes: {name: {"rlo", "hi", "kind"}} (the recorded region; kinds H and rotH record faces)."""
    check_box(grid, pw, cpml_cells, kinds)
    nx, ny, nz = grid.shape
    lo, hi = pw.lo, pw.hi
    who = f"plane wave '{pw.name}'"
    # the cells touching the box surface on either side: the shell between the box shrunk and widened by one cell
    shell = np.zeros((nz - 1, ny - 1, nx - 1), bool)
    shell[lo[2] - 1:hi[2] + 1, lo[1] - 1:hi[1] + 1, lo[0] - 1:hi[0] + 1] = True
    shell[lo[2] + 1:hi[2] - 1, lo[1] + 1:hi[1] - 1, lo[0] + 1:hi[0] - 1] = False

    def first(mask):
        k, j, i = (int(v[0]) for v in np.nonzero(mask))
        return f"cell ({i}, {j}, {k})"
    for what, arr, vac in (("eps_r", eps_r, 1.0), ("kappa", kappa, 0.0), ("mu_r", mu_r, 1.0), ("sigma_m", sigma_m, 0.0)):
        if arr is not None and np.any(arr[shell] != vac):
            bad = shell & (arr != vac)
            raise ValueError(f"{who}: {first(bad)} touches the box surface and has {what} = {float(arr[bad][0]):g}: every cell on either "
                             f"side of the surface must be vacuum (a background crossing the box is not supported)")
    for kind, med in (("Debye", debye), ("Lorentz", lorentz)):
        if med is not None and np.any(med.cell_medium[shell] >= 0):
            bad = shell & (med.cell_medium >= 0)
            m = int(med.cell_medium[bad][0])
            raise ValueError(f"{who}: {first(bad)} touches the box surface and belongs to the {kind} medium '{' / '.join(med.names[m])}': every "
                             f"cell on either side of the surface must be vacuum")
    edges, faces = surface_keys(grid, pw)

    def at(key):
        c, g = key
        k, r = divmod(int(g), nx * ny)
        j, i = divmod(r, nx)
        return f"{'xyz'[c]}-directed at node ({i}, {j}, {k})"

    def hit(keys, comp, idx):
        for c, g in zip(np.asarray(comp).reshape(-1), np.asarray(idx).reshape(-1)):
            if (int(c), int(g)) in keys:
                return (int(c), int(g))
        return None
    if pec is not None:
        for c, g in sorted(edges):
            if pec[c].reshape(-1)[g]:
                raise ValueError(f"{who}: the surface edge {at((c, g))} is metal (PEC): metal may lie inside the box or outside it, not on its surface")
    for what, lst in (("a conducting-sheet edge", sheets), ("a lumped-element edge", elements)):
        if lst is not None and len(lst):
            k = hit(edges, lst.comp, lst.idx)
            if k:
                raise ValueError(f"{who}: the surface edge {at(k)} is {what}: keep it off the box surface")
    if conformal is not None:
        k = hit(edges, conformal.frac.comp, conformal.frac.idx)
        if k:
            raise ValueError(f"{who}: the surface edge {at(k)} is cut by a conformal metal surface: keep curved metal off the box surface")
        k = hit(faces, conformal.comp, conformal.idx)
        if k:
            raise ValueError(f"{who}: the outer face {at(k)} next to the box is a conformal (cut) face: keep curved metal off the box surface")
    for p in ports:
        nr = p.port.number
        kind = {"waveguide": "waveguide", "msl": "MSL"}.get(getattr(p.port, "kind", None), "lumped")
        k = hit(edges, [le.comp for le in p.lumped], [(le.k * ny + le.j) * nx + le.i for le in p.lumped]) or hit(edges, p.src_comp, p.src_idx)
        if k:
            raise ValueError(f"{who}: the surface edge {at(k)} is an edge of {kind} port {nr}: a port lies inside the box (receive mode) or outside it")
        k = hit(edges, p.v_comp, p.v_idx) or hit(faces, p.i_comp, p.i_idx)
        if k:
            raise ValueError(f"{who}: the {'surface edge' if k in edges else 'outer face'} {at(k)} is sampled by a probe of {kind} port {nr}: probes "
                             f"sample before the corrections and would read a mixed field")
    for kind, comp, blo, bhi in dft_boxes:
        for c, g in sorted(edges if kind == 0 else faces):
            if c != comp:
                continue
            k, r = divmod(g, nx * ny)
            j, i = divmod(r, nx)
            if all(blo[a] <= v <= bhi[a] for a, v in enumerate((i, j, k))):
                raise ValueError(f"{who}: the NF2FF box records the {'surface edge' if kind == 0 else 'outer face'} {at((c, g))}: it would hold a mixed "
                                 f"field — keep the NF2FF box strictly outside the plane-wave box (scattered field: RCS) or strictly inside (total field)")
    for name, b in (sar_boxes or {}).items():
        for c, g in sorted(edges):
            k, r = divmod(g, nx * ny)
            j, i = divmod(r, nx)
            if all(b["lo"][a] <= v <= b["hi"][a] for a, v in enumerate((i, j, k))):
                raise ValueError(f"{who}: SAR box '{name}' records the surface edge {at((c, g))}: it would hold a mixed field — keep it strictly "
                                 f"inside the plane-wave box or strictly outside")
    for name, b in (field_boxes or {}).items():
        on_faces = b["kind"] in ("H", "rotH")
        for c, g in sorted(faces if on_faces else edges):
            k, r = divmod(g, nx * ny)
            j, i = divmod(r, nx)
            if all(b["rlo"][a] <= v <= b["hi"][a] for a, v in enumerate((i, j, k))):
                raise ValueError(f"{who}: field box '{name}' records the {'outer face' if on_faces else 'surface edge'} {at((c, g))}: it would hold "
                                 f"a mixed field — keep it (and the node below its low corner) strictly inside the plane-wave box or strictly outside")
