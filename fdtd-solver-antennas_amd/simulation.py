"""Assembly of one FDTD run: operator + boundaries + ports + recording surfaces -> engine(s).

This is the host-side counterpart of what happens between the reference's ``prepare_*`` and the
end of ``FDTD.Run(...)`` (antenna_sim/solver_fdtd_openems_fixed.py:171-220,280): everything the
external engine derives from the scene before and while stepping.  The compute itself is
libfdtd_hip.so (``lib`` argument = a library exporting include/fdtd_hip.h).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence
import numpy as np

from .constants import C0, EPS0, MU0, ETA0
from .grid import RectGrid
from .scene import VoxelScene
from .ecoperator import build_operator, ECOperator, metric_lists, pack_metric_tables, lumped_overrides, LumpedEdge
from . import sheet as _sheet
from . import lumped as _lumped
from . import dispersion as _disp
from . import lorentz as _lorentz
from . import magnetic as _magnetic
from . import conformal as _conformal
from . import subcell as _subcell
from . import sar as _sar
from . import planewave as _planewave
from . import fields as _fields
from . import ports as _ports
from . import field_excitation as _fexc
from . import probes as _probes
from .cpml import CPMLSpec, build_cpml
from .excitation import gauss_pulse, dft_twiddles
from .nf2ff import NF2FFBox, calc_nf2ff
from . import _capi
from ._capi import Engine, KIND_V, KIND_I


def slab_range(nz: int, world: int, rank: int):
    """Contiguous z-planes [k0, k0+nk) of `rank`, planes counted alike; the remainder goes to the first ranks."""
    base, rem = divmod(nz, world)
    k0 = rank * base + min(rank, rem)
    return k0, base + (1 if rank < rem else 0)


# A z-plane inside a z-directed CPML layer reads and writes four more psi arrays per timestep (+16 of 37 bytes per cell and
# half-step) than a plane outside: measured on MI355X it costs 1.3-1.55x as much (NS: 20 layer planes +10.4 us over 60 planes of
# 0.95 us; C3: +18.0 us over 80 planes of 1.78 us — profiles/r02/cpml_axis_cost.txt; per-slab times: profiles/r03/slab_balance.txt).
# With planes counted alike the first and the last rank, which own ALL layer planes, take up to 37 % longer than the interior
# ranks (C5 on 8 GPUs: 10 of their 15 planes), and every rank waits for its neighbours' halos each half-step.
# (weight: each slab timed alone, profiles/r03/slab_balance*.txt — 1.4 leaves max / mean at 1.03 (NS over 8), 1.06 (C4 over 4), 1.03 (C5 over 8);
# 1.5 is better for C4 (1.045) and worse for thin slabs, whose fixed per-launch cost the per-plane model does not know: NS over 4 1.07)
Z_LAYER_PLANE_COST = float(os.environ.get("FDTD_SLAB_WZ", "1.4"))


def plane_costs(nz: int, cpml_lo: int = 0, cpml_hi: int = 0, w_layer: Optional[float] = None) -> np.ndarray:
    """Relative cost of every z-plane of the global grid: 1 outside the z-directed CPML layers, `w_layer` inside
    (planes 0 .. cpml_lo-1 and nz-1-cpml_hi .. nz-1, the planes build_cpml gives psi slots)."""
    w = np.ones(nz)
    wl = Z_LAYER_PLANE_COST if w_layer is None else float(w_layer)
    if cpml_lo:
        w[:cpml_lo] = wl
    if cpml_hi:
        w[nz - 1 - cpml_hi:] = wl
    return w


def slab_partition(costs: Sequence[float], world: int, min_planes: int = 2):
    """[(k0, nk)] * world: contiguous slabs of at least `min_planes` planes whose largest summed cost is as small as possible
    (exact: dynamic programme over the cut positions; ties go to the partition with the smaller sum of squared costs).
    Deterministic, so every rank computes the same cuts."""
    c = np.asarray(costs, float)
    nz = c.size
    if world < 1 or nz < world * min_planes:
        raise ValueError(f"{nz} planes cannot be cut into {world} slabs of >= {min_planes} planes")
    pre = np.concatenate([[0.0], np.cumsum(c)])
    INF = float("inf")
    # best[r][k] = (largest slab cost, sum of squares) of the first k planes in r slabs
    best = [[(INF, INF)] * (nz + 1) for _ in range(world + 1)]
    cut = [[-1] * (nz + 1) for _ in range(world + 1)]
    best[0][0] = (0.0, 0.0)
    for r in range(1, world + 1):
        for k in range(r * min_planes, nz - (world - r) * min_planes + 1):
            for q in range((r - 1) * min_planes, k - min_planes + 1):
                m, sq = best[r - 1][q]
                if m == INF:
                    continue
                sc = pre[k] - pre[q]
                cand = (max(m, sc), sq + sc * sc)
                if cand[0] < best[r][k][0] - 1e-12 or (abs(cand[0] - best[r][k][0]) <= 1e-12 and cand[1] < best[r][k][1] - 1e-12):
                    best[r][k], cut[r][k] = cand, q
    out, k = [], nz
    for r in range(world, 0, -1):
        q = cut[r][k]
        out.append((q, k - q))
        k = q
    return out[::-1]


@dataclass
class BoundarySpec:
    """Per face (x-,x+,y-,y+,z-,z+): 'PEC', 'PMC', 'MUR' or 'CPML' (reference strings 'MUR' / 'PML_8',
    solver_fdtd_openems_microstrip_3d.py:84; openEMS numbers 0 = PEC, 1 = PMC, 2 = MUR, 3 = PML_8).

    A 'PMC' face is a magnetic wall: the tangential face currents of the first dual plane inside the face are held at zero
    (ecoperator.metric_lists), so the wall sits half a cell inside the outer node plane — a symmetry plane of a mirror-symmetric
    scene lies midway between the first two node lines of that side.  The edges on the outer node plane stay dead."""
    kinds: Sequence[str] = ("CPML",) * 6
    cpml_cells: int = 10
    cpml: CPMLSpec = field(default_factory=CPMLSpec)

    @classmethod
    def parse(cls, boundary, cpml_cells: Optional[int] = None) -> "BoundarySpec":
        if isinstance(boundary, BoundarySpec):
            return boundary
        names = [boundary] * 6 if isinstance(boundary, (str, int)) else list(boundary)
        kinds, cells = [], cpml_cells
        for b in names:
            s = str(b).upper()
            if s.startswith("MUR") or s == "2":
                kinds.append("MUR")
            elif s.startswith("PML") or s.startswith("CPML") or s == "3":
                kinds.append("CPML")
                if cells is None and "_" in s and s.split("_")[1].isdigit():
                    cells = int(s.split("_")[1])
            elif s in ("PEC", "0"):
                kinds.append("PEC")
            elif s in ("PMC", "1"):
                kinds.append("PMC")
            else:
                raise ValueError(f"unsupported boundary '{b}'")
        return cls(tuple(kinds), 8 if cells is None else cells)

    def face_cells(self):
        return tuple(self.cpml_cells if k == "CPML" else 0 for k in self.kinds)

    def pmc_faces(self):
        """Six flags for ecoperator.metric_lists, or None without a PMC face."""
        f = tuple(k == "PMC" for k in self.kinds)
        return f if any(f) else None


@dataclass
class RunStats:
    steps: int = 0
    seconds: float = 0.0
    mcells_per_s: float = 0.0
    energy_db: float = 0.0
    stopped_by_energy: bool = False
    schedule_fallback: Optional[str] = None   # set when the run was repeated under the two-launch schedule (see Simulation.run)
    transports_failed: tuple = ()             # decomposed run: halo transports that set up but failed in the first timesteps (see Simulation.run)
    transport_failure_reasons: tuple = ()     # ... and what the library said each time
    sheet_edges: int = 0                      # conducting-sheet edges stepped by the engine (sheet.py)
    sheet_fit_error: Optional[float] = None   # largest band error of the sheets' admittance fits (relative)
    schedule: Optional[dict] = None           # the schedule the engine ran (Engine.schedule_info)
    dispersion: Optional[dict] = None         # Debye media stepped by the engine (dispersion.py): media, K, poles, fit errors, edges
    lorentz: Optional[dict] = None            # Lorentz / Drude media stepped by the engine (lorentz.py): media, K, poles, edges
    lumped: Optional[list] = None             # lumped elements (lumped.py): per element name, kind, R/L/C, edges, split, resonances
    magnetic: Optional[dict] = None           # magnetic materials (magnetic.py): media, classes, faces per component, box extents
    conformal: Optional[dict] = None          # conformal PEC boundaries (conformal.py): faces per component, R, dt factor, faces clamped
    subcell: Optional[dict] = None            # sub-cell averaged dielectric surfaces (subcell.py): listed edges per component, nsub, edges dropped for lumped overrides / dispersive owners, the operator form
    planewave: Optional[dict] = None          # plane-wave excitation (planewave.py): direction, e0, the box in nodes, entries per list
    fields: Optional[dict] = None             # field boxes (fields.py): per name the kind, mode, box and points and, once Simulation.field has run, the interpolation time and device yes/no
    excitations: Optional[list] = None        # field excitations (field_excitation.py): per excitation its type, edges / faces, metal edges dropped, delay
    probes: Optional[list] = None             # stand-alone probes (openems_api: CSX.AddProbe): per probe its type, entries and file
    anisotropic: Optional[dict] = None        # anisotropic dielectrics (scene.py): the materials' names, the cells they own, how the operator was built
    sar: Optional[dict] = None                # SAR boxes (sar.py): per name the voxels, tissue voxels, mass, method and, once Simulation.sar has run, status counts and averaging time


class Simulation:
    def __init__(self, grid: RectGrid, vox: VoxelScene, *, f0: float, fc: float, boundary="CPML",
                 cpml_cells: Optional[int] = None, nr_ts: int = 30000, end_criteria: float = 1e-4,
                 dt: Optional[float] = None, nf2ff_freqs: Optional[Sequence[float]] = None,
                 nf2ff_inset: Optional[int] = None, dft_oversample: float = 4.0, use_classes: bool = True,
                 device_operator: bool = True, nf2ff_mode: str = "dft", rec_budget_bytes: Optional[int] = None,
                 sheet_band: Optional[Sequence[float]] = None, sheet_K: int = _sheet.MAX_K,
                 conformal: bool = False, conformal_ratio: float = _conformal.DEFAULT_RATIO,
                 nf2ff_mirror: Optional[Sequence[int]] = None, nf2ff_half_space: bool = False,
                 subcell: bool = False, subcell_samples: int = 4):
        """nf2ff_mirror: six entries per face (x-, x+, y-, y+, z-, z+), 0 none, 1 PEC, 2 PMC (upstream's numbers): that face is a
        symmetry wall of the scene — its boundary kind must be the same wall — and the NF2FF box is open there; the far field adds
        the mirror images (nf2ff.NF2FFBox, nf2ff.calc_nf2ff).  nf2ff_half_space: the one PEC mirror plane is an infinite ground
        plane instead: nothing radiates behind it and Prad is the half-space's."""
        self.grid, self.vox = grid, vox
        self.f0, self.fc = float(f0), float(fc)
        self.bc = BoundarySpec.parse(boundary, cpml_cells)
        self.nr_ts, self.end_criteria = int(nr_ts), float(end_criteria)
        # conformal PEC boundaries: the faces the metal surfaces cut, each with its four g_e = f_e / a_f <= conformal_ratio; the
        # operator stays the base one, the faces are corrected by the engine after every H update (fdtd_conformal_set); a scene with
        # listed faces runs at courant_dt / sqrt(conformal_ratio)
        self.conformal = None
        if conformal:
            if getattr(vox, "fractions", None) is None:
                raise ValueError("conformal=True needs the fractions of the cut edges: scene.voxelize(scene, grid, conformal=True)")
            self.conformal = _conformal.make_faces(grid, vox.fractions, vox.pec, conformal_ratio)
        # sub-cell averaged dielectric surfaces: the listed edges of scene.voxelize(subcell=) become per-edge (vv, m) overrides next to
        # the lumped ones (_overrides); the Courant limit stays, a mean of eps >= 1 is >= 1
        self.subcell = None
        if subcell:
            nsub = _subcell.check_nsub(subcell_samples)
            if getattr(vox, "cell_voxel", None) is not None:
                raise ValueError("subcell=True on a scene with a disc material (AddDiscMaterial): sub-cell averaging of voxel body models is not supported")
            if getattr(vox, "subcell", None) is None:
                raise ValueError(f"subcell=True needs the listed edges: scene.voxelize(scene, grid, subcell={nsub})")
            if vox.subcell.nsub != nsub:
                raise ValueError(f"subcell_samples = {nsub}, but the scene was voxelised with subcell={vox.subcell.nsub}")
            self.subcell = vox.subcell
        self._subcell_clash = 0
        self.dt = (grid.courant_dt() if self.conformal is None else float(grid.courant_dt() / np.sqrt(self.conformal.ratio))) if dt is None else float(dt)
        self.use_classes = use_classes
        # True: the engine builds the operator itself from materials + mesh (fdtd_build_operator: on the GPU for
        # libfdtd_hip.so); False: numpy build on the host (ecoperator.build_operator, the spec) + array upload
        self.device_operator = device_operator
        self._op: Optional[ECOperator] = None
        cells = self.bc.face_cells()
        self.pmc = self.bc.pmc_faces()
        faces = ("x-", "x+", "y-", "y+", "z-", "z+")
        self.nf2ff_mirror = None
        if nf2ff_mirror is not None:
            self.nf2ff_mirror = tuple(int(v) for v in nf2ff_mirror)
            if len(self.nf2ff_mirror) != 6 or any(m not in (0, 1, 2) for m in self.nf2ff_mirror):
                raise ValueError("nf2ff_mirror: six entries (x-, x+, y-, y+, z-, z+) of 0 (none), 1 (PEC) or 2 (PMC)")
            if nf2ff_freqs is None:
                raise ValueError("nf2ff_mirror needs an NF2FF box (nf2ff_freqs=)")
            for f, m in enumerate(self.nf2ff_mirror):
                want = (None, "PEC", "PMC")[m]
                if m and self.bc.kinds[f] != want:
                    raise ValueError(f"nf2ff_mirror: face {faces[f]} carries a {want} mirror but its boundary is {self.bc.kinds[f]}: "
                                     f"a mirror plane is a {want} wall of the run")
        elif nf2ff_half_space:
            raise ValueError("nf2ff_half_space needs a PEC mirror plane (nf2ff_mirror=), and there is no mirror")
        if self.pmc is not None and nf2ff_freqs is not None:
            bare = [faces[f] for f in range(6) if self.pmc[f] and (self.nf2ff_mirror is None or self.nf2ff_mirror[f] != 2)]
            if bare:
                raise ValueError(f"an NF2FF box together with a PMC face ({', '.join(bare)}) needs that face as a mirror plane: without "
                                 "nf2ff_mirror= (2 on a PMC face) the far field of the mirror image is not added — or run the whole "
                                 "structure, or leave the NF2FF box out")
        self.cpml = None
        if any(cells):
            spec = CPMLSpec(**{**self.bc.cpml.__dict__, "cells": cells})
            self.cpml = build_cpml(grid, self.dt, spec)
        self.mur_enable = np.array([1 if k == "MUR" else 0 for k in self.bc.kinds], np.int32)
        self.mur_coeff_f64 = np.zeros(6, np.float64)
        for f in range(6):
            l = grid.lines[f // 2]
            delta = (l[-1] - l[-2]) if f % 2 else (l[1] - l[0])
            self.mur_coeff_f64[f] = (C0 * self.dt - delta) / (C0 * self.dt + delta)
        self.mur_coeff = self.mur_coeff_f64.astype(np.float32)   # what the C ABI takes
        self.signal = gauss_pulse(self.f0, self.fc, self.dt)
        # (openEMS prints "Requested excitation pulse would be N timesteps ... Cutting to max number of timesteps!" here and goes on; so do we)
        self.excitation_warning = None
        if len(self.signal) > self.nr_ts:
            self.excitation_warning = (f"the excitation pulse is {len(self.signal)} timesteps long (dt = {self.dt:.3e} s: smallest cell "
                                       f"{min(float(np.min(np.diff(l))) for l in grid.lines) * 1e6:.1f} um) but NrTS = {self.nr_ts}: the run ends before the pulse does")
            import warnings
            warnings.warn(self.excitation_warning, RuntimeWarning, stacklevel=2)
        # NF2FF recording
        self.nf2ff_box: Optional[NF2FFBox] = None
        self.nf2ff_warning: Optional[str] = None
        self.nf2ff_freqs = None
        self.nf2ff_mode, self.rec_bytes, self.nf2ff_fmax = "dft", 0, 0.0
        # what add_sar_box needs to set the recorder / DFT up itself when there is no NF2FF box
        self._mode_asked, self._dft_oversample, self._rec_budget = nf2ff_mode, float(dft_oversample), rec_budget_bytes
        self.sar_boxes, self._sar_ids, self._sar_report = {}, {}, {}
        self.field_boxes, self._field_ids, self._field_report, self._kap_e = {}, {}, {}, None
        if nf2ff_freqs is not None:
            self.nf2ff_freqs = np.atleast_1d(np.asarray(nf2ff_freqs, float))
            n = grid.shape
            lo, hi = [], []
            for a in range(3):
                il = (cells[2 * a] + 2) if nf2ff_inset is None else nf2ff_inset
                ih = (cells[2 * a + 1] + 2) if nf2ff_inset is None else nf2ff_inset
                il = max(il, 3); ih = max(ih, 3)
                lo.append(il); hi.append(n[a] - 1 - ih)
            self.nf2ff_box = NF2FFBox(grid, lo, hi, mirror=self.nf2ff_mirror, half_space=bool(nf2ff_half_space))
            lo, hi = list(self.nf2ff_box.lo), list(self.nf2ff_box.hi)     # an open box reaches its walls
            # a Huygens surface that runs ALONG metal is no closed surface around the sources: the far field computed from it is not
            # the antenna's (a ground plane on the very plane of the lower face made a 6 dBi patch read 14.6 dBi).  Metal that merely
            # CROSSES a face (an infinite ground plane, as in the legacy scene) is the caller's modelling decision and not flagged.
            self.nf2ff_warning = None
            for a in range(3):
                for side, pos in ((0, lo[a]), (1, hi[a])):
                    if self.nf2ff_box.mirror[2 * a + side]:      # open there: no face
                        continue
                    sl = [slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1), slice(lo[0], hi[0] + 1)]
                    sl[2 - a] = pos
                    frac = max(float(vox.pec[t][tuple(sl)].mean()) for t in range(3) if t != a)
                    if frac > 0.05 and self.nf2ff_warning is None:
                        self.nf2ff_warning = (f"{100 * frac:.0f} % of the NF2FF box's {'xyz'[a]}-{'max' if side else 'min'} face (node plane {pos}) "
                                              f"lies on metal edges: the far field will not be the antenna's; move the structure or the box")
                        import warnings
                        warnings.warn(self.nf2ff_warning, RuntimeWarning, stacklevel=2)
            fmax = max(self.f0 + self.fc, float(np.max(self.nf2ff_freqs)))
            self.dft_every = max(1, int(np.floor(1.0 / (2.0 * fmax * dft_oversample * self.dt))))
            self.dft_nsamples = self.nr_ts // self.dft_every + 1
            # "record": the faces keep float32 time-domain samples in HBM and any frequency <= fmax can be asked for
            # after the run (what CalcNF2FF does with the engine's dumps); "dft": running sums at nf2ff_freqs only
            # (constant memory).  "auto" records when the samples fit the budget (default 32 GiB of 288 GB per GPU).
            if nf2ff_mode not in ("dft", "record", "auto"):
                raise ValueError("nf2ff_mode must be 'dft', 'record' or 'auto'")
            self.rec_bytes = 4 * self.dft_nsamples * sum(
                int(np.prod([r.hi[a] - r.lo[a] + 1 for a in range(3)])) for r in self.nf2ff_box.requests)
            budget = int(os.environ.get("FDTD_REC_BUDGET_BYTES", 32 << 30)) if rec_budget_bytes is None else int(rec_budget_bytes)
            self.nf2ff_mode = nf2ff_mode if nf2ff_mode != "auto" else ("record" if self.rec_bytes <= budget else "dft")
            self.nf2ff_fmax = fmax
        # conducting sheets: admittance fit per metal over the excitation band (or sheet_band), the implicit part of the update
        # folded into the sheet edges' conductance (lumped-edge overrides), the rest stepped by the engine (fdtd_sheet_set)
        self.sheets = vox.sheets if (vox.sheets is not None and len(vox.sheets)) else None
        self.sheet_fits, self.sheet_lumped, self.sheet_K = [], [], int(sheet_K)
        self.sheet_fit_error = None
        if self.sheets is not None:
            band = _sheet.fit_band(self.f0, self.fc) if sheet_band is None else tuple(map(float, sheet_band))
            self.sheet_fits = [_sheet.fit(m.conductivity, m.thickness, band[0], band[1], K=self.sheet_K) for m in self.sheets.metals]
            self.sheet_fit_error = max(f.band_error for f in self.sheet_fits)
            reqs = [] if self.nf2ff_box is None else [(r.kind, r.comp, r.lo, r.hi) for r in self.nf2ff_box.requests]
            _sheet.check_placement(grid, self.sheets, mur_faces=tuple(self.mur_enable), dft_boxes=reqs)
            nx, ny, _ = grid.shape
            gimp = [f.implicit_G(self.dt) for f in self.sheet_fits]
            k, r = np.divmod(self.sheets.idx, nx * ny)
            j, i = np.divmod(r, nx)
            self.sheet_lumped = [LumpedEdge(int(c), int(a), int(b), int(q), float(sc * gimp[m]))
                                 for c, a, b, q, sc, m in zip(self.sheets.comp, i, j, k, self.sheets.scale, self.sheets.metal)]
        # Debye media: discretised with the run's dt; the part of the branch currents proportional to the mean edge voltage folded
        # into the cells' kappa (exact: linear in per-cell values), the rest stepped by the engine (fdtd_debye_set)
        self.debye = vox.debye if getattr(vox, "debye", None) is not None and len(vox.debye) else None
        # anisotropic dielectrics (scene.VoxelScene.eps_axes): the cells' eps_r / kappa per axis, [3][nz-1][ny-1][nx-1] — what the operator,
        # the lumped overrides and the edge conductivities read in place of the per-cell arrays; the folds below add their term to all
        # three axes of their own cells (dispersive media are isotropic)
        self.anisotropic = getattr(vox, "eps_axes", None) is not None
        self.eps_cells = vox.eps_axes if self.anisotropic else vox.eps_r
        kappa0 = vox.kappa_axes if self.anisotropic else vox.kappa
        self.kappa_cells = kappa0
        if self.debye is not None:
            _disp.check_placement(grid, self.debye.cell_medium, cells, [" / ".join(n) for n in self.debye.names])
            self.kappa_cells = kappa0.copy()
            for q, m in enumerate(self.debye.media):
                on = self.debye.cell_medium == q
                assert np.all(self.eps_cells[..., on] == m.eps_inf)
                self.kappa_cells[..., on] = m.folded(self.dt)[1]
        # Lorentz / Drude media: the same fold with the branches' g0 (lorentz.py), the rest stepped by the engine (fdtd_lorentz_set)
        self.lorentz = vox.lorentz if getattr(vox, "lorentz", None) is not None and len(vox.lorentz) else None
        if self.lorentz is not None:
            _lorentz.check_placement(grid, self.lorentz.cell_medium, cells, [" / ".join(n) for n in self.lorentz.names])
            if self.kappa_cells is kappa0:
                self.kappa_cells = kappa0.copy()
            for q, m in enumerate(self.lorentz.media):
                on = self.lorentz.cell_medium == q
                assert np.all(self.eps_cells[..., on] == m.eps_inf)
                self.kappa_cells[..., on] = m.folded(self.dt)[1]
        # magnetic materials: per-cell mu_r / sigma_m -> face coefficients at this dt -> classes and boxes; the operator stays the
        # base one (ii = 1, iv0), the faces are corrected by the engine after every H update (fdtd_magnetic_set)
        self.magnetic = None
        sgm = None if getattr(vox, "mu_r", None) is None else vox.sigma_m if vox.sigma_m is not None else np.zeros_like(vox.mu_r)
        if sgm is not None and (np.any(vox.mu_r != 1.0) or np.any(sgm != 0.0)):
            _magnetic.check_cells(grid, vox.mu_r, sgm, cells, vox.cell_material, vox.material_names)
            media = []
            if vox.cell_material is not None and vox.material_names is not None:
                on = (vox.mu_r != 1.0) | (sgm != 0.0)
                media = [vox.material_names[q] for q in np.unique(vox.cell_material[on]) if q >= 0]
            self.magnetic = _magnetic.make_faces(grid, vox.mu_r, sgm, self.dt, media)
        if self.conformal is not None:
            _conformal.check_placement(grid, self.conformal, cells, tuple(self.mur_enable),
                                       None if self.magnetic is None else self.magnetic.full_classes(grid.shape[::-1]))
        # lumped elements: a plain 1/R and the implicit part g0 of the stepped branch folded into the edges' conductance, a plain C
        # into their capacitance (lumped-edge overrides); the edges that carry states are stepped by the engine (fdtd_lumped_set)
        self.elements = vox.elements if getattr(vox, "elements", None) is not None and len(vox.elements) else None
        self.element_lumped, self.element_stepped = [], np.zeros(0, np.int64)
        if self.elements is not None:
            el = self.elements
            nx, ny, _ = grid.shape
            fold = [m.discretise(self.dt)[3:] for m in el.elements]
            k, r = np.divmod(el.idx, nx * ny)
            j, i = np.divmod(r, nx)
            self.element_lumped = [LumpedEdge(int(c), int(a), int(b), int(q), float(fold[m][0] + fold[m][1]), float(fold[m][2]))
                                   for c, a, b, q, m in zip(el.comp, i, j, k, el.elem)]
            self.element_stepped = el.stepped()
        # plane-wave excitation: the box checked against everything else in the scene; the two entry lists are built in build(), from the
        # operator the engine holds (fdtd_get_operator), and stepped by the engine (fdtd_planewave_set)
        self.plane_wave = getattr(vox, "plane_wave", None)
        self.signal2, self.planewave_tables = None, None
        if self.plane_wave is not None:
            self._check_plane_wave()
            self.signal2 = _planewave.signal2(self.f0, self.fc, self.dt, len(self.signal))
            reach = int(np.ceil(self.plane_wave.far_delay(grid) / self.dt)) + len(self.signal)
            if reach > self.nr_ts and self.excitation_warning is None:
                self.excitation_warning = (f"the excitation pulse is {len(self.signal)} timesteps long and the plane wave '{self.plane_wave.name}' needs "
                                           f"{reach - len(self.signal)} more to cross its box, but NrTS = {self.nr_ts}: the run ends before the pulse has left the box")
                import warnings
                warnings.warn(self.excitation_warning, RuntimeWarning, stacklevel=2)
        # field excitations: the E types are source lists (a hard one also zeroes its edges' operator entries: _overrides), the H types
        # the two lists of fdtd_excite_set with the pulse at the half-steps; all checked against every other list of this run
        self.excitations = getattr(vox, "field_excitations", None) or None
        self.excite_lists, self.excite_h_args, self.signal_h = None, None, None
        if self.excitations is not None:
            from .scene import _tol
            self.excite_lists = _fexc.lists(grid, self.excitations, vox.unit, self.dt, vox.pec, _tol(grid))
            self._check_field_excitations(1)
            if self.excite_lists.any_h():
                self.signal_h = _fexc.signal_h(self.f0, self.fc, self.dt, len(self.signal))
                self.excite_h_args = self.excite_lists.h_args(self.signal_h)
        self.probes, self._probe_ids = {}, {}          # stand-alone probes (probes.py): name -> probes.ProbeLists, -> device probe ids
        self.engine: Optional[Engine] = None
        self.lib = None
        self.external_transport = None     # distributed.SlabComm when halos travel through the host
        self._port_probe_ids = []
        self._port_probe_lists = []     # per port ([V-probe ids], [I-probe ids]); _port_probe_ids holds the first of each
        self._nf_ids = []
        # waveguide and MSL ports: their planes against the walls and against every correction list of this run (ports.py)
        for p in vox.ports:
            if p.info is not None:
                _ports.check_placement(grid, p.port, p.info, _ports.Probe(p.src_idx, p.src_comp, p.src_amp), p.v_probes, p.i_probes, pec=vox.pec,
                                       kinds=self.bc.kinds, debye=self.debye, lorentz=self.lorentz, sheets=self.sheets, elements=self.elements,
                                       conformal=self.conformal, plane_wave=self.plane_wave)

    def _check_plane_wave(self):
        """planewave.check_placement against the scene as this simulation holds it (again when a SAR box is added)."""
        v = self.vox
        reqs = [] if self.nf2ff_box is None else [(r.kind, r.comp, r.lo, r.hi) for r in self.nf2ff_box.requests]
        eps_r, kappa = v.eps_r, v.kappa
        if self.anisotropic:      # vacuum means vacuum on all three axes: per cell the first axis value that is not the vacuum's
            ea, ka = v.eps_axes, v.kappa_axes
            eps_r = np.where(ea[0] != 1.0, ea[0], np.where(ea[1] != 1.0, ea[1], ea[2]))
            kappa = np.where(ka[0] != 0.0, ka[0], np.where(ka[1] != 0.0, ka[1], ka[2]))
        _planewave.check_placement(self.grid, self.plane_wave, cpml_cells=self.bc.face_cells(), kinds=self.bc.kinds, eps_r=eps_r, kappa=kappa,
                                   mu_r=getattr(v, "mu_r", None), sigma_m=getattr(v, "sigma_m", None), pec=v.pec, sheets=self.sheets,
                                   elements=self.elements, debye=self.debye, lorentz=self.lorentz, conformal=self.conformal, ports=v.ports,
                                   dft_boxes=reqs, sar_boxes=self.sar_boxes, field_boxes=self.field_boxes)

    def add_probe(self, spec: "_probes.ProbeSpec", unit: float = 1e-3) -> "_probes.ProbeLists":
        """A stand-alone probe (before build): probes.ProbeSpec with its box in drawing units of `unit` metres.  One or three device
        probes; a context takes probes.MAX_PROBES, the ports' included."""
        from .scene import _tol
        if self.engine is not None:
            raise ValueError(f"probe '{spec.name}': add_probe comes before build")
        if spec.name in self.probes:
            raise ValueError(f"probe '{spec.name}' is defined twice")
        pl = _probes.lists(self.grid, self.vox.pec, spec, unit, _tol(self.grid))
        used = sum(len(p.v_probes) + len(p.i_probes) for p in self.vox.ports) + sum(len(q.lists) for q in self.probes.values())
        if used + len(pl.lists) > _probes.MAX_PROBES:
            raise ValueError(f"probe '{spec.name}': its {len(pl.lists)} device probe(s) would make {used + len(pl.lists)} probes, a context takes "
                             f"{_probes.MAX_PROBES} (FDTD_MAX_PROBES), the ports' {sum(len(p.v_probes) + len(p.i_probes) for p in self.vox.ports)} included")
        self.probes[spec.name] = pl
        return pl

    def probe_series(self, name, allreduce=None) -> dict:
        """{"t", "val"} of probe `name` after the run: val 1-D, or [3][n] for the field types; t carries the half-step for the
        current types."""
        if name not in self.probes:
            raise KeyError(f"no probe '{name}' (defined: {sorted(self.probes)})")
        if self.engine is None or name not in self._probe_ids:
            raise RuntimeError("probe series: build and run first")
        pl = self.probes[name]
        get = (lambda q: self.engine.get_probe(q)) if allreduce is None else (lambda q: allreduce(self.engine.get_probe(q)))
        val = [get(q) / sc for q, sc in zip(self._probe_ids[name], pl.scale)]
        t = (np.arange(val[0].size) + (0.5 if pl.kind == KIND_I else 0.0)) * self.dt
        return {"t": t, "val": val[0] if len(val) == 1 else np.stack(val)}

    def _check_field_excitations(self, world: int):
        """field_excitation.check_placement against the scene as this simulation holds it."""
        pw_elems = None
        if self.plane_wave is not None:
            g = self.grid
            pw_elems = tuple(np.unique(np.array([g.flat(i, j, k) * 3 + n for n, i, j, k, *_ in _planewave.terms(g, self.plane_wave, phase)], np.int64))
                             for phase in (0, 1))
        _fexc.check_placement(self.grid, self.excitations, self.excite_lists, cpml_cells=self.bc.face_cells(),
                              magnetic_classes=None if self.magnetic is None else self.magnetic.full_classes(self.grid.shape[::-1]),
                              conformal=self.conformal, plane_wave_elems=pw_elems, ports=self.vox.ports, elements=self.elements, sheets=self.sheets,
                              debye=self.debye, lorentz=self.lorentz, world=world)

    def _overrides(self, dtype=np.float32, subcell: bool = True):
        """(edge, comp, vv, m) of the edges whose operator entries the host fixes: the lumped conductances and capacitances, the
        hard E edges of the field excitations with vv = m = 0 (their voltage is the source's alone), and last (`subcell`) the listed
        edges of the sub-cell averaged dielectric surfaces that are none of the former."""
        v = self.vox
        edge, comp, vv, m = lumped_overrides(self.grid, self.eps_cells, self.kappa_cells, v.pec, self.dt, v.lumped + self.sheet_lumped + self.element_lumped, dtype=dtype)
        if self.excite_lists is not None and self.excite_lists.hard_e[0].size:
            h = self.excite_lists.hard_e
            key, first = np.unique(h[0] * 3 + h[1], return_index=True)
            z = np.zeros(first.size, dtype)
            edge, comp, vv, m = np.concatenate([edge, h[0][first]]), np.concatenate([comp, h[1][first]]), np.concatenate([vv, z]), np.concatenate([m, z])
        if subcell and self.subcell is not None:
            s_edge, s_comp, s_vv, s_m = self._subcell_overrides(edge, comp, dtype)
            edge, comp, vv, m = np.concatenate([edge, s_edge]), np.concatenate([comp, s_comp]), np.concatenate([vv, s_vv]), np.concatenate([m, s_m])
        return edge, comp, vv, m

    def _subcell_overrides(self, edge, comp, dtype=np.float32):
        """subcell.overrides of the listed edges that carry no other host-fixed override (edge, comp): the lists stay disjoint."""
        s_edge, s_comp, s_vv, s_m = _subcell.overrides(self.subcell, self.dt, dtype)
        keep = ~np.isin(s_edge * 3 + s_comp, np.asarray(edge, np.int64) * 3 + np.asarray(comp, np.int64))
        self._subcell_clash = int(np.count_nonzero(~keep))
        return s_edge[keep], s_comp[keep], s_vv[keep], s_m[keep]

    @property
    def op(self) -> ECOperator:
        """The operator in its host (numpy) formulation — built on first use; the default product path never asks."""
        if self._op is None:
            v = self.vox
            walls = {} if self.pmc is None else {"pmc": self.pmc}
            if self.subcell is not None:      # the listed edges, never one the host fixes otherwise (as _overrides)
                walls["edge_overrides"] = self._subcell_overrides(*self._overrides(subcell=False)[:2])
            self._op = build_operator(self.grid, self.eps_cells, self.kappa_cells, v.pec, self.dt, v.lumped + self.sheet_lumped + self.element_lumped, **walls)
            if self.excite_lists is not None and self.excite_lists.hard_e[0].size:      # hard E edges: vv = m = 0 (as _overrides)
                h = self.excite_lists.hard_e
                self._op.vv.reshape(3, -1)[h[1].astype(np.int64), h[0]] = 0.0
                self._op.m.reshape(3, -1)[h[1].astype(np.int64), h[0]] = 0.0
        return self._op

    # ---------------------------------------------------------------------------------------------
    def slabs(self, world: int, partition: str = "cost"):
        """[(k0, nk)] of every rank.  "cost": slabs of equal COST — the z-layer planes weigh Z_LAYER_PLANE_COST, so the two
        end ranks own fewer planes; "even": equal plane counts (SURVEY §8e's first cut)."""
        nz = self.grid.shape[2]
        cells = self.bc.face_cells()
        if partition == "even" or world == 1 or not (cells[4] or cells[5]):
            return [slab_range(nz, world, r) for r in range(world)]
        if partition != "cost":
            raise ValueError("partition must be 'cost' or 'even'")
        return slab_partition(plane_costs(nz, cells[4], cells[5]), world)

    def build(self, lib, *, rank: int = 0, world: int = 1, device: int = 0, flags: int = 0, partition: str = "cost") -> Engine:
        g = self.grid
        nx, ny, nz = g.shape
        k0, nk = self.slabs(world, partition)[rank]
        self.partition = partition
        if nk < 2:
            raise ValueError(f"slab of rank {rank} has {nk} planes; need >= 2")
        if self.nf2ff_mirror is not None and any(self.nf2ff_mirror) and world > 1:
            raise ValueError("nf2ff_mirror needs a single slab (world = 1): the open NF2FF box of a decomposed run is not supported")
        if self.sheets is not None and world > 1:
            raise _capi.FdtdError("conducting sheets need a single slab (world = 1): a decomposed lossy-metal run is not supported")
        if self.element_stepped.size and world > 1:
            raise _capi.FdtdError("lumped elements need a single slab (world = 1): a decomposed run with stepped R-L-C elements is not supported")
        if self.debye is not None and world > 1:
            raise _capi.FdtdError("Debye media need a single slab (world = 1): a decomposed run with dispersive media is not supported")
        if self.lorentz is not None and world > 1:
            raise _capi.FdtdError("Lorentz media need a single slab (world = 1): a decomposed run with dispersive media is not supported")
        if self.magnetic is not None and world > 1:
            raise _capi.FdtdError("magnetic materials need a single slab (world = 1): a decomposed run with magnetic media is not supported")
        if self.conformal is not None and world > 1:
            raise _capi.FdtdError("conformal boundaries need a single slab (world = 1): a decomposed run with cut faces is not supported")
        if self.plane_wave is not None and world > 1:
            raise _capi.FdtdError("plane-wave excitation needs a single slab (world = 1): a decomposed run with a plane wave is not supported")
        if self.sar_boxes and world > 1:
            raise _capi.FdtdError("SAR boxes need a single slab (world = 1): a decomposed run with SAR boxes is not supported")
        if self.field_boxes and world > 1:
            raise _capi.FdtdError("field boxes need a single slab (world = 1): a decomposed run with field boxes is not supported")
        if self.excitations is not None and world > 1:
            self._check_field_excitations(world)      # (an H-type excitation on a decomposed run: ValueError naming it)
        e = Engine(lib, nx, ny, nz, self.dt, k0=k0, nk=nk, rank=rank, world=world, device=device,
                   max_steps=self.nr_ts, flags=flags)
        # an anisotropic scene on a library without fdtd_build_operator_axes (the oracle): the host arrays
        if self.device_operator and not (self.anisotropic and not _capi.has_aniso(lib)):
            v = self.vox
            emet, hmet = pack_metric_tables(*metric_lists(g, self.dt, pmc=self.pmc), g, k0, nk)
            if self.anisotropic:
                e.build_operator_axes(g.d, self.eps_cells, self.kappa_cells, v.pec, EPS0, self._overrides(), emet, hmet,
                                      prefer_classes=self.use_classes)
            else:
                e.build_operator(g.d, v.eps_r, self.kappa_cells, v.pec, EPS0,
                                 self._overrides(), emet, hmet,
                                 prefer_classes=self.use_classes)
            self.operator_form = "raw" if e.operator_form()[0] == "raw" else "classes"
            self.operator_build = "device"
        else:
            self.operator_build = "host"
            cls = self.op.classes(k0, nk) if self.use_classes else None
            if cls is not None:
                emet, hmet = self.op.metric_tables(k0, nk)
                e.set_operator_classes(cls[0], cls[1], cls[2], emet, hmet)
                self.operator_form = "classes"
            else:
                e.set_operator_raw(*self.op.raw(k0, nk))
                self.operator_form = "raw"
        if self.debye is not None:
            e.set_debye(*self.debye_tables())
        if self.lorentz is not None:
            e.set_lorentz(*self.lorentz_tables())
        if self.sheets is not None:
            e.set_sheets(*self.sheet_tables())
        if self.element_stepped.size:
            e.set_lumped(*self.lumped_tables())
        if self.magnetic is not None:
            e.set_magnetic(*self.magnetic.tables())
        if self.conformal is not None:
            e.set_conformal(*self.conformal_tables())
        if self.plane_wave is not None:
            op = e.get_operator()
            self.planewave_tables = _planewave.tables(g, self.plane_wave, self.dt, op[1], op[3], self.signal2)
            e.set_planewave(*self.planewave_tables.args())
        if self.excite_h_args is not None:
            e.set_excite(*self.excite_h_args)
        if self.cpml is not None:
            e.set_cpml(*self.cpml.for_slab(k0, nk))
        if self.mur_enable.any():
            e.set_mur(self.mur_enable, self.mur_coeff)
        e.set_signal(self.signal)
        self._port_probe_ids = []
        self._port_probe_lists = []
        for p in self.vox.ports:      # a port = optional resistor edges (in the operator above), one source list, V-probes, I-probes
            if p.port.excite != 0:
                e.add_source(p.src_idx, p.src_comp, p.src_amp,
                             np.full(p.src_idx.size, p.port.delay_steps, np.int32))
            uids = [e.add_probe(KIND_V, q.idx, q.comp, q.w) for q in p.v_probes]
            iids = [e.add_probe(KIND_I, q.idx, q.comp, q.w) for q in p.i_probes]
            self._port_probe_ids.append((uids[0], iids[0]))
            self._port_probe_lists.append((uids, iids))
        self._probe_ids = {name: [e.add_probe(pl.kind, q.idx, q.comp, q.w) for q in pl.lists] for name, pl in self.probes.items()}
        if self.excite_lists is not None:             # the E types: soft list, then hard list (their edges hold vv = vi = 0)
            for l in (self.excite_lists.soft_e, self.excite_lists.hard_e):
                if l[0].size:
                    e.add_source(l[0], l[1], l[2], l[3])
        if self.nf2ff_box is not None or self.sar_boxes or self.field_boxes:
            if self.nf2ff_mode == "record":
                try:
                    e.set_recorder(self.dft_every, self.dft_nsamples)
                    self._register_boxes(e)
                except _capi.FdtdError as err:
                    raise _capi.FdtdError(f"{err} — time-domain NF2FF recording needs {self.rec_bytes / 2**30:.1f} GiB; "
                                          "use nf2ff_mode='dft'") from err
            else:
                tw_v = dft_twiddles(self.nf2ff_freqs, self.dt, self.dft_every, self.dft_nsamples, 0.0)
                tw_i = dft_twiddles(self.nf2ff_freqs, self.dt, self.dft_every, self.dft_nsamples, 0.5)
                e.set_dft(self.dft_every, tw_v, tw_i)
                self._register_boxes(e)
        self.engine, self.lib = e, lib
        self.rank, self.world, self.device = rank, world, device
        self._build_flags = int(flags)
        return e

    def _register_boxes(self, e: Engine):
        """The NF2FF faces, then per SAR box its three voltage boxes (kind V, components 0..2) on the node box, then per field box
        its three voltage or current boxes on the recorded region (fields.region)."""
        if self.nf2ff_box is not None:
            self._nf_ids = self.nf2ff_box.register(e)
        self._sar_ids = {name: [e.add_dft_box(KIND_V, c, b["lo"], b["hi"]) for c in range(3)] for name, b in self.sar_boxes.items()}
        self._field_ids = {name: [e.add_dft_box(KIND_I if _fields.NEEDS_I[b["kind"]] else KIND_V, c, b["rlo"], b["hi"]) for c in range(3)]
                           for name, b in self.field_boxes.items()}

    # ---------------------------------------------------------------------------------------------
    def add_sar_box(self, name, start, stop, freqs, mass, method: str = "ieee"):
        """A SAR box (before build): start / stop in metres, snapped to whole cells; `freqs` the frequencies Simulation.sar may be
        asked for; `mass` the averaging mass in kg (0: local SAR only); `method` "ieee" or "simple" (sar.py).  Its edge voltages are
        recorded like the NF2FF faces, in the mode the run uses; without an NF2FF box the recorder / DFT is set up here, by the
        same rules."""
        if self.engine is not None:
            raise ValueError(f"SAR box '{name}': add_sar_box comes before build")
        if name in self.sar_boxes:
            raise ValueError(f"SAR box '{name}' is defined twice")
        if method not in _sar.METHODS:
            raise ValueError(f"SAR box '{name}': averaging method must be one of {sorted(_sar.METHODS)}, got {method!r}")
        mass = float(mass)
        if not (np.isfinite(mass) and mass >= 0):
            raise ValueError(f"SAR box '{name}': the averaging mass must be finite and >= 0 [kg]")
        f = np.atleast_1d(np.asarray(freqs, float))
        if f.size == 0 or not np.all(np.isfinite(f)) or np.any(f <= 0):
            raise ValueError(f"SAR box '{name}': needs at least one frequency > 0")
        g, n, cells = self.grid, self.grid.shape, self.bc.face_cells()
        lo = [g.snap(a, min(start[a], stop[a])) for a in range(3)]
        hi = [g.snap(a, max(start[a], stop[a])) for a in range(3)]
        for a in range(3):
            if hi[a] <= lo[a]:
                raise ValueError(f"SAR box '{name}': holds no whole cell along {'xyz'[a]} on this mesh (nodes {lo[a]}..{hi[a]})")
            for side, bad in ((0, lo[a] < cells[2 * a]), (1, hi[a] > n[a] - 1 - cells[2 * a + 1])):
                if cells[2 * a + side] and bad:
                    raise ValueError(f"SAR box '{name}' reaches into the CPML layer {'xyz'[a]}{'+' if side else '-'} ({cells[2 * a + side]} cells): "
                                     f"SAR inside absorbing layers is not supported — end the box before the layer")
        sl = tuple(slice(lo[a], hi[a]) for a in (2, 1, 0))
        for kind, edges in (("Debye", self.debye), ("Lorentz", self.lorentz)):
            if edges is not None and np.any(edges.cell_medium[sl] >= 0):
                m = int(edges.cell_medium[sl][edges.cell_medium[sl] >= 0][0])
                raise ValueError(f"SAR box '{name}' holds cells of the {kind} medium '{' / '.join(edges.names[m])}': the loss of a dispersive "
                                 f"medium depends on frequency, its SAR is not supported — use a material with kappa")
        if self.anisotropic:
            ka = self.vox.kappa_axes
            odd = (ka[0][sl] != ka[1][sl]) | (ka[0][sl] != ka[2][sl])
            if odd.any():
                cm, names = getattr(self.vox, "cell_material", None), getattr(self.vox, "material_names", None)
                q = -1 if cm is None else int(cm[sl][odd][0])
                mat = names[q] if names is not None and q >= 0 else "?"
                raise ValueError(f"SAR box '{name}' holds cells of the material '{mat}', whose kappa is anisotropic: SAR takes one "
                                 f"conductivity per cell (anisotropic eps_r alone is fine) — SAR with anisotropic kappa is not supported")
        rho = getattr(self.vox, "density", None)
        if rho is None or not np.any(rho[sl] > 0):
            raise ValueError(f"SAR box '{name}' holds no cell of a material with density > 0: there is no tissue to average over "
                             f"(AddMaterial(..., density=) / Scene.add_material(..., density=))")
        used = (0 if self.nf2ff_box is None else len(self.nf2ff_box.requests)) + 3 * len(self.sar_boxes) + 3 * len(self.field_boxes)
        if used + 3 > _capi.MAX_BOXES:
            raise ValueError(f"SAR box '{name}': its three voltage boxes would make {used + 3} recording boxes, a context takes "
                             f"{_capi.MAX_BOXES} (FDTD_MAX_BOXES)")
        if self.nf2ff_freqs is None:          # no NF2FF box (and no SAR box yet): the rules of __init__'s NF2FF block
            if self._mode_asked not in ("dft", "record", "auto"):
                raise ValueError("nf2ff_mode must be 'dft', 'record' or 'auto'")
            fmax = max(self.f0 + self.fc, float(np.max(f)))
            self.dft_every = max(1, int(np.floor(1.0 / (2.0 * fmax * self._dft_oversample * self.dt))))
            self.dft_nsamples = self.nr_ts // self.dft_every + 1
            self.nf2ff_freqs, self.nf2ff_fmax = f.copy(), fmax
            self.nf2ff_mode = self._mode_asked
        nbytes = 4 * self.dft_nsamples * 3 * int(np.prod([hi[a] - lo[a] + 1 for a in range(3)]))
        if self.nf2ff_mode == "auto":
            budget = int(os.environ.get("FDTD_REC_BUDGET_BYTES", 32 << 30)) if self._rec_budget is None else int(self._rec_budget)
            self.nf2ff_mode = "record" if nbytes <= budget else "dft"
        if self.nf2ff_mode == "record":
            if float(np.max(f)) > self.nf2ff_fmax * (1 + 1e-9):
                raise ValueError(f"SAR box '{name}': frequency {float(np.max(f)):g} Hz is above the recorder's band ({self.nf2ff_fmax:g} Hz)")
        else:
            rec = np.asarray(self.nf2ff_freqs, float)
            miss = [x for x in f if np.min(np.abs(rec - x)) > 1e-6 * max(x, 1.0)]
            if miss:
                raise ValueError(f"SAR box '{name}': frequency {miss[0]:g} Hz is not among nf2ff_freqs ({rec.tolist()}): the running DFT "
                                 f"accumulates those only — add it to nf2ff_freqs or use nf2ff_mode='record'")
        if self.plane_wave is not None:
            self.sar_boxes[name] = {"lo": tuple(lo), "hi": tuple(hi)}
            try:
                self._check_plane_wave()
            finally:
                del self.sar_boxes[name]
        self.rec_bytes += nbytes
        self.sar_boxes[name] = {"lo": tuple(lo), "hi": tuple(hi), "freqs": f, "mass": mass, "method": method}
        self._sar_report[name] = {"voxels": int(np.prod([hi[a] - lo[a] for a in range(3)])), "tissue_voxels": int(np.count_nonzero(rho[sl] > 0)),
                                  "mass_kg": mass, "method": method, "status_counts": None, "averaging_seconds": None, "device": None}

    def sar(self, name, freq=None, normalise_to=None) -> "_sar.SARResult":
        """Local and mass-averaged SAR of box `name` at `freq` (default: the box's first frequency), after the run: the spectra of
        its three voltage boxes (single-sided, as nf2ff_boxes) -> csrc/sar.hip, or sar.py where the library has no SAR entry points
        or FDTD_SAR=host.  normalise_to=P divides the SAR values and P_abs by P — with the accepted power of CalcPort at the same
        frequency (the same single-sided pulse spectrum) that is SAR per watt."""
        if name not in self.sar_boxes:
            raise KeyError(f"no SAR box '{name}' (defined: {sorted(self.sar_boxes)})")
        if self.engine is None or name not in self._sar_ids:
            raise RuntimeError("SAR: build and run first")
        b = self.sar_boxes[name]
        f = float(b["freqs"][0] if freq is None else freq)
        ids = self._sar_ids[name]
        if self.nf2ff_mode == "record":
            if f > self.nf2ff_fmax * (1 + 1e-9):
                raise ValueError(f"SAR frequency {f:g} Hz is above the recorder's band ({self.nf2ff_fmax:g} Hz)")
            tw = dft_twiddles(np.array([f]), self.dt, self.dft_every, self.dft_nsamples, 0.0)
            V = [self.engine.rec_transform(q, tw)[0][0] for q in ids]
        else:
            rec = np.asarray(self.nf2ff_freqs, float)
            row = int(np.argmin(np.abs(rec - f)))
            if abs(rec[row] - f) > 1e-6 * max(f, 1.0):
                raise ValueError(f"SAR frequency {f:g} Hz was not recorded (recorded: {rec.tolist()})")
            V = [self.engine.get_dft_box(q)[0][row] for q in ids]
        scale = 2.0 * self.dt * self.dft_every
        V = [v * scale for v in V]
        lo, hi = b["lo"], b["hi"]
        g = self.grid
        d = [g.d[a][lo[a]:hi[a]] for a in range(3)]
        sl = tuple(slice(lo[a], hi[a]) for a in (2, 1, 0))
        sigma, rho = np.ascontiguousarray(self.vox.kappa[sl]), np.ascontiguousarray(self.vox.density[sl])
        calls = _capi.sar_device(self.lib, self.device)
        p, s_loc, s_avg, half, status, counts, secs = _sar.evaluate(d[0], d[1], d[2], V[0], V[1], V[2], sigma, rho, b["mass"], b["method"], calls)
        vol = d[2][:, None, None] * d[1][None, :, None] * d[0][None, None, :]
        p_abs, box_mass = float(np.sum(p * vol)), float(np.sum(rho * vol))
        if normalise_to is not None:
            s_loc, s_avg, p_abs = s_loc / normalise_to, s_avg / normalise_to, p_abs / normalise_to
        ctr = [g.centers(a)[lo[a]:hi[a]] for a in range(3)]
        if np.all(np.isnan(s_avg)):
            peak, cell = float("nan"), (-1, -1, -1)
        else:
            k, j, i = np.unravel_index(int(np.nanargmax(s_avg)), s_avg.shape)
            peak, cell = float(s_avg[k, j, i]), (int(i), int(j), int(k))
        pos = tuple(float(ctr[a][cell[a]]) for a in range(3)) if cell[0] >= 0 else (float("nan"),) * 3
        cnt = {"valid": int(counts[0]), "used": int(counts[1]), "no_cube": int(counts[2]), "too_small": int(counts[3]),
               "background": int(np.count_nonzero(status == _sar.STATUS_BACKGROUND))}
        self._sar_report[name].update(status_counts=cnt, averaging_seconds=secs, device=calls is not None)
        return _sar.SARResult(name=name, freq=f, averaging_mass=b["mass"], method=b["method"], sar_local=s_loc, sar_avg=s_avg, status=status,
                              half_side=half, peak=peak, peak_cell=cell, peak_position=pos, P_abs=p_abs, mass=box_mass, counts=cnt,
                              x=ctr[0], y=ctr[1], z=ctr[2], device=calls is not None, seconds=secs, normalised_to=normalise_to)

    # ---------------------------------------------------------------------------------------------
    def add_field_box(self, name, start, stop, kind, *, mode: int = 1, freqs=None, timesteps=None, sub_sampling=(1, 1, 1)):
        """A field box (before build): start / stop in metres, snapped to nodes; `kind` "E", "H", "J" or "rotH"; `mode` 0 raw, 1
        node-interpolated, 2 cell-interpolated (fields.py); exactly one of `freqs` (spectra) and `timesteps` (snapshots, which need
        nf2ff_mode='record' and snap to the recorder's samples).  Only the boxes the kind needs are recorded — three voltage boxes
        (E, J) or three current boxes (H, rotH) on the box grown by one node on each low side — like the SAR boxes, in the mode the
        run uses; without an NF2FF or SAR box the recorder / DFT is set up here, by the same rules."""
        who = f"field box '{name}'"
        if self.engine is not None:
            raise ValueError(f"{who}: add_field_box comes before build")
        if name in self.field_boxes:
            raise ValueError(f"{who} is defined twice")
        if kind not in _fields.KINDS:
            raise ValueError(f"{who}: kind must be one of {sorted(_fields.KINDS)}, got {kind!r}")
        if mode not in (_fields.MODE_RAW, _fields.MODE_NODE, _fields.MODE_CELL):
            raise ValueError(f"{who}: mode must be 0 (raw), 1 (node-interpolated) or 2 (cell-interpolated), got {mode!r}")
        if (freqs is None) == (timesteps is None):
            raise ValueError(f"{who}: needs exactly one of freqs=[...] (spectra) and timesteps=[...] (snapshots)")
        sub = tuple(int(v) for v in sub_sampling)
        if len(sub) != 3 or min(sub) < 1 or any(int(v) != v for v in sub_sampling):
            raise ValueError(f"{who}: sub_sampling must be three whole numbers >= 1")
        f = ts = None
        if freqs is not None:
            f = np.atleast_1d(np.asarray(freqs, float))
            if f.size == 0 or not np.all(np.isfinite(f)) or np.any(f <= 0):
                raise ValueError(f"{who}: needs at least one frequency > 0")
        else:
            ts = np.atleast_1d(np.asarray(timesteps))
            if ts.size == 0 or not np.all(np.isfinite(ts.astype(float))) or np.any(ts < 0) or np.any(ts != np.round(ts)):
                raise ValueError(f"{who}: timesteps must be whole numbers >= 0")
            ts = ts.astype(np.int64)
        g = self.grid
        lo = [g.snap(a, min(start[a], stop[a])) for a in range(3)]
        hi = [g.snap(a, max(start[a], stop[a])) for a in range(3)]
        for a in range(3):
            if mode == _fields.MODE_CELL and hi[a] <= lo[a]:
                raise ValueError(f"{who}: holds no whole cell along {'xyz'[a]} on this mesh (nodes {lo[a]}..{hi[a]}): cell interpolation needs one")
        rlo, _ = _fields.region(lo, hi)
        what = "current" if _fields.NEEDS_I[kind] else "voltage"
        used = (0 if self.nf2ff_box is None else len(self.nf2ff_box.requests)) + 3 * len(self.sar_boxes) + 3 * len(self.field_boxes)
        if used + 3 > _capi.MAX_BOXES:
            raise ValueError(f"{who}: its three {what} boxes would make {used + 3} recording boxes, a context takes "
                             f"{_capi.MAX_BOXES} (FDTD_MAX_BOXES)")
        fresh = self.nf2ff_freqs is None      # no NF2FF box, no SAR or field box yet: the rules of __init__'s NF2FF block
        keep = (self.nf2ff_freqs, self.nf2ff_fmax, self.nf2ff_mode, getattr(self, "dft_every", None), getattr(self, "dft_nsamples", None))
        if fresh:
            if self._mode_asked not in ("dft", "record", "auto"):
                raise ValueError("nf2ff_mode must be 'dft', 'record' or 'auto'")
            fmax = self.f0 + self.fc if f is None else max(self.f0 + self.fc, float(np.max(f)))
            self.dft_every = max(1, int(np.floor(1.0 / (2.0 * fmax * self._dft_oversample * self.dt))))
            self.dft_nsamples = self.nr_ts // self.dft_every + 1
            self.nf2ff_freqs, self.nf2ff_fmax = (np.array([self.f0]) if f is None else f.copy()), fmax
            self.nf2ff_mode = self._mode_asked
        try:
            nbytes = 4 * self.dft_nsamples * 3 * int(np.prod([hi[a] - rlo[a] + 1 for a in range(3)]))
            mode_run = self.nf2ff_mode
            if mode_run == "auto":
                budget = int(os.environ.get("FDTD_REC_BUDGET_BYTES", 32 << 30)) if self._rec_budget is None else int(self._rec_budget)
                mode_run = "record" if nbytes <= budget else "dft"
            taken = None
            if ts is not None:
                if mode_run != "record":
                    need = self.rec_bytes + nbytes
                    raise ValueError(f"{who}: snapshots (timesteps=) are samples of the time-domain record, and this run keeps running DFT "
                                     f"sums — nf2ff_mode='record' would take {need} bytes ({need / 2**30:.2f} GiB) of device memory")
                taken = np.clip((ts + self.dft_every // 2) // self.dft_every, 0, self.dft_nsamples - 1) * self.dft_every
            elif mode_run == "record":
                if float(np.max(f)) > self.nf2ff_fmax * (1 + 1e-9):
                    raise ValueError(f"{who}: frequency {float(np.max(f)):g} Hz is above the recorder's band ({self.nf2ff_fmax:g} Hz)")
            else:
                rec = np.asarray(self.nf2ff_freqs, float)
                miss = [x for x in f if np.min(np.abs(rec - x)) > 1e-6 * max(x, 1.0)]
                if miss:
                    raise ValueError(f"{who}: frequency {miss[0]:g} Hz is not among nf2ff_freqs ({rec.tolist()}): the running DFT "
                                     f"accumulates those only — add it to nf2ff_freqs or use nf2ff_mode='record'")
            box = {"lo": tuple(lo), "hi": tuple(hi), "rlo": tuple(rlo), "kind": kind, "mode": int(mode), "freqs": f, "timesteps": taken,
                   "timesteps_asked": ts, "sub": sub}
            if self.plane_wave is not None:
                self.field_boxes[name] = box
                try:
                    self._check_plane_wave()
                finally:
                    del self.field_boxes[name]
        except ValueError:
            if fresh:
                self.nf2ff_freqs, self.nf2ff_fmax, self.nf2ff_mode = keep[:3]
                if keep[3] is None:
                    del self.dft_every, self.dft_nsamples
            raise
        self.nf2ff_mode = mode_run
        self.rec_bytes += nbytes
        self.field_boxes[name] = box
        self._field_report[name] = {"kind": kind, "mode": int(mode), "lo": list(lo), "hi": list(hi), "sub_sampling": list(sub),
                                    "points": list(_fields.out_counts(mode, lo, hi, sub)), "seconds": None, "device": None}

    def edge_conductivity(self):
        """The three kap_e arrays [nz][ny][nx] of the operator (ecoperator._edge_average of the cells' kappa as this run folds it; component
        c averages kappa[c] of an anisotropic scene)."""
        if self._kap_e is None:
            from .ecoperator import _edge_average, cell_axes
            self._kap_e = [_edge_average(k, self.grid, c) for c, k in enumerate(cell_axes(np.asarray(self.kappa_cells, np.float64), self.grid))]
        return self._kap_e

    def field(self, name, freq=None, timestep=None) -> "_fields.FieldDump":
        """The dump of field box `name`, after the run: at `freq` (default: the box's first frequency) the single-sided spectrum, scaled
        like the port spectra; at `timestep` (default: the box's first) the recorder sample nearest to it — the result names the
        timestep taken and its time.  Recorded spectra or samples -> csrc/fields.hip, or fields.py where the library has no
        fdtd_field_interp or FDTD_FIELDS=host.  H and rotH are taken at the time of H, half a step after E."""
        if name not in self.field_boxes:
            raise KeyError(f"no field box '{name}' (defined: {sorted(self.field_boxes)})")
        if self.engine is None or name not in self._field_ids:
            raise RuntimeError("field dump: build and run first")
        b = self.field_boxes[name]
        kind, ids = b["kind"], self._field_ids[name]
        half = 0.5 if _fields.H_TIME[kind] else 0.0
        f = step = when = None
        if b["timesteps"] is not None:
            if freq is not None:
                raise ValueError(f"field box '{name}' holds snapshots: ask with timestep=, not freq=")
            t = int(b["timesteps"][0] if timestep is None else timestep)
            s = int(np.clip((t + self.dft_every // 2) // self.dft_every, 0, self.dft_nsamples - 1))
            if s * self.dft_every > int(self.engine.step):
                raise ValueError(f"field box '{name}': timestep {s * self.dft_every} was not reached (the run made {int(self.engine.step)} timesteps)")
            tw = np.zeros((self.dft_nsamples, 1, 2))
            tw[s, 0, 0] = 1.0                          # one-hot: the transform returns the sample itself
            A = [np.ascontiguousarray(self.engine.rec_transform(q, tw)[0][0].real) for q in ids]
            step, when = s * self.dft_every, (s * self.dft_every + half) * self.dt
        else:
            if timestep is not None:
                raise ValueError(f"field box '{name}' holds spectra: ask with freq=, not timestep=")
            f = float(b["freqs"][0] if freq is None else freq)
            if self.nf2ff_mode == "record":
                if f > self.nf2ff_fmax * (1 + 1e-9):
                    raise ValueError(f"field dump frequency {f:g} Hz is above the recorder's band ({self.nf2ff_fmax:g} Hz)")
                tw = dft_twiddles(np.array([f]), self.dt, self.dft_every, self.dft_nsamples, half)
                A = [self.engine.rec_transform(q, tw)[0][0] for q in ids]
            else:
                rec = np.asarray(self.nf2ff_freqs, float)
                row = int(np.argmin(np.abs(rec - f)))
                if abs(rec[row] - f) > 1e-6 * max(f, 1.0):
                    raise ValueError(f"field dump frequency {f:g} Hz was not recorded (recorded: {rec.tolist()})")
                A = [self.engine.get_dft_box(q)[0][row] for q in ids]
            scale = 2.0 * self.dt * self.dft_every
            A = [a * scale for a in A]
        lo, hi, rlo, mode, sub = b["lo"], b["hi"], b["rlo"], b["mode"], b["sub"]
        kap = None
        if kind == "J":
            sl = tuple(slice(rlo[a], hi[a] + 1) for a in (2, 1, 0))
            kap = [np.ascontiguousarray(k[sl]) for k in self.edge_conductivity()]
        call = _capi.fields_device(self.lib, self.device)
        V, I = (None, A) if _fields.NEEDS_I[kind] else (A, None)
        fld, secs = _fields.evaluate(kind, mode, self.grid.lines, lo, hi, V, I, kap, sub, call)
        x, y, z = _fields.points(mode, self.grid.lines, lo, hi, sub)
        self._field_report[name].update(seconds=secs, device=call is not None)
        return _fields.FieldDump(name=name, type=kind, mode=mode, x=x, y=y, z=z, field=fld, freq=f, timestep=step, time=when,
                                 offsets=_fields.offsets(kind, mode), device=call is not None, seconds=secs)

    def sheet_vi(self) -> np.ndarray:
        """float32 vi of the sheet edges, as the engine expands it: m (the edge's lumped-edge override, float32) times the separable
        metric ex[i] * (ey[j] * ez[k]) in float32 — the association of ECOperator.raw, which the raw and class forms share.  Evaluated
        for the sheet edges alone (no download of the expanded operator)."""
        return self._override_vi(self.sheet_lumped, self.sheets.idx, self.sheets.comp)

    def _override_vi(self, lumped, idx, comp) -> np.ndarray:
        g, v = self.grid, self.vox
        m = lumped_overrides(g, self.eps_cells, self.kappa_cells, v.pec, self.dt, lumped)[3]
        nx, ny, _ = g.shape
        k, r = np.divmod(idx, nx * ny)
        j, i = np.divmod(r, nx)
        emet, _ = metric_lists(g, self.dt)
        vi = np.empty(idx.size, np.float32)
        for c in range(3):
            q = np.nonzero(comp == c)[0]
            ex, ey, ez = emet[c]
            vi[q] = m[q] * (ex[i[q]] * (ey[j[q]] * ez[k[q]]))
        return vi

    def lumped_vi(self) -> np.ndarray:
        """float32 vi of the stepped element edges, from the operator this simulation builds (as sheet_vi)."""
        st, el = self.element_stepped, self.elements
        return self._override_vi([self.element_lumped[q] for q in st], el.idx[st], el.comp[st])

    def lumped_tables(self):
        """(idx, comp, vi, cls, phi, gam, h) of fdtd_lumped_set: the element edges that carry states."""
        st, el = self.element_stepped, self.elements
        cls, phi, gam, h = _lumped.tables(el.elements, el.elem[st], self.dt)
        return el.idx[st], el.comp[st], self.lumped_vi(), cls, phi, gam, h

    def lumped_info(self) -> Optional[list]:
        """What RunStats.lumped reports: per element (box) its values, its edges and split, and for an L-C element the analytic
        resonance and the one the stepped branch has at this dt (bilinear warping)."""
        if self.elements is None:
            return None
        el = self.elements
        return [{"name": m.name, "kind": m.kind, "R": m.R, "L": m.L, "C": m.C, "edges": int(np.count_nonzero(el.elem == q)),
                 "n_ser": m.n_ser, "n_par": m.n_par, "states": m.nstates,
                 "resonance_hz": m.resonance(), "resonance_warped_hz": m.resonance(self.dt)}
                for q, m in enumerate(el.elements)]

    def sheet_tables(self):
        """(idx, comp, vi, cls, alpha, b) of fdtd_sheet_set."""
        sh = self.sheets
        cls, alpha, b = _sheet.class_tables(sh, self.sheet_fits, self.dt, self.sheet_K)
        return sh.idx, sh.comp, self.sheet_vi(), cls, alpha, b

    def debye_tables(self):
        """(alpha, oma, beta, lo, hi, w, med) of fdtd_debye_set (Engine.set_debye)."""
        d = self.debye
        alpha, oma, beta = _disp.tables(d.media, self.dt)
        return alpha, oma, beta, d.lo, d.hi, [w.astype(np.float32) for w in d.w], d.med

    def lorentz_tables(self):
        """(phi, gam, h, lo, hi, w, med) of fdtd_lorentz_set (Engine.set_lorentz)."""
        d = self.lorentz
        phi, gam, h = _lorentz.tables(d.media, self.dt)
        return phi, gam, h, d.lo, d.hi, [w.astype(np.float32) for w in d.w], d.med

    def lorentz_info(self) -> Optional[dict]:
        """What RunStats.lorentz reports: per medium the poles; the dispersive edges per component and their boxes."""
        if self.lorentz is None:
            return None
        d = self.lorentz
        return {"media": [{"names": list(n), "eps_inf": m.eps_inf, "kappa": m.kappa, "plasma_hz": (m.wp / (2 * np.pi)).tolist(),
                           "pole_hz": (m.w0 / (2 * np.pi)).tolist(), "gamma": m.gamma.tolist(), "kappa_cell": m.folded(self.dt)[1]}
                          for m, n in zip(d.media, d.names)],
                "K": d.K, "poles": int(sum(m.K for m in d.media)), "edges": [int(np.count_nonzero(w)) for w in d.w],
                "box_edges": [int(np.prod(w.shape)) for w in d.w]}

    def conformal_tables(self):
        """(comp, idx, coef) of fdtd_conformal_set (Engine.set_conformal): coef = iv0 * g_e, iv0 from the H metric tables alone."""
        return _conformal.tables(self.conformal, metric_lists(self.grid, self.dt, pmc=self.pmc)[1], self.grid.shape)

    def conformal_info(self) -> Optional[dict]:
        """What RunStats.conformal reports: the listed faces per component, the cut edges, R, the factor on dt, the faces clamped."""
        if self.conformal is None:
            return None
        c = self.conformal
        return {"faces": c.faces(), "cut_edges": int(c.frac.idx.size), "ratio": c.ratio, "dt_factor": c.dt_factor, "clamped": c.clamped}

    def subcell_info(self) -> Optional[dict]:
        """What RunStats.subcell reports: the listed edges per component, nsub, the edges dropped because they carry a lumped override
        (those the set-up knew of and those that met a host-fixed edge of this run) or have a sample owned by a dispersive material, and
        the operator form the build ended in ("classes" or "raw"; None before build)."""
        if self.subcell is None:
            return None
        s = self.subcell
        return {"edges": s.edges(), "nsub": s.nsub, "dropped_lumped": s.dropped_lumped + self._subcell_clash,
                "dropped_nonplain": s.dropped_nonplain, "operator_form": getattr(self, "operator_form", None)}

    def anisotropic_info(self) -> Optional[dict]:
        """What RunStats.anisotropic reports: the anisotropic materials that own cells, those cells' number, and whether the operator
        came from fdtd_build_operator_axes ("device") or from the host arrays ("host")."""
        if not self.anisotropic:
            return None
        v = self.vox
        odd = np.any(v.eps_axes != v.eps_axes[0], axis=0) | np.any(v.kappa_axes != v.kappa_axes[0], axis=0)
        return {"materials": list(getattr(v, "anisotropic_names", None) or []), "cells": int(np.count_nonzero(odd)),
                "operator_build": getattr(self, "operator_build", None)}

    def planewave_info(self) -> Optional[dict]:
        """What RunStats.planewave reports: direction, e0, the box in nodes and the entries of the two lists."""
        if self.plane_wave is None:
            return None
        pw, t = self.plane_wave, self.planewave_tables
        return {"name": pw.name, "direction": pw.direction.tolist(), "e0": pw.e0.tolist(), "lo": list(pw.lo), "hi": list(pw.hi),
                "edges": None if t is None else int(t.E[0].size), "faces": None if t is None else int(t.H[0].size)}

    def incident_spectrum(self, freqs) -> np.ndarray:
        """s^(f) of the incident pulse, single-sided and scaled by 2 dt like the port spectra of CalcPort and nf2ff_boxes: the
        incident field at r is E0 s^(f) exp(-j 2 pi f k.(r - r0)/c0)."""
        if self.plane_wave is None:
            raise RuntimeError("incident_spectrum: the scene has no plane wave (Scene.add_plane_wave / AddExcitation)")
        return _planewave.incident_spectrum(freqs, self.signal2, self.dt)

    def rcs(self, freq, theta, phi) -> np.ndarray:
        """Bistatic radar cross-section [m^2] over theta x phi [rad] at `freq`, after the run: 4 pi U(theta, phi) / S_inc with U the
        radiation intensity of the SCATTERED field (an NF2FF box strictly outside the plane-wave box) and
        S_inc = 1/2 |E0|^2 |s^(f)|^2 / Z0 the incident power density."""
        if self.plane_wave is None:
            raise RuntimeError("rcs: the scene has no plane wave (Scene.add_plane_wave / AddExcitation)")
        if self.nf2ff_box is None or self.engine is None:
            raise RuntimeError("rcs: needs an NF2FF box (nf2ff_freqs=) outside the plane-wave box, and a finished run")
        pw, nb = self.plane_wave, self.nf2ff_box
        if any(nb.mirror):
            raise ValueError("rcs: an NF2FF box with mirror planes is not supported (the incident wave has no image)")
        if not all(nb.lo[a] < pw.lo[a] and nb.hi[a] > pw.hi[a] for a in range(3)):
            raise ValueError(f"rcs: the NF2FF box (nodes {nb.lo}..{nb.hi}) does not enclose the box of plane wave '{pw.name}' (nodes {pw.lo}..{pw.hi}): "
                             f"it records the total field, not the scattered one")
        f = float(freq)
        if self.nf2ff_mode == "record":
            boxes = self.nf2ff_boxes(freqs=[f])
        else:
            rec = np.asarray(self.nf2ff_freqs, float)
            row = int(np.argmin(np.abs(rec - f)))
            if abs(rec[row] - f) > 1e-6 * max(f, 1.0):
                raise ValueError(f"rcs: frequency {f:g} Hz was not recorded (recorded: {rec.tolist()})")
            boxes = [b[row:row + 1] for b in self.nf2ff_boxes()]
        centre = [0.5 * (self.grid.lines[a][pw.lo[a]] + self.grid.lines[a][pw.hi[a]]) for a in range(3)]
        res = calc_nf2ff(self.lib, nb, boxes, [f], np.atleast_1d(theta), np.atleast_1d(phi), centre, device=getattr(self, "device", 0))
        s_inc = 0.5 * float(pw.e0 @ pw.e0) * abs(self.incident_spectrum([f])[0]) ** 2 / ETA0
        return 4.0 * np.pi * res.P_rad[0] / s_inc

    def magnetic_info(self) -> Optional[dict]:
        """What RunStats.magnetic reports: the magnetic media, the (a, b) classes, the faces per component and their boxes."""
        if self.magnetic is None:
            return None
        m = self.magnetic
        return {"media": list(m.media), "classes": m.ncls, "faces": m.faces(), "lo": [list(map(int, v)) for v in m.lo],
                "hi": [list(map(int, v)) for v in m.hi], "box_faces": [int(c.size) for c in m.cls]}

    def dispersion_info(self) -> Optional[dict]:
        """What RunStats.dispersion reports: per medium the poles and, for fitted media, the fit's errors."""
        if self.debye is None:
            return None
        d = self.debye
        return {"media": [{"names": list(n), "eps_inf": m.eps_inf, "kappa": m.kappa, "delta_eps": m.delta_eps.tolist(),
                           "tau": m.tau.tolist(), "relaxation_hz": (1.0 / (2 * np.pi * m.tau)).tolist(), "fit": m.fit_info}
                          for m, n in zip(d.media, d.names)],
                "K": d.K, "poles": int(sum(m.K for m in d.media)), "edges": len(d),
                "fit_errors": {"tan_delta": max([m.fit_info["tan_delta_error"] for m in d.media if m.fit_info] or [None], key=lambda v: v or 0),
                               "eps": max([m.fit_info["eps_error"] for m in d.media if m.fit_info] or [None], key=lambda v: v or 0)},
                "box_edges": [int(np.prod(w.shape)) for w in d.w]}

    # ---------------------------------------------------------------------------------------------
    def run(self, *, max_steps: Optional[int] = None, check_every: int = 200, verbose: int = 0,
            allreduce=None, log=print) -> RunStats:
        """Step until nr_ts or until the field energy drops below end_criteria x its maximum
        ([EXT] openEMS end criterion, EndCriteria=1e-4 at solver_fdtd_openems_fixed.py:171).
        `allreduce(np.ndarray) -> np.ndarray` sums the two energy terms over ranks when world > 1."""
        import time
        e = self.engine
        total = self.nr_ts if max_steps is None else min(max_steps, self.nr_ts)
        emax, stats = 0.0, RunStats()
        t0 = time.perf_counter()
        done = e.step
        fresh = done == 0          # stepping from the state build() left: a repeat from scratch reproduces it
        comm = getattr(self, "comm", None)      # distributed.SlabComm.attach leaves itself here
        while done < total:
            n = min(check_every, total - done)
            if self.external_transport is not None:
                self.external_transport.run_steps(e, n)
            elif self.world > 1 and fresh and done == 0 and comm is not None and comm.transport == "auto":
                # Decomposed run, first timesteps: the probe of the halo transport the ranks agreed on.  One that set up (and passed
                # its self-test) but errors once timesteps depend on it — every halo wait is bounded — sends ALL ranks to the next
                # transport (p2p -> rccl -> host): new contexts, from the initial state.
                # What failed decides what happens, and every rank does the same (one all-reduce of a code):
                #   1  a SCHEDULE error (a flag wait of the one-launch schedule ran out): same transport, two launches per timestep;
                #   2  a TRANSPORT error (a halo wait ran out, the transport is refused on this topology, an RCCL error): the next transport;
                #   3  anything else (out of memory, a bad argument, a device fault): raised, on every rank — not papered over.
                code, why = 0, ""
                try:
                    e.run(n)
                except _capi.FdtdError as exc:
                    why = str(exc)
                    low = why.lower()
                    code = 1 if "wavefront schedule" in low else 2 if ("p2p" in low or "nccl" in low or "rccl" in low) else 3
                worst = int(round(float(np.max(comm.allreduce_max(np.array([float(code)]))))))
                if worst == 3:
                    raise _capi.FdtdError(why or f"rank {self.rank}: another rank's engine failed in the first timesteps of the decomposed run")
                if worst:
                    log(f"[fdtd-hip rank {self.rank}] {'one-launch schedule' if worst == 1 else 'halo transport ' + str(comm.transport_used)} failed at run time"
                        + (f" ({why})" if why else "") + (" — every rank repeats under two launches per timestep" if worst == 1 else " — every rank takes the next one"))
                    if worst == 1:
                        stats.schedule_fallback = why or "another rank's one-launch schedule timed out"
                        self._build_flags = (self._build_flags & ~_capi.FLAG_KERNEL_MASK) | _capi.FLAG_KERNEL_DIRECT
                    else:
                        stats.transports_failed += (comm.transport_used,)
                        stats.transport_failure_reasons += (why or "failed on another rank",)
                        comm.skip.add(comm.transport_used)
                    comm.barrier()                  # nobody frees a mailbox a neighbour may still write into
                    e.close()
                    e = self.build(self.lib, rank=self.rank, world=self.world, device=self.device, partition=self.partition,
                                   flags=self._build_flags)
                    comm.attach(self)
                    emax = 0.0
                    continue
            else:
                try:
                    e.run(n)
                except _capi.FdtdError as exc:
                    # The one-launch-per-timestep schedule depends on workgroups being dispatched in order; a block that
                    # waits too long for an earlier block's flag sets an error word and the run comes back invalid
                    # (never a hang).  Heal it here: a new context under the two-launch schedule (no flags, no
                    # dependence on dispatch order), same process, from the initial state — once.
                    if not (fresh and self.world == 1 and ("wavefront schedule" in str(exc) or "resident schedule" in str(exc))
                            and stats.schedule_fallback is None):
                        raise
                    log(f"[fdtd-hip] {exc} — repeating the run under the two-launch schedule")
                    e.close()
                    e = self.build(self.lib, rank=self.rank, world=self.world, device=self.device, partition=self.partition,
                                   flags=(self._build_flags & ~_capi.FLAG_KERNEL_MASK) | _capi.FLAG_KERNEL_DIRECT)
                    stats.schedule_fallback = str(exc)
                    done, emax = 0, 0.0
                    continue
            done += n
            sv, si = e.energy()
            s = np.array([sv, si])
            if allreduce is not None:
                s = allreduce(s)
            en = EPS0 * s[0] + MU0 * s[1]
            emax = max(emax, en)
            ratio = en / emax if emax > 0 else 1.0
            stats.energy_db = 10.0 * np.log10(max(ratio, 1e-300))
            if verbose:
                el = time.perf_counter() - t0
                log(f"[fdtd-hip] step {done:6d}/{total}  energy {stats.energy_db:7.2f} dB  "
                    f"{self.grid.ncells * done / max(el, 1e-9) / 1e6:9.1f} MC/s")
            if self.end_criteria > 0 and done >= len(self.signal) and ratio < self.end_criteria:
                stats.stopped_by_energy = True
                break
        stats.steps = done
        stats.seconds = time.perf_counter() - t0
        stats.sheet_edges = 0 if self.sheets is None else len(self.sheets)
        stats.sheet_fit_error = self.sheet_fit_error
        stats.dispersion = self.dispersion_info()
        stats.lorentz = self.lorentz_info()
        stats.lumped = self.lumped_info()
        stats.magnetic = self.magnetic_info()
        stats.conformal = self.conformal_info()
        stats.subcell = self.subcell_info()
        stats.planewave = self.planewave_info()
        stats.anisotropic = self.anisotropic_info()
        stats.excitations = None if self.excite_lists is None else self.excite_lists.info
        stats.probes = [pl.info for pl in self.probes.values()] or None
        stats.fields = self._field_report if self.field_boxes else None  # Simulation.field fills in the seconds and device yes/no
        stats.sar = self._sar_report if self.sar_boxes else None      # Simulation.sar fills in the status counts and the averaging time
        stats.schedule = e.schedule_info()
        stats.mcells_per_s = self.grid.ncells * done / max(stats.seconds, 1e-9) / 1e6
        return stats

    # ---------------------------------------------------------------------------------------------
    def port_series(self, allreduce=None):
        """[(u(t), i(t))] per port; i is sampled half a step after u."""
        out = []
        for uid, iid in self._port_probe_ids:
            u, i = self.engine.get_probe(uid), self.engine.get_probe(iid)
            if allreduce is not None:
                u, i = allreduce(u), allreduce(i)
            out.append((u, i))
        return out

    def port_probe_series(self, allreduce=None):
        """[([u_A(t), ...], [i_1(t), ...])] per port: every V-probe and every I-probe of it (a lumped port has one of each)."""
        get = (lambda q: self.engine.get_probe(q)) if allreduce is None else (lambda q: allreduce(self.engine.get_probe(q)))
        return [([get(q) for q in uids], [get(q) for q in iids]) for uids, iids in self._port_probe_lists]

    def nf2ff_boxes(self, allreduce=None, freqs=None):
        """Frequency-domain surface data [nfreq][k][j][i] per recording request.  `freqs`: recorder mode only — any
        frequencies up to nf2ff_fmax (default: nf2ff_freqs); in dft mode the recorded set is returned."""
        if self.nf2ff_mode == "record":
            f = self.nf2ff_freqs if freqs is None else np.atleast_1d(np.asarray(freqs, float))
            if f.size and float(np.max(f)) > self.nf2ff_fmax * (1 + 1e-9):
                raise ValueError(f"NF2FF frequency {float(np.max(f)):g} Hz is above the recorder's band ({self.nf2ff_fmax:g} Hz)")
            tw_v = dft_twiddles(f, self.dt, self.dft_every, self.dft_nsamples, 0.0)
            tw_i = dft_twiddles(f, self.dt, self.dft_every, self.dft_nsamples, 0.5)
            boxes = self.nf2ff_box.collect(self.engine, self._nf_ids, tw_v, tw_i)
        else:
            if freqs is not None:
                raise ValueError("dft mode records nf2ff_freqs only")
            boxes = self.nf2ff_box.collect(self.engine, self._nf_ids)
        if allreduce is not None:
            boxes = [allreduce(b) for b in boxes]
        # single-sided spectra, as the port spectra of LumpedPort.CalcPort (2 dt sum u exp(-jwt): [EXT] openEMS's convention for both): with the
        # factor 2 on one side only, Prad / P_acc of a loss-free antenna reads 25 % (tests/test_tutorial_kat_cpu.py: power balance)
        scale = 2.0 * self.dt * self.dft_every
        return [b * scale for b in boxes]
