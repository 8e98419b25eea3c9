"""Host-side mirror of the openEMS / CSXCAD Python interface subset the reference drives.

The reference reaches its FDTD engine exclusively through these calls
(antenna_sim/solver_fdtd_openems_fixed.py:171-220,280,296 and the sibling solver files):

    FDTD = openEMS(NrTS=, EndCriteria=) ; FDTD.SetGaussExcite ; FDTD.SetBoundaryCond ; FDTD.SetCSX
    CSX = ContinuousStructure() ; mesh = CSX.GetGrid() ; mesh.SetDeltaUnit/AddLine/SmoothMeshLines
    CSX.AddMetal/AddMaterial(...).AddBox(...)[.AddTransform(...)]
    FDTD.AddEdges2Grid ; FDTD.AddLumpedPort ; FDTD.CreateNF2FFBox ; FDTD.Run
    nf2ff.CalcNF2FF(sim_path, f, theta_deg, phi_deg, center=) -> .E_norm[0], .Dmax[0], ...
    port.CalcPort(sim_path, f) -> .uf_inc, .uf_ref, ...        (microstrip.py:409-412)

Same names, argument meaning and result attributes — but ``Run`` time-steps on the MI355X through
libfdtd_hip.so (no XML, no HDF5 dumps, no second process) and ``CalcNF2FF`` evaluates the whole
theta x phi grid from device-accumulated DFT surfaces.  ``compat/openEMS`` and ``compat/CSXCAD`` re-export
this module under the upstream module names, so the reference's solver files run unmodified against
the HIP backend.  Every call is also appended to ``.calls`` in a canonical
vocabulary, which is how tests/ pin this layer against call lists captured from the reference.
"""
from __future__ import annotations

import json
import os
import shutil
import time
from typing import List, Optional, Sequence

import numpy as np

from . import constants
from .grid import RectGrid
from .mesher import mesh_hint_from_box, smooth_mesh_lines, unique_lines
from .scene import Scene, Box as SceneBox, voxelize
from . import primitives as _prims
from . import ports as _ports
from .simulation import Simulation, BoundarySpec
from .nf2ff import calc_nf2ff, NF2FFResult

_AX = {"x": 0, "y": 1, "z": 2, 0: 0, 1: 1, 2: 2}


def _plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, np.generic):
        return v.item()
    return v


class _CallLog:
    def __init__(self):
        self.calls: List[dict] = []

    def add(self, op, **kw):
        self.calls.append({"op": op, **{k: _plain(v) for k, v in kw.items()}})


# ---------------------------------------------------------------------------------------------------
# CSXCAD side
# ---------------------------------------------------------------------------------------------------
class CSRectGrid:
    def __init__(self, log: _CallLog):
        self._log = log
        self._unit = 1.0
        self._lines = [[], [], []]
        self.merge_fraction = None      # mesher.smooth_mesh_lines: None = the package default (100), 0 = keep every hint line as openEMS does
        self.merged_lines = [[], [], []]   # per axis: the (line, line) pairs SmoothMeshLines merged into one — where this mesh differs from openEMS's

    def SetDeltaUnit(self, unit):
        self._unit = float(unit)
        self._log.add("SetDeltaUnit", unit=unit)

    def GetDeltaUnit(self):
        return self._unit

    def AddLine(self, ny, lines):
        arr = np.atleast_1d(np.asarray(lines, dtype=float))
        self._lines[_AX[ny]].extend(arr.tolist())
        self._log.add("AddLine", axis="xyz"[_AX[ny]], lines=arr)

    def SetLines(self, ny, lines):
        self._lines[_AX[ny]] = list(np.atleast_1d(np.asarray(lines, dtype=float)))

    def GetLines(self, ny, do_sort=False):
        l = np.asarray(self._lines[_AX[ny]], dtype=float)
        return np.sort(l) if do_sort else l

    def GetQtyLines(self, ny):
        return len(self._lines[_AX[ny]])

    def SmoothMeshLines(self, ny, max_res, ratio=1.5):
        self._log.add("SmoothMeshLines", axis=ny if isinstance(ny, str) else "xyz"[ny], max_res=max_res, ratio=ratio)
        axes = range(3) if ny == "all" else [_AX[ny]]
        for a in axes:
            self._lines[a] = smooth_mesh_lines(self._lines[a], max_res, ratio, merge_fraction=self.merge_fraction,
                                               merged=self.merged_lines[a]).tolist()

    def Sort(self, ny="all"):
        for a in (range(3) if ny == "all" else [_AX[ny]]):
            self._lines[a] = unique_lines(self._lines[a]).tolist()


class _CSPrimitive:
    """What every primitive shares: its call-log entry, priority and transform."""

    def __init__(self, entry: dict, priority):
        self._entry = entry
        self.priority = int(priority)
        self.matrix = np.eye(4)

    def AddTransform(self, kind, *args):
        self._entry.setdefault("transforms", []).append([kind] + [_plain(a) for a in args])
        M = np.eye(4)
        if kind == "Translate":
            M[:3, 3] = np.asarray(args[0], dtype=float)
        elif kind == "RotateAxis":
            ax = _AX[args[0]]
            ang = np.deg2rad(float(args[1]))
            c, s = np.cos(ang), np.sin(ang)
            a1, a2 = (ax + 1) % 3, (ax + 2) % 3
            M[a1, a1] = c; M[a1, a2] = -s; M[a2, a1] = s; M[a2, a2] = c
        else:
            raise ValueError(f"transform '{kind}' is not supported by the HIP backend")
        self.matrix = M @ self.matrix      # applied in the order given, column-vector convention
        return self

    def GetPriority(self):
        return self.priority


class CSPrimBox(_CSPrimitive):
    def __init__(self, entry: dict, start, stop, priority):
        super().__init__(entry, priority)
        self.start = np.asarray(start, dtype=float)
        self.stop = np.asarray(stop, dtype=float)

    def GetStart(self):
        return self.start

    def GetStop(self):
        return self.stop


class CSPrimCurved(_CSPrimitive):
    """AddCylinder, AddCylindricalShell, AddSphere, AddSphericalShell, AddPolygon, AddLinPoly, AddCurve, AddWire: `kind` is the
    primitives.py class name, `prim` the validated primitive (drawing units, without the transform)."""

    def __init__(self, entry: dict, kind: str, priority, **kw):
        super().__init__(entry, priority)
        self.kind = kind
        self.prim = _prims.make(kind, priority, **kw)

    def to_scene(self):
        import copy
        pr = copy.copy(self.prim)
        pr.matrix = self.matrix.copy()
        return pr

    def bounding_box(self):
        """(start, stop) of the world-space bounding box, drawing units (what AddEdges2Grid takes the primitive by)."""
        pr = self.prim
        if self.kind in ("Sphere", "SphericalShell"):
            ext = pr.radius + 0.5 * getattr(pr, "shell_width", 0.0)
            lo, hi = np.asarray(pr.center) - ext, np.asarray(pr.center) + ext
        elif self.kind in ("Cylinder", "CylindricalShell"):
            # exact for an axis along a coordinate direction: the radius extends the two transverse axes only
            a, b = np.asarray(pr.start), np.asarray(pr.stop)
            ext = (pr.radius + 0.5 * getattr(pr, "shell_width", 0.0)) * np.ones(3)
            d = np.nonzero(a != b)[0]
            if d.size == 1 or (d.size == 0):
                ext[d[0] if d.size else 2] = 0.0
            lo, hi = np.minimum(a, b) - ext, np.maximum(a, b) + ext
        elif self.kind in ("Polygon", "LinPoly"):
            n = pr.norm_dir
            lo, hi = np.zeros(3), np.zeros(3)
            e1 = pr.elevation + getattr(pr, "length", 0.0)
            lo[n], hi[n] = min(pr.elevation, e1), max(pr.elevation, e1)
            for q, ax in enumerate(((n + 1) % 3, (n + 2) % 3)):
                lo[ax], hi[ax] = pr.points[q].min(), pr.points[q].max()
        else:
            r = getattr(pr, "radius", 0.0)
            lo, hi = pr.points.min(axis=1) - r, pr.points.max(axis=1) + r
        if not np.allclose(self.matrix, np.eye(4)):
            c = np.array([[x, y, z, 1.0] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]) @ self.matrix.T
            lo, hi = c[:, :3].min(axis=0), c[:, :3].max(axis=0)
        return lo, hi


class CSPrimPolyhedronReader(CSPrimCurved):
    """AddPolyhedronReader: a closed triangle mesh read from an STL file (stl.py), coordinates in the grid's drawing unit."""

    def __init__(self, entry: dict, filename, priority):
        _CSPrimitive.__init__(self, entry, priority)
        self.kind = "Polyhedron"
        self.prim = None
        self._filename = os.fspath(filename)
        self._error = None

    def GetFileName(self):
        return self._filename

    def SetFileName(self, filename):
        self._filename = os.fspath(filename)
        self._entry["filename"] = self._filename
        self.prim = None

    def ReadFile(self) -> bool:
        """Read the file now; False (as CSXCAD does) when it cannot be read — drawing the scene then raises with the reason."""
        from . import stl as _stl
        try:
            self.prim = _prims.make("Polyhedron", self.priority, triangles=_stl.read_stl(self._filename))
            self._error = None
        except ValueError as e:
            self.prim, self._error = None, str(e)
        return self.prim is not None

    def _need(self):
        if self.prim is None and not self.ReadFile():
            raise ValueError(f"AddPolyhedronReader: {self._error}")

    def to_scene(self):
        self._need()
        return super().to_scene()

    def bounding_box(self):
        self._need()
        pts = self.prim.triangles.reshape(-1, 3)
        if not np.allclose(self.matrix, np.eye(4)):
            pts = pts @ self.matrix[:3, :3].T + self.matrix[:3, 3]
        return pts.min(axis=0), pts.max(axis=0)


class CSProperty:
    def __init__(self, log: _CallLog, kind: str, name: str, **kw):
        self._log, self.kind, self.name = log, kind, name
        self.params = dict(kw)
        self.boxes: List[CSPrimBox] = []
        log.add("Add" + kind, name=name, **kw)

    def GetName(self):
        return self.name

    def AddBox(self, start=None, stop=None, priority=0, **kw):
        self._log.add("AddBox", prop=self.name, priority=priority, start=list(start), stop=list(stop))
        b = CSPrimBox(self._log.calls[-1], start, stop, priority)
        self.boxes.append(b)
        return b

    # -- the curved and polygonal primitives (primitives.py), CSXCAD's argument names; `boxes` keeps the drawing order of all ------
    def _add(self, kind, priority, **kw):
        if kind in ("Curve", "Wire") and self.kind != "Metal":
            raise ValueError(f"Add{kind} on {self.kind} '{self.name}': curves and wires are for metals (AddMetal) only")
        if self.kind == "LumpedElement":
            raise ValueError(f"Add{kind} on lumped element '{self.name}': lumped elements take boxes only")
        self._log.add("Add" + kind, prop=self.name, priority=priority, **kw)
        b = CSPrimCurved(self._log.calls[-1], kind, priority, **kw)
        self.boxes.append(b)
        return b

    def AddCylinder(self, start, stop, radius, priority=0, **kw):
        return self._add("Cylinder", priority, start=list(start), stop=list(stop), radius=radius)

    def AddCylindricalShell(self, start, stop, radius, shell_width, priority=0, **kw):
        return self._add("CylindricalShell", priority, start=list(start), stop=list(stop), radius=radius, shell_width=shell_width)

    def AddSphere(self, center, radius, priority=0, **kw):
        return self._add("Sphere", priority, center=list(center), radius=radius)

    def AddSphericalShell(self, center, radius, shell_width, priority=0, **kw):
        return self._add("SphericalShell", priority, center=list(center), radius=radius, shell_width=shell_width)

    def AddPolygon(self, points, norm_dir, elevation, priority=0, **kw):
        return self._add("Polygon", priority, points=np.asarray(points, float), norm_dir=_AX[norm_dir], elevation=elevation)

    def AddLinPoly(self, points, norm_dir, elevation, length, priority=0, **kw):
        return self._add("LinPoly", priority, points=np.asarray(points, float), norm_dir=_AX[norm_dir], elevation=elevation, length=length)

    def AddCurve(self, points, priority=0, **kw):
        return self._add("Curve", priority, points=np.asarray(points, float))

    def AddWire(self, points, radius, priority=0, **kw):
        return self._add("Wire", priority, points=np.asarray(points, float), radius=radius)

    def AddPolyhedronReader(self, filename, priority=0, **kw):
        """A solid from an STL file (binary or ASCII); call ReadFile() on the result, as with CSXCAD (drawing the scene reads a file
        that was not read yet)."""
        if self.kind == "ConductingSheet":
            raise ValueError(f"AddPolyhedronReader on {self.kind} '{self.name}': polyhedra are for materials and metals (AddMetal) only")
        if self.kind == "LumpedElement":
            raise ValueError(f"AddPolyhedronReader on lumped element '{self.name}': lumped elements take boxes only")
        ft = kw.get("file_type")
        if ft is not None and not (isinstance(ft, str) and ft.lower() in ("stl", "stl_file")) and ft != 1:
            raise ValueError(f"AddPolyhedronReader '{filename}': file_type {ft!r} is not supported by the HIP backend: STL only (no PLY)")
        if ft is None and os.path.splitext(os.fspath(filename))[1].lower() != ".stl":
            raise ValueError(f"AddPolyhedronReader '{filename}': the file type is taken from the extension, and only .stl is supported "
                             f"(pass file_type='STL' for an STL file of another name)")
        self._log.add("AddPolyhedronReader", prop=self.name, priority=priority, filename=os.fspath(filename))
        b = CSPrimPolyhedronReader(self._log.calls[-1], filename, priority)
        self.boxes.append(b)
        return b

    def _out_of_scope(self, what):
        raise ValueError(f"{what} is not supported by the HIP backend: out of scope (boxes, cylinders, spheres, shells, polygons, "
                         f"curves and wires are)")

    def AddRotPoly(self, *a, **kw):
        self._out_of_scope("AddRotPoly")

    def AddPolyhedron(self, *a, **kw):
        self._out_of_scope("AddPolyhedron")

    def AddMultiBox(self, *a, **kw):
        self._out_of_scope("AddMultiBox")


class CSPropMaterial(CSProperty):
    """What ContinuousStructure.AddMaterial returns, with CSXCAD's CSPropMaterial calls: SetMaterialProperty / GetMaterialProperty,
    SetIsotropy / GetIsotropy.  ``epsilon`` and ``kappa`` take one value or three, (x, y, z): an anisotropic dielectric with a diagonal
    tensor along the grid axes (scene.Scene.add_material); three values imply anisotropy, as upstream.  ``mue`` and ``sigma`` stay
    isotropic (a sequence is refused when the scene is drawn, as before)."""
    _AXES_OK = ("epsilon", "kappa")

    def __init__(self, log: _CallLog, name: str, **kw):
        kw = {k: self._value(name, k, v) for k, v in kw.items()}
        super().__init__(log, "Material", name, **kw)
        self._isotropic = not any(isinstance(kw.get(k), list) for k in self._AXES_OK)

    @classmethod
    def _value(cls, name, key, v):
        """One value as it was given; three values of epsilon / kappa as a list of floats, anything else refused by name."""
        if key not in cls._AXES_OK or np.ndim(v) == 0:
            return v
        try:
            out = [float(x) for x in np.asarray(v, float).reshape(-1)] if np.ndim(v) == 1 else []
        except (TypeError, ValueError):
            out = []
        if len(out) != 3 or not all(np.isfinite(x) for x in out):
            raise ValueError(f"material '{name}': {key} = {v!r} must be one value or three finite values (x, y, z)")
        return out

    def SetMaterialProperty(self, **kw):
        kw = {k: self._value(self.name, k, v) for k, v in kw.items()}
        self._log.add("SetMaterialProperty", prop=self.name, **kw)
        self.params.update(kw)
        if any(isinstance(kw.get(k), list) for k in self._AXES_OK):
            self._isotropic = False

    def GetMaterialProperty(self, prop_name):
        """The value as set: one number, or a (3,) array for an anisotropic epsilon / kappa; CSXCAD's defaults where nothing was set."""
        if prop_name not in ("epsilon", "mue", "kappa", "sigma", "density"):
            raise ValueError(f"material '{self.name}': unknown material property {prop_name!r}")
        v = self.params.get(prop_name, 1.0 if prop_name in ("epsilon", "mue") else 0.0)
        return np.array(v, float) if isinstance(v, list) else v

    def SetIsotropy(self, val):
        val = bool(val)
        if val:
            for k in self._AXES_OK:
                v = self.params.get(k)
                if isinstance(v, list) and not (v[0] == v[1] == v[2]):
                    raise ValueError(f"material '{self.name}': SetIsotropy(True) with {k} = {v}: the three values differ — set one value "
                                     f"first (SetMaterialProperty({k}=...))")
        self._log.add("SetIsotropy", prop=self.name, val=val)
        self._isotropic = val

    def GetIsotropy(self):
        return self._isotropic


class CSPropDiscMaterial(CSProperty):
    """What ContinuousStructure.AddDiscMaterial returns: a voxel body model (discmaterial.py); AddBox (with or without AddTransform)
    and the analytic solids delimit it, a polyhedron does not."""

    def __init__(self, log: _CallLog, name: str, vmap, filename):
        super().__init__(log, "DiscMaterial", name, filename=filename, scale=vmap.scale,
                         transform=None if vmap.matrix is None else vmap.matrix, use_db_background=vmap.use_db_background,
                         voxels=list(vmap.shape), db_size=vmap.db_size)
        self.vmap = vmap

    def _add(self, kind, priority, **kw):
        if kind in ("Polygon",):
            raise ValueError(f"Add{kind} on disc material '{self.name}': a flat polygon holds no cell")
        return super()._add(kind, priority, **kw)

    def AddPolyhedronReader(self, filename, priority=0, **kw):
        raise ValueError(f"AddPolyhedronReader on disc material '{self.name}': a polyhedron cannot delimit a voxel map (boxes and the "
                         f"analytic solids can)")


class CSExcitation(CSProperty):
    """What ContinuousStructure.AddExcitation returns: a plane wave (excitation type 10) on the box given with AddBox."""

    def __init__(self, log: _CallLog, name: str, exc_type: int, exc_val, delay: float):
        super().__init__(log, "Excitation", name, exc_type=int(exc_type), exc_val=[float(v) for v in exc_val], delay=float(delay))
        self.params["prop_dir"] = None

    def SetPropagationDir(self, val):
        d = [float(v) for v in np.atleast_1d(val)]
        if len(d) != 3:
            raise ValueError(f"excitation '{self.name}': SetPropagationDir takes three values")
        self._log.add("SetPropagationDir", prop=self.name, val=d)
        self.params["prop_dir"] = d

    def SetWeightFunction(self, func):
        raise ValueError(f"excitation '{self.name}': SetWeightFunction is not supported by the HIP backend: out of scope — a plane wave has "
                         f"one amplitude over its box")

    def AddBox(self, start=None, stop=None, priority=0, **kw):
        if self.boxes:
            raise ValueError(f"excitation '{self.name}': one box per plane wave (several boxes are not supported)")
        return super().AddBox(start, stop, priority, **kw)

    def _add(self, kind, priority, **kw):
        raise ValueError(f"Add{kind} on excitation '{self.name}': a plane wave takes one box only")


class CSProbe(CSProperty):
    """What ContinuousStructure.AddProbe returns: a stand-alone probe (probes.py), placed by one AddBox(start, stop)."""

    def __init__(self, log: _CallLog, spec):
        fn = spec.mode_function
        super().__init__(log, "Probe", spec.name, p_type=spec.p_type, weight=spec.weight, norm_dir=spec.norm_dir,
                         mode_function=None if fn is None else [getattr(f, "expression", None) or repr(f) for f in fn])
        self.spec = spec

    def AddBox(self, start=None, stop=None, priority=0, **kw):
        if self.boxes:
            raise ValueError(f"probe '{self.name}': one box per probe")
        b = super().AddBox(start, stop, priority, **kw)
        self.spec.start, self.spec.stop = tuple(float(v) for v in start), tuple(float(v) for v in stop)
        return b

    def _add(self, kind, priority, **kw):
        raise ValueError(f"Add{kind} on probe '{self.name}': a probe takes one box only")


def _take(kw, names, numbered):
    """Per-pole values out of the keywords `kw` (popped): the first of `names` present, as a sequence — else the keywords of
    `numbered` with the suffixes _1, _2, ... as far as they go."""
    for n in names:
        if n in kw:
            return [float(v) for v in np.atleast_1d(kw.pop(n))]
    out, q = [], 1
    while any(f"{n}_{q}" in kw for n in numbered):
        out.append(float(next(kw.pop(f"{n}_{q}") for n in numbered if f"{n}_{q}" in kw)))
        q += 1
    return out


def _one(call, name, key, v):
    """`v` of a dispersive medium, which is isotropic by construction: three values are refused by name."""
    if np.ndim(v) != 0:
        raise ValueError(f"{call} '{name}': {key} = {v!r} must be one value: anisotropic dispersive media are not supported "
                         f"(AddMaterial takes three values)")
    return v


class ContinuousStructure:
    def __init__(self, log: Optional[_CallLog] = None):
        self._log = log or _CallLog()
        self._grid = CSRectGrid(self._log)
        self.properties: List[CSProperty] = []

    def GetGrid(self):
        return self._grid

    def AddMaterial(self, name, **kw):
        """``epsilon``, ``kappa``: one value or three (x, y, z) — an anisotropic dielectric (CSPropMaterial)."""
        p = CSPropMaterial(self._log, name, **kw)
        self.properties.append(p)
        return p

    def AddMetal(self, name):
        p = CSProperty(self._log, "Metal", name)
        self.properties.append(p)
        return p

    def AddConductingSheet(self, name, conductivity, thickness):
        """Metal of finite conductivity [S/m] and thickness [m]: its surface becomes a surface impedance (sheet.py)."""
        p = CSProperty(self._log, "ConductingSheet", name, conductivity=float(conductivity), thickness=float(thickness))
        self.properties.append(p)
        return p

    def AddLumpedElement(self, name, ny, caps=True, R=None, C=None, L=None, LEtype=0):
        """A lumped R-L-C element along direction ``ny`` (lumped.py), CSXCAD's call: ``LEtype`` 0 = R, L, C in parallel, 1 = in
        series; an absent part is None or NaN.  ``caps``: the two end planes of a box with a cross-section become PEC.  ``AddBox``
        on the returned property places it."""
        from .lumped import Element
        spec = Element(str(name), R, L, C, int(LEtype))          # validates (negative, non-finite, shorts)

        def val(v):
            return None if v is None else float(v)
        R, L, C = spec.R, spec.L, spec.C
        p = CSProperty(self._log, "LumpedElement", name, ny=_AX[ny], caps=bool(caps), R=val(R), C=val(C), L=val(L), LEtype=int(LEtype))
        self.properties.append(p)
        return p

    def AddDebyeMaterial(self, name, **kw):
        """A multi-pole Debye medium (dispersion.py), mirroring CSXCAD's Debye material property: ``order`` = K poles, ``epsilon``
        = eps_inf, ``kappa``, and per pole the permittivity step and the relaxation time [s] — as sequences (``eps_delta``,
        ``eps_relax_time``) or numbered from 1 (``eps_delta_1``, ``eps_relaxtime_1`` ...).  Aliases: ``eps_inf``; ``delta_eps``,
        ``epsDelta``; ``tau``, ``eps_relaxtime``, ``epsRelaxTime``.  (The keyword spelling is not pinned against a CSXCAD install.)"""
        kw = dict(kw)
        take = lambda names, numbered: _take(kw, names, numbered)
        deps = take(("eps_delta", "delta_eps", "epsDelta"), ("eps_delta", "delta_eps", "epsDelta"))
        tau = take(("eps_relax_time", "eps_relaxtime", "tau", "epsRelaxTime"), ("eps_relaxtime", "eps_relax_time", "tau", "epsRelaxTime"))
        order = int(kw.pop("order", len(deps)))
        eps_inf = float(_one("AddDebyeMaterial", name, "epsilon", kw.pop("epsilon", kw.pop("eps_inf", 1.0))))
        kappa = float(_one("AddDebyeMaterial", name, "kappa", kw.pop("kappa", 0.0)))
        density = kw.pop("density", None)
        if kw:
            raise TypeError(f"AddDebyeMaterial: unknown keyword(s) {sorted(kw)}")
        if not (1 <= order <= 8) or len(deps) != order or len(tau) != order:
            raise ValueError(f"AddDebyeMaterial: order {order} needs {order} permittivity steps and relaxation times (1..8 poles), got {len(deps)} and {len(tau)}")
        p = CSProperty(self._log, "DebyeMaterial", name, order=order, epsilon=eps_inf, kappa=kappa, eps_delta=deps, eps_relax_time=tau,
                       **({} if density is None else {"density": density}))
        self.properties.append(p)
        return p

    def AddLorentzMaterial(self, name, **kw):
        """Lorentz and Drude poles (lorentz.py), mirroring CSXCAD's Lorentz material property with openEMS's keywords: ``order`` =
        K poles (1..4), ``epsilon`` = eps_inf (the prefactor of the pole sum as well), ``kappa``, and per pole the plasma frequency
        ``eps_plasma`` [Hz], the pole frequency ``eps_pole_freq`` [Hz] (0 or absent: a Drude pole) and the relaxation time
        ``eps_relax`` [s] (0 or absent: a loss-free pole).  Further poles: each keyword as a sequence, or the first pole bare and the
        others numbered from 1 (``eps_plasma_1`` ...).  Magnetic poles (``mue_plasma`` ...) and ``mue`` != 1 are refused."""
        kw = dict(kw)
        mag = sorted(k for k in kw if k.startswith(("mue_plasma", "mue_pole_freq", "mue_relax")))
        if mag:
            raise ValueError(f"AddLorentzMaterial '{name}': magnetic poles ({', '.join(mag)}) are not supported: magnetic dispersion is out of scope")
        mue = kw.pop("mue", 1.0)
        if np.ndim(mue) != 0 or float(mue) != 1.0:
            raise ValueError(f"AddLorentzMaterial '{name}': mue = {mue!r} is not supported on a Lorentz material (mue must be 1)")
        per_pole = lambda n: _take(kw, (n,), ()) + _take(kw, (), (n,))
        fp, f0, relax = per_pole("eps_plasma"), per_pole("eps_pole_freq"), per_pole("eps_relax")
        order = int(kw.pop("order", len(fp)))
        eps_inf = float(_one("AddLorentzMaterial", name, "epsilon", kw.pop("epsilon", 1.0)))
        kappa = float(_one("AddLorentzMaterial", name, "kappa", kw.pop("kappa", 0.0)))
        density = kw.pop("density", None)
        if kw:
            raise TypeError(f"AddLorentzMaterial: unknown keyword(s) {sorted(kw)}")
        if not (1 <= order <= 4) or len(fp) != order or len(f0) not in (0, order) or len(relax) not in (0, order):
            raise ValueError(f"AddLorentzMaterial: order {order} needs {order} plasma frequencies and, where given, as many pole frequencies "
                             f"and relaxation times (1..4 poles), got {len(fp)}, {len(f0)} and {len(relax)}")
        f0, relax = f0 or [0.0] * order, relax or [0.0] * order
        if any(t < 0 for t in relax):
            raise ValueError(f"AddLorentzMaterial '{name}': eps_relax must be >= 0 (0: a loss-free pole)")
        p = CSProperty(self._log, "LorentzMaterial", name, order=order, epsilon=eps_inf, kappa=kappa, eps_plasma=fp, eps_pole_freq=f0,
                       eps_relax=relax, **({} if density is None else {"density": density}))
        self.properties.append(p)
        return p

    def AddDiscMaterial(self, name, filename=None, scale=1.0, transform=None, use_db_background=False, **kw):
        """CSXCAD's discrete material (CSPropDiscMaterial): a segmented voxel phantom.  ``filename``: an .npz holding upstream's dataset
        names mesh_x, mesh_y, mesh_z, DiscData ([nz-1][ny-1][nx-1] uint8), epsR, kappa, density (optionally mueR and sigma, which must
        be 1 / 0) — an .h5 / .hdf5 file is refused (no HDF5 reader here; discmaterial.save_npz writes the .npz).  Without a file the
        same names are taken as keywords.  ``scale`` multiplies the map's mesh lines; ``transform``: a 4x4 matrix (map -> drawing
        coordinates) or a list of ["Translate", [..]] / ["RotateAxis", axis, degrees] steps; ``use_db_background``: voxels of index 0
        take table entry 0 instead of being transparent.  AddBox on the returned property delimits the phantom."""
        from . import discmaterial as _disc
        M = None
        if transform is not None:
            steps = not isinstance(transform, np.ndarray) and len(transform) > 0 and isinstance(transform[0][0], str)
            if not steps:
                M = np.asarray(transform, float)
            else:
                t = _CSPrimitive({}, 0)
                for step in transform:
                    t.AddTransform(step[0], *step[1:])
                M = t.matrix
        if filename is not None:
            if kw:
                raise TypeError(f"AddDiscMaterial '{name}': unknown keyword(s) {sorted(kw)} (a file was given)")
            vmap = _disc.load_npz(filename, name, scale, M, use_db_background)
        else:
            missing = [k for k in _disc.NPZ_KEYS if k not in kw]
            extra = sorted(set(kw) - set(_disc.NPZ_KEYS) - {"mueR", "sigma"})
            if missing or extra:
                raise TypeError(f"AddDiscMaterial '{name}': without a file the keywords {', '.join(_disc.NPZ_KEYS)} are needed"
                                + (f"; missing {missing}" if missing else "") + (f"; unknown {extra}" if extra else ""))
            vmap = _disc.make_map(name, (kw["mesh_x"], kw["mesh_y"], kw["mesh_z"]), kw["DiscData"], kw["epsR"], kw["kappa"], kw["density"],
                                  scale, M, use_db_background, mue_r=kw.get("mueR"), sigma=kw.get("sigma"))
        if sum(q.kind == "DiscMaterial" for q in self.properties) >= _disc.MAX_MAPS:
            raise ValueError(f"AddDiscMaterial '{name}': a structure takes at most {_disc.MAX_MAPS} voxel maps")
        p = CSPropDiscMaterial(self._log, name, vmap, None if filename is None else os.fspath(filename))
        self.properties.append(p)
        return p

    def AddExcitation(self, name, exc_type, exc_val, delay=0):
        """CSXCAD's excitation property, for the plane wave only: ``exc_type`` 10 with ``exc_val`` = E0 [V/m]; ``SetPropagationDir``
        and one ``AddBox`` on the returned property give the direction and the total-field box (planewave.py).  The field
        excitations (types 0..3) are refused: a structure is fed through ``openEMS.AddLumpedPort``."""
        if exc_type in (0, 1, 2, 3):
            raise ValueError(f"AddExcitation '{name}': exc_type {exc_type} (a field excitation) is not supported by the HIP backend: out of scope "
                             f"— feed the structure through a lumped port (openEMS.AddLumpedPort), or use exc_type 10 (plane wave)")
        if exc_type != 10:
            raise ValueError(f"AddExcitation '{name}': exc_type {exc_type!r} is not supported by the HIP backend (10, the plane wave, is)")
        if np.size(exc_val) != 3:
            raise ValueError(f"AddExcitation '{name}': exc_val takes the three components of E0")
        if float(delay) != 0.0:
            raise ValueError(f"AddExcitation '{name}': delay = {delay!r} is not supported: the plane wave starts with the run")
        if any(p.kind == "Excitation" for p in self.properties):
            raise ValueError(f"AddExcitation '{name}': the structure already has a plane wave (one plane-wave box per scene)")
        p = CSExcitation(self._log, name, exc_type, np.asarray(exc_val, float).reshape(-1), delay)
        self.properties.append(p)
        return p

    def AddProbe(self, name, p_type, weight=1, norm_dir=None, mode_function=None):
        """CSXCAD's probe property (probes.py): ``p_type`` 0 voltage, 1 current, 2 E field, 3 H field, 10 / 11 mode-matching voltage /
        current (``mode_function``: three per-component callables (x, y, z) or strings, coordinates in drawing units).  One
        ``AddBox(start, stop)`` on the returned property places it; ``openEMS.GetProbe(name)`` returns its series after ``Run``,
        which also writes upstream's ASCII probe file ``name`` into sim_path."""
        from . import probes as _probes
        if any(p.kind == "Probe" and p.name == str(name) for p in self.properties):
            raise ValueError(f"AddProbe '{name}' is defined twice")
        p = CSProbe(self._log, _probes.make(name, p_type, weight, norm_dir, mode_function))
        self.properties.append(p)
        return p

    SAR_DUMP_MASS = {20: 0.0, 21: 1e-3, 22: 10e-3}      # dump_type -> averaging mass [kg] (20: local SAR)

    def AddDump(self, name, dump_type=0, frequency=None, **kw):
        """CSXCAD's dump box, for the SAR dump types only: ``dump_type`` 20 = local SAR, 21 = 1 g, 22 = 10 g averaged, at the
        frequencies ``frequency`` [Hz]; ``AddBox`` on the returned property places it (one box), ``openEMS.GetSAR(name)`` returns the
        result after ``Run`` (sar.SARResult; no HDF5 file is written).  ``sar_method``: "ieee" (default) or "simple".  Field dumps
        (every other dump_type) are refused here — they have their own entry point, ``openEMS.AddFieldDump``; other keywords
        (dump_mode, file_type ...) are logged and have no effect."""
        if dump_type not in self.SAR_DUMP_MASS:
            raise ValueError(f"AddDump '{name}': dump_type {dump_type!r} is not supported by the HIP backend: out of scope — field dumps are "
                             f"not supported (the SAR dump types 20, 21 and 22 are) by AddDump; the field dump types 0..3 and 10..13 have "
                             f"their own entry point, openEMS.AddFieldDump(name, dump_type, start, stop, ...)")
        f = [] if frequency is None else [float(v) for v in np.atleast_1d(frequency)]
        if not f or not all(np.isfinite(v) and v > 0 for v in f):
            raise ValueError(f"AddDump '{name}': a SAR dump needs frequency=[...] with values > 0")
        from .sar import METHODS
        method = kw.pop("sar_method", "ieee")
        if method not in METHODS:
            raise ValueError(f"AddDump '{name}': sar_method must be one of {sorted(METHODS)}, got {method!r}")
        p = CSProperty(self._log, "Dump", name, dump_type=int(dump_type), frequency=f, sar_method=method, **kw)
        self.properties.append(p)
        return p


# ---------------------------------------------------------------------------------------------------
# openEMS side
# ---------------------------------------------------------------------------------------------------
def _disc_summary(scene, grid, vox) -> dict:
    """Per voxel map of the scene, for the run dump: the cells it owns, and per tissue index how many of them and their mass
    [kg] (the sum of density x cell volume)."""
    out = {}
    dx, dy, dz = (np.diff(l) for l in grid.lines)
    vol = dz[:, None, None] * dy[None, :, None] * dx[None, None, :]
    for qi, m in enumerate(scene.materials):
        vmap = getattr(m, "vmap", None)
        if vmap is None:
            continue
        sel = (vox.cell_material == qi) & (vox.cell_voxel >= 0)
        tissue = vmap.data.reshape(-1)[vox.cell_voxel[sel]]
        cells = np.bincount(tissue, minlength=vmap.db_size)
        mass = np.bincount(tissue, weights=vmap.density[tissue] * vol[sel], minlength=vmap.db_size)
        out[m.name] = {"voxels": list(vmap.shape), "db_size": vmap.db_size, "use_db_background": bool(vmap.use_db_background),
                       "cells_owned": int(sel.sum()), "cells_per_index": cells.tolist(), "mass_kg_per_index": mass.tolist()}
    return out


class UIData:
    def __init__(self, t, val):
        self.ui_time = [np.asarray(t)]
        self.ui_val = [np.asarray(val)]


def dft_time2freq(t, val, freq, signal_type="pulse"):
    """Single-sided spectrum of a sampled pulse ([EXT] openEMS utilities.DFT_time2freq)."""
    t = np.asarray(t, float); val = np.asarray(val, float); freq = np.atleast_1d(np.asarray(freq, float))
    f_val = np.exp(-2j * np.pi * np.outer(freq, t)) @ val
    if signal_type == "pulse":
        f_val = f_val * (t[1] - t[0])
    else:
        f_val = f_val / t.size
    return 2.0 * f_val


def dft_uniform(freq, x, dt, block: int = 128):
    """sum_n x[n] exp(-2 pi j f n dt) for every f, for samples on a uniform time grid, without the len(freq) x len(x) matrix of
    complex exponentials (201 x 12 600 of them were 0.04 s of the 0.29 s plugin call of the reference's default scene):
    n = a * block + b, exp(-j w n dt) = exp(-j w a block dt) * exp(-j w b dt) — two small tables and one real matrix product."""
    freq = np.atleast_1d(np.asarray(freq, float))
    x = np.asarray(x, float)
    n = x.size
    na = (n + block - 1) // block
    xp = np.zeros(na * block)
    xp[:n] = x
    w = -2j * np.pi * freq * dt
    inner = np.exp(np.outer(w, np.arange(block)))            # [f][b]
    outer_ = np.exp(np.outer(w, np.arange(na) * block))       # [f][a]
    part = xp.reshape(na, block) @ inner.T                    # [a][f]
    return np.einsum("fa,af->f", outer_, part)


class LumpedPort:
    """Result side of AddLumpedPort: U/I time series -> incident / reflected waves (row a13 of
    SURVEY §8: the reference's S11 block, microstrip.py:407-426, dead upstream but specified)."""

    def __init__(self, fdtd, number, R, start, stop, exc_dir, excite):
        self._fdtd = fdtd
        self.number, self.R = number, float(R)
        self.start, self.stop = np.asarray(start, float), np.asarray(stop, float)
        self.exc_ny, self.excite = exc_dir, excite
        self.Z_ref = float(R)

    def CalcPort(self, sim_path, freq, ref_impedance=None, ref_plane_shift=None, signal_type="pulse"):
        u, i, dt = self._fdtd._port_series(self.number)
        self.freq = np.atleast_1d(np.asarray(freq, float))
        if ref_impedance is not None:
            self.Z_ref = ref_impedance
        tu = np.arange(u.size) * dt
        ti = (np.arange(i.size) + 0.5) * dt
        self.u_data, self.i_data = UIData(tu, u), UIData(ti, i)
        if u.size == i.size and u.size > 1:
            # uniform time grid: exp(-jw(t + dt/2)) = exp(-jwt) * exp(-jw dt/2), and exp(-jwt) factorised (dft_uniform)
            scale = 2.0 * (dt if signal_type == "pulse" else 1.0 / u.size)
            self.uf_tot = dft_uniform(self.freq, u, dt) * scale
            self.if_tot = dft_uniform(self.freq, i, dt) * np.exp(-1j * np.pi * self.freq * dt) * scale
        else:
            self.uf_tot = dft_time2freq(tu, u, self.freq, signal_type)
            self.if_tot = dft_time2freq(ti, i, self.freq, signal_type)
        self.uf_inc = 0.5 * (self.uf_tot + self.if_tot * self.Z_ref)
        self.if_inc = 0.5 * (self.if_tot + self.uf_tot / self.Z_ref)
        self.uf_ref = self.uf_tot - self.uf_inc
        self.if_ref = self.if_inc - self.if_tot
        self.P_inc = 0.5 * np.real(self.uf_inc * np.conj(self.if_inc))
        self.P_ref = 0.5 * np.real(self.uf_ref * np.conj(self.if_ref))
        self.P_acc = 0.5 * np.real(self.uf_tot * np.conj(self.if_tot))
        return self


class _ModalPort:
    """What WaveguidePort and MSLPort share: the spectra of the probe series (dft_uniform, the half-step phase on I, as
    LumpedPort.CalcPort) and the wave split with Z_ref and the reference-plane shift (ports.waves)."""

    def _spectra(self, freq, signal_type):
        us, is_, dt = self._fdtd._port_all_series(self.number)
        self.freq = np.atleast_1d(np.asarray(freq, float))
        scale = 2.0 * (dt if signal_type == "pulse" else 1.0 / us[0].size)
        uf = [dft_uniform(self.freq, u, dt) * scale for u in us]
        jf = [dft_uniform(self.freq, i, dt) * np.exp(-1j * np.pi * self.freq * dt) * scale for i in is_]
        return us, is_, dt, uf, jf

    def _finish(self, uf_tot, if_tot, ref_impedance, ref_plane_shift):
        self.Z_ref = self.ZL if ref_impedance is None else ref_impedance
        shift = None if ref_plane_shift is None else float(ref_plane_shift) * self._fdtd._csx.GetGrid().GetDeltaUnit()
        (self.uf_tot, self.if_tot, self.uf_inc, self.if_inc, self.uf_ref, self.if_ref) = _ports.waves(uf_tot, if_tot, self.Z_ref, self.beta, shift)
        self.P_inc = 0.5 * np.real(self.uf_inc * np.conj(self.if_inc))
        self.P_ref = 0.5 * np.real(self.uf_ref * np.conj(self.if_ref))
        self.P_acc = 0.5 * np.real(self.uf_tot * np.conj(self.if_tot))
        return self


class WaveguidePort(_ModalPort):
    """Result side of AddWaveGuidePort (ports.py): modal voltage and current -> incident / reflected waves with the analytic beta and
    ZL of the mode.  E_func, H_func: callables (x, y) -> (c_P, c_PP), metres from the box's minimum corner."""

    def __init__(self, fdtd, number, start, stop, p_dir, E_func, H_func, kc, excite, eps_r=1.0, mode=None):
        self._fdtd, self.number = fdtd, number
        self.start, self.stop = np.asarray(start, float), np.asarray(stop, float)
        self.exc_ny, self.excite = p_dir, excite
        self.E_func, self.H_func, self.kc, self.eps_r, self.mode = E_func, H_func, float(kc), float(eps_r), mode

    def _to_scene(self, sc, csx_metals):
        sc.add_waveguide_port(self.number, self.start, self.stop, self.exc_ny, self.E_func, self.H_func, self.kc, self.excite, self.eps_r, mode=self.mode)

    def CalcPort(self, sim_path, freq, ref_impedance=None, ref_plane_shift=None, signal_type="pulse"):
        us, is_, dt, uf, jf = self._spectra(freq, signal_type)
        self.u_data, self.i_data = UIData(np.arange(us[0].size) * dt, us[0]), UIData((np.arange(is_[0].size) + 0.5) * dt, is_[0])
        self.beta, self.ZL = _ports.waveguide_beta_zl(self.freq, self.kc, self.eps_r)
        return self._finish(uf[0], jf[0], ref_impedance, ref_plane_shift)


class RectWGPort(WaveguidePort):
    """Result side of AddRectWaveGuidePort: the TEmn port of an a x b guide, built on the general waveguide port."""

    def __init__(self, fdtd, number, start, stop, p_dir, a, b, mode_name, excite, eps_r=1.0):
        e_func, h_func, kc = _ports.rect_te_mode(a, b, mode_name, f"rectangular waveguide port {number}")
        super().__init__(fdtd, number, start, stop, p_dir, e_func, h_func, kc, excite, eps_r, mode=str(mode_name).upper())
        self.a, self.b = float(a), float(b)


class MSLPort(_ModalPort):
    """Result side of AddMSLPort (ports.py): three voltages and two currents on the line -> beta and ZL extracted from the run, and the
    incident / reflected waves at the measurement plane (or shifted along the line)."""

    def __init__(self, fdtd, number, metal_prop, start, stop, prop_dir, exc_dir, excite, feed_shift, meas_plane_shift, feed_R, priority):
        self._fdtd, self.number, self.metal_prop = fdtd, number, metal_prop
        self.start, self.stop = np.asarray(start, float), np.asarray(stop, float)
        self.prop_ny, self.exc_ny, self.excite = prop_dir, exc_dir, excite
        self.feed_shift, self.measplane_shift, self.feed_R, self.priority = feed_shift, meas_plane_shift, feed_R, priority

    def _to_scene(self, sc, csx_metals):
        metal = csx_metals.get(id(self.metal_prop))
        if metal is None:
            raise ValueError(f"MSL port {self.number}: its metal property '{getattr(self.metal_prop, 'name', self.metal_prop)}' is not a metal of "
                             f"this structure (AddMetal / AddConductingSheet)")
        sc.add_msl_port(self.number, metal, self.start, self.stop, self.prop_ny, self.exc_ny, self.excite, self.feed_shift, self.measplane_shift,
                        self.feed_R, self.priority, add_strip=False)      # (AddMSLPort drew the strip into the CSX property)

    def CalcPort(self, sim_path, freq, ref_impedance=None, ref_plane_shift=None, signal_type="pulse"):
        us, is_, dt, uf, jf = self._spectra(freq, signal_type)
        self.u_data, self.i_data = UIData(np.arange(us[1].size) * dt, us[1]), UIData((np.arange(is_[0].size) + 0.5) * dt, 0.5 * (is_[0] + is_[1]))
        info = self._fdtd._port_info(self.number)
        Et, Ht, self.beta, self.ZL = _ports.msl_beta_zl(uf[0], uf[1], uf[2], jf[0], jf[1], info["dist_AC"], info["dist_loops"])
        return self._finish(Et, Ht, ref_impedance, ref_plane_shift)


class nf2ff:
    def __init__(self, fdtd, name="nf2ff", start=None, stop=None, directions=None, mirror=None, half_space=False):
        self._fdtd, self.name = fdtd, name
        self.start, self.stop = start, stop
        faces = ("x-", "x+", "y-", "y+", "z-", "z+")
        self.mirror = None
        if mirror is not None:
            self.mirror = [int(m) for m in mirror]
            if len(self.mirror) != 6 or any(m not in (0, 1, 2) for m in self.mirror):
                raise ValueError(f"NF2FF box '{name}': mirror takes six entries (x-, x+, y-, y+, z-, z+) of 0 (none), 1 (PEC) or 2 (PMC)")
            if not any(self.mirror):
                self.mirror = None
        self.half_space = bool(half_space)
        if self.half_space and self.mirror is None:
            raise ValueError(f"NF2FF box '{name}': half_space needs a PEC mirror plane, and there is no mirror")
        self.directions = None
        if directions is not None:
            self.directions = [bool(d) for d in directions]
            if len(self.directions) != 6:
                raise ValueError(f"NF2FF box '{name}': directions takes six entries (x-, x+, y-, y+, z-, z+)")
            # a box that is not closed by walls is not a Huygens surface: a face may be switched off only where a mirror stands
            for f, on in enumerate(self.directions):
                if not on and not (self.mirror is not None and self.mirror[f]):
                    raise ValueError(f"NF2FF box '{name}': directions switches face {faces[f]} off but no mirror stands there: "
                                     "an open box is no closed Huygens surface")

    def can_evaluate(self, freq) -> bool:
        """Whether CalcNF2FF can answer for `freq` after this run: any frequency inside the recorder's band when the faces
        were recorded in the time domain (the default) or when the running DFT took the comb it snaps to; else only the
        frequencies the running DFT accumulated."""
        sim = self._fdtd.sim
        if sim is None or sim.nf2ff_box is None:
            return False
        f = np.atleast_1d(np.asarray(freq, float))
        if sim.nf2ff_mode == "record":
            return bool(np.all(f <= sim.nf2ff_fmax * (1 + 1e-9)))
        if self._fdtd._nf2ff_snap:
            return True
        rec = np.asarray(sim.nf2ff_freqs, float)
        return bool(all(np.min(np.abs(rec - x)) <= 1e-6 * max(x, 1.0) for x in f))

    def CalcNF2FF(self, sim_path, freq, theta, phi, radius=1, center=(0, 0, 0), outfile=None,
                  read_cached=False, verbose=0):
        """theta/phi in DEGREES, center in metres (fixed.py:296).  Returns an object with the upstream
        attribute names; arrays are [frequency] lists of (ntheta, nphi).
        Multi-rank runs: Run() has already reduced the faces over the ranks for the excitation's centre frequency (and
        nf2ff_freqs), so a call for those is LOCAL and may be made on rank 0 alone, as upstream post-processing is.  Any
        OTHER frequency (time-domain recording) has to be transformed on every rank's slab first: such a call is a
        collective — every rank must make it, with the same frequencies."""
        return self._fdtd._calc_nf2ff(np.atleast_1d(np.asarray(freq, float)), np.atleast_1d(np.asarray(theta, float)),
                                      np.atleast_1d(np.asarray(phi, float)), float(radius),
                                      np.asarray(center, float))


def nf2ff_comb(f0: float, every: int = 10) -> np.ndarray:
    """Every `every`-th point of the reference's S11 grid linspace(max(1 GHz, 0.7 f0), 1.3 f0, 201)
    (solver_fdtd_openems_microstrip.py:408) plus f0 itself: what the NF2FF faces accumulate when the run is too
    long for time-domain recording and the caller named no frequencies."""
    f = np.linspace(max(1e9, 0.7 * f0), 1.3 * f0, 201)[::every]
    return np.unique(np.append(f, f0))


class openEMS:
    """FDTD front object.  Backend options beyond the upstream signature are keyword-only:
    n_gpus / rank / world (z-slab decomposition), device, cpml_cells (default: the _N of 'PML_N'),
    nf2ff_mode: 'auto' (default) records the NF2FF faces in the time domain in HBM when that fits the budget, so
    that CalcNF2FF can be asked for ANY frequency after the run, as upstream; otherwise / 'dft': running DFT at
    nf2ff_freqs (default then: a 21-point comb over the reference's S11 band, CalcNF2FF snaps to the nearest).
    conformal=True: conformal (Dey-Mittra) PEC boundaries on the surfaces of curved and slanted metals (conformal.py) instead of the
    bare staircase, every g_e = f_e / a_f bounded by conformal_ratio (R, default 2); a scene with cut faces then runs at
    courant_dt / sqrt(R).  The default False changes nothing.
    subcell=True: sub-cell averaged dielectric surfaces (subcell.py) — an edge that the surface of a curved or slanted dielectric
    crosses takes its permittivity and conductivity from subcell_samples (2, 4 or 8, default 4) sub-voxels per cell and axis instead of
    the staircase's four-cell mean; a scene whose dielectrics are boxes on mesh lines lists no edge and builds today's operator.  A
    scene with AddDiscMaterial is refused.  The default False changes nothing."""

    def __init__(self, NrTS=1e9, EndCriteria=1e-5, *, lib=None, device=0, rank=0, world=1, cpml_cells=None,
                 nf2ff_freqs=None, nf2ff_mode="auto", comm=None, conformal=False, conformal_ratio=2.0,
                 subcell=False, subcell_samples=4, **kw):
        self.calls_log = _CallLog()
        self.NrTS, self.EndCriteria = NrTS, EndCriteria
        self.calls_log.add("openEMS", NrTS=NrTS, EndCriteria=EndCriteria)
        self._lib, self._device, self._rank, self._world = lib, device, rank, world
        self._cpml_cells, self._nf2ff_freqs, self._comm = cpml_cells, nf2ff_freqs, comm
        self._nf2ff_mode, self._nf2ff_snap, self._box_cache = nf2ff_mode, False, {}
        self._conformal, self._conformal_ratio = bool(conformal), float(conformal_ratio)
        self._subcell, self._subcell_samples = bool(subcell), subcell_samples
        if self._subcell:
            from .subcell import check_nsub
            check_nsub(subcell_samples)
        self._csx: Optional[ContinuousStructure] = None
        self._bc = ["PEC"] * 6
        self._f0 = self._fc = None
        self._edge_hints = []
        self._ports: List[LumpedPort] = []      # LumpedPort, WaveguidePort and MSLPort, in the order they were added
        self._u_i_all = None
        self._nf2ff: Optional[nf2ff] = None
        self.sim: Optional[Simulation] = None
        self.stats = None
        self._sar = {}                 # (dump name, frequency) -> sar.SARResult of the last Run
        self._field_dumps = {}         # name -> the arguments of AddFieldDump
        self._fields = {}              # (dump name, frequency or timestep taken) -> fields.FieldDump of the last Run
        self._field_excitations = []   # field_excitation.FieldExcitation, in the order of AddFieldExcitation
        self._probes = {}              # probe name -> {"t", "val"} of the last Run

    @property
    def calls(self):
        return self.calls_log.calls

    # -- set-up ---------------------------------------------------------------------------------------
    def SetGaussExcite(self, f0, fc):
        self._f0, self._fc = float(f0), float(fc)
        self.calls_log.add("SetGaussExcite", f0=f0, fc=fc)

    def SetBoundaryCond(self, BC):
        self._bc = list(BC)
        self.calls_log.add("SetBoundaryCond", bc=list(BC))

    def SetCSX(self, CSX: ContinuousStructure):
        # one shared call log, in call order
        self.calls_log.calls.extend(CSX._log.calls)
        CSX._log = self.calls_log
        CSX._grid._log = self.calls_log
        for p in CSX.properties:
            p._log = self.calls_log
        self._csx = CSX

    def GetCSX(self):
        return self._csx

    def AddEdges2Grid(self, dirs, primitives=None, properties=None, **kw):
        mer = kw.get("metal_edge_res")
        self.calls_log.add("AddEdges2Grid", dirs=dirs, prop=getattr(properties, "name", None), metal_edge_res=mer)
        d = [_AX[c] for c in dirs] if isinstance(dirs, str) and dirs != "all" else ([0, 1, 2] if dirs == "all" else [_AX[c] for c in dirs])
        boxes = []
        if properties is not None:
            for p in (properties if isinstance(properties, (list, tuple)) else [properties]):
                boxes.extend(p.boxes)
        if primitives is not None:
            boxes.extend(primitives if isinstance(primitives, (list, tuple)) else [primitives])
        grid = self._csx.GetGrid()
        for b in boxes:
            if isinstance(b, CSPrimCurved):
                start, stop = b.bounding_box()      # a curved primitive is taken by its world-space bounding box
            elif not np.allclose(b.matrix, np.eye(4)):
                continue   # as upstream: edge hints cannot be derived for transformed primitives
            else:
                start, stop = b.start, b.stop
            hint = mesh_hint_from_box(start, stop, d, mer)
            for a in range(3):
                if hint[a]:
                    grid._lines[a].extend(hint[a])

    def AddLumpedPort(self, port_nr, R, start, stop, p_dir, excite=0, **kw):
        self.calls_log.add("AddLumpedPort", port_nr=port_nr, R=R, start=list(start), stop=list(stop), p_dir=p_dir,
                           excite=excite, priority=kw.get("priority", 0), edges2grid=kw.get("edges2grid"))
        port = LumpedPort(self, port_nr, R, start, stop, _AX[p_dir], excite)
        port.priority = kw.get("priority", 0)
        self._ports.append(port)
        e2g = kw.get("edges2grid")
        if e2g:
            dirs = [0, 1, 2] if e2g == "all" else [_AX[c] for c in e2g]
            hint = mesh_hint_from_box(start, stop, dirs, None)
            for a in range(3):
                if hint[a]:
                    self._csx.GetGrid()._lines[a].extend(hint[a])
        return port

    def AddWaveGuidePort(self, port_nr, start, stop, p_dir, E_func, H_func, kc, excite=0, **kw):
        """A modal port (ports.py): E_func, H_func Python callables (x, y) -> (c_P, c_PP), x and y in metres from the box's minimum
        corner along the axes (p + 1) % 3 and (p + 2) % 3; strings (upstream's weight functions) are refused.  eps_r= the filling."""
        self.calls_log.add("AddWaveGuidePort", port_nr=port_nr, start=list(start), stop=list(stop), p_dir=p_dir, kc=kc, excite=excite,
                           eps_r=kw.get("eps_r", 1.0))
        return self._add_waveguide(WaveguidePort(self, port_nr, start, stop, _AX[p_dir], E_func, H_func, kc, excite, kw.get("eps_r", 1.0)))

    def AddRectWaveGuidePort(self, port_nr, start, stop, p_dir, a, b, mode_name, excite=0, **kw):
        """The TEmn port of a rectangular guide, a and b in metres along (p + 1) % 3 and (p + 2) % 3; TM modes are refused."""
        self.calls_log.add("AddRectWaveGuidePort", port_nr=port_nr, start=list(start), stop=list(stop), p_dir=p_dir, a=a, b=b, mode_name=mode_name,
                           excite=excite, eps_r=kw.get("eps_r", 1.0))
        return self._add_waveguide(RectWGPort(self, port_nr, start, stop, _AX[p_dir], a, b, mode_name, excite, kw.get("eps_r", 1.0)))

    def _add_waveguide(self, port):
        who = f"waveguide port {port.number}"
        _ports.check_funcs(who, port.E_func, port.H_func)
        if port.start[port.exc_ny] == port.stop[port.exc_ny]:
            raise ValueError(f"{who}: start and stop coincide along {'xyz'[port.exc_ny]}: the port has no direction (d = 0)")
        self._ports.append(port)
        return port

    def AddMSLPort(self, port_nr, metal_prop, start, stop, prop_dir, exc_dir, excite=0, FeedShift=0, MeasPlaneShift=None, Feed_R=np.inf,
                   priority=0, **kw):
        """A microstrip-line port (ports.py): the strip, a zero-thickness box on the plane stop[exc_dir], is added to metal_prop here."""
        self.calls_log.add("AddMSLPort", port_nr=port_nr, metal=getattr(metal_prop, "name", None), start=list(start), stop=list(stop),
                           prop_dir=prop_dir, exc_dir=exc_dir, excite=excite, FeedShift=FeedShift, MeasPlaneShift=MeasPlaneShift,
                           Feed_R=None if Feed_R is None or not np.isfinite(Feed_R) else Feed_R, priority=priority)
        who = f"MSL port {port_nr}"
        if not isinstance(metal_prop, CSProperty) or metal_prop.kind not in ("Metal", "ConductingSheet"):
            raise ValueError(f"{who}: metal_prop must be a metal of the structure (AddMetal / AddConductingSheet)")
        port = MSLPort(self, port_nr, metal_prop, start, stop, _AX[prop_dir], _AX[exc_dir], excite, FeedShift, MeasPlaneShift,
                       np.inf if Feed_R is None else Feed_R, priority)
        if port.prop_ny == port.exc_ny:
            raise ValueError(f"{who}: the propagation and the excitation direction are both {'xyz'[port.prop_ny]}")
        for a in range(3):
            if port.start[a] == port.stop[a]:
                raise ValueError(f"{who}: its box has zero extent along {'xyz'[a]}")
        strip_start = port.start.copy()
        strip_start[port.exc_ny] = port.stop[port.exc_ny]
        metal_prop.AddBox(strip_start, port.stop, priority=priority)
        self._ports.append(port)
        return port

    def CreateNF2FFBox(self, name="nf2ff", start=None, stop=None, directions=None, mirror=None, half_space=False, **kw):
        """mirror: upstream's list of six (x-, x+, y-, y+, z-, z+) 0 / 1 (PEC) / 2 (PMC): that face is a symmetry wall of the run
        (SetBoundaryCond must name the same wall there) and the box is open on it; CalcNF2FF adds the mirror images
        (Simulation(nf2ff_mirror=)).  directions: six flags, a face may be switched off only where a mirror stands.  half_space:
        the one PEC mirror plane is an infinite ground plane (Simulation(nf2ff_half_space=))."""
        self.calls_log.add("CreateNF2FFBox")
        self._nf2ff = nf2ff(self, name, start, stop, directions=directions, mirror=mirror, half_space=half_space)
        return self._nf2ff

    def AddFieldDump(self, name, dump_type, start, stop, *, dump_mode=1, frequency=None, timesteps=None, sub_sampling=(1, 1, 1),
                     file_type=0):
        """A field dump box, start / stop in drawing units.  ``dump_type`` as upstream: 0 / 1 / 2 / 3 = E / H / J / rot-H in the time
        domain (``timesteps=[...]``: snapshots at the recorder's samples nearest to them), 10 / 11 / 12 / 13 the same in the
        frequency domain (``frequency=[...]`` in Hz).  ``dump_mode`` 0 raw, 1 node-interpolated, 2 cell-interpolated;
        ``sub_sampling`` keeps every s-th point per axis; ``file_type`` 0 writes one ASCII VTK rectilinear grid per frequency or
        snapshot into sim_path, 1 one .npz (no HDF5).  ``GetFieldDump(name)`` returns the result after ``Run`` (fields.FieldDump).
        CSX.AddDump keeps refusing these types: its boxes come by AddBox, after the call, and a scene is built from them."""
        from . import fields as _fields
        self.calls_log.add("AddFieldDump", name=name, dump_type=dump_type, start=list(start), stop=list(stop), dump_mode=dump_mode,
                           frequency=None if frequency is None else [float(v) for v in np.atleast_1d(frequency)],
                           timesteps=None if timesteps is None else [int(v) for v in np.atleast_1d(timesteps)],
                           sub_sampling=list(sub_sampling), file_type=file_type)
        if dump_type not in _fields.DUMP_TYPES:
            raise ValueError(f"AddFieldDump '{name}': dump_type {dump_type!r} is not a field dump type — "
                             + ", ".join(f"{t} ({n})" for t, n in sorted(_fields.DUMP_TYPE_NAMES.items()))
                             + "; the SAR dump types 20, 21 and 22 go through CSX.AddDump")
        if name in self._field_dumps:
            raise ValueError(f"AddFieldDump '{name}' is defined twice")
        kind, in_freq = _fields.DUMP_TYPES[dump_type]
        if frequency is not None and timesteps is not None:
            raise ValueError(f"AddFieldDump '{name}': takes frequency=[...] or timesteps=[...], not both")
        if in_freq and frequency is None:
            raise ValueError(f"AddFieldDump '{name}': dump_type {dump_type} ({_fields.DUMP_TYPE_NAMES[dump_type]}) is a frequency-domain dump and needs "
                             f"frequency=[...]" + (" (timesteps= belongs to the time-domain types 0..3)" if timesteps is not None else ""))
        if not in_freq and timesteps is None:
            raise ValueError(f"AddFieldDump '{name}': dump_type {dump_type} ({_fields.DUMP_TYPE_NAMES[dump_type]}) is a time-domain dump and needs "
                             f"timesteps=[...]" + (" (frequency= belongs to the frequency-domain types 10..13)" if frequency is not None else ""))
        if dump_mode not in (0, 1, 2):
            raise ValueError(f"AddFieldDump '{name}': dump_mode must be 0 (raw), 1 (node-interpolated) or 2 (cell-interpolated), got {dump_mode!r}")
        if file_type not in (0, 1):
            raise ValueError(f"AddFieldDump '{name}': file_type must be 0 (vtk) or 1 (npz; HDF5 is not written), got {file_type!r}")
        self._field_dumps[name] = dict(kind=kind, mode=int(dump_mode), start=np.asarray(start, float), stop=np.asarray(stop, float),
                                       freqs=None if frequency is None else [float(v) for v in np.atleast_1d(frequency)],
                                       timesteps=None if timesteps is None else [int(v) for v in np.atleast_1d(timesteps)],
                                       sub_sampling=tuple(sub_sampling), file_type=int(file_type), dump_type=int(dump_type))

    def AddFieldExcitation(self, name, exc_type, exc_val, start, stop, *, weight=None, delay=0, priority=0):
        """An E- or H-field excitation over a box, a plane, a line or a point, start / stop in drawing units (field_excitation.py).
        ``exc_type`` as upstream: 0 soft E, 1 hard E, 2 soft H, 3 hard H; ``exc_val`` the field vector; ``weight`` None, one callable
        (x, y, z) or three per-component callables or strings (upstream's weight functions; coordinates in drawing units); ``delay``
        in seconds.  CSX.AddExcitation keeps refusing these types, and CSExcitation.SetWeightFunction stays refused: its box and
        weights come after the call, and a scene is built from them."""
        from . import field_excitation as _fexc
        if any(e.name == str(name) for e in self._field_excitations):
            raise ValueError(f"AddFieldExcitation '{name}' is defined twice")
        ex = _fexc.make(name, exc_type, exc_val, start, stop, weight, delay, priority)
        self.calls_log.add("AddFieldExcitation", name=name, exc_type=exc_type, exc_val=[float(v) for v in ex.exc_val], start=list(ex.start),
                           stop=list(ex.stop), weight=[None if f is None else getattr(f, "expression", None) or repr(f) for f in ex.weight],
                           delay=float(delay), priority=int(priority))
        self._field_excitations.append(ex)
        return ex

    # -- run ------------------------------------------------------------------------------------------
    @staticmethod
    def _draw(m, b):
        m.boxes.append(SceneBox(tuple(b.start), tuple(b.stop), b.priority, b.matrix.copy()) if isinstance(b, CSPrimBox) else b.to_scene())

    def _build_scene(self):
        csx = self._csx
        unit = csx.GetGrid().GetDeltaUnit()
        lines = [unique_lines(csx.GetGrid()._lines[a]) * unit for a in range(3)]
        grid = RectGrid(*lines)
        sc = Scene(unit=unit)
        metals = {}                            # id of a CSX metal property -> the scene's metal (an MSL port names its strip's metal)
        for p in csx.properties:
            if p.kind == "LorentzMaterial":
                q = p.params
                m = sc.add_lorentz_material(p.name, q["epsilon"], q["kappa"], wp=[2 * np.pi * f for f in q["eps_plasma"]],
                                            w0=[2 * np.pi * f for f in q["eps_pole_freq"]], gamma=[1.0 / t if t else 0.0 for t in q["eps_relax"]],
                                            density=q.get("density", 0.0))
                for b in p.boxes:
                    self._draw(m, b)
            elif p.kind in ("Material", "DebyeMaterial"):
                m = (sc.add_material(p.name, p.params.get("epsilon", 1.0), p.params.get("kappa", 0.0),
                                     mu_r=p.params.get("mue", 1.0), sigma_m=p.params.get("sigma", 0.0),
                                     density=p.params.get("density", 0.0)) if p.kind == "Material" else
                     sc.add_debye_material(p.name, p.params["epsilon"], p.params["kappa"], p.params["eps_delta"], p.params["eps_relax_time"],
                                           density=p.params.get("density", 0.0)))
                if p.kind == "DebyeMaterial":
                    m.medium.fit_info = getattr(p, "fit_info", None)
                for b in p.boxes:
                    self._draw(m, b)
            elif p.kind == "DiscMaterial":
                m = sc.add_voxel_map(p.vmap)
                for b in p.boxes:
                    self._draw(m, b)
            elif p.kind == "Excitation":
                if p.params["prop_dir"] is None:
                    raise ValueError(f"excitation '{p.name}': a plane wave needs its direction (SetPropagationDir)")
                if len(p.boxes) != 1 or not np.allclose(p.boxes[0].matrix, np.eye(4)):
                    raise ValueError(f"excitation '{p.name}': takes exactly one box, without a transform")
                sc.add_plane_wave(p.name, p.params["exc_val"], p.params["prop_dir"]).add_box(p.boxes[0].start, p.boxes[0].stop)
            elif p.kind in ("Dump", "Probe"):
                continue                       # no part of the scene: Run hands the SAR boxes to Simulation.add_sar_box, the probes to add_probe
            elif p.kind == "LumpedElement":
                m = sc.add_lumped_element(p.name, p.params["ny"], R=p.params["R"], C=p.params["C"], L=p.params["L"],
                                          kind=p.params["LEtype"], caps=p.params["caps"])
                for b in p.boxes:
                    if not isinstance(b, CSPrimBox):
                        raise ValueError(f"lumped element '{p.name}': {b.kind} is not supported, lumped elements take boxes only")
                    if not np.allclose(b.matrix, np.eye(4)):
                        raise ValueError(f"lumped element '{p.name}': transforms of its boxes are not supported")
                    m.add_box(b.start, b.stop, b.priority)
            else:
                m = (sc.add_conducting_sheet(p.name, p.params["conductivity"], p.params["thickness"]) if p.kind == "ConductingSheet"
                     else sc.add_metal(p.name))
                metals[id(p)] = m
                for b in p.boxes:
                    self._draw(m, b)
        for port in self._ports:
            if isinstance(port, LumpedPort):
                sc.add_lumped_port(port.number, port.R, port.start, port.stop, port.exc_ny, port.excite, port.priority)
            else:
                port._to_scene(sc, metals)
        sc.field_excitations.extend(self._field_excitations)
        return grid, sc

    @staticmethod
    def _wipe_sim_path(sim_path):
        """cleanup=True, as upstream's engine does before a run (fixed.py:280): a pre-existing sim_path goes.  Never a
        directory this process runs in (or any of its parents), never a filesystem root."""
        path = os.path.realpath(sim_path)
        cwd = os.path.realpath(os.getcwd())
        if not os.path.isdir(path) or path == os.path.dirname(path) or cwd == path or cwd.startswith(path + os.sep):
            return
        shutil.rmtree(path, ignore_errors=True)

    def Run(self, sim_path, cleanup=False, setup_only=False, verbose=None, **kw):
        """Time-step on the GPU.  Blocks; ctypes releases the GIL so a GUI thread stays live
        (the reference calls this from one background thread, gui_app.py:2688-2690)."""
        from ._capi import load_hip_library, default_rasteriser, default_fractions, default_subcell
        self.calls_log.add("Run", verbose=verbose, cleanup=cleanup)
        if self._csx is None or self._f0 is None:
            raise RuntimeError("SetCSX and SetGaussExcite must be called before Run")
        if cleanup and sim_path and self._rank == 0:
            self._wipe_sim_path(sim_path)
        lib = self._lib or load_hip_library()
        grid, sc = self._build_scene()
        fractions = dict(conformal=True, device_fractions=default_fractions(lib, self._device)) if self._conformal else {}
        if self._subcell:
            fractions.update(subcell=int(self._subcell_samples), device_subcell=default_subcell(lib, self._device))
        vox = voxelize(sc, grid, rasteriser=default_rasteriser(lib, self._device), **fractions)
        bc = BoundarySpec.parse(self._bc, self._cpml_cells)
        freqs = None
        if self._nf2ff is not None:
            freqs = [self._f0] if self._nf2ff_freqs is None else list(self._nf2ff_freqs)

        dumps = [p for p in self._csx.properties if p.kind == "Dump"]
        dump_freqs = sorted({f for p in dumps for f in p.params["frequency"]} | {f for d in self._field_dumps.values() for f in d["freqs"] or []})

        def make(fr):
            if fr is not None and dump_freqs:          # a running DFT accumulates the SAR and field-dump frequencies too
                fr = np.unique(np.concatenate([np.atleast_1d(np.asarray(fr, float)), dump_freqs]))
            sim = Simulation(grid, vox, f0=self._f0, fc=self._fc, boundary=bc, nr_ts=int(min(self.NrTS, 2**31 - 2)),
                             end_criteria=float(self.EndCriteria), nf2ff_freqs=fr, nf2ff_mode=self._nf2ff_mode,
                             conformal=self._conformal, conformal_ratio=self._conformal_ratio,
                             subcell=self._subcell, subcell_samples=self._subcell_samples,
                             **({} if self._nf2ff is None or self._nf2ff.mirror is None
                                else dict(nf2ff_mirror=self._nf2ff.mirror, nf2ff_half_space=self._nf2ff.half_space)))
            for p in dumps:
                if len(p.boxes) != 1 or not isinstance(p.boxes[0], CSPrimBox) or not np.allclose(p.boxes[0].matrix, np.eye(4)):
                    raise ValueError(f"SAR dump '{p.name}': takes exactly one box, without a transform")
                b = p.boxes[0]
                sim.add_sar_box(p.name, b.start * grid_unit, b.stop * grid_unit, p.params["frequency"],
                                ContinuousStructure.SAR_DUMP_MASS[p.params["dump_type"]], p.params["sar_method"])
            for name, d in self._field_dumps.items():
                sim.add_field_box(name, d["start"] * grid_unit, d["stop"] * grid_unit, d["kind"], mode=d["mode"], freqs=d["freqs"],
                                  timesteps=d["timesteps"], sub_sampling=d["sub_sampling"])
            for p in self._csx.properties:
                if p.kind == "Probe":
                    sim.add_probe(p.spec, grid_unit)
            return sim
        grid_unit = self._csx.GetGrid().GetDeltaUnit()
        self.sim = make(freqs)
        self._nf2ff_snap, self._box_cache, self._sar, self._fields, self._probes = False, {}, {}, {}, {}
        if self._nf2ff is not None and self.sim.nf2ff_mode == "dft" and self._nf2ff_freqs is None:
            self.sim = make(nf2ff_comb(self._f0))     # no time-domain record: a comb, CalcNF2FF snaps to it
            self._nf2ff_snap = True
        self.sim.build(lib, rank=self._rank, world=self._world, device=self._device)
        if self._comm is not None:
            self._comm.attach(self.sim)
        if setup_only:
            return
        allreduce = self._comm.allreduce if self._comm is not None else None
        self.stats = self.sim.run(verbose=int(verbose or 0), allreduce=allreduce)
        self._u_i_all = self.sim.port_probe_series(allreduce)
        self._u_i = [(us[0], is_[0]) for us, is_ in self._u_i_all]      # (what Simulation.port_series gives: the first probe of each kind)
        self._allreduce = allreduce
        self._probes = {name: self.sim.probe_series(name, allreduce) for name in self.sim.probes}
        probe_report = [{**info, "file": info["name"], "samples": int(np.shape(self._probes[info["name"]]["val"])[-1])} for info in self.stats.probes or []]
        self._boxes = None
        if self._nf2ff is not None and self.sim.nf2ff_mode == "dft":
            self._boxes = self.sim.nf2ff_boxes(allreduce)
        elif self._nf2ff is not None and allreduce is not None:
            # several ranks, faces recorded in the time domain: transform and reduce the frequencies the caller is known to
            # ask for HERE, where every rank is, so that CalcNF2FF at those is local (rank 0 alone may post-process)
            f = np.asarray(freqs, float)
            self._box_cache = {tuple(float(x) for x in f): self.sim.nf2ff_boxes(allreduce, freqs=f)}
        # the SAR dumps, as upstream writes them during the run: every dump at each of its frequencies (stats.sar: counts and time)
        self._sar = {(p.name, f): self.sim.sar(p.name, f) for p in dumps for f in p.params["frequency"]}
        # the field dumps, likewise: every dump at each of its frequencies or snapshots; the files go into sim_path below
        field_report = {}
        for name, d in self._field_dumps.items():
            b = self.sim.field_boxes[name]
            if b["freqs"] is not None:
                got = [self.sim.field(name, freq=float(f)) for f in b["freqs"]]
                self._fields.update({(name, float(f)): r for f, r in zip(b["freqs"], got)})
            else:
                got = [self.sim.field(name, timestep=int(t)) for t in dict.fromkeys(int(t) for t in b["timesteps"])]
                self._fields.update({(name, int(r.timestep)): r for r in got})
            field_report[name] = {**self.stats.fields[name], "dump_type": d["dump_type"], "file_type": d["file_type"],
                                  "seconds": float(sum(r.seconds for r in got)), "device": all(r.device for r in got), "files": []}
        if sim_path and self._rank == 0:
            try:
                os.makedirs(sim_path, exist_ok=True)
                from . import fields as _fields
                for name, d in self._field_dumps.items():
                    got = [r for (n, _), r in self._fields.items() if n == name]
                    field_report[name]["files"] = [os.path.basename(f) for f in _fields.write(sim_path, got, d["file_type"])]
                nx, ny, nz = grid.shape
                with open(os.path.join(sim_path, "fdtd_hip_run.json"), "w") as fh:
                    json.dump({"grid": [nx, ny, nz], "cells": grid.ncells, "dt": self.sim.dt,
                               "steps": self.stats.steps, "seconds": self.stats.seconds,
                               "mcells_per_s": self.stats.mcells_per_s, "energy_db": float(self.stats.energy_db),
                               "operator": self.sim.operator_form, "n_gpus": self._world,
                               "halo_transport": getattr(self._comm, "transport_used", None),
                               "halo_transports_failed": list(self.stats.transports_failed),
                               "schedule_fallback": self.stats.schedule_fallback,
                               **({"ports": [{"number": q.port.number, **{k: v for k, v in q.info.items() if k not in ("dist_AC", "dist_loops", "meas_pos")}}
                                             for q in vox.ports if q.info is not None]} if any(q.info is not None for q in vox.ports) else {}),
                               **({"nf2ff": self._nf2ff_report()} if self._nf2ff is not None and self._nf2ff.mirror is not None else {}),
                               **({"sar": self.stats.sar} if self.stats.sar else {}),
                               **({"fields": field_report} if field_report else {}),
                               **({"excitations": self.stats.excitations} if self.stats.excitations else {}),
                               **({"probes": probe_report} if probe_report else {}),
                               **({"disc_materials": _disc_summary(sc, grid, vox)} if vox.cell_voxel is not None else {})}, fh)
                # the stand-alone probes as upstream's ASCII probe files: the time column, then the value column(s)
                for name, r in self._probes.items():
                    np.savetxt(os.path.join(sim_path, name), np.c_[r["t"], np.atleast_2d(r["val"]).T], fmt="%.17g",
                               header=f"probe '{name}' ({self.sim.probes[name].info['kind']}): t [s], value" + ("s x, y, z" if np.ndim(r["val"]) == 2 else ""))
                # a plane wave: the excitation signal as upstream's two-column `et` file (time, value), which its RCS post-processing
                # reads for the incident spectrum (P_rad of CalcNF2FF over the spectrum of et)
                if self.sim.plane_wave is not None:
                    sig = np.asarray(self.sim.signal, np.float64)
                    np.savetxt(os.path.join(sim_path, "et"), np.c_[np.arange(sig.size) * self.sim.dt, sig])
                # the port series as upstream's probe files (text): only on request — formatting them takes 0.03 s of a
                # 0.34 s call on the reference's default scene, and CalcPort reads the arrays, not the files
                if int(verbose or 0) > 0 or os.environ.get("FDTD_WRITE_PORT_FILES"):
                    for port, (u, i) in zip(self._ports, self._u_i):
                        np.savetxt(os.path.join(sim_path, f"port_ut{port.number}"), np.c_[np.arange(u.size) * self.sim.dt, u])
                        np.savetxt(os.path.join(sim_path, f"port_it{port.number}"), np.c_[(np.arange(i.size) + 0.5) * self.sim.dt, i])
            except OSError:
                pass

    # -- results --------------------------------------------------------------------------------------
    def _port_series(self, number):
        if self.sim is None:
            raise RuntimeError("Run() first")
        for port, (u, i) in zip(self._ports, self._u_i):
            if port.number == number:
                return u, i, self.sim.dt
        raise KeyError(number)

    def _port_all_series(self, number):
        """([u(t) of every V-probe], [i(t) of every I-probe], dt) of port `number`."""
        if self.sim is None or self._u_i_all is None:
            raise RuntimeError("Run() first")
        for port, (us, is_) in zip(self._ports, self._u_i_all):
            if port.number == number:
                return us, is_, self.sim.dt
        raise KeyError(number)

    def _port_info(self, number):
        for port, p in zip(self._ports, self.sim.vox.ports):
            if port.number == number:
                return p.info
        raise KeyError(number)

    def GetProbe(self, name):
        """{"t", "val"} of the probe `name` (CSX.AddProbe) of the last Run: val is 1-D, or [3][n] for the field types 2 and 3; t [s]
        carries the half-step for the current types 1, 3 and 11."""
        if self.sim is None or self.stats is None:
            raise RuntimeError("Run() first")
        if name not in self._probes:
            raise KeyError(f"no probe '{name}' (defined: {sorted(self._probes)})")
        return self._probes[name]

    def GetSAR(self, name, freq=None, normalise_to=None):
        """The result of the SAR dump `name` (AddDump, dump_type 20 / 21 / 22) at `freq` (default: its first frequency): a
        sar.SARResult.  normalise_to=P divides the SAR values and P_abs by P (CalcPort's P_acc at that frequency: SAR per watt)."""
        if self.sim is None or self.stats is None:
            raise RuntimeError("Run() first")
        dump = next((p for p in self._csx.properties if p.kind == "Dump" and p.name == name), None)
        if dump is None:
            raise KeyError(f"no SAR dump '{name}'")
        f = float(dump.params["frequency"][0] if freq is None else freq)
        if normalise_to is None and (name, f) in self._sar:
            return self._sar[(name, f)]
        return self.sim.sar(name, f, normalise_to=normalise_to)

    def GetFieldDump(self, name, freq=None, timestep=None):
        """The result of the field dump `name` (AddFieldDump): a fields.FieldDump at `freq` (default: the dump's first frequency) or
        at the recorder sample nearest to `timestep` (default: its first)."""
        if self.sim is None or self.stats is None:
            raise RuntimeError("Run() first")
        if name not in self._field_dumps:
            raise KeyError(f"no field dump '{name}'")
        b = self.sim.field_boxes[name]
        if b["freqs"] is not None and timestep is None:
            key = (name, float(b["freqs"][0] if freq is None else freq))
        elif b["freqs"] is None and freq is None:
            t = int(b["timesteps_asked"][0] if timestep is None else timestep)
            key = (name, int(np.clip((t + self.sim.dft_every // 2) // self.sim.dft_every, 0, self.sim.dft_nsamples - 1)) * self.sim.dft_every)
        else:
            key = None
        if key in self._fields:
            return self._fields[key]
        return self.sim.field(name, freq=freq, timestep=timestep)

    def _nf2ff_report(self) -> dict:
        """The NF2FF entry of fdtd_hip_run.json for a box with mirror planes: the open box in nodes and its planes in metres."""
        b = self.sim.nf2ff_box
        planes, half = b.mirror_planes((0.0, 0.0, 0.0))
        return {"name": self._nf2ff.name, "lo": list(b.lo), "hi": list(b.hi), "mirror": list(b.mirror),
                "planes": [{"axis": "xyz"[a], "type": "PEC" if t == 1 else "PMC", "coordinate": c, "half_space": q == half}
                           for q, (a, t, c) in enumerate(planes)],
                "power_factor": b.power_factor}

    def _calc_nf2ff(self, freq, theta_deg, phi_deg, radius, center):
        if self.sim is None or self._nf2ff is None or self.sim.nf2ff_box is None:
            raise RuntimeError("Run() with an NF2FF box first")
        lib = self.sim.lib
        if self.sim.nf2ff_mode == "record":
            # time-domain faces in HBM: transform them for exactly the frequencies asked for (as upstream's nf2ff does
            # with the dumps); cached, since the 3-D variants call once per phi (microstrip_3d.py:224-225)
            key = tuple(float(f) for f in freq)
            if key not in self._box_cache:
                hit = [k for k in self._box_cache if all(any(abs(f - g) <= 1e-9 * max(abs(g), 1.0) for g in k) for f in key)]
                if hit:      # a subset of what is cached (e.g. Run's reduced set): pick the rows
                    src = hit[0]
                    rows = [int(np.argmin(np.abs(np.asarray(src) - f))) for f in key]
                    self._box_cache[key] = [b[rows] for b in self._box_cache[src]]
                else:        # (with several ranks this is a collective: see CalcNF2FF)
                    self._box_cache = {key: self.sim.nf2ff_boxes(self._allreduce, freqs=freq)}
            boxes, f_used = self._box_cache[key], freq
        else:
            rec = self.sim.nf2ff_freqs
            idx = []
            for f in freq:
                k = int(np.argmin(np.abs(rec - f)))
                if abs(rec[k] - f) > 1e-6 * max(f, 1.0) and not self._nf2ff_snap:
                    raise ValueError(f"NF2FF frequency {f:g} Hz was not recorded (recorded: {rec.tolist()}); "
                                     "pass nf2ff_freqs=[...] or nf2ff_mode='record' to openEMS(...)")
                idx.append(k)
            boxes, f_used = [b[idx] for b in self._boxes], rec[idx]
        res = calc_nf2ff(lib, self.sim.nf2ff_box, boxes, f_used, np.deg2rad(theta_deg),
                         np.deg2rad(phi_deg), center, device=self._device)
        out = _NF2FFResults()
        out.theta, out.phi, out.r, out.freq = res.theta, res.phi, radius, res.freq
        out.Dmax = np.asarray(res.Dmax)
        out.Prad = np.asarray(res.Prad)
        out.E_theta = [e / radius for e in res.E_theta]
        out.E_phi = [e / radius for e in res.E_phi]
        out.E_norm = [e / radius for e in res.E_norm]
        out.E_cprh = [(et + 1j * ep) / np.sqrt(2.0) / radius for et, ep in zip(res.E_theta, res.E_phi)]
        out.E_cplh = [(et - 1j * ep) / np.sqrt(2.0) / radius for et, ep in zip(res.E_theta, res.E_phi)]
        out.P_rad = [u / radius ** 2 for u in res.P_rad]
        return out


class _NF2FFResults:
    pass


# upstream module layout: openEMS.openEMS, openEMS.physical_constants, CSXCAD.ContinuousStructure
class physical_constants:
    C0 = constants.C0
    MUE0 = constants.MU0
    EPS0 = constants.EPS0
    Z0 = constants.ETA0
