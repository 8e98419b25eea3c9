"""Scene description + voxeliser: what the reference builds through the CSXCAD/openEMS Python API
(``CSX.AddMaterial/AddMetal(...).AddBox``, ``FDTD.AddLumpedPort``, ``FDTD.CreateNF2FFBox`` —
antenna_sim/solver_fdtd_openems_fixed.py:176-220) kept as plain data, and its mapping onto the
Yee grid (what [EXT] openEMS does when ``FDTD.Run`` sets up its operator):

  * material boxes -> per-cell eps_r / kappa and mu_r / sigma_m (highest priority box containing the cell centre; the magnetic
    pair is turned into face coefficients by magnetic.py);
  * metal boxes (PEC, any thickness incl. zero) -> every edge with both end nodes inside is PEC;
  * conducting-sheet boxes (``add_conducting_sheet``: finite conductivity and thickness, sheet.py) -> the edges on the metal's
    surface become sheet edges (surface impedance, stepped by the engine); interior edges stay PEC.  Where metals overlap, the
    highest box priority wins, as for materials;
  * lumped port  -> per-edge conductance, soft-source edges, voltage line and current loop;
  * waveguide and microstrip-line ports (ports.py) -> one source list, V-probes and I-probes of the same kind, built once the metals are known;
  * lumped element (``add_lumped_element``: R, L, C in parallel or in series, lumped.py) -> the edges of its box along its
    direction, each with its share of the element; with ``caps`` the two end planes of a box with a cross-section become PEC.

Coordinates are in drawing units (``unit`` metres per unit, 1e-3 in every reference scene).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple
import numpy as np

from .grid import RectGrid
from .ecoperator import LumpedEdge
from . import sheet as _sheet
from . import dispersion as _disp
from . import lorentz as _lorentz
from . import lumped as _lumped
from . import magnetic as _magnetic
from . import conformal as _conformal
from . import subcell as _subcell
from . import primitives as _prims
from . import planewave as _planewave
from . import discmaterial as _discmaterial
from . import ports as _ports
from . import field_excitation as _fexc
from . import probes as _probes
from .ports import Probe, WaveguidePort, MSLPort


@dataclass
class Box:
    start: Tuple[float, float, float]
    stop: Tuple[float, float, float]
    priority: int = 0
    matrix: Optional[np.ndarray] = None   # 4x4 local->world (drawing units), None = identity


class _Drawable:
    """The drawing calls beyond add_box (primitives.py); `boxes` holds every primitive of the property in drawing order."""

    def _add(self, kind, priority, **kw):
        self.boxes.append(_prims.make(kind, priority, **kw))
        return self

    def add_cylinder(self, start, stop, radius, priority=0):
        return self._add("Cylinder", priority, start=start, stop=stop, radius=radius)

    def add_cylindrical_shell(self, start, stop, radius, shell_width, priority=0):
        return self._add("CylindricalShell", priority, start=start, stop=stop, radius=radius, shell_width=shell_width)

    def add_sphere(self, center, radius, priority=0):
        return self._add("Sphere", priority, center=center, radius=radius)

    def add_spherical_shell(self, center, radius, shell_width, priority=0):
        return self._add("SphericalShell", priority, center=center, radius=radius, shell_width=shell_width)

    def add_polygon(self, points, norm_dir, elevation, priority=0):
        return self._add("Polygon", priority, points=points, norm_dir=norm_dir, elevation=elevation)

    def add_lin_poly(self, points, norm_dir, elevation, length, priority=0):
        return self._add("LinPoly", priority, points=points, norm_dir=norm_dir, elevation=elevation, length=length)

    def add_polyhedron(self, triangles, priority=0):
        """A closed triangle mesh, triangles [ntri][3][3] in drawing units (stl.read_stl gives them)."""
        if isinstance(self, ConductingSheet):
            raise ValueError(f"conducting sheet '{self.name}': a polyhedron is for materials and plain metals (add_metal) only")
        return self._add("Polyhedron", priority, triangles=triangles)


@dataclass
class Material(_Drawable):
    name: str
    eps_r: float = 1.0
    kappa: float = 0.0
    boxes: List[Box] = field(default_factory=list)
    mu_r: float = 1.0        # relative permeability (>= 1) and magnetic loss sigma* [ohm/m]: magnetic.py
    sigma_m: float = 0.0
    density: float = 0.0     # [kg/m^3], 0: no tissue — what SAR divides by (sar.py)
    # anisotropic dielectric (a diagonal tensor): the (x, y, z) values, None for an isotropic quantity.  eps_r / kappa above then hold
    # the mean of the three — a scalar view for reports, which the operator never reads (ecoperator.build_operator reads the triple)
    eps_axes: Optional[Tuple[float, float, float]] = None
    kappa_axes: Optional[Tuple[float, float, float]] = None

    def add_box(self, start, stop, priority=0):
        self.boxes.append(Box(tuple(map(float, start)), tuple(map(float, stop)), int(priority)))
        return self

    @property
    def anisotropic(self) -> bool:
        return self.eps_axes is not None or self.kappa_axes is not None

    def axes(self):
        """((eps_x, eps_y, eps_z), (kappa_x, kappa_y, kappa_z)), whether the material is anisotropic or not."""
        return (self.eps_axes or (self.eps_r,) * 3, self.kappa_axes or (self.kappa,) * 3)


def _scalar_or_axes(name, what, value, positive):
    """(scalar view, triple or None) of a material value given as one number or as three (x, y, z).  One number is taken as it
    always was, float(value).  Three are checked: finite, and > 0 (`positive`) or >= 0; three equal values are the isotropic
    material.  Anything else is a ValueError naming the material."""
    if np.ndim(value) == 0:
        return float(value), None
    try:
        v = tuple(float(x) for x in np.asarray(value, float).reshape(-1)) if np.ndim(value) == 1 else ()
    except (TypeError, ValueError):
        v = ()
    if len(v) != 3:
        raise ValueError(f"material '{name}': {what} = {value!r} must be one value or three (x, y, z)")
    if not all(np.isfinite(x) and (x > 0 if positive else x >= 0) for x in v):
        raise ValueError(f"material '{name}': {what} = {value!r} must be finite and {'> 0' if positive else '>= 0'} on every axis")
    if v[0] == v[1] == v[2]:
        return v[0], None
    return (v[0] + v[1] + v[2]) / 3.0, v


def _one_value(name, kind, what, value):
    """`value` of a medium that is isotropic by construction; three values are refused by name."""
    if np.ndim(value) != 0:
        raise ValueError(f"{kind} material '{name}': {what} = {value!r} must be one value: anisotropic dispersive media are not supported "
                         f"(add_material takes three values)")
    return value


@dataclass
class DebyeMaterial(Material):
    """add_debye_material(name, eps_inf, kappa, delta_eps, tau): a multi-pole Debye medium (dispersion.py).  eps_r holds eps_inf."""
    medium: Optional[_disp.DebyeMedium] = None


@dataclass
class LorentzMaterial(Material):
    """add_lorentz_material(name, eps_inf, kappa, wp, w0, gamma): Lorentz / Drude poles (lorentz.py).  eps_r holds eps_inf."""
    medium: Optional[_lorentz.LorentzMedium] = None


@dataclass
class DiscMaterial(Material):
    """add_disc_material(name, lines, data, eps_r, kappa, density, ...): a voxel body model (discmaterial.py).  Its boxes and analytic
    solids delimit the map: such a primitive owns a cell whose centre it holds AND whose voxel is not the background (index 0), unless
    use_db_background.  eps_r / kappa / density of the material itself are those of table entry 0; a cell takes its voxel's."""
    vmap: Optional[_discmaterial.VoxelMap] = None

    def add_polyhedron(self, triangles, priority=0):
        raise ValueError(f"disc material '{self.name}': a polyhedron cannot delimit a voxel map (boxes and the analytic solids can)")


@dataclass
class Metal(_Drawable):
    name: str
    boxes: List[Box] = field(default_factory=list)

    def add_box(self, start, stop, priority=0):
        self.boxes.append(Box(tuple(map(float, start)), tuple(map(float, stop)), int(priority)))
        return self

    def _no_sheet(self, what):
        if isinstance(self, ConductingSheet):
            raise ValueError(f"conducting sheet '{self.name}': {what} is for plain metals (add_metal) only")

    def add_curve(self, points, priority=0):
        self._no_sheet("a curve")
        return self._add("Curve", priority, points=points)

    def add_wire(self, points, radius, priority=0):
        self._no_sheet("a wire")
        return self._add("Wire", priority, points=points, radius=radius)


@dataclass
class ConductingSheet(Metal):
    """AddConductingSheet(name, conductivity, thickness): a metal of finite conductivity [S/m] and thickness [m]."""
    conductivity: float = 5.8e7
    thickness: float = 35e-6


@dataclass
class LumpedPort:
    """AddLumpedPort(port_nr, R, start, stop, p_dir, excite, priority) as plain data."""
    number: int
    R: float
    start: Tuple[float, float, float]
    stop: Tuple[float, float, float]
    direction: int            # 0,1,2
    excite: float = 1.0
    priority: int = 5
    delay_steps: int = 0


@dataclass
class LumpedElement:
    """AddLumpedElement(name, ny, caps, R, C, L, LEtype) as plain data: `spec` holds the values and the kind (lumped.Element)."""
    name: str
    direction: int            # 0,1,2
    spec: _lumped.Element = None
    caps: bool = True
    boxes: List[Box] = field(default_factory=list)

    def add_box(self, start, stop, priority=0):
        self.boxes.append(Box(tuple(map(float, start)), tuple(map(float, stop)), int(priority)))
        return self


@dataclass
class PlaneWaveSource:
    """AddExcitation(name, 10, e0) + SetPropagationDir as plain data: a plane wave on a total-field / scattered-field box
    (planewave.py).  `spec` holds e0 (projected perpendicular to the direction) and the direction (normalised)."""
    name: str
    spec: _planewave.PlaneWave = None
    boxes: List[Box] = field(default_factory=list)

    def add_box(self, start, stop, priority=0):
        if self.boxes:
            raise ValueError(f"plane wave '{self.name}': one box per plane wave, and one plane wave per scene (several boxes are not supported)")
        self.boxes.append(Box(tuple(map(float, start)), tuple(map(float, stop)), int(priority)))
        return self


def _density(name, density) -> float:
    if np.ndim(density) != 0 or not (np.isfinite(float(density)) and float(density) >= 0):
        raise ValueError(f"material '{name}': density = {density!r} must be one finite value >= 0 [kg/m^3]")
    return float(density)


@dataclass
class Scene:
    unit: float = 1e-3
    materials: List[Material] = field(default_factory=list)
    metals: List[Metal] = field(default_factory=list)
    ports: List[LumpedPort] = field(default_factory=list)
    elements: List[LumpedElement] = field(default_factory=list)
    plane_waves: List[PlaneWaveSource] = field(default_factory=list)
    field_excitations: List["_fexc.FieldExcitation"] = field(default_factory=list)

    def add_material(self, name, eps_r=1.0, kappa=0.0, mu_r=1.0, sigma_m=0.0, density=0.0) -> Material:
        """mu_r >= 1 and sigma_m >= 0 (magnetic loss sigma* [ohm/m]) make the material magnetic (magnetic.py); anisotropic
        (sequence), negative or non-finite values and mu_r < 1 are refused.  density [kg/m^3] > 0 makes it tissue for SAR (sar.py).
        eps_r and kappa take one value or three, (x, y, z): an anisotropic dielectric with a diagonal tensor along the grid axes
        (ecoperator.build_operator: an edge of direction c sees eps_r[c] and kappa[c]).  Three values are finite, eps_r > 0, kappa >= 0."""
        _magnetic.check_material(name, mu_r, sigma_m)
        eps, eps_axes = _scalar_or_axes(name, "eps_r", eps_r, True)
        kap, kappa_axes = _scalar_or_axes(name, "kappa", kappa, False)
        m = Material(name, eps, kap, mu_r=float(mu_r), sigma_m=float(sigma_m), density=_density(name, density),
                     eps_axes=eps_axes, kappa_axes=kappa_axes)
        self.materials.append(m)
        return m

    def add_debye_material(self, name, eps_inf, kappa=0.0, delta_eps=(), tau=(), density=0.0) -> DebyeMaterial:
        """A dispersive dielectric eps(w) = eps_inf + sum_k delta_eps[k] / (1 + j w tau[k]) - j kappa / (w eps0), 1..8 poles.
        Boxes, rotations and priorities work as for add_material; the highest priority owns a cell."""
        med = _disp.DebyeMedium(_one_value(name, "Debye", "eps_inf", eps_inf), _one_value(name, "Debye", "kappa", kappa), delta_eps, tau)
        m = DebyeMaterial(name, med.eps_inf, med.kappa, medium=med, density=_density(name, density))
        self.materials.append(m)
        return m

    def add_lorentz_material(self, name, eps_inf, kappa=0.0, wp=(), w0=(), gamma=(), density=0.0) -> LorentzMaterial:
        """A resonant dielectric eps(w) = eps_inf (1 + sum_k wp[k]^2 / (w0[k]^2 - w^2 + j w gamma[k])) - j kappa / (w eps0), 1..4
        poles, all in rad/s; w0[k] = 0 (or w0 left out) is a Drude pole, gamma left out a loss-free one.  Boxes, rotations and
        priorities work as for add_material; the highest priority owns a cell."""
        med = _lorentz.LorentzMedium(_one_value(name, "Lorentz", "eps_inf", eps_inf), _one_value(name, "Lorentz", "kappa", kappa), wp, w0, gamma)
        m = LorentzMaterial(name, med.eps_inf, med.kappa, medium=med, density=_density(name, density))
        self.materials.append(m)
        return m

    def add_disc_material(self, name, lines, data, eps_r, kappa, density, scale=1.0, matrix=None, use_db_background=False) -> DiscMaterial:
        """A voxel body model: lines = (X, Y, Z) the map's mesh lines (its own drawing unit, times `scale` the scene's), data uint8
        [nZ-1][nY-1][nX-1] one tissue index per voxel, eps_r / kappa / density one value per tissue (entry 0: the background), matrix
        an optional 4x4 placement (map -> scene drawing coordinates).  add_box (or an analytic solid) on the result delimits it;
        voxels of index 0 are transparent unless use_db_background.  At most discmaterial.MAX_MAPS per scene."""
        vmap = _discmaterial.make_map(name, lines, data, eps_r, kappa, density, scale, matrix, use_db_background)
        return self.add_voxel_map(vmap)

    def add_voxel_map(self, vmap: "_discmaterial.VoxelMap") -> DiscMaterial:
        """add_disc_material for a map that is already validated (discmaterial.make_map / load_npz)."""
        if sum(isinstance(m, DiscMaterial) for m in self.materials) >= _discmaterial.MAX_MAPS:
            raise ValueError(f"disc material '{vmap.name}': a scene takes at most {_discmaterial.MAX_MAPS} voxel maps")
        m = DiscMaterial(vmap.name, float(vmap.eps_r[0]), float(vmap.kappa[0]), density=float(vmap.density[0]), vmap=vmap)
        self.materials.append(m)
        return m

    def add_metal(self, name) -> Metal:
        m = Metal(name)
        self.metals.append(m)
        return m

    def add_conducting_sheet(self, name, conductivity, thickness) -> ConductingSheet:
        if not (float(conductivity) > 0 and float(thickness) > 0):
            raise ValueError("a conducting sheet needs conductivity > 0 and thickness > 0")
        m = ConductingSheet(name, conductivity=float(conductivity), thickness=float(thickness))
        self.metals.append(m)
        return m

    def add_lumped_port(self, number, R, start, stop, direction, excite=1.0, priority=5) -> LumpedPort:
        d = {"x": 0, "y": 1, "z": 2}.get(direction, direction)
        p = LumpedPort(int(number), float(R), tuple(map(float, start)), tuple(map(float, stop)), int(d),
                       float(excite), int(priority))
        self.ports.append(p)
        return p

    def add_waveguide_port(self, number, start, stop, direction, e_func, h_func, kc, excite=0.0, eps_r=1.0, mode=None) -> WaveguidePort:
        """A modal port (ports.py): e_func, h_func callables (x, y) -> (c_P, c_PP), x and y in metres from the box's minimum corner."""
        who = f"waveguide port {number}"
        _ports.check_funcs(who, e_func, h_func)
        p = WaveguidePort(int(number), tuple(map(float, start)), tuple(map(float, stop)), _ports._axis(direction, who), e_func, h_func,
                          float(kc), float(excite), float(eps_r), mode=mode)
        if p.start[p.direction] == p.stop[p.direction]:
            raise ValueError(f"{who}: start and stop coincide along {'xyz'[p.direction]}: the port has no direction (d = 0)")
        self.ports.append(p)
        return p

    def add_rect_waveguide_port(self, number, start, stop, direction, a, b, mode, excite=0.0, eps_r=1.0) -> WaveguidePort:
        """A TEmn port of an a x b [m] rectangular guide, a along (p + 1) % 3, b along (p + 2) % 3 (ports.py)."""
        e_func, h_func, kc = _ports.rect_te_mode(a, b, mode, f"rectangular waveguide port {number}")
        return self.add_waveguide_port(number, start, stop, direction, e_func, h_func, kc, excite, eps_r, mode=str(mode).upper())

    def add_msl_port(self, number, metal: "Metal", start, stop, prop_dir, exc_dir, excite=0.0, feed_shift=0.0, meas_plane_shift=None,
                     feed_R=float("inf"), priority=0, add_strip=True) -> MSLPort:
        """A microstrip-line port (ports.py); its strip is added to `metal` here, as a zero-thickness box on the plane stop[exc]
        (add_strip=False: the caller has drawn it)."""
        who = f"MSL port {number}"
        if not isinstance(metal, Metal):
            raise ValueError(f"{who}: the strip needs a metal of this scene (add_metal / add_conducting_sheet)")
        p = MSLPort(int(number), metal, tuple(map(float, start)), tuple(map(float, stop)), _ports._axis(prop_dir, who), _ports._axis(exc_dir, who),
                    float(excite), float(feed_shift), None if meas_plane_shift is None else float(meas_plane_shift), float(feed_R), int(priority))
        if p.prop == p.exc:
            raise ValueError(f"{who}: the propagation and the excitation direction are both {'xyz'[p.prop]}")
        for a in range(3):
            if p.start[a] == p.stop[a]:
                raise ValueError(f"{who}: its box has zero extent along {'xyz'[a]}")
        if add_strip:
            metal.add_box(*_ports.msl_strip_box(p), priority=p.priority)
        self.ports.append(p)
        return p

    def add_lumped_element(self, name, direction, R=None, C=None, L=None, kind="parallel", caps=True) -> LumpedElement:
        """R [ohm], L [H], C [F] in parallel (kind "parallel" / 0: Y = 1/R + sC + 1/(sL)) or in series ("series" / 1:
        Z = R + sL + 1/(sC)) between the two ends of its boxes along `direction`; None: the part is absent (lumped.py)."""
        d = {"x": 0, "y": 1, "z": 2}.get(direction, direction)
        if d not in (0, 1, 2):
            raise ValueError(f"lumped element '{name}': direction must be 0..2 or 'x', 'y', 'z'")
        el = LumpedElement(str(name), int(d), _lumped.Element(str(name), R, L, C, kind), bool(caps))
        self.elements.append(el)
        return el


    def add_plane_wave(self, name, e0, direction) -> PlaneWaveSource:
        """A plane wave E0 s(t - k.(r - r0)/c0) travelling along `direction`, injected on the surface of the box given with
        .add_box(start, stop): total field inside, scattered field outside (planewave.py).  e0 [V/m] is projected perpendicular to
        the direction; one plane wave per scene."""
        if self.plane_waves:
            raise ValueError(f"plane wave '{name}': the scene already has the plane wave '{self.plane_waves[0].name}' (one plane-wave box per scene)")
        pw = PlaneWaveSource(str(name), _planewave.PlaneWave(str(name), e0, direction))
        self.plane_waves.append(pw)
        return pw


    def add_field_excitation(self, name, exc_type, exc_val, start, stop, weight=None, delay=0.0, priority=0) -> "_fexc.FieldExcitation":
        """An E- or H-field excitation over a box, a plane, a line or a point (field_excitation.py): exc_type 0 soft E, 1 hard E, 2 soft
        H, 3 hard H; exc_val the field vector [V/m or A/m]; start, stop in drawing units; weight None, one callable (x, y, z) or
        three per-component callables or strings (coordinates in drawing units); delay [s]."""
        if any(e.name == str(name) for e in self.field_excitations):
            raise ValueError(f"field excitation '{name}' is defined twice")
        ex = _fexc.make(name, exc_type, exc_val, start, stop, weight, delay, priority)
        self.field_excitations.append(ex)
        return ex


@dataclass
class PortOnGrid:
    """A port on the grid: optional resistor edges, one source list, a list of V-probes and a list of I-probes (ports.Probe).  A
    lumped port has one probe of each kind; v_idx ... i_w read the first of each.  `pec`: edges the port makes metal (an MSL port
    with feed_R = 0); `info`: the summary of a waveguide / MSL port (ports.PortLists.info), None for a lumped port."""
    port: object              # LumpedPort, ports.WaveguidePort or ports.MSLPort
    lumped: List[LumpedEdge]
    src_idx: np.ndarray       # global flat node indices
    src_comp: np.ndarray
    src_amp: np.ndarray
    v_probes: List[Probe]
    i_probes: List[Probe]
    pec: Optional[Tuple[np.ndarray, np.ndarray]] = None
    info: Optional[dict] = None

    v_idx = property(lambda self: self.v_probes[0].idx)
    v_comp = property(lambda self: self.v_probes[0].comp)
    v_w = property(lambda self: self.v_probes[0].w)
    i_idx = property(lambda self: self.i_probes[0].idx)
    i_comp = property(lambda self: self.i_probes[0].comp)
    i_w = property(lambda self: self.i_probes[0].w)


@dataclass
class VoxelScene:
    eps_r: np.ndarray         # [nz-1][ny-1][nx-1]
    kappa: np.ndarray
    pec: np.ndarray           # bool [3][nz][ny][nx]
    ports: List[PortOnGrid]
    sheets: Optional[_sheet.SheetEdges] = None   # conducting-sheet edges (None: the scene has no conducting sheet)
    # Debye media (None: the scene has none): eps_r / kappa hold eps_inf / kappa of their cells — the timestep-dependent part of
    # the fold (kappa += sum_k beta_k) is Simulation's, which knows dt
    debye: Optional[_disp.DebyeEdges] = None
    lorentz: Optional[_lorentz.LorentzEdges] = None  # Lorentz / Drude media, a sibling of debye (the fold kappa += sum_k g0_k is Simulation's too)
    elements: Optional[_lumped.LumpedEdges] = None   # lumped-element edges (None: the scene has no lumped element)
    # magnetic materials (None: mu_r = 1, sigma_m = 0 everywhere): per cell, same priority rule as eps_r; cell_material indexes
    # material_names (-1: background) so that a refusal can name the material
    mu_r: Optional[np.ndarray] = None
    sigma_m: Optional[np.ndarray] = None
    cell_material: Optional[np.ndarray] = None
    material_names: Optional[List[str]] = None
    # conformal PEC boundaries (None: not asked for): the nodes inside the plain metals and the fractions of the cut edges
    # (conformal.Fractions); Simulation(conformal=True) turns them into the face list
    fractions: Optional["_conformal.Fractions"] = None
    # mass density per cell [kg/m^3] of the material that owns it (None: no material of the scene has one): sar.py
    density: Optional[np.ndarray] = None
    # plane-wave excitation (None: the scene has none): direction, e0 and the box snapped to whole nodes (planewave.PlaneWave)
    plane_wave: Optional["_planewave.PlaneWave"] = None
    # voxel body models (None: the scene has no disc material): per cell the linear index of its voxel in the map of the disc
    # material that owns it (cell_material says which), -1 where another material or the background does
    cell_voxel: Optional[np.ndarray] = None
    # field excitations (field_excitation.FieldExcitation, in scene order) and the scene's drawing unit: Simulation, which knows dt,
    # turns them into lists
    field_excitations: Optional[list] = None
    unit: float = 1e-3
    # anisotropic dielectrics (None unless some material of the scene is anisotropic): eps_r / kappa per cell and axis,
    # [3][nz-1][ny-1][nx-1], filled by the ownership rule of eps_r — slice c is what the edges of direction c read
    # (ecoperator.build_operator).  eps_r / kappa above then hold, in the cells of an anisotropic material, the MEAN of its three values
    # (Material.eps_r / .kappa): a scalar view for reports and for the checks that only ask "is this vacuum"; the operator, the
    # lumped overrides and the edge conductivities of the J dumps read the per-axis arrays and never this view.
    eps_axes: Optional[np.ndarray] = None
    kappa_axes: Optional[np.ndarray] = None
    anisotropic_names: Optional[List[str]] = None   # the anisotropic materials that own at least one cell
    # sub-cell averaged dielectric surfaces (None: not asked for): the listed edges with their eps_rel / kap_e (subcell.Listed);
    # Simulation(subcell=True) turns them into per-edge operator overrides
    subcell: Optional["_subcell.Listed"] = None

    def cell_eps(self) -> np.ndarray:
        """What the operator reads: eps_axes when the scene is anisotropic, eps_r otherwise."""
        return self.eps_r if self.eps_axes is None else self.eps_axes

    def cell_kappa(self) -> np.ndarray:
        return self.kappa if self.kappa_axes is None else self.kappa_axes

    @property
    def lumped(self) -> List[LumpedEdge]:
        return [le for p in self.ports for le in p.lumped]


def _tol(grid: RectGrid) -> float:
    return 1e-6 * min(float(np.min(np.diff(l))) for l in grid.lines)


def _index_range(lines: np.ndarray, a: float, b: float, tol: float):  # kept for tools/tests
    """Node indices whose coordinate lies in [min(a,b), max(a,b)] (with tolerance)."""
    lo, hi = (a, b) if a <= b else (b, a)
    idx = np.nonzero((lines >= lo - tol) & (lines <= hi + tol))[0]
    return (int(idx[0]), int(idx[-1])) if idx.size else (0, -1)


def _inside_mask(bx: Box, u: float, tol: float, coords: Sequence[np.ndarray]):
    """Boolean block over the sub-grid of points `coords` (one 1-D array per axis, metres) that lie
    inside the (possibly rotated/translated) box.  Returns (mask[z][y][x], index offsets) or None."""
    lo = np.minimum(bx.start, bx.stop) * u
    hi = np.maximum(bx.start, bx.stop) * u
    if bx.matrix is None or np.allclose(bx.matrix, np.eye(4)):
        sel = [np.nonzero((c >= lo[a] - tol) & (c <= hi[a] + tol))[0] for a, c in enumerate(coords)]
        if any(s_.size == 0 for s_ in sel):
            return None
        off = [int(s_[0]) for s_ in sel]
        shape = [int(s_[-1]) - int(s_[0]) + 1 for s_ in sel]
        return np.ones((shape[2], shape[1], shape[0]), bool), off
    M = np.array(bx.matrix, dtype=float)
    M[:3, 3] *= u
    corners = np.array([[x, y, z, 1.0] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    w = (M @ corners.T).T[:, :3]
    sel = [np.nonzero((c >= w[:, a].min() - tol) & (c <= w[:, a].max() + tol))[0] for a, c in enumerate(coords)]
    if any(s_.size == 0 for s_ in sel):
        return None
    off = [int(s_[0]) for s_ in sel]
    sub = [coords[a][sel[a][0]:sel[a][-1] + 1] for a in range(3)]
    Z, Y, X = np.meshgrid(sub[2], sub[1], sub[0], indexing="ij")
    Minv = np.linalg.inv(M)
    P = np.stack([X, Y, Z, np.ones_like(X)], axis=-1) @ Minv.T
    mask = np.ones(X.shape, bool)
    for a in range(3):
        mask &= (P[..., a] >= lo[a] - tol) & (P[..., a] <= hi[a] + tol)
    return mask, off


def _merged_media(materials, kind):
    """(media, the material names merged into each, key -> medium id) of the materials of class `kind`, in order of appearance."""
    media, names, medium_of = [], [], {}
    for mat in materials:
        if isinstance(mat, kind):
            k = mat.medium.key()
            if k not in medium_of:
                medium_of[k] = len(media)
                media.append(mat.medium)
                names.append([])
            names[medium_of[k]].append(mat.name)
    return media, names, medium_of


def voxelize(scene: Scene, grid: RectGrid, rasteriser=None, conformal: bool = False, device_fractions=None, subcell: int = 0,
             device_subcell=None) -> VoxelScene:
    """A scene drawn with boxes only takes the box path; any other primitive sends every primitive, boxes included, through the
    owner arrays of `rasteriser` (default: primitives.rasterise_spec; _capi.voxelize_device gives the device one).  `conformal`:
    also the fractions of the edges the plain metals cut (conformal.fractions; `device_fractions`: _capi.default_fractions' callable,
    None: numpy) — the staircase itself, every other field of the result, stays what it is.  `subcell` (0: off; 2, 4 or 8 sub-voxels
    per cell and axis): also the edges that dielectric surfaces cross, with their sub-cell averaged eps_rel / kap_e (subcell.listed;
    `device_subcell`: _capi.default_subcell's callable, None: numpy); nothing else of the result changes."""
    if subcell:
        _subcell.check_nsub(subcell)
        _subcell.prop_tables(scene)             # refuses a disc material by name before anything is rasterised
    vs = _voxelize(scene, grid, rasteriser)
    if subcell:
        # the edges whose operator entries the host fixes anyway: the ports' resistors, the sheet edges, the lumped elements' edges
        le = vs.lumped
        edge = [grid.flat(np.array([e.i for e in le], np.int64), np.array([e.j for e in le], np.int64), np.array([e.k for e in le], np.int64))]
        comp = [np.array([e.comp for e in le], np.int64)]
        for lst in (vs.sheets, vs.elements):
            if lst is not None and len(lst):
                edge.append(np.asarray(lst.idx, np.int64)); comp.append(np.asarray(lst.comp, np.int64))
        vs.subcell = _subcell.listed(scene, grid, int(subcell), vs.pec, np.concatenate(edge), np.concatenate(comp), device_subcell)
    if any(m.density > 0 or (isinstance(m, DiscMaterial) and np.any(m.vmap.density > 0)) for m in scene.materials):
        vs.density = np.array([m.density for m in scene.materials] + [0.0])[vs.cell_material]
        _from_voxels(scene, vs.cell_material, vs.cell_voxel, "density", vs.density)
    if conformal:
        vs.fractions = _conformal.fractions(scene, grid, device_fractions)
    for src in getattr(scene, "plane_waves", []):
        if not src.boxes:
            raise ValueError(f"plane wave '{src.name}' has no box: add_box(start, stop) gives the total-field region")
        bx, u = src.boxes[0], scene.unit
        lo = tuple(grid.snap(a, min(bx.start[a], bx.stop[a]) * u) for a in range(3))
        hi = tuple(grid.snap(a, max(bx.start[a], bx.stop[a]) * u) for a in range(3))
        vs.plane_wave = _planewave.PlaneWave(src.name, src.spec.e0, src.spec.direction, lo, hi)
    if getattr(scene, "field_excitations", None):
        vs.field_excitations, vs.unit = list(scene.field_excitations), float(scene.unit)
    return vs


def _from_voxels(scene: Scene, cell_material, cell_voxel, what: str, out: np.ndarray) -> None:
    """out[cell] = the table value `what` (eps_r, kappa, density) of the cell's voxel, for the cells a disc material owns."""
    if cell_voxel is None:
        return
    for qi, m in enumerate(scene.materials):
        if isinstance(m, DiscMaterial):
            sel = (cell_material == qi) & (cell_voxel >= 0)
            out[sel] = getattr(m.vmap, what)[m.vmap.data.reshape(-1)[cell_voxel[sel]]]


def _fill_axes(scene: Scene, vs: VoxelScene) -> VoxelScene:
    """eps_axes / kappa_axes of a scene with an anisotropic material, from the cells' owners (cell_material: highest priority wins,
    later wins ties — the rule that filled eps_r): the owner's three values per axis, eps_r / kappa of the cell (background, disc
    voxels and folds included) three times where the owner is isotropic.  Both voxelisers end here."""
    if not any(m.anisotropic for m in scene.materials):
        return vs
    vs.eps_axes = np.stack([vs.eps_r] * 3)
    vs.kappa_axes = np.stack([vs.kappa] * 3)
    vs.anisotropic_names = []
    for qi, m in enumerate(scene.materials):
        if not m.anisotropic:
            continue
        sel = vs.cell_material == qi
        if sel.any():
            vs.anisotropic_names.append(m.name)
        for c, (e, k) in enumerate(zip(*m.axes())):
            vs.eps_axes[c][sel] = e
            vs.kappa_axes[c][sel] = k
    return vs


def _voxelize(scene: Scene, grid: RectGrid, rasteriser=None) -> VoxelScene:
    if _prims.has_new(scene):
        return voxelize_owners(scene, grid, rasteriser)
    return _fill_axes(scene, _voxelize_boxes(scene, grid))


def _voxelize_boxes(scene: Scene, grid: RectGrid) -> VoxelScene:
    nx, ny, nz = grid.shape
    u = scene.unit
    tol = _tol(grid)
    eps = np.ones((nz - 1, ny - 1, nx - 1))
    kap = np.zeros_like(eps)
    mur = np.ones_like(eps)
    sgm = np.zeros_like(eps)
    cmat = np.full(eps.shape, -1, dtype=np.int32)
    prio = np.full(eps.shape, -(1 << 30), dtype=np.int64)
    centers = [grid.centers(a) for a in range(3)]
    # Debye materials with identical parameters are one medium (as sheets of one metal are one surface), and so are Lorentz materials
    media, media_names, medium_of = _merged_media(scene.materials, DebyeMaterial)
    if len(media) > _disp.MAX_MEDIA:
        raise ValueError(f"{len(media)} different Debye media: at most {_disp.MAX_MEDIA}")
    cmed = np.full(eps.shape, -1, dtype=np.int8) if media else None
    lmedia, lmedia_names, lmedium_of = _merged_media(scene.materials, LorentzMaterial)
    if len(lmedia) > _lorentz.MAX_MEDIA:
        raise ValueError(f"{len(lmedia)} different Lorentz media: at most {_lorentz.MAX_MEDIA}")
    clor = np.full(eps.shape, -1, dtype=np.int8) if lmedia else None
    for qm, mat in enumerate(scene.materials):
        mid = medium_of[mat.medium.key()] if isinstance(mat, DebyeMaterial) else -1
        lid = lmedium_of[mat.medium.key()] if isinstance(mat, LorentzMaterial) else -1
        for bx in mat.boxes:
            r = _inside_mask(bx, u, -tol, centers)     # strict: a cell centre on the surface is outside
            if r is None:
                continue
            mask, off = r
            sl = tuple(slice(off[a], off[a] + mask.shape[2 - a]) for a in (2, 1, 0))
            win = mask & (prio[sl] <= bx.priority)
            e = eps[sl]; k = kap[sl]; p = prio[sl]
            e[win] = mat.eps_r; k[win] = mat.kappa; p[win] = bx.priority
            mur[sl][win] = mat.mu_r; sgm[sl][win] = mat.sigma_m; cmat[sl][win] = qm
            if cmed is not None:
                cmed[sl][win] = mid
            if clor is not None:
                clor[sl][win] = lid
    debye = _disp.make_edges(grid, media, media_names, cmed) if media and np.any(cmed >= 0) else None
    lorentz = _lorentz.make_edges(grid, lmedia, lmedia_names, clor) if lmedia and np.any(clor >= 0) else None
    if lorentz is not None:
        _lorentz.check_disjoint(lorentz, debye)
    magnetic = dict(mu_r=mur, sigma_m=sgm, cell_material=cmat, material_names=[m.name for m in scene.materials])
    if any(isinstance(m, ConductingSheet) for m in scene.metals):
        vs = _voxelize_with_sheets(scene, grid, eps, kap)
        vs.debye, vs.lorentz = debye, lorentz
        vs.mu_r, vs.sigma_m, vs.cell_material, vs.material_names = mur, sgm, cmat, magnetic["material_names"]
        vs.elements = _elements_on_grid(scene, grid, vs.pec, vs.ports, vs.sheets)
        return vs
    pec = np.zeros((3, nz, ny, nx), dtype=bool)
    for met in scene.metals:
        for bx in met.boxes:
            r = _inside_mask(bx, u, tol, grid.lines)
            if r is None:
                continue
            node, off = r
            for c in range(3):
                npa = 2 - c                                   # numpy axis of direction c
                if node.shape[npa] < 2:
                    continue
                a = [slice(None)] * 3; b = [slice(None)] * 3
                a[npa] = slice(0, -1); b[npa] = slice(1, None)
                edge = node[tuple(a)] & node[tuple(b)]        # both end nodes inside
                sl = [slice(off[2], off[2] + edge.shape[0]), slice(off[1], off[1] + edge.shape[1]),
                      slice(off[0], off[0] + edge.shape[2])]
                pec[c][tuple(sl)] |= edge
    ports = _ports_on_grid(scene, grid, pec)
    return VoxelScene(eps, kap, pec, ports, debye=debye, lorentz=lorentz, elements=_elements_on_grid(scene, grid, pec, ports, None), **magnetic)


def _box_edges(node: np.ndarray, c: int):
    """Edges of direction c with both end nodes in the node block (shape along c one less, padded back with False)."""
    npa = 2 - c
    if node.shape[npa] < 2:
        return None
    a = [slice(None)] * 3; b = [slice(None)] * 3
    a[npa] = slice(0, -1); b[npa] = slice(1, None)
    return node[tuple(a)] & node[tuple(b)]


def _voxelize_with_sheets(scene: Scene, grid: RectGrid, eps, kap) -> VoxelScene:
    """voxelize() for a scene with conducting sheets: the metal that owns an edge is the one of the highest-priority box (later
    boxes win ties); edges owned by a sheet metal that lie on its surface become sheet edges, all other metal edges PEC."""
    nx, ny, nz = grid.shape
    u = scene.unit
    tol = _tol(grid)
    centers = [grid.centers(a) for a in range(3)]
    eprio = np.full((3, nz, ny, nx), np.iinfo(np.int64).min, np.int64)
    eown = np.full((3, nz, ny, nx), -1, np.int32)
    node_masks = {}
    for mi, met in enumerate(scene.metals):
        for bx in met.boxes:
            r = _inside_mask(bx, u, tol, grid.lines)
            if r is None:
                continue
            node, off = r
            if isinstance(met, ConductingSheet):
                full = np.zeros((nz, ny, nx), bool)
                full[off[2]:off[2] + node.shape[0], off[1]:off[1] + node.shape[1], off[0]:off[0] + node.shape[2]] = node
                node_masks.setdefault(mi, []).append(full)
            for c in range(3):
                edge = _box_edges(node, c)
                if edge is None:
                    continue
                sl = (slice(off[2], off[2] + edge.shape[0]), slice(off[1], off[1] + edge.shape[1]),
                      slice(off[0], off[0] + edge.shape[2]))
                win = edge & (eprio[c][sl] <= bx.priority)
                eprio[c][sl][win] = bx.priority
                eown[c][sl][win] = mi
    def filled_of(members):
        filled = np.zeros((nz, ny, nx), bool)
        for mi in members:
            for bx in scene.metals[mi].boxes:
                r = _inside_mask(bx, u, -tol, centers)
                if r is None:
                    continue
                mask, off = r
                sl = tuple(slice(off[a], off[a] + mask.shape[2 - a]) for a in (2, 1, 0))
                filled[sl] |= mask
        return filled
    return _sheets_from_owners(scene, grid, eps, kap, eown, node_masks, filled_of)


def _sheets_from_owners(scene: Scene, grid: RectGrid, eps, kap, eown, node_masks, filled_of) -> VoxelScene:
    """The sheet edges from eown (int32 [3][nz][ny][nx]: the metal that owns the edge, -1 none), node_masks (sheet metal -> the node
    masks of its primitives) and filled_of(members) (the cells a group of sheet metals fills, at the lowest node)."""
    nx, ny, nz = grid.shape
    u = scene.unit
    pec = eown >= 0
    sh = _sheet.SheetEdges()
    parts = []
    # The surface of a metal is taken from all sheet metals of the same conductivity and thickness together: where two of them meet
    # edge to edge (a patch and its feed line), the junction is inside one conductor, not a rim of each (half a dual width twice).
    groups = {}
    for mi in node_masks:
        groups.setdefault((scene.metals[mi].conductivity, scene.metals[mi].thickness), []).append(mi)
    for members in groups.values():
        filled = filled_of(members)
        S = _sheet.surface_faces([m for mi in members for m in node_masks[mi]], filled)
        for mi in members:
            met = scene.metals[mi]
            q = len(sh.metals)
            sh.metals.append(_sheet.SheetMetal(met.name, met.conductivity, met.thickness))
            for c in range(3):
                on, scale = _sheet.edge_geometry(grid, c, eown[c] == mi, S, filled)
                flat = np.flatnonzero(on)
                pec[c][on] = False
                parts.append((flat.astype(np.int64), np.full(flat.size, c, np.int8), scale[on].astype(np.float64),
                              np.full(flat.size, q, np.int32)))
    if parts:
        sh.idx, sh.comp, sh.scale, sh.metal = (np.concatenate([p[t] for p in parts]) for t in range(4))
    # edges the correction must not touch: port edges (sources, lumped resistors) and voltage-probe lines (the ports come after the
    # sheets: a waveguide or MSL port leaves PEC edges out of its lists, and a sheet edge is not PEC)
    ports = _ports_on_grid(scene, grid, pec)
    key = sh.idx * 3 + sh.comp
    for p in ports:
        for what, idx, comp in (("voltage-probe line", p.v_idx, p.v_comp), ("port edge", p.src_idx, p.src_comp)):
            hit = np.isin(key, np.asarray(idx, np.int64) * 3 + np.asarray(comp, np.int64))
            if hit.any():
                e = int(np.argmax(hit))
                k, r = divmod(int(sh.idx[e]), nx * ny)
                raise ValueError(f"conducting sheet '{sh.metals[sh.metal[e]].name}': the edge at node {(r % nx, r // nx, k)} "
                                 f"({'xyz'[sh.comp[e]]}) is a {what} of {_ports.label(p.port)}")
    return VoxelScene(eps, kap, pec, ports, sh)


def _port_on_grid(port: LumpedPort, grid: RectGrid, u: float) -> PortOnGrid:
    """Lumped port = series/parallel resistor network on the edges inside the port box, a soft
    voltage source on the same edges, a voltage line through the box centre and a current loop
    around the box at mid-length ([EXT] openEMS ports.LumpedPort: AddLumpedElement + AddExcitation +
    two AddProbe; called from solver_fdtd_openems_fixed.py:215)."""
    d = port.direction
    a1, a2 = (d + 1) % 3, (d + 2) % 3
    lo = [grid.snap(a, min(port.start[a], port.stop[a]) * u) for a in range(3)]
    hi = [grid.snap(a, max(port.start[a], port.stop[a]) * u) for a in range(3)]
    if hi[d] <= lo[d]:
        raise ValueError("lumped port has zero length along its direction on this mesh")
    sign = 1.0 if port.stop[d] >= port.start[d] else -1.0
    n_ser = hi[d] - lo[d]
    n_par = (hi[a1] - lo[a1] + 1) * (hi[a2] - lo[a2] + 1)
    length = grid.lines[d][hi[d]] - grid.lines[d][lo[d]]
    lumped, s_idx, s_amp = [], [], []
    for p1 in range(lo[a1], hi[a1] + 1):
        for p2 in range(lo[a2], hi[a2] + 1):
            for q in range(lo[d], hi[d]):
                pos = [0, 0, 0]
                pos[d], pos[a1], pos[a2] = q, p1, p2
                if port.R > 0:
                    lumped.append(LumpedEdge(d, pos[0], pos[1], pos[2], n_ser / (port.R * n_par)))
                s_idx.append(grid.flat(*pos))
                # field of -excite/length across the port => unit port voltage for excite = 1
                s_amp.append(-sign * port.excite * grid.d[d][q] / length)
    # voltage: U = -dir * sum of edge voltages along the centre line (probes.voltage_path: a stand-alone voltage probe walks the same way)
    c1 = grid.snap(a1, 0.5 * (port.start[a1] + port.stop[a1]) * u)
    c2 = grid.snap(a2, 0.5 * (port.start[a2] + port.stop[a2]) * u)
    p0, p1 = [0, 0, 0], [0, 0, 0]
    p0[d], p1[d] = (lo[d], hi[d]) if sign > 0 else (hi[d], lo[d])
    p0[a1] = p1[a1] = c1
    p0[a2] = p1[a2] = c2
    v_idx, _, v_sign = _probes.voltage_path(grid, p0, p1)
    assert np.all(v_sign == sign)
    # current: loop of dual edges around the port cross-section at the middle edge (probes.current_loop)
    qm = lo[d] + (n_ser - 1) // 2
    i_idx, i_comp, i_w = _probes.current_loop(grid, lo, hi, d, qm)
    i_w = (sign * i_w).astype(np.float32)
    return PortOnGrid(
        port=port, lumped=lumped,
        src_idx=np.array(s_idx, np.int64), src_comp=np.full(len(s_idx), d, np.int8),
        src_amp=np.array(s_amp, np.float32),
        v_probes=[Probe(np.array(v_idx, np.int64), np.full(len(v_idx), d, np.int8), np.full(len(v_idx), -sign, np.float32))],
        i_probes=[Probe(i_idx, i_comp, i_w)])


def _ports_on_grid(scene: "Scene", grid: RectGrid, pec: np.ndarray) -> List[PortOnGrid]:
    """Every port of the scene on the grid, in the order they were added.  A waveguide or MSL port reads `pec` (its lists leave metal
    edges out) and may add to it (an MSL port with feed_R = 0), so the metals come first."""
    out = []
    for p in scene.ports:
        if isinstance(p, LumpedPort):
            out.append(_port_on_grid(p, grid, scene.unit))
            continue
        pl = _ports.lists(grid, pec, p, scene.unit)
        if pl.pec[0].size:
            pec.reshape(3, -1)[pl.pec[1].astype(np.int64), pl.pec[0]] = True
        out.append(PortOnGrid(p, pl.lumped, pl.src.idx, pl.src.comp, pl.src.w, pl.v_probes, pl.i_probes, pl.pec, pl.info))
    return out


def _elements_on_grid(scene: Scene, grid: RectGrid, pec: np.ndarray, ports, sheets) -> Optional[_lumped.LumpedEdges]:
    """The lumped elements' boxes on the mesh, as a port's box: n_ser edges along the direction, n_par parallel lines; one
    lumped.Element per box with these split factors.  `caps`: the transverse edges of the two end planes inside the cross-section
    become PEC (`pec` is updated in place, sheet edges among them leave `sheets`) — a line element has none.  Refused (ValueError): a box of zero length, an edge that is
    PEC, a sheet edge, a port's source edge or voltage-probe line (for the element's edges and for its cap edges), two elements on
    one edge."""
    if not scene.elements:
        return None
    nx, ny, nz = grid.shape
    u = scene.unit
    out = _lumped.LumpedEdges()
    idx, comp, elem = [], [], []
    caps = np.zeros_like(pec)
    cap_of = {}                                   # cap edge key (flat node index * 3 + component) -> element name
    for el in scene.elements:
        d = el.direction
        a1, a2 = (d + 1) % 3, (d + 2) % 3
        for bx in el.boxes:
            lo = [grid.snap(a, min(bx.start[a], bx.stop[a]) * u) for a in range(3)]
            hi = [grid.snap(a, max(bx.start[a], bx.stop[a]) * u) for a in range(3)]
            if hi[d] <= lo[d]:
                raise ValueError(f"lumped element '{el.name}': the box at node {tuple(lo)} has zero length along "
                                 f"{'xyz'[d]} on this mesh")
            n_ser = hi[d] - lo[d]
            n_par = (hi[a1] - lo[a1] + 1) * (hi[a2] - lo[a2] + 1)
            q = len(out.elements)
            out.elements.append(el.spec.split(n_ser, n_par))
            for p1 in range(lo[a1], hi[a1] + 1):
                for p2 in range(lo[a2], hi[a2] + 1):
                    for s in range(lo[d], hi[d]):
                        pos = [0, 0, 0]
                        pos[d], pos[a1], pos[a2] = s, p1, p2
                        idx.append(grid.flat(*pos)); comp.append(d); elem.append(q)
            if el.caps:
                for end in (lo[d], hi[d]):
                    for t, o in ((a1, a2), (a2, a1)):            # t-directed edges, both end nodes inside the cross-section
                        for pt in range(lo[t], hi[t]):
                            for po in range(lo[o], hi[o] + 1):
                                pos = [0, 0, 0]
                                pos[d], pos[t], pos[o] = end, pt, po
                                caps[t, pos[2], pos[1], pos[0]] = True
                                cap_of.setdefault(grid.flat(*pos) * 3 + t, el.name)
    out.idx, out.comp, out.elem = np.array(idx, np.int64), np.array(comp, np.int8), np.array(elem, np.int32)

    def where(e):
        k, r = divmod(int(out.idx[e]), nx * ny)
        return (f"lumped element '{out.elements[out.elem[e]].name}': the edge at node {(r % nx, r // nx, k)} "
                f"({'xyz'[out.comp[e]]})")

    key = out.idx * 3 + out.comp
    uniq, first, count = np.unique(key, return_index=True, return_counts=True)
    if np.any(count > 1):
        e = int(np.min(first[count > 1]))
        other = [int(q) for q in np.nonzero(key == key[e])[0] if q != e][0]
        raise ValueError(f"{where(e)} also belongs to lumped element '{out.elements[out.elem[other]].name}': two elements on one edge")
    # cap edges are metal: a port they would short is refused, a conducting-sheet edge among them becomes PEC and leaves the sheets
    if cap_of:
        ckey = np.fromiter(cap_of, np.int64, len(cap_of))
        for p in ports:
            for what, pidx, pcomp in (("voltage-probe line", p.v_idx, p.v_comp), ("source edge", p.src_idx, p.src_comp)):
                pk = np.asarray(pidx, np.int64) * 3 + np.asarray(pcomp, np.int64)
                hit = np.isin(pk, ckey)
                if hit.any():
                    kk = int(pk[int(np.argmax(hit))])
                    k, r = divmod(kk // 3, nx * ny)
                    raise ValueError(f"lumped element '{cap_of[kk]}': its cap edge at node {(r % nx, r // nx, k)} ({'xyz'[kk % 3]}) is a "
                                     f"{what} of {_ports.label(p.port)}: the port would be shorted (caps=False leaves the end planes open)")
        if sheets is not None and len(sheets):
            keep = ~np.isin(sheets.idx * 3 + sheets.comp, ckey)
            sheets.idx, sheets.comp, sheets.scale, sheets.metal = sheets.idx[keep], sheets.comp[keep], sheets.scale[keep], sheets.metal[keep]
    pec |= caps
    hit = pec.reshape(3, -1)[out.comp.astype(np.int64), out.idx]
    if hit.any():
        raise ValueError(f"{where(int(np.argmax(hit)))} is PEC: the element would be shorted")
    if sheets is not None and len(sheets):
        hit = np.isin(key, sheets.idx * 3 + sheets.comp)
        if hit.any():
            raise ValueError(f"{where(int(np.argmax(hit)))} is a conducting-sheet edge")
    for p in ports:
        for what, pidx, pcomp in (("voltage-probe line", p.v_idx, p.v_comp), ("source edge", p.src_idx, p.src_comp)):
            hit = np.isin(key, np.asarray(pidx, np.int64) * 3 + np.asarray(pcomp, np.int64))
            if hit.any():
                raise ValueError(f"{where(int(np.argmax(hit)))} is a {what} of {_ports.label(p.port)}")
    return out


def voxelize_owners(scene: Scene, grid: RectGrid, rasteriser=None) -> VoxelScene:
    """voxelize() through the owner arrays (primitives.pack_table -> rasteriser(grid, table) -> (cell_owner, edge_owner)): every
    VoxelScene field is filled from the owners, by the ownership rules of the box path (highest priority, later wins ties; an edge
    is metal when one primitive holds both its end nodes).  Curves and wire centre lines are snapped to grid edges on the host."""
    return _fill_axes(scene, _voxelize_owners(scene, grid, rasteriser))


def _voxelize_owners(scene: Scene, grid: RectGrid, rasteriser=None) -> VoxelScene:
    import warnings
    nx, ny, nz = grid.shape
    u = scene.unit
    table = _prims.pack_table(scene, grid)
    res = (rasteriser or _prims.rasterise_spec)(grid, table)
    if len(res) != (3 if table.maps else 2):
        raise ValueError("the rasteriser returned no cell_voxel for a table with voxel maps" if table.maps else
                         "the rasteriser returned three results for a table without voxel maps")
    cown, eown = res[0], res[1]
    cvox = res[2] if table.maps else None         # per cell: the voxel of the owning disc record, -1 elsewhere (None: no maps)
    rec = table.rec
    shape = (nz - 1, ny - 1, nx - 1)
    if cown.shape != shape or eown.shape != (3, nz, ny, nx) or (cvox is not None and cvox.shape != shape):
        raise ValueError("the rasteriser returned owner arrays of the wrong shape")
    media, media_names, medium_of = _merged_media(scene.materials, DebyeMaterial)
    if len(media) > _disp.MAX_MEDIA:
        raise ValueError(f"{len(media)} different Debye media: at most {_disp.MAX_MEDIA}")
    lmedia, lmedia_names, lmedium_of = _merged_media(scene.materials, LorentzMaterial)
    if len(lmedia) > _lorentz.MAX_MEDIA:
        raise ValueError(f"{len(lmedia)} different Lorentz media: at most {_lorentz.MAX_MEDIA}")
    # per-material tables with the background in the last row, indexed by the owner's material (-1: background)
    mats = scene.materials
    cmat = np.where(cown >= 0, rec["prop"][np.maximum(cown, 0)] if rec.size else -1, -1).astype(np.int32)

    def per_cell(values, background, dtype=np.float64):
        return np.array(list(values) + [background], dtype)[cmat]
    eps = per_cell((m.eps_r for m in mats), 1.0)
    kap = per_cell((m.kappa for m in mats), 0.0)
    _from_voxels(scene, cmat, cvox, "eps_r", eps)
    _from_voxels(scene, cmat, cvox, "kappa", kap)
    mur = per_cell((m.mu_r for m in mats), 1.0)
    sgm = per_cell((m.sigma_m for m in mats), 0.0)
    cmed = per_cell((medium_of[m.medium.key()] if isinstance(m, DebyeMaterial) else -1 for m in mats), -1, np.int8) if media else None
    clor = per_cell((lmedium_of[m.medium.key()] if isinstance(m, LorentzMaterial) else -1 for m in mats), -1, np.int8) if lmedia else None
    debye = _disp.make_edges(grid, media, media_names, cmed) if media and np.any(cmed >= 0) else None
    lorentz = _lorentz.make_edges(grid, lmedia, lmedia_names, clor) if lmedia and np.any(clor >= 0) else None
    if lorentz is not None:
        _lorentz.check_disjoint(lorentz, debye)
    # metals: the metal that owns each edge; curve edges go to their metal where no volume owns the edge
    emet = np.where(eown >= 0, rec["prop"][np.maximum(eown, 0)] if rec.size else -1, -1).astype(np.int32)
    for mi, pts in table.curves:
        for c, i, j, k in _prims.snap_curve(grid, pts):
            if emet[c, k, j, i] < 0:
                emet[c, k, j, i] = mi
    owned = np.unique(emet)
    metal_recs = np.nonzero(rec["role"] == _prims.ROLE_METAL)[0] if rec.size else []
    for mi, met in enumerate(scene.metals):
        if met.boxes and mi not in owned and not any(_prims.marks_any_edge(grid, table, q) for q in metal_recs if rec["prop"][q] == mi):
            warnings.warn(f"metal '{met.name}' marks no edge of this mesh: it is thinner than a cell and misses every node "
                          f"(add mesh lines through it)", RuntimeWarning, stacklevel=4)
    names = [m.name for m in mats]
    if any(isinstance(m, ConductingSheet) for m in scene.metals):
        node_masks = {}
        cells_of = {}
        for q in metal_recs:
            mi = int(rec["prop"][q])
            if not isinstance(scene.metals[mi], ConductingSheet):
                continue
            for cells, store in ((False, node_masks), (True, cells_of)):
                res = _prims.node_mask(grid, table, q, cells=cells, role=_prims.ROLE_MATERIAL if cells else None)
                if res is None:
                    continue
                full = np.zeros((nz, ny, nx), bool)
                full[res[1]] = res[0]
                store.setdefault(mi, []).append(full)

        def filled_of(members):
            filled = np.zeros((nz, ny, nx), bool)
            for mi in members:
                for f in cells_of.get(mi, []):
                    filled |= f
            return filled
        vs = _sheets_from_owners(scene, grid, eps, kap, emet, node_masks, filled_of)
        vs.debye, vs.lorentz = debye, lorentz
        vs.mu_r, vs.sigma_m, vs.cell_material, vs.material_names, vs.cell_voxel = mur, sgm, cmat, names, cvox
        vs.elements = _elements_on_grid(scene, grid, vs.pec, vs.ports, vs.sheets)
        return vs
    pec = emet >= 0
    ports = _ports_on_grid(scene, grid, pec)
    return VoxelScene(eps, kap, pec, ports, debye=debye, lorentz=lorentz, elements=_elements_on_grid(scene, grid, pec, ports, None),
                      mu_r=mur, sigma_m=sgm, cell_material=cmat, material_names=names, cell_voxel=cvox)
