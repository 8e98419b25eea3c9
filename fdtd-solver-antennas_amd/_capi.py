"""ctypes binding of the C ABI in include/fdtd_hip.h.

``load_hip_library()`` is the ONLY loader the product uses; it raises if libfdtd_hip.so is
missing (there is no CPU fallback).  ``bind()`` can attach the same prototypes to any library
exporting the ABI — tests use that to drive oracle/libfdtd_oracle.so as the checker.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB_NAME = "libfdtd_hip.so"

ABI_SYMBOLS = [
    "fdtd_version", "fdtd_device_count", "fdtd_backend", "fdtd_create", "fdtd_destroy",
    "fdtd_last_error", "fdtd_set_operator_raw", "fdtd_set_operator_classes", "fdtd_build_operator",
    "fdtd_operator_form", "fdtd_get_operator", "fdtd_set_cpml",
    "fdtd_set_mur", "fdtd_set_signal", "fdtd_add_source", "fdtd_add_probe", "fdtd_get_probe",
    "fdtd_set_dft", "fdtd_add_dft_box", "fdtd_get_dft_box", "fdtd_set_recorder", "fdtd_rec_transform", "fdtd_run", "fdtd_run_profiled",
    "fdtd_get_step", "fdtd_energy", "fdtd_p2p_export", "fdtd_p2p_attach", "fdtd_p2p_selftest", "fdtd_p2p_detach", "fdtd_p2p_link_info", "fdtd_schedule_info", "fdtd_comm_unique_id", "fdtd_comm_init", "fdtd_comm_nranks", "fdtd_link", "fdtd_run_linked", "fdtd_half_step",
    "fdtd_halo_get", "fdtd_halo_put", "fdtd_get_field", "fdtd_set_field", "fdtd_farfield",
]

# include/fdtd_hip_sheet.h: conducting sheets, exported by libfdtd_hip.so only (not part of ABI_SYMBOLS / FDTD_ABI_VERSION)
SHEET_SYMBOLS = ["fdtd_sheet_set", "fdtd_sheet_get"]
SHEET_MAX_K = 8
# include/fdtd_hip_dispersion.h: Debye media, likewise
DEBYE_SYMBOLS = ["fdtd_debye_set", "fdtd_debye_get"]
DEBYE_MAX_K = 8
DEBYE_MAX_MEDIA = 8
# include/fdtd_hip_lorentz.h: Lorentz / Drude media, likewise
LORENTZ_SYMBOLS = ["fdtd_lorentz_set", "fdtd_lorentz_get"]
LORENTZ_MAX_K = 4
LORENTZ_MAX_MEDIA = 8
# include/fdtd_hip_lumped.h: lumped R-L-C elements, likewise
LUMPED_SYMBOLS = ["fdtd_lumped_set", "fdtd_lumped_get"]
# include/fdtd_hip_magnetic.h: magnetic materials, likewise
MAGNETIC_SYMBOLS = ["fdtd_magnetic_set", "fdtd_magnetic_get"]
MAGNETIC_MAX_CLASSES = 255
# include/fdtd_hip_traffic.h: which memory-traffic shortcuts a context took, likewise
TRAFFIC_SYMBOLS = ["fdtd_traffic_info"]
# include/fdtd_hip_voxel.h: primitives rasterised on the device, likewise
VOXEL_SYMBOLS = ["fdtd_voxelize"]
# include/fdtd_hip_voxel.h: voxel body models (disc materials) looked up on the device, likewise
DISCMATERIAL_SYMBOLS = ["fdtd_voxelize_maps"]
VOXEL_MAX_MAPS = 4
# include/fdtd_hip_conformal.h: conformal PEC boundaries and the cut edges' fractions on the device, likewise
CONFORMAL_SYMBOLS = ["fdtd_conformal_set", "fdtd_conformal_get", "fdtd_voxel_fractions"]
# include/fdtd_hip_sar.h: local and mass-averaged SAR on the device, likewise
SAR_SYMBOLS = ["fdtd_sar_local", "fdtd_sar_average"]
# include/fdtd_hip_planewave.h: plane-wave excitation on a total-field / scattered-field box, likewise
PLANEWAVE_SYMBOLS = ["fdtd_planewave_set"]
# include/fdtd_hip_excite.h: H-field excitations on listed faces, likewise
EXCITE_SYMBOLS = ["fdtd_excite_set"]
# include/fdtd_hip_fields.h: field dumps (E, H, J, rot-H on a point lattice) on the device, likewise
FIELDS_SYMBOLS = ["fdtd_field_interp"]
# include/fdtd_hip_farfield.h: the radiation integral over a symmetry half and its mirror images, likewise
FARFIELD_MIRROR_SYMBOLS = ["fdtd_farfield_mirror"]
MIRROR_PEC, MIRROR_PMC = 1, 2      # FDTD_MIRROR_PEC / FDTD_MIRROR_PMC: upstream's numbers
# include/fdtd_hip_aniso.h: the operator build with per-axis cell arrays (anisotropic dielectrics), likewise
ANISO_SYMBOLS = ["fdtd_build_operator_axes"]
# include/fdtd_hip_subcell.h: sub-cell averaged dielectric surfaces sampled on the device, likewise
SUBCELL_SYMBOLS = ["fdtd_voxel_subcell"]
# FDTD_MAX_BOXES (csrc/fdtd_ctx.h; MAX_BOXES of the oracle): the DFT / recorder boxes one context takes
MAX_BOXES = 64


class FdtdDesc(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
                ("k0", C.c_int32), ("nk", C.c_int32),
                ("rank", C.c_int32), ("world", C.c_int32),
                ("device", C.c_int32), ("max_steps", C.c_int32),
                ("flags", C.c_uint32), ("dt", C.c_double)]


class FdtdVoxelMap(C.Structure):
    """struct fdtd_voxel_map (include/fdtd_hip_voxel.h), 152 bytes."""
    _fields_ = [("m", C.c_double * 12), ("lines", C.c_void_p * 3), ("data", C.c_void_p), ("ndata", C.c_int64),
                ("n", C.c_int32 * 3), ("use_db_background", C.c_int32)]


class FdtdProfile(C.Structure):
    _fields_ = [("ms_total", C.c_double), ("ms_update_e", C.c_double), ("ms_update_h", C.c_double),
                ("launches_e", C.c_int32), ("launches_h", C.c_int32),
                ("steps", C.c_int32), ("fused", C.c_int32), ("ms_event_overhead", C.c_double)]


FLAG_KERNEL_AUTO, FLAG_KERNEL_DIRECT, FLAG_KERNEL_WAVEFRONT, FLAG_KERNEL_RESIDENT, FLAG_KERNEL_MASK = 0, 1, 5, 6, 0xF
FLAG_OVERLAP_ON, FLAG_OVERLAP_OFF, FLAG_LOOPBACK = 0x20, 0x40, 0x80
KIND_V, KIND_I = 0, 1
PHASE_E, PHASE_H = 0, 1
HALO_H_UP, HALO_E_DOWN = 0, 1

_vp, _i, _i64p = C.c_void_p, C.c_int, C.POINTER(C.c_int64)


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach argtypes/restype for every ABI symbol (raises AttributeError if one is missing)."""
    p = C.c_void_p
    sig = {
        "fdtd_version": (C.c_int, []),
        "fdtd_device_count": (C.c_int, []),
        "fdtd_backend": (C.c_char_p, []),
        "fdtd_create": (C.c_int, [C.POINTER(FdtdDesc), C.POINTER(p)]),
        "fdtd_destroy": (None, [p]),
        "fdtd_last_error": (C.c_char_p, [p]),
        "fdtd_set_operator_raw": (C.c_int, [p, p, p, p, p]),
        "fdtd_set_operator_classes": (C.c_int, [p, p, C.c_int, p, p, p, p]),
        "fdtd_build_operator": (C.c_int, [p, p, p, p, p, p, p, C.c_double, C.c_int, p, p, p, p, p, p, C.c_int]),
        "fdtd_operator_form": (C.c_int, [p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "fdtd_get_operator": (C.c_int, [p, p, p, p, p]),
        "fdtd_set_cpml": (C.c_int, [p, p, p, p, C.c_int, C.c_int, C.c_int, p]),
        "fdtd_set_mur": (C.c_int, [p, p, p]),
        "fdtd_set_signal": (C.c_int, [p, p, C.c_int]),
        "fdtd_add_source": (C.c_int, [p, C.c_int, p, p, p, p]),
        "fdtd_add_probe": (C.c_int, [p, C.c_int, C.c_int, p, p, p, C.POINTER(C.c_int)]),
        "fdtd_get_probe": (C.c_int, [p, C.c_int, p, C.c_int, C.POINTER(C.c_int)]),
        "fdtd_set_dft": (C.c_int, [p, C.c_int, C.c_int, C.c_int, p, p]),
        "fdtd_add_dft_box": (C.c_int, [p, C.c_int, C.c_int, p, p, C.POINTER(C.c_int)]),
        "fdtd_get_dft_box": (C.c_int, [p, C.c_int, p, p, p]),
        "fdtd_set_recorder": (C.c_int, [p, C.c_int, C.c_int]),
        "fdtd_rec_transform": (C.c_int, [p, C.c_int, C.c_int, p, p, p, p]),
        "fdtd_run": (C.c_int, [p, C.c_int]),
        "fdtd_run_profiled": (C.c_int, [p, C.c_int, C.POINTER(FdtdProfile)]),
        "fdtd_get_step": (C.c_int, [p, C.POINTER(C.c_int64)]),
        "fdtd_energy": (C.c_int, [p, p]),
        "fdtd_p2p_export": (C.c_int, [p, p]),
        "fdtd_p2p_attach": (C.c_int, [p, p, p]),
        "fdtd_p2p_selftest": (C.c_int, [p, C.c_uint]),
        "fdtd_p2p_detach": (C.c_int, [p]),
        "fdtd_p2p_link_info": (C.c_int, [p, C.c_int, p]),
        "fdtd_schedule_info": (C.c_int, [p, p]),
        "fdtd_comm_unique_id": (C.c_int, [p]),
        "fdtd_comm_init": (C.c_int, [p, p]),
        "fdtd_comm_nranks": (C.c_int, [p, C.POINTER(C.c_int)]),
        "fdtd_link": (C.c_int, [p, p]),
        "fdtd_run_linked": (C.c_int, [C.POINTER(p), C.c_int, C.c_int]),
        "fdtd_half_step": (C.c_int, [p, C.c_int]),
        "fdtd_halo_get": (C.c_int, [p, C.c_int, p]),
        "fdtd_halo_put": (C.c_int, [p, C.c_int, p]),
        "fdtd_get_field": (C.c_int, [p, C.c_int, C.c_int, p]),
        "fdtd_set_field": (C.c_int, [p, C.c_int, C.c_int, p]),
        "fdtd_farfield": (C.c_int, [C.c_int, C.c_int, p, p, p, C.c_double, C.c_int, p, p, p, p]),
    }
    assert sorted(sig) == sorted(ABI_SYMBOLS)
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    sheet_sig = {
        "fdtd_sheet_set": (C.c_int, [p, C.c_int, p, p, p, p, C.c_int, C.c_int, p, p]),
        "fdtd_sheet_get": (C.c_int, [p, p, p]),
    }
    assert sorted(sheet_sig) == sorted(SHEET_SYMBOLS)
    for name, (res, args) in sheet_sig.items():     # optional: bound when the library has them
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    debye_sig = {
        "fdtd_debye_set": (C.c_int, [p, C.c_int, C.c_int, p, p, p, p, p, p, p]),
        "fdtd_debye_get": (C.c_int, [p, C.c_int, p, p, p]),
    }
    assert sorted(debye_sig) == sorted(DEBYE_SYMBOLS)
    for name, (res, args) in debye_sig.items():     # optional, as the sheets' entry points are
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    lorentz_sig = {
        "fdtd_lorentz_set": (C.c_int, [p, C.c_int, C.c_int, p, p, p, p, p, p, p]),
        "fdtd_lorentz_get": (C.c_int, [p, C.c_int, p, p, p]),
    }
    assert sorted(lorentz_sig) == sorted(LORENTZ_SYMBOLS)
    for name, (res, args) in lorentz_sig.items():   # optional, likewise
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    lumped_sig = {
        "fdtd_lumped_set": (C.c_int, [p, C.c_int, p, p, p, p, C.c_int, p, p, p]),
        "fdtd_lumped_get": (C.c_int, [p, p, p]),
    }
    assert sorted(lumped_sig) == sorted(LUMPED_SYMBOLS)
    for name, (res, args) in lumped_sig.items():    # optional, likewise
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    magnetic_sig = {
        "fdtd_magnetic_set": (C.c_int, [p, C.c_int, p, p, p, p, p]),
        "fdtd_magnetic_get": (C.c_int, [p, C.c_int, p, p]),
    }
    assert sorted(magnetic_sig) == sorted(MAGNETIC_SYMBOLS)
    for name, (res, args) in magnetic_sig.items():  # optional, likewise
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    traffic_sig = {"fdtd_traffic_info": (C.c_int, [p, p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)])}
    assert sorted(traffic_sig) == sorted(TRAFFIC_SYMBOLS)
    for name, (res, args) in traffic_sig.items():   # optional, likewise
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    voxel_sig = {
        "fdtd_voxelize": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, p, C.c_int, p, C.c_int, p, C.c_double, p, p]),
    }
    assert sorted(voxel_sig) == sorted(VOXEL_SYMBOLS)
    for name, (res, args) in voxel_sig.items():     # optional, likewise
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    disc_sig = {
        "fdtd_voxelize_maps": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, p, C.c_int, p, C.c_int, p, C.c_double, p, p, p, C.c_int, p, p]),
    }
    assert sorted(disc_sig) == sorted(DISCMATERIAL_SYMBOLS)
    for name, (res, args) in disc_sig.items():      # optional, likewise
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    conformal_sig = {
        "fdtd_conformal_set": (C.c_int, [p, C.c_int, p, p, p]),
        "fdtd_conformal_get": (C.c_int, [p, p, p]),
        "fdtd_voxel_fractions": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, p, C.c_int, p, C.c_int, p, C.c_double, C.c_double,
                                           C.c_int, p, C.c_int64, p, p, p]),
    }
    assert sorted(conformal_sig) == sorted(CONFORMAL_SYMBOLS)
    for name, (res, args) in conformal_sig.items():  # optional, likewise
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    subcell_sig = {"fdtd_voxel_subcell": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, p, C.c_int, p, C.c_int, p, C.c_double, p, C.c_int, C.c_int,
                                                   p, p, p, p, C.c_int64, p, p, p, p, p, p])}
    assert sorted(subcell_sig) == sorted(SUBCELL_SYMBOLS)
    for name, (res, args) in subcell_sig.items():    # optional, likewise
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    planewave_sig = {"fdtd_planewave_set": (C.c_int, [p, C.c_int, p, p, p, p, p, C.c_int, p, p, p, p, p, p, C.c_int])}
    assert sorted(planewave_sig) == sorted(PLANEWAVE_SYMBOLS)
    for name, (res, args) in planewave_sig.items():  # optional, likewise
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    excite_sig = {"fdtd_excite_set": (C.c_int, [p, C.c_int, p, p, p, p, C.c_int, p, p, p, p, p, C.c_int])}
    assert sorted(excite_sig) == sorted(EXCITE_SYMBOLS)
    for name, (res, args) in excite_sig.items():     # optional, likewise
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    sar_sig = {
        "fdtd_sar_local": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, p, p, p, p, p, p, p, p, p, p]),
        "fdtd_sar_average": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, p, p, p, p, p, C.c_double, C.c_int, p, p, p, p]),
    }
    assert sorted(sar_sig) == sorted(SAR_SYMBOLS)
    for name, (res, args) in sar_sig.items():        # optional, likewise
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    fields_sig = {"fdtd_field_interp": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, p, p, p, p, p, p, p, p, p, p, p, p, p, p])}
    assert sorted(fields_sig) == sorted(FIELDS_SYMBOLS)
    for name, (res, args) in fields_sig.items():     # optional, likewise
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    mirror_sig = {"fdtd_farfield_mirror": (C.c_int, [C.c_int, C.c_int, p, p, p, C.c_double, C.c_int, p, p, p, C.c_int, C.c_int, p, p, p, p])}
    assert sorted(mirror_sig) == sorted(FARFIELD_MIRROR_SYMBOLS)
    for name, (res, args) in mirror_sig.items():     # optional, likewise
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    aniso_sig = {"fdtd_build_operator_axes": (C.c_int, [p, p, p, p, C.POINTER(p), C.POINTER(p), p, C.c_double, C.c_int, p, p, p, p, p, p, C.c_int])}
    assert sorted(aniso_sig) == sorted(ANISO_SYMBOLS)
    for name, (res, args) in aniso_sig.items():      # optional, likewise
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    return lib


def has_aniso(lib: C.CDLL) -> bool:
    """Whether `lib` exports the operator build with per-axis cell arrays (include/fdtd_hip_aniso.h)."""
    return all(hasattr(lib, n) for n in ANISO_SYMBOLS)


def has_farfield_mirror(lib: C.CDLL) -> bool:
    """Whether `lib` exports the radiation integral with mirror planes (include/fdtd_hip_farfield.h)."""
    return all(hasattr(lib, n) for n in FARFIELD_MIRROR_SYMBOLS)


def has_fields(lib: C.CDLL) -> bool:
    """Whether `lib` exports the field-dump entry point (include/fdtd_hip_fields.h)."""
    return all(hasattr(lib, n) for n in FIELDS_SYMBOLS)


def has_sar(lib: C.CDLL) -> bool:
    """Whether `lib` exports the SAR entry points (include/fdtd_hip_sar.h)."""
    return all(hasattr(lib, n) for n in SAR_SYMBOLS)


def has_excite(lib: C.CDLL) -> bool:
    """Whether `lib` exports the H-field excitation entry point (include/fdtd_hip_excite.h)."""
    return all(hasattr(lib, n) for n in EXCITE_SYMBOLS)


def has_planewave(lib: C.CDLL) -> bool:
    """Whether `lib` exports the plane-wave entry point (include/fdtd_hip_planewave.h)."""
    return all(hasattr(lib, n) for n in PLANEWAVE_SYMBOLS)


def has_conformal(lib: C.CDLL) -> bool:
    """Whether `lib` exports the conformal-boundary entry points (include/fdtd_hip_conformal.h)."""
    return all(hasattr(lib, n) for n in CONFORMAL_SYMBOLS)


def has_subcell(lib: C.CDLL) -> bool:
    """Whether `lib` exports the sub-cell sampling entry point (include/fdtd_hip_subcell.h)."""
    return all(hasattr(lib, n) for n in SUBCELL_SYMBOLS)


def has_voxelize(lib: C.CDLL) -> bool:
    """Whether `lib` exports the device rasteriser (include/fdtd_hip_voxel.h)."""
    return all(hasattr(lib, n) for n in VOXEL_SYMBOLS)


def has_discmaterial(lib: C.CDLL) -> bool:
    """Whether `lib` exports the device rasteriser with voxel maps (include/fdtd_hip_voxel.h: fdtd_voxelize_maps)."""
    return all(hasattr(lib, n) for n in DISCMATERIAL_SYMBOLS)


def has_traffic_info(lib: C.CDLL) -> bool:
    """Whether `lib` exports fdtd_traffic_info (include/fdtd_hip_traffic.h)."""
    return all(hasattr(lib, n) for n in TRAFFIC_SYMBOLS)


def has_magnetic(lib: C.CDLL) -> bool:
    """Whether `lib` exports the magnetic-material entry points (include/fdtd_hip_magnetic.h)."""
    return all(hasattr(lib, n) for n in MAGNETIC_SYMBOLS)


def has_lumped(lib: C.CDLL) -> bool:
    """Whether `lib` exports the lumped-element entry points (include/fdtd_hip_lumped.h)."""
    return all(hasattr(lib, n) for n in LUMPED_SYMBOLS)


def has_dispersion(lib: C.CDLL) -> bool:
    """Whether `lib` exports the Debye-media entry points (include/fdtd_hip_dispersion.h)."""
    return all(hasattr(lib, n) for n in DEBYE_SYMBOLS)


def has_lorentz(lib: C.CDLL) -> bool:
    """Whether `lib` exports the Lorentz-media entry points (include/fdtd_hip_lorentz.h)."""
    return all(hasattr(lib, n) for n in LORENTZ_SYMBOLS)


def has_sheets(lib: C.CDLL) -> bool:
    """Whether `lib` exports the conducting-sheet entry points (include/fdtd_hip_sheet.h)."""
    return all(hasattr(lib, n) for n in SHEET_SYMBOLS)


def hip_library_path(lib_dir: Optional[str] = None) -> str:
    """<lib_dir>/libfdtd_hip.so; default: $FDTD_HIP_LIB_DIR, else the in-tree build under csrc/."""
    return os.path.join(lib_dir or os.environ.get("FDTD_HIP_LIB_DIR") or os.path.join(_HERE, "csrc"), HIP_LIB_NAME)


_hip_lib = None


def load_hip_library(lib_dir: Optional[str] = None) -> C.CDLL:
    """Load libfdtd_hip.so (built by __graft_entry__.build() / csrc/Makefile).  No fallback."""
    global _hip_lib
    if _hip_lib is not None and lib_dir is None:
        return _hip_lib
    path = hip_library_path(lib_dir)
    if not os.path.isfile(path):
        raise RuntimeError(
            f"{HIP_LIB_NAME} not found at {path}: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the FDTD hot path.")
    lib = bind(C.CDLL(path))
    if lib_dir is None:
        _hip_lib = lib
    return lib


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _arr(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


class FdtdError(RuntimeError):
    pass


class Engine:
    """Thin object wrapper over one fdtd_ctx (one z-slab on one device)."""

    def __init__(self, lib: C.CDLL, nx: int, ny: int, nz: int, dt: float, *, k0: int = 0,
                 nk: Optional[int] = None, rank: int = 0, world: int = 1, device: int = 0,
                 max_steps: int = 0, flags: int = 0):
        self.lib = lib
        nk = nz - k0 if nk is None else nk
        self.desc = FdtdDesc(nx, ny, nz, k0, nk, rank, world, device, max_steps, flags, dt)
        self._ctx = C.c_void_p()
        rc = lib.fdtd_create(C.byref(self.desc), C.byref(self._ctx))
        if rc != 0:
            msg = lib.fdtd_last_error(None)
            raise FdtdError(f"fdtd_create failed ({rc}): {msg.decode() if msg else ''}")
        self.nx, self.ny, self.nz, self.k0, self.nk = nx, ny, nz, k0, nk
        self._keep = []

    # -- plumbing ---------------------------------------------------------------------------
    def _ck(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.fdtd_last_error(self._ctx)
            raise FdtdError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def close(self):
        if self._ctx:
            self.lib.fdtd_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def backend(self) -> str:
        return self.lib.fdtd_backend().decode()

    @property
    def local_shape(self):
        return (self.nk, self.ny, self.nx)

    # -- operator -----------------------------------------------------------------------------
    def set_operator_raw(self, vv, vi, ii, iv):
        shp = (3,) + self.local_shape
        arrs = [_arr(a, np.float32) for a in (vv, vi, ii, iv)]
        for a in arrs:
            if a.shape != shp:
                raise ValueError(f"operator array shape {a.shape} != {shp}")
        self._ck(self.lib.fdtd_set_operator_raw(self._ctx, *[_ptr(a) for a in arrs]), "set_operator_raw")

    def set_operator_classes(self, ecls, cls_vv, cls_m, emet, hmet):
        shp = (3,) + self.local_shape
        ecls = _arr(ecls, np.uint8)
        if ecls.shape != shp:
            raise ValueError(f"class array shape {ecls.shape} != {shp}")
        cls_vv, cls_m = _arr(cls_vv, np.float32), _arr(cls_m, np.float32)
        emet, hmet = _arr(emet, np.float32), _arr(hmet, np.float32)
        tl = self.nx + self.ny + self.nk
        if emet.shape != (3, tl) or hmet.shape != (3, tl) or cls_vv.shape != cls_m.shape:
            raise ValueError("metric/class table shape mismatch")
        self._ck(self.lib.fdtd_set_operator_classes(self._ctx, _ptr(ecls), int(cls_vv.size), _ptr(cls_vv),
                                                    _ptr(cls_m), _ptr(emet), _ptr(hmet)), "set_operator_classes")

    def build_operator(self, d, eps_r, kappa, pec, eps0, overrides, emet, hmet, prefer_classes=True):
        """Operator set-up inside the library (on the GPU for libfdtd_hip.so).  d = (dx, dy, dz) primal edge
        lengths of the GLOBAL grid; eps_r/kappa per cell [nz-1][ny-1][nx-1]; pec [3][nz][ny][nx];
        overrides = (edge_index int64, comp int8, vv float32, m float32) for host-fixed (lumped) edges."""
        nx, ny, nz = self.nx, self.ny, self.nz
        dx, dy, dz = (_arr(a, np.float64) for a in d)
        if (dx.size, dy.size, dz.size) != (nx, ny, nz):
            raise ValueError("cell-size tables must have nx, ny, nz entries")
        eps_r, kappa = _arr(eps_r, np.float64), _arr(kappa, np.float64)
        if eps_r.shape != (nz - 1, ny - 1, nx - 1) or kappa.shape != eps_r.shape:
            raise ValueError("cell arrays must be [nz-1][ny-1][nx-1]")
        pec, (oe, oc, ov, om), emet, hmet = self._build_operator_rest(pec, overrides, emet, hmet)
        self._ck(self.lib.fdtd_build_operator(self._ctx, _ptr(dx), _ptr(dy), _ptr(dz), _ptr(eps_r), _ptr(kappa), _ptr(pec),
                                              float(eps0), int(oe.size), _ptr(oe), _ptr(oc), _ptr(ov), _ptr(om),
                                              _ptr(emet), _ptr(hmet), 1 if prefer_classes else 0), "build_operator")

    def build_operator_axes(self, d, eps_axes, kappa_axes, pec, eps0, overrides, emet, hmet, prefer_classes=True):
        """build_operator for anisotropic dielectrics (include/fdtd_hip_aniso.h): eps_axes / kappa_axes per cell and axis
        [3][nz-1][ny-1][nx-1] — the edges of component c read slice c; every other argument as build_operator's.  Needs a library that
        exports fdtd_build_operator_axes (has_aniso): there is no other path to the device build."""
        if not has_aniso(self.lib):
            raise FdtdError("build_operator_axes: this library does not export fdtd_build_operator_axes (include/fdtd_hip_aniso.h)")
        nx, ny, nz = self.nx, self.ny, self.nz
        dx, dy, dz = (_arr(a, np.float64) for a in d)
        if (dx.size, dy.size, dz.size) != (nx, ny, nz):
            raise ValueError("cell-size tables must have nx, ny, nz entries")
        eps_axes, kappa_axes = _arr(eps_axes, np.float64), _arr(kappa_axes, np.float64)
        if eps_axes.shape != (3, nz - 1, ny - 1, nx - 1) or kappa_axes.shape != eps_axes.shape:
            raise ValueError("per-axis cell arrays must be [3][nz-1][ny-1][nx-1]")
        pec, (oe, oc, ov, om), emet, hmet = self._build_operator_rest(pec, overrides, emet, hmet)
        e3 = (C.c_void_p * 3)(*[eps_axes[c].ctypes.data for c in range(3)])
        k3 = (C.c_void_p * 3)(*[kappa_axes[c].ctypes.data for c in range(3)])
        self._ck(self.lib.fdtd_build_operator_axes(self._ctx, _ptr(dx), _ptr(dy), _ptr(dz), e3, k3, _ptr(pec),
                                                   float(eps0), int(oe.size), _ptr(oe), _ptr(oc), _ptr(ov), _ptr(om),
                                                   _ptr(emet), _ptr(hmet), 1 if prefer_classes else 0), "build_operator_axes")

    def _build_operator_rest(self, pec, overrides, emet, hmet):
        """The checks build_operator and build_operator_axes share: pec, the override lists, the metric tables."""
        nx, ny, nz = self.nx, self.ny, self.nz
        pec = np.ascontiguousarray(pec)
        if pec.dtype == np.bool_:
            pec = pec.view(np.uint8)
        pec = _arr(pec, np.uint8)
        if pec.shape != (3, nz, ny, nx):
            raise ValueError("pec must be [3][nz][ny][nx]")
        oe, oc, ov, om = overrides
        oe, oc, ov, om = _arr(oe, np.int64), _arr(oc, np.int8), _arr(ov, np.float32), _arr(om, np.float32)
        if not (oe.size == oc.size == ov.size == om.size):
            raise ValueError("override arrays differ in length")
        emet, hmet = _arr(emet, np.float32), _arr(hmet, np.float32)
        tl = nx + ny + self.nk
        if emet.shape != (3, tl) or hmet.shape != (3, tl):
            raise ValueError("metric table shape mismatch")
        return pec, (oe, oc, ov, om), emet, hmet

    def operator_form(self):
        """('none' | 'classes' | 'classes-packed' | 'raw', number of distinct (vv, m) pairs)."""
        form, ncls = C.c_int(0), C.c_int(0)
        self._ck(self.lib.fdtd_operator_form(self._ctx, C.byref(form), C.byref(ncls)), "operator_form")
        return ("none", "classes", "classes-packed", "raw")[form.value], int(ncls.value)

    def get_operator(self):
        """(vv, vi, ii, iv) float32 [3][nk][ny][nx]: the operator that is set, expanded."""
        out = [np.empty((3,) + self.local_shape, np.float32) for _ in range(4)]
        self._ck(self.lib.fdtd_get_operator(self._ctx, *[_ptr(a) for a in out]), "get_operator")
        return tuple(out)

    # -- boundaries ---------------------------------------------------------------------------
    def set_cpml(self, slot_x, slot_y, slot_z, nsx, nsy, nsz, coef):
        sx, sy, sz = _arr(slot_x, np.int32), _arr(slot_y, np.int32), _arr(slot_z, np.int32)
        coef = _arr(coef, np.float32)
        if sx.size != self.nx or sy.size != self.ny or sz.size != self.nk:
            raise ValueError("cpml slot table length mismatch")
        if coef.size != 6 * (self.nx + self.ny + self.nk):
            raise ValueError("cpml coefficient block size mismatch")
        self._ck(self.lib.fdtd_set_cpml(self._ctx, _ptr(sx), _ptr(sy), _ptr(sz), int(nsx), int(nsy), int(nsz),
                                        _ptr(coef)), "set_cpml")

    def set_mur(self, enable, coeff):
        en, co = _arr(enable, np.int32), _arr(coeff, np.float32)
        if en.size != 6 or co.size != 6:
            raise ValueError("mur needs 6 faces")
        self._ck(self.lib.fdtd_set_mur(self._ctx, _ptr(en), _ptr(co)), "set_mur")

    # -- excitation / probes / dft -----------------------------------------------------------------
    def set_signal(self, sig):
        sig = _arr(sig, np.float32)
        self._ck(self.lib.fdtd_set_signal(self._ctx, _ptr(sig), int(sig.size)), "set_signal")

    def add_source(self, idx, comp, amp, delay=None):
        idx = _arr(idx, np.int64)
        comp = _arr(comp, np.int8)
        amp = _arr(amp, np.float32)
        delay = np.zeros(idx.size, np.int32) if delay is None else _arr(delay, np.int32)
        if not (idx.size == comp.size == amp.size == delay.size):
            raise ValueError("source arrays differ in length")
        self._ck(self.lib.fdtd_add_source(self._ctx, int(idx.size), _ptr(idx), _ptr(comp), _ptr(amp), _ptr(delay)),
                 "add_source")

    def add_probe(self, kind, idx, comp, w) -> int:
        idx, comp, w = _arr(idx, np.int64), _arr(comp, np.int8), _arr(w, np.float32)
        if not (idx.size == comp.size == w.size):
            raise ValueError("probe arrays differ in length")
        pid = C.c_int(-1)
        self._ck(self.lib.fdtd_add_probe(self._ctx, int(kind), int(idx.size), _ptr(idx), _ptr(comp), _ptr(w),
                                         C.byref(pid)), "add_probe")
        return pid.value

    def get_probe(self, pid: int) -> np.ndarray:
        n = C.c_int(0)
        self._ck(self.lib.fdtd_get_probe(self._ctx, pid, None, 0, C.byref(n)), "get_probe")
        out = np.zeros(max(n.value, 1), np.float64)
        self._ck(self.lib.fdtd_get_probe(self._ctx, pid, _ptr(out), n.value, C.byref(n)), "get_probe")
        return out[:n.value]

    def set_dft(self, every: int, tw_v: np.ndarray, tw_i: np.ndarray):
        tw_v, tw_i = _arr(tw_v, np.float64), _arr(tw_i, np.float64)
        if tw_v.shape != tw_i.shape or tw_v.ndim != 3 or tw_v.shape[2] != 2:
            raise ValueError("twiddles must be [nsamples][nfreq][2]")
        self.nfreq = tw_v.shape[1]
        self._ck(self.lib.fdtd_set_dft(self._ctx, tw_v.shape[1], int(every), tw_v.shape[0], _ptr(tw_v), _ptr(tw_i)),
                 "set_dft")

    def set_recorder(self, every: int, nsamples: int):
        """Boxes keep their time-domain samples (float32) on the device instead of running-DFT sums; `rec_transform`
        turns them into any frequency set afterwards."""
        self.nfreq = 0
        self.rec_every, self.rec_nsamples = int(every), int(nsamples)
        self._ck(self.lib.fdtd_set_recorder(self._ctx, int(every), int(nsamples)), "set_recorder")

    def rec_transform(self, bid: int, tw: np.ndarray):
        """(complex128 [nfreq][kk][jj][ii], lo_own, hi_own) of a recorded box for the twiddle table tw
        [nsamples][nfreq][2] of the box's field kind."""
        tw = _arr(tw, np.float64)
        if tw.ndim != 3 or tw.shape[2] != 2 or tw.shape[0] != self.rec_nsamples:
            raise ValueError("twiddles must be [nsamples][nfreq][2]")
        nf = tw.shape[1]
        lo, hi = np.zeros(3, np.int32), np.zeros(3, np.int32)
        self._ck(self.lib.fdtd_rec_transform(self._ctx, bid, nf, None, None, _ptr(lo), _ptr(hi)), "rec_transform")
        ext = hi - lo + 1
        if np.any(ext <= 0):
            return np.zeros((nf, 0, 0, 0), np.complex128), lo, hi
        out = np.zeros((nf, ext[2], ext[1], ext[0], 2), np.float64)
        self._ck(self.lib.fdtd_rec_transform(self._ctx, bid, nf, _ptr(tw), _ptr(out), _ptr(lo), _ptr(hi)), "rec_transform")
        return out[..., 0] + 1j * out[..., 1], lo, hi

    def add_dft_box(self, kind, comp, lo, hi) -> int:
        lo, hi = _arr(lo, np.int32), _arr(hi, np.int32)
        bid = C.c_int(-1)
        self._ck(self.lib.fdtd_add_dft_box(self._ctx, int(kind), int(comp), _ptr(lo), _ptr(hi), C.byref(bid)),
                 "add_dft_box")
        return bid.value

    def get_dft_box(self, bid: int):
        """(complex128 [nfreq][kk][jj][ii], lo_own, hi_own); the array is empty if the slab owns nothing."""
        lo, hi = np.zeros(3, np.int32), np.zeros(3, np.int32)
        self._ck(self.lib.fdtd_get_dft_box(self._ctx, bid, None, _ptr(lo), _ptr(hi)), "get_dft_box")
        ext = hi - lo + 1
        if np.any(ext <= 0):
            return np.zeros((self.nfreq, 0, 0, 0), np.complex128), lo, hi
        out = np.zeros((self.nfreq, ext[2], ext[1], ext[0], 2), np.float64)
        self._ck(self.lib.fdtd_get_dft_box(self._ctx, bid, _ptr(out), _ptr(lo), _ptr(hi)), "get_dft_box")
        return out[..., 0] + 1j * out[..., 1], lo, hi

    # -- stepping -----------------------------------------------------------------------------
    def run(self, nsteps: int):
        self._ck(self.lib.fdtd_run(self._ctx, int(nsteps)), "run")

    def run_profiled(self, nsteps: int) -> FdtdProfile:
        prof = FdtdProfile()
        self._ck(self.lib.fdtd_run_profiled(self._ctx, int(nsteps), C.byref(prof)), "run_profiled")
        return prof

    @property
    def step(self) -> int:
        s = C.c_int64(0)
        self._ck(self.lib.fdtd_get_step(self._ctx, C.byref(s)), "get_step")
        return s.value

    def energy(self):
        s = np.zeros(2, np.float64)
        self._ck(self.lib.fdtd_energy(self._ctx, _ptr(s)), "energy")
        return float(s[0]), float(s[1])

    def half_step(self, phase: int):
        self._ck(self.lib.fdtd_half_step(self._ctx, int(phase)), "half_step")

    def halo_get(self, which: int) -> np.ndarray:
        buf = np.empty((2, self.ny, self.nx), np.float32)
        self._ck(self.lib.fdtd_halo_get(self._ctx, int(which), _ptr(buf)), "halo_get")
        return buf

    def halo_put(self, which: int, buf: np.ndarray):
        buf = _arr(buf, np.float32)
        if buf.shape != (2, self.ny, self.nx):
            raise ValueError("halo buffer must be [2][ny][nx]")
        self._ck(self.lib.fdtd_halo_put(self._ctx, int(which), _ptr(buf)), "halo_put")

    def p2p_export(self) -> bytes:
        """128-byte description of this context's halo mailbox (IPC handle) for the neighbour ranks."""
        buf = C.create_string_buffer(128)
        self._ck(self.lib.fdtd_p2p_export(self._ctx, buf), "p2p_export")
        return buf.raw

    def p2p_attach(self, lower: Optional[bytes], upper: Optional[bytes]):
        """Attach the mailboxes of rank-1 / rank+1 (None where there is no neighbour): halos then travel inside the
        update kernels (csrc/kernels.hip, P2P variants)."""
        lo = C.create_string_buffer(lower, 128) if lower is not None else None
        hi = C.create_string_buffer(upper, 128) if upper is not None else None
        self._ck(self.lib.fdtd_p2p_attach(self._ctx, lo, hi), "p2p_attach")

    def p2p_selftest(self, token: int = 0x5E1F0001):
        self._ck(self.lib.fdtd_p2p_selftest(self._ctx, int(token)), "p2p_selftest")

    def p2p_detach(self):
        self._ck(self.lib.fdtd_p2p_detach(self._ctx), "p2p_detach")

    LINK_TYPES = {0: "hypertransport", 1: "qpi", 2: "pcie", 3: "infiniband", 4: "xgmi"}

    def p2p_link_info(self, which: int) -> dict:
        """The link to the attached lower (which=0) / upper (1) neighbour's GPU (fdtd_p2p_link_info)."""
        a = np.full(8, -1, np.int32)
        self._ck(self.lib.fdtd_p2p_link_info(self._ctx, int(which), _ptr(a)), "p2p_link_info")
        return {"device": int(a[0]), "mapping": {1: "same-process", 2: "ipc"}.get(int(a[1]), None),
                "link": self.LINK_TYPES.get(int(a[2]), None if a[2] < 0 else f"type{int(a[2])}"), "hops": int(a[3]),
                "perf_rank": int(a[4]), "access": int(a[5]), "native_atomics": int(a[6]), "same_device": bool(a[7] == 1)}

    def schedule_info(self) -> dict:
        """Launches per timestep, lag, tiling and halo transport of this context (fdtd_schedule_info)."""
        a = np.zeros(8, np.int32)
        self._ck(self.lib.fdtd_schedule_info(self._ctx, _ptr(a)), "schedule_info")
        return {"launches_per_timestep": int(a[0]), "lag_planes": int(a[1]), "resident": bool(a[1] == -1), "rows_per_strip": int(a[2]),
                "blocks_per_sweep": int(a[3]),
                "transport": ("none", "p2p", "rccl", "linked", "external")[int(a[4])] if 0 <= a[4] <= 4 else None,
                "xcd_shares_weighted": bool(a[5]), "xcd_adaptations": int(a[6]), "timesteps_per_launch_max": int(a[7])}

    def traffic_info(self) -> dict:
        """Inert CPML indices skipped per axis and side, distinct class rows (0: per-cell bytes) and the estimate of bytes per
        timestep saved (fdtd_traffic_info, include/fdtd_hip_traffic.h; libfdtd_hip.so only)."""
        if not has_traffic_info(self.lib):
            raise FdtdError(f"this library ({self.backend}) has no fdtd_traffic_info")
        a = np.zeros(6, np.int32)
        rows, saved = C.c_int32(0), C.c_int64(0)
        self._ck(self.lib.fdtd_traffic_info(self._ctx, _ptr(a), C.byref(rows), C.byref(saved)), "traffic_info")
        return {"psi_skipped": {ax: {"E": int(a[2 * n]), "H": int(a[2 * n + 1])} for n, ax in enumerate("xyz")},
                "class_rows": int(rows.value), "bytes_saved_per_timestep": int(saved.value)}

    def comm_nranks(self) -> int:
        """Ranks of the RCCL communicator attached to this context (0: none)."""
        n = C.c_int(0)
        self._ck(self.lib.fdtd_comm_nranks(self._ctx, C.byref(n)), "comm_nranks")
        return n.value

    def comm_init(self, uid: bytes):
        if len(uid) != 128:
            raise ValueError("unique id must be 128 bytes")
        buf = C.create_string_buffer(uid, 128)
        self._ck(self.lib.fdtd_comm_init(self._ctx, buf), "comm_init")

    # -- the corrections: what they share -----------------------------------------------------------
    _CORRECTIONS = {   # what a library may lack: how to ask it, what to say
        "sheet": (has_sheets, "conducting sheets (fdtd_sheet_set / fdtd_sheet_get)"),
        "lumped": (has_lumped, "lumped elements (fdtd_lumped_set / fdtd_lumped_get)"),
        "debye": (has_dispersion, "Debye media (fdtd_debye_set / fdtd_debye_get)"),
        "lorentz": (has_lorentz, "Lorentz media (fdtd_lorentz_set / fdtd_lorentz_get)"),
        "magnetic": (has_magnetic, "magnetic materials (fdtd_magnetic_set / fdtd_magnetic_get)"),
        "conformal": (has_conformal, "conformal boundaries (fdtd_conformal_set / fdtd_conformal_get)"),
        "planewave": (has_planewave, "plane-wave excitation (fdtd_planewave_set)"),
        "excite": (has_excite, "H-field excitations (fdtd_excite_set)"),
    }

    def _need(self, correction: str):
        """Raise unless the loaded library exports the correction's entry points."""
        has, what = self._CORRECTIONS[correction]
        if not has(self.lib):
            raise FdtdError(f"this library ({self.backend}) has no {what}")

    @staticmethod
    def _boxes(lo, hi, fields, who: str, what: str):
        """The per-component boxes lo[c] <= (x, y, z) < hi[c] of a dense correction and its arrays over them, `fields` = (values per
        component, dtype, whether None stands for zeros)...: (lo, hi as int32 [3][3]; shapes [z][y][x] per component; per field the pointer triple the C
        side takes; the arrays behind the pointers, to be kept until the call has returned).  Empty boxes take empty arrays."""
        lo_a = _arr(np.asarray(lo).reshape(3, 3), np.int32)
        hi_a = _arr(np.asarray(hi).reshape(3, 3), np.int32)
        shapes = [tuple(int(max(0, hi_a[c, a] - lo_a[c, a])) for a in (2, 1, 0)) for c in range(3)]
        keep, ptrs = [], []
        for vals, dtype, optional in fields:
            arrs = [_arr(np.zeros(shapes[c], dtype) if (0 in shapes[c] or (optional and vals is None)) else vals[c], dtype) for c in range(3)]
            for c in range(3):
                if arrs[c].shape != shapes[c]:
                    raise ValueError(f"{who} component {c}: {what} must be [z][y][x] over the box, {shapes[c]}")
            keep.append(arrs)
            ptrs.append(C.cast((C.c_void_p * 3)(*[x.ctypes.data for x in arrs]), C.c_void_p))
        return lo_a, hi_a, shapes, ptrs, keep

    # -- conducting sheets (include/fdtd_hip_sheet.h) ------------------------------------------------
    def set_sheets(self, idx, comp, vi, cls, alpha, b):
        """Sheet edges: global flat node index, component, full vi coefficient, class; alpha / b: [ncls][K] (b = scale * b_k)."""
        self._need("sheet")
        idx, comp, vi, cls = _arr(idx, np.int64), _arr(comp, np.int8), _arr(vi, np.float32), _arr(cls, np.int32)
        alpha, b = _arr(alpha, np.float32), _arr(b, np.float32)
        if not (idx.size == comp.size == vi.size == cls.size) or alpha.ndim != 2 or alpha.shape != b.shape:
            raise ValueError("sheet arrays differ in length / class tables must be [ncls][K]")
        ncls, K = alpha.shape
        self._ck(self.lib.fdtd_sheet_set(self._ctx, int(idx.size), _ptr(idx), _ptr(comp), _ptr(vi), _ptr(cls), int(ncls), int(K),
                                         _ptr(alpha), _ptr(b)), "sheet_set")
        self.sheet_n, self.sheet_K = int(idx.size), int(K)

    def sheet_state(self):
        """(v_prev float32 [n], branch currents float32 [K][n]) of the sheet edges."""
        self._need("sheet")
        n, K = getattr(self, "sheet_n", 0), getattr(self, "sheet_K", 0)
        v = np.zeros(n, np.float32)
        ib = np.zeros((K, n), np.float32)
        self._ck(self.lib.fdtd_sheet_get(self._ctx, _ptr(v), _ptr(ib)), "sheet_get")
        return v, ib

    # -- lumped R-L-C elements (include/fdtd_hip_lumped.h) -------------------------------------------
    def set_lumped(self, idx, comp, vi, cls, phi, gam, h):
        """Element edges: global flat node index, component, full vi coefficient, class; phi [ncls][2][2], gam / h [ncls][2]."""
        self._need("lumped")
        idx, comp, vi, cls = _arr(idx, np.int64), _arr(comp, np.int8), _arr(vi, np.float32), _arr(cls, np.int32)
        phi, gam, h = _arr(phi, np.float32), _arr(gam, np.float32), _arr(h, np.float32)
        if idx.size == 0:
            phi, gam, h = phi.reshape(-1, 2, 2), gam.reshape(-1, 2), h.reshape(-1, 2)
        if (not (idx.size == comp.size == vi.size == cls.size) or phi.ndim != 3 or phi.shape[1:] != (2, 2)
                or gam.shape != (phi.shape[0], 2) or h.shape != gam.shape):
            raise ValueError("lumped arrays differ in length / class tables must be phi [ncls][2][2], gam [ncls][2], h [ncls][2]")
        self._ck(self.lib.fdtd_lumped_set(self._ctx, int(idx.size), _ptr(idx), _ptr(comp), _ptr(vi), _ptr(cls), int(phi.shape[0]),
                                          _ptr(phi), _ptr(gam), _ptr(h)), "lumped_set")
        self.lumped_n = int(idx.size)

    def lumped_state(self):
        """(v_prev float32 [n], states float32 [2][n]) of the element edges."""
        self._need("lumped")
        n = getattr(self, "lumped_n", 0)
        v = np.zeros(n, np.float32)
        x = np.zeros((2, n), np.float32)
        self._ck(self.lib.fdtd_lumped_get(self._ctx, _ptr(v), _ptr(x)), "lumped_get")
        return v, x

    # -- Debye media (include/fdtd_hip_dispersion.h) -------------------------------------------------
    def set_debye(self, alpha, oma, beta, lo, hi, w, med=None):
        """Media tables alpha, oma = 1 - alpha, beta: float32 [nmedia][K]; per component c the box lo[c] <= (x, y, z) < hi[c] of
        edges with the weights w[c] and medium ids med[c] over it, [z][y][x] (an empty box: the component has no dispersive edge)."""
        self._need("debye")
        alpha, oma, beta = _arr(alpha, np.float32), _arr(oma, np.float32), _arr(beta, np.float32)
        if alpha.ndim != 2 or alpha.shape != oma.shape or alpha.shape != beta.shape:
            raise ValueError("Debye tables must be [nmedia][K]")
        nmedia, K = alpha.shape
        lo_a, hi_a, shapes, (wp, mp), _keep = self._boxes(lo, hi, [(w, np.float32, False), (med, np.uint8, True)], "Debye", "weights / medium ids")
        self._ck(self.lib.fdtd_debye_set(self._ctx, int(nmedia), int(K), _ptr(alpha), _ptr(oma), _ptr(beta), _ptr(lo_a), _ptr(hi_a), wp, mp),
                 "debye_set")
        self.debye_K, self.debye_shapes = int(K), shapes

    def debye_state(self, comp: int):
        """(v_prev [z][y][x], u [K][z][y][x], vi [z][y][x]) float32 over component comp's box."""
        self._need("debye")
        shp = getattr(self, "debye_shapes", [(0, 0, 0)] * 3)[comp]
        K = getattr(self, "debye_K", 0)
        v, u, vi = np.zeros(shp, np.float32), np.zeros((K,) + shp, np.float32), np.zeros(shp, np.float32)
        self._ck(self.lib.fdtd_debye_get(self._ctx, int(comp), _ptr(v), _ptr(u), _ptr(vi)), "debye_get")
        return v, u, vi

    # -- Lorentz / Drude media (include/fdtd_hip_lorentz.h) ------------------------------------------
    def set_lorentz(self, phi, gam, h, lo, hi, w, med=None):
        """Media tables phi: float32 [nmedia][K][2][2], gam, h: [nmedia][K][2]; per component c the box lo[c] <= (x, y, z) < hi[c] of
        edges with the weights w[c] and medium ids med[c] over it, [z][y][x] (an empty box: the component has no dispersive edge).
        No media (phi of length 0) removes the set."""
        self._need("lorentz")
        phi, gam, h = _arr(phi, np.float32), _arr(gam, np.float32), _arr(h, np.float32)
        if phi.ndim != 4 or phi.shape[2:] != (2, 2) or gam.shape != phi.shape[:2] + (2,) or h.shape != gam.shape:
            raise ValueError("Lorentz tables must be phi [nmedia][K][2][2], gam and h [nmedia][K][2]")
        nmedia, K = phi.shape[:2]
        lo_a, hi_a, shapes, (wp, mp), _keep = self._boxes(lo, hi, [(w, np.float32, False), (med, np.uint8, True)], "Lorentz", "weights / medium ids")
        self._ck(self.lib.fdtd_lorentz_set(self._ctx, int(nmedia), int(K), _ptr(phi), _ptr(gam), _ptr(h), _ptr(lo_a), _ptr(hi_a), wp, mp),
                 "lorentz_set")
        self.lorentz_K, self.lorentz_shapes = (int(K), shapes) if nmedia else (0, [(0, 0, 0)] * 3)

    def lorentz_state(self, comp: int):
        """(v_prev [z][y][x], x [K][2][z][y][x] (j_k, u_k), vi [z][y][x]) float32 over component comp's box."""
        self._need("lorentz")
        shp = getattr(self, "lorentz_shapes", [(0, 0, 0)] * 3)[comp]
        K = getattr(self, "lorentz_K", 0)
        v, x, vi = np.zeros(shp, np.float32), np.zeros((K, 2) + shp, np.float32), np.zeros(shp, np.float32)
        self._ck(self.lib.fdtd_lorentz_get(self._ctx, int(comp), _ptr(v), _ptr(x), _ptr(vi)), "lorentz_get")
        return v, x, vi

    # -- magnetic materials (include/fdtd_hip_magnetic.h) --------------------------------------------
    def set_magnetic(self, a, b, lo, hi, cls):
        """Class tables a, b: float32 [ncls] of the live classes 1..ncls; per component c the box lo[c] <= (x, y, z) < hi[c] of
        faces with the class bytes cls[c] over it, [z][y][x] (0: not magnetic; an empty box: the component has no magnetic face).
        An empty table removes the set."""
        self._need("magnetic")
        a, b = _arr(a, np.float32).ravel(), _arr(b, np.float32).ravel()
        if a.shape != b.shape:
            raise ValueError("magnetic tables must be a [ncls], b [ncls]")
        lo_a, hi_a, shapes, (cp,), _keep = self._boxes(lo, hi, [(cls, np.uint8, False)], "magnetic", "class bytes")
        self._ck(self.lib.fdtd_magnetic_set(self._ctx, int(a.size), _ptr(a), _ptr(b), _ptr(lo_a), _ptr(hi_a), cp), "magnetic_set")
        self.magnetic_shapes = shapes if a.size else [(0, 0, 0)] * 3

    def magnetic_state(self, comp: int):
        """(i_prev [z][y][x], iv0 [z][y][x]) float32 over component comp's box."""
        self._need("magnetic")
        shp = getattr(self, "magnetic_shapes", [(0, 0, 0)] * 3)[comp]
        ip, iv = np.zeros(shp, np.float32), np.zeros(shp, np.float32)
        self._ck(self.lib.fdtd_magnetic_get(self._ctx, int(comp), _ptr(ip), _ptr(iv)), "magnetic_get")
        return ip, iv

    # -- conformal PEC boundaries (include/fdtd_hip_conformal.h) ------------------------------------
    def set_conformal(self, comp, idx, coef):
        """The listed faces: comp int8 [n], idx int64 [n] (flat node index), coef float32 [n][4] = iv0 * g_e in the order of
        conformal.face_edges.  An empty list removes the set."""
        self._need("conformal")
        comp, idx = _arr(comp, np.int8).ravel(), _arr(idx, np.int64).ravel()
        coef = _arr(coef, np.float32).reshape(-1, 4)
        if not (comp.size == idx.size == coef.shape[0]):
            raise ValueError("conformal faces must be comp [n], idx [n], coef [n][4]")
        self._ck(self.lib.fdtd_conformal_set(self._ctx, int(idx.size), _ptr(comp), _ptr(idx), _ptr(coef)), "conformal_set")

    def conformal_state(self) -> np.ndarray:
        """i_prev float32 [n] of the listed faces, in the order they were set."""
        self._need("conformal")
        n = C.c_int(0)
        self._ck(self.lib.fdtd_conformal_get(self._ctx, None, C.byref(n)), "conformal_get")
        ip = np.zeros(n.value, np.float32)
        self._ck(self.lib.fdtd_conformal_get(self._ctx, _ptr(ip), None), "conformal_get")
        return ip

    # -- fields -------------------------------------------------------------------------------
    # -- plane-wave excitation (include/fdtd_hip_planewave.h) ----------------------------------------
    def set_planewave(self, idxE, compE, coefE, m0E, wE, idxH, compH, coefH, m0H, wH, sig2):
        """The edge list and the face list of planewave.tables (per list idx int64 [n], comp int8 [n], coef float32 [n][2], m0 int32
        [n][2], w float32 [n][2]) and the pulse at half-step resolution.  Two empty lists remove the set."""
        self._need("planewave")
        lists = []
        for idx, comp, coef, m0, w in ((idxE, compE, coefE, m0E, wE), (idxH, compH, coefH, m0H, wH)):
            idx, comp = _arr(idx, np.int64).ravel(), _arr(comp, np.int8).ravel()
            coef, m0, w = _arr(coef, np.float32).reshape(-1, 2), _arr(m0, np.int32).reshape(-1, 2), _arr(w, np.float32).reshape(-1, 2)
            if not (idx.size == comp.size == coef.shape[0] == m0.shape[0] == w.shape[0]):
                raise ValueError("plane-wave lists must be idx [n], comp [n], coef [n][2], m0 [n][2], w [n][2]")
            lists.append((idx, comp, coef, m0, w))
        sig2 = _arr(np.zeros(0) if sig2 is None else sig2, np.float32).ravel()
        args = []
        for l in lists:
            args += [int(l[0].size)] + [_ptr(a) if a.size else None for a in l]
        self._ck(self.lib.fdtd_planewave_set(self._ctx, *args, _ptr(sig2) if sig2.size else None, int(sig2.size)), "planewave_set")

    # -- H-field excitations (include/fdtd_hip_excite.h) ----------------------------------------------
    def set_excite(self, idxH, compH, ampH, delayH, idxS, compS, ampS, delayS, sigH):
        """The hard list and the soft list of field_excitation.ExcitationLists.h_args (per list idx int64 [n], comp int8 [n], amp float32 [n], delay
        int32 [n]) and the pulse at the half-steps, sigH[m] = s((m + 1/2) dt).  Two empty lists remove the set."""
        self._need("excite")
        lists = []
        for idx, comp, amp, delay in ((idxH, compH, ampH, delayH), (idxS, compS, ampS, delayS)):
            l = (_arr(idx, np.int64).ravel(), _arr(comp, np.int8).ravel(), _arr(amp, np.float32).ravel(), _arr(delay, np.int32).ravel())
            if not (l[0].size == l[1].size == l[2].size == l[3].size):
                raise ValueError("excitation lists must be idx [n], comp [n], amp [n], delay [n]")
            lists.append(l)
        sigH = _arr(np.zeros(0) if sigH is None else sigH, np.float32).ravel()
        args = []
        for l in lists:
            args += [int(l[0].size)] + [_ptr(a) if a.size else None for a in l]
        self._ck(self.lib.fdtd_excite_set(self._ctx, *args, _ptr(sigH) if sigH.size else None, int(sigH.size)), "excite_set")

    def get_field(self, kind: int, comp: int) -> np.ndarray:
        out = np.empty(self.local_shape, np.float32)
        self._ck(self.lib.fdtd_get_field(self._ctx, int(kind), int(comp), _ptr(out)), "get_field")
        return out

    def set_field(self, kind: int, comp: int, a: np.ndarray):
        a = _arr(a, np.float32)
        if a.shape != self.local_shape:
            raise ValueError("field shape mismatch")
        self._ck(self.lib.fdtd_set_field(self._ctx, int(kind), int(comp), _ptr(a)), "set_field")

    def fields(self):
        """All six components as [2][3][nk][ny][nx]."""
        return np.stack([np.stack([self.get_field(kind, c) for c in range(3)]) for kind in (KIND_V, KIND_I)])


def link(lower, upper):
    """fdtd_link: adjacent slabs of one process (or one FDTD_FLAG_LOOPBACK slab with itself)."""
    lower._ck(lower.lib.fdtd_link(lower._ctx, upper._ctx), "link")


def run_linked(engines, nsteps: int):
    """Step adjacent slabs that live in this process together (fdtd_link + fdtd_run_linked)."""
    lib = engines[0].lib
    for lo, hi in zip(engines[:-1], engines[1:]):
        lo._ck(lib.fdtd_link(lo._ctx, hi._ctx), "link")
    arr = (C.c_void_p * len(engines))(*[e._ctx for e in engines])
    rc = lib.fdtd_run_linked(arr, len(engines), int(nsteps))
    if rc != 0:   # the message sits in the context that failed, not necessarily the first one
        msgs = [f"rank {r}: {m.decode()}" for r, e in enumerate(engines) if (m := lib.fdtd_last_error(e._ctx))]
        raise FdtdError(f"run_linked failed ({rc}): " + "; ".join(msgs))


def comm_unique_id(lib: C.CDLL) -> bytes:
    buf = C.create_string_buffer(128)
    rc = lib.fdtd_comm_unique_id(buf)
    if rc != 0:
        msg = lib.fdtd_last_error(None)
        raise FdtdError(f"fdtd_comm_unique_id failed ({rc}): {msg.decode() if msg else ''}")
    return buf.raw


def farfield(lib: C.CDLL, pos, Js, Ms, k_wave: float, theta, phi, device: int = 0):
    """theta/phi: paired 1-D direction lists [rad].  Returns complex (E_theta, E_phi) * r."""
    pos = _arr(pos, np.float64)
    npts = pos.shape[0]
    Js = _arr(np.stack([np.real(Js), np.imag(Js)], -1), np.float64)
    Ms = _arr(np.stack([np.real(Ms), np.imag(Ms)], -1), np.float64)
    th, ph = _arr(theta, np.float64), _arr(phi, np.float64)
    if pos.shape != (npts, 3) or Js.shape != (npts, 3, 2) or Ms.shape != (npts, 3, 2) or th.shape != ph.shape:
        raise ValueError("farfield argument shapes")
    eth = np.zeros((th.size, 2), np.float64)
    eph = np.zeros((th.size, 2), np.float64)
    rc = lib.fdtd_farfield(int(device), int(npts), _ptr(pos), _ptr(Js), _ptr(Ms), float(k_wave), int(th.size),
                           _ptr(th), _ptr(ph), _ptr(eth), _ptr(eph))
    if rc != 0:
        msg = lib.fdtd_last_error(None)
        raise FdtdError(f"fdtd_farfield failed ({rc}): {msg.decode() if msg else ''}")
    return eth[:, 0] + 1j * eth[:, 1], eph[:, 0] + 1j * eph[:, 1]


def farfield_mirror(lib: C.CDLL, pos, Js, Ms, k_wave: float, theta, phi, mirrors=(), half_space: Optional[int] = None, device: int = 0):
    """farfield() over the points and their images in `mirrors`: a sequence of up to three (axis, type, coordinate) with type
    MIRROR_PEC / MIRROR_PMC (or 'PEC' / 'PMC') and the coordinate relative to the phase centre, like pos.  half_space = b names
    plane b as an infinite ground: exact zeros behind it.  The numpy statement is nf2ff.farfield_mirror_spec."""
    if not has_farfield_mirror(lib):
        raise FdtdError("this library has no radiation integral with mirror planes (fdtd_farfield_mirror)")
    pos = _arr(pos, np.float64)
    npts = pos.shape[0]
    Js = _arr(np.stack([np.real(Js), np.imag(Js)], -1), np.float64)
    Ms = _arr(np.stack([np.real(Ms), np.imag(Ms)], -1), np.float64)
    th, ph = _arr(theta, np.float64), _arr(phi, np.float64)
    if pos.shape != (npts, 3) or Js.shape != (npts, 3, 2) or Ms.shape != (npts, 3, 2) or th.shape != ph.shape:
        raise ValueError("farfield argument shapes")
    mirrors = [(int(a), {"PEC": MIRROR_PEC, "PMC": MIRROR_PMC}.get(t, t), float(c)) for a, t, c in mirrors]
    if len(mirrors) > 3:
        raise ValueError("farfield: at most three mirror planes")
    ax = _arr([m[0] for m in mirrors] + [0] * (3 - len(mirrors)), np.int32)
    ty = _arr([int(m[1]) for m in mirrors] + [0] * (3 - len(mirrors)), np.int32)
    co = _arr([m[2] for m in mirrors] + [0.0] * (3 - len(mirrors)), np.float64)
    eth = np.zeros((th.size, 2), np.float64)
    eph = np.zeros((th.size, 2), np.float64)
    rc = lib.fdtd_farfield_mirror(int(device), int(npts), _ptr(pos), _ptr(Js), _ptr(Ms), float(k_wave), len(mirrors), _ptr(ax), _ptr(ty),
                                  _ptr(co), -1 if half_space is None else int(half_space), int(th.size), _ptr(th), _ptr(ph), _ptr(eth), _ptr(eph))
    if rc != 0:
        msg = lib.fdtd_last_error(None)
        raise FdtdError(f"fdtd_farfield_mirror failed ({rc}): {msg.decode() if msg else ''}")
    return eth[:, 0] + 1j * eth[:, 1], eph[:, 0] + 1j * eph[:, 1]


def voxelize_raw(lib: C.CDLL, grid, table, device: int = 0, cells: bool = True, edges: bool = True):
    """fdtd_voxelize on a primitives.Table: (cell_owner int32 [nz-1][ny-1][nx-1] or None, edge_owner int32 [3][nz][ny][nx] or None)."""
    if not has_voxelize(lib):
        raise FdtdError("this library has no device rasteriser (fdtd_voxelize)")
    nx, ny, nz = grid.shape
    lines = _arr(np.concatenate(grid.lines), np.float64)
    rec = np.ascontiguousarray(table.rec)
    verts = _arr(table.verts, np.float64)
    if rec.dtype.itemsize != 248:
        raise ValueError("the table's records must be primitives.RECORD")
    cown = np.empty((nz - 1, ny - 1, nx - 1), np.int32) if cells else None
    eown = np.empty((3, nz, ny, nx), np.int32) if edges else None
    if getattr(table, "maps", None):
        return voxelize_maps_raw(lib, grid, table, device, cown, eown)
    rc = lib.fdtd_voxelize(int(device), nx, ny, nz, _ptr(lines), int(rec.size), _ptr(rec) if rec.size else None, int(verts.size),
                           _ptr(verts) if verts.size else None, float(table.tol), _ptr(cown), _ptr(eown))
    if rc != 0:
        msg = lib.fdtd_last_error(None)
        raise FdtdError(f"fdtd_voxelize failed ({rc}): {msg.decode() if msg else ''}")
    return cown, eown


def voxelize_maps_raw(lib: C.CDLL, grid, table, device: int = 0, cown=None, eown=None, force: bool = False):
    """fdtd_voxelize_maps on a primitives.Table: (cell_owner, edge_owner, cell_voxel) into the given arrays (None: that pass is not
    run; cell_voxel is None without cell_owner).  `force`: call the entry point for a table without maps too (nmaps = 0)."""
    if not has_discmaterial(lib):
        raise FdtdError("this library has no device lookup of voxel maps (fdtd_voxelize_maps)")
    nx, ny, nz = grid.shape
    maps = list(getattr(table, "maps", None) or [])
    if not maps and not force:
        raise ValueError("the table has no voxel maps (fdtd_voxelize takes it)")
    if len(maps) > VOXEL_MAX_MAPS:
        raise ValueError(f"{len(maps)} voxel maps: at most {VOXEL_MAX_MAPS}")
    lines = _arr(np.concatenate(grid.lines), np.float64)
    rec = np.ascontiguousarray(table.rec)
    verts = _arr(table.verts, np.float64)
    if rec.dtype.itemsize != 248:
        raise ValueError("the table's records must be primitives.RECORD")
    rec_map = _arr(table.rec_map if maps else np.zeros(rec.size, np.int32), np.int32)
    if rec_map.shape != (rec.size,):
        raise ValueError("the table's rec_map must hold one int32 per record")
    keep = []                                        # the arrays the structs point into
    cmaps = (FdtdVoxelMap * max(len(maps), 1))()
    for q, mp in enumerate(maps):
        M, data = _arr(mp.M, np.float64).reshape(-1), _arr(mp.data, np.uint8).reshape(-1)
        ml = [_arr(l, np.float64).reshape(-1) for l in mp.lines]
        if M.size != 12 or len(ml) != 3:
            raise ValueError("a voxel map needs M[12] and three line arrays")
        keep += [M, data] + ml
        cmaps[q].m[:] = M.tolist()
        for a in range(3):
            cmaps[q].lines[a] = ml[a].ctypes.data
            cmaps[q].n[a] = ml[a].size
        cmaps[q].data, cmaps[q].ndata, cmaps[q].use_db_background = data.ctypes.data, data.size, int(bool(mp.use_db_background))
    cvox = np.empty((nz - 1, ny - 1, nx - 1), np.int32) if cown is not None else None
    rc = lib.fdtd_voxelize_maps(int(device), nx, ny, nz, _ptr(lines), int(rec.size), _ptr(rec) if rec.size else None, int(verts.size),
                                _ptr(verts) if verts.size else None, float(table.tol), _ptr(cown), _ptr(eown),
                                _ptr(rec_map) if rec.size else None, len(maps), C.cast(cmaps, C.c_void_p) if maps else None, _ptr(cvox))
    del keep
    if rc != 0:
        msg = lib.fdtd_last_error(None)
        raise FdtdError(f"fdtd_voxelize_maps failed ({rc}): {msg.decode() if msg else ''}")
    return cown, eown, cvox


def voxelize_device(lib: C.CDLL, device: int = 0):
    """A `rasteriser` for scene.voxelize(scene, grid, rasteriser): primitives.rasterise_spec's result, computed by csrc/voxel.hip.  A
    table with voxel maps takes fdtd_voxelize_maps where `lib` exports it, else the specification."""
    def rasteriser(grid, table):
        if getattr(table, "maps", None) and not has_discmaterial(lib):
            from . import primitives as _prims
            return _prims.rasterise_spec(grid, table)
        return voxelize_raw(lib, grid, table, device)
    return rasteriser


def sar_local_raw(lib: C.CDLL, dx, dy, dz, Vx, Vy, Vz, sigma, rho, device: int = 0):
    """fdtd_sar_local: (p, sar_local) float64 [ncz][ncy][ncx] — sar.local_spec's result, bit for bit."""
    if not has_sar(lib):
        raise FdtdError("this library has no device SAR (fdtd_sar_local / fdtd_sar_average)")
    dx, dy, dz = (_arr(a, np.float64).ravel() for a in (dx, dy, dz))
    shape = (dz.size, dy.size, dx.size)
    sigma, rho = _arr(sigma, np.float64), _arr(rho, np.float64)
    V = [_arr(v, np.complex128) for v in (Vx, Vy, Vz)]
    if sigma.shape != shape or rho.shape != shape or any(v.shape != tuple(n + 1 for n in shape) for v in V):
        raise ValueError("SAR: per-cell arrays must be [ncz][ncy][ncx], edge voltages [ncz+1][ncy+1][ncx+1]")
    p_out, sar_out = np.empty(shape, np.float64), np.empty(shape, np.float64)
    rc = lib.fdtd_sar_local(int(device), dx.size, dy.size, dz.size, _ptr(dx), _ptr(dy), _ptr(dz), _ptr(V[0]), _ptr(V[1]), _ptr(V[2]),
                            _ptr(sigma), _ptr(rho), _ptr(p_out), _ptr(sar_out))
    if rc != 0:
        msg = lib.fdtd_last_error(None)
        raise FdtdError(f"fdtd_sar_local failed ({rc}): {msg.decode() if msg else ''}")
    return p_out, sar_out


def sar_average_raw(lib: C.CDLL, dx, dy, dz, rho, p, mass, method="ieee", device: int = 0):
    """fdtd_sar_average: (sar_avg, half_side float64 [ncz][ncy][ncx], status int8, counts int64 [4]) — sar.average_spec's result."""
    from . import sar as _sar
    if not has_sar(lib):
        raise FdtdError("this library has no device SAR (fdtd_sar_local / fdtd_sar_average)")
    if method not in _sar.METHODS:
        raise ValueError(f"SAR: averaging method must be one of {sorted(_sar.METHODS)}, got {method!r}")
    dx, dy, dz = (_arr(a, np.float64).ravel() for a in (dx, dy, dz))
    shape = (dz.size, dy.size, dx.size)
    rho, p = _arr(rho, np.float64), _arr(p, np.float64)
    if rho.shape != shape or p.shape != shape:
        raise ValueError("SAR: per-cell arrays must be [ncz][ncy][ncx]")
    sar_avg, half = np.empty(shape, np.float64), np.empty(shape, np.float64)
    status, counts = np.empty(shape, np.int8), np.zeros(4, np.int64)
    rc = lib.fdtd_sar_average(int(device), dx.size, dy.size, dz.size, _ptr(dx), _ptr(dy), _ptr(dz), _ptr(rho), _ptr(p), float(mass),
                              int(_sar.METHODS[method]), _ptr(sar_avg), _ptr(half), _ptr(status), _ptr(counts))
    if rc != 0:
        msg = lib.fdtd_last_error(None)
        raise FdtdError(f"fdtd_sar_average failed ({rc}): {msg.decode() if msg else ''}")
    return sar_avg, half, status, counts


def sar_device(lib: C.CDLL, device: int = 0):
    """What Simulation.sar hands to sar.evaluate: the pair (local, average) of csrc/sar.hip when `lib` exports the SAR entry points
    and FDTD_SAR is not "host", else None (the numpy specification, sar.local_spec / sar.average_spec)."""
    if os.environ.get("FDTD_SAR", "").lower() == "host" or not has_sar(lib):
        return None
    return (lambda *a: sar_local_raw(lib, *a, device=device)), (lambda *a: sar_average_raw(lib, *a, device=device))


def field_interp_raw(lib: C.CDLL, kind, mode, lines, lo, hi, V=None, I=None, kappa=None, sub=(1, 1, 1), device: int = 0):
    """fdtd_field_interp: field [3][nz][ny][nx], complex128 or float64 — fields.interp_spec's result, bit for bit (same arguments)."""
    from . import fields as _fields
    if not has_fields(lib):
        raise FdtdError("this library has no device field dumps (fdtd_field_interp)")
    lines, lo, hi, sub = _fields.check_args(kind, mode, lines, lo, hi, sub)
    rlo, _ = _fields.region(lo, hi)
    rshape = tuple(hi[a] - rlo[a] + 1 for a in (2, 1, 0))
    src = I if _fields.NEEDS_I[kind] else V
    if src is None or len(src) != 3:
        raise ValueError(f"field dump: kind {kind} needs the three recorded {'face currents I' if _fields.NEEDS_I[kind] else 'edge voltages V'}")
    src = [np.ascontiguousarray(a) for a in src]
    cplx = [np.iscomplexobj(a) for a in src]
    if any(cplx) != all(cplx):
        raise ValueError("field dump: the three recorded arrays must be all real or all complex")
    src = [_arr(a, np.complex128 if cplx[0] else np.float64) for a in src]
    kap = [None] * 3
    if kind == "J":
        if kappa is None or len(kappa) != 3:
            raise ValueError("field dump: kind J needs the three edge conductivities")
        kap = [_arr(k, np.float64) for k in kappa]
    if any(a.shape != rshape for a in src) or any(k is not None and k.shape != rshape for k in kap):
        raise ValueError(f"field dump: the recorded arrays and conductivities must cover the region [nz][ny][nx] = {rshape}")
    nx, ny, nz = _fields.out_counts(mode, lo, hi, sub)
    out = np.empty((3, nz, ny, nx), np.complex128 if cplx[0] else np.float64)
    i32 = lambda v: _arr(v, np.int32)
    n_a, lo_a, hi_a, sub_a = i32([l.size for l in lines]), i32(lo), i32(hi), i32(sub)
    rc = lib.fdtd_field_interp(int(device), int(_fields.KINDS[kind]), int(mode), 2 if cplx[0] else 1, _ptr(n_a), _ptr(lo_a), _ptr(hi_a),
                               _ptr(sub_a), _ptr(lines[0]), _ptr(lines[1]), _ptr(lines[2]), _ptr(src[0]), _ptr(src[1]), _ptr(src[2]),
                               _ptr(kap[0]), _ptr(kap[1]), _ptr(kap[2]), _ptr(out))
    if rc != 0:
        msg = lib.fdtd_last_error(None)
        raise FdtdError(f"fdtd_field_interp failed ({rc}): {msg.decode() if msg else ''}")
    return out


def fields_device(lib: C.CDLL, device: int = 0):
    """What Simulation.field hands to fields.evaluate: fdtd_field_interp of csrc/fields.hip when `lib` exports it and FDTD_FIELDS is
    not "host", else None (the numpy specification, fields.interp_spec)."""
    if os.environ.get("FDTD_FIELDS", "").lower() == "host" or not has_fields(lib):
        return None
    return lambda *a: field_interp_raw(lib, *a, device=device)


def default_rasteriser(lib: C.CDLL, device: int = 0):
    """What openEMS.Run hands to scene.voxelize (the package's one caller of voxelize; the plugin's scenes reach it through Run): the
    device rasteriser when `lib` exports fdtd_voxelize and FDTD_VOXELIZE is not "host", else None (the numpy specification).  No
    size threshold: the whole device call was 2.7 to 4.6 times faster than the specification on every grid timed, from 50 x 50 x 7 to
    800 x 800 x 120 nodes, and 49 times on a 1000-segment wire (profiles/primitives/timing.txt)."""
    if os.environ.get("FDTD_VOXELIZE", "").lower() == "host" or not has_voxelize(lib):
        return None
    return voxelize_device(lib, device)


def fractions_raw(lib: C.CDLL, grid, table, device: int = 0):
    """fdtd_voxel_fractions on a primitives.Table of plain metal records (conformal.plain_metal_table):
    (node_in bool [nz][ny][nx], comp int8 [ncut], idx int64 [ncut], f float64 [ncut]) — conformal.fractions_spec's result."""
    from . import conformal as _conformal
    if not has_conformal(lib):
        raise FdtdError("this library has no device fractions (fdtd_voxel_fractions)")
    nx, ny, nz = grid.shape
    lines = _arr(np.concatenate(grid.lines), np.float64)
    rec = np.ascontiguousarray(table.rec)
    verts = _arr(table.verts, np.float64)
    if rec.dtype.itemsize != 248:
        raise ValueError("the table's records must be primitives.RECORD")
    snap = _conformal.snap_distance(table)

    def call(node, ncut, code, idx, f):
        rc = lib.fdtd_voxel_fractions(int(device), nx, ny, nz, _ptr(lines), int(rec.size), _ptr(rec) if rec.size else None, int(verts.size),
                                      _ptr(verts) if verts.size else None, float(table.tol), float(snap), int(_conformal.N_BISECT),
                                      _ptr(node), int(ncut), _ptr(code), _ptr(idx), _ptr(f))
        if rc != 0:
            msg = lib.fdtd_last_error(None)
            raise FdtdError(f"fdtd_voxel_fractions failed ({rc}): {msg.decode() if msg else ''}")
    node = np.zeros((nz, ny, nx), np.uint8)
    call(node, 0, None, None, None)
    node_in = node.astype(bool)
    comp, idx, flip = _conformal.cut_edges(node_in)
    f = np.ones(idx.size, np.float64)
    if idx.size:
        code = _arr(comp.astype(np.uint8) | (flip.astype(np.uint8) << 2), np.uint8)
        call(None, idx.size, code, _arr(idx, np.int64), f)
    return node_in, comp, idx, f


def default_fractions(lib: C.CDLL, device: int = 0):
    """What openEMS.Run hands to conformal.fractions: the device call when `lib` exports fdtd_voxel_fractions and FDTD_VOXELIZE is
    not "host", else None (the numpy specification).  Timed once, on the 300 x 300 x 60 circular patch: 3.7 ms against numpy's 8.7 ms for the
    whole call (profiles/conformal/timing.txt)."""
    if os.environ.get("FDTD_VOXELIZE", "").lower() == "host" or not has_conformal(lib):
        return None
    return lambda grid, table: fractions_raw(lib, grid, table, device)


def subcell_raw(lib: C.CDLL, grid, table, nsub, prop_eps, prop_kap, prop_plain, skip, device: int = 0):
    """fdtd_voxel_subcell on a primitives.Table: subcell.edges_spec's result (a subcell.Listed), bit for bit."""
    from . import subcell as _subcell
    if not has_subcell(lib):
        raise FdtdError("this library has no device sub-cell sampling (fdtd_voxel_subcell)")
    nsub = _subcell.check_nsub(nsub)
    nx, ny, nz = grid.shape
    lines = _arr(np.concatenate(grid.lines), np.float64)
    rec = np.ascontiguousarray(table.rec)
    verts = _arr(table.verts, np.float64)
    if rec.dtype.itemsize != 248:
        raise ValueError("the table's records must be primitives.RECORD")
    peps, pkap, plain = _arr(prop_eps, np.float64).reshape(-1, 3), _arr(prop_kap, np.float64).reshape(-1, 3), _arr(prop_plain, np.uint8).reshape(-1)
    if peps.shape != pkap.shape or peps.shape[0] != plain.size or plain.size < 1:
        raise ValueError("subcell: the property tables need one row per material and the background's")
    skip = _arr(skip, np.uint8)
    if skip.shape != (3, nz, ny, nx):
        raise ValueError("subcell: skip must be [3][nz][ny][nx]")
    rec_map = None if getattr(table, "rec_map", None) is None else _arr(table.rec_map, np.int32)
    cap = max(1 << 16, (3 * nx * ny * nz) // 16)
    while True:
        comp, idx = np.empty(cap, np.int8), np.empty(cap, np.int64)
        eps, kap = np.empty(cap, np.float64), np.empty(cap, np.float64)
        n, dropped = C.c_int64(0), np.zeros(2, np.int64)
        rc = lib.fdtd_voxel_subcell(int(device), nx, ny, nz, _ptr(lines), int(rec.size), _ptr(rec) if rec.size else None, int(verts.size),
                                    _ptr(verts) if verts.size else None, float(table.tol), _ptr(rec_map), nsub, int(plain.size - 1), _ptr(peps),
                                    _ptr(pkap), _ptr(plain), _ptr(skip), int(cap), _ptr(comp), _ptr(idx), _ptr(eps), _ptr(kap),
                                    C.byref(n), _ptr(dropped))
        if rc != 0:
            msg = lib.fdtd_last_error(None)
            raise FdtdError(f"fdtd_voxel_subcell failed ({rc}): {msg.decode() if msg else ''}")
        if n.value <= cap:
            break
        cap = int(n.value)           # the list did not fit: once more with room for it
    k = int(n.value)
    return _subcell.Listed(comp[:k].copy(), idx[:k].copy(), eps[:k].copy(), kap[:k].copy(), nsub, int(dropped[0]), int(dropped[1]))


def default_subcell(lib: C.CDLL, device: int = 0):
    """What openEMS.Run hands to scene.voxelize(subcell=..., device_subcell=): the device call when `lib` exports fdtd_voxel_subcell
    and FDTD_SUBCELL is not "host", else None (the numpy specification, subcell.edges_spec)."""
    if os.environ.get("FDTD_SUBCELL", "").lower() == "host" or not has_subcell(lib):
        return None
    return lambda grid, table, nsub, peps, pkap, plain, skip: subcell_raw(lib, grid, table, nsub, peps, pkap, plain, skip, device)
