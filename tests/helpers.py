"""Shared builders for the parity tests: the same seeded/synthetic set-up drives the HIP library
and the oracle through one wrapper (fdtd-solver-antennas_amd/_capi.Engine)."""
import numpy as np
from conftest import pkg


def patch_sim(nx, ny, nz, *, boundary="CPML", cpml_cells=8, nr_ts=400, use_classes=True, nf2ff=True,
              f0=2.45e9, nf2ff_freqs=None, nf2ff_mode="dft"):
    wl, sc, sim = pkg("workloads"), pkg("scene"), pkg("simulation")
    w = wl.patch_workload("test", nx=nx, ny=ny, nz=nz, f0=f0)
    vox = sc.voxelize(w.scene, w.grid)
    return sim.Simulation(w.grid, vox, f0=w.f0, fc=w.fc, boundary=boundary, cpml_cells=cpml_cells,
                          nr_ts=nr_ts, nf2ff_freqs=(nf2ff_freqs if nf2ff_freqs is not None else [w.f0]) if nf2ff else None,
                          use_classes=use_classes, nf2ff_mode=nf2ff_mode)


def seeded_fields(engine, seed=0, scale=1e-3):
    """Fill all six components with seeded noise (exercises every stencil term at once)."""
    rng = np.random.default_rng(seed)
    for kind in (0, 1):
        for c in range(3):
            engine.set_field(kind, c, (scale * rng.standard_normal(engine.local_shape)).astype(np.float32))


def rel_l2(a, b):
    a = np.asarray(a); b = np.asarray(b)
    n = np.linalg.norm(b.ravel())
    return float(np.linalg.norm((a - b).ravel()) / (n if n > 0 else 1.0))


# ---- the double-precision build of the oracle (oracle/Makefile: libfdtd_oracle_f64.so) ---------------------------------
# Same algorithm and C ABI as the float32 oracle, with state and coefficients in double: what float32 costs over a whole run.
# The ABI's tables are float32; staged through the oracle-only fdtd_oracle_stage_f64 the double build takes the SAME tables
# in double instead (metric, lumped-edge overrides, CPML coefficients, excitation signal, Mur coefficients).
STAGE_EMET, STAGE_HMET, STAGE_OVER_VV, STAGE_OVER_M, STAGE_CPML, STAGE_SIGNAL, STAGE_MUR = range(7)


def load_oracle_f64():
    import ctypes, os
    from conftest import ROOT
    path = os.path.join(os.environ.get("FDTD_ORACLE_DIR") or os.path.join(ROOT, "oracle"), "libfdtd_oracle_f64.so")
    lib = pkg("_capi").bind(ctypes.CDLL(path))
    lib.fdtd_oracle_real_bytes.restype = ctypes.c_int
    assert lib.fdtd_oracle_real_bytes() == 8
    lib.fdtd_oracle_stage_f64.restype = ctypes.c_int
    lib.fdtd_oracle_stage_f64.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
    return lib


def stage_f64_tables(sim, lib64):
    """Hand the double build the tables of `sim` in double (consumed by the setters of the next sim.build(lib64))."""
    eco, cp, exc = pkg("ecoperator"), pkg("cpml"), pkg("excitation")
    g, v = sim.grid, sim.vox
    k0, nk = sim.slabs(1)[0]
    f64 = np.float64

    def stage(kind, arr):
        a = np.ascontiguousarray(arr, dtype=f64)
        rc = lib64.fdtd_oracle_stage_f64(kind, a.ctypes.data, a.size)
        assert rc == 0, rc

    assert sim.device_operator, "the double tables are staged for fdtd_build_operator"
    emet, hmet = eco.pack_metric_tables(*eco.metric_lists(g, sim.dt, dtype=f64), g, k0, nk, dtype=f64)
    stage(STAGE_EMET, emet); stage(STAGE_HMET, hmet)
    _, _, o_vv, o_m = eco.lumped_overrides(g, v.eps_r, v.kappa, v.pec, sim.dt, v.lumped, dtype=f64)
    stage(STAGE_OVER_VV, o_vv); stage(STAGE_OVER_M, o_m)
    if sim.cpml is not None:
        spec = cp.CPMLSpec(**{**sim.bc.cpml.__dict__, "cells": sim.bc.face_cells()})
        stage(STAGE_CPML, cp.build_cpml(g, sim.dt, spec, dtype=f64).for_slab(k0, nk, dtype=f64)[-1])
    if sim.mur_enable.any():
        stage(STAGE_MUR, sim.mur_coeff_f64)
    stage(STAGE_SIGNAL, exc.gauss_pulse(sim.f0, sim.fc, sim.dt, len(sim.signal), dtype=f64))


def build_f64(sim, lib64, *, double_tables=True):
    """sim.build(lib64) on the double build of the oracle.  double_tables=False: it sees the float32-rounded tables of the C ABI
    (the difference to the float32 run is then the rounding of the time stepping alone); True: the same tables in double."""
    if double_tables:
        stage_f64_tables(sim, lib64)
    return sim.build(lib64)


# ---- the wait-set arithmetic of the one-launch schedule on the host (csrc/wait_sets.hpp behind csrc/wait_sets_shim.cpp) ----------------
class WsGeom(__import__("ctypes").Structure):
    """csrc/wait_sets.hpp: WsGeom"""
    import ctypes as _c
    _fields_ = [("P4", _c.c_int), ("ny", _c.c_int), ("tys", _c.c_int), ("nstrips", _c.c_int), ("nbs", _c.c_int), ("nk", _c.c_int),
                ("fd_mul", _c.c_uint), ("fd_shr", _c.c_uint), ("fd_d", _c.c_uint), ("b", _c.c_int * 6)]


class WsFail(__import__("ctypes").Structure):
    """csrc/wait_sets_model.hpp: WsFail (what: 1 forward flag missing, 2 backward, 3 Mur candidate, 4 plain flag of a block of a Mur grid,
    5 lane budget, 6 flag outside the table, 7 thread decode)"""
    import ctypes as _c
    _fields_ = [("what", _c.c_int), ("k", _c.c_int), ("strip", _c.c_int), ("pb", _c.c_int), ("thread", _c.c_int), ("flag", _c.c_longlong)]

    def __repr__(self):
        return f"what {self.what} at block (k {self.k}, strip {self.strip}, pb {self.pb}) thread {self.thread}, flag {self.flag}"


def load_wait_sets(drop=0):
    """libfdtd_waitsets.so — or the library without clause `drop` (the negative control) —, built on demand by g++ (make waitsets_host)."""
    import ctypes, os, subprocess
    from conftest import ROOT
    csrc = os.path.join(ROOT, "fdtd-solver-antennas_amd", "csrc")
    so = os.path.join(csrc, f"libfdtd_waitsets_drop{drop}.so" if drop else "libfdtd_waitsets.so")
    srcs = [os.path.join(csrc, f) for f in ("wait_sets.hpp", "wait_sets_model.hpp", "wait_sets_shim.cpp", "Makefile")]
    if not os.path.isfile(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["make", "-s", "-B", "-C", csrc, "waitsets_host"] + ([f"DROP={drop}"] if drop else []))
    lib = ctypes.CDLL(so)
    G, I, LL = ctypes.POINTER(WsGeom), ctypes.c_int, ctypes.c_longlong
    IP = ctypes.POINTER(ctypes.c_int)
    for name, res, args in (("ws_drop", I, []), ("ws_geom", None, [G, I, I, I, I, IP]), ("ws_wait_flag", LL, [G, I, I, I, I]),
                            ("ws_wait_back_flag", LL, [G, I, I, I, I]), ("ws_wait_mur_flag", LL, [G, I, I, I]), ("ws_mur_wide", I, [G, I, I, I]),
                            ("ws_decode", I, [G, I, I, I, IP, IP]), ("ws_dump", None, [G, ctypes.c_void_p]),
                            ("ws_check", I, [G, I, I, ctypes.POINTER(WsFail)]), ("ws_check_mur_faces", I, [I, I, I, I, IP, ctypes.POINTER(WsFail)])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    assert lib.ws_drop() == drop
    return lib


def ws_geom(lib, P4, ny, tys, nk, b=None):
    import ctypes
    g = WsGeom()
    lib.ws_geom(ctypes.byref(g), P4, ny, tys, nk, (ctypes.c_int * 6)(*b) if b is not None else None)
    return g
