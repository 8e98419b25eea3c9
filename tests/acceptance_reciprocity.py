"""Reciprocity KAT of the plane-wave excitation (a script: pytest does not collect it; its report goes to profiles/planewave/kat.txt).

The openEMS "Simple Patch Antenna" tutorial (the scene of tests/tutorial_scene.py, the same public API calls; the air below the ground
plane extended from 50 to 100 mm, for the tutorial's own two cells between ground and PML leave no room for the box) is run once in transmit
mode — port excited, far field at the S11 dip — and then in receive mode: the port terminated in its 50 ohm and not excited, a plane
wave arriving from a direction (theta, phi) with theta^ or phi^ polarisation.  By reciprocity the received port voltage over direction
and polarisation follows the transmit far field,

    |U_port(f_res)| / |s^_inc(f_res)|  ~  |E_theta(theta, phi)|  resp.  |E_phi(theta, phi)|,

both normalised at broadside, co-polar.  This compares the port chain (probes, CalcPort) with the NF2FF chain (recording faces,
far-field transform) by a path that shares nothing with the power balance.  Five directions: broadside and theta = 30, 60 degrees in the
E plane (phi = 0, the patch resonates along x) and in the H plane (phi = 90); two polarisations each.

One run per process, so that every GPU run has its own time limit:

    python tests/acceptance_reciprocity.py transmit OUT            # writes OUT/transmit.json
    python tests/acceptance_reciprocity.py receive K OUT           # K = 0 .. 9, writes OUT/receive_K.json
    python tests/acceptance_reciprocity.py report OUT [TAG]        # the table; with FDTD_WRITE_KAT into profiles/planewave/kat.txt

e.g.  timeout 300 python ... transmit OUT && timeout 300 python ... receive 0 OUT && ... && python ... report OUT MI355X
FDTD_RECIPROCITY_LIB=oracle steps the receive runs with the numpy restatement on the CPU oracle instead (slow)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT, pkg       # noqa: E402

DIRECTIONS = [(0.0, 0.0), (30.0, 0.0), (60.0, 0.0), (30.0, 90.0), (60.0, 90.0)]          # (theta, phi) in degrees
CASES = [(d, pol) for d in DIRECTIONS for pol in ("theta", "phi")]
NR_TS, END = 60000, 1e-5


def unit_vectors(theta_deg, phi_deg):
    t, p = np.deg2rad(theta_deg), np.deg2rad(phi_deg)
    r = np.array([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)])
    th = np.array([np.cos(t) * np.cos(p), np.cos(t) * np.sin(p), -np.sin(t)])
    ph = np.array([-np.sin(p), np.cos(p), 0.0])
    return r, th, ph


def scene(lib, excite, wave=None):
    """The tutorial's calls; `wave` = (e0, direction) adds the plane wave on a box around the antenna."""
    oa = pkg("openems_api")
    C0, EPS0 = oa.physical_constants.C0, oa.physical_constants.EPS0
    patch_w, patch_l, eps_r, h, sub = 32.0, 40.0, 3.38, 1.524, 60.0
    feed_x, feed_R = -6.0, 50.0
    box = np.array([200.0, 200.0, 150.0])
    f0, fc = 2e9, 1e9
    fdtd = oa.openEMS(NrTS=NR_TS, EndCriteria=END, lib=lib)
    fdtd.SetGaussExcite(f0, fc)
    fdtd.SetBoundaryCond([3] * 6)
    csx = oa.ContinuousStructure()
    fdtd.SetCSX(csx)
    mesh = csx.GetGrid()
    mesh.SetDeltaUnit(1e-3)
    res = C0 / (f0 + fc) / 1e-3 / 20.0
    mesh.AddLine("x", [-box[0] / 2, box[0] / 2])
    mesh.AddLine("y", [-box[1] / 2, box[1] / 2])
    mesh.AddLine("z", [-box[2] * 2 / 3, box[2] * 2 / 3])             # (the tutorial's -50 mm leaves two cells between ground and PML: no room for the box)
    patch = csx.AddMetal("patch")
    patch.AddBox(priority=10, start=[-patch_w / 2, -patch_l / 2, h], stop=[patch_w / 2, patch_l / 2, h])
    fdtd.AddEdges2Grid(dirs="xy", properties=patch, metal_edge_res=res / 2)
    substrate = csx.AddMaterial("substrate", epsilon=eps_r, kappa=2 * np.pi * f0 * EPS0 * eps_r * 1e-3)
    substrate.AddBox(priority=0, start=[-sub / 2, -sub / 2, 0.0], stop=[sub / 2, sub / 2, h])
    mesh.AddLine("z", np.linspace(0.0, h, 5).tolist())
    gnd = csx.AddMetal("gnd")
    gnd.AddBox([-sub / 2, -sub / 2, 0.0], [sub / 2, sub / 2, 0.0], priority=10)
    fdtd.AddEdges2Grid(dirs="xy", properties=gnd)
    mesh.AddLine("x", [feed_x])
    mesh.AddLine("z", [0.0, h])
    port = fdtd.AddLumpedPort(1, feed_R, [feed_x, 0.0, 0.0], [feed_x, 0.0, h], "z", excite, priority=5, edges2grid="xy")
    mesh.SmoothMeshLines("all", res, 1.4)
    nf2ff = None
    if wave is None:
        nf2ff = fdtd.CreateNF2FFBox()
    else:
        exc = csx.AddExcitation("plane_wave", 10, list(wave[0]))
        exc.SetPropagationDir(list(wave[1]))
        exc.AddBox([-45.0, -45.0, -20.0], [45.0, 45.0, 25.0])        # 15 mm around the substrate: several cells of air on every side
    return fdtd, port, nf2ff


def load_lib():
    capi = pkg("_capi")
    if os.environ.get("FDTD_RECIPROCITY_LIB") == "oracle":
        import ctypes
        return capi.bind(ctypes.CDLL(os.path.join(ROOT, "oracle", "libfdtd_oracle.so"))), "oracle restatement"
    import torch  # noqa: F401
    return capi.load_hip_library(), "MI355X"


def transmit(out):
    lib, where = load_lib()
    fdtd, port, nf2ff = scene(lib, 1.0)
    fdtd.Run(os.path.join(out, "tx"), verbose=0, cleanup=True)
    f = np.linspace(1e9, 3e9, 401)
    port.CalcPort(out, f)
    s11 = 20 * np.log10(np.abs(port.uf_ref / port.uf_inc))
    k = int(np.argmin(s11))
    rows = []
    for th, ph in DIRECTIONS:
        ff = nf2ff.CalcNF2FF(out, f[k], [th], [ph], center=[0.0, 0.0, 1e-3])
        rows.append([abs(complex(ff.E_theta[0][0, 0])), abs(complex(ff.E_phi[0][0, 0]))])
    json.dump({"where": where, "f_res": float(f[k]), "dip_dB": float(s11[k]), "steps": int(fdtd.stats.steps), "E": rows,
               "grid": list(fdtd.sim.grid.shape)}, open(os.path.join(out, "transmit.json"), "w"))
    print(f"transmit: f_res = {f[k] / 1e9:.4f} GHz, dip {s11[k]:.1f} dB, {fdtd.stats.steps} timesteps, grid {fdtd.sim.grid.shape}")


def receive(case, out):
    lib, where = load_lib()
    (th, ph), pol = CASES[case]
    r, tv, pv = unit_vectors(th, ph)
    if where != "MI355X":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from restatement import install

        class _MP:          # the one call install makes
            @staticmethod
            def setattr(obj, name, value):
                setattr(obj, name, value)
        install(_MP)
    fdtd, port, _ = scene(lib, 0.0, wave=(tv if pol == "theta" else pv, -r))
    fdtd.Run(os.path.join(out, f"rx{case}"), verbose=0, cleanup=True)
    f_res = json.load(open(os.path.join(out, "transmit.json")))["f_res"]
    port.CalcPort(out, [f_res])
    s_inc = fdtd.sim.incident_spectrum([f_res])[0]
    u = abs(complex(port.uf_tot[0])) / abs(s_inc)
    json.dump({"where": where, "theta": th, "phi": ph, "pol": pol, "u_over_s": float(u), "steps": int(fdtd.stats.steps),
               "entries": [fdtd.stats.planewave["edges"], fdtd.stats.planewave["faces"]],
               "launches": fdtd.stats.schedule["launches_per_timestep"]}, open(os.path.join(out, f"receive_{case}.json"), "w"))
    print(f"receive {case}: theta {th}, phi {ph}, {pol}^: |U| / |s^| = {u:.6e}, {fdtd.stats.steps} timesteps")


def report(out, tag=None):
    tx = json.load(open(os.path.join(out, "transmit.json")))
    rx = [json.load(open(os.path.join(out, f"receive_{k}.json"))) for k in range(len(CASES))]
    where = tag or rx[0]["where"]
    e0, u0 = tx["E"][0][0], rx[0]["u_over_s"]                      # broadside, theta^ (= x^: co-polar)
    lines = [f"tutorial patch, port terminated in 50 ohm; transmit run {tx['steps']} timesteps on grid {tx['grid']}, f_res = {tx['f_res'] / 1e9:.4f} GHz "
             f"(S11 dip {tx['dip_dB']:.1f} dB); plane-wave lists {rx[0]['entries'][0]} edges / {rx[0]['entries'][1]} faces, "
             f"{rx[0]['launches']} launches per timestep; all runs: {where}",
             "theta  phi  pol    transmit |E| / broadside [dB]   receive |U|/|s^| / broadside [dB]   deviation [dB]"]
    worst, worst_main = 0.0, 0.0
    for k, ((th, ph), pol) in enumerate(CASES):
        et = tx["E"][DIRECTIONS.index((th, ph))][0 if pol == "theta" else 1]
        a, b = 20 * np.log10(max(et, 1e-30) / e0), 20 * np.log10(max(rx[k]["u_over_s"], 1e-30) / u0)
        if max(a, b) < -60.0:            # a null of both (a symmetry plane of the scene): no deviation to speak of
            lines.append(f"{th:5.0f} {ph:4.0f}  {pol:5s}  {'< -60':>10s}                      {'< -60':>10s}                         {'-':>8s}")
            continue
        lines.append(f"{th:5.0f} {ph:4.0f}  {pol:5s}  {a:10.2f}                      {b:10.2f}                         {b - a:+8.2f}")
        worst = max(worst, abs(b - a))
        if a > -20.0:
            worst_main = max(worst_main, abs(b - a))
    lines.append(f"largest deviation: {worst_main:.2f} dB over the components within 20 dB of broadside, {worst:.2f} dB over all components above "
                 f"-60 dB (cross-polar ones included)")
    print("\n".join(lines))
    if os.environ.get("FDTD_WRITE_KAT"):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from test_planewave_model_cpu import _note
        _note(f"reciprocity, tutorial patch ({where})", lines)


if __name__ == "__main__":
    mode, args = sys.argv[1], sys.argv[2:]
    if mode == "transmit":
        os.makedirs(args[0], exist_ok=True)
        transmit(args[0])
    elif mode == "receive":
        receive(int(args[0]), args[1])
    elif mode == "report":
        report(*args)
    else:
        raise SystemExit(__doc__)
