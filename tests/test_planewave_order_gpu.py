"""Where k_planewave sits in the timestep (include/fdtd_hip_planewave.h), against everything that samples or rewrites its elements:
V-probes and a V-DFT box on listed edges read the voltage in front of the E list, I-probes and an I-DFT box on listed faces read the
current behind the H list, and entries on and next to the node planes of Mur faces go through the Mur passes as the header orders —
under fdtd_run, whatever schedule the planner picks, as under fdtd_half_step and in the restatement on the oracle.  The scene layer
keeps the lists off all of these; fdtd_planewave_set takes any existing edge or face.  Cases and reference: planewave_order_cases.py
(test_planewave_order_cpu.py holds them to telling the two sides of each list apart)."""
import numpy as np
import pytest

from conftest import pkg
from helpers import seeded_fields
import planewave_order_cases as cases


def _order_contexts(hip_lib, o, kind):
    """Two HIP contexts of the order scene with the tables, the three one-cell probes and the DFT box of `kind`, from the seeded
    fields: (engine, probe ids, box id) for fdtd_run and for the half-steps."""
    out = []
    for _ in range(2):
        e = cases.order_sim().build(hip_lib)
        e.set_planewave(*o.tables.args())
        pids = [e.add_probe(kind, *a) for a in o.probe_args(kind)]
        e.set_dft(cases.EVERY, o.tw[0], o.tw[1])
        c, lo, hi = o.box[kind]
        bid = e.add_dft_box(kind, c, lo, hi)
        seeded_fields(e, cases.ORDER_SEED)
        out.append((e, pids, bid))
    return out


def _run_both(contexts):
    capi = pkg("_capi")
    (e_run, _, _), (e_half, _, _) = contexts
    assert e_run.schedule_info()["launches_per_timestep"] == 2, e_run.schedule_info()
    e_run.run(70)
    e_run.run(80)                                   # (the last I-probe sample of a call is flushed at its end)
    for _ in range(cases.ORDER_STEPS):
        e_half.half_step(capi.PHASE_E)
        e_half.half_step(capi.PHASE_H)


def _compare(o, contexts, kind, side):
    """Probe series, fields and box of both contexts against the reference's values on `side` of the list (0: in front, 1: behind)."""
    want, other = o.series[kind][side].astype(np.float64), o.series[kind][1 - side].astype(np.float64)
    acc = o.acc[kind][side]
    scale = np.abs(acc).max()
    # (the other side of the list reads something else: test_planewave_order_cpu holds the reference to that, by more than 1e-3)
    assert all(not np.array_equal(want[:, q], other[:, q]) for q in range(3)) and np.abs(acc - o.acc[kind][1 - side]).max() > 1e-3 * scale
    for (e, pids, bid), how in zip(contexts, ("fdtd_run", "fdtd_half_step")):
        got = np.stack([e.get_probe(p)[:cases.ORDER_STEPS] for p in pids], axis=1)
        assert got.shape == want.shape
        wrong = [q for q in range(3) if not np.array_equal(got[:, q], want[:, q])]
        assert not wrong, (how, [(o.cells[kind][q], "the series of the list's other side" if np.array_equal(got[:, q], other[:, q]) else
                                  f"first differs at step {int(np.argmax(got[:, q] != want[:, q]))}") for q in wrong])
        assert np.array_equal(e.fields(), o.fields), how
        box = e.get_dft_box(bid)[0]
        assert box.shape == acc.shape
        err = np.abs(box - acc).max() / scale
        print(f"{how}: box against the reference's sums: {err:.3g} of the scale")
        assert err <= 1e-12, (how, err)
        e.close()


@pytest.mark.gpu
def test_v_probe_and_v_box_read_the_voltage_before_the_edge_list(hip_lib, oracle_lib):
    """The E list follows the V-probes and the V-DFT boxes.  With fused sources fdtd_run samples the V-probes in update_H's probe
    blocks, behind every correction of the E side, unless the planner knows that a probe cell sits on a corrected edge
    (api.hip probes_first): three one-cell probes of weight 1.0 on listed edges (the sample is the fp32 voltage itself) and a V-DFT box
    over listed and unlisted edges, under fdtd_run in chunks of 70 + 80 and under half-steps, against the oracle's own V-probes of the
    restated run — the oracle samples them inside its E half-step, in front of the restatement's correction."""
    capi = pkg("_capi")
    o = cases.order_reference(oracle_lib)
    assert np.array_equal(o.own[0], o.series[0][0].astype(np.float64))
    contexts = _order_contexts(hip_lib, o, capi.KIND_V)
    _run_both(contexts)
    _compare(o, contexts, capi.KIND_V, 0)


@pytest.mark.gpu
def test_i_probe_and_i_box_read_the_current_behind_the_face_list(hip_lib, oracle_lib):
    """The H list runs before anything samples I: with fused sources the I-probes of a timestep are sampled by the next update_E's
    probe blocks or by the flush at the end of a call, both behind the list — three one-cell I-probes on listed faces and an I-DFT box
    over listed and unlisted faces, against the currents the restatement holds after each timestep.  (The oracle's own I-probes sample
    inside its H half-step, in front of the restatement's correction: they are the series a wrong order would give.)"""
    capi = pkg("_capi")
    o = cases.order_reference(oracle_lib)
    assert np.array_equal(o.own[1], o.series[1][0].astype(np.float64))
    contexts = _order_contexts(hip_lib, o, capi.KIND_I)
    _run_both(contexts)
    _compare(o, contexts, capi.KIND_I, 1)


@pytest.mark.gpu
def test_plane_wave_elements_on_and_next_to_mur_faces(hip_lib, oracle_lib, monkeypatch):
    """Edges on the node plane of a Mur face (the operator holds vi = 0 there; a hand-made coefficient is no multiple of vi, so the
    addition is live), edges on the plane next to it (the Mur post and pre passes read them) and faces touching both.  Without an
    apply pass the face voltages in memory between update_E and update_H are the E update's own and update_H overwrites them with the
    candidates, so an edge of the E list on such a plane takes the apply pass as a launch of its own, as a sheet edge does
    (test_sheet_gpu.test_sheet_edges_on_a_mur_face_node_plane); lists that leave the face planes alone keep the planner's own choice."""
    capi = pkg("_capi")
    refs = {w: cases.mur_reference(oracle_lib, w) for w in ("full", "off-face")}
    assert not np.array_equal(refs["full"], refs["off-face"])
    full, middle, off = (cases.mur_tables(w) for w in ("full", "middle", "off-face"))
    for apply_pass in (None, "1"):
        if apply_pass is None:
            monkeypatch.delenv("FDTD_MUR_APPLY_PASS", raising=False)
        else:
            monkeypatch.setenv("FDTD_MUR_APPLY_PASS", apply_pass)
        alone = 2 if apply_pass is None else 3
        e, eh = cases.mur_sim().build(hip_lib), cases.mur_sim().build(hip_lib)
        e.set_planewave(*middle.args())                 # the middle entries alone: the environment decides
        assert e.schedule_info()["launches_per_timestep"] == alone, e.schedule_info()
        for x in (e, eh):
            x.set_planewave(*full.args())
            seeded_fields(x, cases.MUR_SEED)
        info = e.schedule_info()
        assert info["launches_per_timestep"] == 3 and not info["resident"], info
        e.run(cases.MUR_STEPS)
        for _ in range(cases.MUR_STEPS):
            eh.half_step(capi.PHASE_E)
            eh.half_step(capi.PHASE_H)
        got, half = e.fields(), eh.fields()
        differ = lambda a, b: f"{np.count_nonzero(a != b)} entries differ, first (kind, component, k, j, i) = {tuple(np.argwhere(a != b)[0])}" if np.any(a != b) else ""
        assert np.array_equal(got, refs["full"]), "fdtd_run against the restatement: " + differ(got, refs["full"])
        assert np.array_equal(got, half), "fdtd_run against the half-steps: " + differ(got, half)
        e.close()
        eh.close()
        # the edges next to the faces without those on them: nothing of the E list lies on a face plane, the schedule stays
        e = cases.mur_sim().build(hip_lib)
        e.set_planewave(*off.args())
        assert e.schedule_info()["launches_per_timestep"] == alone, e.schedule_info()
        seeded_fields(e, cases.MUR_SEED)
        e.run(cases.MUR_STEPS)
        got = e.fields()
        assert np.array_equal(got, refs["off-face"]), "the off-face lists against the restatement: " + differ(got, refs["off-face"])
        e.close()
