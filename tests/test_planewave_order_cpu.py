"""The cases of planewave_order_cases.py, on the oracle alone: the lists are what their docstrings say, and the reference can tell a
kernel that keeps the header's launch order (include/fdtd_hip_planewave.h) from one that does not — every probed element and every
box changes across its list, and the entries on the Mur faces' node planes change the fields.  test_planewave_order_gpu.py compares
the HIP library with the same reference.  The bars are conditions on the drawn tables (1e-3 of the scale, what test_lorentz_gpu asks
of its own order test), not measurements: a table that misses one is to be drawn again."""
import numpy as np

import planewave_order_cases as cases


def _peak_rel(a, b):
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))) / float(np.max(np.abs(a)))


def test_order_scene_lists_and_probes():
    o = cases.Order()
    (i0, j0, k0), (i1, j1, k1) = cases.ORDER_BLOCK
    for kind, l in enumerate((o.tables.E, o.tables.H)):
        el = cases.elements(l)
        assert len(el) == len(set(el)) == 40 and {e[0] for e in el} == {0, 1, 2}
        assert all(i0 <= i <= i1 and j0 <= j <= j1 and k0 <= k <= k1 and not cases.near_port(i, j, k) for _, i, j, k in el)
        idx, comp, coef, m0, w = l
        assert coef.dtype == np.float32 and 1e-4 < np.abs(coef[:, 0]).mean() < 1e-2 and np.all(coef[::4, 1] == 0) and np.any(coef[1::4, 1] != 0)
        assert m0.min() >= 0 and m0.max() <= 40 and np.all(w >= 0) and np.all(w < 1)
        # one probe cell per component, each a listed element; the box holds listed and unlisted elements of its component
        assert [c for c, _, _, _ in o.cells[kind]] == [0, 1, 2] and all(cell in el for cell in o.cells[kind])
        assert o.listed[kind].any() and not o.listed[kind].all() and o.box[kind][0] == 1
        for idx_p, comp_p, w_p in o.probe_args(kind):
            assert idx_p.size == 1 and w_p[0] == 1.0
    assert o.tables.sig2.size == cases.NSIG2 and 2 * cases.ORDER_STEPS > cases.NSIG2 + 40        # late steps read past the pulse's end


def test_order_reference_tells_before_from_behind(oracle_lib):
    o = cases.order_reference(oracle_lib)
    assert np.abs(o.fields).max() > 0 and np.all(np.isfinite(o.fields))
    for kind, what in ((0, "voltage"), (1, "current")):
        before, after = o.series[kind]
        # the oracle samples its own probes inside the half-step, i.e. in front of the list, and to the bit (one cell of weight 1.0)
        assert np.array_equal(o.own[kind], before.astype(np.float64))
        for q in range(3):
            d = _peak_rel(after[:, q], before[:, q])
            print(f"{what} of probe cell {o.cells[kind][q]}: peak |behind - in front| / peak = {d:.3g}")
            assert d > 1e-3, (kind, q, d)
        a0, a1 = o.acc[kind]
        scale = np.abs(a0).max()
        d = np.abs(a1 - a0).max() / scale
        print(f"{what} box {o.box[kind]}: |behind - in front| / scale = {d:.3g}")
        assert d > 1e-3, (kind, d)
        # ... through the listed elements alone: what the list leaves alone is the same in front of it and behind it
        assert np.all((a1 != a0)[:, o.listed[kind]]) and not np.any((a1 != a0)[:, ~o.listed[kind]])


def test_mur_scene_lists():
    E, H = cases.mur_elements()
    full, middle, off = (cases.mur_tables(w) for w in ("full", "middle", "off-face"))
    assert cases.elements(full.E) == E and cases.elements(full.H) == H and len(set(E)) == len(E) and len(set(H)) == len(H)
    assert not any(cases.near_port(*e[1:]) for e in E + H)
    n = cases.N
    face_E = cases.on_face_plane(E)
    for a in range(3):
        for side, (plane, nxt) in enumerate(((0, 1), (n[a] - 1, n[a] - 2))):
            # tangential edges of both components on the face's node plane, and on the plane next to it clear of every face plane
            for c in range(3):
                if c == a:
                    continue
                assert sum(1 for e in E if e[0] == c and e[1 + a] == plane) >= 4, (a, side, c)
                assert sum(1 for e, f in zip(E, face_E) if e[0] == c and e[1 + a] == nxt and not f) >= 4, (a, side, c)
            # faces of the normal component in both planes, faces of the others touching them
            for c in range(3):
                for p in (plane, nxt):
                    at = p if (c == a or p <= 1) else p - 1
                    assert sum(1 for e in H if e[0] == c and e[1 + a] == at) >= 4, (a, side, c, p)
    assert sum(1 for e in E if sum(p == 0 or p == m - 1 for p, m in zip(e[1:], n)) >= 2) >= 3        # edges on the grid's own edges
    # every edge exists (one cell along its own axis), every face too (one cell along both transverse axes)
    assert all(e[1 + e[0]] < n[e[0]] - 1 for e in E)
    assert all(e[1 + q] < n[q] - 1 for e in H for q in range(3) if q != e[0])
    mE, mH = cases.elements(middle.E), cases.elements(middle.H)
    assert len(mE) >= 5 and len(mH) >= 5 and {e[0] for e in mE} == {e[0] for e in mH} == {0, 1, 2}
    assert not cases.on_face_plane(mE).any() and all(1 < p < m - 2 for e in mE + mH for p, m in zip(e[1:], n))
    oE = cases.elements(off.E)
    assert oE == [e for e, f in zip(E, face_E) if not f] and 0 < len(oE) < len(E) and cases.elements(off.H) == H
    # a kept entry keeps its numbers
    keep = np.nonzero(~face_E)[0]
    assert all(np.array_equal(a[keep], b) for a, b in zip(full.E, off.E))


def test_mur_reference_feels_the_face_plane_entries(oracle_lib):
    full, off, middle = (cases.mur_reference(oracle_lib, w) for w in ("full", "off-face", "middle"))
    assert np.all(np.isfinite(full)) and np.abs(full).max() > 0
    scale = np.abs(full).max()
    d = np.abs(full.astype(np.float64) - off).max() / scale
    print(f"fields with the face-plane edges against without: {d:.3g} of the peak, {np.count_nonzero(full != off)} entries differ")
    assert not np.array_equal(full, off) and not np.array_equal(off, middle)
