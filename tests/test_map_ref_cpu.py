"""tests/map_ref.py (the numpy reference of the scan-to-map refine step) against the CPU oracle on every scene of tests/map_cases.py and on two
frames of the synthetic world, and the scenes' own preconditions.  This agreement is what entitles map_ref to judge the kernels in
tests/test_map_refine_edges_gpu.py.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_cases  # noqa: E402
import map_ref  # noqa: E402

SCENES = [s["name"] for s in map_cases.all_scenes()]


def oracle_rows(oracle, cloud, Q):
    """The oracle's kd-tree 5-NN of every query, with laserMapping's refusal (fewer than five, or the fifth squared distance not < 1)."""
    cloud = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
    out = np.full((len(Q), 5), -1, np.int32)
    if len(cloud) == 0:
        return out
    L = oracle.lib()
    L.lo_kdtree_build.restype = C.c_void_p
    L.lo_kdtree_build.argtypes = [C.c_void_p, C.c_int]
    L.lo_kdtree_free.argtypes = [C.c_void_p]
    L.lo_kdtree_knn.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
    t = L.lo_kdtree_build(cloud.ctypes.data, len(cloud))
    idx = np.zeros(5, np.int32); d2 = np.zeros(5, np.float32)
    for i, q in enumerate(Q):
        if L.lo_kdtree_knn(t, float(q[0]), float(q[1]), float(q[2]), 5, idx.ctypes.data, d2.ctypes.data) == 5 and float(d2[4]) < 1.0:
            out[i] = idx
    L.lo_kdtree_free(t)
    return out


def compare_with_oracle(oracle, s):
    r = map_ref.refine(s["cmap"], s["smap"], s["cstack"], s["sstack"], s["x0"])
    xo, st, corr = oracle.map_refine(s["cmap"], s["smap"], s["cstack"], s["sstack"], s["x0"])
    assert r.stats == [st.n_edge[0], st.n_edge[1], st.n_plane[0], st.n_plane[1], st.lm_iters[0], st.lm_iters[1]]
    assert np.abs(r.pose - xo).max() < 1e-9
    # the accepted blocks are the same stack points, and their neighbour rows are the kd-tree's at the pose between the two solves
    acc = np.nonzero(r.nn[:, 0] >= 0)[0]
    stack = np.concatenate([s["cstack"], s["sstack"]])
    assert len(acc) == len(corr)
    if len(acc):
        assert np.array_equal(stack[acc, :3], np.array([[c.cp[0], c.cp[1], c.cp[2]] for c in corr], np.float32))
    if len(s["cmap"]) > 10 and len(s["smap"]) > 50:
        qc, qs = map_ref.associate(r.x_mid, s["cstack"]), map_ref.associate(r.x_mid, s["sstack"])
        rows = np.concatenate([oracle_rows(oracle, s["cmap"], qc), oracle_rows(oracle, s["smap"], qs)])
        assert np.array_equal(rows[acc], r.nn[acc])
        # the search alone, before the gates: the kd-tree finds and refuses what the brute-force search finds and refuses, on every query
        assert np.array_equal(rows, np.concatenate([map_ref.knn5_many(s["cmap"], qc), map_ref.knn5_many(s["smap"], qs)]))
    return r, xo, st


@pytest.mark.parametrize("name", SCENES)
def test_reference_agrees_with_the_oracle(oracle, name):
    s = map_cases.by_name(name)
    r, xo, st = compare_with_oracle(oracle, s)
    if s["kind"] in ("L", "H"):
        # precondition of the exact scenes, on the reference and on the oracle: no LM iteration, the pose bytes unchanged
        assert r.stats[4:] == [0, 0] and [st.lm_iters[0], st.lm_iters[1]] == [0, 0]
        assert r.pose.tobytes() == s["x0"].tobytes() and xo.tobytes() == s["x0"].tobytes()
        assert r.stats[1] > 0 and r.stats[3] > 0 and (r.nn[:, 0] < 0).any()
    if s["kind"] == "T":
        assert (r.stats[1] + r.stats[3] > 0) == s["solves"]
    if s["kind"] == "S":
        assert s["tag"] in r.traces[0] + r.traces[1], r.traces
        assert r.stats == s["stats"] and r.traces == s["traces"], (r.stats, r.traces)
        if name == "S_outliers":          # most residuals in Huber's linear part at the start
            blocks = map_ref.build_blocks(s["cmap"], s["smap"], s["cstack"], s["sstack"], s["x0"])[0]
            assert map_ref.huber_linear_share(blocks, s["x0"]) > 0.5
        assert np.isfinite(r.pose).all()


def test_lattice_scene_holds_its_edge_cases():
    s = map_cases.by_name("L_lattice")
    r = map_ref.refine(s["cmap"], s["smap"], s["cstack"], s["sstack"], s["x0"])
    base, note = len(s["cstack"]), s["note"]
    for tag in ("fifth_at_1", "fifth_at_1_neg", "three_in_reach", "four_in_reach_fifth_far"):
        assert r.nn[base + note[tag], 0] < 0 and map_ref.knn5(s["smap"], s["sstack"][note[tag], :3]) is None, tag
    for tag in ("fifth_below_1", "fifth_below_1_tie", "diagonal_cell", "diagonal_cell_neg", "diagonal_cell_mixed"):
        assert r.nn[base + note[tag], 0] >= 0, tag
    q = s["sstack"][note["fifth_at_1"], :3]; row = np.argsort(((s["smap"][:, :3] - q) ** 2).sum(axis=1), kind="stable")[:5]
    assert ((s["smap"][row[4], :3] - q) ** 2).sum() == 1.0
    q = s["sstack"][note["fifth_below_1_tie"], :3]; row = r.nn[base + note["fifth_below_1_tie"]]
    d = ((s["smap"][:, :3] - q) ** 2).sum(axis=1)
    assert d[row[4]] == 61.0 / 64.0 and (d == d[row[4]]).sum() == 3 and row[4] == np.nonzero(d == d[row[4]])[0][0]      # the tie goes to the lowest index
    # the diagonal query's own cell and its face neighbours hold nothing
    q = s["sstack"][note["diagonal_cell"], :3]
    cells = np.floor(s["smap"][r.nn[base + note["diagonal_cell"]], :3]) - np.floor(q)
    assert (np.abs(cells[:, :2]).sum(axis=1) == 2).all()


def test_gate_scene_keeps_enough_clusters_on_each_side():
    g = map_cases.gate_scene()
    for gates in (g["line_gates"], g["plane_gates"]):
        assert sum(x.ok for x in gates) >= 200 and sum(not x.ok for x in gates) >= 200
        assert min(x.margin for x in gates) >= map_cases.MIN_MARGIN
    for tag in ("two_equal", "collinear", "four_coincide"):
        assert tag in g["corner_tags"]
    for tag in ("near_origin", "constant_column", "zero_column", "two_zero_columns"):
        assert tag in g["surf_tags"]
    # isolation: every cluster within 0.5 m of its centroid, every other map point more than 3 m from it
    for P, cloud in ((g["corner_clusters"], g["cmap"]), (g["surf_clusters"], g["smap"])):
        c = P.astype(np.float64).mean(axis=1)
        assert np.sqrt(((P - c[:, None]) ** 2).sum(axis=2)).max() <= 0.5
        for i in range(0, len(P), 7):
            d = np.sqrt(((cloud[:, :3].astype(np.float64) - c[i]) ** 2).sum(axis=1))
            d[5 * i:5 * i + 5] = np.inf
            assert d.min() > 3.5, i


def test_oracle_gates_agree_with_the_reference_on_every_cluster(oracle):
    g = map_cases.gate_scene()
    for p, ref in zip(g["corner_clusters"], g["line_gates"]):
        P = p.astype(np.float64)
        c = P.sum(axis=0) / 5.0
        ev, vec = oracle.sym_eig3((P - c).T @ (P - c))
        assert bool(ev[2] > 3.0 * ev[1]) == ref.ok
        assert np.abs(ev - ref.ev).max() <= 1e-12 * max(ref.ev[2], 1e-300)
        if ref.ok and ref.ev[2] > 1.5 * ref.ev[1]:
            assert abs(abs(vec[:, 2] @ ref.direction) - 1.0) < 1e-9
    for p, ref in zip(g["surf_clusters"], g["plane_gates"]):
        ok, n, d = oracle.plane_fit5(p.astype(np.float64))
        assert ok == ref.ok
        assert abs(d - ref.d) < 1e-9 * max(1.0, ref.d) and np.abs(n - ref.normal).max() < 1e-9


def test_reference_agrees_with_the_oracle_on_two_frames_of_the_synthetic_world(oracle):
    from test_mapping_gpu import _scan_clouds
    w = oracle.S1World(n_az=500)
    x, off = w.scans(w.trajectory(6))
    ref = oracle.run_sequence(x, off)
    m = oracle.Map()
    for k in range(6):
        ls, lf = _scan_clouds(oracle, x, off, k)
        if k >= 4:
            s = dict(cmap=m.all_points(0), smap=m.all_points(1), cstack=oracle.voxel_filter(ls, 0.4), sstack=oracle.voxel_filter(lf, 0.8), x0=ref["poses"][k].copy())
            r, _, _ = compare_with_oracle(oracle, s)
            assert r.stats[1] > 100 and r.stats[3] > 500
        m.process(ls, lf, ref["poses"][k, :4], ref["poses"][k, 4:])
