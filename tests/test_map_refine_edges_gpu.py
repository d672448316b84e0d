"""lmono_map_refine (k_grid_*, k_map_correspond, k_map_factor, k_map_solve) against tests/map_ref.py on the built scenes of tests/map_cases.py:
the exact neighbour rows of the lattice and hash scenes, the thresholds, the gates on isolated clusters, the solve's branches and a batch of 13
different streams.  tests/test_map_ref_cpu.py shows that map_ref agrees with the CPU oracle on every one of these scenes.

Kernel mutations these tests were seen to fail under (one run each, on a scratch copy of the kernels):
    no index tie-break in top5_insert     test_exact_neighbour_rows[L_lattice, H_single_cell, H_interrupted]
    d5 <= 1.0 for d5 < 1.0                test_exact_neighbour_rows[L_lattice, H_1023, H_1024, H_2047, H_2048]
    ev[2] > 3 ev[0] for 3 ev[1]           test_gates_decide_like_the_reference
    k_map_solve's stream = blockIdx.x % 8 (the group of eight dropped)     test_streams_do_not_depend_on_their_batch
(each of the first three also fails test_streams_do_not_depend_on_their_batch, which compares every stream with the reference's counts).
Not caught: `>= 0.2` for `> 0.2` in plane_fit5 differs only for a distance bit-equal to the double 0.2, which no scene produces; and the
(block, stream) decode of map_block_of is not reached from lmono_map_refine at all -- it launches k_map_correspond / k_map_factor on a 2-D grid
for any number of streams (the 1-D decode belongs to lmono_mapper_process_batch) -- so the batch test covers k_map_solve's decode only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_cases  # noqa: E402
import map_ref  # noqa: E402

pytestmark = pytest.mark.gpu

_REF = {}


def reference(s):
    if s["name"] not in _REF:
        _REF[s["name"]] = map_ref.refine(s["cmap"], s["smap"], s["cstack"], s["sstack"], s["x0"])
    return _REF[s["name"]]


def run(gpu_ctx, scenes):
    poses, stats, nn = gpu_ctx.map_refine([s["cmap"] for s in scenes], [s["smap"] for s in scenes], [s["cstack"] for s in scenes], [s["sstack"] for s in scenes],
                                          np.array([s["x0"] for s in scenes]), want_nn=True)
    off = np.concatenate([[0], np.cumsum([len(s["cstack"]) + len(s["sstack"]) for s in scenes])])
    return [(poses[i], stats[i, :6].copy(), nn[off[i]:off[i + 1]].copy()) for i in range(len(scenes))]


@pytest.mark.parametrize("name", [s["name"] for s in map_cases.all_scenes() if s["kind"] in ("L", "H")])
def test_exact_neighbour_rows(gpu_ctx, name):
    """L and H: the same five indices in the same order on every query, -1 rows where the reference refuses; no tolerance, no exceptions."""
    s = map_cases.by_name(name)
    r = reference(s)
    pose, stats, nn = run(gpu_ctx, [s])[0]
    assert r.stats[4:] == [0, 0] and (r.nn[:, 0] >= 0).sum() > 40 and (r.nn[:, 0] < 0).any()
    assert list(stats) == r.stats
    assert pose.tobytes() == s["x0"].tobytes()
    assert np.array_equal(nn, r.nn), np.nonzero((nn != r.nn).any(axis=1))[0][:10]


def test_thresholds(gpu_ctx):
    """T: no blocks and an untouched pose unless the corner map has more than 10 and the surf map more than 50 points."""
    for s in (x for x in map_cases.all_scenes() if x["kind"] == "T"):
        pose, stats, nn = run(gpu_ctx, [s])[0]
        r = reference(s)
        assert list(stats) == r.stats and np.array_equal(nn, r.nn), s["name"]
        assert pose.tobytes() == s["x0"].tobytes()
        assert (stats[1] > 0 and stats[3] > 0) == s["solves"], s["name"]
        if not s["solves"]:
            assert not stats.any() and (nn < 0).all()


def test_gates_decide_like_the_reference(gpu_ctx):
    """G: every isolated cluster gives a block if and only if the reference's gate says yes, with exactly the cluster's five points."""
    g = map_cases.gate_scene()
    r = reference(g)
    pose, stats, nn = run(gpu_ctx, [g])[0]
    nc, ncs = len(g["corner_clusters"]), len(g["cstack"])
    for base, gates in ((0, g["line_gates"]), (ncs, g["plane_gates"])):
        for c, gate in enumerate(gates):
            row = nn[base + c]
            assert (row[0] >= 0) == gate.ok, (base, c, gate)
            if gate.ok:
                assert sorted(row.tolist()) == list(range(5 * c, 5 * c + 5)), (base, c)
    assert nc >= 400 and len(g["plane_gates"]) >= 400
    assert list(stats[:4]) == r.stats[:4]
    assert np.array_equal(nn, r.nn)
    assert np.abs(pose - g["x0"]).max() < 5e-3 and np.abs(pose - r.pose).max() < 1e-9


@pytest.mark.parametrize("name", [s["name"] for s in map_cases.all_scenes() if s["kind"] == "S"])
def test_solver_branches(oracle, gpu_ctx, name):
    """S: one scene per way through k_map_solve's trust-region loop (the reference's trace names it): the iteration counts of the reference and of
    the oracle, the oracle's pose within 1e-9."""
    s = map_cases.by_name(name)
    r = reference(s)
    assert s["tag"] in r.traces[0] + r.traces[1] and r.traces == s["traces"] and r.stats == s["stats"]
    xo, st, _ = oracle.map_refine(s["cmap"], s["smap"], s["cstack"], s["sstack"], s["x0"])
    pose, stats, nn = run(gpu_ctx, [s])[0]
    assert list(stats) == r.stats == [st.n_edge[0], st.n_edge[1], st.n_plane[0], st.n_plane[1], st.lm_iters[0], st.lm_iters[1]]
    assert np.isfinite(pose).all() and np.abs(pose - xo).max() < 1e-9
    assert np.array_equal(nn, r.nn)


def test_streams_do_not_depend_on_their_batch(gpu_ctx):
    """B: 13 different streams (an empty map, empty stacks, one with far more queries than the rest) as batches of 8, 9 and 13 give, byte for
    byte, what each stream gives alone.  Of the two (block, stream) decodes only k_map_solve's is covered: lmono_map_refine launches
    k_map_correspond and k_map_factor on a 2-D grid for any number of streams, so map_block_of's 1-D decode (lmono_mapper_process_batch) is
    not run here."""
    streams = map_cases.batch_streams()
    alone = [run(gpu_ctx, [s])[0] for s in streams]
    key = [a[0].tobytes() + a[1].tobytes() + a[2].tobytes() for a in alone]
    assert len(set(key)) == len(key)                          # no two streams alike: a mix-up cannot hide
    nq = sorted(len(a[2]) for a in alone)
    assert nq[0] == 0 and nq[-1] > 3 * nq[-2]
    for s, a in zip(streams, alone):
        if s["kind"] != "B":
            assert list(a[1]) == reference(s).stats, s["name"]
    for n in (8, 9, 13):
        got = run(gpu_ctx, streams[:n])
        for i in range(n):
            assert got[i][0].tobytes() == alone[i][0].tobytes(), (n, i, streams[i]["name"])
            assert np.array_equal(got[i][1], alone[i][1]), (n, i, streams[i]["name"])
            assert np.array_equal(got[i][2], alone[i][2]), (n, i, streams[i]["name"])
