"""Loop-closure pose graph on the GPU (lmono_pose_graph_*, SURVEY.md row 8f-2 -- a new feature: the checker is the CPU oracle's
statement of the same graph, not the reference) on S4 graphs: same trust-region path (iterations, accepted / rejected steps),
costs to 1e-9 relative and keyframes to 1e-7 (sin / cos and the elimination order differ in the last bits).

Below the solves: the elimination order and the linearisation [H | g | cost] against tests/posegraph_ref.py (an independent numpy
statement of the graph) and the oracle, the band classes of the panelled Cholesky (tests/posegraph_cases.py: BANDS), the reject
and invalid-step branches of the trust region driven through the round API, and the small edges.

  test                                   half bandwidth w   panel width P   n % P
  linearisation n2 / n6 / n120 / n300    1 / 5 / 36 / 64    8               2 / 6 / 0 / 4
  band w8_last                           113                8               601 % 8 = 1
  band w4_first (+ linearisation)        128                4               601 % 4 = 1
  band w4_widest                         255 (= the cap)    4               603 % 4 = 3
  refused                                299                -               create fails
  step branches                          26                 8               150 % 8 = 6
  small edges n = 2, 3, 5                1, 2, 4            8               n < P"""
import numpy as np
import pytest

from tests import posegraph_cases as K
from tests import posegraph_ref as A
from workloads import s4

pytestmark = pytest.mark.gpu


def _compare(oracle, ctx, g, max_iter=5, tol=1e-7):
    import lmono_amd
    pg = lmono_amd.PoseGraph(ctx, g["odom"], g["loops"], g["loop_info"])
    out, st = pg.optimize(max_iter)
    ref, rs = oracle.pose_graph_optimize(g["odom"], g["loops"], g["loop_info"], max_iter=max_iter)
    assert (st["iterations"], st["accepted"], st["rejected"]) == (rs["iterations"], rs["accepted"], rs["rejected"]), (st, rs)
    assert st["bandwidth"] == rs["bandwidth"] == pg.bandwidth, (st, rs)
    assert abs(st["initial_cost"] - rs["initial_cost"]) <= 1e-9 * max(rs["initial_cost"], 1e-12)
    assert abs(st["final_cost"] - rs["final_cost"]) <= 1e-9 * max(rs["final_cost"], 1e-12)
    assert np.abs(out[:, :3] - ref[:, :3]).max() < tol and np.abs(np.abs(out[:, 3:]) - np.abs(ref[:, 3:])).max() < tol
    pg.close()
    return out, st


def test_matches_oracle_on_a_two_lap_graph(oracle, gpu_ctx):
    g = s4.make_graph(n=300)
    out, st = _compare(oracle, gpu_ctx, g)
    assert st["final_cost"] < 0.2 * st["initial_cost"] and st["bandwidth"] >= 4
    assert s4.ate(out, g["truth"]) < 0.4 * s4.ate(g["odom"], g["truth"])
    assert np.abs(out[0] - g["odom"][0]).max() < 1e-12


def test_configs3_graph_at_its_size(oracle, gpu_ctx):
    """BASELINE configs[3]'s graph at its named size: 4541 keyframes (KITTI seq 00), the graph `bench.py --workload posegraph` measures
    (2.2 laps, half bandwidth ~67 blocks) against oracle/lo_posegraph.c -- same accepted / rejected steps, costs to 1e-9, keyframes to 1e-7."""
    g = s4.make_graph(n=4541, laps=2.2)
    out, st = _compare(oracle, gpu_ctx, g)
    assert st["bandwidth"] > 40 and len(g["loops"]) > 100
    assert s4.ate(out, g["truth"]) < 0.5 * s4.ate(g["odom"], g["truth"])


def test_more_iterations_outliers_and_short_graphs(oracle, gpu_ctx):
    _compare(oracle, gpu_ctx, s4.make_graph(n=300, outliers=3), max_iter=12)
    _compare(oracle, gpu_ctx, s4.make_graph(n=120, loop_gap=30, seed=3), max_iter=8)
    _compare(oracle, gpu_ctx, s4.make_graph(n=6, loop_gap=3, loop_radius=100.0, loop_every=1, seed=5), max_iter=5)


def test_no_loops_and_bad_arguments(oracle, gpu_ctx):
    import lmono_amd
    g = s4.make_graph(n=80)
    pg = lmono_amd.PoseGraph(gpu_ctx, g["odom"], np.zeros((0, 2)), np.zeros((0, 8)))
    out, st = pg.optimize(5)
    assert st["iterations"] == 0 and st["bandwidth"] == 4 and np.abs(out[:, :3] - g["odom"][:, :3]).max() < 1e-12
    with pytest.raises(lmono_amd.LmonoError):
        lmono_amd.PoseGraph(gpu_ctx, g["odom"], [[0, 80]], np.zeros((1, 8)))          # loop index out of range
    with pytest.raises(lmono_amd.LmonoError):
        lmono_amd.PoseGraph(gpu_ctx, g["odom"][:1], np.zeros((0, 2)), np.zeros((0, 8)))


def test_rank_split_rounds_on_one_gpu(oracle, gpu_ctx):
    """The multi-GPU round structure with two rank objects on one device: the buffers each rank linearises (its own edges only)
    are summed the way the all-reduce would, both ranks step identically, and the result equals the single-rank solve."""
    import torch
    import lmono_amd
    from lmono_amd import sharding
    g = s4.make_graph(n=300)
    single, st = lmono_amd.PoseGraph(gpu_ctx, g["odom"], g["loops"], g["loop_info"]).optimize(5)
    world = 2
    ranks = [lmono_amd.PoseGraph(gpu_ctx, g["odom"], g["loops"], g["loop_info"]) for _ in range(world)]
    bufs = [torch.zeros(pg.reduce_count, dtype=torch.float64, device="cuda:0") for pg in ranks]
    for pg, b in zip(ranks, bufs):
        pg.use_reduce_tensor(b)
    for _ in range(6):
        for r, pg in enumerate(ranks):
            pg.linearise(r, world)
        gpu_ctx.synchronize()
        assert float(bufs[0].abs().sum()) > 0 and float(bufs[1].abs().sum()) > 0
        total = bufs[0] + bufs[1]
        for b in bufs:
            b.copy_(total)
        torch.cuda.synchronize()
        done = [pg.step(5) for pg in ranks]
        assert done[0] == done[1]
        if done[0]:
            break
    for pg in ranks:
        out, s2 = pg.result()
        assert s2["iterations"] == st["iterations"] and np.abs(out - single).max() < 1e-9
    # the driver used by bench.py / multi-GPU runs, world = 1
    pg = lmono_amd.PoseGraph(gpu_ctx, g["odom"], g["loops"], g["loop_info"])
    assert sharding.pose_graph_rounds(pg, 0, 1, max_iter=5) >= 2
    assert np.abs(pg.result()[0] - single).max() == 0.0


# ---- order, linearisation, band classes, step branches, small edges ---------------------------------------------------------
def _assert_close(what, a, b, rel=1e-12):
    ok, gap, bound = K.close(a, b, rel)
    print("%s: max|a - b| = %.3e, bound %.3e" % (what, gap, bound))
    assert ok, (what, gap, bound)


def _all_graphs():
    out = {name: mk() for name, mk in K.LINEARISATION_GRAPHS.items()}
    out.update({name: K.band_graph(name) for name in K.BANDS if name != "refused"})
    return out


class _Pair:
    """The same graph on the GPU (on a torch reduce tensor) and in the oracle."""

    def __init__(self, oracle, ctx, g):
        import torch
        import lmono_amd
        self.ctx = ctx
        self.gpu = lmono_amd.PoseGraph(ctx, g["odom"], g["loops"], g["loop_info"])
        self.buf = torch.zeros(self.gpu.reduce_count, dtype=torch.float64, device="cuda:0")
        self.gpu.use_reduce_tensor(self.buf)
        self.cpu = oracle.PoseGraph(g["odom"], g["loops"], g["loop_info"])
        self.n, self.w = self.gpu.n, self.gpu.bandwidth
        self.hsz, self.n4 = self.n * (self.w + 1) * 16, 4 * self.n           # both layouts: hsz doubles of H, then n4 of g

    def gpu_buffer(self, rank=0, world=1):
        self.gpu.linearise(rank, world)
        self.ctx.synchronize()
        return self.buf.cpu().numpy().copy()

    def gpu_system(self, rank=0, world=1):
        return K.expand_gpu(self.gpu_buffer(rank, world), self.n, self.w, self.gpu.order())

    def cpu_system(self):
        self.cpu.linearise(0, 1)
        return K.expand_oracle(self.cpu.reduce_tensor, self.n, self.cpu.bandwidth, self.cpu.order())

    def close(self):
        self.gpu.close()


def test_elimination_order_and_bandwidth_equal_the_oracles(oracle, gpu_ctx):
    import lmono_amd
    for name, g in _all_graphs().items():
        pg = lmono_amd.PoseGraph(gpu_ctx, g["odom"], g["loops"], g["loop_info"])
        ref = oracle.PoseGraph(g["odom"], g["loops"], g["loop_info"])
        assert pg.bandwidth == ref.bandwidth, (name, pg.bandwidth, ref.bandwidth)
        assert np.array_equal(pg.order(), ref.order()), name
        if name in K.BANDS:
            assert K.BANDS[name][4] <= pg.bandwidth <= K.BANDS[name][5] and K.panel_width(pg.bandwidth) == K.BANDS[name][6]
        pg.close()


@pytest.mark.parametrize("name", sorted(K.LINEARISATION_GRAPHS) + ["w4_first"])
def test_linearisation_equals_the_reference_and_the_oracle(oracle, gpu_ctx, name):
    """[H | g | cost] of the GPU expanded to dense, at the starting point against tests/posegraph_ref.py and the oracle, and
    after one accepted step (the linearisation point is then the candidate) against the oracle at its own candidate."""
    g = _all_graphs()[name]
    ref = A.edges(g["odom"], g["loops"], g["loop_info"])
    if name in K.LINEARISATION_GRAPHS:
        K.assert_coverage(ref)
    else:
        assert 121 <= oracle.PoseGraph(g["odom"], g["loops"], g["loop_info"]).bandwidth <= 128
    pair = _Pair(oracle, gpu_ctx, g)
    assert pair.w == pair.cpu.bandwidth
    H, grad, cost = pair.gpu_system()
    Ho, go, co = pair.cpu_system()
    Hr, gr, cr = A.dense_system(ref, ref.x0)
    for what, a, b in (("H vs reference", H, Hr), ("g vs reference", grad, gr), ("H vs oracle", H, Ho), ("g vs oracle", grad, go),
                       ("cost vs reference", cost.sum(), cr), ("cost vs oracle", cost.sum(), co)):
        _assert_close(name + " x0 " + what, a, b)
    # the cost segment holds every edge once: at the position of its newer keyframe
    per_node = np.zeros(pair.n)
    np.add.at(per_node, ref.b, A.edge_costs(ref, ref.x0))
    _assert_close(name + " cost per keyframe", cost[pair.gpu.order()], per_node)
    # one accepted step on each side, then the linearisation at the candidate
    assert not pair.gpu.step(5) and not pair.cpu.step(5)
    H, grad, cost = pair.gpu_system()
    Ho, go, co = pair.cpu_system()
    assert not np.array_equal(Ho, Hr)
    for what, a, b in (("H", H, Ho), ("g", grad, go), ("cost", cost.sum(), co)):
        _assert_close(name + " candidate " + what + " vs oracle", a, b)
    assert pair.gpu.step(5) == pair.cpu.step(5)
    assert pair.gpu.result()[1]["accepted"] == pair.cpu.result()[1]["accepted"] == 1
    pair.close()


@pytest.mark.parametrize("world", [2, 3, 7])
def test_rank_splits_on_one_device_sum_to_the_whole(oracle, gpu_ctx, world):
    for name in sorted(K.LINEARISATION_GRAPHS) + ["w4_first"]:
        pair = _Pair(oracle, gpu_ctx, _all_graphs()[name])
        whole = pair.gpu_buffer(0, 1)
        total = np.zeros_like(whole)
        for r in range(world):
            total += pair.gpu_buffer(r, world)
        _assert_close("%s world %d" % (name, world), total, whole)
        pair.close()


@pytest.mark.parametrize("name", ["w8_last", "w4_first", "w4_widest"])
def test_band_classes_of_the_panelled_cholesky(oracle, gpu_ctx, name):
    """Same path, costs to 1e-9 and keyframes to 1e-7 as on the narrow graphs; every case asserts the band class it ran in."""
    n, n_loops, seed, keep, lo, hi, P = K.BANDS[name]
    g = K.band_graph(name)
    out, st = _compare(oracle, gpu_ctx, g)
    assert lo <= st["bandwidth"] <= hi and K.panel_width(st["bandwidth"]) == P and n % P in (1, P - 1)
    assert st["iterations"] == 5 and st["final_cost"] < 0.5 * st["initial_cost"]


def test_too_wide_a_band_is_refused_and_the_next_graph_solves(oracle, gpu_ctx):
    import lmono_amd
    g = K.band_graph("refused")
    w = oracle.PoseGraph(g["odom"], g["loops"], g["loop_info"]).bandwidth
    assert w >= 256
    with pytest.raises(lmono_amd.LmonoError, match=r"bandwidth %d\b" % w):
        lmono_amd.PoseGraph(gpu_ctx, g["odom"], g["loops"], g["loop_info"])
    _compare(oracle, gpu_ctx, K.LINEARISATION_GRAPHS["n120"](), max_iter=8)


def _tampered_rounds(oracle, ctx, g, tamper, max_iter):
    """Both sides through the round API; tamper(round, buffer, hsz, n4) edits each side's own [H | g | cost] between linearise
    and step.  -> ((gpu poses, stats), (oracle poses, stats)); done is compared round by round."""
    import torch
    pair = _Pair(oracle, ctx, g)
    for r in range(max_iter + 2):
        pair.gpu.linearise(0, 1)
        ctx.synchronize()
        tamper(r, pair.buf, pair.hsz, pair.n4)
        torch.cuda.synchronize()
        pair.cpu.linearise(0, 1)
        tamper(r, pair.cpu.reduce_tensor, pair.hsz, pair.n4)
        done = pair.gpu.step(max_iter), pair.cpu.step(max_iter)
        assert done[0] == done[1], (r, done)
        if done[0]:
            break
    assert done[0]
    res = pair.gpu.result(), pair.cpu.result()
    pair.close()
    (out, st), (ref, rs) = res
    assert (st["iterations"], st["accepted"], st["rejected"]) == (rs["iterations"], rs["accepted"], rs["rejected"]), (st, rs)
    assert abs(st["initial_cost"] - rs["initial_cost"]) <= 1e-9 * rs["initial_cost"]
    assert abs(st["final_cost"] - rs["final_cost"]) <= 1e-9 * rs["final_cost"]
    assert np.abs(out[:, :3] - ref[:, :3]).max() < 1e-7 and np.abs(np.abs(out[:, 3:]) - np.abs(ref[:, 3:])).max() < 1e-7
    return res


def test_rejected_steps_follow_the_oracle(oracle, gpu_ctx):
    """The cost segment times 4 in rounds 2 and 3 makes the trust region reject two candidates in a row (radius / 2, then / 4,
    the diagonal reused); both sides then go the same way: 8 iterations, 6 accepted, 2 rejected, and end near the plain run's
    cost (both are within the solver's function tolerance, 1e-6 relative, of the minimum: 1e-5 is asserted)."""
    g = s4.make_graph(n=150, loop_gap=30)

    def cost_times_4(r, buf, hsz, n4):
        if r in (2, 3):
            buf[hsz + n4:] *= 4.0

    plain = _tampered_rounds(oracle, gpu_ctx, g, lambda *a: None, 8)
    assert plain[0][1]["rejected"] == 0
    (out, st), _ = _tampered_rounds(oracle, gpu_ctx, g, cost_times_4, 8)
    assert st["rejected"] >= 2 and (st["iterations"], st["accepted"], st["rejected"]) == (8, 6, 2), st
    assert abs(st["final_cost"] - plain[0][1]["final_cost"]) <= 1e-5 * plain[0][1]["final_cost"]


def test_invalid_steps_stop_after_five_and_keep_the_last_accepted_keyframes(oracle, gpu_ctx):
    """H negated from round 1 on: the candidate of round 0 is still accepted (its cost is untouched), then the pivot fails five
    times (radius halved, no candidate) and the solve stops: 6 iterations, 1 accepted; the keyframes are those of the one
    accepted step, bit for bit."""
    g = s4.make_graph(n=150, loop_gap=30)

    def negate_h(r, buf, hsz, n4):
        if r >= 1:
            buf[:hsz] *= -1.0

    (out, st), (ref, rs) = _tampered_rounds(oracle, gpu_ctx, g, negate_h, 8)
    assert (st["iterations"], st["accepted"], st["rejected"]) == (6, 1, 0), st
    (one, s1), (one_ref, _) = _tampered_rounds(oracle, gpu_ctx, g, lambda *a: None, 1)
    assert s1["accepted"] == 1 and np.array_equal(out, one) and np.array_equal(ref, one_ref)
    assert st["final_cost"] == s1["final_cost"]


@pytest.mark.parametrize("n", [2, 3, 5])
@pytest.mark.parametrize("loops", [True, False])
def test_fewer_keyframes_than_a_panel(oracle, gpu_ctx, n, loops):
    import lmono_amd
    g = K.small_graph(n, loops=loops, seed=10 + n)
    out, st = _compare(oracle, gpu_ctx, g, max_iter=8)
    assert st["bandwidth"] == min(n - 1, 4) and (st["iterations"] > 0) == loops
    # max_iter = 0: the input poses (through yaw / pitch / roll and back), no iteration
    pg = lmono_amd.PoseGraph(gpu_ctx, g["odom"], g["loops"], g["loop_info"])
    out0, st0 = pg.optimize(0)
    ref0, rs0 = oracle.pose_graph_optimize(g["odom"], g["loops"], g["loop_info"], max_iter=0)
    assert st0["iterations"] == rs0["iterations"] == 0 and st0["accepted"] == 0
    assert abs(st0["initial_cost"] - rs0["initial_cost"]) <= 1e-9 * max(rs0["initial_cost"], 1e-12) and st0["final_cost"] == st0["initial_cost"]
    assert np.array_equal(out0[:, :3], g["odom"][:, :3]) and np.abs(np.abs(out0[:, 3:]) - np.abs(g["odom"][:, 3:])).max() < 1e-12
    # reset() and a second solve: the same bytes
    pg.reset()
    a, sa = pg.optimize(8)
    pg.reset()
    b, sb = pg.optimize(8)
    assert np.array_equal(a, b) and sa == sb and np.array_equal(a, out) and sa == st
    pg.close()


def test_reset_and_two_graphs_alive_at_once(oracle, gpu_ctx):
    """A wide (width-4 panels, 143 KB of LDS) and a narrow graph (width-8) alive together and stepped alternately each give the
    bytes of their solo run: the dynamic-LDS attribute belongs to the kernel, not to a graph.  reset() on either repeats it."""
    import lmono_amd
    graphs = [K.band_graph("w4_first"), K.LINEARISATION_GRAPHS["n120"]()]
    solo = []
    for g in graphs:
        pg = lmono_amd.PoseGraph(gpu_ctx, g["odom"], g["loops"], g["loop_info"])
        solo.append(pg.optimize(5))
        pg.close()
    pgs = [lmono_amd.PoseGraph(gpu_ctx, g["odom"], g["loops"], g["loop_info"]) for g in graphs]
    assert K.panel_width(pgs[0].bandwidth) == 4 and K.panel_width(pgs[1].bandwidth) == 8
    for attempt in range(2):
        done = [False, False]
        for _ in range(6):
            for k, pg in enumerate(pgs):
                if not done[k]:
                    pg.linearise(0, 1)
                    done[k] = pg.step(5)
        assert all(done)
        for k, pg in enumerate(pgs):
            out, st = pg.result()
            assert np.array_equal(out, solo[k][0]) and st == solo[k][1], (attempt, k)
            pg.reset()
    for pg in pgs:
        pg.close()
