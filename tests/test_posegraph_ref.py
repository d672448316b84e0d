"""The pose-graph oracle (oracle/lo_posegraph.c) pinned to an independent statement of the graph (tests/posegraph_ref.py: numpy,
complex-step Jacobians): its linearisation [H | g | cost] expanded to dense, its converged answer, and its rank splits.  fp64
against fp64 in another operation order: max|a - b| <= 1e-12 (max|b| + 1), the form of tests/test_ba_factors_gpu.py."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import posegraph_cases as K
from tests import posegraph_ref as A

GRAPHS = sorted(K.LINEARISATION_GRAPHS)


def _assert_close(what, a, b, rel=1e-12):
    ok, gap, bound = K.close(a, b, rel)
    print("%s: max|a - b| = %.3e, bound %.3e" % (what, gap, bound))
    assert ok, (what, gap, bound)


def _oracle_system(g, rank=0, world=1):
    pg = O.PoseGraph(g["odom"], g["loops"], g["loop_info"])
    pg.linearise(rank, world)
    return pg, K.expand_oracle(pg.reduce_tensor, pg.n, pg.bandwidth, pg.order())


@pytest.mark.parametrize("name", GRAPHS)
def test_oracle_linearisation_equals_the_reference_system(name):
    g = K.LINEARISATION_GRAPHS[name]()
    ref = A.edges(g["odom"], g["loops"], g["loop_info"])
    K.assert_coverage(ref)
    pg, (H, grad, cost) = _oracle_system(g)
    assert sorted(pg.order()) == list(range(pg.n))
    Hr, gr, cr = A.dense_system(ref, ref.x0)
    assert np.array_equal(Hr, Hr.T) and np.array_equal(Hr[:4, :4], np.eye(4)) and not Hr[4:, :4].any() and not gr[:4].any()
    _assert_close(name + " H", H, Hr)
    _assert_close(name + " g", grad, gr)
    _assert_close(name + " cost", cost, cr)


def test_reference_jacobians_are_the_derivative_of_its_residual():
    """The complex step against a central difference of the same residual (1e-6 of the largest entry: the difference's own
    truncation), and the gradient of the cost against J^T r with the robust weight: the reference is consistent with itself."""
    g = K.LINEARISATION_GRAPHS["n6"]()
    ref = A.edges(g["odom"], g["loops"], g["loop_info"])
    Ja, Jb = A.jacobians(ref, ref.x0)
    h = 1e-5
    for e in range(len(ref.a)):
        for node, J in ((ref.a[e], Ja[e]), (ref.b[e], Jb[e])):
            for k in range(4):
                xp, xm = ref.x0.copy(), ref.x0.copy()
                xp[node, k] += h; xm[node, k] -= h
                fd = (A.residual(ref, xp, e) - A.residual(ref, xm, e)) / (2 * h)
                assert np.abs(fd - J[:, k]).max() <= 1e-6 * (np.abs(J).max() + 1)
    H, grad, _ = A.dense_system(ref, ref.x0)
    _assert_close("gradient", grad[4:], A.gradient(ref, ref.x0).reshape(-1)[4:])


# max|gradient(x*)| / max|gradient(x0)| over the free keyframes, measured with the oracle as committed (max_iter = 50: every solve
# stops on the function tolerance after 3, 3, 9 and 6 iterations); the test allows ten times the measured figure.
MEASURED_GRADIENT_RATIO = {"n2": 1.55e-5, "n6": 3.73e-6, "n120": 1.67e-3, "n300_outliers": 5.37e-3}


@pytest.mark.parametrize("name", GRAPHS)
def test_converged_oracle_solve_is_a_stationary_point_of_the_reference_cost(name):
    """Measured: cost(x*) of the reference against the oracle's final_cost differs by 0, 1.4e-16, 1.1e-14 and 2.3e-16 relative
    (n2, n6, n120, n300_outliers); the gradient ratios are MEASURED_GRADIENT_RATIO."""
    g = K.LINEARISATION_GRAPHS[name]()
    ref = A.edges(g["odom"], g["loops"], g["loop_info"])
    out, st = O.pose_graph_optimize(g["odom"], g["loops"], g["loop_info"], max_iter=50)
    assert 0 < st["iterations"] < 50, st                                   # stopped on a tolerance, not on the count
    xs = A.edges(out, g["loops"], g["loop_info"]).x0                        # (yaw, t) of the result, edges still those of the input
    c = A.cost(ref, xs)
    print("%s: cost %.17g, oracle final_cost %.17g" % (name, c, st["final_cost"]))
    assert abs(c - st["final_cost"]) <= 1e-9 * st["final_cost"]
    assert abs(A.cost(ref, ref.x0) - st["initial_cost"]) <= 1e-9 * st["initial_cost"]
    ratio = np.abs(A.gradient(ref, xs)[1:]).max() / np.abs(A.gradient(ref, ref.x0)[1:]).max()
    print("%s: gradient ratio %.3e" % (name, ratio))
    assert ratio <= 10.0 * MEASURED_GRADIENT_RATIO[name]


@pytest.mark.parametrize("world", [2, 3, 7])
def test_oracle_rank_splits_sum_to_the_whole(world):
    for name in GRAPHS:
        g = K.LINEARISATION_GRAPHS[name]()
        pg = O.PoseGraph(g["odom"], g["loops"], g["loop_info"])
        pg.linearise(0, 1)
        whole = pg.reduce_tensor.copy()
        total = np.zeros_like(whole)
        for r in range(world):
            pg.linearise(r, world)
            total += pg.reduce_tensor
        _assert_close("%s world %d" % (name, world), total, whole)


@pytest.mark.parametrize("name", sorted(K.BANDS))
def test_band_graphs_stay_in_their_class(name):
    """The frozen random-loop graphs give the half bandwidth they were searched for (a change to the ordering must not move a
    case back onto the covered path unnoticed) and the n % panel width the table states."""
    n, n_loops, seed, keep, lo, hi, P = K.BANDS[name]
    g = K.band_graph(name)
    pg = O.PoseGraph(g["odom"], g["loops"], g["loop_info"])
    assert lo <= pg.bandwidth <= hi, (name, pg.bandwidth)
    assert K.panel_width(pg.bandwidth) == P and sorted(pg.order()) == list(range(n))
    assert len(g["loops"]) == keep and (g["loops"][:, 1] - g["loops"][:, 0] >= 5).all()
    found, w = K.search_band(O, n, lo, hi, n_loops=n_loops, seeds=[seed])
    assert found == (n, n_loops, seed, keep) and w == pg.bandwidth          # the search that froze it is reproducible


def test_band_graphs_cover_the_panel_remainders():
    rem = {name: (K.BANDS[name][6], K.BANDS[name][0] % K.BANDS[name][6]) for name in K.BANDS}
    assert rem["w8_last"][0] == 8 and rem["w8_last"][1] in (1, 7)
    assert rem["w4_first"] == (4, 1) and rem["w4_widest"] == (4, 3)
