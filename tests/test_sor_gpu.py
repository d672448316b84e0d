"""The statistical outlier removal on the GPU (lmono_sor_*) against the numpy restatement of its definition
(tests/sor_ref.py, brute force over all pairs): flags, v, the eight statistics, thr and the output cloud as bytes, for every shape at
which the search could go wrong and every way the same points can arrive."""
import os
import subprocess

import numpy as np
import pytest

from tests import colour_cases as CC
from tests import sor_ref as R
from tests import voxel_map_ref as VR

pytestmark = pytest.mark.gpu

ECAPACITY, EINVAL = -4, -1
H = np.float32(0.1)


def _pts(xyz, seed=0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return VR.points(xyz, np.random.default_rng(seed).integers(0, 1 << 32, len(xyz), dtype=np.uint64).astype(np.uint32))


def _assert_equal(f, ref, stats=None):
    keep, v = f.scores()
    if stats is not None:
        assert stats.tolist() == ref.stats.tolist()
    assert f.stats.tolist() == ref.stats.tolist()
    assert v.tobytes() == ref.v.tobytes() and keep.tobytes() == ref.keep.tobytes()
    assert f.threshold().tobytes() == np.array([ref.mean, ref.sd, ref.thr], np.float64).tobytes()
    assert f.cloud().tobytes() == ref.cloud.tobytes()


def _check(gpu_ctx, p, k, mul=1.0, cell=0.1, rings=8):
    import lmono_amd
    ref = R.run(p, k, mul, cell, rings)
    f = lmono_amd.OutlierFilter(gpu_ctx, max(len(p), 1), k, mul, cell, rings)
    _assert_equal(f, ref, f.filter(p))
    f.close()
    return ref


def _blob(n, seed, span=0.4, at=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    return _pts(rng.uniform(-span, span, (n, 3)) + np.asarray(at), seed)


def _m_is_one():
    """k = 2: the middle point of B - A - C has both others within rho, B and C are 1.2 rho apart."""
    s = 0.6 * float(R.rho_of(0.1, 8))
    return _pts([[5.0 - s, 1.0, 1.0], [5.0, 1.0, 1.0], [5.0 + s, 1.0, 1.0]])


SMALL = {
    "n0": lambda: (_pts(np.zeros((0, 3))), 4, [0, 0, 0, 0, 0]),
    "n_is_k": lambda: (_blob(6, 1, 0.04), 6, [6, 0, 6, 0, 0]),
    "k_plus_1_in_one_cell": lambda: (_blob(7, 2, 0.02, (0.05, 0.05, 0.05)), 6, [7, 0, 0, 7, None]),
    "identical": lambda: (_pts([[3.21, -4.5, 0.77]] * 40), 12, [40, 0, 0, 40, 40]),
    "m_is_1": lambda: (_m_is_one(), 2, [3, 0, 2, 1, 1]),
}


@pytest.mark.parametrize("shape", sorted(SMALL))
def test_smallest_shapes(gpu_ctx, shape):
    p, k, want = SMALL[shape]()
    ref = _check(gpu_ctx, p, k)
    assert all(w is None or int(s) == w for s, w in zip(ref.stats[:5], want)), ref.stats
    if shape == "identical":
        assert (ref.v == 0).all() and ref.thr == 0.0
    if shape == "k_plus_1_in_one_cell":
        assert len(set(VR.key_of(VR.cell_of(p, 0.1)[1]).tolist())) == 1


@pytest.mark.parametrize("k,mul", [(1, 1.0), (128, 1.0), (10, 0.0), (10, -0.7)])
def test_k_and_multiplier_extremes(gpu_ctx, k, mul):
    p = np.concatenate([_blob(500, 5, 0.3), _blob(40, 6, 2.0)])
    ref = _check(gpu_ctx, p, k, mul)
    assert ref.stats[3] > 400 and 0 < ref.stats[4] < ref.stats[3]


def _stopping_set(r, direction, k=4):
    """A query 0.001 h inside the faces of its cell towards `direction`; k points (r + 0.5) h away on the other side, in ring r; two points
    (r + 0.015) h away on this side, in ring r + 1.  Ring r holds k neighbours, none of them among the k nearest."""
    d = np.asarray(direction, np.float64)
    h = float(H)
    q = np.where(d > 0, 0.999, np.where(d < 0, 0.001, 0.5)) * h
    rng = np.random.default_rng(r)
    far = q - d * (r + 0.5) * h + np.where(d == 0, 1.0, 0.0) * rng.uniform(-0.02, 0.02, (k, 3)) * h
    near = q + d * (r + 0.015) * h + np.where(d == 0, 1.0, 0.0) * rng.uniform(-0.02, 0.02, (2, 3)) * h
    return np.concatenate([q[None, :], far, near])


DIRECTIONS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 1), (-1, -1, -1)]


@pytest.mark.parametrize("at", [(0.0, 0.0, 0.0), (6000.0, -6000.0, 300.0), (-41.3, -77.7, -3.1)])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_stopping_rule(gpu_ctx, r, at):
    k = 4
    sets = [_stopping_set(r, d, k) + 40.0 * float(H) * n * np.array([1.0, 0.0, 0.0]) for n, d in enumerate(DIRECTIONS)]      # 4 m apart: far beyond rho
    xyz = np.concatenate(sets)
    if at == (0.0, 0.0, 0.0):
        # on the restatement's cells: the k far points lie in ring r of the query's cell, the two near ones in ring r + 1
        for s in sets:
            c = VR.cell_of(_pts(s), float(H))[1]
            ring = np.abs(c[1:] - c[0]).max(1)
            assert (ring[:k] == r).all() and (ring[k:] == r + 1).all()
    p = _pts(xyz + np.asarray(at), r)
    ref = _check(gpu_ctx, p, k, 1.0, float(H), 8)
    assert ref.stats[3] >= len(DIRECTIONS)                                  # every query is scored


def test_points_on_cell_faces(gpu_ctx):
    m = np.arange(-6, 7)
    g = np.stack(np.meshgrid(m, m, m[:5], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    p = _pts(g * H, 3)                                                      # x = m * h in float32, on every axis
    ref = _check(gpu_ctx, p, 6, 1.0, float(H), 3)
    assert ref.stats[3] == len(p)
    _check(gpu_ctx, _pts(g * H * np.float32(0.5) - np.float32(0.3), 4), 26, 1.0, float(H), 2)


def test_isolation_boundary(gpu_ctx):
    """R = 2 (rho = 1.75 h).  A chain 0.34 h apart with k = 10: the tenth neighbour of an inner point is 1.7 h away, beyond ring 1's 0.75 h, so
    it is found in ring R itself; the points near the ends are isolated.  Then k = 1: a pair at d2 == rho2 exactly (both scored) and a pair
    one float further apart (both isolated)."""
    h = float(H)
    chain = np.stack([7.0 + 0.34 * h * np.arange(40), np.full(40, 2.03), np.full(40, -1.01)], 1)
    ref = _check(gpu_ctx, _pts(chain), 10, 1.0, h, 2)
    assert ref.stats[2] > 0 and ref.stats[3] > 20
    rho = R.rho_of(h, 2)
    above = np.nextafter(rho, np.float32(10.0), dtype=np.float32)
    pair = _pts([[0.0, 0.0, 0.0], [rho, 0.0, 0.0], [0.0, 100.0, 0.0], [above, 100.0, 0.0]])
    ref = _check(gpu_ctx, pair, 1, 1.0, h, 2)
    assert ref.v[:2].tolist() == [int(R.u_of(np.array([rho * rho], np.float32))[0]) >> 16] * 2 and (ref.v[2:] == R.NO_SCORE).all()
    assert ref.stats[2] == 2 and ref.stats[3] == 2


def test_a_crowded_cell(gpu_ctx):
    """3000 points in one cell, k = 100: thirty times more candidates than queries of a wave, far more than any on-chip buffer of values."""
    p = _blob(3000, 8, 0.045, (1.25, 1.25, 1.25))
    assert len(set(VR.key_of(VR.cell_of(p, 0.1)[1]).tolist())) == 1
    ref = _check(gpu_ctx, p, 100)
    assert ref.stats[3] == 3000


def test_mostly_single_cells_with_rejected_points(gpu_ctx):
    p = _blob(3000, 9, 1.5)
    keys = VR.key_of(VR.cell_of(p, 0.1)[1])
    assert len(set(keys.tolist())) > 2700
    bad = VR.rejected_points()
    p = np.concatenate([bad, p[:1500], bad, p[1500:], _blob(5, 10, 40.0, (100.0, 100.0, 100.0)), bad])
    ref = _check(gpu_ctx, p, 8)
    assert ref.stats[1] == 3 * len(bad) and ref.stats[3] > 2000 and ref.stats[2] >= 5
    assert (ref.keep[:len(bad)] == 0).all() and (ref.v[:len(bad)] == R.NO_SCORE).all()


@pytest.fixture(scope="module")
def walls():
    p, _ = R.walls(2)
    p = np.concatenate([p[:2000], R.rejected_points(0.2)])
    return p, R.run(p, 16, 1.0, 0.2, 4)


@pytest.mark.parametrize("how", ["host_twice", "device", "permuted"])
def test_same_bytes_however_it_arrives(gpu_ctx, walls, how):
    import torch
    import lmono_amd
    p, ref = walls
    f = lmono_amd.OutlierFilter(gpu_ctx, 4096, 16, 1.0, 0.2, 4)
    if how == "host_twice":
        _assert_equal(f, ref, f.filter(p))
        small = _blob(300, 12, 0.2)
        _assert_equal(f, R.run(small, 16, 1.0, 0.2, 4), f.filter(small))   # the same handle, another cloud in between
        _assert_equal(f, ref, f.filter(p))
    elif how == "device":
        d = torch.from_numpy(p.view(np.uint8).copy()).to("cuda:0")
        torch.cuda.synchronize()
        _assert_equal(f, ref, f.filter_d(d.data_ptr(), len(p)))
    else:
        perm = np.random.default_rng(3).permutation(len(p))
        f.filter(p[perm])
        keep, v = f.scores()
        assert f.stats.tolist() == ref.stats.tolist() and f.threshold().tobytes() == np.array([ref.mean, ref.sd, ref.thr]).tobytes()
        assert (keep == ref.keep[perm]).all() and (v == ref.v[perm]).all()
        assert f.cloud().tobytes() == p[perm][ref.keep[perm].astype(bool)].tobytes()
    f.close()


def _camera(w, h):
    import lmono_amd
    s = w / 1241.0
    return lmono_amd.Camera(w, h, 718.856 * s, 718.856 * s, 607.1928 * s, h / 2.0, 0, 0, 0, 0, 5, 0, 0)


def _builders(gpu_ctx, sizes, empty=()):
    import torch
    import lmono_amd
    M = CC.lidar_to_camera()
    q, t = np.array([0.0, 0.0, 0.0, 1.0]), np.array([1.0, 2.0, 3.0])
    clouds = [CC.random_cloud(20000, seed=w * 1000 + h + 7 * s, zmax=30.0) for s, (w, h) in enumerate(sizes)]
    for s in empty:
        clouds[s] = clouds[s][:0]
    images = [CC.noise_image(h, w, seed=w + s) for s, (w, h) in enumerate(sizes)]
    mbs = [lmono_amd.MapBuilder(gpu_ctx, _camera(w, h), max_cloud_points=16, map_capacity_points=2 * w * h) for w, h in sizes]
    dc = [torch.from_numpy(c).to("cuda:0") for c in clouds]; di = [torch.from_numpy(i).to("cuda:0") for i in images]
    torch.cuda.synchronize()
    n = lmono_amd.MapBuilder.associate_batch(gpu_ctx, mbs, [x.data_ptr() if len(c) else 0 for x, c in zip(dc, clouds)], [len(c) for c in clouds], [M] * len(sizes),
                                             [x.data_ptr() for x in di], [q] * len(sizes), [t] * len(sizes))
    return mbs, n


def test_a_batch_of_five_filters_equals_their_single_runs(gpu_ctx):
    import lmono_amd
    sizes = [(64, 32), (65, 33), (64, 32), (65, 33), (64, 32)]
    params = [(4, 1.0, 0.5, 8), (8, 0.5, 1.0, 6), (16, 1.0, 2.0, 4), (3, 2.0, 0.7, 8), (6, 0.0, 1.5, 5)]
    mbs, n = _builders(gpu_ctx, sizes, empty=(2,))
    assert n[2] == 0 and min(n[s] for s in (0, 1, 3, 4)) > 500
    fs = [lmono_amd.OutlierFilter(gpu_ctx, w * h, *pr) for (w, h), pr in zip(sizes, params)]
    stats = lmono_amd.OutlierFilter.filter_frames(fs, mbs)
    for s in range(5):
        world = mbs[s].cloud(1)
        ref = R.run(world, *params[s])
        _assert_equal(fs[s], ref, stats[s])
        if s != 2:
            assert ref.stats[3] > 100 and 0 < ref.stats[4]                 # on the restatement: the stream is not all isolated
        alone = lmono_amd.OutlierFilter(gpu_ctx, sizes[s][0] * sizes[s][1], *params[s])
        _assert_equal(alone, ref, lmono_amd.OutlierFilter.filter_frames([alone], [mbs[s]])[0])
        alone.close()
    assert stats[2].tolist() == [0] * 8 and len(fs[2].cloud()) == 0
    for a, b in (([fs[0], fs[0]], mbs[:2]), (fs[:2], [mbs[0], mbs[0]])):
        with pytest.raises(lmono_amd.LmonoError) as e:
            lmono_amd.OutlierFilter.filter_frames(a, b)
        assert e.value.code == EINVAL
    mbs[0].clear()                                                         # its last world cloud left with rgb_map
    with pytest.raises(lmono_amd.LmonoError) as e:
        lmono_amd.OutlierFilter.filter_frames(fs[:1], mbs[:1])
    assert e.value.code == EINVAL
    for x in fs + mbs:
        x.close()


def _moving_frame(k, w, h):
    cloud = CC.s1_scan(n_rings=32, n_az=600, k=k)
    bgr = CC.noise_image(h, w, seed=100 + k)
    q = np.round(np.array([0.01 * k, -0.02, np.sin(0.05 * k), np.cos(0.05 * k)]), 6)
    return cloud, bgr, q, np.round(np.array([0.8 * k, 0.1 * k, 0.02 * k]), 6)


def test_the_chain_builder_filter_voxel_map(gpu_ctx):
    """Two frames: MapBuilder -> filter_frames -> insert_filtered equals sor_ref + voxel_map_ref over the builder's clouds; insert_frames next
    to it still gives the unfiltered map; a full map refuses insert_filtered as it refuses insert_frames."""
    import lmono_amd
    w, h = 64, 32
    M = CC.lidar_to_camera()
    params = (8, 1.0, 0.5, 8)
    mb = lmono_amd.MapBuilder(gpu_ctx, _camera(w, h), max_cloud_points=1 << 16, map_capacity_points=4 * w * h)
    f = lmono_amd.OutlierFilter(gpu_ctx, w * h, *params)
    vm, plain, tiny = (lmono_amd.VoxelMap(gpu_ctx, leaf=0.5, max_voxels=mv) for mv in (1 << 14, 1 << 14, 2))
    want, want_plain = VR.VoxelMapRef(0.5), VR.VoxelMapRef(0.5)
    for k in range(2):
        cloud, bgr, q, t = _moving_frame(k, w, h)
        assert mb.associate(cloud, M, bgr, q, t) > 500
        world = mb.cloud(1)
        ref = R.run(world, *params)
        assert 100 < ref.stats[4] < len(world)                             # on the restatement: the filter removes some and keeps some
        stats = lmono_amd.OutlierFilter.filter_frames([f], [mb])
        _assert_equal(f, ref, stats[0])
        vstats = lmono_amd.VoxelMap.insert_filtered([vm], [f])
        lmono_amd.VoxelMap.insert_frames(gpu_ctx, [plain], [mb])
        want.insert(ref.cloud); want_plain.insert(world)
        assert vstats[0][0] + vstats[0][1] == ref.stats[4] and vstats[0][3] == len(want.table)
    for got, exp in ((vm, want), (plain, want_plain)):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got.cells(), exp.cells())) and got.read().tobytes() == exp.read().tobytes()
    assert len(want.table) < len(want_plain.table)
    with pytest.raises(lmono_amd.LmonoError) as e:
        lmono_amd.VoxelMap.insert_filtered([tiny], [f])
    assert e.value.code == ECAPACITY and tiny.size == 0
    with pytest.raises(lmono_amd.LmonoError) as e:
        lmono_amd.VoxelMap.insert_filtered([vm, vm], [f, f])
    assert e.value.code == EINVAL
    for x in (f, vm, plain, tiny, mb):
        x.close()


def test_errors(gpu_ctx):
    import lmono_amd
    good = dict(max_points=100, mean_k=8, stddev_mul=1.0, cell=0.1, max_rings=8)
    bad = [dict(max_points=0), dict(max_points=(1 << 28) + 1), dict(mean_k=0), dict(mean_k=129), dict(stddev_mul=float("nan")), dict(stddev_mul=float("inf")),
           dict(cell=0.0), dict(cell=-0.1), dict(cell=float("nan")), dict(cell=float("inf")), dict(max_rings=0), dict(max_rings=65),
           dict(cell=4.1, max_rings=63)]                                    # rho = 62.75 * 4.1 > 256
    for b in bad:
        with pytest.raises(lmono_amd.LmonoError):
            lmono_amd.OutlierFilter(gpu_ctx, **dict(good, **b))
    lmono_amd.OutlierFilter(gpu_ctx, **dict(good, cell=4.0, max_rings=64)).close()      # rho = 255: accepted
    f = lmono_amd.OutlierFilter(gpu_ctx, **good)
    p = _blob(101, 1)
    with pytest.raises(lmono_amd.LmonoError) as e:
        f.filter(p)
    assert e.value.code == ECAPACITY
    ref = R.run(p[:100], 8)
    _assert_equal(f, ref, f.filter(p[:100]))                               # exactly max_points fit
    f.close()


def test_cpp_map_build_filters_in_front_of_the_voxel_map(gpu_ctx, tmp_path):
    """map_build ... sor=16:1.0 voxel=0.1 writes rgb_map_voxel.ply, equal to the Python chain's read() over the same frames."""
    import lmono_amd
    from lmono_amd import kitti_io as IO
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lmono_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "map_build"])
    w, h, n = 320, 96, 3
    fx = fy = 185.0; cx = 156.5; cy = 47.25
    seq = tmp_path / "seq"; out = tmp_path / "out"
    os.makedirs(seq / "velodyne"); os.makedirs(seq / "image_bgr"); os.makedirs(out)
    M = CC.lidar_to_camera()
    mb = lmono_amd.MapBuilder(gpu_ctx, lmono_amd.Camera(w, h, fx, fy, cx, cy, 0, 0, 0, 0, 5, 0, 0), max_cloud_points=1 << 16)
    f = lmono_amd.OutlierFilter(gpu_ctx, w * h, 16, 1.0)
    vm, plain = (lmono_amd.VoxelMap(gpu_ctx, leaf=0.1, max_voxels=1 << 18) for _ in range(2))
    qt = np.zeros((n, 7))
    kept = 0
    for k in range(n):
        cloud, bgr, q, t = _moving_frame(k, w, h)
        IO.write_velodyne_bin(IO.velodyne_path(str(seq), k), cloud)
        (seq / "image_bgr" / ("%06d.bgr" % k)).write_bytes(bgr.tobytes())
        qt[k, :4] = q; qt[k, 4:] = t
        mb.associate(cloud, M, bgr, q, t)
        kept += int(lmono_amd.OutlierFilter.filter_frames([f], [mb])[0][4])
        lmono_amd.VoxelMap.insert_filtered([vm], [f])
        plain.insert_frame(mb)
    IO.write_trajectory(str(tmp_path / "traj.txt"), 50.0 + 0.1 * np.arange(n), qt)
    subprocess.check_output([os.path.join(host, "map_build"), str(seq), str(tmp_path / "traj.txt"), str(out), str(n), str(w), str(h),
                             repr(fx), repr(fy), repr(cx), repr(cy), "sor=16:1.0", "voxel=0.1:%d" % (1 << 18)], text=True)
    ply = IO.read_ply_binary(str(out / "rgb_map_voxel.ply"))
    want = vm.read()
    assert kept > 1000 and 100 < len(want) < plain.size and ply.tobytes() == want.tobytes()
    for x in (f, vm, plain, mb):
        x.close()
