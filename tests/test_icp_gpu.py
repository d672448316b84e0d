"""The point-to-point ICP on the GPU (lmono_icp_*) against the numpy restatement of its definition (tests/icp_ref.py, brute force
over all pairs): the transform, stats, history, distances and the aligned cloud as bytes, for every shape at which the search or the sums could go
wrong and every way the same points can arrive.  A NaN's sign and payload are not part of the definition: NaNs compare as NaNs."""
import functools

import numpy as np
import pytest

from tests import icp_cases as IC
from tests import icp_ref as R
from tests import voxel_map_ref as VR

pytestmark = pytest.mark.gpu

ECAPACITY, EINVAL = -4, -1


@functools.lru_cache(maxsize=None)
def _case(name):
    tgt, src, kw = IC.CASES[name]()
    return tgt, src, kw, R.run(tgt, src, **kw)


def _aligner(gpu_ctx, n_src, n_tgt, kw):
    import lmono_amd
    a = lmono_amd.CloudAligner(gpu_ctx, max(n_src, 1), max(n_tgt, 1), **{k: v for k, v in kw.items() if k != "guess"})
    if kw.get("guess") is not None:
        a.set_guess(kw["guess"])
    return a


def _assert_equal(a, ref, stats=None):
    if stats is not None:
        assert stats.tolist() == ref.stats.tolist()
    assert a.stats.tolist() == ref.stats.tolist()
    assert a.transform().tobytes() == ref.transform.tobytes()
    assert a.history().tolist() == ref.history.tolist()
    assert R.canon(a.distances()) == R.canon(ref.d2)
    assert R.cloud_bytes(a.cloud()) == R.cloud_bytes(ref.cloud)


def _check(gpu_ctx, tgt, src, kw, ref):
    a = _aligner(gpu_ctx, len(src), len(tgt), kw)
    a.set_target(tgt)
    _assert_equal(a, ref, a.align(src))
    a.close()


@pytest.mark.parametrize("name", sorted(IC.CASES))
def test_every_case_equals_the_restatement(gpu_ctx, name):
    """Smallest shapes, the D bound, ties, a target point given 40 times, the stopping sets, a dense cell, invalid and out-of-span points, a guess,
    2000 x 2000 points away from the origin: what each case is, and that it is that, is checked on the restatement in tests/test_icp_ref_cpu.py."""
    tgt, src, kw, ref = _case(name)
    _check(gpu_ctx, tgt, src, kw, ref)


@pytest.mark.parametrize("name", ["phys3_origin", "far_2000", "dense_cell"])
@pytest.mark.parametrize("div,rings", [(0.75, 1), (1.75, 2), (3.75, 4)])
def test_grid_tuning_changes_no_byte(gpu_ctx, name, div, rings):
    tgt, src, kw, ref = _case(name)
    cell = np.float32(kw.get("max_corr", 0.5)) / np.float32(div)
    tuned = R.run(tgt, src, **dict(kw, cell=cell, max_rings=rings))
    assert tuned.transform.tobytes() == ref.transform.tobytes() and tuned.cloud.tobytes() == ref.cloud.tobytes()      # on the restatement
    _check(gpu_ctx, tgt, src, dict(kw, cell=float(cell), max_rings=rings), ref)


def test_order_of_target_and_source(gpu_ctx):
    tgt, src, kw, ref = _case("far_2000")
    rng = np.random.default_rng(5)
    pt, ps = rng.permutation(len(tgt)), rng.permutation(len(src))
    a = _aligner(gpu_ctx, len(src), len(tgt), kw)
    a.set_target(tgt[pt])
    stats = a.align(src[ps])
    assert stats.tolist() == ref.stats.tolist() and a.transform().tobytes() == ref.transform.tobytes() and a.history().tolist() == ref.history.tolist()
    assert a.cloud().tobytes() == ref.cloud[ps].tobytes() and a.distances().tobytes() == ref.d2[ps].tobytes()
    a.close()


def test_poll_interval_changes_no_byte(gpu_ctx):
    for name in ("eps0", "phys3_origin"):
        tgt, src, kw, ref = _case(name)
        for pairs in (1, 7):
            a = _aligner(gpu_ctx, len(src), len(tgt), kw)
            a.set_poll_interval(pairs)
            a.set_target(tgt)
            _assert_equal(a, ref, a.align(src))
            a.close()


def test_a_target_serves_many_aligns_and_device_pointers(gpu_ctx):
    import torch
    tgt, src, kw, ref = _case("phys3_origin")
    tgt2, src2, kw2, ref2 = _case("phys_origin")
    a = _aligner(gpu_ctx, 400, 400, kw)
    dt = torch.from_numpy(tgt.view(np.uint8).reshape(-1, 16).copy()).to("cuda:0"); ds = torch.from_numpy(src2.view(np.uint8).reshape(-1, 16).copy()).to("cuda:0")
    torch.cuda.synchronize()
    a.set_target_d(dt.data_ptr(), len(tgt))
    _assert_equal(a, ref, a.align(src))
    _assert_equal(a, ref2, a.align_d(ds.data_ptr(), len(src2)))       # phys_origin has the same target
    _assert_equal(a, ref, a.align(src))
    a.close()


def test_voxel_map_and_aligned_cloud_as_targets(gpu_ctx):
    import lmono_amd
    tgt, src, kw, _ = _case("far_2000")
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=0.1, max_voxels=1 << 12)
    vm.insert(tgt)
    cloud = vm.read()
    assert 1000 < len(cloud) <= len(tgt)
    ref = R.run(cloud, src, **kw)
    a = _aligner(gpu_ctx, len(src), len(tgt), kw)
    a.set_target_map(vm)
    _assert_equal(a, ref, a.align(src))
    a.set_target(cloud)
    _assert_equal(a, ref, a.align(src))
    # the aligned cloud as the next target ("last cloud")
    src2 = IC.moved_blob(2000, 10, at=(-41.3, -77.7, -3.1), span=4.0, deg=2.5)[1]
    ref2 = R.run(ref.cloud, src2, **kw)
    a.set_target_aligned()
    _assert_equal(a, ref2, a.align(src2))
    small = _aligner(gpu_ctx, 10, len(cloud) - 1, kw)
    with pytest.raises(lmono_amd.LmonoError) as e:
        small.set_target_map(vm)
    assert e.value.code == ECAPACITY
    with pytest.raises(lmono_amd.LmonoError) as e:
        small.set_target_aligned()                                       # no align has run
    assert e.value.code == EINVAL
    empty = lmono_amd.VoxelMap(gpu_ctx, leaf=0.1, max_voxels=16)
    small.set_target_map(empty)
    assert small.align(src[:10]).tolist()[4:] == [1, 3, 0, 0]
    for x in (a, small, vm, empty):
        x.close()


def test_a_batch_of_five_aligners_equals_their_single_runs(gpu_ctx):
    """Five streams of different sizes from five builders, one empty; stream 1 ends at its second iteration (mse_eps = 1, eps = 0) while stream 3 runs to
    max_iter (eps = 0)."""
    import lmono_amd
    from tests.test_sor_gpu import _builders
    sizes = [(64, 32), (65, 33), (64, 32), (65, 33), (64, 32)]
    params = [dict(max_corr=1.0), dict(max_corr=1.0, eps=0.0, mse_eps=1.0), dict(max_corr=0.5), dict(max_corr=2.0, eps=0.0, max_iter=7, cell=1.0, max_rings=3), dict(max_corr=1.0, max_iter=3)]
    mbs, n = _builders(gpu_ctx, sizes, empty=(2,))
    assert n[2] == 0 and min(n[s] for s in (0, 1, 3, 4)) > 500
    worlds = [mb.cloud(1) for mb in mbs]
    move = IC.rotation((0.2, 0.1, 0.9), 0.4)
    targets = []
    for s, w in enumerate(worlds):
        src_w = worlds[(s + 1) % 5] if len(w) == 0 else w
        xyz = np.stack([src_w[a] for a in "xyz"], 1).astype(np.float64)
        targets.append(IC.pts((xyz - xyz.mean(0)) @ move.T + xyz.mean(0) + np.array([0.05, -0.03, 0.02]), s))
    al = [_aligner(gpu_ctx, w * h, 65 * 33, pr) for (w, h), pr in zip(sizes, params)]      # the empty stream's target comes from its larger neighbour
    for a, t in zip(al, targets):
        a.set_target(t)
    stats = lmono_amd.CloudAligner.align_frames(al, mbs)
    refs = [R.run(t, w, **pr) for t, w, pr in zip(targets, worlds, params)]
    assert refs[1].stats.tolist()[4:6] == [2, 2] and refs[3].stats.tolist()[4:6] == [7, 1] and refs[2].stats.tolist()[4:6] == [0, 3]      # on the restatement
    assert min(refs[s].N for s in (0, 1, 3, 4)) > 100
    for s in range(5):
        _assert_equal(al[s], refs[s], stats[s])
        alone = _aligner(gpu_ctx, sizes[s][0] * sizes[s][1], len(targets[s]), params[s])
        alone.set_target(targets[s])
        _assert_equal(alone, refs[s], lmono_amd.CloudAligner.align_frames([alone], [mbs[s]])[0])
        alone.close()
    for a, b in (([al[0], al[0]], mbs[:2]), (al[:2], [mbs[0], mbs[0]])):
        with pytest.raises(lmono_amd.LmonoError) as e:
            lmono_amd.CloudAligner.align_frames(a, b)
        assert e.value.code == EINVAL
    for x in al + mbs:
        x.close()


def test_the_chain_builder_filter_aligner_voxel_map(gpu_ctx):
    """Two frames: MapBuilder -> filter_frames -> align_filtered against the voxel map -> insert_aligned.  The map holds what insert(aligner.cloud())
    gives, and the colour sums of the filtered frames."""
    import lmono_amd
    from tests.test_sor_gpu import _camera, _moving_frame
    from tests import colour_cases as CC
    from tests import sor_ref as SR
    w, h = 64, 32
    M = CC.lidar_to_camera()
    sor_params = (8, 1.0, 0.5, 8)
    kw = dict(max_corr=0.5, max_iter=5)
    mb = lmono_amd.MapBuilder(gpu_ctx, _camera(w, h), max_cloud_points=1 << 16, map_capacity_points=4 * w * h)
    f = lmono_amd.OutlierFilter(gpu_ctx, w * h, *sor_params)
    a = _aligner(gpu_ctx, w * h, 1 << 14, kw)
    vm, by_host = (lmono_amd.VoxelMap(gpu_ctx, leaf=0.5, max_voxels=1 << 14) for _ in range(2))
    want = VR.VoxelMapRef(0.5)
    colour = np.zeros(3, np.int64)
    for k in range(2):
        cloud, bgr, q, t = _moving_frame(k, w, h)
        assert mb.associate(cloud, M, bgr, q, t) > 500
        lmono_amd.OutlierFilter.filter_frames([f], [mb])
        kept = SR.run(mb.cloud(1), *sor_params).cloud
        assert f.cloud().tobytes() == kept.tobytes() and len(kept) > 100
        if k == 0:
            lmono_amd.VoxelMap.insert_filtered([vm], [f])            # the first frame has no target and is inserted as it is
            by_host.insert(kept); want.insert(kept)
        else:
            a.set_target_map(vm)
            ref = R.run(want.read(), kept, **kw)
            _assert_equal(a, ref, lmono_amd.CloudAligner.align_filtered([a], [f])[0])
            vstats = lmono_amd.VoxelMap.insert_aligned([vm], [a])
            by_host.insert(a.cloud()); want.insert(ref.cloud)
            assert vstats[0][0] + vstats[0][1] == len(kept) and vstats[0][1] == 0 and vstats[0][3] == len(want.table)
        colour += np.array([int(((kept["bgra"] >> sh) & 0xFF).sum()) for sh in (16, 8, 0)], np.int64)
    for got in (vm, by_host):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got.cells(), want.cells())) and got.read().tobytes() == want.read().tobytes()
    assert vm.cells()[2][:, 3:].sum(0).astype(np.int64).tolist() == colour.tolist()
    with pytest.raises(lmono_amd.LmonoError) as e:
        lmono_amd.VoxelMap.insert_aligned([vm, vm], [a, a])
    assert e.value.code == EINVAL
    for x in (a, f, vm, by_host, mb):
        x.close()


def test_the_default_grid_is_accepted_for_every_max_corr(gpu_ctx):
    """At defaults (cell from lmono_icp_default_cell, 2 rings) create accepts every max_corr in (0, 16], 0.95, 1.9 and 3.8 among them, for which
    max_corr / 1.75 in float32 misses the bound by an ulp; and an align at such a max_corr equals the restatement."""
    import lmono_amd
    sweep = [0.95, 1.9, 3.8, 1e-3, 0.01, 16.0] + np.random.default_rng(12).uniform(0.0, 16.0, 60).astype(np.float32).tolist()
    for D in sweep:
        lmono_amd.CloudAligner(gpu_ctx, 16, 16, max_corr=float(D)).close()
    tgt, src, _, _ = _case("phys_origin")
    for D in (0.95, 1.9):
        kw = dict(max_corr=D, max_iter=4)
        _check(gpu_ctx, tgt, src, kw, R.run(tgt, src, **kw))


def test_refusals(gpu_ctx):
    import lmono_amd
    good = dict(max_source_points=100, max_target_points=100, max_corr=0.5, max_iter=50, eps=1e-8, mse_eps=0.0, cell=0.3, max_rings=2)
    bad = [dict(max_source_points=0), dict(max_source_points=(1 << 28) + 1), dict(max_target_points=0), dict(max_target_points=(1 << 28) + 1), dict(max_corr=0.0), dict(max_corr=-1.0),
           dict(max_corr=16.5, cell=10.0), dict(max_corr=float("nan")), dict(max_iter=0), dict(max_iter=65537), dict(eps=-1e-9), dict(eps=float("nan")), dict(mse_eps=-1.0), dict(mse_eps=float("nan")),
           dict(cell=0.0), dict(cell=-0.3), dict(cell=float("nan")), dict(cell=float("inf")), dict(max_rings=0), dict(max_rings=65),
           dict(cell=0.28, max_rings=2)]                                # rho = 1.75 * 0.28 = 0.49 < max_corr
    for b in bad:
        with pytest.raises(lmono_amd.LmonoError):
            lmono_amd.CloudAligner(gpu_ctx, **dict(good, **b))
    lmono_amd.CloudAligner(gpu_ctx, **dict(good, max_corr=16.0, cell=16.0, max_rings=2)).close()
    lmono_amd.CloudAligner(gpu_ctx, **dict(good, max_iter=65536)).close()            # the largest history
    a = lmono_amd.CloudAligner(gpu_ctx, **good)
    tgt, src = IC.moved_blob(101, 3)
    with pytest.raises(lmono_amd.LmonoError) as e:
        a.align(src[:50])                                                # no target yet
    assert e.value.code == EINVAL
    with pytest.raises(lmono_amd.LmonoError) as e:
        a.set_target(tgt)
    assert e.value.code == ECAPACITY
    a.set_target(tgt[:100])                                              # exactly max_target_points fit
    with pytest.raises(lmono_amd.LmonoError) as e:
        a.align(src)
    assert e.value.code == ECAPACITY
    ref = R.run(tgt[:100], src[:100], **{k: v for k, v in good.items() if not k.startswith("max_s") and not k.startswith("max_t")})
    _assert_equal(a, ref, a.align(src[:100]))
    other = lmono_amd.Context(0)
    L = gpu_ctx.L
    assert L.lmono_icp_align(other.h, a.h, src.ctypes.data, 10, None) == EINVAL          # a foreign handle
    assert L.lmono_icp_align(gpu_ctx.h, None, src.ctypes.data, 10, None) == EINVAL
    assert L.lmono_icp_set_target(gpu_ctx.h, None, tgt.ctypes.data, 10) == EINVAL
    assert L.lmono_icp_transform(gpu_ctx.h, None, None) == EINVAL
    other.close()
    a.close()
