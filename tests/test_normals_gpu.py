"""The surface normals on the GPU (lmono_normals_*) against the numpy restatement of their definition (tests/normals_ref.py, brute
force over all pairs): records, counts and stats as bytes, for every shape at which the search or the sums could go wrong and every way the same
points can arrive.  A NaN's sign and payload are not part of the definition: NaNs compare as NaNs."""
import functools

import numpy as np
import pytest

from tests import normals_cases as NC
from tests import normals_ref as R
from tests.test_normals_ref_cpu import tuned_cell

pytestmark = pytest.mark.gpu

ECAPACITY, EINVAL = -4, -1


@functools.lru_cache(maxsize=None)
def _case(name):
    p, kw = NC.CASES[name]()
    return p, kw, R.run(p, **kw)


def _handle(gpu_ctx, n, kw):
    import lmono_amd
    return lmono_amd.SurfaceNormals(gpu_ctx, max(n, 1), **{k: v for k, v in kw.items() if k != "viewpoint"})


def _assert_equal(s, ref, stats=None, order=None):
    """order: the rows of ref that the handle's rows correspond to."""
    rec, cnt = s.read()
    want_rec, want_cnt = (ref.records, ref.counts) if order is None else (ref.records[order], ref.counts[order])
    if stats is not None:
        assert stats.tolist() == ref.stats.tolist()
    assert s.stats.tolist() == ref.stats.tolist()
    assert cnt.dtype == np.uint32 and cnt.tobytes() == want_cnt.tobytes()
    assert R.canon(R.records_of(rec)) == R.canon(want_rec)


def _check(gpu_ctx, p, kw, ref):
    s = _handle(gpu_ctx, len(p), kw)
    _assert_equal(s, ref, s.compute(p, kw.get("viewpoint")))
    assert s.cloud().tobytes() == p.tobytes()
    s.close()


@pytest.mark.parametrize("name", sorted(NC.CASES))
def test_every_case_equals_the_restatement(gpu_ctx, name):
    """What each case is, and that it is that, is checked on the restatement in tests/test_normals_ref_cpu.py."""
    p, kw, ref = _case(name)
    _check(gpu_ctx, p, kw, ref)


@pytest.mark.parametrize("name", ["tilted_plane_far", "dense_cell", "invalid_and_span", "sphere_out"])
def test_a_permutation_permutes_the_records(gpu_ctx, name):
    p, kw, ref = _case(name)
    perm = np.random.default_rng(6).permutation(len(p))
    s = _handle(gpu_ctx, len(p), kw)
    _assert_equal(s, ref, s.compute(p[perm], kw.get("viewpoint")), order=perm)
    s.close()


@pytest.mark.parametrize("name", ["tilted_plane", "dense_cell", "ring_edge"])
@pytest.mark.parametrize("div,rings", [(0.75, 1), (1.75, 2), (3.75, 4)])
def test_grid_tuning_changes_no_byte(gpu_ctx, name, div, rings):
    p, kw, ref = _case(name)
    _check(gpu_ctx, p, dict(kw, cell=float(tuned_cell(kw["radius"], div, rings)), max_rings=rings), ref)


def test_device_pointers_and_a_second_compute_replaces_the_first(gpu_ctx):
    import torch
    p, kw, ref = _case("tail_1000")
    p2, kw2, ref2 = _case("tail_257")
    assert kw["radius"] == kw2["radius"]
    s = _handle(gpu_ctx, 1000, kw)
    d = torch.from_numpy(p.view(np.uint8).reshape(-1, 16).copy()).to("cuda:0")
    torch.cuda.synchronize()
    _assert_equal(s, ref, s.compute_d(d.data_ptr(), len(p), kw["viewpoint"]))
    assert s.cloud().tobytes() == p.tobytes()
    _assert_equal(s, ref2, s.compute(p2))                                 # a smaller cloud, no viewpoint: nothing of the first result is left
    assert s.cloud().tobytes() == p2.tobytes() and len(s.read()[0]) == 257
    _assert_equal(s, ref, s.compute_d(d.data_ptr(), len(p), kw["viewpoint"]))
    s.close()


def test_a_batch_of_three_equals_their_single_runs(gpu_ctx):
    """Three streams of different sizes from three builders, one empty, each with its own radius, minimum, grid and viewpoint."""
    import lmono_amd
    from tests.test_sor_gpu import _builders
    sizes = [(64, 32), (65, 33), (64, 32)]
    params = [dict(radius=2.0), dict(radius=1.0, min_neighbours=4), dict(radius=3.0, min_neighbours=5, cell=1.0, max_rings=4)]
    vps = np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [-5.0, 40.0, 2.5]], np.float32)
    mbs, n = _builders(gpu_ctx, sizes, empty=(1,))
    assert n[1] == 0 and min(n[0], n[2]) > 500
    worlds = [mb.cloud(1) for mb in mbs]
    hs = [_handle(gpu_ctx, w * h, pr) for (w, h), pr in zip(sizes, params)]
    stats = lmono_amd.SurfaceNormals.compute_frames(hs, mbs, vps)
    refs = [R.run(w, viewpoint=v, **pr) for w, v, pr in zip(worlds, vps, params)]
    assert refs[0].stats[2] > 50 and refs[2].stats[2] > 50 and refs[1].stats.tolist() == [0] * 8      # on the restatement
    for s in range(3):
        _assert_equal(hs[s], refs[s], stats[s])
        assert hs[s].cloud().tobytes() == worlds[s].tobytes()
        alone = _handle(gpu_ctx, sizes[s][0] * sizes[s][1], params[s])
        _assert_equal(alone, refs[s], lmono_amd.SurfaceNormals.compute_frames([alone], [mbs[s]], vps[s])[0])
        _assert_equal(alone, refs[s], alone.compute(worlds[s], vps[s]))
        alone.close()
    plain = R.run(worlds[0], **params[0])                                  # without viewpoints: the canonical sign
    assert R.canon(plain.records) != R.canon(refs[0].records)
    _assert_equal(hs[0], plain, lmono_amd.SurfaceNormals.compute_frames(hs[:1], mbs[:1])[0])
    other = lmono_amd.Context(0)
    foreign = lmono_amd.SurfaceNormals(other, 64 * 32, radius=2.0)
    for a, b in (([hs[0], hs[0]], mbs[:2]), (hs[:2], [mbs[0], mbs[0]]), ([hs[0], foreign], mbs[:2])):
        with pytest.raises(lmono_amd.LmonoError) as e:
            lmono_amd.SurfaceNormals.compute_frames(a, b)
        assert e.value.code == EINVAL
    small = lmono_amd.SurfaceNormals(gpu_ctx, n[0] - 1, radius=2.0)
    with pytest.raises(lmono_amd.LmonoError) as e:
        lmono_amd.SurfaceNormals.compute_frames([small], [mbs[0]])
    assert e.value.code == ECAPACITY
    mbs[0].clear()                                                         # its last world cloud left with rgb_map
    with pytest.raises(lmono_amd.LmonoError) as e:
        lmono_amd.SurfaceNormals.compute_frames(hs[:1], mbs[:1])
    assert e.value.code == EINVAL
    _assert_equal(hs[0], plain)                                            # refused before any launch: the last result stands
    foreign.close(); other.close()
    for x in hs + mbs + [small]:
        x.close()


def _by_point(p):
    return np.lexsort((p["bgra"], p["z"], p["y"], p["x"]))


def test_the_points_of_a_voxel_map(gpu_ctx):
    """compute_map takes one point per occupied voxel in the device's order: cloud() is VoxelMap.read() as a set, and the records are the
    restatement's on cloud()'s points."""
    import lmono_amd
    p, _, _ = _case("sphere_in")
    kw = dict(radius=0.3, viewpoint=tuple(NC.SPHERE_CENTRE))
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=0.1, max_voxels=1 << 12)
    vm.insert(p)
    want = vm.read()
    assert 500 < len(want) <= len(p)
    s = _handle(gpu_ctx, len(p), kw)
    stats = s.compute_map(vm, kw["viewpoint"])
    cloud = s.cloud()
    assert cloud[_by_point(cloud)].tobytes() == want[_by_point(want)].tobytes()
    ref = R.run(cloud, **kw)
    assert ref.stats[2] == len(cloud)
    _assert_equal(s, ref, stats)
    sorted_ref = R.run(want, **kw)                                         # the same set in read()'s order: the same records, point by point
    back = np.empty(len(want), np.int64); back[_by_point(want)] = _by_point(cloud)
    assert R.canon(R.records_of(s.read()[0])[back]) == R.canon(sorted_ref.records)
    small = _handle(gpu_ctx, len(want) - 1, kw)
    with pytest.raises(lmono_amd.LmonoError) as e:
        small.compute_map(vm)
    assert e.value.code == ECAPACITY
    empty = lmono_amd.VoxelMap(gpu_ctx, leaf=0.1, max_voxels=16)
    assert small.compute_map(empty).tolist() == [0] * 8 and len(small.cloud()) == 0 and len(small.read()[0]) == 0
    for x in (s, small, vm, empty):
        x.close()


def test_refusals(gpu_ctx):
    import lmono_amd
    good = dict(max_points=100, radius=0.5, min_neighbours=3, cell=0.3, max_rings=2)
    bad = [dict(max_points=0), dict(max_points=(1 << 26) + 1), dict(radius=0.0), dict(radius=-1.0), dict(radius=4.5, cell=4.0), dict(radius=float("nan")),
           dict(min_neighbours=2), dict(cell=0.0), dict(cell=-0.3), dict(cell=float("nan")), dict(cell=float("inf")), dict(max_rings=0), dict(max_rings=65),
           dict(cell=0.28, max_rings=2)]                                # rho = 1.75 * 0.28 = 0.49 < radius
    for b in bad:
        with pytest.raises(lmono_amd.LmonoError):
            lmono_amd.SurfaceNormals(gpu_ctx, **dict(good, **b))
    lmono_amd.SurfaceNormals(gpu_ctx, **dict(good, radius=4.0, cell=4.0)).close()
    for r in [0.05, 0.95, 1.9, 3.8, 1e-3, 4.0] + np.random.default_rng(15).uniform(0.0, 4.0, 30).astype(np.float32).tolist():
        lmono_amd.SurfaceNormals(gpu_ctx, 16, radius=float(r)).close()             # the default cell is accepted for every radius
    s = lmono_amd.SurfaceNormals(gpu_ctx, **good)
    p = NC.pts(np.random.default_rng(16).uniform(-1.0, 1.0, (101, 3)), 16)
    ref = R.run(p[:100], **{k: v for k, v in good.items() if k != "max_points"})
    _assert_equal(s, ref, s.compute(p[:100]))                             # exactly max_points fit
    with pytest.raises(lmono_amd.LmonoError) as e:
        s.compute(p)
    assert e.value.code == ECAPACITY
    _assert_equal(s, ref)                                                 # refused before any launch: the last result stands
    assert s.compute(p[:0]).tolist() == [0] * 8 and len(s.read()[0]) == 0 and len(s.read()[1]) == 0 and len(s.cloud()) == 0      # n == 0 replaces it
    with pytest.raises(lmono_amd.LmonoError) as e:
        s.compute(p[:10], (np.nan, 0.0, 0.0))
    assert e.value.code == EINVAL
    other = lmono_amd.Context(0)
    L = gpu_ctx.L
    assert L.lmono_normals_compute(other.h, s.h, p.ctypes.data, 10, None, None) == EINVAL          # a foreign handle
    assert L.lmono_normals_compute(gpu_ctx.h, None, p.ctypes.data, 10, None, None) == EINVAL
    assert L.lmono_normals_read(gpu_ctx.h, None, None, None, 0) == EINVAL
    assert L.lmono_normals_cloud(other.h, s.h, None, 0) == EINVAL
    other.close()
    s.close()
