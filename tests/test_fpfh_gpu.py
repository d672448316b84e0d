"""The FPFH descriptors on the GPU (lmono_fpfh_*) against the numpy restatement of their definition (tests/fpfh_ref.py, brute force
over all pairs): descriptors, contributing points, flags and stats as bytes, for every shape at which the search or the sums could go wrong and
every way the same points can arrive.  The surface is a SurfaceNormals handle after a compute on the device; the restatement runs on the normals'
restatement, whose bytes the device's normals equal (tests/test_normals_gpu.py)."""
import numpy as np
import pytest

from tests import fpfh_cases as FC
from tests import fpfh_ref as R
from tests import normals_ref as NR
from tests.test_fpfh_ref_cpu import case, normals_of, tuned_cell

pytestmark = pytest.mark.gpu

ECAPACITY, EINVAL = -4, -1


def _normals(gpu_ctx, p, nkw):
    import lmono_amd
    s = lmono_amd.SurfaceNormals(gpu_ctx, max(len(p), 1), **{k: v for k, v in nkw.items() if k != "viewpoint"})
    s.compute(p, nkw.get("viewpoint"))
    return s


def _handle(gpu_ctx, n, m, fkw):
    import lmono_amd
    return lmono_amd.FpfhDescriptors(gpu_ctx, max(n, 1), max(m, 1), **fkw)


def _assert_equal(f, ref, stats=None, order=None):
    """order: the rows of ref that the handle's rows correspond to."""
    desc, cnt, flag = f.read()
    want = (ref.desc, ref.counts, ref.flags) if order is None else (ref.desc[order], ref.counts[order], ref.flags[order])
    if stats is not None:
        assert stats.tolist() == ref.stats.tolist()
    assert f.stats.tolist() == ref.stats.tolist()
    assert cnt.dtype == np.uint32 and cnt.tobytes() == want[1].tobytes() and flag.tobytes() == want[2].tobytes()
    assert desc.dtype == np.float32 and desc.shape == want[0].shape and R.canon(desc) == R.canon(want[0])


def _check(gpu_ctx, p, nkw, k, fkw, ref, nrm=None):
    s = nrm or _normals(gpu_ctx, p, nkw)
    f = _handle(gpu_ctx, len(p), len(k), fkw)
    _assert_equal(f, ref, f.compute(s, k))
    assert f.keypoints().tobytes() == np.ascontiguousarray(k, np.float32).tobytes()
    f.close()
    if nrm is None:
        s.close()


@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_every_case_equals_the_restatement(gpu_ctx, name):
    """What each case is, and that it is that, is checked on the restatement in tests/test_fpfh_ref_cpu.py."""
    p, nkw, k, fkw, ref = case(name)
    s = _normals(gpu_ctx, p, nkw)
    assert NR.canon(NR.records_of(s.read()[0])) == NR.canon(normals_of(name).records)          # the surface the restatement ran on
    _check(gpu_ctx, p, nkw, k, fkw, ref, s)
    s.close()


@pytest.mark.parametrize("name", ["scene", "dense_cell", "invalid_and_span", "duplicates"])
def test_a_permutation_of_the_cloud_changes_no_byte_and_one_of_the_keypoints_permutes(gpu_ctx, name):
    p, nkw, k, fkw, ref = case(name)
    perm = np.random.default_rng(6).permutation(len(p))
    _check(gpu_ctx, p[perm], nkw, k, fkw, ref)
    kperm = np.random.default_rng(7).permutation(len(k))
    s = _normals(gpu_ctx, p, nkw)
    f = _handle(gpu_ctx, len(p), len(k), fkw)
    stats = f.compute(s, k[kperm])
    assert stats.tolist() == ref.stats.tolist()
    _assert_equal(f, ref, order=kperm)
    f.close(); s.close()


@pytest.mark.parametrize("name", ["scene", "dense_cell", "keypoint_on_point"])
@pytest.mark.parametrize("div,rings", [(0.75, 1), (1.75, 2), (3.75, 4)])
def test_grid_tuning_changes_no_byte(gpu_ctx, name, div, rings):
    p, nkw, k, fkw, ref = case(name)
    _check(gpu_ctx, p, nkw, k, dict(fkw, cell=float(tuned_cell(fkw["radius"], div, rings)), max_rings=rings), ref)


@pytest.mark.parametrize("names", [("m65",), ("scene", "m0", "dense_cell"), ("m1", "scene_resampled", "keypoint_alone", "duplicates", "far_from_origin")])
def test_a_batch_equals_the_single_runs(gpu_ctx, names):
    """1, 3 and 5 streams of unequal sizes, radii and keypoint counts (one with none), one launch per phase; then two handles over one surface."""
    import lmono_amd
    cs = [case(n) for n in names]
    ns = [_normals(gpu_ctx, c[0], c[1]) for c in cs]
    fs = [_handle(gpu_ctx, len(c[0]), len(c[2]), c[3]) for c in cs]
    stats = lmono_amd.FpfhDescriptors.compute_batch(fs, ns, [c[2] for c in cs])
    for f, c, st in zip(fs, cs, stats):
        _assert_equal(f, c[4], st)
    if len(cs) == 3:
        other = R.run(cs[0][0], normals_of(names[0]).records, cs[0][2][::2], radius=0.4)
        pair = [fs[0], lmono_amd.FpfhDescriptors(gpu_ctx, len(cs[0][0]), len(cs[0][2]), radius=0.4)]
        stats = lmono_amd.FpfhDescriptors.compute_batch(pair, [ns[0], ns[0]], [cs[0][2], cs[0][2][::2]])
        _assert_equal(pair[0], cs[0][4], stats[0]); _assert_equal(pair[1], other, stats[1])
        pair[1].close()
    for x in fs + ns:
        x.close()


def test_a_second_compute_replaces_the_first(gpu_ctx):
    p, nkw, k, fkw, ref = case("keypoint_on_point")
    p2, nkw2, k2, fkw2, ref2 = case("m65")
    assert fkw == fkw2
    s, s2 = _normals(gpu_ctx, p, nkw), _normals(gpu_ctx, p2, nkw2)
    f = _handle(gpu_ctx, len(p), len(k), fkw)
    _assert_equal(f, ref, f.compute(s, k))
    _assert_equal(f, ref2, f.compute(s2, k2))                              # a smaller surface, fewer keypoints: nothing of the first result is left
    assert len(f.read()[0]) == 65
    _assert_equal(f, ref, f.compute(s, k))
    s.compute(p2, nkw2.get("viewpoint"))                                   # the surface is read at compute time: a new cloud in the same handle
    _assert_equal(f, ref2, f.compute(s, k2))
    for x in (f, s, s2):
        x.close()


def test_refusals(gpu_ctx):
    import lmono_amd
    good = dict(max_points=300, max_keypoints=70, radius=0.5, cell=0.3, max_rings=2)
    bad = [dict(max_points=0), dict(max_points=(1 << 26) + 1), dict(max_keypoints=0), dict(max_keypoints=4097), dict(radius=0.0), dict(radius=-1.0),
           dict(radius=4.5, cell=4.0), dict(radius=float("nan")), dict(cell=0.0), dict(cell=-0.3), dict(cell=float("nan")), dict(cell=float("inf")),
           dict(max_rings=0), dict(max_rings=65), dict(cell=0.28, max_rings=2)]                # rho = 1.75 * 0.28 = 0.49 < radius
    for b in bad:
        with pytest.raises(lmono_amd.LmonoError) as e:
            lmono_amd.FpfhDescriptors(gpu_ctx, **dict(good, **b))
        assert "max_keypoints in 1 .. 4096" in str(e.value) and "0 < radius <= 4" in str(e.value)          # the message names the bounds
    lmono_amd.FpfhDescriptors(gpu_ctx, **dict(good, radius=4.0, cell=4.0, max_keypoints=4096)).close()
    p, nkw, k, fkw, ref = case("m65")
    f = lmono_amd.FpfhDescriptors(gpu_ctx, len(p), 65, **fkw)
    s = _normals(gpu_ctx, p, nkw)
    _assert_equal(f, ref, f.compute(s, k))                                 # exactly max_points and max_keypoints fit
    fresh = lmono_amd.SurfaceNormals(gpu_ctx, 300, radius=0.3)
    with pytest.raises(lmono_amd.LmonoError) as e:
        f.compute(fresh, k)                                                # a normals handle without a result
    assert e.value.code == EINVAL
    with pytest.raises(lmono_amd.LmonoError) as e:
        f.compute(s, np.concatenate([k, k[:1]]))
    assert e.value.code == ECAPACITY
    for v in (np.nan, np.inf, -np.inf):
        kb = k.copy(); kb[7, 1] = v
        with pytest.raises(lmono_amd.LmonoError) as e:
            f.compute(s, kb)
        assert e.value.code == EINVAL
    small = lmono_amd.FpfhDescriptors(gpu_ctx, len(p) - 1, 65, **fkw)
    with pytest.raises(lmono_amd.LmonoError) as e:
        small.compute(s, k)
    assert e.value.code == ECAPACITY
    _assert_equal(f, ref)                                                  # refused before any launch: the last result stands
    assert f.compute(s, k[:0]).tolist() == [0] * 8 and len(f.read()[0]) == 0 and len(f.keypoints()) == 0          # m == 0 replaces it
    other = lmono_amd.Context(0)
    L = gpu_ctx.L
    assert L.lmono_fpfh_compute(other.h, f.h, s.h, k.ctypes.data, 10, None) == EINVAL          # a foreign handle
    assert L.lmono_fpfh_compute(gpu_ctx.h, None, s.h, k.ctypes.data, 10, None) == EINVAL
    assert L.lmono_fpfh_compute(gpu_ctx.h, f.h, None, k.ctypes.data, 10, None) == EINVAL
    assert L.lmono_fpfh_read(gpu_ctx.h, None, None, None, None, 0) == EINVAL
    assert L.lmono_fpfh_keypoints(other.h, f.h, None, 0) == EINVAL
    with pytest.raises(lmono_amd.LmonoError) as e:
        lmono_amd.FpfhDescriptors.compute_batch([f, f], [s, s], [k, k])                        # one handle twice
    assert e.value.code == EINVAL
    other.close()
    for x in (f, s, fresh, small):
        x.close()
