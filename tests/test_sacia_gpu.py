"""The sample-consensus initial alignment on the GPU (lmono_sacia_*) against the numpy restatement of its definition
(tests/sacia_ref.py): transform, per-hypothesis error words and inliers, winning hypothesis and void count as bytes.  The descriptors are computed
on the device (SurfaceNormals -> FpfhDescriptors); the restatement runs on the FPFH restatement, whose bytes the device's descriptors equal
(tests/test_fpfh_gpu.py)."""
import numpy as np
import pytest

from tests import icp_ref as IR
from tests import sacia_cases as SC
from tests import sacia_ref as R

pytestmark = pytest.mark.gpu

EINVAL = -1


@pytest.fixture(scope="module")
def refs():
    """Every case's restatement, computed once and left unchanged."""
    return {name: R.run(*SC.sides(name), **SC.CASES[name][4]) for name in SC.CASES}


def _fpfh(gpu_ctx, name, keep):
    import lmono_amd
    p, nkw, k, fkw, ref = SC.fpfh_of(name, keep)
    s = lmono_amd.SurfaceNormals(gpu_ctx, len(p), **{a: v for a, v in nkw.items() if a != "viewpoint"})
    s.compute(p, nkw.get("viewpoint"))
    f = lmono_amd.FpfhDescriptors(gpu_ctx, len(p), len(k), **fkw)
    f.compute(s, k)
    assert f.read()[2].tobytes() == ref.flags.tobytes()
    return s, f


def _sides(gpu_ctx, name):
    s, t, ks, kt, _ = SC.CASES[name]
    return _fpfh(gpu_ctx, s, ks), _fpfh(gpu_ctx, t, kt)


def _close(*pairs):
    for s, f in pairs:
        f.close(); s.close()


def _assert_equal(a, stats, ref):
    assert stats.tolist() == ref.stats.tolist() and a.stats.tolist() == ref.stats.tolist()
    err, inl = a.errors()
    assert err.dtype == np.uint64 and err.tobytes() == ref.err.tobytes() and inl.tobytes() == ref.inl.tobytes()
    if ref.ok:
        assert a.transform().tobytes() == ref.T.tobytes()
    else:
        with pytest.raises(Exception) as e:
            a.transform()
        assert e.value.code == EINVAL


def _run(gpu_ctx, name, ref, **more):
    import lmono_amd
    src, tgt = _sides(gpu_ctx, name)
    a = lmono_amd.CoarseAligner(gpu_ctx, **dict(SC.CASES[name][4], **more))
    _assert_equal(a, a.align(src[1], tgt[1]), ref)
    a.close(); _close(src, tgt)


@pytest.mark.parametrize("name", sorted(n for n in SC.CASES if n != "two_usable"))
def test_every_case_equals_the_restatement(gpu_ctx, refs, name):
    """k_corr 1, 3 and 10, n_hyp = 1, every hypothesis void (ok = 0, no transform), tied errors (the lowest h wins), exactly 3 usable keypoints, two
    seeds, the resampled source.  What each case is, is checked on the restatement in tests/test_sacia_ref_cpu.py."""
    _run(gpu_ctx, name, refs[name])


def test_two_seeds_differ(refs):
    assert refs["rigid_k10"].err.tobytes() != refs["rigid_seed2"].err.tobytes()


def test_two_usable_keypoints_are_refused(gpu_ctx, refs):
    import lmono_amd
    assert refs["two_usable"] is None
    src, tgt = _sides(gpu_ctx, "two_usable")
    a = lmono_amd.CoarseAligner(gpu_ctx, **SC.CASES["two_usable"][4])
    with pytest.raises(lmono_amd.LmonoError) as e:
        a.align(src[1], tgt[1])
    assert e.value.code == EINVAL
    with pytest.raises(lmono_amd.LmonoError):
        a.transform()
    a.close(); _close(src, tgt)


@pytest.mark.parametrize("launch_hyps", [1, 7, 64])
def test_hypotheses_split_over_launches_give_equal_bytes(gpu_ctx, refs, launch_hyps):
    _run(gpu_ctx, "rigid_k10", refs["rigid_k10"], launch_hyps=launch_hyps)


def test_a_failed_align_hides_the_last_result(gpu_ctx, refs):
    import lmono_amd
    src, tgt = _sides(gpu_ctx, "rigid_k1")
    few = _fpfh(gpu_ctx, "scene", (5, 50))
    a = lmono_amd.CoarseAligner(gpu_ctx, **SC.CASES["rigid_k1"][4])
    _assert_equal(a, a.align(src[1], tgt[1]), refs["rigid_k1"])
    with pytest.raises(lmono_amd.LmonoError):
        a.align(few[1], tgt[1])
    with pytest.raises(lmono_amd.LmonoError):
        a.transform()
    assert len(a.errors()[0]) == 0
    a.close(); _close(src, tgt, few)


def test_end_to_end_coarse_then_fine(gpu_ctx, refs):
    """SurfaceNormals -> FpfhDescriptors on both clouds -> CoarseAligner.align -> refine(CloudAligner): the refined transform is the restatement's
    chain, tests/icp_ref.run started from the coarse transform."""
    import lmono_amd
    src, tgt = _sides(gpu_ctx, "rigid_k1")
    ps, pt = SC.fpfh_of("scene")[0], SC.fpfh_of("scene_rigid")[0]
    a = lmono_amd.CoarseAligner(gpu_ctx, **SC.CASES["rigid_k1"][4])
    a.align(src[1], tgt[1])
    icp = lmono_amd.CloudAligner(gpu_ctx, len(ps), len(pt), max_corr=0.5, max_iter=50)
    icp.set_target(pt)
    stats = a.refine(icp, ps)
    want = IR.run(pt, ps, max_corr=0.5, max_iter=50, guess=refs["rigid_k1"].T)
    assert stats.tolist() == want.stats.tolist() and icp.transform().tobytes() == want.transform.tobytes()
    icp.close(); a.close(); _close(src, tgt)


def test_bad_input(gpu_ctx):
    import lmono_amd
    for kw in (dict(min_sample_dist=-1.0), dict(max_corr=0.0), dict(max_corr=17.0), dict(k_corr=0), dict(k_corr=33), dict(n_hyp=0), dict(n_hyp=65537)):
        with pytest.raises(lmono_amd.LmonoError) as e:
            lmono_amd.CoarseAligner(gpu_ctx, **kw)
        assert "k_corr in 1 .. 32" in str(e.value) and "n_hyp in 1 .. 65536" in str(e.value)
    # a descriptor handle without a result
    f = lmono_amd.FpfhDescriptors(gpu_ctx, 16, 16)
    a = lmono_amd.CoarseAligner(gpu_ctx)
    with pytest.raises(lmono_amd.LmonoError) as e:
        a.align(f, f)
    assert e.value.code == EINVAL
    a.close(); f.close()
