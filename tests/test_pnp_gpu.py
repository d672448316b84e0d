"""The loop verification on the device (lmono_pnp_ransac, lmono_keyframes_verify) against the CPU restatement
tests/pnp_ref.py: equal bytes up to the pose, a tolerance behind it (R2ypr uses atan2 / sin / cos)."""
import os

import numpy as np
import pytest

from tests import keyframe_ref as K
from tests import pnp_cases as S
from tests import pnp_ref as P
from tests import track_ref as R
from workloads import s5

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN_FILE = os.path.join(ROOT, "tests", "golden", "brief_pattern.yml")
IDENT = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
Z0 = 10.0            # depth of the s5 texture, taken as a fronto-parallel plane


def _params(**kw):
    import lmono_amd
    p = lmono_amd.PnPParams()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _error_code(exc):
    return int(str(exc.value).split("lmono error ")[1].split(":")[0])


def _check(got, ref, what):
    st, pose, stats = got
    rs, rp, rstats = ref
    assert stats.tolist() == rstats.tolist(), (what, stats, rstats)
    assert st.tobytes() == rs.tobytes(), what + ": status"
    assert pose.tobytes() == rp.tobytes(), what + ": pose bytes"


@pytest.mark.parametrize("m,n_hyp", [(4, 256), (5, 256), (65, 256), (150, 256), (512, 256), (150, 1), (150, 100), (150, 1024)])
def test_pnp_ransac_equals_restatement(gpu_ctx, m, n_hyp):
    import lmono_amd
    p3, p2, g, _, _ = S.scene(m, 17 * m + n_hyp, 0.25)
    st, pose, stats = lmono_amd.pnp_ransac(gpu_ctx, [p3], [p2], [g], [m + n_hyp], _params(n_hyp=n_hyp, seed=9))
    _check((st[0], pose[0], stats[0]), P.pnp_ransac(p3, p2, g, m + n_hyp, P.PnPParams(n_hyp=n_hyp, seed=9)), "m %d n_hyp %d" % (m, n_hyp))


def test_degenerate_inputs(gpu_ctx):
    import lmono_amd
    for name, (p3, p2, g) in S.degenerate_cases().items():
        st, pose, stats = lmono_amd.pnp_ransac(gpu_ctx, [p3], [p2], [g], [1])
        _check((st[0], pose[0], stats[0]), P.pnp_ransac(p3, p2, g, 1), name)
        assert not st[0].any() and pose[0].tobytes() == g.tobytes(), name
    p3, p2, g, _, _ = S.scene(65, 11, 0.0)
    p2[7, 0] = np.nan
    st, pose, stats = lmono_amd.pnp_ransac(gpu_ctx, [p3], [p2], [g], [1])
    _check((st[0], pose[0], stats[0]), P.pnp_ransac(p3, p2, g, 1), "one NaN observation")
    assert st[0][7] == 0 and st[0].sum() == 64


@pytest.mark.parametrize("n", [1, 3, 70])
def test_batch_equals_single_calls(gpu_ctx, n):
    """Problems of mixed sizes (fewer than 4 pairs and the cap of 512 among them) in one launch: each one's bytes are those of its own call."""
    import lmono_amd
    sizes = [150, 3, 512, 4, 0, 65, 26, 5, 257, 64]
    probs = [S.scene(max(sizes[i % len(sizes)], 1), 300 + i, 0.25) for i in range(n)]
    p3 = [p[0][:sizes[i % len(sizes)]] for i, p in enumerate(probs)]; p2 = [p[1][:sizes[i % len(sizes)]] for i, p in enumerate(probs)]
    g = np.stack([p[2] for p in probs]); keys = np.arange(n, dtype=np.uint32) * 65537 + 5
    prm = _params(n_hyp=100, seed=4)
    st, pose, stats = lmono_amd.pnp_ransac(gpu_ctx, p3, p2, g, keys, prm)
    for i in range(n):
        s1, q1, t1 = lmono_amd.pnp_ransac(gpu_ctx, [p3[i]], [p2[i]], [g[i]], [keys[i]], prm)
        _check((st[i], pose[i], stats[i]), (s1[0], q1[0], t1[0]), "problem %d of %d (m = %d)" % (i, n, len(p3[i])))
    for i in range(min(n, 10)):
        _check((st[i], pose[i], stats[i]), P.pnp_ransac(p3[i], p2[i], g[i], int(keys[i]), P.PnPParams(n_hyp=100, seed=4)), "problem %d against the restatement" % i)


def test_pnp_ransac_error_returns(gpu_ctx):
    import lmono_amd
    p3, p2, g, _, _ = S.scene(20, 1, 0.0)
    big = np.zeros((513, 3), np.float32)
    with pytest.raises(lmono_amd.LmonoError) as e:
        lmono_amd.pnp_ransac(gpu_ctx, [big], [big[:, :2]], [g])
    assert _error_code(e) == -4, "more than 512 pairs: LMONO_ECAPACITY"
    for bad in (dict(n_hyp=1025), dict(n_hyp=-1), dict(threshold=-1.0), dict(threshold=float("nan")), dict(min_pnp_loop_num=-1), dict(angle_threshold=-1.0)):
        with pytest.raises(lmono_amd.LmonoError) as e:
            lmono_amd.pnp_ransac(gpu_ctx, [p3], [p2], [g], None, _params(**bad))
        assert _error_code(e) == -1, bad
    for bad_g in (np.zeros(7), np.array([0, 0, 0, 0, 0, 0, np.nan])):
        with pytest.raises(lmono_amd.LmonoError) as e:
            lmono_amd.pnp_ransac(gpu_ctx, [p3], [p2], [bad_g])
        assert _error_code(e) == -1
    st, pose, stats = lmono_amd.pnp_ransac(gpu_ctx, [p3], [p2], [g])        # and the context still works
    assert stats[0][0] > 0


# ---- KeyFrames.verify ------------------------------------------------------------------------------------------------------------
def _cams(w, h):
    import lmono_amd
    fx = 0.9 * w
    return (lmono_amd.Camera(w, h, fx, fx * 1.01, 0.5 * w - 3.0, 0.5 * h + 2.0, 0.0, 0.0, 0.0, 0.0, 5, 0, 0), R.Camera(w, h, fx, fx * 1.01, 0.5 * w - 3.0, 0.5 * h + 2.0, 0.0, 0.0, 0.0, 0.0))


_S5 = {}


def s5_case():
    """workloads/s5 320 x 240, seed 1, keyframes of frame 2 and frame 8 (DESIGN.md 6f's pair), the texture a fronto-parallel plane at Z0.
    The world frame is frame 2's camera frame, so the old camera's true pose is the identity; frame 8's camera is shifted by the
    known flow.  A third keyframe is frame 0 of another world (seed 2).  Computed once, on the CPU restatements alone."""
    if _S5:
        return _S5
    w, h = 320, 240
    _, rc = _cams(w, h)
    pat = _pattern_rows()
    seq = s5.Sequence(w, h, 9, seed=1, step=(1.5, 0.5))
    trk = R.TrackerRef(rc, 150, 15)
    rec = [trk.track(0.1 * k, seq.frames[k]) for k in range(9)]
    uv2 = np.stack([rec[2]["u"], rec[2]["v"]], 1); uv8 = np.stack([rec[8]["u"], rec[8]["v"]], 1)
    other = s5.Sequence(w, h, 1, seed=2).frames[0]
    in2 = seq.from_canvas(2, seq.to_canvas(8, uv8.astype(np.float64)))          # where frame 8's window points lie in frame 2
    p3 = np.stack([(in2[:, 0] - rc.cx) / rc.fx * Z0, (in2[:, 1] - rc.cy) / rc.fy * Z0, np.full(len(in2), Z0)], 1).astype(np.float32)
    shift = seq.from_canvas(2, seq.to_canvas(8, np.array([[0.0, 0.0]])))[0]     # frame 8's pixel (0, 0) in frame 2: the camera moved by this
    delta = np.array([shift[0] / rc.fx * Z0, shift[1] / rc.fy * Z0, 0.0])
    vio = np.concatenate([delta, [0.0, 0.0, 0.0, 1.0]])
    refs = [K.KeyFrameRef(rc, pat, seq.frames[2], uv2), K.KeyFrameRef(rc, pat, seq.frames[8], uv8), K.KeyFrameRef(rc, pat, other, uv2)]
    _S5.update(seq=seq, other=other, uv2=uv2, uv8=uv8, in2=in2, p3=p3, delta=delta, vio=vio, refs=refs, rc=rc)
    return _S5


def _pattern_rows():
    import lmono_amd
    return lmono_amd.load_brief_pattern(PATTERN_FILE)


def ref_verify(case, cur, olds, old_tq=None, params=None):
    """pnp_ref fed with the restatement's match: what lmono_keyframes_verify must return."""
    prm = params or P.PnPParams()
    refs, out = case["refs"], []
    guess = P.guess_from_vio(case["vio"], IDENT)
    for n, o in enumerate(olds):
        status, _, _, uv, nm, count = refs[cur].match(refs[o])
        sel = status.astype(bool)
        full = np.zeros(len(sel), np.uint8)
        if count > prm.min_brief_loop_num:
            st, pose, stats = P.pnp_ransac(case["p3"][sel], nm[sel], guess, P.caller_key(cur, o), prm)
            full[np.nonzero(sel)[0]] = st
        else:
            pose, stats = guess.copy(), np.full(4, -1, np.int32)
        inl = int(stats[2]) if stats[0] > 0 and stats[2] >= 4 else 0
        r = P.after_pnp(pose, count, inl, case["vio"], IDENT, None if old_tq is None else old_tq[n], cur, prm)
        r.update(count=count, inliers=inl, status=full, pose=pose, stats=stats, old_uv=uv, sel=sel)
        out.append(r)
    return out


def _store(gpu_ctx, case):
    import lmono_amd
    gc, _ = _cams(320, 240)
    kf = lmono_amd.KeyFrames(gpu_ctx, gc, _pattern_rows(), 8, 8192)
    kf.add(case["seq"].frames[2], case["uv2"]); kf.add(case["seq"].frames[8], case["uv8"]); kf.add(case["other"], case["uv2"])
    return kf


def _check_verify(v, ref, n_old, with_channel):
    for o in range(n_old):
        r = ref[o]
        assert v["counts"][o] == r["count"] and v["inliers"][o] == r["inliers"] and v["stats"][o].tolist() == r["stats"].tolist(), (o, v["stats"][o], r["stats"])
        assert v["status"][o].tobytes() == r["status"].tobytes(), "status after both reductions"
        assert v["pose"][o].tobytes() == r["pose"].tobytes(), "pose bytes"
        assert bool(v["has_loop"][o]) == r["has_loop"]
        assert np.abs(v["pnp_tq_old"][o] - np.concatenate([r["pnp_t_old"], r["pnp_q_old"]])).max() < 1e-12
        assert np.abs(v["loop_info"][o] - r["loop_info"]).max() < 1e-9 and np.abs(v["relative_euler"][o] - r["relative_euler"]).max() < 1e-9
        if with_channel:
            assert np.abs(v["channel"][o] - r["channel"]).max() < 1e-9


def test_verify_on_s5_equals_restatement_and_finds_the_revisit(gpu_ctx):
    case = s5_case()
    kf = _store(gpu_ctx, case)
    old_tq = np.stack([IDENT, np.concatenate([[1.0, 2.0, 3.0], S.quat_axis_angle([0, 0, 1], 0.3)])])
    v = kf.verify(1, [0, 2], case["p3"], case["vio"], IDENT, old_tq)
    ref = ref_verify(case, 1, [0, 2], old_tq)
    _check_verify(v, ref, 2, True)
    rev, oth = ref[0], ref[1]
    print("revisit: matched %d, inliers %d, relative_t %s (true %s); other world: matched %d, inliers %d, has_loop %s" %
          (rev["count"], rev["inliers"], rev["relative_t"], case["delta"], oth["count"], oth["inliers"], oth["has_loop"]))
    # the physical claims, as the restatement gives them
    assert v["has_loop"][0] and v["loops"].tolist()[0] == [0, 1] and len(v["loops"]) == len(v["loops_info"]) == int(v["has_loop"].sum())
    # an inlier lies within thr of its reprojection, i.e. within thr * Z0 on the plane: the camera's shift over the plane is found at least that well
    assert np.abs(v["loop_info"][0][:3] - case["delta"]).max() < P.THRESHOLD * Z0
    wrong = np.hypot(*(rev["old_uv"] - case["in2"]).T) > 50.0
    assert (rev["sel"] & wrong).sum() > 0 and not (v["status"][0].astype(bool) & wrong).any(), "a match more than 50 px off survived"
    assert v["inliers"][1] < v["inliers"][0] // 4 and bool(v["has_loop"][1]) == oth["has_loop"]
    kf.close()


def test_verify_gated_candidate_in_a_batch_and_no_old_poses(gpu_ctx):
    """A gate between the two candidates' counts: the lower one skips PnP (stats -1, has_loop 0), the other is as alone; old_tq=None."""
    case = s5_case()
    kf = _store(gpu_ctx, case)
    counts = kf.match(1, [0, 2])["counts"]
    lo, hi = int(counts.min()), int(counts.max())
    assert lo < hi
    prm = _params(min_brief_loop_num=lo, n_hyp=100)
    v = kf.verify(1, [2, 0, 0], case["p3"], case["vio"], IDENT, None, prm)
    ref = ref_verify(case, 1, [2, 0, 0], None, P.PnPParams(min_brief_loop_num=lo, n_hyp=100))
    _check_verify(v, ref, 3, False)
    gated = int(np.argmin(counts))          # position in [0, 2] -> in [2, 0, 0]
    g = 0 if gated == 1 else 1
    assert v["channel"] is None and (v["stats"][g] == -1).all() and not v["has_loop"][g] and not v["status"][g].any() and v["inliers"][g] == 0
    assert v["pose"][1].tobytes() == v["pose"][2].tobytes(), "the same candidate twice in a batch"
    alone = kf.verify(1, [0], case["p3"], case["vio"], IDENT, None, prm)
    assert alone["pose"][0].tobytes() == v["pose"][1].tobytes() and alone["status"][0].tobytes() == v["status"][1].tobytes()
    kf.close()


def test_verify_error_returns(gpu_ctx):
    import lmono_amd
    case = s5_case()
    kf = _store(gpu_ctx, case)
    for args in ((5, [0]), (1, [7]), (-1, [0])):
        with pytest.raises(lmono_amd.LmonoError) as e:
            kf.verify(args[0], args[1], case["p3"], case["vio"], IDENT)
        assert _error_code(e) == -1
    with pytest.raises(lmono_amd.LmonoError) as e:
        kf.verify(1, [0], case["p3"], np.zeros(7), IDENT)
    assert _error_code(e) == -1
    with pytest.raises(lmono_amd.LmonoError) as e:
        kf.verify(1, [0], case["p3"], case["vio"], IDENT, None, _params(n_hyp=2000))
    assert _error_code(e) == -1
    with pytest.raises(lmono_amd.LmonoError):
        kf.verify(1, [0], case["p3"][:5], case["vio"], IDENT)
    assert kf.verify(1, [0], case["p3"], case["vio"], IDENT)["has_loop"][0]
    kf.close()


def test_loop_from_verify_feeds_the_pose_graph(gpu_ctx):
    """A 12-keyframe chain along the camera's shift whose odometry drifts; the loop between keyframes 0 and 11 comes from verify on the
    s5 pair; PoseGraph takes verify's arrays as they are and optimize lowers the cost.  Plumbing only."""
    import lmono_amd
    case = s5_case()
    kf = _store(gpu_ctx, case)
    v = kf.verify(1, [0], case["p3"], case["vio"], IDENT)
    assert v["has_loop"][0]
    n = 12
    poses = np.tile(IDENT, (n, 1))
    poses[:, :3] = np.outer(np.arange(n) / (n - 1.0), case["delta"] + np.array([0.4, -0.3, 0.0]))        # the chain ends 0.5 m off
    loops = np.array([[0, n - 1]], np.int32)           # verify's (old, cur) pair, renumbered into the chain
    pg = lmono_amd.PoseGraph(gpu_ctx, poses, loops, v["loops_info"])
    out, st = pg.optimize(10)
    print("pose graph: cost %.6g -> %.6g" % (st["initial_cost"], st["final_cost"]))
    assert st["final_cost"] < st["initial_cost"] and np.isfinite(out).all()
    pg.close(); kf.close()


def test_host_mirror_verify_mode_equals_python_path(gpu_ctx, tmp_path):
    """lmono_amd/host/keyframe_test ... verify: KeyFrame::findConnection to its end (KeyFrame.cc:354-691) over lmono_keyframes_verify.  The lines it
    adds behind its unchanged output equal the Python path's on the same frames, line by line."""
    import subprocess
    import lmono_amd
    exe = os.path.join(ROOT, "lmono_amd", "host", "keyframe_test")
    assert os.path.exists(exe), "build() makes lmono_amd/host/keyframe_test"
    w, h, k, delta = 320, 240, 2, 6
    seq = s5.Sequence(w, h, k + delta + 1, seed=1, step=(1.5, 0.5), rot_step=0.002, zoom_step=0.001)
    raw = tmp_path / "frames.raw"
    with open(raw, "wb") as f:
        f.write(("%d %d %d\n" % (w, h, len(seq.frames))).encode())
        for img in seq.frames:
            f.write(np.ascontiguousarray(img).tobytes())
    plain = subprocess.run([exe, str(raw), PATTERN_FILE, str(k), str(delta)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    res = subprocess.run([exe, str(raw), PATTERN_FILE, str(k), str(delta), "verify"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert plain.returncode == 0 and res.returncode == 0, res.stderr[-2000:]
    got = res.stdout.splitlines()
    n_plain = len(plain.stdout.splitlines())
    assert got[:n_plain] == plain.stdout.splitlines(), "the mode changes none of the existing output lines"
    # the Python path with the camera, limits and made-up geometry of keyframe_test.cpp
    cam = lmono_amd.Camera(w, h, 300.0, 300.0, 0.5 * w, 0.5 * h, -0.1, 0.02, 0.0005, -0.0005, 5, 0, 0)
    trk = lmono_amd.FeatureTracker(gpu_ctx, cam, 150, 15)
    kf = lmono_amd.KeyFrames(gpu_ctx, cam, _pattern_rows(), 8, 16384)
    recs = {}
    for f in range(k + delta + 1):
        rec = trk.track(0.1 * f, seq.frames[f])
        if f in (k, k + delta):
            recs[kf.add(seq.frames[f], np.stack([rec["u"], rec["v"]], 1))[0]] = rec
    rec = recs[1]
    ten = np.float32(10.0)
    p3 = np.stack([rec["x_n"] * ten + np.float32(0.3), rec["y_n"] * ten + np.float32(0.1), np.full(len(rec), ten)], 1).astype(np.float32)
    vio = np.array([0.3, 0.1, 0.0, 0.0, 0.0, 0.0, 1.0])
    v = kf.verify(1, [0], p3, vio, IDENT, [IDENT])
    m = kf.match(1, [0])
    loop = bool(v["has_loop"][0])
    lines = ["VERIFY brief %d pnp %d has_loop %d loop_index %d" % (v["counts"][0], v["inliers"][0], 1 if loop else 0, 0 if loop else -1)]
    if loop:
        lines.append("LOOP_INFO" + "".join(" %.9g" % x for x in v["loop_info"][0]))
        lines.append("CHANNEL" + "".join(" %.9g" % x for x in v["channel"][0]))
        for i in np.nonzero(v["status"][0])[0]:
            on = m["old_norm"][0][i]
            lines.append("LOOP_POINT %d cur_norm %.9g %.9g old_norm %.9g %.9g published %.9g %.9g %.9g" %
                         (rec["id"][i], rec["x_n"][i], rec["y_n"][i], on[0], on[1], on[0], on[1], np.float32(rec["id"][i])))
    print("\n".join(lines[:3]))
    assert got[n_plain + 1:] == lines
    # KeyFrame::PnPRANSAC on the matched pairs (key 0): the same inliers as lmono_pnp_ransac from Python, PnP_T_old / PnP_R_old as the restatement derives them
    word = got[n_plain].split()
    assert word[0] == "PNPRANSAC"
    sel = m["status"][0].astype(bool)
    st, pose, _ = lmono_amd.pnp_ransac(gpu_ctx, [p3[sel]], [m["old_norm"][0][sel]], [P.guess_from_vio(vio, IDENT)], [0])
    r = P.after_pnp(pose[0], 0, 0, vio, IDENT)
    assert int(word[2]) == int(sel.sum()) and int(word[4]) == int(st[0].sum()) > 0
    assert np.abs(np.array(word[6:9], np.float64) - r["pnp_t_old"]).max() < 1e-9 and np.abs(np.array(word[10:14], np.float64) - r["pnp_q_old"]).max() < 1e-9
    trk.close(); kf.close()
