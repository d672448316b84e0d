"""k_compact_index counts the two "last" clouds per (scan line, azimuth bin) while it writes them, and runs two workgroups per CU.  The
order of the points inside one bucket of the index copy is not observable (exact searches, ties broken by cloud index; the ABI does not
expose the copy), so everything here compares through the four feature clouds (bitwise against oracle.scanreg) and through
ScanBatch.correspond (index for index against oracle.odom_step)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q = np.array([0.0, 0.0, 0.01, 1.0]) / np.linalg.norm([0.0, 0.0, 0.01, 1.0])
T = np.array([0.7, 0.02, 0.0])
IRREGULAR = 4          # kStatusIrregularLines
NAMES = ((1, "sharp"), (2, "less_sharp"), (3, "flat"), (4, "less_flat"))


def _batch(gpu_ctx, parts, n_lines=64, min_range=5.0):
    import torch
    import lmono_amd
    cat = np.ascontiguousarray(np.concatenate(parts, 0), np.float32)
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    dev = torch.from_numpy(cat if len(cat) else np.zeros((1, 4), np.float32)).to("cuda:0")
    batch = lmono_amd.ScanBatch(gpu_ctx, len(parts), max(len(cat), 1))
    batch.scanreg(dev.data_ptr(), off, n_lines, min_range, keepalive=dev)
    return batch


def _check_clouds(batch, s, ref, cnt=None):
    """counts and the four feature clouds of scan s, bitwise"""
    cnt = batch.counts() if cnt is None else cnt
    info = ref["info"]
    assert list(cnt[s, :5]) == [info.n_cloud, info.n_sharp, info.n_less_sharp, info.n_flat, info.n_less_flat], "scan %d: counts" % s
    cap = max(int(info.n_cloud), 1)
    for which, name in NAMES:
        got = batch.cloud(s, which, cap)
        assert np.array_equal(got.view(np.uint32), ref[name].view(np.uint32)), "scan %d: %s differs (bitwise)" % (s, name)


def _check_corr(oracle, batch, k, cur, last, q=Q, t=T):
    """correspondences of scan k's features in scan k - 1's "last" clouds"""
    _, _, _, corr = oracle.odom_step(cur["sharp"], cur["flat"], last["less_sharp"], last["less_flat"], q, t, want_corr=True)
    got = batch.correspond(k, q, t)
    assert got.shape == corr[0].shape and np.array_equal(got, corr[0]), "correspondence indices differ at scan %d" % k


@pytest.fixture(scope="module")
def small_ref(oracle, small_seq):
    """oracle.scanreg of the six small scans, computed once"""
    xyzi, off = small_seq["xyzi"], small_seq["off"]
    pts = [xyzi[off[s]:off[s + 1]] for s in range(len(off) - 1)]
    return pts, [oracle.scanreg(p) for p in pts]


def test_empty_and_tiny_clouds_beside_normal_ones(oracle, gpu_ctx, small_ref):
    """n = 0 in the merged pass (no trip of the copy loops, table[kLineKeys] = 0, elevation rows of empty lines only) as the first, a
    middle and the last scan of a batch, and a 40-point scan (no ring long enough for the voxel filter: less-flat cloud empty, 27 less-sharp points) between normal scans."""
    pts, ref = small_ref
    empty = np.zeros((0, 4), np.float32)
    tiny = pts[2][:40].copy()
    parts = [empty, pts[0], pts[1], empty, pts[2], tiny, pts[3], pts[4], empty]
    refs = [oracle.scanreg(empty), ref[0], ref[1], None, ref[2], oracle.scanreg(tiny), ref[3], ref[4], None]
    refs[3] = refs[8] = refs[0]
    assert refs[0]["info"].n_less_flat == 0 and refs[5]["info"].n_less_flat == 0 and refs[5]["info"].n_less_sharp < 64
    batch = _batch(gpu_ctx, parts)
    cnt = batch.counts()
    for s in range(len(parts)):
        _check_clouds(batch, s, refs[s], cnt)
    _check_corr(oracle, batch, 2, refs[2], refs[1])                       # normal beside normal
    _check_corr(oracle, batch, 7, refs[7], refs[6])                       # ... two workgroups behind the tiny scan's
    for k in (1, 4, 6):                                                   # "last" clouds empty (an empty scan, the tiny one)
        _check_corr(oracle, batch, k, refs[k], refs[k - 1])


def test_sixteen_bit_limit_inside_one_batch(oracle, gpu_ctx, full_seq):
    """A less-flat cloud of more than 65535 points (scan stretched by 4) beside one below the limit: the large one is copied plainly and
    indexed by the full-width launch, the shared counters serve the clouds around it."""
    xyzi, off = full_seq["xyzi"], full_seq["off"]
    a = xyzi[off[0]:off[1]].copy()
    b = xyzi[off[1]:off[2]].copy()
    b[:, :3] *= 4.0
    ra, rb = oracle.scanreg(a), oracle.scanreg(b)
    q = np.array([0.0, 0.0, 0.004, 1.0]); q /= np.linalg.norm(q)
    t = np.array([2.9, 0.0, 0.0])
    batch = _batch(gpu_ctx, [a, b])
    cnt = batch.counts()
    assert cnt[0, 4] <= 65535 < cnt[1, 4], cnt[:, 4]
    _check_clouds(batch, 0, ra, cnt)
    _check_clouds(batch, 1, rb, cnt)
    _check_corr(oracle, batch, 1, rb, ra, q, t)                           # "last" = the 16-bit cloud
    swapped = _batch(gpu_ctx, [b, a])
    cnt = swapped.counts()
    assert cnt[1, 4] <= 65535 < cnt[0, 4], cnt[:, 4]
    _check_clouds(swapped, 0, rb, cnt)
    _check_clouds(swapped, 1, ra, cnt)
    _check_corr(oracle, swapped, 1, ra, rb, q, t)                         # "last" = the deferred cloud


def test_one_azimuth_bin_many_lines_and_two_lines_all_bins(oracle, gpu_ctx, small_ref):
    """A scan cut to 0.8 degrees of azimuth inside one 0.9375-degree bin (dense rings: every point of a line in ONE counter; a wave's 64
    points span several lines: the per-lane elevation fallback) and a scan cut to two rings (a line's points in every bin; whole waves
    on one line: the wave-uniform path), each beside a normal scan."""
    pts, ref = small_ref
    w = oracle.S1World(n_az=24000)
    dense, _ = w.scans(w.trajectory(1))
    az = np.degrees(np.arctan2(dense[:, 1], dense[:, 0])) + 180.0
    lo = 100 * 360.0 / 384 + 0.05                                          # inside bin 100 of the index
    sector = dense[(az > lo) & (az < lo + 0.8)].copy()
    assert 1500 < len(sector) < 5000
    el = np.degrees(np.arctan2(pts[1][:, 2], np.hypot(pts[1][:, 0], pts[1][:, 1])))
    rings = np.degrees(oracle.hdl64_elevations_rad())
    two = pts[1][(np.abs(el - rings[12]) < 0.05) | (np.abs(el - rings[40]) < 0.05)].copy()
    assert 500 < len(two) < 1100
    r_sector, r_two = oracle.scanreg(sector), oracle.scanreg(two)
    assert r_two["info"].n_less_flat > 50 and len(np.unique(r_two["less_flat"][:, 3].astype(np.int32))) <= 2
    parts = [pts[0], sector, pts[2], two, pts[3]]
    refs = [ref[0], r_sector, ref[2], r_two, ref[3]]
    batch = _batch(gpu_ctx, parts)
    cnt = batch.counts()
    for s in range(len(parts)):
        _check_clouds(batch, s, refs[s], cnt)
    for k in range(1, len(parts)):
        _check_corr(oracle, batch, k, refs[k], refs[k - 1])


def test_shuffled_input(oracle, gpu_ctx, small_ref):
    """Points in random order (the stable ring sort still defines the cloud): clouds, counts and status bits as the oracle pins them, and
    the correspondences whichever search the status selects."""
    pts, ref = small_ref
    rng = np.random.default_rng(3)
    b = pts[1].copy()
    rng.shuffle(b, axis=0)
    c = pts[3].copy()
    rng.shuffle(c, axis=0)
    parts = [pts[0], b, pts[2], c]
    refs = [ref[0], oracle.scanreg(b), ref[2], oracle.scanreg(c)]
    batch = _batch(gpu_ctx, parts)
    cnt = batch.counts()
    for s in range(4):
        _check_clouds(batch, s, refs[s], cnt)
    # the irregular-lines flag (bit 2 of the status word) says exactly what the cloud says: some line a >= b + 3 starts before line b ends
    for s in range(4):
        irregular = False
        for name in ("less_sharp", "less_flat"):
            ln = np.clip(refs[s][name][:, 3].astype(np.int32), 0, 65)
            first = np.full(66, 1 << 30); last = np.full(66, -1)
            np.minimum.at(first, ln, np.arange(len(ln))); np.maximum.at(last, ln, np.arange(len(ln)))
            irregular |= any(first[a] < last[b] for a in range(66) for b in range(max(a - 2, 0)))
        assert bool(cnt[s, 5] & IRREGULAR) == irregular, "scan %d: irregular-lines flag" % s
    for k in (1, 2, 3):
        _check_corr(oracle, batch, k, refs[k], refs[k - 1])


def test_more_workgroups_than_fit_the_card_at_once(oracle, gpu_ctx, small_ref):
    """600 scans (two alternating, so that neighbouring workgroups hold different clouds): more workgroups than 2 x 256 CUs start at once.
    Nothing in static or dynamic LDS may be shared between the workgroups of one CU."""
    pts, ref = small_ref
    n = 600
    parts = [pts[s & 1] for s in range(n)]
    batch = _batch(gpu_ctx, parts)
    cnt = batch.counts()
    for s in range(n):
        info = ref[s & 1]["info"]
        assert list(cnt[s, :5]) == [info.n_cloud, info.n_sharp, info.n_less_sharp, info.n_flat, info.n_less_flat], "scan %d: counts" % s
    for s in list(range(0, n, 37)) + [n - 2, n - 1]:
        _check_clouds(batch, s, ref[s & 1], cnt)
    _check_corr(oracle, batch, n - 1, ref[1], ref[0])
    _check_corr(oracle, batch, n - 2, ref[0], ref[1])


def test_online_path_gives_the_batch_increments(gpu_ctx, small_seq):
    """lmono_odom_step registers one scan per call through the same kernel (grid of one workgroup): the increments of the batch path."""
    import lmono_amd
    xyzi, off = small_seq["xyzi"], small_seq["off"]
    pts = [xyzi[off[s]:off[s + 1]] for s in range(4)]
    batch = _batch(gpu_ctx, pts)
    ref_incr, _ = batch.odometry(1, 0)
    ref_cnt = batch.counts()
    st = lmono_amd.OdomStream(gpu_ctx, max(len(p) for p in pts) + 100, 64, 5.0, history=2)
    for k in range(4):
        incr, _, info = st.step(pts[k])
        assert (info[:6] == ref_cnt[k]).all(), "scan %d: counts / status differ" % k
        assert np.array_equal(incr, ref_incr[k]), "scan %d: increment differs from the batch run" % k
        for which, _name in NAMES:
            assert np.array_equal(st.cloud(which, len(pts[k])), batch.cloud(k, which, len(pts[k])))
    st.close()
