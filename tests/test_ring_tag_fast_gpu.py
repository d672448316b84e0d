"""k_ring_tag decides ring id and half sweep without an arctangent (lmono_amd/csrc/ring_decide.hpp: an odd polynomial in z / rho, the signs
of a dot and a cross product with the sweep's start direction) and with the fp64 forms inside a guard of every threshold.  Scans of a
few thousand points placed on both sides of those guards (2e-3 deg, 4e-5 rad) must come out bit for bit as the oracle's: the ring-sorted
cloud with its .w (ring + 0.1 relTime), the counts, the four feature clouds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MIN_RANGE = 0.5
# start directions (x0, y0) of the sweep: the four axes and one per quadrant
STARTS = [(7.0, 0.0), (0.0, 3.0), (-12.0, 0.0), (0.0, -5.5), (4.1, 9.3), (-8.7, 2.2), (-3.3, -6.1), (21.0, -17.5)]
WINDOW = {16: (-14.0, 14.0), 32: (-30.0, 10.0), 64: (-17.0, 1.5)}       # elevations every sensor keeps


def _ring_thresholds(n_lines):
    """Elevations (deg) at which the reference's ring id changes its answer."""
    if n_lines == 16:
        return [-18.0] + [2.0 * k - 16.0 for k in range(1, 17)]
    if n_lines == 32:
        return [-32.0] + [k * 4.0 / 3.0 - 92.0 / 3.0 for k in range(1, 33)]
    return [2.0, -8.83, -24.33] + [2.0 - (k - 0.5) / 3.0 for k in range(1, 33)] + [-8.83 - (k - 0.5) / 2.0 for k in range(1, 20)]


def _points(rho, az, el_deg, rng):
    return np.stack([rho * np.cos(az), rho * np.sin(az), rho * np.tan(np.radians(el_deg)), rng.uniform(0, 1, len(rho))], 1).astype(np.float32)


def _log_rho(rng, n):
    return np.exp(rng.uniform(np.log(0.6), np.log(200.0), n))            # 0.6 m .. 200 m


def _threshold_scan(n_lines, rng, start, shuffle=True):
    lo, hi = WINDOW[n_lines]
    # elevation: offsets on both sides of the guard's edge (2e-3 deg), on the threshold and far inside the band
    d_el = np.array([0.0, 1e-6, 1e-5, 1e-4, 1.8e-3, 1.95e-3, 2.05e-3, 2.2e-3, 4e-3])
    ang = np.array([t + sg * d for t in _ring_thresholds(n_lines) for d in d_el for sg in (-1.0, 1.0)])
    ang = np.repeat(ang, 2)
    el_pts = _points(_log_rho(rng, len(ang)), rng.uniform(-np.pi, np.pi, len(ang)), ang, rng)
    # azimuth: ori = -atan2(y, x) relative to the first valid point's; pi and 3 pi / 2 = -pi / 2 are thresholds, 0 and pi / 2 are none
    ori0 = -np.arctan2(start[1], start[0])
    d_az = np.array([0.0, 1e-7, 1e-6, 1e-5, 3.6e-5, 3.9e-5, 4.1e-5, 4.4e-5, 1e-4])
    ori = np.array([ori0 + t + sg * d for t in (np.pi, 1.5 * np.pi, -0.5 * np.pi, 0.0, 0.5 * np.pi) for d in d_az for sg in (-1.0, 1.0)])
    ori = np.repeat(ori, 6)
    az_pts = _points(_log_rho(rng, len(ori)), -ori, rng.uniform(lo, hi, len(ori)), rng)
    fill = _points(_log_rho(rng, 1500), rng.uniform(-np.pi, np.pi, 1500), rng.uniform(lo - 3.0, hi + 3.0, 1500), rng)
    el0 = np.radians(0.5 * (lo + hi))
    special = np.array([
        [0.0, 0.0, 7.0, 0.5], [0.0, -0.0, -9.0, 0.5], [-0.0, 0.0, 0.6, 0.1],                       # x = y = 0: elevation +-90 deg
        [1e-40, 0.0, 3.0, 0.2], [0.0, 1e-20, 8.0, 0.1], [1e-40, 2.0, 2.0 * np.tan(el0), 0.3],         # denormal coordinates, a radius below 1e-15
        [3.0, -1e-42, 3.0 * np.tan(el0), 0.3], [5.0, 4.0, 1e-41, 0.4], [5.0, 4.0, -0.0, 0.4],
        [np.nan, 1.0, 1.0, 0.0], [1.0, np.inf, 1.0, 0.0], [1.0, 1.0, -np.inf, 0.0], [np.nan, np.nan, np.nan, 0.0],
    ], np.float32)
    first = np.array([[start[0], start[1], np.hypot(*start) * np.tan(el0), 0.7]], np.float32)
    mid = np.concatenate([el_pts, az_pts, fill, special], 0)
    if shuffle:
        rng.shuffle(mid, axis=0)
    dead = np.tile(np.array([[0.3, 0.2, -0.1, 0.0]], np.float32), (300, 1))                          # inside min_range
    dead[::7, 1] = np.nan
    return np.concatenate([dead, first, mid, dead], 0)


def _cat(scans):
    return np.concatenate(scans, 0), np.concatenate([[0], np.cumsum([len(p) for p in scans])]).astype(np.int64)


def _check_scan(oracle, get_cloud, counts, scan, n_lines):
    ref = oracle.scanreg(scan, n_lines, MIN_RANGE)
    info = ref["info"]
    if counts is not None:
        assert list(counts[:5]) == [info.n_cloud, info.n_sharp, info.n_less_sharp, info.n_flat, info.n_less_flat]
    for which, name in ((0, "cloud"), (1, "sharp"), (2, "less_sharp"), (3, "flat"), (4, "less_flat")):
        got = get_cloud(which, len(scan))
        assert got.shape == ref[name].shape, name + ": %d points, the oracle has %d" % (len(got), len(ref[name]))
        assert np.array_equal(got.view(np.uint32), ref[name].view(np.uint32)), name + " differs (bitwise)"
    return info


def _run_batch(oracle, gpu_ctx, scans, n_lines):
    import torch
    import lmono_amd
    cat, off = _cat(scans)
    dev = torch.from_numpy(np.ascontiguousarray(cat)).to("cuda:0")
    batch = lmono_amd.ScanBatch(gpu_ctx, len(scans), len(cat))
    batch.scanreg(dev.data_ptr(), off, n_lines, MIN_RANGE, keepalive=dev)
    cnt = batch.counts()
    return [_check_scan(oracle, lambda which, cap, s=s: batch.cloud(s, which, cap), cnt[s], scans[s], n_lines) for s in range(len(scans))]


@pytest.mark.parametrize("n_lines", [16, 32, 64])
def test_threshold_points_with_every_start_direction(oracle, gpu_ctx, n_lines):
    """One scan per start direction (axes and quadrants): points straddling the guards of every ring and half-sweep threshold at 0.6 to
    200 m, shuffled, behind an invalid head and before an invalid tail, with NaN / Inf / denormal coordinates and x = y = 0."""
    rng = np.random.default_rng(1400 + n_lines)
    infos = _run_batch(oracle, gpu_ctx, [_threshold_scan(n_lines, rng, st) for st in STARTS], n_lines)
    assert min(i.n_cloud for i in infos) > 1500


@pytest.mark.parametrize("n_lines", [16, 32, 64])
def test_ring_major_order_and_a_scan_that_is_discarded_whole(oracle, gpu_ctx, n_lines):
    """Unshuffled threshold points (long runs of one ring per wave), a scan whose every valid point lies outside the sensor's window
    (by the comparison of z / rho alone and by the polynomial next to the window's ends), a scan of x = y = 0 only."""
    rng = np.random.default_rng(2400 + n_lines)
    lo, hi = WINDOW[n_lines]
    out_el = np.concatenate([rng.uniform(35.0, 89.0, 1200), rng.uniform(-89.0, -35.0, 1200), rng.uniform(17.0, 20.0, 300), rng.uniform(-24.0, -18.2, 300) if n_lines != 32 else rng.uniform(-35.0, -32.1, 300)])
    gone = _points(_log_rho(rng, len(out_el)), rng.uniform(-np.pi, np.pi, len(out_el)), out_el, rng)
    poles = np.zeros((500, 4), np.float32)
    poles[:, 2] = rng.uniform(1.0, 9.0, 500) * np.where(np.arange(500) % 2, 1.0, -1.0)
    scans = [_threshold_scan(n_lines, rng, STARTS[5], shuffle=False), gone, _threshold_scan(n_lines, rng, STARTS[0]), poles]
    infos = _run_batch(oracle, gpu_ctx, scans, n_lines)
    assert infos[1].n_cloud == 0 and infos[3].n_cloud == 0 and infos[0].n_cloud > 1500


@pytest.mark.parametrize("n_lines", [16, 32, 64])
def test_one_scan_online_path(oracle, gpu_ctx, n_lines):
    """The online stream registers one scan per launch in a slot longer than the scan (n_limit): the same threshold scans, one after the other."""
    import lmono_amd
    rng = np.random.default_rng(3400 + n_lines)
    scans = [_threshold_scan(n_lines, rng, STARTS[6]), _threshold_scan(n_lines, rng, STARTS[3])[:-150], _threshold_scan(n_lines, rng, STARTS[4])]
    st = lmono_amd.OdomStream(gpu_ctx, max(len(p) for p in scans) + 777, n_lines, MIN_RANGE, history=2)
    try:
        for scan in scans:
            st.step(scan)
            info = _check_scan(oracle, st.cloud, None, scan, n_lines)
            assert info.n_cloud > 1500
    finally:
        st.close()
