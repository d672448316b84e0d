"""k_select computes the curvature and the gap flags of a sector itself, from the ring-sorted cloud (lmono_amd/csrc/curv_window.hpp):
no k_curvature in the registration, and lmono_batch_get_curvature runs it on demand.  Small synthetic scans through ScanBatch.scanreg
against the CPU oracle, bit for bit: labels, the four feature clouds, counts, and curvature() against the oracle's curvature array.

The shapes are those at which the new code can go wrong: the halo of a sector (five points before its first element, five behind its
last) comes from the neighbouring lanes, from the lanes behind the sector's end, or from loads of lane 0 and lane 63 -- which of them
depends on the sector's length and the elements per lane (5 up to 320 points, 6 up to 384, 11 above).  Every case states its
precondition on the oracle's output alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _gaps(cloud):
    """gap[i]: the step from point i to point i + 1 of the cloud is long (float32, as the kernels evaluate it)."""
    d = cloud[1:, :3] - cloud[:-1, :3]
    s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return np.concatenate([s.astype(np.float64) > 0.05, [False]])


def _sectors(n):
    """(sp, ep) of the six sectors of a ring of n points, ring-local."""
    span = n - 11
    return [(5 + span * j // 6, 5 + span * (j + 1) // 6 - 1) for j in range(6)]


def _check(gpu_ctx, xyzi, off, n_lines, min_range, refs):
    import torch
    import lmono_amd
    dev = torch.from_numpy(np.ascontiguousarray(xyzi)).to("cuda:0")
    batch = lmono_amd.ScanBatch(gpu_ctx, len(off) - 1, max(len(xyzi), 1))
    batch.scanreg(dev.data_ptr(), off, n_lines, min_range, keepalive=dev)
    cnt = batch.counts()
    for s, ref in enumerate(refs):
        info = ref["info"]
        n = int(off[s + 1] - off[s])
        assert cnt[s, 0] == info.n_cloud
        assert list(cnt[s, 1:5]) == [info.n_sharp, info.n_less_sharp, info.n_flat, info.n_less_flat], "counts of scan %d" % s
        cv, lb = batch.curvature(s, n)
        assert np.array_equal(lb, ref["label"]), "labels of scan %d differ at %s" % (s, np.flatnonzero(lb != ref["label"])[:8])
        assert np.array_equal(cv.view(np.uint32), ref["curvature"].view(np.uint32)), "curvature of scan %d differs (bitwise)" % s
        for which, name in ((1, "sharp"), (2, "less_sharp"), (3, "flat"), (4, "less_flat")):
            got = batch.cloud(s, which, n)
            assert np.array_equal(got.view(np.uint32), ref[name].view(np.uint32)), "%s cloud of scan %d differs (bitwise)" % (name, s)
    return batch


def _set_range(a, beg, end, rho):
    """Points beg .. end - 1 moved along their rays to the ranges rho (same ring, same azimuth)."""
    p = a[beg:end, :3].astype(np.float64)
    a[beg:end, :3] = (p * (np.asarray(rho, np.float64) / np.linalg.norm(p, axis=1))[:, None]).astype(np.float32)


# ring lengths: 16 (skipped ring), 17 (sectors of one point: span 6), sectors of 320 | 321 (5 -> 6 a lane), 384 | 385 (6 -> 11),
# kSelSmallCap | kSelSmallCap + 1 (the second launch)
RING_LENGTHS = [16, 17, 1931, 1937, 2315, 2321, 2304, 2305]


@pytest.fixture(scope="module")
def rings64(oracle):
    """One 64-line scan at 3000 azimuth steps in the oracle's ring-sorted order (fed again as input it is its own ring-sorted cloud),
    eight of its full rings cut to RING_LENGTHS; returns (cloud, ring table, the eight rings)."""
    w = oracle.S1World(n_az=3000)
    xyzi, off = w.scans(w.trajectory(1))
    ref0 = oracle.scanreg(xyzi[off[0]:off[1]], 64, 5.0)
    cloud, rb = ref0["cloud"].copy(), ref0["ring_begin"].copy()
    full = np.flatnonzero(np.diff(rb[:65]) >= 2400)
    assert len(full) >= len(RING_LENGTHS)
    chosen = [int(r) for r in full[np.linspace(0, len(full) - 1, len(RING_LENGTHS)).astype(int)]]
    for r, n in zip(chosen, RING_LENGTHS):
        cloud[int(rb[r]) + n:int(rb[r + 1]), 0] = np.nan
    return cloud, rb, chosen


def _ring_of(ref, r):
    return int(ref["ring_begin"][r]), int(ref["ring_begin"][r + 1] - ref["ring_begin"][r])


def test_ring_and_sector_lengths(oracle, gpu_ctx, rings64):
    cloud, rb, chosen = rings64
    ref = oracle.scanreg(cloud, 64, 5.0)
    for r, n in zip(chosen, RING_LENGTHS):
        beg, got = _ring_of(ref, r)
        assert got == n
        if n >= 17:
            assert max(ep - sp + 1 for sp, ep in _sectors(n)) == (n - 11 + 5) // 6
            assert (ref["curvature"][beg + 5:beg + n - 5] > 0.1).any()
        assert not ref["label"][beg:beg + n].any() or n >= 17
    assert sorted((n - 11 + 5) // 6 for n in RING_LENGTHS[1:]) == [1, 320, 321, 383, 383, 384, 385]
    _check(gpu_ctx, cloud, np.array([0, len(cloud)], np.int64), 64, 5.0, [ref])


def test_large_curvature_at_the_first_and_last_element_of_every_sector(oracle, gpu_ctx, rings64):
    """The cut rings on a circle of 10 m, the first and the last element of every sector moved out by 0.2 m (a short step: c = 4 at the
    point): their windows are the halo -- in the full sectors of 320 and 384 points lane 0's and lane 63's loads."""
    cloud, rb, chosen = rings64
    a = cloud.copy()
    marks = []
    for r, n in zip(chosen, RING_LENGTHS):
        if n < 17:
            continue
        beg = int(rb[r])
        rho = np.full(n, 10.0)
        for sp, ep in _sectors(n):
            rho[sp] += 0.2
            if ep > sp + 12:
                rho[ep] += 0.2 + 0.001
            marks += [(r, sp), (r, ep)]
        _set_range(a, beg, beg + n, rho)
    ref = oracle.scanreg(a, 64, 5.0)
    assert [_ring_of(ref, r)[1] for r in chosen] == RING_LENGTHS
    marks = np.array([int(ref["ring_begin"][r]) + p for r, p in marks])
    big = marks[ref["curvature"][marks] > 1.0]
    assert len(big) >= 60, len(big)
    # picked as edge points: the first and the last of a long ring's, and one at least of the two that meet at each of its five borders
    assert (ref["label"][big] > 0).sum() >= 6 * 7
    g = _gaps(ref["cloud"])
    assert not g[marks].any() and not g[marks - 1].any()
    _check(gpu_ctx, a, np.array([0, len(a)], np.int64), 64, 5.0, [ref])


def test_long_gaps_around_the_sector_borders_and_between_rings(oracle, gpu_ctx, rings64):
    """A step of 1 m in range after point p, for p = sp - 5, sp - 1, ep + 1 and ep + 4 of different sectors (the outermost flags a
    sector's windows read, and the ones next to its elements), and between the last point of a ring and the first of the next."""
    cloud, rb, chosen = rings64
    a = cloud.copy()
    want = []
    for q, (r, n) in enumerate(zip(chosen, RING_LENGTHS)):
        if n < 1000:
            continue
        beg = int(rb[r])
        sec = _sectors(n)
        steps = sorted([sec[1][0] - 5, sec[2][0] - 1, sec[3][1] + 1, sec[4][1] + 4] if q % 2 == 0 else [sec[1][1] + 4, sec[2][1] + 1, sec[4][0] - 1, sec[5][0] - 5])
        rho = np.full(n, 10.0)
        for k, p in enumerate(steps):
            rho[p + 1:] = 11.0 if k % 2 == 0 else 10.0
            want.append((r, p))
        _set_range(a, beg, beg + n, rho)
    # the ring behind the longest cut ring starts 8 m further out than that ring ends
    r = chosen[RING_LENGTHS.index(2321)]
    nxt = r + 1
    assert rb[nxt + 1] - rb[nxt] > 100 and nxt not in chosen
    _set_range(a, int(rb[nxt]), int(rb[nxt]) + 1, [18.0])
    ref = oracle.scanreg(a, 64, 5.0)
    assert [_ring_of(ref, r)[1] for r in chosen] == RING_LENGTHS
    g = _gaps(ref["cloud"])
    want = np.array([int(ref["ring_begin"][r]) + p for r, p in want])
    assert len(want) == 24 and g[want].all() and not g[want - 1].any() and not g[want + 1].any()
    end = int(ref["ring_begin"][nxt]) - 1
    assert g[end] and g[end + 1]
    _check(gpu_ctx, a, np.array([0, len(a)], np.int64), 64, 5.0, [ref])


@pytest.mark.parametrize("n_lines", [16, 32, 64])
def test_sensors(oracle, gpu_ctx, n_lines):
    w = oracle.S1World(n_az=600, n_rings=n_lines)
    xyzi, off = w.scans(w.trajectory(1))
    a = xyzi[off[0]:off[1]]
    ref = oracle.scanreg(a, n_lines, 5.0 if n_lines == 64 else 0.5)
    assert (ref["label"] > 0).sum() >= n_lines and (ref["label"] < 0).sum() >= n_lines
    _check(gpu_ctx, a, np.array([0, len(a)], np.int64), n_lines, 5.0 if n_lines == 64 else 0.5, [ref])


@pytest.fixture(scope="module")
def seq16(oracle):
    w = oracle.S1World(n_az=600, n_rings=16)
    xyzi, off = w.scans(w.trajectory(4))
    return xyzi, off


def test_empty_and_tiny_scans_first_in_the_middle_and_last(oracle, gpu_ctx, seq16):
    xyzi, off = seq16
    full = [xyzi[off[k]:off[k + 1]] for k in range(2)]
    tiny = full[0][::len(full[0]) // 40][:40]
    none = np.zeros((0, 4), np.float32)
    parts = [none, tiny, full[0], none, tiny, full[1], tiny, none]
    a = np.ascontiguousarray(np.concatenate(parts))
    o = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    refs = [oracle.scanreg(p, 16, 0.5) for p in parts]
    assert refs[0]["info"].n_cloud == 0 and 0 < refs[1]["info"].n_cloud <= 40 and refs[2]["info"].n_sharp > 0
    _check(gpu_ctx, a, o, 16, 0.5, refs)


def test_curvature_calls_leave_the_odometry_alone(oracle, gpu_ctx, seq16):
    """curvature() before and after odometry(), and twice in a row: the same curvature every time, and the odometry's increments are
    those of a batch that never called it."""
    import torch
    import lmono_amd
    xyzi, off = seq16
    refs = [oracle.scanreg(xyzi[off[k]:off[k + 1]], 16, 0.5) for k in range(len(off) - 1)]
    dev = torch.from_numpy(xyzi).to("cuda:0")

    def registered():
        b = lmono_amd.ScanBatch(gpu_ctx, len(off) - 1, len(xyzi))
        b.scanreg(dev.data_ptr(), off, 16, 0.5, keepalive=dev)
        return b

    plain = registered()
    incr0, poses0 = plain.odometry(1, 0)
    b = registered()
    n = int(np.diff(off).max())

    def same(s):
        cv, lb = b.curvature(s, n)
        return np.array_equal(cv.view(np.uint32), refs[s]["curvature"].view(np.uint32)) and np.array_equal(lb, refs[s]["label"])

    assert same(2) and same(2) and same(0)
    incr1, poses1 = b.odometry(1, 0)
    assert same(3) and same(1) and same(1)
    assert incr1.tobytes() == incr0.tobytes() and poses1.tobytes() == poses0.tobytes()
    # and once more over the same registration, the curvature buffer in between
    incr2, _ = b.odometry(1, 0)
    assert incr2.tobytes() == incr0.tobytes()
    ref = oracle.run_sequence(xyzi, off, 16, 0.5)
    assert np.abs(incr0 - ref["incr"]).max() < 1e-9


def test_online_stream_for_three_steps(oracle, gpu_ctx, seq16):
    import lmono_amd
    xyzi, off = seq16
    ref = oracle.run_sequence(xyzi[:off[3]], off[:4], 16, 0.5)
    st = lmono_amd.OdomStream(gpu_ctx, int(np.diff(off).max()) + 1000, 16, 0.5, history=2)
    incr = []
    for k in range(3):
        incr.append(st.step(xyzi[off[k]:off[k + 1]])[0])
        want = oracle.scanreg(xyzi[off[k]:off[k + 1]], 16, 0.5)
        for which, name in ((1, "sharp"), (2, "less_sharp"), (3, "flat"), (4, "less_flat")):
            got = st.cloud(which, int(off[k + 1] - off[k]))
            assert np.array_equal(got.view(np.uint32), want[name].view(np.uint32)), "%s cloud of step %d differs (bitwise)" % (name, k)
    st.close()
    err = np.abs(np.stack(incr) - ref["incr"]).max()
    print("online stream: max |incr - oracle| %.3e" % err)
    assert err < 1e-9
