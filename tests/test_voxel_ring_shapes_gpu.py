"""k_voxel (the voxel-grid filter of the less-flat cloud, one workgroup per ring) on the ring shapes at which its code takes another
path, bit for bit against the CPU oracle through ScanBatch.scanreg / cloud(s, 4, n) / counts().

Every case first asserts its precondition on the oracle's output alone (ring-sorted cloud, labels and ring table, from which the
candidates, cells, segments, runs and buckets of a ring are recomputed in numpy as the kernel defines them), so a case cannot silently
stop covering its branch.  The candidates of ring r are its points 5 .. len - 7 with label <= 0; a cell is the 0.2 m voxel inside the
ring's bounding box; a segment is a maximal run of consecutive candidates of one cell; the small instantiation sorts segments into
2048 buckets of the cell index (11 bits below the top of the ring's cell count).

Which path a ring takes in the kernel as it stands: up to 2304 points, up to 2^31 cells -> first instantiation (9 register slots,
bucket sort, whatever the number of segments up to 2304); more points, or more cells -> work list of the second instantiation
(16 slots), which bucket-sorts up to 1024 segments and 2^32 cells and runs the bitonic network otherwise."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BUCKET_BITS = 11


def _ring_stats(ref, r):
    """Candidates, cells, segments and buckets of ring r, from the oracle's output alone."""
    rb = ref["ring_begin"]
    beg, end = int(rb[r]), int(rb[r + 1])
    n = end - beg
    st = dict(len=n, nseg=0, runs=np.zeros(0, np.int64), heads=np.zeros(0, np.int64), ncell=0, max_bucket=0, max_voxel_segs=0)
    if n - 11 < 6:
        return st
    p = ref["cloud"][beg:end]
    i = np.arange(n)
    cand = (i >= 5) & (i <= n - 7) & (ref["label"][beg:end] <= 0)
    if not cand.any():
        return st
    five = np.float32(5.0)
    fl = np.floor(p[:, :3] * five)                                   # float32, as the kernel: floorf(x * 5.0f)
    minb = fl[cand].min(0).astype(np.int64)
    maxb = fl[cand].max(0).astype(np.int64)
    div = maxb - minb + 1
    ncell = int(div[0]) * int(div[1]) * int(div[2])
    ijk = (fl - minb.astype(np.float32)).astype(np.int64)
    cell = ijk[:, 0] + ijk[:, 1] * int(div[0]) + ijk[:, 2] * int(div[0]) * int(div[1])
    cont = cand.copy()
    cont[0] = False
    cont[1:] &= cand[:-1] & (cell[1:] == cell[:-1])
    head = cand & ~cont
    heads = np.flatnonzero(head)
    # run length of a head: up to the next point that does not continue
    stop = np.flatnonzero(~cont)                                      # every index whose bit is 0
    nxt = np.searchsorted(stop, heads, side="right")
    ends = np.where(nxt < len(stop), stop[np.minimum(nxt, len(stop) - 1)], n)
    runs = ends - heads
    cell_bits = (ncell - 1).bit_length() if ncell > 1 else 0
    bshift = max(cell_bits - BUCKET_BITS, 0)
    hc = cell[heads]
    st.update(nseg=len(heads), runs=runs, heads=heads, ncell=ncell)
    if ncell <= 2 ** 32:
        st["max_bucket"] = int(np.bincount(hc >> bshift).max())
        st["max_voxel_segs"] = int(np.unique(hc, return_counts=True)[1].max())
    return st


def _all_stats(ref, n_lines):
    return [_ring_stats(ref, r) for r in range(n_lines)]


def _check(oracle, gpu_ctx, xyzi, off, n_lines, min_range, refs):
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
        assert list(cnt[s, 1:5]) == [info.n_sharp, info.n_less_sharp, info.n_flat, info.n_less_flat]
        got = batch.cloud(s, 4, n)
        assert np.array_equal(got.view(np.uint32), ref["less_flat"].view(np.uint32)), "less-flat cloud of scan %d differs (bitwise)" % s


def _ring_major(oracle, xyzi, n_lines, min_range):
    """The scan in the oracle's ring-sorted order (what the ring sort keeps, ring after ring), its ring table with it: fed again as
    input it is its own ring-sorted cloud, so points can be addressed by (ring, position in the ring)."""
    ref = oracle.scanreg(xyzi, n_lines, min_range)
    return ref["cloud"].copy(), ref["ring_begin"].copy()


@pytest.fixture(scope="module")
def scan16(oracle):
    """One 16-line scan at 2000 azimuth steps, ring-major."""
    w = oracle.S1World(n_az=2000, n_rings=16)
    xyzi, off = w.scans(w.trajectory(1))
    return _ring_major(oracle, xyzi[off[0]:off[1]], 16, 0.5)


def test_long_runs(oracle, gpu_ctx, scan16):
    """Every ring pulled in to a circle of 0.6 m around the sensor (min_range 0.5): about 100 consecutive points per 0.2 m cell, so the
    run lengths come from more than one word of the continuation bitmap.  A cell of 0.2 m at 0.6 m holds at most some 125 of a ring's
    1900 points, so in three rings a stretch of 150, 200 and 300 consecutive points is put onto the stretch's first point as well."""
    cloud, rb = scan16
    a = cloud.copy()
    rho = np.hypot(a[:, 0].astype(np.float64), a[:, 1].astype(np.float64))
    a[:, :3] = (a[:, :3].astype(np.float64) * (0.6 / rho)[:, None]).astype(np.float32)
    for r, first, count in ((2, 100, 150), (4, 700, 200), (7, 1111, 300)):
        beg = int(rb[r])
        assert rb[r + 1] - beg > first + count + 100
        a[beg + first:beg + first + count, :3] = a[beg + first, :3]
    ref = oracle.scanreg(a, 16, 0.5)
    sts = _all_stats(ref, 16)
    runs = np.concatenate([s["runs"] for s in sts])
    heads = np.concatenate([s["heads"] for s in sts])
    last = heads + runs - 1
    assert runs.max() >= 130, runs.max()                                         # longer than two bitmap words
    assert (runs > 15).any()
    assert ((heads // 64) != (last // 64)).any(), "no run crosses a multiple of 64"
    assert ((heads // 256) != (last // 256)).any(), "no run crosses a multiple of 256"
    assert (runs > 64).sum() >= 100
    off = np.array([0, len(a)], np.int64)
    _check(oracle, gpu_ctx, a, off, 16, 0.5, [ref])


def test_every_run_of_length_one(oracle, gpu_ctx, scan16):
    """Every second point of every ring moved radially by +-15 %: neighbours never share a cell, every candidate is a segment.  Scan 0
    keeps the whole rings (more than 1024 segments, at most 2304 points), scan 1 the first 1000 points of every ring (at most 1024
    segments); both are sorted by the first instantiation's bucket sort, whose capacity is the ring."""
    cloud, rb = scan16
    rng = np.random.default_rng(5)
    a = cloud.copy()
    pos = np.arange(len(a)) - np.repeat(rb[:16], np.diff(rb[:17]))               # position inside the ring
    sgn = rng.choice(np.array([-1.0, 1.0], np.float32), len(a))
    scale = np.where(pos % 2 == 1, np.float32(1.0) + np.float32(0.15) * sgn, np.float32(1.0)).astype(np.float32)
    a[:, :3] *= scale[:, None]
    b = a.copy()
    b[pos >= 1000, 0] = np.nan
    ra, rfb = oracle.scanreg(a, 16, 0.5), oracle.scanreg(b, 16, 0.5)
    sa, sb = _all_stats(ra, 16), _all_stats(rfb, 16)
    long_ones = [s for s in sa if s["nseg"] > 1024 and s["len"] <= 2304 and s["runs"].max() == 1]
    short_ones = [s for s in sb if 0 < s["nseg"] <= 1024 and s["len"] > 900 and s["runs"].max() == 1]
    assert len(long_ones) >= 1, [(s["len"], s["nseg"]) for s in sa]
    assert len(short_ones) >= 1, [(s["len"], s["nseg"]) for s in sb]
    cat = np.concatenate([a, b], 0)
    off = np.array([0, len(a), len(a) + len(b)], np.int64)
    _check(oracle, gpu_ctx, cat, off, 16, 0.5, [ra, rfb])


def test_two_cells_in_turn(oracle, gpu_ctx, scan16):
    """A B A B: 600 consecutive points of three rings alternate between two points of one ray, half a metre apart: two voxels of
    300 segments each, all of them in one or two buckets."""
    cloud, rb = scan16
    a = cloud.copy()
    for r in (3, 6, 7):
        beg = int(rb[r])
        assert rb[r + 1] - beg > 1200
        pa = a[beg + 300, :3].astype(np.float64)
        rho = np.linalg.norm(pa)
        assert rho > 3.0
        pb = pa * (1.0 + 0.5 / rho)
        blk = np.where((np.arange(600) % 2 == 0)[:, None], pa[None, :], pb[None, :]).astype(np.float32)
        a[beg + 300:beg + 900, :3] = blk
    ref = oracle.scanreg(a, 16, 0.5)
    sts = _all_stats(ref, 16)
    assert max(s["max_voxel_segs"] for s in sts) >= 100, [s["max_voxel_segs"] for s in sts]
    assert max(s["max_bucket"] for s in sts) >= 100, [s["max_bucket"] for s in sts]
    off = np.array([0, len(a)], np.int64)
    _check(oracle, gpu_ctx, a, off, 16, 0.5, [ref])


RING_LENGTHS = [17, 18, 255, 256, 257, 1024, 1025, 2304, 2305, 16]


def test_ring_lengths(oracle, gpu_ctx):
    """Rings cut to 17 (the shortest with a sector), 18, 255 / 256 / 257 (one register slot), 1024 / 1025 (four slots), 2304 (all nine),
    2305 (handed to the second instantiation) and 16 points (no sector: no output) by masking the rest of the ring to NaN."""
    w = oracle.S1World(n_az=3000)
    xyzi, off = w.scans(w.trajectory(1))
    cloud, rb = _ring_major(oracle, xyzi[off[0]:off[1]], 64, 5.0)
    full = np.flatnonzero(np.diff(rb[:65]) >= 2400)
    assert len(full) >= len(RING_LENGTHS)
    a = cloud.copy()
    chosen = full[np.linspace(0, len(full) - 1, len(RING_LENGTHS)).astype(int)]
    for r, want in zip(chosen, RING_LENGTHS):
        a[int(rb[r]) + want:int(rb[r + 1]), 0] = np.nan
    ref = oracle.scanreg(a, 64, 5.0)
    lens = np.diff(ref["ring_begin"][:65])
    for r, want in zip(chosen, RING_LENGTHS):
        assert lens[r] == want, (r, lens[r], want)
    sts = _all_stats(ref, 64)
    for r, want in zip(chosen, RING_LENGTHS):
        assert (sts[r]["nseg"] > 0) == (want >= 17), (want, sts[r]["nseg"])
    off1 = np.array([0, len(a)], np.int64)
    _check(oracle, gpu_ctx, a, off1, 64, 5.0, [ref])


def test_bounding_box_of_more_than_2_32_cells(oracle, gpu_ctx, scan16):
    """Two stretches of 60 points of a ring moved out to 10 km along their rays, in opposite directions (a single far point has the
    largest curvature of its sector and is labelled sharp: no candidate): the ring's box has more than 2^32 cells, which no bucket sort
    takes (bitonic network of the second instantiation)."""
    cloud, rb = scan16
    a = cloud.copy()
    for r in (4, 7):
        beg, end = int(rb[r]), int(rb[r + 1])
        az = np.arctan2(a[beg:end, 1], a[beg:end, 0])
        for target in (np.pi / 4, -3 * np.pi / 4):
            k = beg + 100 + int(np.argmin(np.abs(az[100:-100] - target)))
            p = a[k - 30:k + 30, :3].astype(np.float64)
            a[k - 30:k + 30, :3] = (p * (10000.0 / np.linalg.norm(p, axis=1))[:, None]).astype(np.float32)
    ref = oracle.scanreg(a, 16, 0.5)
    sts = _all_stats(ref, 16)
    assert sum(1 for s in sts if s["ncell"] > 2 ** 32) >= 1, [s["ncell"] for s in sts]
    off = np.array([0, len(a)], np.int64)
    _check(oracle, gpu_ctx, a, off, 16, 0.5, [ref])


@pytest.mark.parametrize("n_lines", [16, 32, 64])
def test_sensors(oracle, gpu_ctx, n_lines):
    w = oracle.S1World(n_az=600, n_rings=n_lines)
    xyzi, off = w.scans(w.trajectory(1))
    mr = 5.0 if n_lines == 64 else 0.5
    ref = oracle.scanreg(xyzi[off[0]:off[1]], n_lines, mr)
    sts = _all_stats(ref, n_lines)
    assert sum(1 for s in sts if s["nseg"] > 0) >= n_lines // 2
    assert ref["info"].n_less_flat > 0
    _check(oracle, gpu_ctx, xyzi[off[0]:off[1]], np.array([0, off[1] - off[0]], np.int64), n_lines, mr, [ref])
