"""k_lm_solve keeps a chain's staged residual blocks in LDS (LMONO_LM_LDS_PLANES=4, the A/B side) or in the batch's scratch (the shipped
instantiation).  Where the blocks live must not move a bit of the result: every case runs through two contexts, one created under
LMONO_LM_LDS_PLANES=4 and one under the shipped value, and compares increments and poses byte for byte; the strictly sequential run is
also held to the 1e-9 of the oracle that tests/test_lidar_gpu.py uses.  The inputs are built so that the ORACLE alone shows each case's
precondition (block counts per pair, pairs without a block, edge-only / plane-only pairs, a boundary that does not agree); the builders
and those checks need no GPU."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_LM_T = 256          # threads of a k_lm_solve workgroup: a thread evaluates the blocks tid, tid + 256, ...
THIN_STRIDE, THIN_BLOCKS = 4, 18      # kThinStride, kThinBlocks (= 2304 / 128) of odometry.hip


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs (CPU only)
def _ring_and_bin(w, xyzi):
    elev = np.arctan2(xyzi[:, 2].astype(np.float64), np.hypot(xyzi[:, 0].astype(np.float64), xyzi[:, 1].astype(np.float64)))
    ring = np.abs(elev[:, None] - np.asarray(w.elev)[None, :]).argmin(axis=1)
    az = np.arctan2(xyzi[:, 1].astype(np.float64), xyzi[:, 0].astype(np.float64))
    return ring, np.floor((np.pi - az) / (2 * np.pi / w.n_az)).astype(np.int64)        # the generator's rays: az = pi - (k + 0.5) * step


def _select(xyzi, off, keep):
    scan_of = np.searchsorted(off, np.arange(len(xyzi)), side="right") - 1
    off2 = np.concatenate([[0], np.cumsum(np.bincount(scan_of[keep], minlength=len(off) - 1))]).astype(off.dtype)
    return np.ascontiguousarray(xyzi[keep]), off2


def seq_rings64(oracle, n=12):
    """A dozen 64-ring scans at 500 azimuth steps: more than 1024 blocks per pair (several trips per thread)."""
    w = oracle.S1World(n_az=500)
    xyzi, off = w.scans(w.trajectory(n))
    return dict(xyzi=xyzi, off=off, n_lines=64, min_range=5.0)


def seq_rings16(oracle, n=6):
    """16-ring scans: a few hundred blocks per pair, no multiple of 256."""
    w = oracle.S1World(n_az=600, n_rings=16)
    xyzi, off = w.scans(w.trajectory(n))
    return dict(xyzi=xyzi, off=off, n_lines=16, min_range=5.0, world=w)


def seq_few_rings(oracle, n=5):
    """Six neighbouring rings of the 16 (+1.7 to -11.7 degrees: structure and ground): at most 256 blocks, one trip."""
    s = seq_rings16(oracle, n)
    ring, _ = _ring_and_bin(s["world"], s["xyzi"])
    xyzi, off = _select(s["xyzi"], s["off"], np.isin(ring, (5, 6, 7, 8, 9, 10)))
    return dict(xyzi=xyzi, off=off, n_lines=16, min_range=5.0)


def seq_no_block_pair(oracle, n=5):
    """Scan 0 is 40 neighbouring points of ONE ring: its less-flat cloud is empty (no plane block) and an edge needs a second point on
    another ring (no edge block), so the pair (0, 1) has no usable block at all; the pairs behind it are ordinary."""
    s = seq_rings16(oracle, n)
    xyzi, off = s["xyzi"], s["off"]
    ring, _ = _ring_and_bin(s["world"], xyzi[off[0]:off[1]])
    first = np.flatnonzero(ring == 8)[:40]
    assert len(first) == 40
    xyzi2 = np.concatenate([xyzi[first], xyzi[off[1]:]])
    off2 = np.concatenate([[0], off[1:] - off[1] + 40]).astype(off.dtype)
    return dict(xyzi=np.ascontiguousarray(xyzi2), off=off2, n_lines=16, min_range=5.0)


def _room(oracle, n_az):
    """The sensor inside a 36 m x 28 m room of four 40 m high walls, no noise, no dropouts: every ray returns, every ring is a closed curve."""
    w = oracle.S1World(n_az=n_az, n_rings=16, range_sigma=0.0, dropout=0.0)
    t = 1.0
    w.boxes[:] = 0.0
    w.boxes[:4] = [[-18 - t, -14 - t, -1.73, -18, 14 + t, 40], [18, -14 - t, -1.73, 18 + t, 14 + t, 40],
                   [-18 - t, -14 - t, -1.73, 18 + t, -14, 40], [-18 - t, 14, -1.73, 18 + t, 14 + t, 40]]
    w.boxes[4:] = [500.0, 500.0, -1.73, 500.1, 500.1, -1.7]          # the other boxes and the poles: out of range
    w.cyls[:, :2] = 500.0
    return w


def _room_poses(n):
    k = np.arange(n, dtype=np.float64)
    return np.stack([-3.0 + 0.5 * k, -2.0 + 0.2 * k, np.zeros(n), 0.2 + 0.03 * k], 1)


def seq_plane_only(oracle, n=4):
    """The room as a 1 : 20 model (coordinates x 0.05, min_range 0.25) at 1200 azimuth steps: curvature is a squared length, so every
    corner's falls below the 0.1 a sharp point needs.  No scan has a sharp point: n_edge = 0, every block is a plane block."""
    w = _room(oracle, 1200)
    xyzi, off = w.scans(_room_poses(n))
    xyzi = xyzi.copy()
    xyzi[:, :3] *= np.float32(0.05)
    return dict(xyzi=xyzi, off=off, n_lines=16, min_range=0.25)


def seq_edge_only(oracle, n=4):
    """The room at 2000 azimuth steps with the range of every other step stretched by 2 %: of a point's ten neighbours the six of the
    other parity lie 2 % of its range off it, 0.12 of the range in sum (at 2000 steps the room's own corners add less), so curvature is
    above (0.12 x 5 m)^2 > 0.1 everywhere.  No scan has a flat point: n_edge = nq, every block is an edge block."""
    w = _room(oracle, 2000)
    xyzi, off = w.scans(_room_poses(n))
    _, b = _ring_and_bin(w, xyzi)
    xyzi = xyzi.copy()
    xyzi[:, :3] *= np.where(b % 2 == 0, 1.02, 1.0).astype(np.float32)[:, None]
    return dict(xyzi=xyzi, off=off, n_lines=16, min_range=5.0)


def block_counts(oracle, s):
    """(n_edge, nq) of every scan as k_lm_solve sees them: sharp points, sharp + flat points."""
    out = []
    for k in range(len(s["off"]) - 1):
        f = oracle.scanreg(s["xyzi"][s["off"][k]:s["off"][k + 1]], s["n_lines"], s["min_range"])
        out.append((int(f["info"].n_sharp), int(f["info"].n_sharp + f["info"].n_flat)))
    return out


def pair_blocks_from_identity(oracle, s, k):
    """Edge and plane blocks the oracle finds for the pair (k - 1, k) from the identity, both outer iterations."""
    f = [oracle.scanreg(s["xyzi"][s["off"][j]:s["off"][j + 1]], s["n_lines"], s["min_range"]) for j in (k - 1, k)]
    _, _, st, _ = oracle.odom_step(f[1]["sharp"], f[1]["flat"], f[0]["less_sharp"], f[0]["less_flat"], [0, 0, 0, 1], [0, 0, 0])
    return list(st.n_corner_corr), list(st.n_plane_corr)


def chain_bounds(n, n_chains, c):
    return c * n // n_chains, (c + 1) * n // n_chains


def thinned_pairs(n, n_chains, lead, lead_full):
    """(chain, k) of the lead-in pairs that run on every fourth workgroup's share of the features (lead_in_thinned of odometry.hip)."""
    out = []
    for c in range(n_chains):
        s, _ = chain_bounds(n, n_chains, c)
        for k in range(max(s - lead, 0) + 1, s):
            if s - k > lead_full:
                out.append((c, k))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx_pair():
    """(context created under LMONO_LM_LDS_PLANES=4, context created under the shipped value)"""
    import torch
    import lmono_amd
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    old = os.environ.get("LMONO_LM_LDS_PLANES")
    try:
        os.environ["LMONO_LM_LDS_PLANES"] = "4"
        in_lds = lmono_amd.Context(0)
        del os.environ["LMONO_LM_LDS_PLANES"]
        shipped = lmono_amd.Context(0)
    finally:
        if old is None:
            os.environ.pop("LMONO_LM_LDS_PLANES", None)
        else:
            os.environ["LMONO_LM_LDS_PLANES"] = old
    return in_lds, shipped


def _register(ctx, s):
    import torch
    import lmono_amd
    dev = torch.from_numpy(np.ascontiguousarray(s["xyzi"])).to("cuda:0")
    batch = lmono_amd.ScanBatch(ctx, len(s["off"]) - 1, max(len(s["xyzi"]), 1))
    batch.scanreg(dev.data_ptr(), s["off"], s["n_lines"], s["min_range"], keepalive=dev)
    return batch


def _same_bytes(a, b):
    return a.tobytes() == b.tobytes()


def _sequential_on_both(oracle, ctx_pair, s):
    """The sequential run on both contexts: byte-equal, and within 1e-9 of the oracle.  Returns the oracle's result."""
    ref = oracle.run_sequence(s["xyzi"], s["off"], s["n_lines"], s["min_range"])
    res = [_register(c, s).odometry(1, 0) for c in ctx_pair]
    assert _same_bytes(res[0][0], res[1][0]) and _same_bytes(res[0][1], res[1][1])
    err = np.abs(res[1][0] - ref["incr"]).max()
    print("sequential: max |incr - oracle| %.3e" % err)
    assert err < 1e-9
    return ref


def test_pair_without_a_usable_block(oracle, ctx_pair):
    s = seq_no_block_pair(oracle)
    assert pair_blocks_from_identity(oracle, s, 1) == ([0, 0], [0, 0])           # n_used = 0: the solve leaves the warm start alone
    edges, planes = pair_blocks_from_identity(oracle, s, 2)
    assert min(edges) > 10 and min(planes) > 50                                   # and the next pair is an ordinary one
    ref = _sequential_on_both(oracle, ctx_pair, s)
    assert np.array_equal(ref["incr"][1], [0, 0, 0, 1, 0, 0, 0])


def test_one_trip(oracle, ctx_pair):
    s = seq_few_rings(oracle)
    nq = [n for _, n in block_counts(oracle, s)[1:]]
    assert 0 < min(nq) and max(nq) <= K_LM_T, nq
    _sequential_on_both(oracle, ctx_pair, s)


def test_several_trips_the_last_one_ragged(oracle, ctx_pair):
    s = seq_rings16(oracle)
    nq = [n for _, n in block_counts(oracle, s)[1:]]
    assert all(K_LM_T < n <= 4 * K_LM_T and n % K_LM_T for n in nq), nq
    _sequential_on_both(oracle, ctx_pair, s)


def test_more_than_1024_blocks(oracle, ctx_pair):
    s = seq_rings64(oracle, 4)
    cnt = block_counts(oracle, s)[1:]
    assert all(n > 1024 for _, n in cnt), cnt
    assert any(e % K_LM_T and n % K_LM_T for e, n in cnt)                        # the edge loop hands over to the plane loop inside a trip
    _sequential_on_both(oracle, ctx_pair, s)


def test_plane_only_pairs(oracle, ctx_pair):
    s = seq_plane_only(oracle)
    cnt = block_counts(oracle, s)
    assert all(e == 0 and n > K_LM_T for e, n in cnt), cnt
    _sequential_on_both(oracle, ctx_pair, s)


def test_edge_only_pairs(oracle, ctx_pair):
    s = seq_edge_only(oracle)
    cnt = block_counts(oracle, s)
    assert all(e == n and n > 0 for e, n in cnt), cnt
    edges, planes = pair_blocks_from_identity(oracle, s, 1)
    assert min(edges) > 10 and planes == [0, 0]
    _sequential_on_both(oracle, ctx_pair, s)


def test_chained_run_with_a_thinned_lead_in(oracle, ctx_pair):
    """4 chains over a dozen scans, lead-in of 3 pairs of which the last one runs on all features: stale records of the workgroups a
    thinned pair does not run must be skipped wherever the blocks are staged.  The validated result is the sequential one."""
    s = seq_rings64(oracle, 12)
    n, n_chains, lead, lead_full = 12, 4, 3, 1
    thin = thinned_pairs(n, n_chains, lead, lead_full)
    assert len({c for c, _ in thin}) >= 2, thin
    res = []
    for c in ctx_pair:
        batch = _register(c, s)
        c.set_option(c.OPT_LEAD_FULL, lead_full)
        try:
            res.append(batch.odometry(n_chains, lead))
        finally:
            c.set_option(c.OPT_LEAD_FULL, -1)
    assert _same_bytes(res[0][0], res[1][0]) and _same_bytes(res[0][1], res[1][1])
    ref = oracle.run_sequence(s["xyzi"], s["off"])
    print("4 chains, lead 3, lead_full 1: max |incr - oracle| %.3e" % np.abs(res[1][0] - ref["incr"]).max())
    assert np.abs(res[1][0] - ref["incr"]).max() < 1e-4            # the bound of a repaired layout in tests/test_lidar_gpu.py


def test_flagged_boundaries_are_repaired_through_the_chain_list(oracle, ctx_pair):
    """3 chains with a lead-in of one pair from the identity: the oracle's plain chained schedule shows that the boundaries do not
    agree with the sequential run, so the validation flags them and the repair launches address the chains through the list."""
    s = seq_rings64(oracle, 12)
    seq = oracle.run_sequence(s["xyzi"], s["off"])
    plain = oracle.run_sequence(s["xyzi"], s["off"], n_chains=3, lead=1)
    assert np.abs(plain["incr"] - seq["incr"]).max() > 1e-4
    res, reps = [], []
    for c in ctx_pair:
        batch = _register(c, s)
        res.append(batch.odometry(3, 1))
        reps.append(batch.boundary_report())
    for rep in reps:
        print("flagged %d, chains re-run %d, pairs re-run %d, unresolved %d" % (rep["flagged"], rep["chains_rerun"], rep["pairs_rerun"], rep["unresolved"]))
        assert rep["flagged"] >= 1 and rep["pairs_rerun"] >= 1 and rep["unresolved"] == 0
    assert reps[0]["flagged"] == reps[1]["flagged"] and reps[0]["pairs_rerun"] == reps[1]["pairs_rerun"]
    assert _same_bytes(res[0][0], res[1][0]) and _same_bytes(res[0][1], res[1][1])
    assert np.abs(res[1][0] - seq["incr"]).max() < 1e-4


def test_two_batches_alive_on_one_context(oracle, ctx_pair):
    """The scratch belongs to the batch, the LDS attribute to the kernel: two batches of one context stepped alternately, with
    different chain counts (the second call grows the first batch's workspace), give what each gives alone."""
    sa, sb = seq_rings64(oracle, 12), seq_rings16(oracle)
    alone = (_register(ctx_pair[0], sa).odometry(1, 0), _register(ctx_pair[0], sb).odometry(1, 0))
    for c in ctx_pair:
        a, b = _register(c, sa), _register(c, sb)
        for n_chains in (1, 3, 1):
            ra, rb = a.odometry(n_chains, 3 if n_chains > 1 else 0), b.odometry(1, 0)
            assert _same_bytes(rb[0], alone[1][0]) and _same_bytes(rb[1], alone[1][1])
            if n_chains == 1:
                assert _same_bytes(ra[0], alone[0][0]) and _same_bytes(ra[1], alone[0][1])
            else:
                assert np.abs(ra[0] - alone[0][0]).max() < 1e-4
