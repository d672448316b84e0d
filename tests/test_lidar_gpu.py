"""Parity of the HIP LiDAR path (through the C ABI) against the CPU oracle on identical seeded inputs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _register(gpu_ctx, xyzi, off, n_lines=64, min_range=5.0):
    import torch
    import lmono_amd
    dev = torch.from_numpy(np.ascontiguousarray(xyzi)).to("cuda:0")
    batch = lmono_amd.ScanBatch(gpu_ctx, len(off) - 1, max(len(xyzi), 1))
    batch.scanreg(dev.data_ptr(), off, n_lines, min_range, keepalive=dev)
    return batch


def _check_scanreg(oracle, batch, xyzi, off, n_lines=64, min_range=5.0):
    cnt = batch.counts()
    for s in range(len(off) - 1):
        ref = oracle.scanreg(xyzi[off[s]:off[s + 1]], n_lines, min_range)
        n = off[s + 1] - off[s]
        info = ref["info"]
        assert cnt[s, 0] == info.n_cloud
        assert list(cnt[s, 1:5]) == [info.n_sharp, info.n_less_sharp, info.n_flat, info.n_less_flat]
        cloud = batch.cloud(s, 0, int(n))
        assert np.array_equal(cloud.view(np.uint32), ref["cloud"].view(np.uint32)), "ring-sorted cloud differs (bitwise)"
        cv, lb = batch.curvature(s, int(n))
        assert np.array_equal(cv.view(np.uint32), ref["curvature"].view(np.uint32)), "curvature differs (bitwise)"
        assert np.array_equal(lb, ref["label"]), "labels differ"
        for which, name in ((1, "sharp"), (2, "less_sharp"), (3, "flat"), (4, "less_flat")):
            got = batch.cloud(s, which, int(n))
            assert np.array_equal(got.view(np.uint32), ref[name].view(np.uint32)), name + " differs (bitwise)"


def test_scanreg_bit_exact_small(oracle, gpu_ctx, small_seq):
    batch = _register(gpu_ctx, small_seq["xyzi"], small_seq["off"])
    _check_scanreg(oracle, batch, small_seq["xyzi"], small_seq["off"])
    assert (batch.counts()[:, 5] == 0).all()


def test_scanreg_bit_exact_full_resolution(oracle, gpu_ctx, full_seq):
    batch = _register(gpu_ctx, full_seq["xyzi"], full_seq["off"])
    _check_scanreg(oracle, batch, full_seq["xyzi"], full_seq["off"])


def test_scanreg_edge_cases(oracle, gpu_ctx, small_seq):
    """NaNs, points inside minimum range, an empty scan, a scan too small for any sector, shuffled (non ring-major) input."""
    xyzi, off = small_seq["xyzi"], small_seq["off"]
    a = xyzi[off[0]:off[1]].copy()
    a[::97, 0] = np.nan
    a[5::101, :3] *= 0.01
    rng = np.random.default_rng(3)
    b = xyzi[off[1]:off[2]].copy()
    rng.shuffle(b, axis=0)                         # azimuth-major / random order: stable ring sort still defined
    c = np.zeros((0, 4), np.float32)               # empty scan
    d = xyzi[off[2]:off[2] + 40].copy()            # 40 points: no ring long enough
    e = xyzi[off[3]:off[4]].copy()
    parts = [a, b, c, d, e]
    cat = np.concatenate(parts, 0)
    o = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    batch = _register(gpu_ctx, cat, o)
    _check_scanreg(oracle, batch, cat, o)


def _boundary_scan(n_lines, rng, base):
    """Points placed ON and next to every decision threshold of the ring sort: the elevation angles at which ring_of changes its answer
    (and the discard limits), azimuths at the three half-sweep thresholds relative to the scan's first point, x = y = 0, and points whose
    first / last 300 are invalid.  Offsets from 0 to 3e-3 deg / 1e-4 rad straddle the guard bands (2e-3 deg, 4e-5 rad) of k_ring_tag, so
    both the single-precision decisions and the fp64 forms run."""
    if n_lines == 64:
        edges = [2.0 - (k - 0.5) / 3.0 for k in range(0, 34)] + [-8.83 - (k - 0.5) / 2.0 for k in range(0, 34)] + [2.0, -24.33, -8.83]
    elif n_lines == 32:
        edges = [(k + 0.0) * 4.0 / 3.0 - 92.0 / 3.0 for k in range(-1, 34)]
    else:
        edges = [(k - 0.5) * 2.0 - 15.0 for k in range(-1, 18)]
    deltas = np.array([0.0, 1e-7, 1e-6, 1e-5, 1e-4, 5e-4, 1.5e-3, 2.5e-3, 3e-3])
    ang = np.array([e + sgn * d for e in edges for d in deltas for sgn in (-1.0, 1.0)])
    ang = np.repeat(ang, 3)
    az = rng.uniform(-np.pi, np.pi, len(ang))
    rho = rng.uniform(6.0, 60.0, len(ang))
    pts = np.stack([rho * np.cos(az), rho * np.sin(az), rho * np.tan(np.radians(ang)), rng.uniform(0, 1, len(ang))], 1).astype(np.float32)
    # azimuth thresholds: ori = -atan2(y, x); start azimuth = that of the scan's first valid point (base[0] after the invalid head)
    x0, y0 = float(base[0, 0]), float(base[0, 1])
    start = -np.arctan2(y0, x0)
    d_az = np.array([0.0, 1e-7, 1e-6, 1e-5, 3e-5, 5e-5, 1e-4])
    oris = np.array([start + t + sgn * d for t in (np.pi, -np.pi / 2, 1.5 * np.pi, -np.pi, 0.5 * np.pi) for d in d_az for sgn in (-1.0, 1.0)])
    oris = np.repeat(oris, 4)
    rho2 = rng.uniform(8.0, 40.0, len(oris))
    el = np.radians(rng.uniform(-20.0, 1.5, len(oris)) if n_lines == 64 else rng.uniform(-14.0, 14.0, len(oris)))
    thr = np.stack([rho2 * np.cos(-oris), rho2 * np.sin(-oris), rho2 * np.tan(el), rng.uniform(0, 1, len(oris))], 1).astype(np.float32)
    axis = np.array([[0, 0, 7.0, 0.5], [0, 0, -9.0, 0.5], [0.0, 1e-20, 8.0, 0.1]], np.float32)        # x = y = 0 (and a denormal radius)
    dead = np.tile(np.array([[0.5, 0.2, -0.1, 0.0]], np.float32), (300, 1))                           # inside min_range
    mid = np.concatenate([base[1:], pts, thr, axis], 0)
    rng.shuffle(mid, axis=0)
    return np.concatenate([dead, base[:1], mid, dead], 0)


@pytest.mark.parametrize("n_lines", [64, 32, 16])
def test_scanreg_at_the_ring_and_half_sweep_thresholds(oracle, gpu_ctx, n_lines):
    """k_ring_tag decides ring id and half sweep from single-precision angles inside proven margins and from the fp64 forms next to a
    threshold: a scan made of threshold points (plus an invalid head and tail, so that the first / last valid point are far from the ends)
    must still come out bit for bit as the oracle's."""
    rng = np.random.default_rng(64 + n_lines)
    w = oracle.S1World(n_az=500, n_rings=n_lines)
    xyzi, off = w.scans(w.trajectory(2))
    mr = 5.0 if n_lines == 64 else 0.5
    scans = []
    for s in range(2):
        base = xyzi[off[s]:off[s + 1]]
        r2 = (base[:, :3].astype(np.float64) ** 2).sum(1)
        base = base[r2 > (mr + 1.0) ** 2]
        scans.append(_boundary_scan(n_lines, rng, base))
    cat = np.concatenate(scans, 0)
    o = np.concatenate([[0], np.cumsum([len(p) for p in scans])]).astype(np.int64)
    batch = _register(gpu_ctx, cat, o, n_lines, mr)
    _check_scanreg(oracle, batch, cat, o, n_lines, mr)
    assert batch.counts()[:, 0].min() > 1000


@pytest.mark.parametrize("n_lines", [16, 32])
def test_scanreg_other_sensors(oracle, gpu_ctx, n_lines):
    w = oracle.S1World(n_az=600, n_rings=n_lines)
    xyzi, off = w.scans(w.trajectory(2))
    batch = _register(gpu_ctx, xyzi, off, n_lines, 0.5)
    _check_scanreg(oracle, batch, xyzi, off, n_lines, 0.5)


def test_scanreg_long_rings_take_the_second_voxel_kernel(oracle, gpu_ctx):
    """Rings of more than 2304 points (azimuth step 0.12 deg) and rings with more than 1024 voxel segments (points scattered
    over many 0.2 m cells) are handed to k_voxel's second instantiation (work list, bitonic network): still bit-exact."""
    w = oracle.S1World(n_az=3000)
    xyzi, off = w.scans(w.trajectory(2))
    a = xyzi[off[0]:off[1]].copy()
    b = xyzi[off[1]:off[2]].copy()
    # scan b: radial jitter of +-3 m on every second point: neighbouring ring points fall into different voxels
    rng = np.random.default_rng(11)
    scale = 1.0 + (rng.uniform(-0.15, 0.15, len(b)) * (np.arange(len(b)) % 2)).astype(np.float32)
    b[:, :3] *= scale[:, None]
    cat = np.concatenate([a, b], 0)
    o = np.array([0, len(a), len(a) + len(b)], np.int64)
    batch = _register(gpu_ctx, cat, o)
    _check_scanreg(oracle, batch, cat, o)


def test_correspondences_match_oracle(oracle, gpu_ctx, small_seq):
    xyzi, off = small_seq["xyzi"], small_seq["off"]
    batch = _register(gpu_ctx, xyzi, off)
    f = [oracle.scanreg(xyzi[off[s]:off[s + 1]]) for s in range(3)]
    q = np.array([0.0, 0.0, 0.01, 1.0]); q /= np.linalg.norm(q)
    t = np.array([0.7, 0.02, 0.0])
    for k in (1, 2):
        _, _, _, corr = oracle.odom_step(f[k]["sharp"], f[k]["flat"], f[k - 1]["less_sharp"], f[k - 1]["less_flat"], q, t, want_corr=True)
        got = batch.correspond(k, q, t)
        assert np.array_equal(got, corr[0]), "correspondence indices differ at scan %d" % k


def test_search_formulations_agree_in_the_diagnostic_build(gpu_ctx):
    """The product library compiles the default search only (every LMONO_OPT_CORR_TILE but 3 is refused); its equality with the round-1
    hash-grid search runs against the diagnostic build of the same sources in a child process (tests/diag_search_modes.py)."""
    import os
    import subprocess
    import sys
    import lmono_amd
    with pytest.raises(lmono_amd.LmonoError):
        gpu_ctx.set_option(gpu_ctx.OPT_CORR_TILE, 0)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    diag = os.path.join(root, "lmono_amd", "lib", "liblmono_hip_diag.so")
    assert os.path.exists(diag), "run __graft_entry__.build() first: it also builds the diagnostic library"
    env = dict(os.environ, LMONO_HIP_LIB=diag)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "diag_search_modes.py"), "-m", "gpu", "-x", "-q"],
                         capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "4 passed" in out.stdout


def test_odometry_sequential_matches_oracle(oracle, gpu_ctx, small_seq):
    xyzi, off = small_seq["xyzi"], small_seq["off"]
    batch = _register(gpu_ctx, xyzi, off)
    incr, poses = batch.odometry(1, 0)
    ref = oracle.run_sequence(xyzi, off)
    # fp64 solve, different summation order only: 1e-9 m / 1e-9 on quaternion components
    assert np.abs(incr - ref["incr"]).max() < 1e-9
    assert np.abs(poses - ref["poses"]).max() < 1e-8
    assert oracle.ate(poses, ref["poses"]) < 1e-8


def test_odometry_chain_sharded_matches_oracle(oracle, gpu_ctx, small_seq):
    """The oracle's chained schedule is the plain one (lead-in from the identity, nothing validated): compared with the boundary
    validation off.  With it on (default) the same layout is repaired to the strictly sequential result."""
    xyzi, off = small_seq["xyzi"], small_seq["off"]
    batch = _register(gpu_ctx, xyzi, off)
    gpu_ctx.set_option(gpu_ctx.OPT_BOUNDARY_TOL, 0)
    try:
        incr, poses = batch.odometry(3, 2)
    finally:
        gpu_ctx.set_option(gpu_ctx.OPT_BOUNDARY_TOL, 1000)
    ref = oracle.run_sequence(xyzi, off, n_chains=3, lead=2)
    assert np.abs(incr - ref["incr"]).max() < 1e-9
    assert np.abs(poses - ref["poses"]).max() < 1e-8
    incr_v, _ = batch.odometry(3, 2)
    seq = oracle.run_sequence(xyzi, off)
    assert np.abs(incr_v - seq["incr"]).max() < 1e-4 and np.abs(incr - seq["incr"]).max() > 1e-4


@pytest.mark.parametrize("n_lines,min_range", [(16, 0.5), (32, 0.5), (64, 0.5)])
def test_odometry_other_sensors_and_near_points(oracle, gpu_ctx, n_lines, min_range):
    """The (scan line, azimuth bin) search on 16- / 32-line sensors and with points from 0.5 m on (feature points close to the sensor
    axis: their search balls cover every azimuth): correspondences of every search mode and the sequential odometry against the oracle."""
    w = oracle.S1World(n_az=600, n_rings=n_lines)
    xyzi, off = w.scans(w.trajectory(5))
    batch = _register(gpu_ctx, xyzi, off, n_lines, min_range)
    f = [oracle.scanreg(xyzi[off[s]:off[s + 1]], n_lines, min_range) for s in range(3)]
    q = np.array([0.0, 0.0, 0.008, 1.0]); q /= np.linalg.norm(q)
    t = np.array([0.75, -0.01, 0.0])
    for k in (1, 2):
        _, _, _, corr = oracle.odom_step(f[k]["sharp"], f[k]["flat"], f[k - 1]["less_sharp"], f[k - 1]["less_flat"], q, t, want_corr=True)
        try:
            for mode in (3,):          # the other formulations: tests/diag_search_modes.py (diagnostic build)
                gpu_ctx.set_option(gpu_ctx.OPT_CORR_TILE, mode)
                assert np.array_equal(batch.correspond(k, q, t), corr[0]), "mode %d, scan %d" % (mode, k)
        finally:
            gpu_ctx.set_option(gpu_ctx.OPT_CORR_TILE, 3)
    incr, poses = batch.odometry(1, 0)
    ref = oracle.run_sequence(xyzi, off, n_lines, min_range)
    assert np.abs(incr - ref["incr"]).max() < 1e-9 and np.abs(poses - ref["poses"]).max() < 1e-8


def test_odometry_dense_rings(oracle, gpu_ctx):
    """3000 azimuth steps per ring (rings beyond the small-slice kernels' 2304 points, denser azimuth bins): sequential odometry and the
    correspondences of the default search against the oracle."""
    w = oracle.S1World(n_az=3000)
    xyzi, off = w.scans(w.trajectory(3))
    batch = _register(gpu_ctx, xyzi, off)
    assert (batch.counts()[:, 5] == 0).all()
    incr, poses = batch.odometry(1, 0)
    ref = oracle.run_sequence(xyzi, off)
    assert np.abs(incr - ref["incr"]).max() < 1e-9 and np.abs(poses - ref["poses"]).max() < 1e-8
    f = [oracle.scanreg(xyzi[off[s]:off[s + 1]]) for s in range(2)]
    q = np.array([0.0, 0.0, 0.0, 1.0]); t = np.array([0.0, 0.0, 0.0])      # identity warm start: the largest search radii
    _, _, _, corr = oracle.odom_step(f[1]["sharp"], f[1]["flat"], f[0]["less_sharp"], f[0]["less_flat"], q, t, want_corr=True)
    assert np.array_equal(batch.correspond(1, q, t), corr[0])


def test_line_index_full_width_counters_for_huge_clouds(oracle, gpu_ctx, full_seq):
    """k_line_index counts in 16-bit halves; a less-flat cloud of more than 65535 points goes through its work list to the 32-bit
    launch.  Scans stretched by 4 (0.2 m voxels merge almost nothing any more) have such clouds: same correspondences and odometry."""
    xyzi = full_seq["xyzi"].copy(); off = full_seq["off"]
    xyzi[:, :3] *= 4.0
    batch = _register(gpu_ctx, xyzi, off)
    cnt = batch.counts()
    assert (cnt[:, 4] > 65535).all(), cnt[:, 4]
    f = [oracle.scanreg(xyzi[off[s]:off[s + 1]]) for s in range(2)]
    q = np.array([0.0, 0.0, 0.004, 1.0]); q /= np.linalg.norm(q)
    t = np.array([2.9, 0.0, 0.0])
    _, _, _, corr = oracle.odom_step(f[1]["sharp"], f[1]["flat"], f[0]["less_sharp"], f[0]["less_flat"], q, t, want_corr=True)
    assert np.array_equal(batch.correspond(1, q, t), corr[0])
    incr, poses = batch.odometry(1, 0)
    ref = oracle.run_sequence(xyzi, off)
    assert np.abs(incr - ref["incr"]).max() < 1e-8


def test_chain_groups_on_streams_change_nothing(gpu_ctx, small_seq):
    """LMONO_OPT_ODOM_STREAMS on a small batch: groups need >= 32 chains each, so 6 chains stay on one stream whatever the option
    says (the grouped path itself is checked at 256 chains in test_full_sequence_gpu.py); same increments bit for bit."""
    xyzi, off = small_seq["xyzi"], small_seq["off"]
    batch = _register(gpu_ctx, xyzi, off)
    ref_i, ref_p = batch.odometry(6, 2)
    try:
        for g in (2, 4):
            gpu_ctx.set_option(gpu_ctx.OPT_ODOM_STREAMS, g)
            i, p = batch.odometry(6, 2)
            assert np.array_equal(i, ref_i) and np.array_equal(p, ref_p)
    finally:
        gpu_ctx.set_option(gpu_ctx.OPT_ODOM_STREAMS, 4)       # the library default


def test_odometry_full_resolution(oracle, gpu_ctx, full_seq):
    xyzi, off = full_seq["xyzi"], full_seq["off"]
    batch = _register(gpu_ctx, xyzi, off)
    incr, poses = batch.odometry(1, 0)
    ref = oracle.run_sequence(xyzi, off)
    assert np.abs(incr - ref["incr"]).max() < 1e-9
    # the estimate must also be physically right: ~0.8 m forward per scan
    assert 0.6 < incr[2, 4] < 1.0


def test_pose_prefix_and_rebase_kernels(gpu_ctx):
    """k_pose_prefix / k_pose_rebase against the numpy mirror in lmono_amd.sharding (the N > 1 exchange path)."""
    import torch
    from lmono_amd import sharding
    rng = np.random.default_rng(5)
    n = 300
    q = np.concatenate([rng.normal(0, 0.02, (n, 3)), np.ones((n, 1))], 1); q /= np.linalg.norm(q, axis=1, keepdims=True)
    incr = np.concatenate([q, rng.normal([0.8, 0, 0], 0.05, (n, 3))], 1)
    incr[0] = sharding.IDENTITY
    d_incr = torch.from_numpy(incr).cuda()
    for first in (0, 7):
        d_pose = torch.zeros((n - first, 7), dtype=torch.float64, device="cuda")
        gpu_ctx.pose_prefix_d(d_incr.data_ptr(), first, n, d_pose.data_ptr())
        torch.cuda.synchronize()
        ref = sharding.prefix(incr, first)
        assert np.abs(d_pose.cpu().numpy() - ref).max() < 1e-12
    bases = incr[1:4].copy()
    d_b = torch.from_numpy(bases).cuda()
    gpu_ctx.pose_rebase_d(d_b.data_ptr(), 3, d_pose.data_ptr(), n - 7)
    torch.cuda.synchronize()
    assert np.abs(d_pose.cpu().numpy() - sharding.rebase(bases, ref)).max() < 1e-12


def test_two_rank_sharded_run_matches_unsharded():
    """N > 1 path end to end on the GPU kernels: 2 processes (gloo rendezvous, both on cuda:0) vs one batch."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533", os.path.join(root, "scripts", "shard_check.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.count("max |pose - unsharded|") == 2


def test_bench_multi_rank_step_rehearsed_on_one_gpu():
    """bench.py's N > 1 step end to end -- scan-range shards, the deferred rank-boundary validation, the pose exchange, the reductions of
    time and tolerance -- with two ranks on cuda:0 and the collectives over gloo (LMONO_BENCH_REHEARSE=1).  The run checks itself against the
    committed trajectory of the sequential CPU path; here: it finishes, reports two ranks and stays within the tolerance."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LMONO_BENCH_REHEARSE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29537",
           os.path.join(root, "bench.py"), "--gpus", "2", "--scans", "96", "--chains", "8", "--steps", "2", "--warmup", "1", "--full", "--no-extras", "--cpu-sample", "0"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["config"]["scans_total"] == 192 and d["scaling"] == "weak"
    assert d["parity"]["scans_compared"] == 192 and d["parity"]["feature_counts_equal"]
    assert d["ate_vs_cpu_m"] < 1e-3, d["ate_vs_cpu_m"]
    assert d["boundary_validation"]["unresolved"] == 0 and d["boundary_validation"]["rank_boundary_rounds"] >= 1
    print("2-rank rehearsal: %.0f scans/s (not a measurement), ATE vs CPU %.2e m, rank-boundary rounds %s"
          % (d["value"], d["ate_vs_cpu_m"], d["boundary_validation"]["rank_boundary_rounds"]))


def test_bench_strong_scaling_step_rehearsed_with_four_ranks():
    """`bench.py --gpus N --scaling strong` as the driver's SCALE tier launches it, rehearsed with FOUR ranks on cuda:0 over gloo (the GPU box
    admits six GPU processes of ours at once; this pytest process and the launcher are two of them, so 8 ranks cannot be rehearsed on one card): the
    4541 scans of configs[1] sharded into four scan ranges, three rank boundaries validated through the deferred rank-boundary validation, chains per rank by
    the rule of bench.py (chain length >= 3 x lead), parity against the committed sequential trajectory over ALL 4541 scans."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LMONO_BENCH_REHEARSE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1", "--master-port", "29541",
           os.path.join(root, "bench.py"), "--gpus", "4", "--scaling", "strong", "--steps", "2", "--warmup", "1", "--full", "--no-extras", "--cpu-sample", "0"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 4 and d["scaling"] == "strong" and d["config"]["scans_total"] == 4541
    assert d["parity"]["scans_compared"] == 4541 and d["parity"]["feature_counts_equal"]
    assert d["ate_vs_cpu_m"] < 1e-3, d["ate_vs_cpu_m"]                   # the 1 cm bar of north_star with a factor 10 in hand
    assert d["boundary_validation"]["unresolved"] == 0 and d["boundary_validation"]["rank_boundary_rounds"] >= 1
    print("4-rank strong-scaling rehearsal on one GPU: ATE vs CPU %.2e m over %d scans, chains per rank %s, rank-boundary rounds %s"
          % (d["ate_vs_cpu_m"], d["parity"]["scans_compared"], d["config"].get("odometry_chains_per_gpu"), d["boundary_validation"]["rank_boundary_rounds"]))


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain bench run prints the headline line without the --full figures, and --dump-outputs writes the last timed step's outputs as
    float64 .npy files: the same bytes in a second run, the poses and increments of --dump-poses."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    for k in range(2):
        d = tmp_path / ("out%d" % k)
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--scans", "96", "--chains", "8", "--steps", "3", "--warmup", "1",
               "--dump-outputs", str(d), "--dump-poses", str(tmp_path / ("poses%d.npz" % k))]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
        line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
        runs.append((line, {f[:-4]: np.load(d / f) for f in os.listdir(d)}, np.load(tmp_path / ("poses%d.npz" % k))))
    (a, da, pa), (_, db, _) = runs
    assert a["steps"] == 3 and a["ms_per_step"] > 0 and a["unit"] == "scans/s" and a["higher_is_better"] is True
    for key in ("parity", "ate_vs_cpu_m", "ate_vs_truth_m", "sequential", "latency", "streamed", "secondary", "cpu_baseline"):
        assert key not in a, key
    assert sorted(da) == ["boundary_residual", "incr", "poses", "scan_counts"]
    assert da["poses"].shape == (96, 7) and da["incr"].shape == (96, 7) and da["scan_counts"].shape == (96, 6)
    for name in da:
        assert da[name].dtype == np.float64 and da[name].tobytes() == db[name].tobytes(), name
    assert da["poses"].tobytes() == pa["poses"].tobytes() and da["incr"].tobytes() == pa["incr"].tobytes()


def test_api_errors_and_limits(oracle, gpu_ctx, small_seq):
    import torch
    import lmono_amd
    xyzi, off = small_seq["xyzi"], small_seq["off"]
    dev = torch.from_numpy(xyzi).cuda()
    b = lmono_amd.ScanBatch(gpu_ctx, 2, 10)                        # capacity: 2 scans, 10 points
    with pytest.raises(lmono_amd.LmonoError):
        b.scanreg(dev.data_ptr(), off[:3], 64, 5.0)                 # too many points -> LMONO_ECAPACITY
    b = lmono_amd.ScanBatch(gpu_ctx, 8, len(xyzi))
    with pytest.raises(lmono_amd.LmonoError):
        b.odometry(1, 0)                                            # odometry before registration -> LMONO_EINVAL
    with pytest.raises(lmono_amd.LmonoError):
        b.scanreg(dev.data_ptr(), off, 48, 5.0)                     # n_lines must be 16 / 32 / 64
    b.scanreg(dev.data_ptr(), off, 64, 5.0, keepalive=dev)
    gpu_ctx.set_option(gpu_ctx.OPT_BOUNDARY_TOL, 0)                 # the oracle's chained schedule validates nothing
    incr, poses = b.odometry(1000, 2)                               # n_chains is clamped to the number of scans
    gpu_ctx.set_option(gpu_ctx.OPT_BOUNDARY_TOL, 1000)
    ref = oracle.run_sequence(xyzi, off, n_chains=len(off) - 1, lead=2)
    assert np.abs(incr - ref["incr"]).max() < 1e-9
    one = lmono_amd.ScanBatch(gpu_ctx, 1, len(xyzi))
    one.scanreg(dev.data_ptr(), off[:2], 64, 5.0, keepalive=dev)
    incr, poses = one.odometry(1, 0)                                # a single scan: identity
    assert np.array_equal(incr, np.array([[0, 0, 0, 1, 0, 0, 0.0]])) and np.array_equal(poses, incr)
    # options: values are range-checked, a rejected value leaves the option as it was, values may be negative
    for key, bad in ((gpu_ctx.OPT_CORR_TILE, 4), (gpu_ctx.OPT_CORR_TILE, -1), (gpu_ctx.OPT_CORR_TILE, 1), (gpu_ctx.OPT_BA_CLUSTER, 3), (gpu_ctx.OPT_BA_CLUSTER, 16), (gpu_ctx.OPT_LEAD_SEED, 2), (gpu_ctx.OPT_LEAD_SEED, -1), (gpu_ctx.OPT_ODOM_STREAMS, 0), (gpu_ctx.OPT_ODOM_STREAMS, 9),
                     (gpu_ctx.OPT_DEFER_EVERY, -1), (gpu_ctx.OPT_LEAD_FULL, -2), (gpu_ctx.OPT_BOUNDARY_TOL, -1), (17, 0)):
        before = gpu_ctx.get_option(key) if key < 7 else None
        with pytest.raises(lmono_amd.LmonoError):
            gpu_ctx.set_option(key, bad)
        if before is not None:
            assert gpu_ctx.get_option(key) == before
    assert gpu_ctx.get_option(gpu_ctx.OPT_LEAD_FULL) == -1


def test_ring_longer_than_kernel_limit_is_flagged(gpu_ctx):
    """A ring with more than LMONO_RING_CAP = 4096 points sets status bit 1 for that scan and contributes no features."""
    import torch
    import lmono_amd
    n = 6000
    az = np.linspace(-3.1, 3.1, n)
    elev = np.deg2rad(-5.0)
    pts = np.stack([20 * np.cos(elev) * np.cos(az), 20 * np.cos(elev) * np.sin(az), np.full(n, 20 * np.sin(elev)), np.zeros(n)], 1).astype(np.float32)
    dev = torch.from_numpy(pts).cuda()
    b = lmono_amd.ScanBatch(gpu_ctx, 1, n)
    b.scanreg(dev.data_ptr(), np.array([0, n], np.int64), 64, 5.0, keepalive=dev)
    cnt = b.counts()
    assert cnt[0, 0] == n and cnt[0, 5] & 1 and cnt[0, 1] == 0 and cnt[0, 3] == 0


def test_points_beyond_the_grid_code_range_are_flagged_not_fatal(oracle, gpu_ctx, small_seq):
    """A return 1500 m away lies outside the +-1024 m range of the hash grid's 32-bit cell code: the table page of that
    scan is written empty and status bit 2 is set; the run terminates and the other scans are unaffected."""
    xyzi, off = small_seq["xyzi"].copy(), small_seq["off"]
    a = xyzi[off[1]:off[2]]
    # stretch a stretch of one ring radially (same direction, same ring id): smooth, so some of it survives as less-flat
    a[200:260, :3] *= (1500.0 / np.linalg.norm(a[200:260, :3], axis=1))[:, None].astype(np.float32)
    batch = _register(gpu_ctx, xyzi, off)
    incr, poses = batch.odometry(1, 0)
    cnt = batch.counts()
    assert np.isfinite(incr).all() and np.isfinite(poses).all()
    assert (cnt[[0, 2, 3], 5] & 2 == 0).all()


def test_full_size_batch_properties(gpu_ctx, oracle):
    """32 full-resolution scans (size-independent properties at bench scale): sharp is a prefix-subset of less_sharp per
    sector, counts respect the per-sector caps, labels agree with the clouds, poses have unit quaternions."""
    import torch
    import lmono_amd
    w = oracle.S1World()
    xyzi, off = w.scans(w.trajectory(32, speed=8.0), scan_id0=1000)
    dev = torch.from_numpy(xyzi).cuda()
    b = lmono_amd.ScanBatch(gpu_ctx, 32, len(xyzi))
    b.scanreg(dev.data_ptr(), off, keepalive=dev)
    cnt = b.counts()
    assert (cnt[:, 5] == 0).all()
    assert (cnt[:, 1] <= 51 * 6 * 2).all() and (cnt[:, 2] <= 51 * 6 * 20).all() and (cnt[:, 3] <= 51 * 6 * 4).all()
    for s in (0, 17, 31):
        n = int(off[s + 1] - off[s])
        cv, lb = b.curvature(s, n)
        assert (lb == 2).sum() == cnt[s, 1] and ((lb == 2) | (lb == 1)).sum() == cnt[s, 2] and (lb == -1).sum() == cnt[s, 3]
        assert (cv[lb > 0] > 0.1).all() and (cv[lb == -1] < 0.1).all()
        sharp = b.cloud(s, 1, n); ls = b.cloud(s, 2, n)
        keys = {p.tobytes() for p in ls}
        assert all(p.tobytes() in keys for p in sharp)
    incr, poses = b.odometry(4, 3)
    assert np.abs(np.linalg.norm(poses[:, :4], axis=1) - 1).max() < 1e-9
    fwd = incr[1:, 4]
    assert (fwd > 0.5).all() and (fwd < 1.1).all()                  # ~0.8 m per scan


@pytest.mark.parametrize("n_lines,n_az,min_range", [(64, 500, 5.0), (64, 2000, 5.0), (32, 1800, 0.5), (16, 600, 0.5)])
def test_fall_back_search_changes_nothing_in_any_schedule(oracle, gpu_ctx, n_lines, n_az, min_range):
    """LMONO_OPT_DEFER_EVERY hands every n-th feature point of the default search to its fall-back kernel (k_correspond_list on the same
    (azimuth bin, scan line) index, no hash grid): bit-identical increments -- sequential, chained with a thinned lead-in and repairs, and
    from bad warm starts (the first pair of every chain starts from the identity)."""
    w = oracle.S1World(n_az=n_az, n_rings=n_lines)
    xyzi, off = w.scans(w.trajectory(8))
    batch = _register(gpu_ctx, xyzi, off, n_lines, min_range)
    out = {}
    try:
        for every in (0, 3, 7):
            gpu_ctx.set_option(gpu_ctx.OPT_DEFER_EVERY, every)
            gpu_ctx.timing_reset()
            res = [batch.odometry(1, 0)[0]]
            gpu_ctx.set_option(gpu_ctx.OPT_LEAD_FULL, 1)
            res.append(batch.odometry(4, 2)[0])
            gpu_ctx.set_option(gpu_ctx.OPT_LEAD_FULL, -1)
            res.append(batch.odometry(2, 3)[0])
            deferred = gpu_ctx.timing()[0]["deferred_features"]
            assert (deferred > 0) == (every > 0)
            out[every] = res
    finally:
        gpu_ctx.set_option(gpu_ctx.OPT_LEAD_FULL, -1)
        gpu_ctx.set_option(gpu_ctx.OPT_DEFER_EVERY, 0)
    for every in (3, 7):
        for a, b_ in zip(out[0], out[every]):
            assert np.array_equal(a, b_)
    ref = oracle.run_sequence(xyzi, off, n_lines, min_range)
    assert np.abs(out[0][0] - ref["incr"]).max() < 1e-9


def test_odometry_workspace_regrown_for_more_chains(oracle, gpu_ctx):
    """One batch runs the odometry with one chain and then with two: the workspace is allocated again at the larger size (the outgrown one
    stays with the batch).  The two-chain increments equal those of a fresh batch that only ever ran two chains."""
    w = oracle.S1World(n_az=500)
    xyzi, off = w.scans(w.trajectory(4))
    batch = _register(gpu_ctx, xyzi, off)
    one, _ = batch.odometry(1, 0)
    two, _ = batch.odometry(2, 1)
    fresh = _register(gpu_ctx, xyzi, off)
    ref, _ = fresh.odometry(2, 1)
    assert two.tobytes() == ref.tobytes()
    assert np.abs(one[1:, 4:]).max() > 0.1 and np.abs(two[1:, 4:]).max() > 0.1      # both runs found the motion (~0.8 m per scan)
    batch.close(); fresh.close()
