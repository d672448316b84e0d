"""Composing voxel maps under rigid transforms on the GPU (lmono_voxel_map_compose) against the numpy restatement of its
definition (tests/voxel_compose_ref.py): cells() as exact integers and read() as bytes, for every way the same sources can arrive."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import colour_cases as CC
from tests import voxel_compose_ref as CR
from tests import voxel_map_ref as R

pytestmark = pytest.mark.gpu

LEAF = 0.1
ECAPACITY, EINVAL = -4, -1


def _cloud(n, seed, span=3.0):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-span, span, (n, 3)).astype(np.float32)
    xyz[: n // 2] = (xyz[: n // 2] / 8.0).astype(np.float32)              # a dense half: voxels shared by several points
    return R.points(xyz, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))


def _distinct_voxels(n, leaf, seed):
    """n points in n different cells of `leaf`."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    cells = np.stack([k % 23 - 11, k // 23 - 11, k % 5], 1)
    xyz = ((cells + rng.uniform(0.1, 0.9, (n, 3))) * leaf).astype(np.float32)
    p = R.points(xyz, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
    assert len(R.VoxelMapRef(leaf).insert(p).table) == n
    return p


def _assert_equal(vm, ref):
    keys, counts, sums = vm.cells()
    rk, rc, rs = ref.cells()
    assert vm.size == len(rk)
    assert keys.tobytes() == rk.tobytes() and counts.tobytes() == rc.tobytes() and sums.tobytes() == rs.tobytes()
    assert vm.read().tobytes() == ref.read().tobytes()


def _bytes(vm):
    return [a.tobytes() for a in vm.cells()] + [vm.read().tobytes()]


def _pair(ctx, p, leaf, max_voxels=1 << 14):
    """A device map and its restatement holding the points p."""
    import lmono_amd
    vm = lmono_amd.VoxelMap(ctx, leaf=leaf, max_voxels=max_voxels)
    if len(p):
        vm.insert(p)
    return vm, R.VoxelMapRef(leaf).insert(p)


def _totals(ref):
    return [sum(r[w] for r in ref.table.values()) for w in (0, 4, 5, 6)]


CASES = {
    "identity": (lambda: [(_cloud(3000, 1), 0.1, CR.IDENTITY)]),
    "rotation_translation": (lambda: [(_cloud(3000, 2), 0.05, CR.rigid(0.7, -0.2, 0.1, (3.0, -40.5, 0.25)))]),
    "three_leaves": (lambda: [(_cloud(2500, 3), 0.05, CR.rigid(0.3, 0.0, 0.0, (0.5, 0.0, 0.0))), (_cloud(2000, 4), 0.05, CR.IDENTITY),
                              (_cloud(2500, 5), 0.2, CR.rigid(-0.2, 0.1, 0.0, (0.0, 0.25, 0.0)))]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_sources_and_transforms(gpu_ctx, case):
    import lmono_amd
    srcs = CASES[case]()
    pairs = [_pair(gpu_ctx, p, leaf) for p, leaf, _ in srcs]
    T = [t for _, _, t in srcs]
    before = [_bytes(vm) for vm, _ in pairs]
    dst = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=1 << 15)
    ref = R.VoxelMapRef(LEAF)
    want = CR.compose(ref, [r for _, r in pairs], T)
    got = dst.compose([vm for vm, _ in pairs], np.array(T).reshape(-1, 3, 4), stats=True)
    assert got.tolist() == want and want[1] == 0 and want[0] == sum(len(r.table) for _, r in pairs)
    _assert_equal(dst, ref)
    # conservation: counts and colour sums of dst are those of the source voxels
    _, counts, sums = dst.cells()
    tot = [sum(x) for x in zip(*[_totals(r) for _, r in pairs])]
    assert [int(counts.astype(np.uint64).sum())] + [int(v) for v in sums[:, 3:].sum(0)] == tot and want[2] == tot[0]
    assert [_bytes(vm) for vm, _ in pairs] == before                      # the sources are not modified
    # the same sources again: no new voxel, every sum doubles
    got = dst.compose([vm for vm, _ in pairs], T, stats=True)
    assert got.tolist() == want[:4] + [0, want[5]]
    CR.compose(ref, [r for _, r in pairs], T)
    _assert_equal(dst, ref)
    for vm, _ in pairs:
        vm.close()
    dst.close()


def test_source_sizes_around_the_tile_and_an_empty_source(gpu_ctx):
    import lmono_amd
    tile = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=2)
    assert tile.TILE == 512
    tile.close()
    sizes = [511, 0, 512, 513, 1]
    pairs = [_pair(gpu_ctx, _distinct_voxels(n, 0.05, 10 + n) if n else _cloud(0, 0), 0.05) for n in sizes]
    assert [vm.size for vm, _ in pairs] == sizes
    T = [CR.rigid(0.1 * k, 0.0, 0.0, (0.3 * k, -0.1 * k, 0.05)) for k in range(len(sizes))]
    dst = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=1 << 12)
    ref = R.VoxelMapRef(LEAF)
    want = CR.compose(ref, [r for _, r in pairs], T)
    assert dst.compose([vm for vm, _ in pairs], T, stats=True).tolist() == want and want[0] == sum(sizes)
    _assert_equal(dst, ref)
    # each size alone, into a fresh map
    for (vm, r), t, n in zip(pairs, T, sizes):
        one = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=1 << 10)
        one_ref = R.VoxelMapRef(LEAF)
        assert one.compose([vm], [t], stats=True).tolist() == CR.compose(one_ref, [r], [t])
        _assert_equal(one, one_ref)
        one.close()
    # no source, and only empty sources: successful no-ops
    assert dst.compose([], np.zeros((0, 12)), stats=True).tolist() == [0, 0, 0, 0, 0, len(ref.table)]
    assert dst.compose([pairs[1][0]], [CR.IDENTITY], stats=True).tolist() == [0, 0, 0, 0, 0, len(ref.table)]
    _assert_equal(dst, ref)
    for vm, _ in pairs:
        vm.close()
    dst.close()


def test_a_voxel_of_70000_points_needs_64_bit_products(gpu_ctx):
    """count * q = 70 000 * ~65 535 > 2^32: what a 32-bit entry or LDS word gets wrong."""
    import lmono_amd
    one = R.points([[0.31, -0.42, 0.53]], [0xFF80FF01])
    src = lmono_amd.VoxelMap(gpu_ctx, leaf=0.05, max_voxels=4)
    rep = np.repeat(one, 7000)
    for _ in range(10):
        src.insert(rep)
    src_ref = R.VoxelMapRef(0.05)
    src_ref.table = {k: [70000 * v for v in r] for k, r in R.VoxelMapRef(0.05).insert(one).table.items()}
    _assert_equal(src, src_ref)
    T = CR.rigid(t=(0.0999985 - 0.31, 0.1, 0.2))                           # the moved x lands just below a cell boundary
    dst, ref = _pair(gpu_ctx, _cloud(300, 8, span=1.0), LEAF)
    want = CR.compose(ref, [src_ref], [T])
    assert dst.compose([src], [T], stats=True).tolist() == want and want[2] == 70000
    heavy = [r for r in ref.table.values() if r[0] >= 70000]
    assert len(heavy) == 1 and heavy[0][1] > 1 << 32 and heavy[0][1] // heavy[0][0] >= 65000
    _assert_equal(dst, ref)
    src.close(); dst.close()


def test_call_orders_give_the_same_bytes(gpu_ctx):
    import lmono_amd
    srcs = CASES["three_leaves"]()
    pairs = [_pair(gpu_ctx, p, leaf) for p, leaf, _ in srcs]
    T = [t for _, _, t in srcs]
    vms = [vm for vm, _ in pairs]
    extra = _cloud(1500, 9)
    ref = R.VoxelMapRef(LEAF)
    CR.compose(ref, [r for _, r in pairs], T)
    one = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=1 << 15)
    one.compose(vms, T)
    _assert_equal(one, ref)
    for order in ((2, 0, 1), (1, 2, 0)):
        m = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=1 << 15)
        for k in order:
            m.compose([vms[k]], [T[k]])
        assert _bytes(m) == _bytes(one)
        m.close()
    # a composed map is an ordinary map: compose into inserted points == insert after the compose; and it can be a source itself
    first = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=1 << 15)
    first.insert(extra)
    first.compose(vms, T)
    one.insert(extra)
    ref.insert(extra)
    _assert_equal(one, ref)
    assert _bytes(first) == _bytes(one)
    again = lmono_amd.VoxelMap(gpu_ctx, leaf=0.25, max_voxels=1 << 15)
    again_ref = R.VoxelMapRef(0.25)
    t2 = CR.rigid(1.0, 0.2, -0.1, (-2.0, 1.0, 0.5))
    assert again.compose([one], [t2], stats=True).tolist() == CR.compose(again_ref, [ref], [t2])
    _assert_equal(again, again_ref)
    for x in vms + [one, first, again]:
        x.close()


def test_rejected_voxels_are_counted_and_a_nan_transform_is_refused(gpu_ctx):
    import lmono_amd
    p = _cloud(2000, 12)
    p["x"] = (p["x"] * np.float32(100.0)).astype(np.float32)               # +-300 m along x
    src, src_ref = _pair(gpu_ctx, p, 0.05)
    T = CR.rigid(0.0, 0.0, 0.0, (104857.6 - 100.0, 0.0, 0.0))              # part of the source lands at or beyond cell 2^20 of the 0.1 m map
    dst, ref = _pair(gpu_ctx, _cloud(200, 13), LEAF)
    want = CR.compose(ref, [src_ref], [T])
    assert want[0] > 50 and want[1] > 50 and want[3] >= want[1] and want[2] + want[3] == len(p)
    assert dst.compose([src], [T], stats=True).tolist() == want
    _assert_equal(dst, ref)
    before = _bytes(dst)
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 7, 11):
            Tb = CR.IDENTITY.copy(); Tb[at] = bad
            with pytest.raises(lmono_amd.LmonoError) as e:
                dst.compose([src], [Tb])
            assert e.value.code == EINVAL
    assert _bytes(dst) == before
    src.close(); dst.close()


def test_capacity_is_exact_all_or_nothing_and_sticky(gpu_ctx):
    import lmono_amd
    a, a_ref = _pair(gpu_ctx, _distinct_voxels(600, LEAF, 20), LEAF)
    b, b_ref = _pair(gpu_ctx, R.points([[50.05, 0.05, 0.05], [-50.05, 0.05, 0.05]], [1, 2]), LEAF)
    T = [CR.IDENTITY, CR.IDENTITY]
    src_before = _bytes(a) + _bytes(b)
    held = _cloud(40, 21, span=0.3)
    held["x"] += np.float32(20.0)                                          # away from both sources
    dst, ref = _pair(gpu_ctx, held, LEAF, max_voxels=len(R.VoxelMapRef(LEAF).insert(held).table) + 601)
    probe = R.VoxelMapRef(LEAF).insert(held)
    assert CR.compose(probe, [a_ref, b_ref], T)[5] == dst.max_voxels + 1    # needs max_voxels + 1 voxels
    before = _bytes(dst)
    with pytest.raises(lmono_amd.LmonoError) as e:
        dst.compose([a, b], T)
    assert e.value.code == ECAPACITY
    assert _bytes(dst) == before and dst.size == len(ref.table)            # nothing of either source entered
    with pytest.raises(lmono_amd.LmonoError) as e:                         # full until cleared, even for nothing at all
        dst.compose([], np.zeros((0, 12)))
    assert e.value.code == ECAPACITY
    with pytest.raises(lmono_amd.LmonoError) as e:
        dst.insert(held[:1])
    assert e.value.code == ECAPACITY
    assert _bytes(a) + _bytes(b) == src_before
    dst.clear()
    dst.insert(held)
    one = R.points([[50.05, 0.05, 0.05]], [1])
    c, c_ref = _pair(gpu_ctx, one, LEAF)
    want = CR.compose(ref, [a_ref, c_ref], T)
    assert want[5] == dst.max_voxels                                       # exactly max_voxels fit
    assert dst.compose([a, c], T, stats=True).tolist() == want
    _assert_equal(dst, ref)
    for x in (a, b, c, dst):
        x.close()


def test_bad_handles_are_refused_before_any_launch(gpu_ctx):
    import lmono_amd
    a, _ = _pair(gpu_ctx, _cloud(100, 30), LEAF)
    b, _ = _pair(gpu_ctx, _cloud(100, 31), LEAF)
    dst, ref = _pair(gpu_ctx, _cloud(100, 32), LEAF)
    before = _bytes(dst)
    for srcs in ([a, dst], [dst], [a, b, a]):
        with pytest.raises(lmono_amd.LmonoError) as e:
            dst.compose(srcs, [CR.IDENTITY] * len(srcs))
        assert e.value.code == EINVAL
    L = gpu_ctx.L
    T = np.ascontiguousarray(CR.IDENTITY)
    null = (C.c_void_p * 1)(None)
    ok = (C.c_void_p * 1)(a.h)
    assert L.lmono_voxel_map_compose(gpu_ctx.h, dst.h, 1, null, T.ctypes.data, None) == EINVAL
    assert L.lmono_voxel_map_compose(gpu_ctx.h, None, 1, ok, T.ctypes.data, None) == EINVAL
    assert L.lmono_voxel_map_compose(gpu_ctx.h, dst.h, -1, ok, T.ctypes.data, None) == EINVAL
    assert _bytes(dst) == before
    for x in (a, b, dst):
        x.close()


@pytest.fixture(scope="module")
def corridor():
    return CR.corridor_reference()


def test_submap_atlas_follows_the_corrected_poses(gpu_ctx, corridor):
    import lmono_amd
    c = CR.CORRIDOR
    atlas = lmono_amd.SubmapAtlas(gpu_ctx, c["per_submap"], leaf_sub=c["leaf_sub"], max_voxels_sub=1 << 16)
    plain = lmono_amd.VoxelMap(gpu_ctx, leaf=c["leaf"], max_voxels=1 << 16)
    for f, p in enumerate(corridor["frames"]):
        atlas.insert_frame(p, corridor["drifted"][f])
        plain.insert(p)
    frames, poses = atlas.anchors
    assert frames.tolist() == [0, 2, 4] and poses.tobytes() == corridor["drifted"][::2].tobytes()
    for sub, ref in zip(atlas.submaps, corridor["subs"]):
        _assert_equal(sub, ref)
    dst = lmono_amd.VoxelMap(gpu_ctx, leaf=c["leaf"], max_voxels=1 << 16)
    st = atlas.compose(dst, corridor["true"], stats=True)                  # one pose per frame: the anchors' are taken
    assert st.tolist() == corridor["stats"] and st[1] == 0
    _assert_equal(dst, corridor["dst"])
    per_anchor = lmono_amd.VoxelMap(gpu_ctx, leaf=c["leaf"], max_voxels=1 << 16)
    atlas.compose(per_anchor, corridor["true"][::2])
    assert _bytes(per_anchor) == _bytes(dst)
    bound = CR.corridor_bound()
    err = CR.distance_to_world(dst.read(), corridor["world"])
    drift = CR.distance_to_world(plain.read(), corridor["world"])
    print("composed max %.4f m, bound %.4f m; uncomposed max %.3f m" % (err.max(), bound, drift.max()))
    assert err.max() <= bound and drift.max() > bound
    with pytest.raises(lmono_amd.LmonoError):
        atlas.compose(dst, corridor["true"][:2])
    atlas.close(); dst.close(); plain.close(); per_anchor.close()


def _moving_frame(k, w, h):
    cloud = CC.s1_scan(n_rings=32, n_az=600, k=k)
    bgr = CC.noise_image(h, w, seed=100 + k)
    q = np.round(np.array([0.01 * k, -0.02, np.sin(0.05 * k), np.cos(0.05 * k)]), 6)
    return cloud, bgr, q, np.round(np.array([0.8 * k, 0.1 * k, 0.02 * k]), 6)


def test_cpp_map_build_writes_the_global_map(gpu_ctx, tmp_path):
    """map_build ... submap=2:corrected.txt voxel=0.1 writes rgb_map_global.ply, equal to the Python chain over the same frames; rgb_map_voxel.ply and
    rgb_map10.ply are what the same command line without submap= writes."""
    import lmono_amd
    from lmono_amd import kitti_io as IO
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lmono_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "map_build"])
    w, h, n = 320, 96, 11
    fx = fy = 185.0; cx = 156.5; cy = 47.25
    seq = tmp_path / "seq"; out = tmp_path / "out"; out0 = tmp_path / "out0"
    os.makedirs(seq / "velodyne"); os.makedirs(seq / "image_bgr"); os.makedirs(out); os.makedirs(out0)
    qt = np.zeros((n, 7)); fixed = np.zeros((n, 7))
    frames = []
    for k in range(n):
        cloud, bgr, q, t = _moving_frame(k, w, h)
        IO.write_velodyne_bin(IO.velodyne_path(str(seq), k), cloud)
        (seq / "image_bgr" / ("%06d.bgr" % k)).write_bytes(bgr.tobytes())
        qt[k, :4] = q; qt[k, 4:] = t
        yaw = 0.004 * k
        fixed[k, :4] = np.round(np.array([0.01 * k, -0.02, np.sin(0.05 * k + yaw), np.cos(0.05 * k + yaw)]), 6)
        fixed[k, 4:] = np.round(t + np.array([0.0, 0.03 * k, -0.01 * k]), 6)
        frames.append((cloud, bgr))
    IO.write_trajectory(str(tmp_path / "traj.txt"), 50.0 + 0.1 * np.arange(n), qt)
    IO.write_trajectory(str(tmp_path / "corrected.txt"), 50.0 + 0.1 * np.arange(n), fixed)
    traj = IO.read_trajectory(str(tmp_path / "traj.txt"))[:, 1:]           # x y z qx qy qz qw, as the program parses them
    corrected = IO.read_trajectory(str(tmp_path / "corrected.txt"))[:, 1:]
    M = CC.lidar_to_camera()
    mb = lmono_amd.MapBuilder(gpu_ctx, lmono_amd.Camera(w, h, fx, fy, cx, cy, 0, 0, 0, 0, 5, 0, 0), max_cloud_points=1 << 16)
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=0.1, max_voxels=1 << 18)
    atlas = lmono_amd.SubmapAtlas(gpu_ctx, 2, leaf_sub=0.05, max_voxels_sub=1 << 18)
    for k, (cloud, bgr) in enumerate(frames):
        mb.associate(cloud, M, bgr, traj[k, 3:], traj[k, :3])
        vm.insert_frame(mb)
        atlas.insert_frame(mb, traj[k])
        if (k + 1) % 10 == 0:
            mb.clear()                                                     # processMapping's every-tenth-frame clear
    glob = lmono_amd.VoxelMap(gpu_ctx, leaf=0.1, max_voxels=1 << 18)
    st = atlas.compose(glob, corrected, stats=True)
    assert st[1] == 0 and len(atlas.submaps) == 6
    base = [os.path.join(host, "map_build"), str(seq), str(tmp_path / "traj.txt")]
    cam = [str(n), str(w), str(h), repr(fx), repr(fy), repr(cx), repr(cy)]
    txt = subprocess.check_output(base + [str(out)] + cam + ["submap=2:%s:0.05" % (tmp_path / "corrected.txt"), "voxel=0.1:%d" % (1 << 18)], text=True).strip().split("\n")
    txt0 = subprocess.check_output(base + [str(out0)] + cam + ["voxel=0.1:%d" % (1 << 18)], text=True).strip().split("\n")
    assert len(txt) == n and txt[9].endswith("wrote " + IO.rgb_map_path(str(out), 10)) and len(txt0) == n
    want = glob.read()
    assert len(want) > 1000 and IO.read_ply_binary(str(out / "rgb_map_global.ply")).tobytes() == want.tobytes()
    assert want.tobytes() != vm.read().tobytes()
    assert IO.read_ply_binary(str(out / "rgb_map_voxel.ply")).tobytes() == vm.read().tobytes()
    for name in ("rgb_map_voxel.ply", "rgb_map10.ply"):
        assert (out / name).read_bytes() == (out0 / name).read_bytes()
    assert not (out0 / "rgb_map_global.ply").exists()
    for x in (vm, glob, mb):
        x.close()
    atlas.close()
