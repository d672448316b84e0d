"""The voxel-grid global colour map on the GPU (lmono_voxel_map_*) against the numpy restatement of its definition
(tests/voxel_map_ref.py): cells() as exact integers and read() as bytes, for every way the same points can arrive."""
import os
import subprocess

import numpy as np
import pytest

from tests import colour_cases as CC
from tests import voxel_map_ref as R

pytestmark = pytest.mark.gpu

LEAF = 0.1
ECAPACITY, EINVAL = -4, -1


def _cloud(n, seed, span=3.0):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-span, span, (n, 3)).astype(np.float32)
    xyz[: n // 2] = (xyz[: n // 2] / 8.0).astype(np.float32)              # a dense half: voxels shared by several points
    return R.points(xyz, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))


def _assert_equal(vm, ref):
    keys, counts, sums = vm.cells()
    rk, rc, rs = ref.cells()
    assert vm.size == len(rk)
    assert keys.tobytes() == rk.tobytes() and counts.tobytes() == rc.tobytes() and sums.tobytes() == rs.tobytes()
    assert vm.read().tobytes() == ref.read().tobytes()


def _one_voxel(n=5000):
    rng = np.random.default_rng(11)
    return R.points(rng.uniform(7.3001, 7.3999, (n, 3)).astype(np.float32), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))


def _all_different(n=5000):
    k = np.arange(n)
    xyz = np.stack([(k % 71 - 35) * 8.45 + 0.05, (k // 71 - 35) * 8.45 + 0.05, (k % 13) * 0.31 - 2.0], 1).astype(np.float32)
    return R.points(xyz, (k * 2654435761 % (1 << 32)).astype(np.uint32))


def _extreme_colours():
    p = _cloud(700, 21)
    p["bgra"] = np.where(np.arange(700) % 3 == 0, 0xFFFFFFFF, 0).astype(np.uint32)
    p["bgra"][:50] = 0x00FFFFFF                                            # alpha of the input is not kept
    return p


SHAPES = {
    "n1": lambda t: _cloud(1, 1), "n63": lambda t: _cloud(63, 2), "n64": lambda t: _cloud(64, 3), "n65": lambda t: _cloud(65, 4),
    "tile-1": lambda t: _cloud(t - 1, 5), "tile": lambda t: _cloud(t, 6), "tile+1": lambda t: _cloud(t + 1, 7),
    "one_voxel": lambda t: _one_voxel(), "all_different": lambda t: _all_different(), "colours": lambda t: _extreme_colours(),
    "edges": lambda t: R.edge_points(LEAF), "edges_and_rejected": lambda t: np.concatenate([R.rejected_points(), R.edge_points(LEAF), R.rejected_points()]),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_smallest_shapes(gpu_ctx, shape):
    import lmono_amd
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=8192)
    assert vm.TILE >= 64
    p = SHAPES[shape](vm.TILE)
    ref = R.VoxelMapRef(LEAF).insert(p)
    if shape == "one_voxel":
        assert len(ref.table) == 1
    if shape == "all_different":
        assert len(ref.table) == len(p)
    stats = vm.insert(p)
    assert stats.tolist() == [len(p) - ref.rejected, ref.rejected, len(ref.table), len(ref.table)]
    _assert_equal(vm, ref)
    # the same points again: no new voxel, every sum doubles
    stats = vm.insert(p)
    assert stats.tolist() == [len(p) - ref.rejected, ref.rejected, 0, len(ref.table)]
    _assert_equal(vm, ref.insert(p))
    vm.close()


def test_a_call_of_rejected_points_and_an_empty_call(gpu_ctx):
    import lmono_amd
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=16)
    bad = R.rejected_points()
    assert vm.insert(bad).tolist() == [0, len(bad), 0, 0]
    assert vm.size == 0 and len(vm.read()) == 0 and len(vm.cells()[0]) == 0
    assert vm.insert(bad[:0]).tolist() == [0, 0, 0, 0]
    vm.close()
    for leaf, mv in ((0.0, 8), (-0.1, 8), (float("nan"), 8), (float("inf"), 8), (0.1, 0), (0.1, (1 << 30) + 1)):
        with pytest.raises(lmono_amd.LmonoError):
            lmono_amd.VoxelMap(gpu_ctx, leaf=leaf, max_voxels=mv)


def _cells_starting_at(slot, slots, count, seed):
    """`count` cells within +-300 m whose keys start their probe at `slot` of a `slots`-slot table (by the restated mix)."""
    rng = np.random.default_rng(seed)
    cells = rng.integers(-2999, 3000, (4096, 3))
    cells = cells[(R.mix(R.key_of(cells)) & np.uint64(slots - 1)) == np.uint64(slot)][:count]
    assert len(cells) == count
    return cells


def _points_in(cells, per_cell, seed):
    rng = np.random.default_rng(seed)
    xyz = ((np.repeat(cells, per_cell, 0) + rng.uniform(0.1, 0.9, (per_cell * len(cells), 3))) * 0.1).astype(np.float32)
    return R.points(xyz, rng.integers(0, 1 << 32, len(xyz), dtype=np.uint64).astype(np.uint32))


@pytest.mark.parametrize("form", [1, 0])
def test_tiny_table_probes_collide_and_wrap(gpu_ctx, monkeypatch, form):
    """max_voxels = 4 (8 slots): three voxels whose probes start at the LAST slot and one that starts at slot 0, spread over +-300 m.  Whatever the
    order, the keys end in slots 7, 0, 1, 2: every probe but one collides, and at least two step from slot 7 to slot 0.  Asserted on the numpy
    restatement of the mix, so the test cannot silently stop covering the wrap."""
    import lmono_amd
    cells = np.concatenate([_cells_starting_at(7, 8, 3, seed=1), _cells_starting_at(0, 8, 1, seed=2)])
    p = _points_in(cells, 40, seed=3)
    p = p[np.random.default_rng(4).permutation(len(p))]
    ref = R.VoxelMapRef(LEAF).insert(p)
    assert len(ref.table) == 4 and float(np.abs(np.stack([p["x"], p["y"], p["z"]])).max()) > 100.0
    for order in (sorted(ref.table), sorted(ref.table, reverse=True)):
        at, wrapped = R.probe_slots(order, 8)
        assert wrapped and sorted(at) == [0, 1, 2, 7]
    monkeypatch.setenv("LMONO_VOXEL_FORM", str(form))
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=4)
    monkeypatch.delenv("LMONO_VOXEL_FORM")
    vm.insert(p[:50]); vm.insert(p[50:])                                   # the second call finds, through the same wrapped probes, what the first claimed
    _assert_equal(vm, ref)
    vm.close()


def test_two_slot_table_wraps(gpu_ctx):
    """max_voxels = 1 (2 slots).  One key cannot wrap on its own, so: map A holds a voxel that starts at slot 1, and a second voxel that also starts
    at slot 1 must step to slot 0 before it is refused (the map holds max_voxels already), leaving A unchanged; map B takes that second voxel alone;
    map C a voxel that starts at slot 0."""
    import lmono_amd
    last = _cells_starting_at(1, 2, 2, seed=5)
    first = _cells_starting_at(0, 2, 1, seed=6)
    assert R.probe_slots(R.key_of(last), 2) == ([1, 0], True)
    a, b, c = _points_in(last[:1], 40, 7), _points_in(last[1:], 40, 8), _points_in(first, 40, 9)
    A, B, C = (lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=1) for _ in range(3))
    A.insert(a[:13]); A.insert(a[13:])
    _assert_equal(A, R.VoxelMapRef(LEAF).insert(a))
    with pytest.raises(lmono_amd.LmonoError) as e:
        A.insert(b)
    assert e.value.code == ECAPACITY
    _assert_equal(A, R.VoxelMapRef(LEAF).insert(a))
    B.insert(b); C.insert(c)
    _assert_equal(B, R.VoxelMapRef(LEAF).insert(b))
    _assert_equal(C, R.VoxelMapRef(LEAF).insert(c))
    for m in (A, B, C):
        m.close()


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(41)
    xyz = np.concatenate([rng.uniform(-10.0, 10.0, (30000, 3)), rng.uniform(3.0, 5.0, (170000, 3))]).astype(np.float32)
    p = R.points(xyz, rng.integers(0, 1 << 32, len(xyz), dtype=np.uint64).astype(np.uint32))[rng.permutation(len(xyz))]
    ref = R.VoxelMapRef(LEAF).insert(p)
    return p, ref


@pytest.mark.parametrize("how", ["one_call", "seven_calls", "permuted", "device"])
def test_same_bytes_however_it_arrives(gpu_ctx, big, how):
    import torch
    import lmono_amd
    p, ref = big
    assert len(p) == 200000 and len(ref.table) < len(p) // 4              # on the restatement alone: not a test of singletons
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=1 << 16)
    if how == "one_call":
        vm.insert(p)
    elif how == "seven_calls":
        for part in np.array_split(p, 7):
            vm.insert(part)
    elif how == "permuted":
        vm.insert(p[np.random.default_rng(2).permutation(len(p))])
    else:
        d = torch.from_numpy(p.view(np.uint8).copy()).to("cuda:0")
        torch.cuda.synchronize()
        stats = vm.insert_d(d.data_ptr(), len(p))
        assert stats.tolist() == [len(p), 0, len(ref.table), len(ref.table)]
    _assert_equal(vm, ref)
    vm.close()


def test_plain_form_gives_the_same_bytes(gpu_ctx, big, monkeypatch):
    """LMONO_VOXEL_FORM=0 at create: one probe and one set of adds per point, the baseline the summed insert is measured against."""
    import lmono_amd
    p, ref = big
    monkeypatch.setenv("LMONO_VOXEL_FORM", "0")
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=1 << 16)
    tiny = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=2)
    monkeypatch.delenv("LMONO_VOXEL_FORM")
    parts = np.array_split(np.concatenate([p, R.rejected_points()]), 3)
    stats = [vm.insert(part) for part in parts]
    assert sum(int(s[0]) for s in stats) == len(p) and sum(int(s[1]) for s in stats) == len(R.rejected_points())
    _assert_equal(vm, ref)
    two = R.points([[0.05, 0.05, 0.05], [-0.05, 0.05, 0.05]] * 300, np.arange(600))
    assert tiny.insert(two).tolist() == [600, 0, 2, 2]
    _assert_equal(tiny, R.VoxelMapRef(LEAF).insert(two))
    with pytest.raises(lmono_amd.LmonoError) as e:
        tiny.insert(p[:1000])
    assert e.value.code == ECAPACITY
    _assert_equal(tiny, R.VoxelMapRef(LEAF).insert(two))
    vm.close(); tiny.close()


def test_capacity_is_exact_and_sticky(gpu_ctx):
    import lmono_amd
    eight = R.points([[k + 0.05, 0.05, 0.05] for k in range(8)], np.arange(8) * 1000 + 0xFF000000)
    ninth = R.points([[100.05, 0.05, 0.05]], [0xFF123456])
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=8)
    assert vm.insert(eight).tolist() == [8, 0, 8, 8]                       # exactly max_voxels fit
    ref = R.VoxelMapRef(LEAF).insert(eight)
    _assert_equal(vm, ref)
    before = [a.tobytes() for a in vm.cells()]
    with pytest.raises(lmono_amd.LmonoError) as e:
        vm.insert(np.concatenate([eight[:3], ninth, eight[5:]]))
    assert e.value.code == ECAPACITY
    assert [a.tobytes() for a in vm.cells()] == before and vm.size == 8
    with pytest.raises(lmono_amd.LmonoError) as e:                         # full until cleared, even for voxels it holds
        vm.insert(eight[:2])
    assert e.value.code == ECAPACITY
    _assert_equal(vm, ref)                                                 # read() and cells() keep working
    vm.clear()
    assert vm.size == 0 and len(vm.read()) == 0
    again = np.concatenate([eight[:7], ninth])
    assert vm.insert(again).tolist() == [8, 0, 8, 8]
    _assert_equal(vm, R.VoxelMapRef(LEAF).insert(again))
    vm.close()


def _camera(w, h):
    import lmono_amd
    s = w / 1241.0
    return lmono_amd.Camera(w, h, 718.856 * s, 718.856 * s, 607.1928 * s, h / 2.0, 0, 0, 0, 0, 5, 0, 0)


def test_insert_frames_reads_the_builders_device_clouds(gpu_ctx):
    import torch
    import lmono_amd
    sizes = [(97, 53), (64, 32), (65, 33)]                                 # the ragged images of test_colour_gpu.py
    M = CC.lidar_to_camera()
    q, t = np.array([0.0, 0.0, 0.0, 1.0]), np.array([1.0, 2.0, 3.0])
    clouds = [CC.random_cloud(20000, seed=w * 1000 + h, zmax=80.0) for w, h in sizes]
    clouds[1] = clouds[1][:0]                                              # an empty cloud: an empty frame
    images = [CC.noise_image(h, w, seed=w) for w, h in sizes]
    mbs = [lmono_amd.MapBuilder(gpu_ctx, _camera(w, h), max_cloud_points=16, map_capacity_points=2 * w * h) for w, h in sizes]
    dc = [torch.from_numpy(c).to("cuda:0") for c in clouds]; di = [torch.from_numpy(i).to("cuda:0") for i in images]
    torch.cuda.synchronize()
    n = lmono_amd.MapBuilder.associate_batch(gpu_ctx, mbs, [x.data_ptr() if len(c) else 0 for x, c in zip(dc, clouds)], [len(c) for c in clouds], [M] * 3,
                                             [x.data_ptr() for x in di], [q] * 3, [t] * 3)
    assert n[0] > 0 and n[1] == 0 and n[2] > 0
    leaf = 0.5
    vms = [lmono_amd.VoxelMap(gpu_ctx, leaf=leaf, max_voxels=1 << 14) for _ in sizes]
    stats = lmono_amd.VoxelMap.insert_frames(gpu_ctx, vms, mbs)
    for s in range(3):
        world = mbs[s].cloud(1)
        host = lmono_amd.VoxelMap(gpu_ctx, leaf=leaf, max_voxels=1 << 14)
        hs = host.insert(world)
        assert stats[s].tolist() == hs.tolist() and stats[s][0] + stats[s][1] == n[s]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(vms[s].cells(), host.cells())) and vms[s].read().tobytes() == host.read().tobytes()
        _assert_equal(vms[s], R.VoxelMapRef(leaf).insert(world))
        host.close()
    assert vms[1].size == 0 and vms[0].size > 0
    for maps, builders in (([vms[0], vms[0]], mbs[:2]), (vms[:2], [mbs[0], mbs[0]])):
        with pytest.raises(lmono_amd.LmonoError) as e:
            lmono_amd.VoxelMap.insert_frames(gpu_ctx, maps, builders)
        assert e.value.code == EINVAL
    mbs[0].clear()                                                         # its last world cloud left with rgb_map
    with pytest.raises(lmono_amd.LmonoError) as e:
        vms[0].insert_frame(mbs[0])
    assert e.value.code == EINVAL
    for x in vms + mbs:
        x.close()


def _moving_frame(k, w, h):
    cloud = CC.s1_scan(n_rings=32, n_az=600, k=k)
    bgr = CC.noise_image(h, w, seed=100 + k)
    q = np.round(np.array([0.01 * k, -0.02, np.sin(0.05 * k), np.cos(0.05 * k)]), 6)
    return cloud, bgr, q, np.round(np.array([0.8 * k, 0.1 * k, 0.02 * k]), 6)


def test_ten_frames_keep_what_rgb_map_lost(gpu_ctx):
    import lmono_amd
    w, h = 320, 96
    M = CC.lidar_to_camera()
    mb = lmono_amd.MapBuilder(gpu_ctx, lmono_amd.Camera(w, h, 185.0, 185.0, 156.5, 47.25, 0, 0, 0, 0, 5, 0, 0), max_cloud_points=1 << 16, map_capacity_points=6 * w * h)
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=1 << 18)
    worlds = []
    for k in range(10):
        cloud, bgr, q, t = _moving_frame(k, w, h)
        assert mb.associate(cloud, M, bgr, q, t) > 1000
        worlds.append(mb.cloud(1).copy())
        vm.insert_frame(mb)
        if k == 4:
            mb.clear()
    total = sum(len(x) for x in worlds)
    assert len(mb.map()) == sum(len(x) for x in worlds[5:]) < total        # rgb_map lost the first five frames
    ref = R.VoxelMapRef(LEAF).insert(np.concatenate(worlds))
    _assert_equal(vm, ref)
    assert int(vm.cells()[1].sum()) == total - ref.rejected and ref.rejected == 0
    vm.close(); mb.close()


def test_cpp_map_build_writes_the_voxel_map(gpu_ctx, tmp_path):
    """map_build ... voxel=0.1 writes rgb_map_voxel.ply, equal to the Python path's read() over the same frames; rgb_map10.ply is written as without it."""
    import lmono_amd
    from lmono_amd import kitti_io as IO
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lmono_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "map_build"])
    w, h, n = 320, 96, 11
    fx = fy = 185.0; cx = 156.5; cy = 47.25
    seq = tmp_path / "seq"; out = tmp_path / "out"
    os.makedirs(seq / "velodyne"); os.makedirs(seq / "image_bgr"); os.makedirs(out)
    M = CC.lidar_to_camera()
    mb = lmono_amd.MapBuilder(gpu_ctx, lmono_amd.Camera(w, h, fx, fy, cx, cy, 0, 0, 0, 0, 5, 0, 0), max_cloud_points=1 << 16)
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=0.1, max_voxels=1 << 18)
    qt = np.zeros((n, 7))
    for k in range(n):
        cloud, bgr, q, t = _moving_frame(k, w, h)
        IO.write_velodyne_bin(IO.velodyne_path(str(seq), k), cloud)
        (seq / "image_bgr" / ("%06d.bgr" % k)).write_bytes(bgr.tobytes())
        qt[k, :4] = q; qt[k, 4:] = t
        mb.associate(cloud, M, bgr, q, t)
        vm.insert_frame(mb)
        if (k + 1) % 10 == 0:
            mb.clear()                                                     # processMapping's every-tenth-frame clear
    IO.write_trajectory(str(tmp_path / "traj.txt"), 50.0 + 0.1 * np.arange(n), qt)
    txt = subprocess.check_output([os.path.join(host, "map_build"), str(seq), str(tmp_path / "traj.txt"), str(out), str(n), str(w), str(h),
                                   repr(fx), repr(fy), repr(cx), repr(cy), "voxel=0.1:%d" % (1 << 18)], text=True).strip().split("\n")
    assert len(txt) == n and txt[9].endswith("wrote " + IO.rgb_map_path(str(out), 10))
    ply = IO.read_ply_binary(str(out / "rgb_map_voxel.ply"))
    want = vm.read()
    assert len(want) > 1000 and ply.tobytes() == want.tobytes()
    vm.close(); mb.close()
