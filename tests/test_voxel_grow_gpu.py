"""A live voxel map changes size on the GPU (lmono_voxel_map_reserve / set_growth / capacity): its content is the same bytes
whatever its growth history was.  Every expected value comes from the numpy restatement of the map (tests/voxel_map_ref.py), of compose
(tests/voxel_compose_ref.py) or of the growth rule (tests/voxel_grow_ref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import colour_cases as CC
from tests import voxel_compose_ref as CR
from tests import voxel_grow_ref as G
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


def _bytes(vm):
    return [a.tobytes() for a in vm.cells()] + [vm.read().tobytes()]


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


def _refused(call, code=ECAPACITY):
    import lmono_amd
    with pytest.raises(lmono_amd.LmonoError) as e:
        call()
    assert e.value.code == code


EIGHT = R.points([[k + 0.05, 0.05, 0.05] for k in range(8)], np.arange(8) * 1000 + 0xFF000000)
NINTH = R.points([[100.05, 0.05, 0.05]], [0xFF123456])
TENTH = R.points([[200.05, 0.05, 0.05]], [0xFF654321])


@pytest.mark.parametrize("form", [1, 0])
def test_reserve_up_through_a_wrapped_probe(gpu_ctx, monkeypatch, form):
    """The four cells of the tiny-table test (three keys that start at slot 7 of 8, one at slot 0) are moved out of their wrapped probes into 16
    slots, then into 2^11, and the map goes on taking points."""
    import lmono_amd
    cells = np.concatenate([_cells_starting_at(7, 8, 3, seed=1), _cells_starting_at(0, 8, 1, seed=2)])
    p = _points_in(cells, 40, seed=3)
    p = p[np.random.default_rng(4).permutation(len(p))]
    ref = R.VoxelMapRef(LEAF).insert(p)
    at, wrapped = R.probe_slots(sorted(ref.table), 8)
    assert len(ref.table) == 4 and wrapped and sorted(at) == [0, 1, 2, 7]
    monkeypatch.setenv("LMONO_VOXEL_FORM", str(form))
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=4)
    monkeypatch.delenv("LMONO_VOXEL_FORM")
    vm.insert(p[:50]); vm.insert(p[50:])
    assert tuple(vm.capacity) == (4, 8, 0, 0)
    vm.reserve(5)
    assert tuple(vm.capacity) == (5, 16, 0, 1) and vm.max_voxels == 5
    _assert_equal(vm, ref)
    vm.reserve(1 << 10)
    assert tuple(vm.capacity) == (1 << 10, 1 << 11, 0, 2)
    _assert_equal(vm, ref)
    more = _cloud(50, 5)
    st = vm.insert(more)
    ref.insert(more)
    assert st.tolist() == [50, 0, len(ref.table) - 4, len(ref.table)]
    _assert_equal(vm, ref)
    vm.close()


def test_reserve_down_where_the_rehash_must_wrap(gpu_ctx):
    import lmono_amd
    cells = _cells_starting_at(7, 8, 3, seed=11)
    keys = R.key_of(cells)
    for order in (sorted(keys), sorted(keys, reverse=True)):               # whatever order the movers arrive in: slots 7, 0, 1
        at, wrapped = R.probe_slots(order, 8)
        assert wrapped and sorted(at) == [0, 1, 7]
    p = _points_in(cells, 40, seed=12)
    ref = R.VoxelMapRef(LEAF).insert(p)
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=1 << 10)
    vm.insert(p)
    vm.reserve(4)
    assert vm.capacity.slots == 8 and vm.capacity.max_voxels == 4
    _assert_equal(vm, ref)
    vm.close()
    # two slots: one voxel, whichever slot it starts at
    for start in (0, 1):
        one = _points_in(_cells_starting_at(start, 2, 1, seed=13 + start), 40, seed=15)
        vm = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=1 << 10)
        vm.insert(one)
        vm.reserve(1)
        assert tuple(vm.capacity)[:2] == (1, 2)
        _assert_equal(vm, R.VoxelMapRef(LEAF).insert(one))
        _refused(lambda: vm.insert(NINTH))                                 # exactly one voxel fits
        vm.close()


def test_shrink_to_fit_is_exact(gpu_ctx):
    import lmono_amd
    p = _cloud(20000, 31, span=1.0)
    ref = R.VoxelMapRef(LEAF).insert(p)
    n = len(ref.table)
    assert 1000 < n < len(p) // 2
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=1 << 14)
    vm.insert(p)
    vm.shrink_to_fit()
    assert tuple(vm.capacity) == (n, G.slots(n), 0, 1) and vm.size == n
    _assert_equal(vm, ref)
    st = vm.insert(p[:300])                                                # voxels it holds: fits
    ref.insert(p[:300])
    assert st.tolist() == [300, 0, 0, n]
    _assert_equal(vm, ref)
    _refused(lambda: vm.insert(R.points([[50.05, 0.05, 0.05]], [0xFF000001])))      # one new voxel: growth is off
    _assert_equal(vm, ref)
    vm.close()


def test_rebuild_repairs_a_refused_map_and_drops_the_ghosts(gpu_ctx):
    import lmono_amd
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=8)
    assert vm.insert(EIGHT).tolist() == [8, 0, 8, 8]
    ref = R.VoxelMapRef(LEAF).insert(EIGHT)
    _refused(lambda: vm.insert(np.concatenate([EIGHT[:3], NINTH, EIGHT[5:]])))
    _refused(lambda: vm.insert(EIGHT[:2]))                                 # full
    vm.reserve(8)
    assert tuple(vm.capacity) == (8, 16, 0, 1)
    assert vm.insert(EIGHT[:2]).tolist() == [2, 0, 0, 8]
    _assert_equal(vm, ref.insert(EIGHT[:2]))
    vm.reserve(9)
    assert vm.insert(NINTH).tolist() == [1, 0, 1, 9]                       # not [.., 10]: the refused call's claim is gone, the counter starts at 8
    _assert_equal(vm, ref.insert(NINTH))
    _refused(lambda: vm.insert(TENTH))
    _assert_equal(vm, ref)
    vm.close()


@pytest.fixture(scope="module")
def scattered():
    return _cloud(5000, 51, span=1.0)


@pytest.mark.parametrize("how", ["one_call", "seven_calls", "permuted", "device", "plain", "tile-1", "tile", "tile+1"])
def test_automatic_growth_however_the_points_arrive(gpu_ctx, scattered, monkeypatch, how):
    import torch
    import lmono_amd
    p = scattered
    limit = 1 << 12
    if how == "plain":
        monkeypatch.setenv("LMONO_VOXEL_FORM", "0")
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=2, grow_limit=limit)
    fixed = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=limit)
    monkeypatch.delenv("LMONO_VOXEL_FORM", raising=False)
    assert tuple(vm.capacity) == (2, 4, limit, 0)
    if how == "seven_calls":
        parts = np.array_split(p, 7)
    elif how == "permuted":
        parts = np.array_split(p[np.random.default_rng(2).permutation(len(p))], 2)
    elif how.startswith("tile"):
        first = vm.TILE + {"tile-1": -1, "tile": 0, "tile+1": 1}[how]
        parts = [p[:first], p[first:]]
    else:
        parts = [p]
    ref = R.VoxelMapRef(LEAF)
    cap = 2
    for part in parts:
        if how == "device":
            d = torch.from_numpy(part.view(np.uint8).copy()).to("cuda:0")
            torch.cuda.synchronize()
            st, fst = vm.insert_d(d.data_ptr(), len(part)), fixed.insert_d(d.data_ptr(), len(part))
        else:
            st, fst = vm.insert(part), fixed.insert(part)
        before = len(ref.table)
        ref.insert(part)
        assert st.tolist() == fst.tolist() == [len(part), 0, len(ref.table) - before, len(ref.table)]
        cap = G.capacity(cap, limit, len(ref.table))
        assert vm.capacity.max_voxels == cap and vm.capacity.slots == G.slots(cap)
    assert 600 <= len(ref.table) < len(p) and cap == 4096                  # on the restatement: several doublings, voxels shared by points
    assert vm.capacity.rehashes > 0 and fixed.capacity.rehashes == 0
    if how == "one_call":
        assert vm.capacity.rehashes == 11                                  # 2 -> 4096, a step at a time
    _assert_equal(vm, ref)
    _assert_equal(fixed, ref)
    vm.close(); fixed.close()


def test_the_limit_holds(gpu_ctx):
    import lmono_amd
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=2, grow_limit=8)
    assert vm.insert(EIGHT).tolist() == [8, 0, 8, 8]
    assert tuple(vm.capacity) == (8, 16, 8, 2)
    ref = R.VoxelMapRef(LEAF).insert(EIGHT)
    _assert_equal(vm, ref)
    _refused(lambda: vm.insert(np.concatenate([EIGHT[:3], NINTH])))
    _assert_equal(vm, ref)
    assert tuple(vm.capacity) == (8, 16, 8, 2)
    _refused(lambda: vm.insert(EIGHT[:2]))                                 # sticky
    _refused(lambda: vm.insert(EIGHT[:0]))
    vm.reserve(16)                                                         # above the limit: allowed, and growth then never triggers
    assert tuple(vm.capacity) == (16, 32, 8, 3)
    assert vm.insert(NINTH).tolist() == [1, 0, 1, 9]
    _assert_equal(vm, ref.insert(NINTH))
    vm.close()


def _camera(w, h):
    import lmono_amd
    s = w / 1241.0
    return lmono_amd.Camera(w, h, 718.856 * s, 718.856 * s, 607.1928 * s, h / 2.0, 0, 0, 0, 0, 5, 0, 0)


def _batched(ctx, fn, maps, others):
    """The batched C entry itself: its return value AND its stats rows (the wrapper raises on LMONO_ECAPACITY and drops the rows)."""
    n = len(maps)
    mh = (C.c_void_p * n)(*[m.h for m in maps]); oh = (C.c_void_p * n)(*[o.h for o in others])
    stats = np.full((n, 4), -7, np.int64)
    return getattr(ctx.L, fn)(ctx.h, n, mh, oh, stats.ctypes.data), stats


def test_batched_call_repeats_only_the_refused_streams(gpu_ctx):
    import torch
    import lmono_amd
    sizes = [(97, 53), (64, 32), (65, 33)]                                 # the ragged images of test_colour_gpu.py
    M = CC.lidar_to_camera()
    q, t = np.array([0.0, 0.0, 0.0, 1.0]), np.array([1.0, 2.0, 3.0])
    clouds = [CC.random_cloud(20000, seed=w * 1000 + h, zmax=80.0) for w, h in sizes]
    images = [CC.noise_image(h, w, seed=w) for w, h in sizes]
    mbs = [lmono_amd.MapBuilder(gpu_ctx, _camera(w, h), max_cloud_points=16, map_capacity_points=2 * w * h) for w, h in sizes]
    dc = [torch.from_numpy(c).to("cuda:0") for c in clouds]; di = [torch.from_numpy(i).to("cuda:0") for i in images]
    torch.cuda.synchronize()
    n = lmono_amd.MapBuilder.associate_batch(gpu_ctx, mbs, [x.data_ptr() for x in dc], [len(c) for c in clouds], [M] * 3,
                                             [x.data_ptr() for x in di], [q] * 3, [t] * 3)
    assert min(n) > 0
    leaf = 0.5
    fs = [lmono_amd.OutlierFilter(gpu_ctx, w * h, 4, 1.0, 2.0, 8) for w, h in sizes]
    lmono_amd.OutlierFilter.filter_frames(fs, mbs)
    for fn, others, cloud_of in (("lmono_voxel_map_insert_frames", mbs, lambda s: mbs[s].cloud(1)), ("lmono_voxel_map_insert_filtered", fs, lambda s: fs[s].cloud())):
        vms = [lmono_amd.VoxelMap(gpu_ctx, leaf=leaf, max_voxels=1 << 14), lmono_amd.VoxelMap(gpu_ctx, leaf=leaf, max_voxels=1, grow_limit=1 << 14),
               lmono_amd.VoxelMap(gpu_ctx, leaf=leaf, max_voxels=1)]
        refs = [R.VoxelMapRef(leaf).insert(cloud_of(s)) for s in range(3)]
        assert min(len(r.table) for r in refs) > 1                         # frame 3 cannot fit into one voxel; map 1 has to grow
        rc, stats = _batched(gpu_ctx, fn, vms, others)
        assert rc == ECAPACITY
        for s in range(2):
            host = lmono_amd.VoxelMap(gpu_ctx, leaf=leaf, max_voxels=1 << 14)
            assert stats[s].tolist() == host.insert(cloud_of(s)).tolist()
            assert _bytes(vms[s]) == _bytes(host)                          # map 0 in particular: inserted once, not once per round
            _assert_equal(vms[s], refs[s])
            host.close()
        assert vms[1].capacity.max_voxels == G.capacity(1, 1 << 14, len(refs[1].table)) and vms[1].capacity.rehashes > 0
        assert vms[0].capacity.rehashes == 0 and tuple(vms[2].capacity) == (1, 2, 0, 0)
        assert vms[2].size == 0 and stats[2].tolist() == [0, stats[2][1], 0, 0]
        _refused(lambda: vms[2].insert(EIGHT[:0]))                         # full
        for x in vms:
            x.close()
    for x in fs + mbs:
        x.close()


def test_compose_into_a_growing_destination(gpu_ctx):
    import lmono_amd
    srcs = [(_cloud(3000, 61, span=1.0), CR.rigid(0.7, -0.2, 0.1, (3.0, -40.5, 0.25))), (_cloud(2500, 62, span=1.0), CR.rigid(-0.3, 0.1, 0.0, (0.5, 0.25, 0.0))),
            (_cloud(2000, 63, span=1.0), CR.IDENTITY)]
    subs = [lmono_amd.VoxelMap(gpu_ctx, leaf=0.05, max_voxels=1 << 13) for _ in srcs]
    sub_refs = []
    for vm, (p, _) in zip(subs, srcs):
        vm.insert(p)
        sub_refs.append(R.VoxelMapRef(0.05).insert(p))
    T = np.array([t for _, t in srcs]).reshape(-1, 3, 4)
    ref = R.VoxelMapRef(LEAF)
    want = CR.compose(ref, sub_refs, T)
    assert want[5] > 1000
    limit = 1 << 14
    grown = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=1, grow_limit=limit)
    fixed = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=limit)
    assert grown.compose(subs, T, stats=True).tolist() == fixed.compose(subs, T, stats=True).tolist() == want
    assert _bytes(grown) == _bytes(fixed)
    _assert_equal(grown, ref)
    assert grown.capacity.max_voxels == G.capacity(1, limit, want[5]) and grown.capacity.rehashes > 0
    held = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=1, grow_limit=64)
    _refused(lambda: held.compose(subs, T))                                # at its limit: all or nothing
    assert held.size == 0 and tuple(held.capacity)[:3] == (64, 128, 64)
    _refused(lambda: held.insert(EIGHT[:1]))
    for x in subs + [grown, fixed, held]:
        x.close()


def test_atlas_of_growing_compacted_submaps(gpu_ctx):
    import lmono_amd
    frames = [_cloud(1500, 70 + k, span=1.0) for k in range(6)]
    for k, f in enumerate(frames):
        f["x"] += np.float32(0.4 * k)
    poses = [CR.pose_tq((0.4 * k, 0.0, 0.0), 0.02 * k) for k in range(6)]
    fixed_poses = [CR.pose_tq((0.4 * k + 0.05 * (k // 2), 0.03 * k, 0.0), 0.02 * k + 0.01 * (k // 2)) for k in range(6)]
    compact = lmono_amd.SubmapAtlas(gpu_ctx, frames_per_submap=2, max_voxels_sub=64, grow_limit_sub=1 << 16, compact_closed=True)
    today = lmono_amd.SubmapAtlas(gpu_ctx, frames_per_submap=2)
    assert today.grow_limit_sub == 0 and today.compact_closed is False and today.max_voxels_sub == 1 << 20
    for f, pose in zip(frames, poses):
        a, b = compact.insert_frame(f, pose), today.insert_frame(f, pose)
        assert a.tolist() == b.tolist()
    assert [m.capacity.max_voxels == m.size for m in compact.submaps] == [True, True, False]      # closed ones are shrunk already, the open one not yet
    dsts = [lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=1 << 16) for _ in range(2)]
    sa = compact.compose(dsts[0], fixed_poses, stats=True)
    sb = today.compose(dsts[1], fixed_poses, stats=True)
    assert sa.tolist() == sb.tolist() and sa[5] > 1000 and _bytes(dsts[0]) == _bytes(dsts[1])
    for m, u in zip(compact.submaps, today.submaps):
        assert m.capacity.max_voxels == m.size > 64 and m.capacity.slots == G.slots(m.size) and m.capacity.grow_limit == 1 << 16
        assert tuple(u.capacity) == (1 << 20, 1 << 21, 0, 0) and _bytes(m) == _bytes(u)
    compact.close(); today.close()
    for d in dsts:
        d.close()


def test_refusals_before_any_launch(gpu_ctx):
    import lmono_amd
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=16)
    other = lmono_amd.VoxelMap(gpu_ctx, leaf=LEAF, max_voxels=16)
    vm.insert(EIGHT)
    before, cap = _bytes(vm), tuple(vm.capacity)
    for call in (lambda: vm.reserve(7), lambda: vm.reserve(0), lambda: vm.reserve((1 << 30) + 1), lambda: lmono_amd.VoxelMap.reserve_batch([vm, vm], [16, 32]),
                 lambda: lmono_amd.VoxelMap.reserve_batch([other, vm, other], [16, 32, 64]), lambda: lmono_amd.VoxelMap.reserve_batch([other, vm], [32, 7]),
                 lambda: vm.set_growth(15), lambda: vm.set_growth((1 << 30) + 1), lambda: vm.set_growth(-1)):
        _refused(call, EINVAL)
        assert tuple(vm.capacity) == cap == (16, 32, 0, 0) and tuple(other.capacity) == (16, 32, 0, 0)
    assert gpu_ctx.L.lmono_voxel_map_reserve(gpu_ctx.h, 0, None, None) == EINVAL
    assert _bytes(vm) == before
    vm.set_growth(16); vm.set_growth(1 << 30); vm.set_growth(0)
    assert tuple(vm.capacity) == cap
    other.reserve(1)                                                       # an empty map: nothing to move
    assert tuple(other.capacity) == (1, 2, 0, 1) and other.size == 0
    assert other.insert(NINTH).tolist() == [1, 0, 1, 1]
    lmono_amd.VoxelMap.reserve_batch([other, vm], [3, 8])                  # one up, one down, in one call
    assert tuple(other.capacity) == (3, 8, 0, 2) and tuple(vm.capacity) == (8, 16, 0, 1)
    assert _bytes(vm) == before
    _assert_equal(other, R.VoxelMapRef(LEAF).insert(NINTH))
    vm.close(); other.close()


def _moving_frame(k, w, h):
    cloud = CC.s1_scan(n_rings=32, n_az=600, k=k)
    bgr = CC.noise_image(h, w, seed=100 + k)
    q = np.round(np.array([0.01 * k, -0.02, np.sin(0.05 * k), np.cos(0.05 * k)]), 6)
    return cloud, bgr, q, np.round(np.array([0.8 * k, 0.1 * k, 0.02 * k]), 6)


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    """The 11 frames at 320 x 96 of test_cpp_map_build_writes_the_voxel_map as files, with a corrected trajectory beside them."""
    from lmono_amd import kitti_io as IO
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lmono_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "map_build"])
    w, h, n = 320, 96, 11
    tmp = tmp_path_factory.mktemp("grow_seq")
    seq = tmp / "seq"
    os.makedirs(seq / "velodyne"); os.makedirs(seq / "image_bgr")
    qt = np.zeros((n, 7)); fixed = np.zeros((n, 7))
    for k in range(n):
        cloud, bgr, q, t = _moving_frame(k, w, h)
        IO.write_velodyne_bin(IO.velodyne_path(str(seq), k), cloud)
        (seq / "image_bgr" / ("%06d.bgr" % k)).write_bytes(bgr.tobytes())
        qt[k, :4] = q; qt[k, 4:] = t
        yaw = 0.004 * k
        fixed[k, :4] = np.round(np.array([0.01 * k, -0.02, np.sin(0.05 * k + yaw), np.cos(0.05 * k + yaw)]), 6)
        fixed[k, 4:] = np.round(t + np.array([0.0, 0.03 * k, -0.01 * k]), 6)
    IO.write_trajectory(str(tmp / "traj.txt"), 50.0 + 0.1 * np.arange(n), qt)
    IO.write_trajectory(str(tmp / "corrected.txt"), 50.0 + 0.1 * np.arange(n), fixed)
    cmd = [os.path.join(host, "map_build"), str(seq), str(tmp / "traj.txt")]
    cam = [str(n), str(w), str(h), repr(185.0), repr(185.0), repr(156.5), repr(47.25)]
    return tmp, cmd, cam


@pytest.mark.parametrize("submaps", [False, True])
def test_cpp_map_build_with_a_growth_limit_writes_the_same_maps(gpu_ctx, sequence, submaps):
    from lmono_amd import kitti_io as IO
    tmp, cmd, cam = sequence
    front = ["submap=2:%s:0.05" % (tmp / "corrected.txt")] if submaps else []
    outs = []
    for tag, voxel in (("fixed", "voxel=0.1"), ("grow", "voxel=0.1:64:1048576")):
        out = tmp / ("out_%s_%d" % (tag, submaps))
        os.makedirs(out)
        txt = subprocess.check_output(cmd + [str(out)] + cam + front + [voxel], text=True).strip().split("\n")
        assert len(txt) == 11
        outs.append(out)
    names = ["rgb_map_voxel.ply"] + (["rgb_map_global.ply"] if submaps else [])
    for name in names:
        assert (outs[0] / name).read_bytes() == (outs[1] / name).read_bytes() and len(IO.read_ply_binary(str(outs[0] / name))) > 1000
    assert not submaps or (outs[0] / "rgb_map_global.ply").read_bytes() != (outs[0] / "rgb_map_voxel.ply").read_bytes()
