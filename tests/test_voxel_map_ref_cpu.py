"""The voxel-grid colour map without a GPU: (a) the numpy restatement's own properties, (b) the host program
lmono_amd/host/voxel_map_test -- the header the kernels include, over a std::map -- equals the restatement byte for byte, (c) the same
program as a stand-alone executable under AddressSanitizer and UBSan runs clean on the same input."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import voxel_map_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lmono_amd", "host")
LEAF = 0.1


def _random_points(n=20000, seed=5, span=300.0):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-span, span, (n, 3)).astype(np.float32)
    xyz[: n // 4] = (xyz[: n // 4] / 100.0).astype(np.float32)          # a dense part, so that voxels hold several points
    return R.points(xyz, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a.cells(), b.cells())) and a.read().tobytes() == b.read().tobytes()


def test_order_and_split_do_not_change_the_cells():
    p = _random_points(6000)
    one = R.VoxelMapRef(LEAF).insert(p)
    perm = R.VoxelMapRef(LEAF).insert(p[np.random.default_rng(1).permutation(len(p))])
    split = R.VoxelMapRef(LEAF)
    for part in np.array_split(p, 7):
        split.insert(part)
    assert len(one.table) < len(p)
    assert _same(one, perm) and _same(one, split)


def test_minus_1e_9_lands_in_cell_minus_one_with_the_last_offset():
    p = R.points([[-1e-9, 0.5, 0.5]], [0xFF000000])
    ok, i, q = R.cell_of(p, LEAF)
    t = p["x"][0] * (np.float32(1.0) / np.float32(LEAF))
    assert t - np.floor(t) == np.float32(1.0)                          # why the min is needed
    assert ok[0] and i[0, 0] == -1 and q[0, 0] == 65535


def test_negative_coordinates_floor_downwards_and_boundaries():
    L = np.float32(LEAF)
    p = R.points([[-0.05, -0.15, -0.25], [0.05, 0.15, 0.25]], [0, 0])
    ok, i, q = R.cell_of(p, LEAF)
    assert ok.all() and i[0].tolist() == [-1, -2, -3] and i[1].tolist() == [0, 1, 2]
    inv = np.float32(1.0) / L
    for k in (-1000, -3, -1, 0, 1, 2, 7, 1000):
        x = np.float32(k) * L
        ok, i, q = R.cell_of(R.points([[x, x, x]], [0]), LEAF)
        t = x * inv
        assert ok[0] and i[0, 0] == int(np.floor(t)) and 0 <= q[0, 0] <= 65535
        assert abs(i[0, 0] - k) <= 1                                   # k * L lands in cell k or, by the rounding of x * inv, in k - 1
        below = np.nextafter(x, np.float32(-1e9), dtype=np.float32)
        ok2, i2, q2 = R.cell_of(R.points([[below, 0, 0]], [0]), LEAF)
        assert ok2[0] and (i2[0, 0], q2[0, 0]) <= (i[0, 0], q[0, 0])   # monotone across the boundary


def test_rejected_points_are_counted_and_never_inserted():
    m = R.VoxelMapRef(LEAF).insert(R.rejected_points())
    assert m.rejected == len(R.rejected_points()) and len(m.table) == 0
    # the last accepted and the first rejected cell index
    inv = np.float32(1.0) / np.float32(LEAF)
    x = np.float32(104857.0)
    assert x * inv < np.float32(1048576.0)
    assert R.cell_of(R.points([[x, 0, 0]], [0]), LEAF)[0][0]
    assert not R.cell_of(R.points([[np.float32(104857.7), 0, 0]], [0]), LEAF)[0][0]
    assert R.cell_of(R.points([[np.float32(-104857.5), 0, 0]], [0]), LEAF)[0][0]
    assert not R.cell_of(R.points([[np.float32(-104857.7), 0, 0]], [0]), LEAF)[0][0]


def test_output_point_is_the_mean_within_the_fixed_point_step():
    """|output - fp64 mean of the voxel's points| <= 2^-16 L (the offset's step: truncation below, the half-step centring) + the float32
    rounding of x * inv carried back to metres + the rounding of the float32 output, all from the inputs' magnitudes."""
    p = _random_points(8000, seed=9)
    m = R.VoxelMapRef(LEAF).insert(p)
    ok, i, q = R.cell_of(p, LEAF)
    keys = R.key_of(i)
    out = m.read()
    order = {int(k): n for n, k in enumerate(sorted(m.table))}
    L = float(np.float32(LEAF)); inv = float(np.float32(1.0) / np.float32(LEAF))
    eps = 2.0 ** -24
    sums = np.zeros((len(out), 3)); cnt = np.zeros(len(out)); mag = np.zeros((len(out), 3))
    xyz = np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float64)
    for k in range(len(p)):
        n = order[int(keys[k])]
        sums[n] += xyz[k]; cnt[n] += 1; mag[n] = np.maximum(mag[n], np.abs(xyz[k]))
    mean = sums / cnt[:, None]
    got = np.stack([out["x"], out["y"], out["z"]], 1).astype(np.float64)
    # t = fl(x * inv): |t - x * inv| <= eps |x inv|; inv itself is fl(1 / L): |inv L - 1| <= eps, so x inv L differs from x by <= eps |x|; f = t - c is exact
    bound = 2.0 ** -16 * L + (mag * inv * eps) * L + mag * eps * (1 + eps) + (mag + L) * eps + 1e-12
    assert (np.abs(got - mean) <= bound).all(), float((np.abs(got - mean) - bound).max())
    assert len(out) < len(p)
    # colours: the truncated integer mean
    b = p["bgra"].astype(np.int64)
    n0 = order[int(keys[0])]
    sel = keys == keys[0]
    assert int(out["bgra"][n0]) & 255 == int((b[sel] & 255).sum()) // int(sel.sum()) and int(out["bgra"][n0]) >> 24 == 255


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("voxel_map")
    out = []
    for name, p in (("random", np.concatenate([_random_points(), R.rejected_points()])), ("edges", np.concatenate([R.edge_points(LEAF), R.rejected_points()]))):
        path = str(d / (name + ".bin"))
        p.tofile(path)
        out.append((path, R.VoxelMapRef(LEAF).insert(p).text()))
    return out


def test_host_program_equals_the_restatement(cases):
    subprocess.check_call(["make", "-s", "-C", HOST, "voxel_map_test"])
    for path, want in cases:
        got = subprocess.check_output([os.path.join(HOST, "voxel_map_test"), path, repr(LEAF)], text=True)
        assert got == want
    assert cases[0][1].count("\n") > 15000 and cases[0][1].startswith("rejected 7\n")


def test_host_program_runs_clean_under_sanitizers(cases, tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "voxel_map_test_san")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HOST, "voxel_map_test.cpp"), "-o", exe])
    for path, want in cases:
        r = subprocess.run([exe, path, repr(LEAF)], text=True, capture_output=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
        assert r.stdout == want
