"""Composing voxel maps under rigid transforms without a GPU: (a) the host program lmono_amd/host/voxel_compose_test --
the header the kernels include, over std::map -- equals the numpy restatement (tests/voxel_compose_ref.py) byte for byte, (b) the
restatement's own conservation and order properties, (c) the same program as a stand-alone executable under AddressSanitizer and UBSan,
(d) the end-to-end bound on a small synthetic corridor: the composed map lies on the world, the uncomposed one does not."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import voxel_compose_ref as CR
from tests import voxel_map_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lmono_amd", "host")
LEAF = 0.1


def _random_cloud(n, seed, span=20.0):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-span, span, (n, 3)).astype(np.float32)
    xyz[: n // 2] = (xyz[: n // 2] / 40.0).astype(np.float32)              # a dense half: voxels of several points
    return R.points(xyz, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))


def _heavy_voxel(count=70000):
    """One voxel of `count` identical points: count * q passes 32 bits."""
    return R.points(np.tile(np.array([[0.31, -0.42, 0.53]], np.float32), (count, 1)), np.full(count, 0xFF80FF01, np.uint32))


# name -> (destination leaf, [(points, source leaf, transform)])
def _cases():
    heavy_T = CR.rigid(t=(0.0999985 - 0.31, 0.1, 0.2))                    # moved x lands just below a cell boundary: q near 65535
    return {
        "edges": (LEAF, [(R.edge_points(LEAF), 0.1, CR.IDENTITY), (R.edge_points(LEAF), 0.05, CR.rigid(t=(0.013, -0.2, 7.0)))]),
        "rotated": (LEAF, [(_random_cloud(6000, 1), 0.05, CR.rigid(0.7, -0.2, 0.1, (3.0, -40.5, 0.25))), (_random_cloud(3000, 2), 0.2, CR.rigid(-2.9, 0.0, 0.0, (-1.0, 0.0, 0.0)))]),
        "heavy": (LEAF, [(_heavy_voxel(), 0.05, heavy_T), (_random_cloud(500, 3, span=1.0), 0.05, CR.IDENTITY)]),
    }


def _reference(case):
    leaf_dst, srcs = case
    dst = R.VoxelMapRef(leaf_dst)
    st = CR.compose(dst, [R.VoxelMapRef(leaf).insert(p) for p, leaf, _ in srcs], [T for _, _, T in srcs])
    return dst, st


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("voxel_compose")
    out = {}
    for name, case in _cases().items():
        leaf_dst, srcs = case
        tpath = str(d / (name + "_T.bin"))
        np.array([T for _, _, T in srcs], np.float64).tofile(tpath)
        args = [repr(leaf_dst), tpath]
        for k, (p, leaf, _) in enumerate(srcs):
            ppath = str(d / ("%s_%d.bin" % (name, k)))
            p.tofile(ppath)
            args += [ppath, repr(leaf)]
        dst, st = _reference(case)
        out[name] = (args, CR.text(dst, st), dst, st)
    return out


def test_heavy_voxel_needs_64_bit_products(cases):
    _, _, dst, st = cases["heavy"]
    heavy = [r for r in dst.table.values() if r[0] >= 70000]
    assert len(heavy) == 1 and heavy[0][1] > 1 << 32 and heavy[0][1] // heavy[0][0] >= 65000, heavy
    assert st[1] == 0


def test_host_program_equals_the_restatement(cases):
    subprocess.check_call(["make", "-s", "-C", HOST, "voxel_compose_test"])
    for name, (args, want, dst, st) in cases.items():
        got = subprocess.check_output([os.path.join(HOST, "voxel_compose_test")] + args, text=True)
        assert got == want, name
        assert want.count("\n") == len(dst.table) + 1 and len(dst.table) > 5


def test_host_program_runs_clean_under_sanitizers(cases, tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "voxel_compose_test_san")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HOST, "voxel_compose_test.cpp"), "-o", exe])
    for name, (args, want, _, _) in cases.items():
        r = subprocess.run([exe] + args, text=True, capture_output=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
        assert r.stdout == want, name


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a.cells(), b.cells())) and a.read().tobytes() == b.read().tobytes()


def _totals(ref):
    return [sum(r[w] for r in ref.table.values()) for w in (0, 4, 5, 6)]


def test_restatement_conserves_counts_and_colour_sums_and_ignores_order():
    A, B, Cm = (R.VoxelMapRef(leaf).insert(_random_cloud(n, seed, span=4.0)) for n, seed, leaf in ((900, 4, 0.05), (700, 5, 0.05), (800, 6, 0.2)))
    T = [CR.rigid(0.3, 0.0, 0.0, (0.5, 0.0, 0.0)), CR.IDENTITY, CR.rigid(-0.2, 0.1, 0.0, (0.0, 0.25, 0.0))]
    one = R.VoxelMapRef(LEAF)
    st = CR.compose(one, [A, B, Cm], T)
    assert st[1] == 0 and st[0] == len(A.table) + len(B.table) + len(Cm.table) and st[5] == len(one.table) < st[0]
    want = [sum(x) for x in zip(_totals(A), _totals(B), _totals(Cm))]
    assert _totals(one) == want and st[2] == want[0]
    for order in ((2, 0, 1), (1, 2, 0)):
        m = R.VoxelMapRef(LEAF)
        for k in order:
            CR.compose(m, [(A, B, Cm)[k]], [T[k]])
        assert _same(one, m)
    # a composed map is an ordinary map: inserting before or after the compose gives the same bytes
    p = _random_cloud(400, 7, span=4.0)
    first = R.VoxelMapRef(LEAF).insert(p)
    CR.compose(first, [A, B, Cm], T)
    assert _same(first, one.insert(p))
    # a rejected voxel is counted with its points and adds nothing
    far = R.VoxelMapRef(LEAF)
    st = CR.compose(far, [A], [CR.rigid(t=(2.0e5, 0.0, 0.0))])
    assert st[:4] == [0, len(A.table), 0, _totals(A)[0]] and len(far.table) == 0


def test_pose_delta_carries_the_inserted_pose_to_the_corrected_one():
    a = np.array([1.0, -2.0, 0.5, 0.1, -0.2, 0.3, 0.9]); b = np.array([4.0, 0.25, -1.0, -0.3, 0.1, 0.2, 0.8])
    D = CR.pose_delta(a, b).reshape(3, 4)
    Ra, ta = CR._pose_matrix(a)
    Rb, tb = CR._pose_matrix(b)
    assert np.abs(D[:, :3] @ Ra - Rb).max() < 1e-15 * 8 and np.abs(D[:, :3] @ ta + D[:, 3] - tb).max() < 1e-15 * 32
    assert np.abs(CR.pose_delta(a, a) - CR.IDENTITY).max() < 1e-15 * 32
    import lmono_amd
    assert lmono_amd.pose_delta(a, b).tobytes() == CR.pose_delta(a, b).tobytes()


def test_composed_corridor_lies_on_the_world_and_the_drifted_map_does_not():
    """Composed: every point within sqrt(3) (leaf_sub + leaf) + 1e-3 m of a world point.  Uncomposed: not."""
    c = CR.corridor_reference()
    bound = CR.corridor_bound()
    n_pts = sum(len(f) for f in c["frames"])
    assert c["stats"][1] == 0 and c["stats"][2] == n_pts == _totals(c["dst"])[0]
    assert _totals(c["dst"])[1:] == [sum(x) for x in zip(*[_totals(s)[1:] for s in c["subs"]])]
    err = CR.distance_to_world(c["dst"].read(), c["world"])
    drift = CR.distance_to_world(c["plain"].read(), c["world"])
    print("composed max %.4f m, bound %.4f m; uncomposed max %.3f m, %.1f %% beyond the bound" % (err.max(), bound, drift.max(), 100.0 * (drift > bound).mean()))
    assert err.max() <= bound
    assert drift.max() > bound and (drift > bound).mean() > 0.2
