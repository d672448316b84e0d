"""The point-to-point ICP without a GPU: (a) the host program lmono_amd/host/icp_test -- the header the kernels include, by
brute force -- equals the numpy restatement byte for byte on every case of tests/icp_cases.py, and the Jacobi sweeps leave no off-diagonal,
(b) the restatement recovers a known motion within the fixed point's resolution, at the origin and 6000 m from it, (c) with a third of the
source dropped and 20 outliers added, (d) the constructions of the bound and tie cases are what they claim, (e) the result does not depend on
the order of the input."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import icp_cases as IC
from tests import icp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lmono_amd", "host")


@functools.lru_cache(maxsize=None)
def _case(name):
    tgt, src, kw = IC.CASES[name]()
    return tgt, src, kw, R.run(tgt, src, **kw)


def _host_lines(tmp_path, tgt, src, kw):
    subprocess.check_call(["make", "-s", "-C", HOST, "icp_test"])
    tp, sp = str(tmp_path / "target.bin"), str(tmp_path / "source.bin")
    tgt.tofile(tp); src.tofile(sp)
    D = np.float32(kw.get("max_corr", 0.5))
    cell = np.float32(kw["cell"]) if kw.get("cell") is not None else R.default_cell(D)
    args = [os.path.join(HOST, "icp_test"), tp, sp, repr(float(D)), str(kw.get("max_iter", 50)), repr(float(kw.get("eps", 1e-8))), repr(float(kw.get("mse_eps", 0.0))),
            repr(float(cell)), str(kw.get("max_rings", 2))]
    if kw.get("guess") is not None:
        args += [repr(float(g)) for g in np.asarray(kw["guess"], np.float64).reshape(12)]
    out = subprocess.check_output(args, text=True).split("\n")
    # a NaN's sign and payload are not part of the definition
    nan = lambda m: "7fc00000" if (int(m.group(0), 16) & 0x7FFFFFFF) > 0x7F800000 else m.group(0)
    return [ln if ln.startswith(("transform", "stats", "history", "offdiag")) or " " not in ln or len(ln) != 35 else re.sub(r"[0-9a-f]{8}", nan, ln) for ln in out if ln]


@pytest.mark.parametrize("name", sorted(IC.CASES))
def test_host_program_equals_the_restatement(tmp_path, name):
    tgt, src, kw, ref = _case(name)
    got = _host_lines(tmp_path, tgt, src, kw)
    off = [ln for ln in got if ln.startswith("offdiag")]
    assert off == ["offdiag 0"] and ref.offdiag == 0.0             # kIcpSweeps sweeps diagonalise every 4 x 4 problem of the case exactly
    assert [ln for ln in got if not ln.startswith("offdiag")] == R.text(ref)


def _recovery_error(name, truth):
    """Per point: distance of the aligned point from its true target, and the bound 2^-13 m (8 quanta of the fixed point) + one float32 ulp of the
    largest coordinate of that target."""
    ref = _case(name)[3]
    got = np.stack([ref.cloud[a] for a in ("x", "y", "z")], 1).astype(np.float64)
    err = np.sqrt(((got - truth.astype(np.float64)) ** 2).sum(1))
    bound = 2.0 ** -13 + np.spacing(np.abs(truth).max(1).astype(np.float32)).astype(np.float64)
    return ref, err, bound


@pytest.mark.parametrize("name,at", [("phys_origin", (0.0, 0.0, 0.0)), ("phys_far", (6000.0, -6000.0, 300.0))])
def test_a_known_motion_is_recovered(name, at):
    """Both cases end in 2 iterations: the first finds every true pair, the second finds them again and the state does not move."""
    truth = IC.physical(at)[2]
    ref, err, bound = _recovery_error(name, truth)
    print(name, "iterations", ref.iterations, "status", ref.status, "N", ref.N, "max error", err.max(), "bound", bound.min())
    assert ref.iterations == 2 and ref.status == 0 and ref.N == 218 and ref.stats[1] == 0 and ref.stats[3] == 0
    assert (err <= bound).all()


@pytest.mark.parametrize("name,args,iterations", [("phys3_origin", ((0.0, 0.0, 0.0), 3.0, (0.11, -0.06, 0.08), True), 3),
                                                  ("phys2_far", ((6000.0, -6000.0, 300.0), 2.0, (-0.07, 0.11, 0.05), True), 4)])
def test_a_known_motion_with_missing_points_and_outliers(name, args, iterations):
    """3 and 4 iterations.  The issue's prototype ended both in 4; which third of the source is dropped, where the 20 outliers lie and the sign of
    the shifts are this project's choice (tests/icp_cases.py), and at the origin they leave one round of wrong pairs fewer: the history is
    N = 146 in every iteration with E = 49876189, 5143219, 0, so the solve of the second iteration already lands on the exact motion and the
    third repeats it with no change of state.  At 6000 m E ends at 8 (float32 coordinates), after 4 iterations as in the issue."""
    truth = IC.physical(*args)[2]
    ref, err, bound = _recovery_error(name, truth)
    print(name, "iterations", ref.iterations, "status", ref.status, "N", ref.N, "max error", err[:146].max(), "bound", bound.min())
    assert ref.iterations == iterations and ref.status == 0 and ref.stats[0] == 166 and ref.N == 146
    assert (ref.history[:, 0] <= 146).all() and np.isinf(ref.d2[146:]).all() and np.isfinite(ref.d2[:146]).all()      # the outliers are never matched
    assert (err[:146] <= bound[:146]).all()


def test_the_constructions_are_what_they_claim():
    # the bound: pair 0 at d2 == D2 exactly and accepted, pair 1 at the next float32 above and rejected
    ref = _case("d_bound")[3]
    D2 = np.float32(0.5) * np.float32(0.5)
    assert ref.d2[0] == D2 and np.isinf(ref.d2[1]) and ref.history[0, 0] == 4
    tgt, src, _ = IC.d_bound()
    dy = np.float32(tgt["y"][1]) - np.float32(src["y"][1])
    assert (np.float32(0.25) + dy * dy) == np.nextafter(D2, np.float32(1.0))
    # the ties: both mirrored targets are equally far in the first iteration; the smaller coordinate wins
    tgt, src, kw = IC.ties()
    one = R.run(tgt, src, **dict(kw, max_iter=1))
    assert one.d2[:3].tolist() == [0.0625] * 3 and one.N == 5
    win = [(1.75, 2, 2), (6, 1.75, 2), (2, 6, 1.75), (6, 6.125, 3), (4.125, 4, 4)]
    only = R.run(IC.pts(np.array(win, np.float32)), src, **dict(kw, max_iter=1))
    assert only.origin.tobytes() == one.origin.tobytes() and only.transform.tobytes() == one.transform.tobytes()
    # the smallest shapes end as the definition says
    assert _case("n_src0")[3].stats.tolist()[4:] == [0, 3, 0, 0]
    assert _case("n_tgt0")[3].stats.tolist()[4:] == [1, 3, 0, 0]
    assert _case("all_beyond")[3].stats.tolist()[4:] == [1, 3, 0, 0]
    assert _case("two_pairs")[3].stats.tolist()[4:7] == [1, 3, 2]
    assert _case("three_pairs")[3].status == 0 and _case("three_pairs")[3].N == 3
    assert _case("three_collinear")[3].N == 3
    assert _case("max_iter1")[3].stats.tolist()[4:6] == [1, 1]
    assert _case("eps0")[3].stats.tolist()[4:6] == [6, 1]
    assert _case("mse1")[3].stats.tolist()[4:6] == [2, 2]
    inv = _case("invalid")[3]
    assert inv.stats[1] == 6 and inv.stats[3] == 6 and inv.status == 0 and np.isinf(inv.d2[10:16]).all()
    assert not np.isfinite(np.stack([inv.cloud[a] for a in "xyz"], 1)[10:13]).all(1).any()      # a non-finite point stays non-finite
    # a usable source point whose q the cell function rejects: counted as usable, unmatched, carried through the aligned cloud
    tgt, src, kw, qr = _case("q_rejected")
    from tests import voxel_map_ref as VR
    h = R.default_cell(kw["max_corr"])
    assert qr.stats[1] == 0 and qr.stats[3] == 0 and qr.status == 0 and qr.N == 40 and np.isinf(qr.d2[40]) and np.isfinite(qr.d2[:40]).all()
    assert VR.cell_of(tgt, h)[0].all() and VR.cell_of(src, h)[0].tolist() == [True] * 40 + [False] and not VR.cell_of(qr.cloud[40:], h)[0][0]
    from tests.test_sor_gpu import DIRECTIONS
    len2 = np.array([sum(c * c for c in d) for d in DIRECTIONS], np.float64)
    for r in (1, 2, 3):
        tgt, src, kw = IC.CASES["stopping_r%d_at0" % r]()
        st = R.run(tgt, src, **dict(kw, max_iter=1))
        assert st.N == 8 and (st.d2 < len2 * ((r + 0.25) * 0.1) ** 2).all()                    # every query takes the point of ring r + 1, not ring r's


def test_the_order_of_the_input_does_not_matter():
    tgt, src, kw, ref = _case("phys3_origin")
    rng = np.random.default_rng(3)
    pt, ps = rng.permutation(len(tgt)), rng.permutation(len(src))
    got = R.run(tgt[pt], src[ps], **kw)
    assert got.transform.tobytes() == ref.transform.tobytes() and got.stats.tolist() == ref.stats.tolist() and got.history.tolist() == ref.history.tolist()
    assert got.cloud.tobytes() == ref.cloud[ps].tobytes() and got.d2.tobytes() == ref.d2[ps].tobytes()


def test_the_grid_tuning_does_not_matter():
    tgt, src, kw, ref = _case("phys3_origin")
    for cell, rings in ((0.5 / 0.75, 1), (0.5 / 3.75, 4)):
        got = R.run(tgt, src, **dict(kw, cell=cell, max_rings=rings))
        assert got.transform.tobytes() == ref.transform.tobytes() and got.history.tolist() == ref.history.tolist() and got.cloud.tobytes() == ref.cloud.tobytes()


SWEEP_D = [0.95, 1.9, 3.8, 0.5, 0.7, 1.0, 2.0, 0.01, 16.0, 1e-3] + np.random.default_rng(11).uniform(0.0, 16.0, 2000).astype(np.float32).tolist()


def test_the_default_cell_meets_the_create_bound_for_every_max_corr():
    """max_corr / 1.75 in float32 misses (2 - 0.25) cell >= max_corr by one ulp for about one max_corr in twenty (0.95, 1.9, 3.8 ...); the default
    cell is the smallest float32 at or above it that meets the bound, one definition in icp.hpp, the library and the restatement."""
    import ctypes
    import lmono_amd
    L = lmono_amd.load_library()
    plain_fails = 0
    for D in SWEEP_D:
        D = np.float32(D)
        h = R.default_cell(D)
        plain = D / np.float32(1.75)
        plain_fails += not R.params_ok(D, 50, 1e-8, 0.0, plain, 2)
        assert R.params_ok(D, 50, 1e-8, 0.0, h, 2) and h >= plain and h <= np.nextafter(np.nextafter(plain, np.float32(np.inf)), np.float32(np.inf))
        assert h == plain or not R.params_ok(D, 50, 1e-8, 0.0, np.nextafter(h, np.float32(0.0)), 2)          # the smallest such cell
        assert np.float32(L.lmono_icp_default_cell(ctypes.c_float(D))).tobytes() == h.tobytes()
    assert plain_fails > 50 and not R.params_ok(np.float32(0.95), 50, 1e-8, 0.0, np.float32(0.95) / np.float32(1.75), 2)


def test_the_host_program_takes_the_default_cell(tmp_path):
    tgt, src, _ = IC.CASES["phys_origin"]()
    for D in (0.95, 1.9, 3.8):
        kw = dict(max_corr=D, max_iter=3)
        assert [ln for ln in _host_lines(tmp_path, tgt, src, kw) if not ln.startswith("offdiag")] == R.text(R.run(tgt, src, **kw))
