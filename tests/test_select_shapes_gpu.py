"""k_select (edge / planar picks of every sector, one wave per ring) on the sector shapes at which its code takes another path, bit for
bit against the CPU oracle through ScanBatch.scanreg / counts() / cloud(s, 1..4, n) / curvature() (the labels).

Every case first asserts its precondition on the oracle's output alone: _restate() recomputes, in numpy, the gap flags, the reaches, and
per sector the live candidates, the members of the independent set that the sharp picks are the head of, the parallel rounds that
settle it, the picks and their marks, as the kernel defines them (and checks that restatement against the oracle's labels), so a case
cannot silently stop covering its branch.  The kernel as it stands: sectors of up to 320 / 384 / more points run 5 / 6 / 11 elements a
lane (lane = element // M); the sharp picks are settled in rounds (winners join, their reach dies) and the members ranked one per lane;
when more than 64 members come out, those below the 20th largest of the 64 lanes' best member curvatures are left out first (the
filter), and if more than 64 are still left the picks are made one after the other (the sequential loop); rings longer than 2304 points
go through the work list of the second launch.  _restate() gives each sector's path: "ranked", "filter" or "sequential"."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _restate(ref, n_lines):
    """Sectors of a scan from the oracle's ring-sorted cloud, curvature and ring table; returns (list of per-sector dicts, labels)."""
    cloud, cv, rb = ref["cloud"], ref["curvature"], ref["ring_begin"]
    n = len(cloud)
    d = cloud[1:, :3] - cloud[:-1, :3]
    s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]                    # float32, as k_curvature
    gap = np.zeros(n + 16, bool)
    gap[:n - 1] = s.astype(np.float64) > 0.05                                         # gap[i]: between points i and i + 1
    gpad = np.concatenate([np.ones(8, bool), gap])
    lf = np.zeros(n, np.int64); lb = np.zeros(n, np.int64)
    runf = np.ones(n, bool); runb = np.ones(n, bool)
    for k in range(5):
        runf &= ~gap[k:k + n]; lf += runf
        runb &= ~gpad[7 - k:7 - k + n]; lb += runb
    bits = cv.view(np.uint32).astype(np.int64)
    cd = cv.astype(np.float64)
    picked = np.zeros(n + 16, bool)
    lab = np.zeros(n, np.int32)
    secs = []
    for r in range(n_lines):
        beg, end = int(rb[r]), int(rb[r + 1])
        S, E = beg + 5, end - 6
        if E - S < 6:
            continue
        span = E - S
        for j in range(6):
            sp, ep = S + span * j // 6, S + span * (j + 1) // 6 - 1
            idx = np.arange(sp, ep + 1)
            cand = idx[(cd[idx] > 0.1) & ~picked[idx]]
            order = cand[np.lexsort((cand, bits[cand]))][::-1]
            base = max(sp - 8, 0)
            sup = picked[base:ep + 9].copy()
            members = []
            for i in order:
                if sup[i - base]:
                    continue
                members.append(int(i))
                sup[i - lb[i] - base:i + lf[i] + 1 - base] = True
            # the parallel rounds over the same candidates
            m = ep - sp + 1
            key = np.zeros(m + 12, np.int64); live = np.zeros(m + 12, bool)
            key[6 + cand - sp] = bits[cand] * (1 << 20) + (cand - sp) + 1
            live[6 + cand - sp] = True
            f5 = np.zeros(m + 12, np.int64); b5 = np.zeros(m + 12, np.int64)
            f5[6:6 + m] = lf[idx]; b5[6:6 + m] = lb[idx]
            rounds, in_set = 0, np.zeros(m + 12, bool)
            while live.any():
                rounds += 1
                kk = np.where(live, key, 0)
                best = np.zeros(m + 12, np.int64)
                for k in range(1, 6):
                    best[:-k] = np.maximum(best[:-k], np.where(f5[:-k] >= k, kk[k:], 0))
                    best[k:] = np.maximum(best[k:], np.where(b5[k:] >= k, kk[:-k], 0))
                win = live & (kk > best)
                die = win.copy()
                for k in range(1, 6):
                    die[:-k] |= (f5[:-k] >= k) & win[k:]
                    die[k:] |= (b5[k:] >= k) & win[:-k]
                in_set |= win
                live &= ~die
            assert sorted(members) == list(sp + np.flatnonzero(in_set) - 6), "rounds and walk disagree in ring %d sector %d" % (r, j)
            tie = False
            for k in range(1, 6):
                a = cand[(lf[cand] >= k) & (cand + k <= ep)]
                a = a[(cd[a + k] > 0.1) & ~picked[a + k] & (bits[a + k] == bits[a])]
                tie |= len(a) > 0
            # the path the kernel takes: blocked layout, the lanes' best member curvature, the bound, what is left to rank
            M = 5 if m <= 320 else 6 if m <= 384 else 11
            ntop = len(members)
            if len(members) > 64:
                mem = np.array(members)
                best = np.zeros(64, np.int64)
                np.maximum.at(best, (mem - sp) // M, bits[mem])
                above = (best[None, :] > best[:, None]).sum(1)
                bound = best[above < 20].min()
                ntop = int((bits[mem] >= bound).sum())
            path = "ranked" if len(members) <= 64 else "filter" if ntop <= 64 else "sequential"
            picks = members[:20]
            for k, i in enumerate(picks):
                lab[i] = 2 if k < 2 else 1
                picked[i - lb[i]:i + lf[i] + 1] = True
            fc = idx[cd[idx] < 0.1]
            cnt = 0
            for i in fc[np.lexsort((fc, bits[fc]))]:
                if picked[i]:
                    continue
                lab[i] = -1
                cnt += 1
                if cnt >= 4:
                    break
                picked[i - lb[i]:i + lf[i] + 1] = True
            secs.append(dict(ring=r, sector=j, sp=sp - beg, slen=m, ring_len=end - beg, ncand=len(cand), nbig=int((cd[idx] > 0.1).sum()),
                             nmem=len(members), ntop=ntop, path=path, M=M, rounds=rounds, tie=bool(tie), lf_min=int(lf[idx].min()), lf_max=int(lf[idx].max()),
                             lb_min=int(lb[idx].min()), lb_max=int(lb[idx].max()),
                             marks_before=any(i - lb[i] < sp for i in picks), marks_behind=any(i + lf[i] > ep for i in picks)))
    assert np.array_equal(lab, ref["label"]), "the restatement does not reproduce the oracle's labels (%d differ)" % int((lab != ref["label"]).sum())
    return secs


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
        assert list(cnt[s, 1:5]) == [info.n_sharp, info.n_less_sharp, info.n_flat, info.n_less_flat]
        cv, lb = batch.curvature(s, n)
        assert np.array_equal(lb, ref["label"]), "labels of scan %d differ at %s" % (s, np.flatnonzero(lb != ref["label"])[:8])
        for which, name in ((1, "sharp"), (2, "less_sharp"), (3, "flat"), (4, "less_flat")):
            got = batch.cloud(s, which, n)
            assert np.array_equal(got.view(np.uint32), ref[name].view(np.uint32)), "%s cloud of scan %d differs (bitwise)" % (name, s)


@pytest.fixture(scope="module")
def scan16(oracle):
    """One 16-line scan at 2000 azimuth steps in the oracle's ring-sorted order with its ring table: fed again as input it is its own
    ring-sorted cloud, so points can be addressed by (ring, position in the ring)."""
    w = oracle.S1World(n_az=2000, n_rings=16)
    xyzi, off = w.scans(w.trajectory(1))
    ref = oracle.scanreg(xyzi[off[0]:off[1]], 16, 0.5)
    return ref["cloud"].copy(), ref["ring_begin"].copy()


def _set_range(a, beg, end, rho):
    """Points beg .. end - 1 moved along their rays to the ranges rho (same ring, same azimuth)."""
    p = a[beg:end, :3].astype(np.float64)
    a[beg:end, :3] = (p * (np.asarray(rho, np.float64) / np.linalg.norm(p, axis=1))[:, None]).astype(np.float32)


def _long_rings(rb, min_len=1880):
    return [r for r in range(16) if rb[r + 1] - rb[r] >= min_len]


def _one(oracle, gpu_ctx, a, n_lines=16, min_range=0.5, want=None):
    ref = oracle.scanreg(a, n_lines, min_range)
    secs = _restate(ref, n_lines)
    if want is not None:
        want(secs)
    if gpu_ctx is not None:
        _check(gpu_ctx, a, np.array([0, len(a)], np.int64), n_lines, min_range, [ref])
    return secs


def build_staircase(scan16):
    """Ranges 10 m +- a_k in turn over 80 points of three rings, a_k growing from 4 cm by 1 mm a point: the curvature (about 144 a_k^2)
    grows from point to point while every gap stays short, so a round settles one member and its reach only."""
    cloud, rb = scan16
    a = cloud.copy()
    for r in _long_rings(rb)[:3]:                  # (the first is the ring of the second launch, 11 elements a lane)
        beg, n = int(rb[r]), int(rb[r + 1] - rb[r])
        rho = np.full(n, 10.0)
        k = np.arange(80)
        rho[400:480] = 10.0 + (0.04 + 0.001 * k) * (1 - 2 * (k % 2))
        _set_range(a, beg, beg + n, rho)

    def want(secs):
        assert max(s["rounds"] for s in secs) >= 8, sorted(s["rounds"] for s in secs)[-5:]
    return a, want


def build_ties(scan16):
    """Four points (a radial zig-zag) repeated 150 times in three rings: curvatures repeat exactly at distance 4, inside a reach."""
    cloud, rb = scan16
    a = cloud.copy()
    for r in _long_rings(rb)[:3]:
        beg, n = int(rb[r]), int(rb[r + 1] - rb[r])
        _set_range(a, beg, beg + n, np.full(n, 10.0))
        k0 = beg + 300 + r
        _set_range(a, k0, k0 + 4, 10.0 + np.array([0.10, -0.10, 0.12, -0.07]))
        a[k0:k0 + 600, :3] = np.tile(a[k0:k0 + 4, :3], (150, 1))

    def want(secs):
        t = [s for s in secs if s["tie"] and s["ncand"] > 20]
        assert len(t) >= 3, len(t)
    return a, want


def build_every_gap_long(scan16):
    """Every second point of every ring moved radially by +-15 %: no reach, every candidate a member, more than 64 in a sector."""
    cloud, rb = scan16
    rng = np.random.default_rng(5)
    a = cloud.copy()
    pos = np.arange(len(a)) - np.repeat(rb[:16], np.diff(rb[:17]))
    sgn = rng.choice(np.array([-1.0, 1.0], np.float32), len(a))
    a[:, :3] *= np.where(pos % 2 == 1, np.float32(1.0) + np.float32(0.15) * sgn, np.float32(1.0)).astype(np.float32)[:, None]

    def want(secs):
        t = [s for s in secs if s["nmem"] > 64 and s["lf_max"] == 0 and s["lb_max"] == 0]
        assert len(t) >= 10, len(t)
        # the curvatures differ from point to point, so the bound leaves at most 64 to rank in most of them (both layouts of this scan)
        f = [s for s in t if s["path"] == "filter"]
        assert len(f) >= 20 and any(s["M"] == 5 for s in f) and any(s["M"] == 11 for s in f), (len(f), sorted(set(s["M"] for s in f)))
    return a, want


def build_one_curvature_in_more_than_64_members(scan16):
    """Two points of one ray, 3 m apart, in turn along three whole rings (exact copies): every gap long, every candidate a member, and all
    the members on the one point share one curvature, far more than 64 of them in a sector: the bound leaves them all, the picks are made
    one after the other."""
    cloud, rb = scan16
    a = cloud.copy()
    rings = _long_rings(rb)[:3]                   # (the first is the ring of the second launch, 11 elements a lane)
    for r in rings:
        beg, n = int(rb[r]), int(rb[r + 1] - rb[r])
        k0 = beg + n // 2
        _set_range(a, k0, k0 + 2, np.array([10.0, 13.0]))
        a[beg:beg + n, :3] = np.tile(a[k0:k0 + 2, :3], ((n + 1) // 2, 1))[:n]

    def want(secs):
        t = [s for s in secs if s["ring"] in rings and s["path"] == "sequential"]
        assert len(t) >= 12, (len(t), [(s["ring"], s["sector"], s["nmem"], s["ntop"]) for s in secs if s["ring"] in rings])
        assert any(s["M"] == 5 for s in t) and any(s["M"] == 11 for s in t)
        assert min(s["ntop"] for s in t) > 100
    return a, want


def build_every_gap_short_every_point_a_candidate(scan16):
    """Ranges 10 m +- 6 cm in turn along whole rings: every gap short, every point of a sector a candidate."""
    cloud, rb = scan16
    a = cloud.copy()
    for r in range(16):
        beg, n = int(rb[r]), int(rb[r + 1] - rb[r])
        _set_range(a, beg, beg + n, 10.0 + 0.06 * (1 - 2 * (np.arange(n) % 2)))

    def want(secs):
        t = [s for s in secs if s["lf_min"] == 5 and s["lb_min"] == 5]
        assert len(t) >= 30, len(t)
        assert sum(1 for s in t if s["nbig"] == s["slen"]) >= 30
        assert sum(1 for s in t if s["ncand"] == s["slen"]) >= 5           # (the sectors behind it start with the marks of the one before)
    return a, want


def build_few_candidates_and_borders(scan16):
    """Rings on a circle of 10 m (no candidate away from the ring's two ends) with single points moved out by 0.2 m (a short gap: c = 4 at
    the point, 0.04 beside it).  Three rings: sectors with none, one, five and 25 candidates.  Three more: candidates next to both sides
    of a sector border, whose marks land in the neighbouring sector."""
    cloud, rb = scan16
    a = cloud.copy()
    rings = _long_rings(rb)
    assert len(rings) >= 6
    for q, r in enumerate(rings[:6]):
        beg, n = int(rb[r]), int(rb[r + 1] - rb[r])
        rho = np.full(n, 10.0)
        span = n - 11
        sp = [5 + span * j // 6 for j in range(7)]
        if q < 3:
            rho[sp[2] + 100] += 0.2                                             # sector 1: none, sector 2: one
            rho[sp[3] + 20:sp[3] + 120:20] += 0.2                               # sector 3: five
            rho[sp[4] + 10:sp[4] + 310:12] += 0.2 + 0.001 * np.arange(25)       # sector 4: 25
        else:
            for k in (1, 3):                                                    # sectors 2 | 3: next to the border on either side
                rho[sp[3] - 1 - k] += 0.2 + 0.01 * k
                rho[sp[3] + k] += 0.21 + 0.003 * k
        _set_range(a, beg, beg + n, rho)

    def want(secs):
        mine = [s for s in secs if s["ring"] in rings[:3]]
        assert sum(1 for s in mine if s["nbig"] == 0) >= 3
        assert sum(1 for s in mine if s["ncand"] == 1) >= 2
        assert sum(1 for s in mine if 2 <= s["ncand"] < 20) >= 3
        assert sum(1 for s in mine if s["ncand"] > 20 and s["nmem"] > 20) >= 3
        edge = [s for s in secs if s["ring"] in rings[3:6]]
        assert sum(1 for s in edge if s["marks_behind"]) >= 2 and sum(1 for s in edge if s["marks_before"]) >= 2
    return a, want


RING_LENGTHS = [1931, 1937, 2315, 2321, 16, 17, 2304, 2305]      # sectors of 320 / 321 / 384 / 385 points; no sector / one; the work list


def build_lengths(oracle):
    w = oracle.S1World(n_az=3000)
    xyzi, off = w.scans(w.trajectory(1))
    ref0 = oracle.scanreg(xyzi[off[0]:off[1]], 64, 5.0)
    cloud, rb = ref0["cloud"].copy(), ref0["ring_begin"].copy()
    full = np.flatnonzero(np.diff(rb[:65]) >= 2400)
    assert len(full) >= len(RING_LENGTHS)
    chosen = full[np.linspace(0, len(full) - 1, len(RING_LENGTHS)).astype(int)]
    for r, n in zip(chosen, RING_LENGTHS):
        cloud[int(rb[r]) + n:int(rb[r + 1]), 0] = np.nan

    def want(secs):
        by_ring = {}
        for s in secs:
            by_ring.setdefault(s["ring"], []).append(s)
        for r, n in zip(chosen, RING_LENGTHS):
            got = by_ring.get(int(r), [])
            assert (len(got) > 0) == (n >= 17), (n, len(got))
            if n >= 17:
                assert got[0]["ring_len"] == n
            if n in (1931, 1937, 2315, 2321):
                assert max(s["slen"] for s in got) == (n - 11) // 6 and sum(s["ncand"] for s in got) > 0, n
    return cloud, want


def test_staircase_needs_many_rounds(oracle, gpu_ctx, scan16):
    a, want = build_staircase(scan16)
    _one(oracle, gpu_ctx, a, want=want)


def test_equal_curvatures_within_reach(oracle, gpu_ctx, scan16):
    a, want = build_ties(scan16)
    _one(oracle, gpu_ctx, a, want=want)


def test_every_gap_long_more_than_64_members(oracle, gpu_ctx, scan16):
    a, want = build_every_gap_long(scan16)
    _one(oracle, gpu_ctx, a, want=want)


def test_one_curvature_in_more_than_64_members_sequential_loop(oracle, gpu_ctx, scan16):
    a, want = build_one_curvature_in_more_than_64_members(scan16)
    _one(oracle, gpu_ctx, a, want=want)


def test_every_gap_short_every_point_a_candidate(oracle, gpu_ctx, scan16):
    a, want = build_every_gap_short_every_point_a_candidate(scan16)
    _one(oracle, gpu_ctx, a, want=want)


def test_few_candidates_and_picks_next_to_sector_borders(oracle, gpu_ctx, scan16):
    a, want = build_few_candidates_and_borders(scan16)
    _one(oracle, gpu_ctx, a, want=want)


def test_sector_and_ring_lengths(oracle, gpu_ctx):
    a, want = build_lengths(oracle)
    _one(oracle, gpu_ctx, a, 64, 5.0, want=want)


@pytest.mark.parametrize("n_lines", [16, 32, 64])
def test_sensors(oracle, gpu_ctx, n_lines):
    w = oracle.S1World(n_az=600, n_rings=n_lines)
    xyzi, off = w.scans(w.trajectory(1))

    def want(secs):
        assert sum(1 for s in secs if s["ncand"] > 0) >= n_lines
    _one(oracle, gpu_ctx, xyzi[off[0]:off[1]], n_lines, 5.0 if n_lines == 64 else 0.5, want=want)
