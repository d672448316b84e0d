"""Small built scenes for the scan-to-map refine step (tests/test_map_ref_cpu.py, tests/test_map_refine_edges_gpu.py).  Every scene is a dict
with `name`, `kind` (L H T G S), `path` (the kernel path it is for), the four clouds `cmap smap cstack sstack` ([n,4] float32) and the start
pose `x0`; a few thousand points at most.  Everything is generated from fixed seeds: the scenes are the same in every process.

Lattice scenes (L, H, T and the anchor): coordinates are multiples of 1/8 with magnitude below 64 -- 10 significant bits, so every difference,
square (20 bits) and sum of three squares (22 bits) is exact in float32 whatever the order of the operations, and exact ties abound.  Two H clouds
use multiples of 1/16 (below 64) or 1/64 (below 4): still at most 22 bits, still exact.  The start pose is exactly the identity, the stack points
lie on the map's planes and lines: all residuals vanish, the first solve leaves by the gradient tolerance, the pose bytes do not change and the
queries of the last outer iteration are the stack points themselves."""
import functools

import numpy as np

import map_ref

IDENTITY = map_ref.IDENTITY


def cloud(xyz):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    out = np.zeros((len(xyz), 4), np.float32)
    out[:, :3] = xyz
    return out


def _lattice(xyz, unit=8, bound=64):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    assert np.array_equal(xyz * unit, np.round(xyz * unit)) and np.abs(xyz).max() < bound, "not a lattice cloud"
    return cloud(xyz)


def _grid2(x, y):
    X, Y = np.meshgrid(x, y, indexing="ij")
    return X.ravel(), Y.ravel()


def _scene(name, kind, path, cmap, smap, cstack, sstack, x0=IDENTITY, **extra):
    d = dict(name=name, kind=kind, path=path, cmap=np.asarray(cmap, np.float32).reshape(-1, 4), smap=np.asarray(smap, np.float32).reshape(-1, 4),
             cstack=np.asarray(cstack, np.float32).reshape(-1, 4), sstack=np.asarray(sstack, np.float32).reshape(-1, 4), x0=np.array(x0, np.float64))
    d.update(extra)
    return d


# ---- lattice pieces --------------------------------------------------------------------------------------------------------
def _corner_lines():
    """Three axis-parallel lattice lines, 1/4 apart along each, more than 2 m from one another; and queries on them at every 1/8: lattice points
    (five distinct distances) and midpoints (the fifth neighbour is one of two at the same distance: the lower index wins)."""
    t = np.arange(-8, 8.01, 0.25)
    pts = np.concatenate([np.stack([t, 0 * t + 5, 0 * t + 1], 1), np.stack([0 * t - 3, t, 0 * t - 2], 1), np.stack([0 * t - 7, 0 * t - 7, t], 1)])
    q = np.arange(-7, 7.01, 0.125)
    qs = np.concatenate([np.stack([q, 0 * q + 5, 0 * q + 1], 1), np.stack([0 * q - 3, q, 0 * q - 2], 1), np.stack([0 * q - 7, 0 * q - 7, q], 1)])
    return pts, qs


def _patch(origin, offsets):
    return np.asarray(origin, np.float64)[None] + np.asarray(offsets, np.float64) / 8.0


def lattice_scene():
    """L: the exact search.  Surf map = the plane z = 2: a dense square (1/4 apart, some points twice, order shuffled) and isolated five-point
    patches around single queries; corner map = three lattice lines."""
    rng = np.random.default_rng(101)
    gx, gy = _grid2(np.arange(-4, 4, 0.25), np.arange(-4, 4, 0.25))
    dense = np.stack([gx, gy, 0 * gx + 2], 1)
    dup = dense[rng.choice(len(dense), 60, replace=False)]                   # duplicated map points: ties go to the lower index
    surf = [dense, dup]
    queries, note = [], {}

    def add(tag, origin, offsets, q_off=(0, 0, 0)):
        surf.append(_patch(origin, offsets))
        note[tag] = sum(len(q) for q in queries)
        queries.append(_patch(origin, [q_off]))
    z = 0
    # the fifth neighbour at squared distance exactly 1.0: refused (d5 < 1.0 is strict)
    add("fifth_at_1", (12, 12, 2), [(0, 0, z), (1, 0, z), (0, 1, z), (-1, 0, z), (8, 0, z)])
    add("fifth_at_1_neg", (-12, -12, 2), [(0, 0, z), (1, 0, z), (0, -8, z), (-1, 0, z), (0, 1, z)])
    # the fifth neighbour at 61/64, the largest in-plane lattice value below 1 (61 = 36 + 25): accepted.  (1 - 1/64 itself cannot occur: 63 * 4^k
    # is of the form 4^a (8 b + 7), never a sum of three squares, on any dyadic lattice; in the plane 62 = 2 * 31 is no sum of two squares either.)
    add("fifth_below_1", (12, -12, 2), [(0, 0, z), (1, 0, z), (0, 1, z), (-1, 0, z), (6, 5, z)])
    add("fifth_below_1_tie", (-12, 12, 2), [(0, 0, z), (1, 0, z), (0, 1, z), (-1, 0, z), (6, 5, z), (5, 6, z), (-6, 5, z)])
    # the five nearest in a diagonal neighbour cell only: the query's own cell and the two face neighbours are empty
    add("diagonal_cell", (20, 20, 2), [(-1, -1, z), (-2, -1, z), (-1, -2, z), (-2, -2, z), (-3, -1, z)], (1, 1, 0))
    add("diagonal_cell_neg", (-20, -20, 2), [(1, 1, z), (2, 1, z), (1, 2, z), (2, 2, z), (3, 1, z)], (-1, -1, 0))
    add("diagonal_cell_mixed", (-20, 20, 2), [(1, -1, z), (2, -1, z), (1, -2, z), (2, -2, z), (3, -3, z)], (-1, 1, 0))
    # fewer than five map points in reach
    add("three_in_reach", (20, -20, 2), [(0, 0, z), (1, 0, z), (0, 1, z)])
    add("four_in_reach_fifth_far", (28, 0, 2), [(0, 0, z), (1, 0, z), (0, 1, z), (2, 2, z), (24, 0, z)])
    smap = np.concatenate(surf)
    smap = smap[rng.permutation(len(smap))]
    # queries of the dense square: every integer corner (cell corners and faces, both signs), lattice points, cell centres of the 1/4 grid (four
    # nearest at one distance, the fifth among eight), and points of the 1/8 lattice at random
    ix, iy = _grid2(np.arange(-3, 4, 1.0), np.arange(-3, 4, 1.0))
    hx, hy = _grid2(np.arange(-3, 3, 0.25) + 0.125, np.arange(-3, 3, 0.5) + 0.125)
    r = rng.integers(-24, 25, (500, 2)) / 8.0
    queries += [np.stack([ix, iy, 0 * ix + 2], 1), np.stack([hx, hy, 0 * hx + 2], 1), np.concatenate([r, np.full((500, 1), 2.0)], 1), dup[:20]]
    cpts, cq = _corner_lines()
    cpts = np.concatenate([cpts, cpts[5:15]])                                 # duplicated corner points
    return _scene("L_lattice", "L", "k_grid_* one wave per run, k_map_correspond ties / faces / d5 gate", _lattice(cpts[rng.permutation(len(cpts))]), _lattice(smap),
                  _lattice(cq), _lattice(np.concatenate(queries)), note=note)


def _block9_cells(n):
    """n distinct 1 m cells of the plane z = 2 with one lattice point each.  Cells come in 3 x 3 blocks whose nine points crowd around the
    block's centre (0.875, 1.375, 2.0 along each axis: 0.5 and 0.625 apart), so a query there has its five nearest in five different cells;
    blocks spiral out from the origin over both signs."""
    f = (0.875, 0.375, 0.0)
    side = int(np.ceil(np.sqrt(n / 9.0))) + 1
    blocks = sorted(((a, b) for a in range(-side, side) for b in range(-side, side)), key=lambda ab: (max(abs(ab[0] + 0.5), abs(ab[1] + 0.5)), ab))
    pts, centres = [], []
    for a, b in blocks:
        centres.append((3 * a + 1.375, 3 * b + 1.375, 2.0))
        for v in range(3):
            for u in range(3):
                pts.append((3 * a + u + f[u], 3 * b + v + f[v], 2.0))
    pts = np.array(pts[:n])
    cells = np.floor(pts[:, :2]).astype(int)
    assert len(set(map(tuple, cells))) == n and cells.min() < 0
    return pts, np.array(centres[:(n + 8) // 9 + 2])


def hash_scene(n):
    """H: a surf map of n points in n distinct cells (n = 2^k - 1: the table has n + 1 slots, one of them empty; n = 2^k: twice as many)."""
    pts, centres = _block9_cells(n)
    off = np.array([(0, 0, 0), (5, 5, 0), (-3, -3, 0), (5, -3, 0), (2, 0, 0), (0, -11, 0), (12, 12, 0)]) / 8.0   # centre point, the integer corner, ...
    q = (centres[:, None, :] + off[None]).reshape(-1, 3)
    cpts, cq = _corner_lines()
    return _scene("H_%d" % n, "H", "k_grid_insert / probes at table load n / T, T = %d" % max(1024, 1 << int(n).bit_length()), _lattice(cpts), _lattice(pts),
                  _lattice(cq[::7]), _lattice(q))


def single_cell_scene():
    """H: 5000 surf points in ONE cell, in input order (4096 positions of the 1/64 lattice of the cell [1,2) x [1,2) on the plane z = 2, row by row,
    904 of them twice in a row): one run of 5000 through k_grid_insert -- 78 waves, both `u` halves, every workgroup."""
    rng = np.random.default_rng(102)
    gx, gy = _grid2(1 + np.arange(64) / 64.0, 1 + np.arange(64) / 64.0)
    rep = np.ones(4096, int); rep[rng.choice(4096, 904, replace=False)] = 2
    pts = np.repeat(np.stack([gx, gy, 0 * gx + 2], 1), rep, axis=0)
    assert len(pts) == 5000
    q = np.concatenate([rng.integers(64, 128, (400, 2)) / 64.0, np.full((400, 1), 2.0)], 1)      # inside: from the far side of an edge the five nearest can be collinear
    q = np.concatenate([q, [(1, 1, 2), (3.0, 1.5, 2)]])          # the cell's corner; nothing within 1 m of the last one
    cpts, cq = _corner_lines()
    return _scene("H_single_cell", "H", "k_grid_insert runs longer than a wave, across i0 / i0 + stride", _lattice(cpts), _lattice(pts, 64, 4), _lattice(cq[::7]), _lattice(q, 64, 4))


def interrupted_cell_scene():
    """H: the same cell comes back after an interruption: runs of cells A, B, A, C, A, ... of lengths around and across the 64-lane wave."""
    rng = np.random.default_rng(103)
    corner = {"A": (1, 1), "B": (2, 1), "C": (-3, -2), "D": (1, 2)}
    free = {k: list(rng.permutation(256)) for k in corner}
    pts = []
    for cell, length in (("A", 70), ("B", 30), ("A", 64), ("C", 1), ("A", 63), ("D", 65), ("B", 100), ("A", 40), ("C", 130), ("D", 2), ("A", 19)):
        for _ in range(length):
            k = free[cell].pop()
            pts.append((corner[cell][0] + (k % 16) / 16.0, corner[cell][1] + (k // 16) / 16.0, 2.0))
    pts = np.array(pts)
    # queries inside the cell that came back four times (A, full: all 256 positions), and far ones that find nothing
    q = np.concatenate([np.concatenate([rng.integers(20, 29, (300, 2)) / 16.0, np.full((300, 1), 2.0)], 1), [(8, 8, 2), (-8.5, 3, 2)]])
    cpts, cq = _corner_lines()
    return _scene("H_interrupted", "H", "k_grid_insert: a cell claimed again by a later run", _lattice(cpts), _lattice(pts, 16), _lattice(cq[::7]), _lattice(q, 16))


# ---- anchor: three orthogonal lattice planes and three lattice lines ---------------------------------------------------------
def _anchor(rng, n_cs=150, n_ss=450):
    h = np.arange(-6, 6.01, 0.5); v = np.arange(-1, 5.01, 0.5)
    ax, ay = _grid2(h, h); bx, bz = _grid2(h, v)
    planes = [np.stack([ax, ay, 0 * ax - 2], 1), np.stack([0 * bx - 7, bx, bz], 1), np.stack([bx, 0 * bx + 7, bz], 1)]
    t = np.arange(-6, 6.01, 0.25)
    lines = [np.stack([t, 0 * t, 0 * t + 1], 1), np.stack([0 * t + 2, t, 0 * t + 3], 1), np.stack([0 * t - 4, 0 * t - 4, t], 1)]
    a = rng.integers(-40, 41, (n_ss, 2)) / 8.0; bz_ = rng.integers(0, 33, n_ss) / 8.0
    which = np.arange(n_ss) % 3
    ss = np.where((which == 0)[:, None], np.stack([a[:, 0], a[:, 1], 0 * bz_ - 2], 1),
                  np.where((which == 1)[:, None], np.stack([0 * bz_ - 7, a[:, 0], bz_], 1), np.stack([a[:, 0], 0 * bz_ + 7, bz_], 1)))
    s = rng.integers(-40, 41, n_cs) / 8.0
    which = np.arange(n_cs) % 3
    cs = np.where((which == 0)[:, None], np.stack([s, 0 * s, 0 * s + 1], 1),
                  np.where((which == 1)[:, None], np.stack([0 * s + 2, s, 0 * s + 3], 1), np.stack([0 * s - 4, 0 * s - 4, s], 1)))
    return planes, lines, cs, ss


def threshold_scenes():
    """T: the solve runs only when the corner map has MORE than 10 and the surf map MORE than 50 points."""
    planes, lines, _, _ = _anchor(np.random.default_rng(104))
    cs = lines[0][2:9] + np.array([0.125, 0, 0]); ss = planes[0][[27, 28, 29, 52, 53]] + np.array([0.125, 0.125, 0])
    out = []
    for nc, ns in ((10, 51), (11, 50), (11, 51)):
        out.append(_scene("T_%d_%d" % (nc, ns), "T", "n_map > 10 / > 50 in k_map_correspond", _lattice(lines[0][:nc]), _lattice(planes[0][:ns]), _lattice(cs), _lattice(ss),
                          solves=nc > 10 and ns > 50))
    return out


# ---- G: the gates ----------------------------------------------------------------------------------------------------------
def _sites(rng):
    """Cluster centres 5 m apart (+- 0.45 of jitter, radius <= 0.5: more than 3 m between the points of two clusters), outside the anchor's box."""
    g = np.arange(-50, 50.1, 5.0)
    out = [(x, y, z) for z in (12.0, -12.0) for x in g for y in g if max(abs(x), abs(y)) > 10]
    out = np.array(out)
    return out[rng.permutation(len(out))]


def _frame(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def _zero_mean_basis(rng):
    q, _ = np.linalg.qr(np.concatenate([np.ones((5, 1)), rng.normal(size=(5, 3))], 1))
    return q[:, 1:]


def _corner_clusters(rng, sites):
    """(points [m,5,3] float32, queries [m,3] float32, kind tags)."""
    P, tags = [], []
    k = 0
    for side in (+1, -1):
        for m in 10.0 ** rng.uniform(-6, -1, 290):
            c = sites[k] + rng.uniform(-0.45, 0.45, 3); k += 1
            F, B = _frame(rng), _zero_mean_basis(rng)
            s2 = 0.35; s1 = s2 / np.sqrt(3.0 * (1.0 + side * m)); s0 = rng.uniform(0, 1) * s1
            P.append(c[None] + s2 * B[:, 0:1] * F[:, 0][None] + s1 * B[:, 1:2] * F[:, 1][None] + s0 * B[:, 2:3] * F[:, 2][None])
            tags.append("drawn")
    h = 0.25
    for axes in ((0, 1), (1, 2), (2, 0), (0, 2)):
        c = np.round(sites[k] * 8) / 8; k += 1
        e = np.eye(3)
        P.append(c[None] + h * np.array([0 * e[0], e[axes[0]], -e[axes[0]], e[axes[1]], -e[axes[1]]])); tags.append("two_equal")     # ev = 0, 2 h^2, 2 h^2
        c = np.round(sites[k] * 8) / 8; k += 1
        P.append(c[None] + 0.5 * h * np.outer([-2, -1, 0, 1, 2], e[axes[0]] + e[axes[1]])); tags.append("collinear")                       # ev = 0, 0, 5 h^2
        c = np.round(sites[k] * 8) / 8; k += 1
        P.append(c[None] + h * np.outer([0, 0, 0, 0, 1], e[axes[0]] - e[axes[1]])); tags.append("four_coincide")                     # ev = 0, 0, 1.6 h^2
    P = np.array(P).astype(np.float32)
    Q = np.zeros((len(P), 3), np.float32)
    for i, p in enumerate(P):
        g = map_ref.line_gate(p)
        Q[i] = g.centre + rng.uniform(-0.15, 0.15) * g.direction
    return P, Q, tags, k


def _fit_offset(base, normal, target):
    """h so that the worst of the five points, the first one lifted by h along the normal, is `target` from the fitted plane (bisection)."""
    def worst(h):
        p = base.copy(); p[0] += h * normal
        return map_ref.plane_gate(p).max_dist
    lo, hi = 0.05, 0.6
    if not worst(lo) < target < worst(hi):
        return None
    for _ in range(44):
        mid = 0.5 * (lo + hi)
        if worst(mid) < target: lo = mid
        else: hi = mid
    return 0.5 * (lo + hi)


def _surf_clusters(rng, sites, k):
    P, tags = [], []
    def lifted(c, F, tag, side, m):
        base = c[None] + rng.uniform(-0.25, 0.25, (5, 1)) * F[:, 0][None] + rng.uniform(-0.25, 0.25, (5, 1)) * F[:, 1][None]
        h = _fit_offset(base, F[:, 2], 0.2 + side * m)
        if h is None or h > 0.35:
            return False
        base[0] += h * F[:, 2]
        P.append(base); tags.append(tag)
        return True
    for side in (+1, -1):
        for m in 10.0 ** rng.uniform(-6, -2, 270):
            for _ in range(50):
                if lifted(sites[k] + rng.uniform(-0.45, 0.45, 3), _frame(rng), "drawn", side, m):
                    break
            k += 1
        # planes through the origin's neighbourhood: the fitted x is large, 1 / |x| small
        for m in 10.0 ** rng.uniform(-6, -2, 12):
            c = sites[k] + rng.uniform(-0.45, 0.45, 3); k += 1
            done = False
            for _ in range(50):
                if done:
                    break
                e = np.cross(c, rng.normal(size=3)); e /= np.linalg.norm(e)
                sin = rng.uniform(0.05, 0.5) / np.linalg.norm(c)
                n = e * np.sqrt(1 - sin * sin) + c / np.linalg.norm(c) * sin
                u = np.cross(n, rng.normal(size=3)); u /= np.linalg.norm(u)
                done = lifted(c, np.stack([u, np.cross(n, u), n], 1), "near_origin", side, m)
    # axis-aligned lattice planes: one column of A is constant, every point on the plane
    for axis in (0, 1, 2):
        for _ in range(2):
            c = np.round(sites[k] * 8) / 8; k += 1
            o = np.array([(0, 0), (2, 1), (-1, 2), (-2, -2), (1, -1)]) / 8.0
            p = np.repeat(c[None], 5, 0); p[:, (axis + 1) % 3] += o[:, 0]; p[:, (axis + 2) % 3] += o[:, 1]
            P.append(p); tags.append("constant_column")
    # a zero column: five points of the plane x = 0 (a line fit in y, z; the fit's last pivot column is exactly zero), on both sides of the limit;
    # two zero columns: points of the z axis
    for j in range(20):
        a = rng.uniform(0, np.pi)
        u, n = np.array([0.0, np.cos(a), np.sin(a)]), np.array([0.0, -np.sin(a), np.cos(a)])
        c = np.array([0.0, (1 - 2 * (j % 2)) * (15.0 + 4.0 * (j // 2)), 24.0])                 # 4 m apart, 12 m from the cluster layers
        base = c[None] + rng.uniform(-0.3, 0.3, (5, 1)) * u[None]
        base[0] += (0.15, 0.2, 0.25, 0.3, 0.35)[j % 5] * n
        P.append(base); tags.append("zero_column")
    for z0, spread in ((36.0, 0.1), (-36.0, 0.12), (44.0, 0.3), (-44.0, 0.33)):
        P.append(np.stack([np.zeros(5), np.zeros(5), z0 + spread * np.array([-1.0, -0.4, 0.1, 0.5, 1.0])], 1)); tags.append("two_zero_columns")
    P = np.array(P).astype(np.float32)
    Q = np.zeros((len(P), 3), np.float32)
    for i, p in enumerate(P):
        g = map_ref.plane_gate(p)
        c = p.astype(np.float64).mean(axis=0)
        Q[i] = c - (c @ g.normal + g.d) * g.normal
    return P, Q, tags


MIN_MARGIN = 1e-9


@functools.lru_cache(maxsize=None)
def gate_scene():
    """G: one isolated cluster of exactly five map points per query.  Clusters whose reference margin is below 1e-9 are discarded (double rounding
    cannot flip a decision that far out); every kept cluster is compared.  Cluster c of the corner map sits at map indices 5 c .. 5 c + 4 in front
    of the anchor's lines (the surf map likewise), its query at stack index c in front of the anchor's stack points."""
    rng = np.random.default_rng(105)
    sites = _sites(rng)
    planes, lines, cs, ss = _anchor(rng)
    Pc, Qc, tc, k = _corner_clusters(rng, sites)
    Ps, Qs, ts = _surf_clusters(rng, _sites(rng), 0)
    lg = [map_ref.line_gate(p) for p in Pc]; pg = [map_ref.plane_gate(p) for p in Ps]
    keep_c = [i for i, g in enumerate(lg) if g.margin >= MIN_MARGIN]
    keep_s = [i for i, g in enumerate(pg) if g.margin >= MIN_MARGIN]
    Pc, Qc, tc, lg = Pc[keep_c], Qc[keep_c], [tc[i] for i in keep_c], [lg[i] for i in keep_c]
    Ps, Qs, ts, pg = Ps[keep_s], Qs[keep_s], [ts[i] for i in keep_s], [pg[i] for i in keep_s]
    cmap = np.concatenate([Pc.reshape(-1, 3).astype(np.float64)] + lines); smap = np.concatenate([Ps.reshape(-1, 3).astype(np.float64)] + planes)
    return _scene("G_gates", "G", "k_map_factor: sym_eig3 near ev2 = 3 ev1, plane_fit5 near 0.2, rank-deficient fits", cloud(cmap), cloud(smap),
                  cloud(np.concatenate([Qc.astype(np.float64), cs])), cloud(np.concatenate([Qs.astype(np.float64), ss])),
                  corner_clusters=Pc, surf_clusters=Ps, corner_tags=tc, surf_tags=ts, line_gates=lg, plane_gates=pg)


# ---- S: the solve's branches -------------------------------------------------------------------------------------------------
def _pose(rot_deg=(0, 0, 0), t=(0, 0, 0)):
    r = np.radians(np.asarray(rot_deg, np.float64)) / 2
    x = map_ref.IDENTITY.copy()
    for axis in range(3):
        d = np.zeros(6); d[axis] = r[axis]
        x = map_ref._plus(x, d)
    x[4:] = t
    return x


def _solver_scene(name, tag, x0, noise=0.0, seed=0, planes_used=(0, 1, 2), lines_used=(0, 1, 2), corner_stack=True, surf_stack=True, outliers=0.0, far=False,
                  n_cs=150, n_ss=450, **pins):
    rng = np.random.default_rng(200 + seed)
    planes, lines, cs, ss = _anchor(rng, n_cs, n_ss)
    cm = np.concatenate([lines[i] for i in lines_used]); sm = np.concatenate([planes[i] for i in planes_used])
    cs = cs[np.isin(np.arange(len(cs)) % 3, lines_used)]; ss = ss[np.isin(np.arange(len(ss)) % 3, planes_used)]
    if noise:
        cm = cm + rng.normal(0, noise, cm.shape); sm = sm + rng.normal(0, noise, sm.shape)
        cs = cs + rng.normal(0, noise, cs.shape); ss = ss + rng.normal(0, noise, ss.shape)
    if outliers:                                   # stack points pushed 0.3 .. 0.6 m off their plane or line: Huber's linear part
        for st in (cs, ss):
            hit = rng.random(len(st)) < outliers
            st[hit] += rng.choice([-1, 1], (hit.sum(), 3)) * rng.uniform(0.3, 0.6, (hit.sum(), 3))
    if far:
        cs = cs + 30.0; ss = ss + 30.0
    if not corner_stack: cs = cs[:0]
    if not surf_stack: ss = ss[:0]
    return _scene(name, "S", "k_map_solve: " + tag, cloud(cm), cloud(sm), cloud(cs), cloud(ss), x0, tag=tag, **pins)


def solver_scenes():
    """S: the anchor, exact or with off-lattice noise, one scene per way through the trust-region loop; `tag` is the branch that map_ref.refine's
    trace of the scene must contain and `traces` the whole expected trace of the two solves (asserted in tests/test_map_ref_cpu.py); `zero` lists
    the stats that must be zero (a class without blocks)."""
    make = lambda *a, **k: out.append(_solver_scene(*a, **k))
    out = []
    make("S_converged", "grad_exit_start", _pose())
    make("S_near_exact", "param_tol", _pose(t=(1e-5, -1e-5, 1e-5)))
    make("S_near_noisy", "func_tol", _pose(t=(1e-5, -1e-5, 1e-5)), noise=0.02, seed=1)
    make("S_far", "func_tol", _pose((2, -2, 2), (0.3, -0.3, 0.3)), noise=0.02, seed=2)
    make("S_outliers", "cost_only_last", _pose((1, 1, -1), (0.2, 0.2, -0.2)), noise=0.02, seed=3, outliers=0.7)
    make("S_one_plane", "func_tol", _pose((0, 0, 0), (0.0, 0.0, 0.1)), noise=0.02, seed=4, planes_used=(0,), corner_stack=False)
    make("S_one_line", "cost_only_last", _pose((0, 0, 0), (0.0, 0.1, 0.1)), noise=0.02, seed=5, lines_used=(0,), surf_stack=False)
    make("S_corner_only", "func_tol", _pose((1, 0, 0), (0.1, 0.0, 0.1)), noise=0.02, seed=6, surf_stack=False)
    make("S_surf_only", "func_tol", _pose((0, 1, 0), (0.1, 0.1, 0.0)), noise=0.02, seed=7, corner_stack=False)
    make("S_no_block", "n_used_zero", _pose(), noise=0.02, seed=8, far=True)
    # under-determined problems of a few blocks (found by a search over seeds and start poses): here a step can raise the cost
    few = dict(noise=0.15, n_cs=3, corner_stack=False)
    make("S_reject", "reject", [0.015914849186495886, -0.012171581027740942, 0.01585231143152608, 0.9996735839327426, -0.11290112879370873, -0.046004130616454586,
                                0.19662155629226502], seed=1000, n_ss=6, **few)
    make("S_reject_last", "max_iter", [-0.013941552575912031, -0.0008840401384293177, 0.004856611889597462, 0.9998906264715958, -0.0695907489052141,
                                       0.2924636056297723, -0.0564067367106611], seed=1074, n_ss=6, **few)
    make("S_grad_after_step", "grad_exit_step", [-0.0007871901907315989, 0.016769596608348192, 0.016120580715246448, 0.9997291072278531, 0.1348739644641202,
                                                 0.02473611332846054, -0.1338652775727775], seed=1004, n_ss=3, **few)
    for sc in out:
        sc["stats"], sc["traces"] = S_EXPECT[sc["name"]]
    return out


_A3, _A2, _A1 = ["accept", "accept", "accept", "cost_only_last", "accept"], ["accept", "accept", "func_tol"], ["accept", "func_tol"]
_R = ["reject", "reuse_diagonal", "reject", "reject", "cost_only_last"]
# what map_ref.refine gives on every S scene: the six stats (a class without blocks shows as zeros) and the traces of the two solves
S_EXPECT = {
    "S_converged": ([150, 150, 450, 450, 0, 0], [["grad_exit_start"], ["grad_exit_start"]]),
    "S_near_exact": ([150, 150, 450, 450, 2, 1], [["accept", "param_tol"], ["param_tol"]]),
    "S_near_noisy": ([150, 150, 450, 450, 2, 2], [_A1, _A1]),
    "S_far": ([150, 150, 450, 450, 3, 2], [_A2, _A1]),
    "S_outliers": ([115, 142, 424, 450, 4, 4], [_A3, _A3]),
    "S_one_plane": ([0, 0, 150, 150, 3, 2], [_A2, _A1]),
    "S_one_line": ([50, 50, 0, 0, 4, 4], [_A3, _A3]),
    "S_corner_only": ([150, 150, 0, 0, 3, 2], [_A2, _A1]),
    "S_surf_only": ([0, 0, 450, 450, 3, 2], [_A2, _A1]),
    "S_no_block": ([0, 0, 0, 0, 0, 0], [["n_used_zero"], ["n_used_zero"]]),
    "S_reject": ([0, 0, 5, 4, 4, 4], [_R + ["accept"], _A3]),
    "S_reject_last": ([0, 0, 5, 5, 4, 4], [_A3, _R + ["reject", "max_iter"]]),
    "S_grad_after_step": ([0, 0, 2, 3, 4, 3], [_A3, ["accept", "accept", "accept", "grad_exit_step"]]),
}


# ---- all of them, and the batch ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_scenes():
    s = [lattice_scene()] + [hash_scene(n) for n in (1023, 1024, 2047, 2048)] + [single_cell_scene(), interrupted_cell_scene()]
    return tuple(s + threshold_scenes() + [gate_scene()] + solver_scenes())


def by_name(name):
    return next(s for s in all_scenes() if s["name"] == name)


def batch_streams():
    """B: 13 different streams of different sizes: an empty map, empty stacks, and one with far more queries than the rest (it alone sets the
    launch's max_nq; the others take the grid-stride tail).  The first 8 and the first 9 are used as batches of their own."""
    rng = np.random.default_rng(106)
    far, noisy = by_name("S_far"), by_name("S_near_noisy")
    _, _, cs, ss = _anchor(rng, 1500, 4500)
    many = _scene("B_many_queries", "B", "max_nq", noisy["cmap"], noisy["smap"], cloud(cs + rng.normal(0, 0.02, cs.shape)), cloud(ss + rng.normal(0, 0.02, ss.shape)),
                  _pose((1, -1, 1), (0.1, -0.1, 0.1)))
    no_map = _scene("B_empty_map", "B", "n_map = 0", np.zeros((0, 4)), np.zeros((0, 4)), far["cstack"], far["sstack"], _pose((3, 0, 1), (1, 2, 3)))
    no_stack = _scene("B_empty_stacks", "B", "nq = 0", far["cmap"], far["smap"], np.zeros((0, 4)), np.zeros((0, 4)), _pose((0, 3, 1), (3, 2, 1)))
    order = [many, "S_far", "H_1023", "S_outliers", no_map, "G_gates", "S_near_noisy", no_stack, "T_11_51", "H_interrupted", "S_one_plane", "L_lattice", "S_corner_only"]
    streams = [by_name(s) if isinstance(s, str) else s for s in order]
    assert len(streams) == 13
    return streams
