"""The voxel-grid colour map restated in numpy from the definition, not from the kernel: float32 operations
spelled out one by one, Python integers for the sums, a dict for the table.  The checker of the voxel-map tests."""
import numpy as np

POINT_RGB = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("bgra", np.uint32)])
F32 = np.float32
LIMIT = F32(1048576.0)


def points(xyz, bgra):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    p = np.zeros(len(xyz), POINT_RGB)
    p["x"] = xyz[:, 0]; p["y"] = xyz[:, 1]; p["z"] = xyz[:, 2]; p["bgra"] = np.asarray(bgra, np.uint32).reshape(-1)
    return p


def cell_of(p, leaf):
    """Per point: accepted [n] bool, cell index [n][3] int64, offset q [n][3] int64 (garbage where not accepted)."""
    inv = F32(1.0) / F32(leaf)
    with np.errstate(all="ignore"):
        t = np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float32) * inv       # float32 multiply
        ok = ((t >= -LIMIT) & (t < LIMIT)).all(1)                                 # NaN and inf fail both comparisons
        t = np.where(ok[:, None], t, F32(0.0))
        c = np.floor(t)                                                           # float32
        f = t - c                                                                 # float32 subtract
        q = np.minimum(65535, (f * F32(65536.0)).astype(np.int64))
    return ok, c.astype(np.int64), q


def key_of(i):
    i = np.asarray(i, np.int64) + (1 << 20)
    return (i[..., 2].astype(np.uint64) << np.uint64(42)) | (i[..., 1].astype(np.uint64) << np.uint64(21)) | i[..., 0].astype(np.uint64)


def mix(keys):
    """The 64-bit mix the table hashes a key with (the finaliser of splitmix64, as the header states it), modulo 2^64."""
    k = np.asarray(keys, np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(30); k *= np.uint64(0xBF58476D1CE4E5B9)
        k ^= k >> np.uint64(27); k *= np.uint64(0x94D049BB133111EB)
        k ^= k >> np.uint64(31)
    return k


def probe_slots(keys, slots):
    """Linear probing of `keys`, in this order, into an empty table of `slots`: the slot each key ends in and whether any probe stepped from the
    last slot to slot 0."""
    start = (mix(keys) & np.uint64(slots - 1)).astype(np.int64)
    used, at, wrapped = set(), [], False
    for h in start:
        h = int(h)
        while h in used:
            wrapped |= h == slots - 1
            h = (h + 1) % slots
        used.add(h); at.append(h)
    return at, wrapped


class VoxelMapRef:
    def __init__(self, leaf):
        self.leaf = F32(leaf)
        self.table = {}            # key -> [count, sx, sy, sz, sr, sg, sb] as Python integers
        self.rejected = 0

    def insert(self, p):
        ok, i, q = cell_of(p, self.leaf)
        self.rejected += int((~ok).sum())
        keys = key_of(i)
        b = p["bgra"].astype(np.int64)
        rgb = np.stack([b >> 16 & 255, b >> 8 & 255, b & 255], 1)
        for k in np.nonzero(ok)[0]:
            r = self.table.setdefault(int(keys[k]), [0] * 7)
            r[0] += 1
            for a in range(3):
                r[1 + a] += int(q[k, a]); r[4 + a] += int(rgb[k, a])
        return self

    def cells(self):
        ks = sorted(self.table)
        keys = np.array(ks, np.uint64)
        counts = np.array([self.table[k][0] for k in ks], np.uint32)
        sums = np.array([self.table[k][1:] for k in ks], np.uint64).reshape(len(ks), 6)
        return keys, counts, sums

    def read(self):
        out = np.zeros(len(self.table), POINT_RGB)
        L = float(self.leaf)                                     # (double)L
        for n, k in enumerate(sorted(self.table)):
            r = self.table[k]
            cnt = r[0]
            idx = [(k & 0x1FFFFF) - (1 << 20), (k >> 21 & 0x1FFFFF) - (1 << 20), (k >> 42 & 0x1FFFFF) - (1 << 20)]
            for a, name in enumerate(("x", "y", "z")):
                out[name][n] = F32((float(idx[a]) + (float(r[1 + a]) + 0.5 * float(cnt)) / (65536.0 * float(cnt))) * L)   # fp64, then one cast
            out["bgra"][n] = (r[6] // cnt) | (r[5] // cnt) << 8 | (r[4] // cnt) << 16 | 0xFF000000
        return out

    def text(self):
        """What lmono_amd/host/voxel_map_test prints for the same points."""
        keys, counts, sums = self.cells()
        pts = self.read()
        lines = ["rejected %d" % self.rejected]
        for n in range(len(keys)):
            bits = [int(np.array(pts[a][n], np.float32).view(np.uint32)) for a in ("x", "y", "z")]
            lines.append("%d %d %s %08x %08x %08x %08x" % (int(keys[n]), int(counts[n]), " ".join(str(int(v)) for v in sums[n]), bits[0], bits[1], bits[2], int(pts["bgra"][n])))
        return "\n".join(lines) + "\n"


def edge_points(leaf=0.1):
    """The edge cases of the definition: the -1e-9 point, negative cells, k * leaf boundaries, colours 0 and 255."""
    L = np.float32(leaf)
    xyz = [[-1e-9, 0.5, 0.5], [-0.05, -0.05, -0.05], [-0.1, -0.2, -0.3], [-299.95, -150.05, -3.31], [0.0, 0.0, 0.0]]
    for k in (-3, -1, 1, 2, 7, 1000, -1000):
        xyz.append([np.float32(k) * L, np.float32(k) * L, np.float32(-k) * L])
        xyz.append([np.nextafter(np.float32(k) * L, np.float32(-1e9), dtype=np.float32), 0.25, np.nextafter(np.float32(k) * L, np.float32(1e9), dtype=np.float32)])
    xyz = np.array(xyz, np.float32)
    bgra = np.array([0xFF000000, 0xFFFFFFFF, 0xFF00FF00, 0xFF0000FF, 0xFFFF0000] * 8, np.uint32)[:len(xyz)]
    return points(xyz, bgra)


def rejected_points():
    big = np.float32(1048576.0 * 0.1 * 1.01)
    xyz = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [big, 0, 0], [0, -big * 2, 0], [0, 0, 3e38], [np.nan, np.nan, np.nan]], np.float32)
    return points(xyz, np.full(len(xyz), 0xFF102030, np.uint32))
