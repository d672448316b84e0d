"""tests/track_ref.py -- CPU restatement of the device feature tracker, numpy only.  Test infrastructure: the
kernels of lmono_amd/csrc/track.hip and this file implement one written definition; every accumulation is an exact integer
and every floating-point step is a single IEEE fp32 / fp64 operation in the order written here, so "equal" means equal bytes.
Restates FeatureTracker::trackImage (mono_lidar_mapping/src/image_process/FeatureTracker.cc:189-433) with use_rejectF = 0."""
import numpy as np

WIN = 21
HALF = 10
MAX_LEVEL = 3
MAX_ITERS = 30
MAX_POINTS = 512
F32 = np.float32

RECORD = np.dtype([("id", np.int32), ("x_n", np.float32), ("y_n", np.float32), ("u", np.float32), ("v", np.float32),
                   ("vx", np.float32), ("vy", np.float32), ("track_cnt", np.int32)])


def reflect101(i, n):
    """BORDER_REFLECT_101 for indices at most n - 1 outside [0, n)."""
    i = np.abs(np.asarray(i))
    return np.where(i >= n, 2 * (n - 1) - i, i)


def bgr_to_grey(bgr):
    """cv::cvtColor BGR2GRAY for 8-bit images (FeatureTracker.cc:193)."""
    b = bgr[..., 0].astype(np.int32); g = bgr[..., 1].astype(np.int32); r = bgr[..., 2].astype(np.int32)
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)


def pyr_down(img):
    h, w = img.shape
    ow, oh = (w + 1) // 2, (h + 1) // 2
    k = np.array([1, 4, 6, 4, 1], np.int32)
    a = img.astype(np.int32)
    xs = reflect101(2 * np.arange(ow)[:, None] + np.arange(-2, 3)[None, :], w)
    rows = (a[:, xs] * k[None, None, :]).sum(2)
    ys = reflect101(2 * np.arange(oh)[:, None] + np.arange(-2, 3)[None, :], h)
    out = (rows[ys, :] * k[None, :, None]).sum(1)
    return ((out + 128) >> 8).astype(np.uint8)


def n_levels(w, h):
    """cv::buildOpticalFlowPyramid: a level exists while both of its sides exceed the window (level 0 always)."""
    n = 1
    while n <= MAX_LEVEL:
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= WIN or h <= WIN:
            break
        n += 1
    return n


def scharr(img):
    """[3 10 3] (x) [-1 0 1] derivatives as int16, BORDER_REFLECT_101."""
    p = np.pad(img.astype(np.int32), 1, mode="reflect")
    sm_v = 3 * p[:-2, :] + 10 * p[1:-1, :] + 3 * p[2:, :]       # smoothed over rows, all padded columns
    dx = sm_v[:, 2:] - sm_v[:, :-2]
    sm_h = 3 * p[:, :-2] + 10 * p[:, 1:-1] + 3 * p[:, 2:]
    dy = sm_h[2:, :] - sm_h[:-2, :]
    return dx.astype(np.int16), dy.astype(np.int16)


def build_pyramid(img):
    """-> list of (image u8, dx i16, dy i16) per level."""
    h, w = img.shape
    levels = []
    cur = np.ascontiguousarray(img, np.uint8)
    for l in range(n_levels(w, h)):
        if l > 0:
            cur = pyr_down(cur)
        dx, dy = scharr(cur)
        levels.append((cur, dx, dy))
    return levels


def sobel_box(img):
    """3 x 3 Sobel of the u8 image and 3 x 3 box sums of dx^2, dx dy, dy^2 (both BORDER_REFLECT_101) as int32."""
    p = np.pad(img.astype(np.int32), 1, mode="reflect")
    dx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    dy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])

    def box(a):
        q = np.pad(a, 1, mode="reflect")
        h, w = a.shape
        return sum(q[i:i + h, j:j + w] for i in range(3) for j in range(3)).astype(np.int32)
    return box(dx * dx), box(dx * dy), box(dy * dy)


RESP_SCALE = 1.0 / (12.0 * 255.0)          # cv::cornerMinEigenVal: 1 / (2^(aperture - 1) * block_size) / 255
RESP_SCALE2 = RESP_SCALE * RESP_SCALE


def min_eig_response(sxx, sxy, syy):
    a = sxx.astype(np.float64) * RESP_SCALE2
    b = sxy.astype(np.float64) * RESP_SCALE2
    c = syy.astype(np.float64) * RESP_SCALE2
    d = a - c
    return (0.5 * (a + c) - np.sqrt((0.25 * d) * d + b * b)).astype(np.float32)


def response(img):
    return min_eig_response(*sobel_box(img))


def circle_spans(r):
    """Half widths hw[|dy|], |dy| <= r, of the rows of cv::circle(img, c, r, colour, -1) (filled midpoint circle)."""
    hw = np.zeros(r + 1, np.int32)
    err, dx, dy, plus, minus = 0, r, 0, 1, 2 * r - 1
    while dx >= dy:
        hw[dy] = max(hw[dy], dx)
        hw[dx] = max(hw[dx], dy)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return hw


def circle_mask(r):
    hw = circle_spans(r)
    d = np.arange(-r, r + 1)
    return np.abs(d)[None, :] <= hw[np.abs(d)][:, None]


def round_px(x):
    """cvRound of a float32 -> int (round half to even)."""
    return int(np.rint(F32(x)))


def set_mask(pts, ids, cnt, r, w, h):
    """FeatureTracker::setMask (:55-84) with the stable order.  -> kept indices (in output order), mask (bool, True = free)."""
    order = np.argsort(-np.asarray(cnt, np.int64), kind="stable")
    mask = np.ones((h, w), bool)
    cm = circle_mask(r)
    keep = []
    for i in order:
        px, py = round_px(pts[i][0]), round_px(pts[i][1])
        if not mask[py, px]:
            continue
        keep.append(int(i))
        y0, y1, x0, x1 = max(py - r, 0), min(py + r, h - 1), max(px - r, 0), min(px + r, w - 1)
        mask[y0:y1 + 1, x0:x1 + 1] &= ~cm[y0 - py + r:y1 - py + r + 1, x0 - px + r:x1 - px + r + 1]
    return keep, mask


def detect_candidates(resp, mask):
    """-> (threshold fp32, candidate pixel indices sorted strongest first, ties lower pixel index first)."""
    h, w = resp.shape
    m = resp[mask]
    maxv = F32(max(float(m.max()), 0.0)) if m.size else F32(0)
    thr = F32(np.float64(maxv) * 0.01)
    c = resp[1:-1, 1:-1]
    nb = np.full(c.shape, -np.inf, np.float32)
    for i in range(3):
        for j in range(3):
            nb = np.maximum(nb, resp[i:i + h - 2, j:j + w - 2])
    ok = (c > thr) & (c == nb) & mask[1:-1, 1:-1]
    ys, xs = np.nonzero(ok)
    pix = (ys + 1) * w + (xs + 1)
    vals = resp.reshape(-1)[pix]
    order = np.lexsort((pix, -vals.astype(np.float64)))
    return thr, pix[order]


def detect(resp, mask, quota, min_dist):
    """cv::goodFeaturesToTrack selection -> [(x, y)] in selection order."""
    h, w = resp.shape
    _, pix = detect_candidates(resp, mask)
    out = []
    if quota <= 0:
        return out
    sel = np.zeros((0, 2), np.int64)
    r2 = min_dist * min_dist
    for p in pix:
        x, y = int(p % w), int(p // w)
        if len(sel) and ((sel[:, 0] - x) ** 2 + (sel[:, 1] - y) ** 2 < r2).any():
            continue
        sel = np.vstack([sel, [[x, y]]])
        out.append((x, y))
        if len(out) >= quota:
            break
    return out


def _weights(a, b):
    one, s = F32(1), F32(16384)
    iw00 = int(np.rint((one - a) * (one - b) * s))
    iw01 = int(np.rint(a * (one - b) * s))
    iw10 = int(np.rint((one - a) * b * s))
    return iw00, iw01, iw10, 16384 - iw00 - iw01 - iw10


def _bilin(p22, w, shift):
    v = p22[:-1, :-1] * w[0] + p22[:-1, 1:] * w[1] + p22[1:, :-1] * w[2] + p22[1:, 1:] * w[3]
    return (v + (1 << (shift - 1))) >> shift


def _img_patch(img, ix, iy):
    h, w = img.shape
    ys = reflect101(iy + np.arange(WIN + 1), h); xs = reflect101(ix + np.arange(WIN + 1), w)
    return img[np.ix_(ys, xs)].astype(np.int64)


def _der_patch(d, ix, iy):
    h, w = d.shape
    ys = iy + np.arange(WIN + 1); xs = ix + np.arange(WIN + 1)
    ok = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
    v = d[np.ix_(np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1))].astype(np.int64)
    return np.where(ok, v, 0)


def _origin(p, w, h):
    """floor of the window origin and whether it lies in [-21, cols) x [-21, rows), decided on the fp32 floor."""
    fx, fy = np.floor(p[0]), np.floor(p[1])
    ok = bool(fx >= -WIN and fx < w and fy >= -WIN and fy < h)
    return (int(fx), int(fy), fx, fy) if ok else None


def lk_level(lev_i, lev_j, prev_pt, next_pt, level0):
    """One pyramid level of cv::calcOpticalFlowPyrLK for one point.  prev_pt, next_pt: fp32 pairs at this level's scale.
    -> (next_pt, failed) where failed only matters at level 0."""
    img_i, dx_i, dy_i = lev_i
    img_j = lev_j[0]
    h, w = img_i.shape
    half = F32(HALF)
    pp = (F32(prev_pt[0]) - half, F32(prev_pt[1]) - half)
    o = _origin(pp, w, h)
    if o is None:
        return next_pt, True
    ix, iy, fx, fy = o
    wt = _weights(F32(pp[0] - F32(fx)), F32(pp[1] - F32(fy)))
    I = _bilin(_img_patch(img_i, ix, iy), wt, 9)
    Ix = _bilin(_der_patch(dx_i, ix, iy), wt, 14)
    Iy = _bilin(_der_patch(dy_i, ix, iy), wt, 14)
    sc = 1.0 / (1 << 20)
    A11 = float(int((Ix * Ix).sum())) * sc
    A12 = float(int((Ix * Iy).sum())) * sc
    A22 = float(int((Iy * Iy).sum())) * sc
    D = A11 * A22 - A12 * A12
    t = A11 - A22
    min_eig = ((A22 + A11) - np.sqrt(t * t + 4.0 * (A12 * A12))) / (2.0 * WIN * WIN)
    if min_eig < 1e-4 or D < float(np.finfo(np.float32).eps):
        return next_pt, True
    out = (F32(next_pt[0]), F32(next_pt[1]))
    npt = (out[0] - half, out[1] - half)
    prev_d = (F32(0), F32(0))
    failed = False
    for j in range(MAX_ITERS):
        o = _origin(npt, w, h)
        if o is None:
            failed = True
            break
        jx, jy, fx, fy = o
        wt = _weights(F32(npt[0] - F32(fx)), F32(npt[1] - F32(fy)))
        diff = _bilin(_img_patch(img_j, jx, jy), wt, 9) - I
        b1 = float(int((diff * Ix).sum())) * sc
        b2 = float(int((diff * Iy).sum())) * sc
        d = (F32((A12 * b2 - A22 * b1) / D), F32((A12 * b1 - A11 * b2) / D))
        npt = (F32(npt[0] + d[0]), F32(npt[1] + d[1]))
        out = (F32(npt[0] + half), F32(npt[1] + half))
        if float(d[0]) * float(d[0]) + float(d[1]) * float(d[1]) <= 1e-4:
            break
        if j > 0 and float(np.abs(F32(d[0] + prev_d[0]))) < 0.01 and float(np.abs(F32(d[1] + prev_d[1]))) < 0.01:
            out = (F32(out[0] - F32(d[0] * F32(0.5))), F32(out[1] - F32(d[1] * F32(0.5))))
            break
        prev_d = d
    return out, failed


def lk_track(pyr_i, pyr_j, prev_pts, max_level, init=None):
    """cv::calcOpticalFlowPyrLK(I, J, prev_pts, ..., Size(21, 21), max_level) [+ OPTFLOW_USE_INITIAL_FLOW when init is given].
    -> (next_pts [n, 2] fp32, status [n] uint8)."""
    prev_pts = np.asarray(prev_pts, np.float32).reshape(-1, 2)
    n = len(prev_pts)
    out = np.zeros((n, 2), np.float32); status = np.ones(n, np.uint8)
    top = min(max_level, len(pyr_i) - 1)
    for k in range(n):
        nxt = None
        for level in range(top, -1, -1):
            s = F32(1.0 / (1 << level))
            pp = (prev_pts[k, 0] * s, prev_pts[k, 1] * s)
            if level == top:
                nxt = (F32(init[k][0]) * s, F32(init[k][1]) * s) if init is not None else pp
            else:
                nxt = (nxt[0] * F32(2), nxt[1] * F32(2))
            nxt, failed = lk_level(pyr_i[level], pyr_j[level], pp, nxt, level == 0)
            if level == 0 and failed:
                status[k] = 0
        out[k] = nxt
    return out, status


class Camera:
    """camodocal PinholeCamera (PinholeCamera.cc:278-295, 450-510)."""

    def __init__(self, width, height, fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0):
        self.width, self.height = int(width), int(height)
        self.fx, self.fy, self.cx, self.cy, self.k1, self.k2, self.p1, self.p2 = (float(v) for v in (fx, fy, cx, cy, k1, k2, p1, p2))
        self.ik11 = 1.0 / self.fx; self.ik13 = -self.cx / self.fx; self.ik22 = 1.0 / self.fy; self.ik23 = -self.cy / self.fy
        self.distort = not (self.k1 == 0.0 and self.k2 == 0.0 and self.p1 == 0.0 and self.p2 == 0.0)

    def _distortion(self, ux, uy):
        mx2, my2, mxy = ux * ux, uy * uy, ux * uy
        rho2 = mx2 + my2
        rad = self.k1 * rho2 + self.k2 * rho2 * rho2
        return (ux * rad + 2.0 * self.p1 * mxy + self.p2 * (rho2 + 2.0 * mx2),
                uy * rad + 2.0 * self.p2 * mxy + self.p1 * (rho2 + 2.0 * my2))

    def lift(self, u, v):
        mx_d = self.ik11 * float(u) + self.ik13; my_d = self.ik22 * float(v) + self.ik23
        mx_u, my_u = mx_d, my_d
        if self.distort:
            for _ in range(8):
                dx, dy = self._distortion(mx_u, my_u)
                mx_u, my_u = mx_d - dx, my_d - dy
        return F32(mx_u), F32(my_u)


class TrackerRef:
    """One stream of FeatureTracker::trackImage."""

    def __init__(self, cam, max_cnt=150, min_dist=30):
        self.cam, self.max_cnt, self.min_dist = cam, int(max_cnt), int(min_dist)
        self.reset()

    def reset(self):
        self.prev_pyr = None
        self.cur_pyr = None
        self.pts = np.zeros((0, 2), np.float32)
        self.ids = np.zeros(0, np.int32); self.cnt = np.zeros(0, np.int32)
        self.un = np.zeros((0, 2), np.float32)        # undistorted points of the previous frame, per point
        self.n_id = 0
        self.prev_time = 0.0
        self.last_resp = None
        self.last_status = None

    def track(self, time, image):
        image = np.asarray(image, np.uint8)
        grey = bgr_to_grey(image) if image.ndim == 3 else image
        h, w = grey.shape
        assert (w, h) == (self.cam.width, self.cam.height)
        self.cur_pyr = build_pyramid(grey)
        pts, ids, cnt, pun = self.pts, self.ids, self.cnt, self.un
        has_prev = np.ones(len(pts), bool)
        if len(pts):
            cur, st = lk_track(self.prev_pyr, self.cur_pyr, pts, MAX_LEVEL)
            rev = pts.copy(); rst = np.zeros(len(pts), np.uint8)
            live = np.nonzero(st)[0]                   # the backward pass of a point that failed forward cannot change its fate
            if len(live):
                rev[live], rst[live] = lk_track(self.cur_pyr, self.prev_pyr, cur[live], 1, init=pts[live])
            keep = np.zeros(len(pts), bool)
            for i in range(len(pts)):
                if not (st[i] and rst[i]):
                    continue
                dx = float(F32(pts[i, 0] - rev[i, 0])); dy = float(F32(pts[i, 1] - rev[i, 1]))
                if not np.sqrt(dx * dx + dy * dy) <= 0.5:
                    continue
                rx, ry = np.rint(cur[i, 0]), np.rint(cur[i, 1])
                keep[i] = bool(1 <= rx and rx < w - 1 and 1 <= ry and ry < h - 1)
            self.last_status = keep.copy()
            pts, ids, cnt, pun = cur[keep], ids[keep], cnt[keep], pun[keep]
            has_prev = has_prev[keep]
        cnt = cnt + 1
        order, mask = set_mask(pts, ids, cnt, self.min_dist, w, h)
        pts, ids, cnt, pun, has_prev = pts[order], ids[order], cnt[order], pun[order], has_prev[order]
        quota = self.max_cnt - len(pts)
        if quota > 0:
            self.last_resp = response(grey)
            new = detect(self.last_resp, mask, quota, self.min_dist)
            if new:
                k = len(new)
                pts = np.vstack([pts, np.array(new, np.float32).reshape(-1, 2)])
                ids = np.concatenate([ids, np.arange(self.n_id, self.n_id + k, dtype=np.int32)]); self.n_id += k
                cnt = np.concatenate([cnt, np.ones(k, np.int32)])
                pun = np.vstack([pun, np.zeros((k, 2), np.float32)])
                has_prev = np.concatenate([has_prev, np.zeros(k, bool)])
        n = len(pts)
        rec = np.zeros(n, RECORD)
        un = np.zeros((n, 2), np.float32)
        dt = float(time) - self.prev_time
        for i in range(n):
            un[i] = self.cam.lift(pts[i, 0], pts[i, 1])
            if has_prev[i]:
                with np.errstate(divide="ignore", invalid="ignore"):
                    rec["vx"][i] = F32(np.float64(F32(un[i, 0] - pun[i, 0])) / np.float64(dt))
                    rec["vy"][i] = F32(np.float64(F32(un[i, 1] - pun[i, 1])) / np.float64(dt))
        rec["id"] = ids; rec["track_cnt"] = cnt
        rec["x_n"] = un[:, 0]; rec["y_n"] = un[:, 1]; rec["u"] = pts[:, 0]; rec["v"] = pts[:, 1]
        self.pts, self.ids, self.cnt, self.un = pts.astype(np.float32), ids.astype(np.int32), cnt.astype(np.int32), un
        self.prev_pyr = self.cur_pyr
        self.prev_time = float(time)
        return rec
