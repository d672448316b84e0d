"""workloads/s6.py -- synthetic image sequences with independently moving objects "S6": a far textured layer and several near
textured cards seen by a camera that translates in the image plane, so static content at depth Z moves along one image
direction by focal * t / Z pixels per frame and every epipolar line is parallel to that direction.  A few *mover* cards get an
extra per-frame shift perpendicular to it: a KLT tracker follows them consistently (the forward-backward test passes), and
only an epipolar gate can tell them from the static scene.  class_of() gives the ground truth per pixel.  numpy only.
Input plumbing for tests, examples and scripts; neither the hot path nor a checker."""
import numpy as np

from workloads import s5

STATIC, MOVER, BOUNDARY = 0, 1, 2
BOUNDARY_PX = 12.0


def _bilinear(canvas, x, y):
    x0 = np.floor(x).astype(np.int64); y0 = np.floor(y).astype(np.int64)
    a = x - x0; b = y - y0
    x0 = np.clip(x0, 0, canvas.shape[1] - 2); y0 = np.clip(y0, 0, canvas.shape[0] - 2)
    return ((1 - a) * (1 - b) * canvas[y0, x0] + a * (1 - b) * canvas[y0, x0 + 1] + (1 - a) * b * canvas[y0 + 1, x0] + a * b * canvas[y0 + 1, x0 + 1])


class Sequence:
    """frames[k]: uint8 [height, width].  Layer 0 is the far layer; cards[i] = dict(rect=(x0, y0, x1, y1) at frame 0, depth,
    mover): a card moves by shift(i, k) = k * (flow_far * depth_far / depth) * direction (+ k * mover_step * perpendicular)."""

    def __init__(self, width=640, height=480, n_frames=20, seed=0, direction=(1.0, 0.0), flow_far=3.0, depth_far=20.0,
                 cards=None, mover_step=3.0, margin=200):
        self.width, self.height, self.n_frames = int(width), int(height), int(n_frames)
        d = np.asarray(direction, np.float64)
        self.direction = d / np.sqrt((d * d).sum())
        self.perp = np.array([-self.direction[1], self.direction[0]])
        self.flow_far, self.depth_far, self.mover_step, self.margin = float(flow_far), float(depth_far), float(mover_step), int(margin)
        if cards is None:
            w, h = self.width, self.height
            # Flows that lie near one line in (dx, dy) fit an affine F whatever made them, and a flow below the gate's threshold fits
            # any epipole.  So the static flows span 3 .. 8.6 px per frame along the direction, on both sides of the movers' 5 and
            # 6 px, and the movers sit 3 px off that line.  Card sizes keep the boundary class below 30 % of the tracked points
            cards = [dict(rect=(0.10 * w, 0.10 * h, 0.26 * w, 0.32 * h), depth=10.0, mover=True),
                     dict(rect=(0.55 * w, 0.45 * h, 0.71 * w, 0.67 * h), depth=12.0, mover=True),
                     dict(rect=(0.05 * w, 0.55 * h, 0.25 * w, 0.83 * h), depth=7.0, mover=False)]
        self.cards = sorted(cards, key=lambda c: -c["depth"])            # far to near: later cards cover earlier ones
        cw, ch = self.width + 2 * self.margin, self.height + 2 * self.margin
        self.canvases = [s5.make_canvas(cw, ch, seed * 16 + i) for i in range(len(self.cards) + 1)]
        self.frames = [self._render(k) for k in range(self.n_frames)]

    def shift(self, layer, k):
        """Displacement (x, y) in pixels of layer `layer` (0: far, i + 1: cards[i]) between frame 0 and frame k."""
        if layer == 0:
            return k * self.flow_far * self.direction
        c = self.cards[layer - 1]
        s = k * (self.flow_far * self.depth_far / c["depth"]) * self.direction
        return s + (k * self.mover_step * self.perp if c["mover"] else 0.0)

    def _rect(self, i, k):
        x0, y0, x1, y1 = self.cards[i]["rect"]
        s = self.shift(i + 1, k)
        return x0 + s[0], y0 + s[1], x1 + s[0], y1 + s[1]

    def layer_of(self, k, xy):
        """Visible layer (0: far, i + 1: cards[i]) at frame-k pixels xy [n, 2]."""
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        layer = np.zeros(len(xy), np.int64)
        for i in range(len(self.cards)):
            x0, y0, x1, y1 = self._rect(i, k)
            inside = (xy[:, 0] >= x0) & (xy[:, 0] < x1) & (xy[:, 1] >= y0) & (xy[:, 1] < y1)
            layer[inside] = i + 1
        return layer

    def class_of(self, k, xy):
        """STATIC, MOVER (interior of a mover card) or BOUNDARY (within BOUNDARY_PX of an edge of any card) per frame-k pixel."""
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        layer = self.layer_of(k, xy)
        mover = np.array([False] + [c["mover"] for c in self.cards])[layer]
        cls = np.where(mover, MOVER, STATIC)
        for i in range(len(self.cards)):
            x0, y0, x1, y1 = self._rect(i, k)
            dx = np.maximum(np.maximum(x0 - xy[:, 0], xy[:, 0] - x1), 0.0); dy = np.maximum(np.maximum(y0 - xy[:, 1], xy[:, 1] - y1), 0.0)
            outside = np.sqrt(dx * dx + dy * dy)                                   # distance to the rectangle from outside
            inside = np.minimum(np.minimum(xy[:, 0] - x0, x1 - xy[:, 0]), np.minimum(xy[:, 1] - y0, y1 - xy[:, 1]))
            dist = np.where(inside >= 0.0, inside, outside)
            cls = np.where(dist <= BOUNDARY_PX, BOUNDARY, cls)
        return cls

    def flow(self, frame_a, frame_b, xy):
        """Where the scene point visible at xy in frame_a appears in frame_b (ignores occlusion in frame_b)."""
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        layer = self.layer_of(frame_a, xy)
        out = xy.copy()
        for l in range(len(self.cards) + 1):
            out[layer == l] += self.shift(l, frame_b) - self.shift(l, frame_a)
        return out

    def _render(self, k):
        ys, xs = np.mgrid[0:self.height, 0:self.width]
        xy = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)
        layer = self.layer_of(k, xy)
        img = np.zeros(len(xy))
        for l in range(len(self.cards) + 1):
            sel = layer == l
            s = self.shift(l, k)
            img[sel] = _bilinear(self.canvases[l], xy[sel, 0] - s[0] + self.margin, xy[sel, 1] - s[1] + self.margin)
        return np.clip(np.rint(img), 0, 255).astype(np.uint8).reshape(self.height, self.width)
