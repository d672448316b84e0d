"""workloads/s5.py -- synthetic image sequences with known flow "S5": one textured plane (band-limited random texture plus
random rectangles, which give corner-like structure) on a canvas larger than the frame; every frame is cut out of the canvas
under a known similarity (translation, rotation, zoom about the frame centre), optionally with an occluder rectangle that
appears mid-sequence, so that forward-backward rejection in a KLT tracker has something to reject.  numpy only.
Input plumbing for tests, examples and scripts; neither the hot path nor a checker."""
import numpy as np


def make_canvas(width, height, seed=0, n_rect=None):
    """-> float64 canvas [height, width] in 0..255."""
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal((height, width))
    fy = np.fft.fftfreq(height)[:, None]; fx = np.fft.fftfreq(width)[None, :]
    f2 = fx * fx + fy * fy
    band = np.exp(-f2 / (2 * 0.06 ** 2)) - 0.7 * np.exp(-f2 / (2 * 0.012 ** 2))      # pass band around 1 / 16 cycles per pixel
    tex = np.real(np.fft.ifft2(np.fft.fft2(noise) * band))
    tex = tex / tex.std()
    img = 128.0 + 30.0 * tex
    if n_rect is None:
        n_rect = width * height // 1500
    for _ in range(n_rect):
        w, h = rng.integers(6, 28, 2)
        x, y = rng.integers(0, width - w), rng.integers(0, height - h)
        img[y:y + h, x:x + w] += rng.uniform(-70, 70)
    # one light smoothing pass so that edges are not aliased under the bilinear cut
    k = np.array([0.25, 0.5, 0.25])
    img = k[0] * np.roll(img, 1, 0) + k[1] * img + k[2] * np.roll(img, -1, 0)
    img = k[0] * np.roll(img, 1, 1) + k[1] * img + k[2] * np.roll(img, -1, 1)
    return np.clip(img, 0.0, 255.0)


def _bilinear(canvas, x, y):
    x0 = np.floor(x).astype(np.int64); y0 = np.floor(y).astype(np.int64)
    a = x - x0; b = y - y0
    x0 = np.clip(x0, 0, canvas.shape[1] - 2); y0 = np.clip(y0, 0, canvas.shape[0] - 2)
    return ((1 - a) * (1 - b) * canvas[y0, x0] + a * (1 - b) * canvas[y0, x0 + 1] + (1 - a) * b * canvas[y0 + 1, x0] + a * b * canvas[y0 + 1, x0 + 1])


class Sequence:
    """frames[k]: uint8 [height, width]; motion[k] = (tx, ty, angle_rad, zoom) of frame k relative to the canvas centre."""

    def __init__(self, width=320, height=240, n_frames=30, seed=0, step=(1.5, 0.5), rot_step=0.0, zoom_step=0.0, margin=96,
                 occluder=None, occluder_from=None, motion=None, occluder_fill=None):
        self.width, self.height, self.n_frames = int(width), int(height), int(n_frames)
        self.margin = int(margin)
        cw, ch = self.width + 2 * self.margin, self.height + 2 * self.margin
        self.canvas = make_canvas(cw, ch, seed)
        if motion is None:
            motion = [(step[0] * k, step[1] * k, rot_step * k, (1.0 + zoom_step) ** k) for k in range(self.n_frames)]
        self.motion = [tuple(float(v) for v in m) for m in motion]
        self.occluder = occluder                    # (x0, y0, x1, y1) in frame pixels, half-open
        self.occluder_fill = occluder_fill          # None: fresh noise every frame; a number: that flat grey level
        self.occluder_from = occluder_from if occluder_from is not None else (self.n_frames // 2 if occluder else None)
        self.frames = [self._render(k) for k in range(self.n_frames)]

    def to_canvas(self, k, xy):
        """frame k pixel coordinates -> canvas coordinates."""
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        tx, ty, ang, zoom = self.motion[k]
        c, s = np.cos(ang), np.sin(ang)
        dx = xy[:, 0] - 0.5 * (self.width - 1); dy = xy[:, 1] - 0.5 * (self.height - 1)
        X = (c * dx - s * dy) / zoom + tx + 0.5 * (self.canvas.shape[1] - 1)
        Y = (s * dx + c * dy) / zoom + ty + 0.5 * (self.canvas.shape[0] - 1)
        return np.stack([X, Y], 1)

    def from_canvas(self, k, XY):
        XY = np.asarray(XY, np.float64).reshape(-1, 2)
        tx, ty, ang, zoom = self.motion[k]
        c, s = np.cos(ang), np.sin(ang)
        X = (XY[:, 0] - tx - 0.5 * (self.canvas.shape[1] - 1)) * zoom; Y = (XY[:, 1] - ty - 0.5 * (self.canvas.shape[0] - 1)) * zoom
        return np.stack([c * X + s * Y + 0.5 * (self.width - 1), -s * X + c * Y + 0.5 * (self.height - 1)], 1)

    def flow(self, frame_a, frame_b, xy):
        """Where the scene point seen at xy in frame_a appears in frame_b (ignores the occluder)."""
        return self.from_canvas(frame_b, self.to_canvas(frame_a, xy))

    def occluded(self, k, xy, pad=0.0):
        """True where xy (frame k pixels) lies under the occluder (grown by pad) in frame k."""
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        if self.occluder is None or k < self.occluder_from:
            return np.zeros(len(xy), bool)
        x0, y0, x1, y1 = self.occluder
        return (xy[:, 0] >= x0 - pad) & (xy[:, 0] < x1 + pad) & (xy[:, 1] >= y0 - pad) & (xy[:, 1] < y1 + pad)

    def _render(self, k):
        ys, xs = np.mgrid[0:self.height, 0:self.width]
        XY = self.to_canvas(k, np.stack([xs.ravel(), ys.ravel()], 1))
        img = _bilinear(self.canvas, XY[:, 0], XY[:, 1]).reshape(self.height, self.width)
        if self.occluder is not None and k >= self.occluder_from:
            x0, y0, x1, y1 = self.occluder
            rng = np.random.default_rng(1000 + k)                     # fresh fine noise every frame: nothing under it can be tracked
            img[y0:y1, x0:x1] = rng.uniform(0, 255, (y1 - y0, x1 - x0)) if self.occluder_fill is None else float(self.occluder_fill)
        return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def bgr_of(grey, seed=0):
    """A BGR8 image with some colour structure whose channels average near the grey image (for the BGR2GRAY path)."""
    rng = np.random.default_rng(seed)
    g = grey.astype(np.int32)
    off = rng.integers(-20, 21, grey.shape)
    return np.stack([np.clip(g + off, 0, 255), np.clip(g - off // 2, 0, 255), np.clip(g + off // 3, 0, 255)], 2).astype(np.uint8)
