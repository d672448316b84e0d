"""examples/track_sequence.py -- images -> feature tracks on the GPU (lmono_amd.FeatureTracker), optionally on into the Estimator.

  python examples/track_sequence.py --synthetic 20 --out tracks/                 # workloads/s5 frames with known flow
  python examples/track_sequence.py --sequence /data/kitti/05 --out tracks/      # <sequence>/image_0/%06d.png (+ times.txt)
  ... --reject-f 1.0 0.5                                                         # use_rejectF: 1 with F_THRESHOLD, F_DIS of the config
  ... --estimator                                                                # every frame's tracks go into Estimator::processImage

Per frame one text file <out>/%06d.txt: "id x_n y_n u v vx vy track_cnt" per feature (FeatureTracker.cc:372-397).  With
--estimator the frames are written as a stream for lmono_amd/host/estimator_seq (the host mirror's processImage loop) together
with the sequence's LiDAR poses: the synthetic camera path, or the KITTI directory's pose file (--poses, 3 x 4 row-major per line)."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(n, width=320, height=240, focal=300.0, depth=10.0):
    """-> frames, times, camera (Camera args), poses [n, 16]: an s5 plane at `depth` metres seen by a fronto-parallel camera."""
    from workloads import s5
    seq = s5.Sequence(width, height, n, seed=1, step=(1.5, 0.5), rot_step=0.002, zoom_step=0.001)
    poses = np.zeros((n, 16))
    for k, (tx, ty, ang, zoom) in enumerate(seq.motion):
        T = np.eye(4)
        c, s = np.cos(ang), np.sin(ang)
        T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
        T[:3, 3] = [tx * depth / focal, ty * depth / focal, depth - depth / zoom]
        poses[k] = T.reshape(16)
    cam = (width, height, focal, focal, 0.5 * (width - 1), 0.5 * (height - 1), 0.0, 0.0, 0.0, 0.0)
    return seq.frames, [0.1 * k for k in range(n)], cam, poses


def kitti(root, first, count, poses_file):
    from PIL import Image
    d = os.path.join(root, "image_0")
    names = sorted(f for f in os.listdir(d) if f.endswith(".png"))[first:]
    if count is not None:
        names = names[:count]
    frames = [np.asarray(Image.open(os.path.join(d, f)).convert("L"), np.uint8) for f in names]
    tf = os.path.join(root, "times.txt")
    times = [float(x) for x in open(tf).read().split()][first:first + len(frames)] if os.path.exists(tf) else [0.1 * k for k in range(len(frames))]
    h, w = frames[0].shape
    cam = (w, h, 718.856, 718.856, 607.1928, 185.2157, 0.0, 0.0, 0.0, 0.0)          # KITTI odometry P0 (sequences 00-02; --camera overrides)
    poses = np.tile(np.eye(4).reshape(16), (len(frames), 1))
    if poses_file:
        P = np.loadtxt(poses_file).reshape(-1, 12)[first:first + len(frames)]
        poses[:, :12] = P
    return frames, times, cam, poses


def write_stream(path, times, poses, records):
    """The binary layout lmono_amd/host/estimator_seq reads (doubles): n, TLC[16], per frame header, L0_Pos[16], 0, n_f, (id x y u v)*."""
    out = [float(len(times))] + list(np.eye(4).reshape(16))
    for t, L0, rec in zip(times, poses, records):
        out += [float(t)] + list(L0) + [0.0, float(len(rec))]
        for r in rec:
            out += [float(r["id"]), float(r["x_n"]), float(r["y_n"]), float(r["u"]), float(r["v"])]
    np.asarray(out, np.float64).tofile(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequence", help="directory with image_0/%%06d.png and times.txt")
    ap.add_argument("--synthetic", type=int, default=0, help="generate this many s5 frames instead of reading a sequence")
    ap.add_argument("--out", required=True)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--count", type=int, default=None)
    ap.add_argument("--poses", help="pose file of the sequence (KITTI layout), for --estimator")
    ap.add_argument("--camera", help="fx,fy,cx,cy[,k1,k2,p1,p2] of the PINHOLE cam yaml")
    ap.add_argument("--max-cnt", type=int, default=150)
    ap.add_argument("--min-dist", type=int, default=30)
    ap.add_argument("--reject-f", type=float, nargs=2, metavar=("THR", "DIS"), help="rejectWithF with F_THRESHOLD, F_DIS (use_rejectF: 1)")
    ap.add_argument("--estimator", action="store_true", help="feed every frame into Estimator::processImage (lmono_amd/host/estimator_seq)")
    a = ap.parse_args()
    if not a.synthetic and not a.sequence:
        ap.error("--synthetic N or --sequence DIR")
    import lmono_amd
    frames, times, cam, poses = synthetic(a.synthetic) if a.synthetic else kitti(a.sequence, a.first, a.count, a.poses)
    if a.camera:
        v = [float(x) for x in a.camera.split(",")]
        cam = cam[:2] + tuple(v) + cam[2 + len(v):]
    os.makedirs(a.out, exist_ok=True)
    ctx = lmono_amd.Context(0)
    tracker = lmono_amd.FeatureTracker(ctx, lmono_amd.Camera(*cam, 5, 0, 0), a.max_cnt, min(a.min_dist, 15) if a.synthetic else a.min_dist)
    if a.reject_f:
        tracker.set_reject_f(a.reject_f[0], a.reject_f[1])
    records = []
    for k, (t, img) in enumerate(zip(times, frames)):
        rec = tracker.track(t, img)
        if a.reject_f:
            st, _ = tracker.reject_stats()
            if st[0] >= 0:
                print("frame %d: rejectWithF: %d valid hypotheses, best %d, %d gate-1 inliers, %d kept after gate 2" % (k, st[0], st[1], st[2], st[3]))
        records.append(rec)
        with open(os.path.join(a.out, "%06d.txt" % k), "w") as f:
            for r in rec:
                f.write("%d %.9g %.9g %.9g %.9g %.9g %.9g %d\n" % (r["id"], r["x_n"], r["y_n"], r["u"], r["v"], r["vx"], r["vy"], r["track_cnt"]))
        print("frame %d: %d features, %d tracked from the previous frame, longest track %d" % (k, len(rec), int((rec["track_cnt"] > 1).sum()), int(rec["track_cnt"].max()) if len(rec) else 0))
    tracker.close()
    if a.estimator:
        exe = os.path.join(ROOT, "lmono_amd", "host", "estimator_seq")
        if not os.path.exists(exe):
            raise SystemExit("lmono_amd/host/estimator_seq is missing: run build() first")
        stream = os.path.join(a.out, "stream.bin")
        write_stream(stream, times, poses, records)
        del ctx
        res = subprocess.run([exe, stream, os.path.join(a.out, "new_odometry.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if res.returncode != 0:
            raise SystemExit("estimator_seq failed (%d): %s" % (res.returncode, res.stderr[-2000:]))
        frm = [l.split() for l in res.stdout.splitlines() if l.startswith("FRM ")]
        for l in frm:
            print("estimator frame %s: keyframe %s stage %s tracks %s" % (l[1], l[2], l[3], l[-1]))
        if len(frm) != len(frames):
            raise SystemExit("the estimator accepted %d of %d frames" % (len(frm), len(frames)))
        print("estimator ok: %d frames accepted" % len(frm))


if __name__ == "__main__":
    main()
