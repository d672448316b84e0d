"""scripts/keyframe_bench.py -- throughput of the device keyframe descriptors (lmono_keyframes_*): keyframes/s of
lmono_keyframes_add_batch for 1, 8, 64 streams at 1241 x 376 with 150 window points, images resident on the device; matches/s of
lmono_keyframes_match for one current keyframe against 4 and against 1024 stored keyframes; per-kernel times of one 64-stream add and
of one 1024-keyframe match from the torch profiler's device events; verifies/s of lmono_keyframes_verify (match, PnP RANSAC,
gates) for the same current keyframe against 4 and 1024 candidates, with the device time of k_pnp_ransac; with --vocabulary FILE (a BRIEF
vocabulary in the reference's binary layout, e.g. one of train_brief_vocabulary) also BoW builds/s and queries/s of one store
at 64 / 1024 / 4096 stored keyframes and of 64 stores per call (detect_loop_batch).  Prints one JSON line.  One process; run it under `timeout`;
exits non-zero on any HIP error.

  timeout 300 python scripts/keyframe_bench.py [--pattern tests/golden/brief_pattern.yml] [--streams 1,8,64] [--old 4,1024]
                                               [--calls 12] [--warmup 3] [--no-kernels] [--vocabulary FILE] [--stored 64,1024,4096]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _kernel_times(prof):
    kern = {}
    for e in prof.key_averages():
        tag = next((t for t in ("k_kf_", "k_pnp_", "k_bow_") if t in e.key), None)
        if tag:
            name = e.key[e.key.index(tag):].split("(")[0]
            name = name.split("E")[0] if e.key.startswith("_Z") else name
            us = getattr(e, "device_time_total", None)
            if us is None:
                us = getattr(e, "cuda_time_total", 0.0)
            kern[name] = kern.get(name, 0.0) + float(us)
    return kern


def _timed(fn, calls, warmup):
    ms = []
    for f in range(calls + warmup):
        t0 = time.perf_counter()
        fn()                                                                             # every entry point synchronises before it returns
        if f >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return np.array(ms)


def _bow(a, ctx, cam, pat, seeds, lmono_amd, torch):
    """BoW builds/s (every vector of the store, after the watermark is reset) and queries/s (the last keyframe against all before it)."""
    voc = lmono_amd.BriefVocabulary(ctx, lmono_amd.load_brief_vocabulary(a.vocabulary))
    runs = []

    def fill(store, n):
        for o in range(n):
            g = seeds[o % 4]
            store.load(g["keypoints"], g["norm"], g["descriptors"])

    def build(store, n):
        store.set_vocabulary(voc)                                                        # resets the watermark
        store.bow(n - 1)

    for n in [int(x) for x in a.stored.split(",")]:
        store = lmono_amd.KeyFrames(ctx, cam, pat, n, a.max_keypoints)
        fill(store, n)
        b = _timed(lambda: build(store, n), a.calls, a.warmup)
        q = _timed(lambda: store.query(n - 1, 4, -1), a.calls, a.warmup)
        d = _timed(lambda: store.detect_loop(n - 1, 100), a.calls, a.warmup)
        run = {"stored": n, "build_ms_median": float(np.median(b)), "bow_builds_per_s": float(n * 1e3 / np.median(b)), "query_ms_median": float(np.median(q)),
               "query_ms_min": float(q.min()), "queries_per_s": float(1e3 / np.median(q)), "detect_loop_ms_median": float(np.median(d)),
               "words_mean": float(np.mean([len(store.bow(i)[0]) for i in range(4)]))}
        if n == max(int(x) for x in a.stored.split(",")) and not a.no_kernels:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                build(store, n)
                store.query(n - 1, 4, -1)
                torch.cuda.synchronize()
            run["kernels_us"] = _kernel_times(prof)
        runs.append(run)
        store.close()
    stores = [lmono_amd.KeyFrames(ctx, cam, pat, 64, a.max_keypoints) for _ in range(64)]
    for s in stores:
        s.set_vocabulary(voc)
        fill(s, 64)
    curs = [63] * 64
    lmono_amd.KeyFrames.detect_loop_batch(stores, curs, 20)                              # builds the vectors
    q = _timed(lambda: lmono_amd.KeyFrames.detect_loop_batch(stores, curs, 20), a.calls, a.warmup)
    batch = {"streams": 64, "stored": 64, "ms_per_call_median": float(np.median(q)), "queries_per_s": float(64 * 1e3 / np.median(q))}
    for s in stores:
        s.close()
    voc.close()
    return {"vocabulary": {"file": os.path.basename(a.vocabulary)}, "one_store": runs, "batch": batch}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pattern", default=os.path.join(ROOT, "tests", "golden", "brief_pattern.yml"))
    ap.add_argument("--streams", default="1,8,64")
    ap.add_argument("--old", default="4,1024")
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1241)
    ap.add_argument("--height", type=int, default=376)
    ap.add_argument("--window", type=int, default=150)
    ap.add_argument("--max-keypoints", type=int, default=8192)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--vocabulary", default=None, help="BRIEF vocabulary file: also measure BoW builds/s and queries/s")
    ap.add_argument("--stored", default="64,1024,4096")
    a = ap.parse_args()
    import torch
    import lmono_amd
    from workloads import s5
    w, h = a.width, a.height
    pat = lmono_amd.load_brief_pattern(a.pattern)
    n_img = a.calls + a.warmup
    variants = [s5.Sequence(w, h, 2, seed=20 + v, step=(2.0 + 0.5 * v, 0.5 * v - 0.5), margin=64).frames for v in range(4)]
    dev = [[torch.from_numpy(f).to("cuda:0") for f in seq] for seq in variants]       # 4 x 2 images shared by all streams (device resident)
    torch.cuda.synchronize()
    rng = np.random.default_rng(1)
    uv = np.stack([rng.uniform(20, w - 20, a.window), rng.uniform(20, h - 20, a.window)], 1).astype(np.float32)
    ctx = lmono_amd.Context(0)
    cam = lmono_amd.Camera(w, h, 718.856, 718.856, 607.1928, 185.2157, 0.0, 0.0, 0.0, 0.0, 5, 0, 0)
    out = {"bench": "keyframe", "width": w, "height": h, "window": a.window, "max_keypoints": a.max_keypoints, "calls": a.calls, "warmup": a.warmup,
           "add": [], "match": [], "verify": []}
    for n in [int(x) for x in a.streams.split(",")]:
        stores = [lmono_amd.KeyFrames(ctx, cam, pat, 2, a.max_keypoints) for _ in range(n)]
        ms, nkp = [], None
        for f in range(n_img):
            for s in stores:
                s.clear()
            ptrs = [dev[s % 4][f % 2].data_ptr() for s in range(n)]
            t0 = time.perf_counter()
            _, nkp = lmono_amd.KeyFrames.add_batch(stores, ptrs, [uv] * n)               # synchronises before it returns
            dt = (time.perf_counter() - t0) * 1e3
            if f >= a.warmup:
                ms.append(dt)
        ms = np.array(ms)
        run = {"streams": n, "ms_per_call_median": float(np.median(ms)), "ms_per_call_min": float(ms.min()), "ms_per_call_max": float(ms.max()),
               "keyframes_per_s": float(n * 1e3 / np.median(ms)), "keypoints_mean": float(np.mean(nkp))}
        if n == 64 and not a.no_kernels:
            from torch.profiler import ProfilerActivity, profile
            for s in stores:
                s.clear()
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                lmono_amd.KeyFrames.add_batch(stores, [dev[s % 4][0].data_ptr() for s in range(n)], [uv] * n)
                torch.cuda.synchronize()
            run["kernels_us"] = _kernel_times(prof)
        out["add"].append(run)
        for s in stores:
            s.close()
    # one current keyframe against stored keyframes: the store is filled by lmono_keyframes_load with copies of four real keyframes
    olds = [int(x) for x in a.old.split(",")]
    store = lmono_amd.KeyFrames(ctx, cam, pat, max(olds) + 1, a.max_keypoints)
    seeds = []
    for v in range(4):
        store.add(variants[v][0], uv)
        seeds.append(store.get(v))
    store.clear()
    for o in range(max(olds)):
        g = seeds[o % 4]
        store.load(g["keypoints"], g["norm"], g["descriptors"])
    cur, _ = store.add(variants[0][1], uv)
    for n_old in olds:
        idx = list(range(n_old))
        ms, counts = [], None
        for f in range(n_img):
            t0 = time.perf_counter()
            counts = store.match(cur, idx)["counts"]
            dt = (time.perf_counter() - t0) * 1e3
            if f >= a.warmup:
                ms.append(dt)
        ms = np.array(ms)
        pairs = float(a.window) * float(sum(len(seeds[o % 4]["keypoints"]) for o in range(n_old)))
        run = {"old_keyframes": n_old, "ms_per_call_median": float(np.median(ms)), "ms_per_call_min": float(ms.min()),
               "matches_per_s": float(n_old * 1e3 / np.median(ms)), "descriptor_pairs_per_s": float(pairs * 1e3 / np.median(ms)),
               "matched_mean": float(np.mean(counts))}
        if n_old == max(olds) and not a.no_kernels:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                store.match(cur, idx)
                torch.cuda.synchronize()
            run["kernels_us"] = _kernel_times(prof)
        out["match"].append(run)
    # the same keyframe verified against the same candidates: the window points back-projected to a plane at 10 m, the body at the origin.
    # Every candidate above the MIN_BRIEF_LOOP_NUM gate runs the full, fixed hypothesis count, so the time does not depend on the geometry
    K = np.array([[cam.fx, cam.cx], [cam.fy, cam.cy]])
    p3 = np.stack([(uv[:, 0] - K[0, 1]) / K[0, 0] * 10.0, (uv[:, 1] - K[1, 1]) / K[1, 0] * 10.0, np.full(len(uv), 10.0)], 1).astype(np.float32)
    ident = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    for n_old in olds:
        idx = list(range(n_old))
        ms, v = [], None
        for f in range(n_img):
            t0 = time.perf_counter()
            v = store.verify(cur, idx, p3, ident, ident)                                 # synchronises before it returns
            dt = (time.perf_counter() - t0) * 1e3
            if f >= a.warmup:
                ms.append(dt)
        ms = np.array(ms)
        run = {"old_keyframes": n_old, "ms_per_call_median": float(np.median(ms)), "ms_per_call_min": float(ms.min()),
               "verifies_per_s": float(n_old * 1e3 / np.median(ms)), "pnp_ran": int((v["stats"][:, 0] >= 0).sum()), "loops": int(v["has_loop"].sum())}
        if not a.no_kernels:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                store.verify(cur, idx, p3, ident, ident)
                torch.cuda.synchronize()
            run["kernels_us"] = _kernel_times(prof)
        out["verify"].append(run)
    store.close()
    if a.vocabulary:
        out["bow"] = _bow(a, ctx, cam, pat, seeds, lmono_amd, torch)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
