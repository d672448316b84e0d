"""scripts/excalib_bench.py -- throughput of the camera-LiDAR rotation calibration (lmono_excalib_step): stream steps per
second for 1, 64 and 256 streams of m = 150 pairs in one call (stages 1-4, one launch, uploads and read-back included); next to it the
same steps through lmono_amd/host/excalib_test (the kernel's arithmetic as plain C++ on one core) and through the numpy restatement
tests/excalib_ref.py.  Prints one JSON line.  One process; run it under `timeout`; exits non-zero on any HIP error.

  timeout 300 python scripts/excalib_bench.py [--streams 1,64,256] [--pairs 150] [--calls 30] [--warmup 5] [--no-gpu]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,64,256")
    ap.add_argument("--pairs", type=int, default=150)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    from tests import excalib_cases as C
    from tests import excalib_ref as X
    frames = C.scene(3, a.pairs, 8, 8.0, 12.0, noise_px=0.5)
    out = {"pairs": a.pairs, "runs": []}
    # the host arithmetic on one core, and the restatement
    exe = os.path.join(ROOT, "lmono_amd", "host", "excalib_test")
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "cases.bin")
        C.write_cases(path, [(10, [(1, P, None, ql) for P, _, ql in frames])])
        txt = subprocess.run([exe, "--time", path, "200"], check=True, capture_output=True, text=True).stdout
        out["host_one_core_steps_per_s"] = float(txt.split(":")[1].split()[0])
    t0 = time.perf_counter()
    ref = X.Calibrator(10)
    for P, _, ql in frames:
        ref.step(P, ql)
    out["numpy_restatement_steps_per_s"] = len(frames) / (time.perf_counter() - t0)
    if not a.no_gpu:
        import lmono_amd
        ctx = lmono_amd.Context(0)
        for n in [int(v) for v in a.streams.split(",")]:
            cal = lmono_amd.ExtrinsicCalibrator(ctx, n, 10)
            ms = []
            st = np.arange(n, dtype=np.int32); m = np.full(n, a.pairs, np.int32)
            R = np.zeros((n, 9)); stats = np.zeros((n, 6), np.int32); rlc = np.zeros((n, 9)); sv = np.zeros((n, 4)); hub = np.zeros(n); ok = np.zeros(n, np.int32)
            packed = [(np.ascontiguousarray(np.tile(P, (n, 1))), np.ascontiguousarray(np.tile(ql, (n, 1)))) for P, _, ql in frames]
            for c in range(a.calls + a.warmup):
                flat, q = packed[c % len(packed)]
                t0 = time.perf_counter()                         # the C entry point on packed arrays: it synchronises before it returns
                ctx.check(ctx.L.lmono_excalib_step(cal.h, n, st.ctypes.data, m.ctypes.data, flat.ctypes.data, q.ctypes.data, 10, R.ctypes.data, stats.ctypes.data,
                                                   rlc.ctypes.data, sv.ctypes.data, hub.ctypes.data, ok.ctypes.data))
                if c >= a.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            ms = np.array(ms)
            out["runs"].append({"streams": n, "ms_per_call_median": float(np.median(ms)), "ms_per_call_min": float(ms.min()),
                                "steps_per_s": n / (float(np.median(ms)) * 1e-3)})
            cal.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
