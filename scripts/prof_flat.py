#!/usr/bin/env python3
"""Diagnostic: where a k_corr_flat workgroup spends its cycles.  Run on the GPU box through scripts/prof_flat.sh, which builds a
-DLMONO_TILE_PROF library into gpurun_out/ and points LMONO_HIP_LIB at it (s_memtime ticks of thread 0 of every workgroup, 100 MHz)."""
# Every stamp charges the ticks since the previous stamp to its own counter, so the counters partition the kernel's time between the
# first and the last stamp: stage 2 is the sum of its sub-stamps plus the wait at the barrier behind it, and the total is the sum of all.
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
assert os.environ.get("LMONO_HIP_LIB"), "run through scripts/prof_flat.sh"
sys.path.insert(0, ROOT)
import numpy as np, torch, lmono_amd
from workloads import s1 as S1
a = [int(v) for v in sys.argv[1:]]
n, chains, lead = (a + [4541, 256, 7])[:3] if len(a) < 3 else a[:3]
w = S1.S1World(n_az=2000)
xyzi, off = w.scans(w.trajectory(n))
ctx = lmono_amd.Context(0)
xd = torch.from_numpy(xyzi).cuda()
batch = lmono_amd.ScanBatch(ctx, n, int(off[-1]))
batch.scanreg(xd.data_ptr(), off, 64, 5.0, keepalive=xd)
incr = torch.zeros((n, 7), dtype=torch.float64, device="cuda")
batch.odometry_d(chains, lead, incr.data_ptr(), None)
ctx.timing_reset()
batch.odometry_d(chains, lead, incr.data_ptr(), None)
groups, _, _ = ctx.timing()
d = ctx.diag
wgs = max(d[0], 1)
# d[1 + i] = stamp i: 0 1a, 1 1b, 2 barrier behind stage 2, 3 decide + vote, 4 set-up, 10 .. 14 the sub-stamps of stage 2
fine = [("2: chunk search", d[11]), ("2: issuing the gathers", d[12]), ("2: descriptor walk + gathers in flight", d[13]),
        ("2: arithmetic + flushes", d[14]), ("2: last flush", d[15]), ("2: wait at the barrier behind it", d[3])]
stage2 = sum(v for _, v in fine)
stages = [("1a requests", d[1]), ("1b resolve + prefix", d[2]), ("2 candidates", stage2), ("3 decide + vote", d[4]), ("setup", d[5])]
tot = sum(v for _, v in stages)
print("workgroups %d: NN rounds %.2f, walk rounds %.2f per workgroup; 4-point chunks per NN round %.0f, per walk round %.0f" %
      (wgs, d[7] / wgs, d[8] / wgs, d[9] / max(d[7], 1), d[10] / max(d[8], 1)))
for nm, v in stages:
    print("  %-22s %9.0f cycles / workgroup (%4.1f %%)" % (nm, v / wgs, 100 * v / tot))
print("  total %.0f cycles / workgroup" % (tot / wgs))
for nm, v in fine:
    print("    %-40s %9.0f (%4.1f %%)" % (nm, v / wgs, 100 * v / tot))
print("    gather batches per workgroup (thread 0) %.1f, owner switches %.1f" % (d[16] / wgs, d[17] / wgs))
print("    rounds per workgroup as run (max nearest + max walk) %.2f; max over its features of (nearest + walk) %.2f; mean per feature %.2f" %
      ((d[7] + d[8]) / wgs, d[18] / wgs, d[19] / wgs / 128.0))
print({k: round(v, 3) for k, v in groups.items()})
