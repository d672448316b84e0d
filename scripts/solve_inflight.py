#!/usr/bin/env python3
"""How much of the odometry's main pass do k_lm_solve launches hold?  Reads a rocprofv3 kernel trace (csv with start and end stamps) of a
headline run and prints, per step and in all: the span covered by k_corr_flat launches, the time integral of the number of k_lm_solve
launches in flight inside it, and per-launch durations of both kernels.
  usage: solve_inflight.py <kernel_trace.csv | launches.csv written by an earlier run> [launches_out.csv]"""
import csv
import sys


def main():
    rows = []
    with open(sys.argv[1], newline="") as f:
        for r in csv.DictReader(f):
            if "start_ns" in r:          # a launches file written by this script
                rows.append((int(r["start_ns"]), int(r["end_ns"]), r["kernel"], int(r["workgroup"]), int(r["grid"]), int(r["lds"]), int(r["vgpr"])))
                continue
            name = r["Kernel_Name"]
            short = "k_lm_solve" if "k_lm_solve" in name else "k_corr_flat" if "k_corr_flat" in name else "k_correspond_list" if "k_correspond_list" in name else None
            if short:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short, int(r.get("Workgroup_Size_X", 0) or 0), int(r.get("Grid_Size_X", 0) or 0),
                             int(r.get("LDS_Block_Size", 0) or 0), int(r.get("VGPR_Count", 0) or 0) + int(r.get("Accum_VGPR_Count", 0) or 0)))
    rows.sort()
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write("start_ns,end_ns,kernel,workgroup,grid,lds,vgpr\n")
            t0 = rows[0][0]
            for s, e, n, wg, g, lds, vg in rows:
                f.write("%d,%d,%s,%d,%d,%d,%d\n" % (s - t0, e - t0, n, wg, g, lds, vg))
    # steps: a gap of more than 5 ms between search launches separates two steps (the front end runs in between)
    cf = [r for r in rows if r[2] == "k_corr_flat"]
    steps, cur = [], [cf[0]]
    for r in cf[1:]:
        if r[0] - max(x[1] for x in cur[-8:]) > 5_000_000:
            steps.append(cur); cur = []
        cur.append(r)
    steps.append(cur)
    lm = [r for r in rows if r[2] == "k_lm_solve"]
    print("step  span_ms  main_pass_ms  lm_launches  lm_sum_ms  lm_inflight_mean  lm_wg_mean  cu_share_of_256")
    tot_span = tot_int = tot_wg = 0.0
    for i, st in enumerate(steps):
        a, b = min(r[0] for r in st), max(r[1] for r in st)
        # the main pass: the longest run of search launches without a gap above 0.1 ms (the boundary check and every repair chunk follow a
        # host synchronisation, 0.06 - 0.2 ms without a search launch)
        st.sort()
        runs, run = [], [st[0]]
        for r in st[1:]:
            if r[0] - max(x[1] for x in run[-8:]) > 100_000:
                runs.append(run); run = []
            run.append(r)
        runs.append(run)
        mp = max(runs, key=lambda q: max(r[1] for r in q) - q[0][0])
        ma, mb = mp[0][0], max(r[1] for r in mp)
        inside = [r for r in lm if r[1] > ma and r[0] < mb]
        integ = sum(min(r[1], mb) - max(r[0], ma) for r in inside)
        wg_integ = sum((min(r[1], mb) - max(r[0], ma)) * (r[4] // max(r[3], 1)) for r in inside)
        span = mb - ma
        print("%4d  %7.3f  %12.3f  %11d  %9.3f  %16.3f  %10.1f  %15.3f" % (i, (b - a) / 1e6, span / 1e6, len(inside), sum(r[1] - r[0] for r in inside) / 1e6,
                                                                     integ / span, wg_integ / max(integ, 1), wg_integ / span / 256.0))
        if i > 0:            # step 0 is the warm-up
            tot_span += span; tot_int += integ; tot_wg += wg_integ
    if tot_span:
        print("timed steps: k_lm_solve launches in flight over the main pass, mean %.3f; workgroups (= CUs held at one per CU) %.1f; share of 256 CUs %.3f"
              % (tot_int / tot_span, tot_wg / tot_span, tot_wg / tot_span / 256.0))
    for n in ("k_corr_flat", "k_correspond_list", "k_lm_solve"):
        d = sorted((r[1] - r[0]) / 1e3 for r in rows if r[2] == n)
        if d:
            print("%-18s launches %5d  us: mean %8.1f  min %8.1f  median %8.1f  p90 %8.1f  max %8.1f  lds %s vgpr %s"
                  % (n, len(d), sum(d) / len(d), d[0], d[len(d) // 2], d[int(len(d) * 0.9)], d[-1],
                     sorted({r[5] for r in rows if r[2] == n}), sorted({r[6] for r in rows if r[2] == n})))


if __name__ == "__main__":
    main()
