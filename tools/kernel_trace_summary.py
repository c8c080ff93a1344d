#!/usr/bin/env python3
"""Developer tool: turn the CSV output of `rocprofv3 --kernel-trace --stats -f csv` over the pipelined bench
into the one-file text summary to keep under profiles/ (r07_*_launch_trace_*.txt): the stats table, then every
dispatch of the MPC kernel in start order with its hardware queue, grid, start and duration, then per queue how
its launches follow each other and how many launches overlap in time.

  kernel_trace_summary.py <rocprof output dir> <out.txt> [key=value ...]   (the pairs go into the file's head)
"""
import csv
import glob
import os
import sys


def find(d, suffix):
    hits = sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True))
    return hits[0] if hits else None


def col(row, *names):
    for n in names:
        if n in row and row[n] != "":
            return row[n]
    return ""


def main():
    d, out = sys.argv[1], sys.argv[2]
    head = sys.argv[3:]
    lines = ["rocprofv3 --kernel-trace --stats of `python bench.py --gpus 1` (nothing else traced)"]
    lines += head
    stats = find(d, "kernel_stats.csv")
    if stats:
        lines.append("")
        lines.append("kernel stats (name, calls, total us, average us, percentage):")
        with open(stats, newline="") as f:
            for r in csv.DictReader(f):
                lines.append("  %-60s %5s %14.1f %12.1f %7.2f" % (
                    col(r, "Name")[:60], col(r, "Calls"), float(col(r, "TotalDurationNs") or 0) / 1e3,
                    float(col(r, "AverageNs") or 0) / 1e3, float(col(r, "Percentage") or 0)))
    trace = find(d, "kernel_trace.csv")
    rows = []
    if trace:
        with open(trace, newline="") as f:
            for r in csv.DictReader(f):
                if "fbstab_mpc" not in col(r, "Kernel_Name"):
                    continue
                rows.append((int(col(r, "Start_Timestamp")), int(col(r, "End_Timestamp")), col(r, "Queue_Id"),
                             int(col(r, "Grid_Size_X", "Grid_Size") or 0), int(col(r, "Workgroup_Size_X", "Workgroup_Size") or 1)))
    rows.sort()
    if rows:
        t0 = rows[0][0]
        lines.append("")
        lines.append("MPC kernel dispatches in start order (queue, workgroups, start ms, duration ms, launches running at its start):")
        for s, e, q, g, w in rows:
            live = sum(1 for s2, e2, _, _, _ in rows if s2 <= s < e2)
            lines.append("  queue %-4s wgs %5d  start %10.3f  dur %9.3f  running %d" % (q, g // max(w, 1), (s - t0) / 1e6, (e - s) / 1e6, live))
        lines.append("")
        lines.append("per queue: launches, mean duration ms, mean gap ms from one launch's end to the next one's start")
        for q in sorted(set(r[2] for r in rows)):
            mine = [r for r in rows if r[2] == q]
            gaps = [(b[0] - a[1]) / 1e6 for a, b in zip(mine, mine[1:])]
            lines.append("  queue %-4s n %3d  dur %9.3f  gap %9.3f" % (
                q, len(mine), sum(e - s for s, e, _, _, _ in mine) / 1e6 / len(mine), sum(gaps) / len(gaps) if gaps else 0.0))
        # time-weighted number of launches running, first start to last end
        ev = sorted([(s, 1) for s, _, _, _, _ in rows] + [(e, -1) for _, e, _, _, _ in rows])
        area, live, last = 0.0, 0, ev[0][0]
        for t, dlt in ev:
            area += live * (t - last)
            live += dlt
            last = t
        span = max(r[1] for r in rows) - t0
        lines.append("")
        lines.append("dispatches %d  mean duration %.3f ms  span %.3f ms  launches running, time-weighted mean %.2f" % (
            len(rows), sum(e - s for s, e, _, _, _ in rows) / 1e6 / len(rows), span / 1e6, area / span))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
