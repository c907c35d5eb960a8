#!/usr/bin/env python3
"""tools/front_end_trace.py <kernel_trace.csv> [steps] -- what runs in front of the best-first scan, from a
`rocprofv3 --kernel-trace` file of the default bench command: per kernel the mean and median time of its last
`steps` dispatches (default 20: the timed steps), and the start-to-start gap from each of them to the dispatch
that follows it.  One JSON object on stdout; profiles/front_end_*.json are its output."""
import csv
import json
import re
import statistics
import sys

FRONT = ("project_tile_kernel", "project_kernel", "lut_build_batch_kernel", "lut_build_kernel", "query_cost_kernel",
         "cost_sort_kernel", "cost_scatter_kernel", "fillBufferAligned", "scan_bytes_bf_kernel")


def short(name):
    m = re.search(r"([A-Za-z_0-9]+)(<[^(]*>)?\(", name)
    base = m.group(1) if m else name.split("(")[0].split(" ")[-1].split("<")[0]
    if base == "scan_bytes_bf_kernel":
        t = re.search(r"scan_bytes_bf_kernel(<[^(]*>)", name)
        return base + (t.group(1) if t else "")
    return base


def main():
    path = sys.argv[1]
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    dur, gap = {}, {}
    for i, (s, e, n) in enumerate(rows):
        if not any(n.startswith(p) for p in FRONT):
            continue
        dur.setdefault(n, []).append((e - s) / 1e3)
        if i + 1 < len(rows):
            gap.setdefault(n + " -> " + rows[i + 1][2], []).append((rows[i + 1][0] - s) / 1e3)

    def stat(v):
        v = v[-steps:]
        return {"n": len(v), "mean_us": round(statistics.mean(v), 2), "median_us": round(statistics.median(v), 2),
                "min_us": round(min(v), 2), "max_us": round(max(v), 2)}

    out = {"source": path, "last_dispatches": steps,
           "kernel_us": {k: stat(v) for k, v in sorted(dur.items())},
           "start_to_start_us": {k: stat(v) for k, v in sorted(gap.items()) if len(v) >= steps}}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
