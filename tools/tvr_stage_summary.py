#!/usr/bin/env python3
"""Per-stage device time of the two-view reconstruction from a `rocprofv3 --kernel-trace --stats` run of tools/tvr_probe.py:
    python tools/tvr_stage_summary.py <dir with *kernel_stats.csv>  ->  name, calls, total ms, mean us of every k_tvr_* kernel"""
import csv
import glob
import os
import sys


def main():
    files = glob.glob(os.path.join(sys.argv[1], "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit("no kernel_stats.csv under " + sys.argv[1])
    for row in csv.DictReader(open(files[0])):
        if "k_tvr_" in row["Name"]:
            name = row["Name"].split("k_tvr_")[1].split("(")[0].split("E")[0]
            print("k_tvr_%-12s calls %5s total %10.3f ms mean %10.1f us" % (name, row["Calls"], float(row["TotalDurationNs"]) / 1e6, float(row["AverageNs"]) / 1e3))


if __name__ == "__main__":
    main()
