"""Per-launch durations of the search kernels from a rocprofv3 kernel trace of bench.py
(`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python3 bench.py`), as
the launch lists of profiles/r13_search_trace_*.txt: the last 40 launches with the start-to-start
gap to the next one, and the second half of the run summarised.

usage: python tools/search_trace_summary.py DIR"""
import csv
import pathlib
import statistics
import sys


def main():
    root = pathlib.Path(sys.argv[1])
    rows = []
    for f in root.rglob("*kernel_trace.csv"):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                name = r["Kernel_Name"]
                if "template_mfma_kernel" in name or "template_share_kernel" in name:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name.split("(")[0].replace("void ", "")))
    rows.sort()
    print(f"search kernel launches: {len(rows)}")
    print("last 40 launches, ms (start-to-start gap to the next in parentheses):")
    for i in range(max(0, len(rows) - 40), len(rows)):
        s, e, name = rows[i]
        gap = (rows[i + 1][0] - s) / 1e6 if i + 1 < len(rows) else float("nan")
        print(f"  {name[-42:]:>42} {(e - s) / 1e6:8.4f} ({gap:8.4f})")
    half = [(e - s) / 1e6 for s, e, _ in rows[len(rows) // 2:]]
    print(f"second half of the run: min {min(half):.4f} median {statistics.median(half):.4f} max {max(half):.4f} "
          f"mean {statistics.mean(half):.4f} ms; launches under 1 ms: {sum(t < 1 for t in half)} of {len(half)}")
    for f in root.rglob("*kernel_stats.csv"):
        print(f"\nkernel stats ({f.name}):")
        print("".join(open(f).readlines()[:8]).rstrip())


if __name__ == "__main__":
    main()
