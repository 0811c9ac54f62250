"""Shares of a process's kernel time from a `rocprofv3 --kernel-trace --stats --output-format csv` run: the largest rows, then every row
whose name contains one of the given substrings.  The vendor-GEMM probe and torch's random fills of a benchmark's set-up are left out.
usage: python tools/kernel_share.py <directory with *kernel_stats.csv> [substring ...]"""
import csv, glob, sys

fs = glob.glob(sys.argv[1] + "/**/*kernel_stats.csv", recursive=True)
rows = list(csv.DictReader(open(fs[0])))
rows = [r for r in rows if not any(s in r["Name"].lower() for s in ("cijk", "gemm", "randn", "distribution"))]
total = sum(float(r["TotalDurationNs"]) for r in rows)
print(f"{fs[0]}: {total / 1e6:.2f} ms of kernel time without the vendor-GEMM probe and the random fills")


def show(r, digits):
    print(f"{100 * float(r['TotalDurationNs']) / total:7.{digits}f} %  {float(r['TotalDurationNs']) / 1e6:9.3f} ms  {r['Calls']:>7s} calls  {r['Name'][:110]}")


for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:14]:
    show(r, 2)
for key in sys.argv[2:]:
    for r in rows:
        if key in r["Name"]:
            show(r, 3)
