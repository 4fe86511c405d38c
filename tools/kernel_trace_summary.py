"""Per-kernel launches / median / min / max duration (us) from the kernel-trace csv of a
`rocprofv3 --kernel-trace --output-format csv` run, longest total first.
    python tools/kernel_trace_summary.py DIR/..._kernel_trace.csv"""
import csv
import re
import statistics
import sys

rows = {}
for r in csv.DictReader(open(sys.argv[1])):
    rows.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)


def short(n):
    n = re.sub(r"\(anonymous namespace\)::|mvn::|void ", "", n)
    n = n.replace("unsigned short", "bf16")
    n = re.sub(r"\(.*", "", n)
    return n[:100]


for name, v in sorted(rows.items(), key=lambda kv: -sum(kv[1])):
    print(f"{short(name):100s} launches {len(v):5d}  median {statistics.median(v):8.2f}  min {min(v):8.2f}  max {max(v):8.2f}")
