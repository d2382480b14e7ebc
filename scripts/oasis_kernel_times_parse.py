"""Durations of the oasis kernels of one rocprofv3 kernel trace, in launch order."""
import csv
import glob
import sys

for path in sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)):
    rows = list(csv.DictReader(open(path)))
    if not rows:
        print(path, "empty")
        continue
    keys = rows[0].keys()
    name = "Kernel_Name" if "Kernel_Name" in keys else [k for k in keys if "ame" in k][0]
    rows = [r for r in rows if "oasis" in r[name]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for kern in ("oasis_ar1_kernel", "oasis_ar2_kernel"):
        d = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if kern in r[name]]
        print(path.split("/")[-1], kern, "ns in launch order:", d)
