"""Medians per launch of the tracker kernels from the rocprofv3 runs of tools/lazy_entry_probe.py under <dir>/kt_* (kernel traces: durations)
and <dir>/pmc_* (counter passes: values summed over the device per dispatch)."""
import collections, csv, glob, os, statistics, sys
O = sys.argv[1]
for d in sorted(glob.glob(os.path.join(O, "kt_*"))):
    if not os.path.isdir(d):
        continue
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        dur = collections.defaultdict(list)
        for r in csv.DictReader(open(f)):
            n = r["Kernel_Name"]
            if "track_kernel" in n or "smooth_grad" in n:
                dur[n[:70]].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        for n, v in dur.items():
            print(os.path.basename(d), n, "launches", len(v), "median us %.2f min %.2f" % (statistics.median(v), min(v)))
for d in sorted(glob.glob(os.path.join(O, "pmc_*"))):
    if not os.path.isdir(d):
        continue
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        per = collections.defaultdict(float)
        for r in csv.DictReader(open(f)):
            if "track_kernel_quad" in r["Kernel_Name"]:
                per[(r["Dispatch_Id"], r["Counter_Name"], r["Kernel_Name"][40:75])] += float(r["Counter_Value"])
        by = collections.defaultdict(list)
        for (disp, c, n), v in per.items():
            by[(c, n)].append(v)
        for (c, n), v in sorted(by.items()):
            print(os.path.basename(d), n, c, "dispatches", len(v), "median %.0f" % statistics.median(v))
