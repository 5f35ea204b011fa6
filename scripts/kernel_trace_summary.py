"""Per-kernel duration summary of a rocprofv3 --kernel-trace csv: median, p10, p90 over the second half of the run."""
import csv, glob, re, sys
import numpy as np
f = glob.glob(sys.argv[1] + "/**/*_kernel_trace.csv", recursive=True)[0]
rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))), key=lambda r: r[0])
rows = rows[len(rows) // 2:]
def short(n):
    n = re.sub(r"\(.*", "", n).replace("isdqn::", "").replace("void ", "")
    return n[:78]
by = {}
order = []
for s, e, n in rows:
    k = short(n)
    if k not in by:
        by[k] = []; order.append(k)
    by[k].append((e - s) / 1e3)
first = [s for s, e, n in rows if "conv_fwd_u8_pair" in n]
if len(first) > 2:
    d = np.diff(first) / 1e3
    print("step period us: median %.1f p10 %.1f p90 %.1f (n %d)" % (np.median(d), np.percentile(d, 10), np.percentile(d, 90), len(d)))
for k in order:
    v = np.array(by[k])
    if len(v) < 50: continue
    print("%-80s n %5d  med %7.2f  p10 %7.2f  p90 %7.2f" % (k, len(v), np.median(v), np.percentile(v, 10), np.percentile(v, 90)))
