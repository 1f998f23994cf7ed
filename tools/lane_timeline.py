"""Where the launches of consecutive frames lie when two frames are in flight (frame_timeline.py assumes one stream): rocprofv3
--kernel-trace of a bench run -> per frame k + 1, relative to the END of frame k's path launch (us; negative = inside its drain):
when the prepass of frame k + 1 begins and ends, when its path launch begins, and when frame k's accumulate launch runs.
    python tools/lane_timeline.py <dir with *_kernel_trace.csv> [frames from the end, default 10]"""
import csv, glob, sys

f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
last = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(f))]
rows.sort(key=lambda r: r[1])
paths = [r for r in rows if "k_paths" in r[0]]
prim = [r for r in rows if "k_primary" in r[0]]
acc = [r for r in rows if "k_accumulate_paths" in r[0]]
# only the full-size launches (the bench's counting and depth-0 contexts and the reference frame launch smaller or other kernels)
long_ = max(p[2] - p[1] for p in paths)
paths = [p for p in paths if p[2] - p[1] > long_ / 2][-(last + 1):]
us = lambda t, t0: (t - t0) / 1e3
cols = ("prepass begin", "prepass end", "paths begin", "paths runs", "accumulate begin", "accumulate end")
table = []
for a, b in zip(paths[:-1], paths[1:]):
    t0 = a[2]
    p = [r for r in prim if a[1] < r[1] < b[1]]
    c = [r for r in acc if r[1] >= t0 - 1000]
    table.append((us(p[-1][1], t0) if p else None, us(p[-1][2], t0) if p else None, us(b[1], t0), us(b[2], b[1]),
                  us(c[0][1], t0) if c else None, us(c[0][2], t0) if c else None))
print("%d frames; us relative to the end of the previous frame's path launch (paths runs: begin to end)" % len(table))
print("  " + "".join("%18s" % c for c in cols))
for row in table:
    print("  " + "".join("%18s" % ("-" if v is None else "%.1f" % v) for v in row))
med = []
for i in range(len(cols)):
    v = sorted(r[i] for r in table if r[i] is not None)
    med.append(v[len(v) // 2] if v else None)
print("median" + "".join("%18s" % ("-" if v is None else "%.1f" % v) for v in med)[4:])
period = sorted(us(b[1], a[1]) for a, b in zip(paths[:-1], paths[1:]))
print("path launch begin to next path launch begin: median %.1f us" % period[len(period) // 2])
