"""One row per world-changing API call and region size from rocprofv3 kernel traces of tools/slab_timing.py and
tools/terrain_gen_bench.py: the call's device time = the sum of the kernels it launches, averaged over its calls.

    python tools/world_rows.py RUN_NAME kernel_trace.csv [kernel_trace.csv ...]

A call starts at its head kernel and owns the map / fill kernels that follow it.  R comes from the head's grid (an edit's and a
self-test's from the call before them), a generated slab's axis from k_terrain_fill's grid, an uploaded slab's from slab_timing.py's order (axis by axis,
equal counts)."""
import csv, re, sys
from collections import defaultdict

HEADS = {"k_flatten_voxels": "rt_upload_world", "k_flatten_slab": "rt_upload_slice", "k_rebuild_chunks": "rt_edit_voxels",
         "k_terrain_heights": "rt_generate", "k_check_maps": "rt_selftest(maps)"}
TAIL = re.compile(r"k_(build_|terrain_|rebuild_chunk_maps)")   # the fill and map kernels a head is followed by

run = sys.argv[1]
rows = defaultdict(list)      # (api, R, axis) -> [(total ns, {kernel: ns})]
for path in sys.argv[2:]:
    trace = sorted(csv.DictReader(open(path)), key=lambda d: int(d["Start_Timestamp"]))
    calls, R = [], 0
    for d in trace:
        name = re.sub(r"^(void )?(rtd::)?", "", d["Kernel_Name"]).split("(")[0].split("<")[0]
        ns = int(d["End_Timestamp"]) - int(d["Start_Timestamp"])
        grid = [int(d["Grid_Size_" + a]) // max(int(d["Workgroup_Size_" + a]), 1) for a in "XYZ"]
        if name in HEADS:
            threads = grid[0] * int(d["Workgroup_Size_X"])
            if name == "k_flatten_voxels": R = round(threads ** (1 / 3))
            elif name == "k_flatten_slab": R = round((threads / 16) ** 0.5)
            calls.append({"api": HEADS[name], "R": R, "axis": "", "ns": {name: ns}})
        elif TAIL.match(name) and calls and calls[-1] is not None:
            c = calls[-1]
            c["ns"][name] = c["ns"].get(name, 0) + ns
            if name == "k_terrain_fill":
                R = c["R"] = max(grid) * 64
                thin = [a for a in range(3) if grid[a] * 64 < c["R"]]
                c["api"], c["axis"] = ("rt_generate_slice", thin[0]) if thin else ("rt_generate_world", "")
        else:
            calls.append(None)    # any other kernel ends the call before it
    calls = [c for c in calls if c]
    for R in {c["R"] for c in calls}:
        slabs = [c for c in calls if c["api"] == "rt_upload_slice" and c["R"] == R]
        assert len(slabs) % 3 == 0, "slab_timing.py uploads the same number of slabs per axis, axis by axis"
        for i, c in enumerate(slabs):
            c["axis"] = i * 3 // len(slabs)
    for c in calls:
        rows[(c["api"], c["R"], c["axis"])].append(c["ns"])
print("run,api,R,axis,calls,avg_us,kernels_avg_us")
for (api, R, axis), cs in sorted(rows.items(), key=lambda kv: (kv[0][0], kv[0][1], str(kv[0][2]))):
    per = defaultdict(float)
    for ns in cs:
        for k, v in ns.items():
            per[k] += v / len(cs) / 1e3
    print("%s,%s,%d,%s,%d,%.2f,%s" % (run, api, R, axis, len(cs), sum(per.values()), " ".join("%s=%.2f" % kv for kv in per.items())))
