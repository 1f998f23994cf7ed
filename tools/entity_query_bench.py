"""Entity-query cost on the MI355X (DESIGN.md "Entity queries"): rt_trace_entities against rt_trace_rays on the same rays.

    python tools/entity_query_bench.py [OUT]

Runs `rt_bench --entity-rays N [--coherent] --boxes B --models M` for every configuration under `rocprofv3 --kernel-trace --stats` (no
counters; the program after `--`; a process of its own each) and writes, per configuration, the device time of k_entity_query and of
k_query from the trace beside rt_bench's own JSON line (call-to-return ms of both calls, the device ms of their asynchronous twins
between two events, rays that report an entity, rays whose entity the world occludes) to OUT (default profiles/entity_query_bench.txt)."""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAYS = [1 << 16, 1 << 20]
ENTITIES = [(0, 0), (64, 64), (1024, 1024), (4096, 4096)]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "entity_query_bench.txt")
    bench = os.path.join(ROOT, "raytrace_amd", "rt_bench")
    rows = ["# rocprofv3 --kernel-trace --stats, MI355X: rt_bench --entity-rays N [--coherent] --boxes B --models M (tools/entity_query_bench.py;",
            "# one process per configuration): rt_trace_entities and rt_trace_rays on the same rays, 1920x1080 camera, 9 x 9 x 12 stamp at 1/8",
            "# (the rows with the most calls are the timed calls and their asynchronous twins, and the ratio is theirs; a k_entity_query row with",
            "# one call is rt_bench's count of occluded entities: the window moved away, every ray under the sky, the kernel's other instantiation)"]
    for coherent in (True, False):
        for n in RAYS:
            for nb, nm in ENTITIES:
                tag = "%s_%d_%db_%dm" % ("coherent" if coherent else "incoherent", n, nb, nm)
                with tempfile.TemporaryDirectory() as tmp:
                    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", bench, "--entity-rays", str(n),
                           "--boxes", str(nb), "--models", str(nm), "--width", "1920", "--height", "1080"] + (["--coherent"] if coherent else [])
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
                    if r.returncode != 0:
                        sys.exit("%s: rocprofv3 exited with %d\n%s" % (tag, r.returncode, r.stderr[-2000:]))
                    stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
                    if not stats:
                        sys.exit("%s: no kernel_stats.csv" % tag)
                    avg, calls = {}, {}
                    for rec in csv.DictReader(open(stats[0])):
                        col = lambda key: next(v for k, v in rec.items() if k.lower().startswith(key))   # Name, Calls, AverageNs, MinNs, MaxNs
                        for kernel in ("k_entity_query", "k_query"):
                            if kernel in col("name"):
                                # (rt_bench's one call with the window moved away runs the kernel's other instantiation: a row of its own)
                                if int(col("calls")) > calls.get(kernel, 0):
                                    avg[kernel], calls[kernel] = float(col("average")) / 1e6, int(col("calls"))
                                rows.append("%-36s %-16s calls %4d avg_ms %9.4f min_ms %9.4f max_ms %9.4f" % (
                                    tag, kernel, int(col("calls")), float(col("average")) / 1e6, float(col("min")) / 1e6, float(col("max")) / 1e6))
                    if len(avg) != 2:
                        sys.exit("%s: a kernel is missing from the trace" % tag)
                    rows.append("%-36s k_entity_query / k_query = %.2f" % (tag, avg["k_entity_query"] / avg["k_query"]))
                    line = [l for l in r.stdout.splitlines() if l.startswith("{\"entity_rays\"")]
                    if line:
                        j = json.loads(line[-1])
                        rows.append("%-36s rt_bench: call to return %.3f / %.3f ms, events round the asynchronous calls %.4f / %.4f ms, %d rays report an "
                                    "entity, %d occluded, %d under the sky" % (
                                        tag, j["trace_entities_call_ms"], j["trace_rays_call_ms"], j["trace_entities_device_ms"], j["trace_rays_device_ms"],
                                        j["entities_reported"], j["entities_occluded"], j["reported_under_sky"]))
                    print("\n".join(x for x in rows if x.startswith(tag)), flush=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
