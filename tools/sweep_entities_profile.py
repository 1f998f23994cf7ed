"""What rt_sweep_entities costs beside the world sweep it contains (profiles/sweep_entities_bench.txt, DESIGN.md "Entity sweeps").

    python tools/sweep_entities_profile.py                              # every configuration, each under rocprofv3 in a process of its own
    python tools/sweep_entities_profile.py COUNT BOXES MODELS COHERENT  # one configuration (what the first form runs under the profiler)

One configuration is `rt_bench --entity-sweeps COUNT --boxes BOXES --models MODELS [--coherent]`: player-sized sweeps beside BOXES
player boxes and MODELS 9 x 9 x 12 models at scale 1/8 scattered over the view, in entity order (coherent) or shuffled; the program
runs rt_sweep_entities and rt_sweep_boxes — the yardstick: k_sweep, which the parent has — on the same records, synchronously and
asynchronously.  The first form runs `rocprofv3 --kernel-trace --stats` (nothing else traced; the program after `--`) over 4096,
100 000 and 2^20 sweeps, coherent and not, against 0, 256 + 64 and 4096 + 4096 entities, and writes the mean duration of
k_sweep_entities and of k_sweep and their ratio.  There is no pass/fail bar."""
import csv, glob, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "raytrace_amd", "rt_bench")
COUNTS = (4096, 100000, 1 << 20)
ENTITIES = ((0, 0), (256, 64), (4096, 4096))
KERNELS = ("k_sweep_entities", "k_sweep<")


def command(count, boxes, models, coherent):
    return [BENCH, "--width", "256", "--height", "144", "--entity-sweeps", str(count), "--boxes", str(boxes), "--models", str(models)] + (["--coherent"] if coherent else [])


def one(count, boxes, models, coherent):
    r = subprocess.run(command(count, boxes, models, coherent), cwd=ROOT, capture_output=True, text=True, timeout=280)
    sys.stderr.write(r.stderr[-2000:])
    print([l for l in r.stdout.splitlines() if l.startswith("{")][-1] if r.returncode == 0 else "failed %d" % r.returncode)
    return r.returncode


def profile_all(out_path):
    rows = ["# rocprofv3 --kernel-trace --stats, MI355X: rt_bench --entity-sweeps N --boxes B --models M [--coherent], one process per",
            "# configuration (tools/sweep_entities_profile.py): mean of all launches of k_sweep_entities and of k_sweep on the same sweeps.",
            "%9s %6s %6s %9s %19s %12s %7s  %s" % ("sweeps", "boxes", "models", "coherent", "k_sweep_entities", "k_sweep", "ratio", "")]
    for n in COUNTS:
        for (b, m) in ENTITIES:
            for coherent in (True, False):
                with tempfile.TemporaryDirectory() as tmp:
                    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--"] + command(n, b, m, coherent)
                    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=280)
                    if r.returncode != 0:
                        sys.exit("%d x %d + %d: rocprofv3 exited with %d\n%s" % (n, b, m, r.returncode, r.stderr[-2000:]))
                    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
                    stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
                    if not stats:
                        sys.exit("%d x %d + %d: no kernel_stats.csv" % (n, b, m))
                    avg = {}
                    for rec in csv.DictReader(open(stats[0])):
                        col = lambda key: next(v for k, v in rec.items() if k.lower().startswith(key))   # Name, Calls, AverageNs, MinNs, MaxNs
                        for k in KERNELS:
                            if k in col("name"):
                                avg[k] = float(col("average")) / 1e3
                    note = ""
                    if line:
                        j = json.loads(line[-1])
                        note = "blocked by entity %d, embedded %d, by world %d" % (j["blocked_by_entity"], j["embedded_in_entity"], j["blocked_by_world"])
                    rows.append("%9d %6d %6d %9s %16.2f us %9.2f us %7.2f  %s" % (n, b, m, "yes" if coherent else "no", avg[KERNELS[0]], avg[KERNELS[1]],
                                                                                 avg[KERNELS[0]] / avg[KERNELS[1]], note))
                    print(rows[-1], flush=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    if len(sys.argv) >= 5:
        sys.exit(one(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4] not in ("0", "no", "false")))
    profile_all(sys.argv[1] if len(sys.argv) == 2 else os.path.join(ROOT, "profiles", "sweep_entities_bench.txt"))
