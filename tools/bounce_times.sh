#!/bin/bash
# Launch times of a batch's kernels from a rocprofv3 kernel trace (run on the GPU box from the repo root):
#   bash tools/bounce_times.sh <tag> [bench args]   -> gpurun_out/<tag>_bounce_times.txt
# A batch ends with its k_accumulate.  One line per batch: the instrumented batch of bench.py --full, the warm-up step (the
# one batch after it that (re)builds the primary stage: k_raygen, the bounce-0 walk, k_primary_hit; the first full-size
# batch is also slower than the later ones), then the three timed steps, which start at their first k_shade while the camera
# stands still; then the timed steps' means per launch.  BENCH_ROOT=<dir>: trace that checkout's
# bench.py (A/B against another build).
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
BENCH=${BENCH_ROOT:-$ROOT}
TAG=$1; shift
OUT=$ROOT/gpurun_out/bt_$TAG
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --output-format csv -d $OUT -- python3 $BENCH/bench.py --full --no-cpu-baseline --no-secondary --steps 3 --warmup 1 "$@" > $OUT/run.log 2>&1 || { tail -5 $OUT/run.log; exit 1; }
python3 - "$OUT" <<'PY' | tee $ROOT/gpurun_out/${TAG}_bounce_times.txt
import csv, glob, sys
STAGES = ("k_raygen", "k_traverse", "k_occluded8_seeded", "k_primary_hit", "k_shade", "k_accumulate")
TIMED = 3  # --steps above
rows = []
for f in glob.glob(sys.argv[1] + "/*/*kernel_trace.csv"):
    for r in csv.DictReader(open(f)):
        n = r["Kernel_Name"].split("(")[0]
        n = n[5:] if n.startswith("void ") else n
        if n.startswith(STAGES):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), n))
rows.sort()
batches, cur = [], []
for t, d, n in rows:
    cur.append((d, n, t))
    if n.startswith("k_accumulate"):
        batches.append(cur)
        cur = []
print(f"{len(batches)} batches; per batch: launches, sum of the launches, first launch's start to last launch's end, each launch (us)")
for i, b in enumerate(batches):
    print(f"{i} {len(b):2d} sum {sum(d for d, _, _ in b) / 1e3:9.1f} span {(b[-1][2] + b[-1][0] - b[0][2]) / 1e3:9.1f} |",
          " ".join(f"{d / 1e3:.0f}" for d, _, _ in b))
timed = batches[-TIMED:]
shape = [n for _, n, _ in timed[0]]
if all([n for _, n, _ in b] == shape for b in timed):
    print(f"--- the {TIMED} timed steps, mean per launch (us)")
    total = 0.0
    for k, n in enumerate(shape):
        m = sum(b[k][0] for b in timed) / TIMED / 1e3
        total += m
        print(f"{k:2d} {m:9.1f}  {n[:90]}")
    print(f"   {total:9.1f}  sum of a batch's launches")
    print(f"   {sum(b[-1][2] + b[-1][0] - b[0][2] for b in timed) / TIMED / 1e3:9.1f}  first launch's start to last launch's end")
else:
    print("the timed steps launched different kernel sequences")
PY
