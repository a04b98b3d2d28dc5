#!/bin/bash
# The raw-point store's cost per frame: the resident chain of tools/replay.py (as tools/frame_prof.sh, 60 000-point
# synthetic sweeps) with the store on and off, alternated on / off / on / off, each run under
# rocprofv3 --kernel-trace --stats; then the store at the end of the street drive (tools/probe_raw_points.py).
#   usage (GPU box): bash tools/raw_points_prof.sh OUTDIR [frames] [points]
set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$1; F=${2:-40}; P=${3:-60000}
mkdir -p "$OUT"
i=0
for mode in on off on off; do
  i=$((i + 1))
  flag=""; [ "$mode" = on ] && flag="--raw-points-on-device"
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/run$i" -o $mode -- \
    python3 "$ROOT/tools/replay.py" --synthetic "$F" --points "$P" --device-map --resident $flag --out "$OUT/traj$i.tum" \
    > "$OUT/run$i.log" 2>&1 || { echo "run $i ($mode) failed"; tail -20 "$OUT/run$i.log"; exit 1; }
  grep -E "raw points kept" "$OUT/run$i.log"
  python3 - "$OUT/run$i" "$F" "$mode" <<'PY'
import csv, glob, sys, collections
d, frames, mode = sys.argv[1], int(sys.argv[2]), sys.argv[3]
busy = collections.Counter(); calls = collections.Counter()
for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"].replace("vgicp::(anonymous namespace)::", "").split("(")[0]
        if "insert_" in name or "raw_" in name:
            busy[name] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"]); calls[name] += 1
per_insert = sum(t for n, t in busy.items() if n.startswith("void insert_")) / max(1, calls["void insert_prepare_kernel<true>"])
print(f"store {mode}: {calls['void insert_prepare_kernel<true>']} insertions over {frames} frames, "
      f"insert_prepare + insert_apply_list {per_insert / 1e3:.2f} us per insertion")
for name, t in sorted(busy.items()):
    what = "per insertion" if name.startswith("void insert_") else "(store growth / export, not per frame)"
    print(f"  {t / calls[name] / 1e3:7.2f} us per launch  {calls[name]:4d} launches  {name}  {what}")
PY
done
timeout -k 10 300 python3 "$ROOT/tools/probe_raw_points.py" 300 2>&1 | tail -4
