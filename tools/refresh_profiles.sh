#!/bin/bash
# Regenerates the bench lines, rocprofv3 kernel statistics and PMC traffic kept under profiles/ (run on an MI355X:
# `bash tools/refresh_profiles.sh OUTDIR`; results land in OUTDIR and are copied to profiles/ by hand).
# Every step appends to OUTDIR/refresh.log so a long run never looks silent.
set -e
OUT="$(realpath -m "${1:?usage: tools/refresh_profiles.sh OUTDIR}")"
cd "$(dirname "$0")/.."
R=r04
mkdir -p "$OUT"
log() { echo "[$(date +%T)] $*" | tee -a "$OUT/refresh.log"; }
export TMPDIR=/tmp
log "bench --streams 1 under rocprofv3 --kernel-trace --stats"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof1" -o p1 -- python3 bench.py --full --no-cpu-baseline --steps 10 --streams 1 --steps-720p 0 > "$OUT/${R}_bench_streams1_under_rocprof.json" 2>> "$OUT/refresh.log"
log "bench default under rocprofv3 --kernel-trace --stats"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof3" -o p3 -- python3 bench.py --full --no-cpu-baseline --steps 10 --steps-720p 0 > "$OUT/${R}_bench_default_under_rocprof.json" 2>> "$OUT/refresh.log"
cp "$(find "$OUT/prof1" -name '*kernel_stats.csv' | head -1)" "$OUT/${R}_bench_streams1_kernel_stats.csv"
cp "$(find "$OUT/prof3" -name '*kernel_stats.csv' | head -1)" "$OUT/${R}_bench_default_kernel_stats.csv"
find "$OUT/prof3" "$OUT/prof1" -name "*kernel_trace.csv" -delete
cp "$(find "$OUT/prof1" -name '*kernel_stats.csv' | head -1)" "$OUT/${R}_bench_streams1_kernel_stats.csv"
log "PMC passes (separate runs, counters only): FETCH_SIZE, WRITE_SIZE"
rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/pmc_fetch" -o f -- python3 bench.py --no-cpu-baseline --steps 2 --warmup 1 --streams 1 --steps-720p 0 --no-profile > /dev/null 2>> "$OUT/refresh.log"
rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/pmc_write" -o w -- python3 bench.py --no-cpu-baseline --steps 2 --warmup 1 --streams 1 --steps-720p 0 --no-profile > /dev/null 2>> "$OUT/refresh.log"
python3 tools/pmc_traffic.py "$OUT/pmc_fetch" "$OUT/pmc_write" --out "$OUT/${R}_traffic.json" \
    --command "rocprofv3 --pmc FETCH_SIZE|WRITE_SIZE -- python3 bench.py --no-cpu-baseline --steps 2 --warmup 1 --streams 1 --steps-720p 0 --no-profile" >> "$OUT/refresh.log"
# (the raw counter rows of the dominant kernel stay, so that the digest can be recomputed: VERDICT r03 item 6)
for d in fetch write; do python3 - "$d" "$OUT" <<'PY'
import csv, glob, sys
d, out = sys.argv[1:3]
src = glob.glob(f"{out}/pmc_{d}/**/*counter_collection.csv", recursive=True)[0]
rows = [r for r in csv.DictReader(open(src)) if "conv3x3_winograd4m_kernel" in r["Kernel_Name"]]
keep = ["Dispatch_Id", "Kernel_Name", "Grid_Size", "Workgroup_Size", "Counter_Name", "Counter_Value"]
with open(f"{out}/r04_traffic_{d}_rows.csv", "w", newline="") as f:
    w = csv.DictWriter(f, keep); w.writeheader()
    for r in rows:
        r = {k: r[k] for k in keep}; r["Kernel_Name"] = r["Kernel_Name"].split("(")[0][-60:]; w.writerow(r)
PY
done
find "$OUT/pmc_fetch" "$OUT/pmc_write" -name "*counter_collection.csv" -delete
# (the line of the default run reads roofline.traffic from profiles/: put this build's digest there first)
cp "$OUT/${R}_traffic.json" profiles/${R}_traffic.json
log "bench default (3 CPU runs)"
python bench.py --full > "$OUT/${R}_bench_default.json" 2>> "$OUT/refresh.log"
log "pyramid kernels"
rocprofv3 --kernel-trace --output-format csv -d "$OUT/pyrprof" -o pp -- python3 tools/pyramid_bench.py > "$OUT/${R}_pyramid_bench_under_rocprof.txt" 2>> "$OUT/refresh.log"
python3 tools/pyr_kernel_table.py "$(find "$OUT/pyrprof" -name '*kernel_trace.csv' | head -1)" 40 > "$OUT/${R}_pyramid_kernel_table.txt"
find "$OUT/pyrprof" -name "*kernel_trace.csv" -delete
python3 tools/pyramid_bench.py > "$OUT/${R}_pyramid_bench.txt" 2>> "$OUT/refresh.log"
log "pyramid PMC passes (counters only, one pass per set)"
PA="SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVE_CYCLES SQ_WAIT_ANY"
PB="SQ_WAVES SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_ANY"
export ITERS=2
rocprofv3 --pmc $PA --output-format csv -d "$OUT/pyrpmc_a" -o p -- python3 tools/pyramid_bench.py > /dev/null 2>> "$OUT/refresh.log"
rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/pyrpmc_f" -o p -- python3 tools/pyramid_bench.py > /dev/null 2>> "$OUT/refresh.log"
rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/pyrpmc_w" -o p -- python3 tools/pyramid_bench.py > /dev/null 2>> "$OUT/refresh.log"
rocprofv3 --pmc $PB --output-format csv -d "$OUT/pyrpmc_b" -o p -- python3 tools/pyramid_bench.py > /dev/null 2>> "$OUT/refresh.log"
unset ITERS
python3 tools/pyr_pmc_table.py "$OUT/pyrpmc_a" "$OUT/pyrpmc_f" "$OUT/pyrpmc_w" > "$OUT/${R}_pyramid_pmc_a.txt"
python3 tools/pyr_pmc_table.py "$OUT/pyrpmc_b" > "$OUT/${R}_pyramid_pmc_b.txt"
find "$OUT/pyrpmc_a" "$OUT/pyrpmc_f" "$OUT/pyrpmc_w" "$OUT/pyrpmc_b" -name "*counter_collection.csv" -delete
log "host enqueue time per frame (eager) and two ranks on one GPU over RCCL"
python3 tools/probes/enqueue_time.py > "$OUT/${R}_enqueue_time.txt" 2>> "$OUT/refresh.log"
# (RCCL refuses two ranks on one device -- "Duplicate GPU detected" -- so the one-GPU rehearsal of the N = 2 path runs on gloo)
VFI_BENCH_SHARE_GPUS=1 VFI_DIST_BACKEND=gloo python3 bench.py --gpus 2 --steps 6 --warmup 2 --steps-720p 0 --no-profile > "$OUT/${R}_bench_2ranks_one_gpu_gloo.json" 2>> "$OUT/refresh.log" || log "2-rank rehearsal failed"
log done
