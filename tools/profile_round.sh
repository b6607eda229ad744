#!/bin/bash
# Round evidence, run ON THE GPU BOX (through gpurun):  tools/profile_round.sh TAG
#  1. rocprofv3 --kernel-trace --stats over the default bench command (2 timed steps) -> gpurun_out/prof_TAG/ + kernel_stats csv
#  2. PMC traffic of the attention kernels: FETCH_SIZE and WRITE_SIZE in SEPARATE passes (they do not fit one, MI355X_MICROARCH.md
#     "rocprofv3 PMC slots"), no trace domains next to --pmc -> gpurun_out/pmc_TAG_{fetch,write}/
#  3. gpurun_out/pmc_traffic_TAG.json: per kernel HBM bytes per launch = (2 x FETCH_SIZE + WRITE_SIZE) KB  (gfx950: FETCH_SIZE counts
#     128-B requests as 64 B -> doubled, as the guide prescribes; WRITE_SIZE taken as reported)
tag=${1:-r02}
R=${GRAFT_REPO_ROOT:-/root/repo}
cd /tmp && export TMPDIR=/tmp
# the HEADLINE process only (--no-other-configs --no-scorer: round 5 profiled the default command, whose cfg3 child wrote the first csv `find | head -1` picked up)
PSTEPS=2; PWARM=1
timeout 900 rocprofv3 --kernel-trace --stats -d $R/gpurun_out/prof_$tag --output-format csv -- python $R/bench.py --steps $PSTEPS --warmup $PWARM --no-cpu-baseline \
    --full \
    --no-other-configs --no-scorer > $R/gpurun_out/prof_${tag}_bench.json 2> $R/gpurun_out/prof_$tag.log
nf=$(find $R/gpurun_out/prof_$tag -name "*kernel_stats.csv" | wc -l)
[ "$nf" -ne 1 ] && echo "profile_round.sh: expected ONE kernel_stats.csv (one traced process), found $nf" | tee -a $R/gpurun_out/prof_$tag.log
f=$(find $R/gpurun_out/prof_$tag -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && cp $f $R/gpurun_out/${tag}_bench_kernel_stats.csv && python $R/profiles/summarize.py $f 40 > $R/gpurun_out/${tag}_bench_kernel_stats_summary.txt
# the trace must be the headline's: 84 forward launches (42 blocks x reference + policy pass) per step x (steps + warm-up)
python - "$f" $((84 * (PSTEPS + PWARM))) <<'PYEOF' | tee -a $R/gpurun_out/prof_$tag.log
import csv, sys
want = int(sys.argv[2])
n = sum(int(r["Calls"]) for r in csv.DictReader(open(sys.argv[1])) if r["Name"].startswith("void attn_fwd_w1_kernel<false>") or r["Name"].startswith("attn_fwd_w1_kernel<false>"))
print(f"profile_round.sh: attn_fwd_w1_kernel<false> launches in the trace: {n} (expected {want})" + ("" if n == want else "  <-- NOT the headline process's trace"))
sys.exit(0 if n == want else 3)
PYEOF
find $R/gpurun_out/prof_$tag -name "*kernel_trace.csv" -delete    # large; the stats are what is kept
timeout 300 rocprofv3 --pmc FETCH_SIZE -d $R/gpurun_out/pmc_${tag}_fetch --output-format csv -- python $R/tools/attn_bench.py --iters 2 > $R/gpurun_out/pmc_${tag}_fetch.log 2>&1
timeout 300 rocprofv3 --pmc WRITE_SIZE -d $R/gpurun_out/pmc_${tag}_write --output-format csv -- python $R/tools/attn_bench.py --iters 2 > $R/gpurun_out/pmc_${tag}_write.log 2>&1
# matrix-pipe occupancy and the clock the kernels really run at: SQ counters in one pass, GRBM in its own; kernel durations from a --stats pass
timeout 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_MFMA SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAVE_CYCLES -d $R/gpurun_out/pmc_${tag}_sq --output-format csv -- python $R/tools/attn_bench.py --iters 2 > $R/gpurun_out/pmc_${tag}_sq.log 2>&1
timeout 300 rocprofv3 --pmc GRBM_GUI_ACTIVE -d $R/gpurun_out/pmc_${tag}_grbm --output-format csv -- python $R/tools/attn_bench.py --iters 2 > $R/gpurun_out/pmc_${tag}_grbm.log 2>&1
timeout 300 rocprofv3 --kernel-trace --stats -d $R/gpurun_out/prof_${tag}_attn --output-format csv -- python $R/tools/attn_bench.py --iters 4 > $R/gpurun_out/prof_${tag}_attn.log 2>&1
fa=$(find $R/gpurun_out/prof_${tag}_attn -name "*kernel_stats.csv" | head -1)
[ -n "$fa" ] && cp $fa $R/gpurun_out/${tag}_attn_kernel_stats.csv
find $R/gpurun_out/prof_${tag}_attn -name "*kernel_trace.csv" -delete
timeout 300 rocprofv3 --pmc FETCH_SIZE -d $R/gpurun_out/pmc_${tag}_fetch_ew --output-format csv -- python $R/tools/ew_bench.py > $R/gpurun_out/pmc_${tag}_fetch_ew.log 2>&1
timeout 300 rocprofv3 --pmc WRITE_SIZE -d $R/gpurun_out/pmc_${tag}_write_ew --output-format csv -- python $R/tools/ew_bench.py > $R/gpurun_out/pmc_${tag}_write_ew.log 2>&1
# cfg5 (Wan2.2-TI2V-5B): kernel stats of its bench line, and the same PMC passes over the head_dim-128 attention kernels at the pair-batch shape
timeout 600 rocprofv3 --kernel-trace --stats -d $R/gpurun_out/prof_${tag}_cfg5 --output-format csv -- python $R/bench.py --config cfg5 --steps 2 --warmup 1 \
    --full \
    > $R/gpurun_out/prof_${tag}_bench_cfg5.json 2> $R/gpurun_out/prof_${tag}_cfg5.log
f5=$(find $R/gpurun_out/prof_${tag}_cfg5 -name "*kernel_stats.csv" | head -1)
[ -n "$f5" ] && cp $f5 $R/gpurun_out/${tag}_bench_cfg5_kernel_stats.csv && python $R/profiles/summarize.py $f5 40 > $R/gpurun_out/${tag}_bench_cfg5_kernel_stats_summary.txt
find $R/gpurun_out/prof_${tag}_cfg5 -name "*kernel_trace.csv" -delete
export PYTHONPATH=$R
A128="python $R/tools/attn128_time.py --B 2 --product-only --iters 2"
timeout 300 rocprofv3 --pmc FETCH_SIZE -d $R/gpurun_out/pmc_${tag}_fetch_a128 --output-format csv -- $A128 > $R/gpurun_out/pmc_${tag}_fetch_a128.log 2>&1
timeout 300 rocprofv3 --pmc WRITE_SIZE -d $R/gpurun_out/pmc_${tag}_write_a128 --output-format csv -- $A128 > $R/gpurun_out/pmc_${tag}_write_a128.log 2>&1
timeout 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_MFMA SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAVE_CYCLES -d $R/gpurun_out/pmc_${tag}_sq_a128 --output-format csv -- $A128 > $R/gpurun_out/pmc_${tag}_sq_a128.log 2>&1
timeout 300 rocprofv3 --pmc GRBM_GUI_ACTIVE -d $R/gpurun_out/pmc_${tag}_grbm_a128 --output-format csv -- $A128 > $R/gpurun_out/pmc_${tag}_grbm_a128.log 2>&1
timeout 300 rocprofv3 --kernel-trace --stats -d $R/gpurun_out/prof_${tag}_a128 --output-format csv -- $A128 > $R/gpurun_out/prof_${tag}_a128.log 2>&1
fb=$(find $R/gpurun_out/prof_${tag}_a128 -name "*kernel_stats.csv" | head -1)
[ -n "$fb" ] && cp $fb $R/gpurun_out/${tag}_attn128_kernel_stats.csv
find $R/gpurun_out/prof_${tag}_a128 -name "*kernel_trace.csv" -delete
# socket power / shader clock during the default bench command (the power-limit evidence of DESIGN section 4.2)
rocm-smi --showpower --showclocks --showmaxpower --json > $R/gpurun_out/${tag}_rocm_smi_idle.json 2>&1
timeout 300 python $R/tools/power_trace.py --out $R/gpurun_out/power_${tag}.json -- python $R/bench.py --steps 6 --warmup 1 --no-cpu-baseline --no-kernel-timer \
    --full \
    > $R/gpurun_out/power_${tag}_bench.json 2> $R/gpurun_out/power_${tag}.log
# the geometry scorer at the reference's scale (10 x 518^2): kernel stats + FETCH / WRITE traffic of project_zbuf / project_resolve / conf_threshold / mvcs / mse
timeout 300 rocprofv3 --kernel-trace --stats -d $R/gpurun_out/prof_${tag}_scorer --output-format csv -- python $R/tools/scorer_bench.py > $R/gpurun_out/prof_${tag}_scorer.log 2>&1
fs=$(find $R/gpurun_out/prof_${tag}_scorer -name "*kernel_stats.csv" | head -1)
[ -n "$fs" ] && cp $fs $R/gpurun_out/${tag}_scorer_kernel_stats.csv && python $R/profiles/summarize.py $fs 20 > $R/gpurun_out/${tag}_scorer_kernel_stats_summary.txt
find $R/gpurun_out/prof_${tag}_scorer -name "*kernel_trace.csv" -delete
timeout 300 rocprofv3 --pmc FETCH_SIZE -d $R/gpurun_out/pmc_${tag}_fetch_scorer --output-format csv -- python $R/tools/scorer_bench.py --quick > $R/gpurun_out/pmc_${tag}_fetch_scorer.log 2>&1
timeout 300 rocprofv3 --pmc WRITE_SIZE -d $R/gpurun_out/pmc_${tag}_write_scorer --output-format csv -- python $R/tools/scorer_bench.py --quick > $R/gpurun_out/pmc_${tag}_write_scorer.log 2>&1
python $R/tools/pmc_traffic.py $R/gpurun_out $tag
