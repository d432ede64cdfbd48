#!/bin/bash
# Regenerates the evidence under profiles/ on a GPU box (run through gpurun; results land in gpurun_out/profiles/):
#   1. the default bench line                          -> bench.json
#   2. rocprofv3 --kernel-trace --stats of the same command, train steps only (--no-eval) -> kernel_stats.csv;
#      the evaluation loop alone (tools/eval_loop.py) -> kernel_stats_eval.csv
#   3. separate counter passes (FETCH_SIZE; WRITE_SIZE; MFMA busy) -> pmc_fetch.csv, pmc_write.csv, pmc_mfma.csv
#      and tools/traffic_from_pmc.py -> traffic.json
#   4. the GPU test suite's achieved errors            -> parity_errors.json (tools/parity_summary.py)
#   5. ablation of the layer-1 GEMMs (tools/ablate_planes.py), FETCH_SIZE calibration (tools/calib_fetch.sh),
#      launch-mode comparison, one step's kernel timeline
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=$R/gpurun_out/profiles
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
B="$R/bench.py"
Q="--full --no-cpu-baseline --no-profile --no-dense --no-pcie --no-configs --no-parity-check --no-strict --no-eval"
timeout 600 python3 $B --full --no-cpu-baseline --no-dense --no-pcie --no-configs --steps 30 --warmup 10 > /dev/null 2>&1   # page the image in
timeout 900 python3 $B --full > $O/bench.json 2> $O/bench.err; echo "bench rc=$?"
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt -o kt -- python3 $B $Q --steps 50 --warmup 10 > $O/kt.log 2>&1; echo "kernel-trace rc=$?"
timeout 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_fetch -o pmc -- python3 $B $Q --steps 5 --warmup 3 > $O/pmc_fetch.log 2>&1; echo "pmc fetch rc=$?"
timeout 600 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pmc_write -o pmc -- python3 $B $Q --steps 5 --warmup 3 > $O/pmc_write.log 2>&1; echo "pmc write rc=$?"
timeout 600 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_BF16 --kernel-trace --output-format csv -d $O/pmc_mfma -o pmc -- python3 $B $Q --steps 5 --warmup 3 > $O/pmc_mfma.log 2>&1; echo "pmc mfma rc=$?"
cp $O/pmc_mfma/pmc_counter_collection.csv $O/pmc_mfma.csv 2>/dev/null
# pipe counters of the two layer-1 kernels (what bounds them): LDS, VALU, MFMA instruction and busy counts
for set in "SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_BUSY_CYCLES" "SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_INSTS_VALU_MFMA_MOPS_BF16 SQ_BUSY_CYCLES" "SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_BUSY_CYCLES"; do
  n=$(echo $set | cut -d" " -f1)
  timeout 600 rocprofv3 --pmc $set --kernel-trace --output-format csv -d $O/pmcg_$n -o pmc -- python3 $B $Q --steps 3 --warmup 2 > $O/pmcg_$n.log 2>&1; echo "pmc pipes $n rc=$?"
done
python3 - > $O/pmc_gemm_pipes.txt 2>/dev/null <<PY
import csv, collections, glob
res = collections.defaultdict(dict)
for f in sorted(glob.glob('$O/pmcg_*/pmc_counter_collection.csv')):
    agg = collections.defaultdict(lambda: collections.defaultdict(list))
    for r in csv.DictReader(open(f)):
        agg[r['Kernel_Name'][:48]][r['Counter_Name']].append(float(r['Counter_Value']))
    for k, d in agg.items():
        for c, v in d.items():
            res[k][c] = sum(v) / len(v)
for k, d in res.items():
    if 'gemm_p2' in k or 'gemm_p3' in k or 'gemm_bf16x3_kernel<0, 0' in k or 'gemm_bf16x3_kernel<1, 3' in k:
        print(k)
        for c, v in sorted(d.items()):
            print('   %-34s %16.0f' % (c, v))
PY
rm -rf $O/pmcg_*
cp $O/kt/kt_kernel_stats.csv $O/kernel_stats.csv 2>/dev/null
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kte -o kt -- python3 $R/tools/eval_loop.py 50 > $O/kt_eval.log 2>&1; echo "kernel-trace (eval) rc=$?"
cp $O/kte/kt_kernel_stats.csv $O/kernel_stats_eval.csv 2>/dev/null
cp $O/pmc_fetch/pmc_counter_collection.csv $O/pmc_fetch.csv 2>/dev/null
cp $O/pmc_write/pmc_counter_collection.csv $O/pmc_write.csv 2>/dev/null
python3 $R/tools/traffic_from_pmc.py $O/pmc_fetch.csv $O/pmc_write.csv $O/traffic.json $O/pmc_mfma.csv commit=${LIREC_COMMIT:-unknown} > $O/traffic.log 2>&1
# the pieces-fed step (bench.py's resident_store_layer1_on_pieces leg as a program of its own): kernel stats + FETCH / WRITE passes
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/ktp -o kt -- python3 $R/tools/pieces_step.py resident 30 > $O/kt_pieces.log 2>&1; echo "kernel-trace (pieces) rc=$?"
cp $O/ktp/kt_kernel_stats.csv $O/pieces_kernel_stats.csv 2>/dev/null
for c in FETCH_SIZE WRITE_SIZE; do
  timeout 600 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $O/pmcp_$c -o pmc -- python3 $R/tools/pieces_step.py resident 5 > $O/pmc_pieces_$c.log 2>&1; echo "pmc pieces $c rc=$?"
  python3 $R/tools/pmc_sum.py $O/pmcp_$c/pmc_counter_collection.csv $c 10 > $O/pieces_pmc_$c.txt 2>/dev/null
done
(python3 $R/tools/pieces_step.py gathered 30 --sites; python3 $R/tools/pieces_step.py tables 30 --sites; python3 $R/tools/pieces_step.py resident 30 --sites) 2>/dev/null > $O/pieces_sites.txt
rm -rf $O/kt $O/kte $O/ktp $O/pmcp_FETCH_SIZE $O/pmcp_WRITE_SIZE $O/pmc_fetch $O/pmc_write $O/pmc_mfma
# micro-benchmarks behind the gate kernels: what a CU takes into LDS from cache-resident panels; where a k-step of gemm_p3 goes
(cd $R && timeout 300 tools/micro/l2_lds_intake.bin > $O/l2_lds_intake.txt 2>&1; timeout 120 tools/micro/p3_bench.bin > $O/p3_bench.txt 2>&1)
# the layer-1 kernels stand-alone: exactness against a naive kernel, k-loop ablations, cycle stamps of the two wave groups' half-steps
(cd $R && timeout 300 tools/micro/p2_bench.bin 7097 20 2>&1 | grep -v "^  *[0-9]*: *[0-9.]* *[0-9.]*  xcc" > $O/p2_bench.txt)
# a register-path loader measured on the forward (fp32 rows split in LDS by the loader waves); the single-pass forward's bounds at T = 32
(cd $R && timeout 200 tools/micro/p2x_bench.bin 7221 > $O/p2x_bench.txt 2>&1; timeout 200 tools/micro/p2o_bench.bin 14000 64 > $O/p2o_bench.txt 2>&1)
# --- the rest is supporting material ---
cd $R
if [ "${LIREC_PROFILES_QUICK:-0}" != "1" ]; then
  # (three passes of the whole GPU suite in ONE session: a cross-stream dependency that holds by timing only shows up as a
  #  box- and run-dependent bit-identity failure -- HISTORY round 5)
  for pass in 1 2 3; do
    timeout 2400 python3 -m pytest tests -m gpu -q > $O/pytest_$pass.log 2>&1; echo "pytest pass $pass rc=$?"; tail -2 $O/pytest_$pass.log
  done
  cp $O/pytest_3.log $O/pytest.log
  python3 tools/parity_summary.py gpurun_out/parity_errors.json $O/parity_errors.json
  (python3 tools/ablate_planes.py; ABL_PDROP=0 python3 tools/ablate_planes.py) 2>/dev/null > $O/ablate_planes.txt
  bash tools/calib_fetch.sh > /dev/null 2>&1; cat gpurun_out/calib/fetch.txt gpurun_out/calib/rdreq.txt 2>/dev/null | grep -v "at::native::(anonymous\|FillFunc" > $O/calib_fetch.txt
  bash tools/ab_bench.sh "--launch recorded" "--launch eager" > $O/launch_modes.txt 2>&1
  for l in recorded eager; do
    LIREC_BENCH_FORCE_DP=1 python3 bench.py $Q --batch-sweep "" --launch $l 2>/dev/null | tail -1 | python3 -c "
import json,sys
d=json.loads(sys.stdin.read()); print('one-rank RCCL data-parallel path, %-9s %9.1f clips/s  %.3f ms  host %.3f ms' % (sys.argv[1], d['value'], d['ms_per_step'], d['host_enqueue_ms_per_step']))" $l >> $O/launch_modes.txt
  done
  bash tools/ab_fetch.sh "--ablate 768" "--ablate 0" > $O/tile_order_fetch.txt 2>&1
  bash tools/ab_sites.sh "--ablate 768" "--ablate 0" >> $O/tile_order_fetch.txt 2>&1
  bash tools/trace_step.sh trace_step --launch recorded --no-strict --no-eval > /dev/null 2>&1; cp gpurun_out/trace_step/trace.csv $O/step_trace.csv 2>/dev/null
  (for a in "0 host" "2 host" "0 resident" "1 resident"; do echo "training() over PiecesDataset, loader threads / feed: $a"; python3 tools/profile_training.py $a 2>/dev/null | grep "clips/s" | tail -3; done) > $O/training_entry.txt
  python3 tools/mode3_sites.py 2>/dev/null | cut -c1-400 > $O/mode3_sites.txt
  cp gpurun_out/trajectory_*.json gpurun_out/onepass_*.json $O/ 2>/dev/null
fi
ls -la $O
