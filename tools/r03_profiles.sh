# Round-3 evidence run (on the GPU box, via gpurun): per config a
# rocprofv3 kernel trace of `bench.py --config <c> --no-g-step` (D-step launches only: the generator-step side
# measurement would mix other shapes into the same kernel names) joined with the bench's own shape table
# (tools/rocpd_rows.py -> one row per (kernel, layer shape) with GFLOP per launch), and the PMC passes (own runs,
# --kernel-trace only beside the counters), then `bench.py --full` (all configs + CPU baselines).  Usage: PMC_CONFIGS="c10_b512 sg2_32 sg2_512" bash tools/r03_profiles.sh [tag]
R=$GRAFT_REPO_ROOT
TAG=${1:-r03}
O=$R/gpurun_out/${TAG}p
rm -rf $O; mkdir -p $O
cd $R
cd /tmp && export TMPDIR=/tmp
for c in ${KT_CONFIGS-c10_b512 sg2_32 sg2_512}; do
  case $c in c10_b512) S="--steps 5 --warmup 3";; sg2_32) S="--steps 5 --warmup 3";; sg2_512) S="--steps 16 --warmup 2";; esac
  timeout 400 rocprofv3 --kernel-trace -d $O -o ${c}_kt -- python $R/bench.py --config $c $S --full --no-cpu-baseline --no-g-step --shape-table $O/${c}_shapes.json > $O/${c}_kt.log 2>&1
  python $R/tools/rocpd_summary.py $O/${c}_kt_results.db > $O/${c}_kernel_trace.txt 2>&1
  python $R/tools/rocpd_rows.py $O/${c}_kt_results.db $O/${c}_shapes.json > $O/${c}_rows.txt 2>&1
  grep -h '^{' $O/${c}_kt.log > $O/${c}_under_rocprof.json
  rm -f $O/${c}_kt_results.db
done
for c in ${PMC_CONFIGS-c10_b512 sg2_32 sg2_512}; do       # PMC_CONFIGS="" skips the counter passes
  case $c in c10_b512) S="--steps 3 --warmup 2";; sg2_32) S="--steps 3 --warmup 2";; sg2_512) S="--steps 2 --warmup 2";; esac
  P=$O/pmc_$c; mkdir -p $P
  B="python $R/bench.py --config $c $S --no-cpu-baseline --no-g-step --graph off"
  timeout 240 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $P -o fetch -- $B > $P/fetch.log 2>&1
  timeout 240 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $P -o write -- $B > $P/write.log 2>&1
  timeout 240 rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_ANY SQ_INSTS_VALU_MFMA_MOPS_F32 -d $P -o sq -- $B > $P/sq.log 2>&1
  timeout 240 rocprofv3 --kernel-trace --pmc GRBM_GUI_ACTIVE SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d $P -o misc -- $B > $P/misc.log 2>&1
  cd $R && python tools/make_pmc_profile.py $P ${TAG}_${c}_n1 "bench.py --config $c $S --no-cpu-baseline --no-g-step --graph off" > $P/summary.txt 2>&1; cd /tmp
  rm -f $P/*.db
done
cd $R
if [ -z "$SKIP_BENCH" ]; then     # after the counter passes: its roofline.traffic then comes from THIS run's PMC summaries
  timeout 900 python bench.py --full > $O/bench_n1.json 2> $O/bench_n1.err; echo "bench rc=$?"
fi
mkdir -p $O/profiles
for c in ${KT_CONFIGS-c10_b512 sg2_32 sg2_512}; do
  cp $O/${c}_kernel_trace.txt $O/profiles/${TAG}_${c}_n1_kernel_trace.txt
  cp $O/${c}_rows.txt $O/profiles/${TAG}_${c}_n1_rows.txt
  cp $O/${c}_shapes.json $O/profiles/${TAG}_${c}_n1_shapes.json
  cp $O/${c}_under_rocprof.json $O/profiles/${TAG}_${c}_n1_under_rocprof.json
done
[ -f $O/bench_n1.json ] && tail -1 $O/bench_n1.json > $O/profiles/${TAG}_bench_n1.json
cp profiles/${TAG}_*_pmc.* $O/profiles/ 2>/dev/null
ls -la $O/profiles; [ -f $O/bench_n1.json ] && head -c 600 $O/bench_n1.json; echo
for c in ${KT_CONFIGS-c10_b512 sg2_32 sg2_512}; do head -30 $O/${c}_rows.txt; done
