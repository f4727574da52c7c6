#!/bin/bash
# Profiles `bench.py` on the GPU box: kernel trace + stats, then PMC passes (each in its own run, no trace
# domains mixed with --pmc).  Three configurations: the bench default (1200x675x500, tag "target"),
# BASELINE configs[1] (1200x675x100, tag "cfg2"), configs[3] (10k spheres, 1920x1080x256, tag "tenk": the large-grid kernel) and
# configs[2] (3840x2160x500, tag "weak": the N = 1 half of the weak-scaling pair, `bench.py --weak-baseline`).  Output under gpurun_out/prof_<tag>/; summaries are copied
# into profiles/ by tools/summarize_profile.py.  Every run has a time limit of its own (LIMIT seconds), and the first run that fails,
# faults or times out ends the script: nothing more is started on the GPU after it.
# CONFIGS="target cfg2" profiles only those tags; SUFFIX=_classic writes to prof_<tag>_classic beside prof_<tag> (e.g. with RTIOW_DENSE_BODY=classic
# in the environment: the same bench on the classic body of the dense kernel, the "before" of a before/after pair).
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
LIMIT=${LIMIT:-300}
run_cfg() {
  TAG=$1; shift
  OUT=gpurun_out/prof_$TAG
  OUT=$OUT$SUFFIX
  rm -rf $OUT; mkdir -p $OUT
  STEPS=5; [ "$TAG" = weak ] && STEPS=2
  ARGS="bench.py --steps $STEPS --warmup 1 --no-cpu-baseline --no-other-configs --no-end-to-end $@"
  echo "$ARGS" > $OUT/command.txt
  timeout -k 10 $LIMIT rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -- python3 $ARGS > $OUT/trace.log 2>&1
  rc=$?; echo "$TAG trace rc=$rc"
  [ $rc -eq 0 ] || { tail -5 $OUT/trace.log; exit 1; }
  i=0
  for pmc in "SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_LDS SQ_INSTS_VMEM" \
             "SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_BF16 SQ_INSTS_BRANCH SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE" \
             "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_INST_CYCLES_SALU SQ_THREAD_CYCLES_VALU SQ_ACTIVE_INST_SCA SQ_WAIT_INST_LDS" \
             "GRBM_GUI_ACTIVE GRBM_COUNT" \
             "FETCH_SIZE" "WRITE_SIZE" \
             "SQ_INSTS_VALU_ADD_F32 SQ_INSTS_VALU_MUL_F32 SQ_INSTS_VALU_FMA_F32 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_TRANS_F32 SQ_INSTS_VALU_INT32"; do
    i=$((i+1))
    timeout -k 10 $LIMIT rocprofv3 --pmc $pmc --output-format csv -d $OUT/pmc$i -- python3 $ARGS > $OUT/pmc$i.log 2>&1
    rc=$?; echo "$TAG pmc$i rc=$rc ($pmc)"
    [ $rc -eq 0 ] || { tail -5 $OUT/pmc$i.log; exit 1; }
  done
}
for c in ${CONFIGS:-target cfg2 tenk weak}; do
  case $c in
    target) run_cfg target ;;
    cfg2) run_cfg cfg2 --width 1200 --height 675 --spp 100 ;;
    tenk) run_cfg tenk --tenk ;;
    weak) run_cfg weak --weak-baseline ;;
    *) echo "unknown configuration $c"; exit 2 ;;
  esac || exit 1
done
