#!/bin/bash
# Round-4 evidence, run on the GPU box from the repo root:  bash profiles/collect_r04.sh [trace|pmc]
#   trace: rocprofv3 --kernel-trace --stats of the default bench command (c4) -> per-kernel summary + prefill timeline
#   pmc:   SEPARATE counter passes on the headline models (70B + 1B, workload c3, 4 steps): FETCH_SIZE, WRITE_SIZE (HBM traffic
#          of the GEMM family) and MfmaUtil / VALUBusy.  PMC passes never carry a trace domain.
# Everything lands in gpurun_out/r04/; the summaries worth judging are copied into profiles/ by hand.
set -u
cd /tmp && export TMPDIR=/tmp
cd "${GRAFT_REPO_ROOT:-/root/repo}"
O=gpurun_out/r04
mkdir -p $O
what="${1:-trace}"
if [ "$what" = "trace" ]; then
  P="--no-cpu-baseline --ttft-samples 6 --ref-seqs 0 --no-roofline"
  timeout 500 rocprofv3 --kernel-trace --stats -d $O/kt_c4 -- python bench.py --full --steps 20 --warmup 3 $P > $O/kt_c4.json 2> /dev/null
  DB="$(ls $O/kt_c4/*/*.db | tail -1)"
  python profiles/kstats.py "$DB" $O/c4_kernel_stats.csv > $O/c4_kernel_stats.txt 2>&1
  python profiles/prefill_timeline.py "$DB" > $O/c4_prefill_timeline.txt 2>&1
  rm -rf $O/kt_c4
else
  Q="--workload c3 --steps 4 --warmup 1 --no-cpu-baseline --no-roofline --ttft-samples 1 --ref-seqs 0"
  for c in FETCH_SIZE WRITE_SIZE "MfmaUtil VALUBusy"; do
    tag=$(echo $c | tr ' ' '_')
    timeout 420 rocprofv3 --pmc $c -d $O/pmc_$tag -- python bench.py --full $Q > /dev/null 2> $O/pmc_$tag.err
    python profiles/pmcstats.py "$(ls $O/pmc_$tag/*/*.db | tail -1)" > $O/pmc_$tag.csv 2>&1
    rm -rf $O/pmc_$tag/
  done
fi
ls -la $O | tail -n 12
