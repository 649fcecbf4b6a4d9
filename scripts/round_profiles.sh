#!/bin/bash
# Everything profiles/rNN_* is regenerated from, in one GPU call (GPU box): kernel-trace summaries of the bench at cfg 2/4/5, the PMC
# traffic passes, and the one-rank RCCL lines.  usage: scripts/round_profiles.sh r03      (outputs under gpurun_out/)
tag=${1:-r05}
cd "$GRAFT_REPO_ROOT"
# The backward picks its row loop by timing both on the live data (functional.row_skip_tuner); a profiler perturbs that timing, so the
# traced and counter runs are pinned (SMD_BWD_SKIP) to what the un-traced bench of the same workload chose.
for wl in cfg2 cfg4 cfg5; do
  skip=$(python bench.py --workload $wl --full --no-cpu-baseline 2>/dev/null | python -c "import json,sys; print(2 if json.loads(sys.stdin.read().strip().splitlines()[-1])['roofline_bwd']['row_loop']['dead_row_skipping'] else 0)")
  echo "$wl: un-traced bench chose SMD_BWD_SKIP=$skip" | tee gpurun_out/row_loop_$wl.txt
  SMD_BWD_SKIP=$skip bash scripts/gpu_profile.sh ${tag}_$wl --workload $wl > gpurun_out/prof_${tag}_$wl.log 2>&1
  grep -m1 '"metric"' gpurun_out/prof_${tag}_$wl/bench.log | cut -c1-200
  SMD_BWD_SKIP=$skip PMC_TIMEOUT=400 bash scripts/pmc_traffic.sh ${tag}_tmp $wl > gpurun_out/pmc_traffic_${tag}_$wl.log 2>&1
  rm -rf gpurun_out/pmc_${tag}_bench_$wl; mv gpurun_out/pmc_${tag}_tmp_bench_$wl gpurun_out/pmc_${tag}_bench_$wl
  if ! grep -q FETCH_SIZE gpurun_out/pmc_${tag}_bench_$wl/summary.txt; then
    # (round 4: under `rocprofv3 --pmc` the bf16 ConvNeXt workload dies inside MIOpen's convolution backward; the loss path alone — same kernels, same
    # shapes, scripts/dev/microbench.py inputs — is counted instead, and the summary says so)
    echo "$wl: counter passes over bench.py failed; counting the loss path alone (scripts/dev/microbench.py $wl)" | tee gpurun_out/pmc_fallback_$wl.txt
    SMD_BWD_SKIP=$skip PMC_TIMEOUT=300 PMC_GROUPS="FETCH_SIZE;WRITE_SIZE;TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum" bash scripts/pmc.sh ${tag}_bench_$wl python $GRAFT_REPO_ROOT/scripts/dev/microbench.py $wl 5 > /dev/null
    sed -i "1i (counter passes over scripts/dev/microbench.py $wl 5: bench.py --workload $wl crashes inside MIOpen under rocprofv3 --pmc)" gpurun_out/pmc_${tag}_bench_$wl/summary.txt
  fi
done
python scripts/make_traffic_json.py $tag cfg2 cfg4 cfg5 > gpurun_out/traffic_$tag.json
tail -5 gpurun_out/traffic_$tag.json
bash scripts/rccl_one_rank.sh $tag
cut -c1-160 gpurun_out/rccl_one_rank_$tag.txt
