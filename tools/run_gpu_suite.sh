#!/bin/bash
# Full evidence run on the GPU box (round 5): parity tests + report, bench lines (headline with same-run PMC traffic,
# config1, trained-like, batched views, operator path, config3/4), rocprofv3 kernel stats + launch gaps, SQ counters.
#   gpurun --timeout 3000 -- 'bash tools/run_gpu_suite.sh'
# Everything lands in gpurun_out/ev/; copy what should be judged into profiles/ (tools/collect_profiles.py).
R=${GRAFT_REPO_ROOT:-/root/repo}
O=$R/gpurun_out/ev
rm -rf $O; mkdir -p $O
cd $R
F='^RCCL\|^HIP\|^ROCm\|^Hostname\|^Librccl'
rm -f $R/gpurun_out/parity_report.jsonl
timeout 1500 python -m pytest tests -m gpu -q --tb=short 2>&1 | grep -v "$F" | tail -15 > $O/pytest_gpu.log
cp $R/gpurun_out/parity_report.jsonl $O/parity_report.jsonl 2>/dev/null
( time timeout 900 python bench.py --full ) 2>$O/bench_default.err | tail -1 > $O/bench_default.json
timeout 600 python bench.py --full --config config1 --no-extra 2>/dev/null | tail -1 > $O/bench_config1.json
timeout 600 python bench.py --full --config config2 --init-opacity --no-cpu-baseline --no-extra 2>/dev/null | tail -1 > $O/bench_config2_init_opacity.json
for c in config3 config4; do
  timeout 900 python bench.py --full --config $c --no-cpu-baseline --no-extra 2>/dev/null | tail -1 > $O/bench_${c}.json
  timeout 600 python bench.py --full --config $c --init-opacity --no-cpu-baseline --no-traffic --no-extra 2>/dev/null | tail -1 > $O/bench_${c}_init_opacity.json
done
tools/microbench/issue_rates > $O/issue_rates.txt 2>&1
EG_FWD_PROF=1 python tools/fwd_prof.py config2 --spread 2>/dev/null | grep -v "^RCCL\|^HIP\|amdgpu.ids" > $O/fwd_wave_phases_config2.txt
EG_FWD_PROF=1 python tools/fwd_prof.py config2 2>/dev/null | grep -v "^RCCL\|^HIP\|amdgpu.ids" >> $O/fwd_wave_phases_config2.txt
EG_FWD_PROF=1 python tools/fwd_prof.py config4 --spread 2>/dev/null | grep -v "^RCCL\|^HIP\|amdgpu.ids" > $O/fwd_wave_phases_config4.txt
for S in 1 2 4 8; do timeout 300 python bench.py --config config1 --scenes-per-gpu $S 2>/dev/null | tail -1 > $O/bench_config1_scenes$S.json; done
timeout 300 python bench.py --config config1 --scenes-per-gpu 8 --scenes-driver threads 2>/dev/null | tail -1 > $O/bench_config1_scenes8_threads.json
timeout 300 python bench.py --config config2 --scenes-per-gpu 4 2>/dev/null | tail -1 > $O/bench_config2_scenes4.json
timeout 300 python bench.py --full --force-dp --no-cpu-baseline --no-traffic --no-extra 2>/dev/null | tail -1 > $O/bench_config2_force_dp.json
timeout 300 python tools/bench_regularizers.py 2>/dev/null | tail -1 > $O/regularizers_timing.json
timeout 300 python tools/operator_profile.py config2 2>/dev/null | grep -v "^RCCL\|^HIP\|amdgpu.ids" > $O/operator_profile_config2.txt
( echo "--- with edgegaussians_amd.optim.Adam ---"; timeout 300 python tools/operator_profile.py config2 native 2>/dev/null | grep -v "^RCCL\|^HIP\|amdgpu.ids" ) >> $O/operator_profile_config2.txt
for a in torch native; do timeout 300 python bench.py --path operator --operator-adam $a --no-cpu-baseline --no-traffic --no-extra 2>/dev/null | tail -1 > $O/bench_config2_operator_${a}_adam.json; done
timeout 300 python tools/late_epoch_bench.py 2>/dev/null | grep -v "^RCCL\|^HIP\|amdgpu.ids" > $O/late_epoch_bench.txt
timeout 300 python tools/train_abc_fixture.py 2>/dev/null | tail -5 > $O/train_abc_fixture.txt
( echo "--- first run of the process (--cold) ---"; timeout 300 python tools/train_abc_fixture.py --cold 2>/dev/null | tail -2 | head -1 ) >> $O/train_abc_fixture.txt
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/ev_roctx
timeout 300 rocprofv3 --kernel-trace --marker-trace --stats -d /tmp/ev_roctx -o r -- python $R/bench.py --config config2 --roctx --steps 100 --warmup 10 --profile-only > /dev/null 2>$O/prof_roctx.err
python $R/tools/roctx_summary.py /tmp/ev_roctx/r_results.db $O/roctx_ranges_config2.txt > /dev/null 2>&1
for c in config1 config2 config2i config3 config4; do
  rm -rf /tmp/ev_$c /tmp/evsq_$c
  a="--config $c"; [ $c = config2i ] && a="--config config2 --init-opacity"
  timeout 300 rocprofv3 --kernel-trace --stats -d /tmp/ev_$c -o r -- python $R/bench.py $a --steps 300 --warmup 20 --profile-only > /dev/null 2>$O/prof_$c.err
  python $R/tools/rocpd_summary.py /tmp/ev_$c/r_results.db $O/kernel_stats_$c.txt > /dev/null
  python $R/tools/timeline_gaps.py /tmp/ev_$c/r_results.db > $O/timeline_gaps_$c.txt
  timeout 300 rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_WAIT_ANY SQ_WAIT_INST_ANY -d /tmp/evsq_$c -o q -- python $R/bench.py $a --steps 40 --warmup 5 --profile-only > /dev/null 2>$O/sq_$c.err
  python $R/tools/pmc_sq_summary.py $O/sq_counters_$c.txt /tmp/evsq_$c/q_results.db > /dev/null
done
cd $R
tail -4 $O/pytest_gpu.log; head -c 700 $O/bench_default.json; echo; cat $O/bench_default.err | tail -4; head -9 $O/kernel_stats_config2.txt; cat $O/sq_counters_config2.txt | head -8
