# tools/gpu_evidence.sh -- the evidence session of a round on ONE box, on the FINAL build: parity tests, smoke, the default bench line (as the
# driver runs it) and its in-order twin, the torchrun 1-rank RCCL path, rocprofv3 kernel-trace stats of every workload the line reports, and PMC
# passes for EVERY one of them (SQ counters + GRBM_GUI_ACTIVE, FETCH_SIZE and WRITE_SIZE in passes of their own, every launch a full batch).
# tools/collect_profiles.py copies the summaries into profiles/<tag>_* and stamps them with the library's source hash (bench.py refuses
# counters of another build).   usage: bash tools/gpu_evidence.sh r6
TAG=${1:-r6}
mkdir -p gpurun_out
export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
(timeout 900 python -m pytest tests -m gpu -q -s > gpurun_out/pytest_gpu.log 2>&1; echo "pytest rc=$?" >> gpurun_out/pytest_gpu.log)
(timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > gpurun_out/smoke.log 2>&1; echo "smoke rc=$?" >> gpurun_out/smoke.log)
rm -rf gpurun_out/prof_* gpurun_out/pmc_*
PROF="--no-cpu-baseline --no-extra --no-single --min-seconds 0 --settle-seconds 0 --steps 8 --warmup 2"
TRACE="--no-cpu-baseline --no-extra --no-single --min-seconds 0 --settle-seconds 0 --steps 40 --warmup 5"
for wl in cfg2 cfg1 cfg3 cfg4 cfg5; do
  (cd /tmp && timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/gpurun_out/prof_$wl -- python $R/bench.py $TRACE --workload $wl > $R/gpurun_out/rocprof_$wl.log 2>&1)
done
(cd /tmp && timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/gpurun_out/prof_cfg2_nopipe -- python $R/bench.py $TRACE --no-pipeline > $R/gpurun_out/rocprof_cfg2_nopipe.log 2>&1)
(cd /tmp && timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/gpurun_out/prof_cfg4_plain -- python $R/bench.py $TRACE --workload cfg4 --no-topology > $R/gpurun_out/rocprof_cfg4_plain.log 2>&1)
# the distance trace WITH the untimed burns in front of every leg (round 6, VERDICT r5 item 3: a cold trace read 0.42 / 0.55 where the line says 0.52 / 0.68;
# the burns are a few thousand warm launches of the same kernels, so the per-kernel averages of the stats file are the warm figures; the log holds the line of THIS
# pass with the shader clock of every leg beside its roofline fraction)
(cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $R/gpurun_out/prof_dist -- python $R/bench.py --workload dist --no-cpu-baseline --steps 40 --warmup 5 > $R/gpurun_out/rocprof_dist.log 2>&1)
pmc() { name=$1; wl=$2; shift; shift; (cd /tmp && timeout 300 rocprofv3 --kernel-trace --pmc "$@" --output-format csv -d $R/gpurun_out/pmc_${wl}_$name -- python $R/bench.py $PROF --workload $wl $PMC_EXTRA > $R/gpurun_out/pmc_${wl}_$name.log 2>&1); }
SQ1="SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAVES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAIT_INST_LDS GRBM_GUI_ACTIVE"
SQ2="SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_VMEM SQ_ACTIVE_INST_SCA SQ_IFETCH"
for wl in cfg2 cfg1 cfg3 cfg4 cfg5; do
  PMC_EXTRA=""
  pmc sq1 $wl $SQ1
  pmc fetch $wl FETCH_SIZE
  pmc write $wl WRITE_SIZE
done
PMC_EXTRA=""
pmc sq2 cfg2 $SQ2
PMC_EXTRA="--no-pipeline"
pmc nopipe_fetch cfg2 FETCH_SIZE
pmc nopipe_write cfg2 WRITE_SIZE
pmc nopipe_sq1 cfg2 $SQ1
# the distance leg: one kernel variant per pass (MKAMD_DIST_ONLY), SQ + waits + traffic
dpmc() { name=$1; mode=$2; shift; shift; (cd /tmp && MKAMD_DIST_ONLY=$mode timeout 300 rocprofv3 --kernel-trace --pmc "$@" --output-format csv -d $R/gpurun_out/pmc_dist_${mode}_$name -- python $R/bench.py --workload dist --no-cpu-baseline --settle-seconds 0 --steps 8 --warmup 2 > $R/gpurun_out/pmc_dist_${mode}_$name.log 2>&1); }
for mode in periodic nonperiodic; do
  dpmc sq1 $mode $SQ1
  dpmc fetch $mode FETCH_SIZE
  dpmc write $mode WRITE_SIZE
done
# the group-reduction leg alone (k_dist_reduction_closest, periodic, the default block): a trace WITH its burn -- every launch of the pass is the same call, so the
# stats file's average is the leg's kernel time -- and SQ counters in two passes
(cd /tmp && MKAMD_DIST_ONLY=reduction timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/gpurun_out/prof_reduction -- python $R/bench.py --workload dist --no-cpu-baseline --steps 40 --warmup 5 > $R/gpurun_out/rocprof_reduction.log 2>&1)
rpmc() { name=$1; shift; (cd /tmp && MKAMD_DIST_ONLY=reduction timeout 300 rocprofv3 --kernel-trace --pmc "$@" --output-format csv -d $R/gpurun_out/pmc_reduction_$name -- python $R/bench.py --workload dist --no-cpu-baseline --settle-seconds 0 --steps 4 --warmup 1 > $R/gpurun_out/pmc_reduction_$name.log 2>&1); }
rpmc sq1 $SQ1
rpmc sq2 $SQ2
# the one-molecule call: latencies, the host side of the drop-in call, and the gated HIP-graph experiment
(timeout 300 python tools/graph_latency.py > gpurun_out/graph_latency.txt 2>&1)
(for i in 1 2 3; do timeout 120 python tools/single_latency.py; done > gpurun_out/single_latency.txt 2>&1)
(timeout 200 python tools/dropin_profile.py > gpurun_out/dropin_profile.txt 2>&1)
# dist_trajectory at the shapes the projections call it with, under every kernel choice
(timeout 300 python tools/dist_shapes_probe.py > gpurun_out/dist_shapes_probe.txt 2>&1)
# random parity sweeps on this build: the voxelizer (automatic mode and the workgroup-per-item kernel) and dist_trajectory
(timeout 600 python tests/sweep_gpu_random.py 9000 600; MKAMD_TILE_ITEMS=1 timeout 300 python tests/sweep_gpu_random.py 9600 200; timeout 600 python tests/sweep_gpu_dist.py 0 600; timeout 600 python tests/sweep_gpu_reduction.py 0 600; timeout 600 python tests/sweep_gpu_contacts.py 0 600; timeout 600 python tests/sweep_gpu_topology.py 0 1000) > gpurun_out/random_sweeps.txt 2>&1
# the device XTC decoder: kernels alone per chunk size
(timeout 200 python tools/xtc_gpu_probe.py > gpurun_out/xtc_gpu_probe.txt 2>&1)
(timeout 600 python tools/reduction_probe.py > gpurun_out/reduction_probe.txt 2>&1)
(timeout 600 python tools/reduction_few_probe.py 2>&1 | grep -v amdgpu > gpurun_out/reduction_few_probe.txt)
# topology calls with wide atoms (ions): the split fix-up (k_exact_shells / k_exact_redo) against the in-k_tail form, same process
(timeout 600 python tools/topology_wide_ab.py 2>&1 | grep -v amdgpu > gpurun_out/topology_wide_ab_final.txt)
grep -a "cutoff shell" gpurun_out/pytest_gpu.log | sort -u; tail -3 gpurun_out/pytest_gpu.log; tail -2 gpurun_out/smoke.log
python tools/collect_profiles.py $TAG > /dev/null      # the PMC summaries of THIS build first: the bench lines below then carry roofline.traffic
# the bench lines proper (the default one as the driver runs it, with --full: everything it measures), after the counters so that they can quote them;
# their logs go to bench_logs/, where tools/collect_profiles.py reads them
mkdir -p bench_logs
(timeout 900 python bench.py --gpus 1 --steps 20 --warmup 5 --full > bench_logs/bench_cfg2.log 2>&1; echo "rc=$?" >> bench_logs/bench_cfg2.log)
(timeout 400 python bench.py --full --no-cpu-baseline --no-extra --no-pipeline --min-seconds 1 > bench_logs/bench_cfg2_nopipe.log 2>&1; echo "rc=$?" >> bench_logs/bench_cfg2_nopipe.log)
# one rank under torchrun: every collective an N-rank run issues runs on RCCL once (bench.py --full: collectives_exercised), RCCL's warnings captured
(NCCL_DEBUG=WARN timeout 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29517 bench.py --gpus 1 --steps 10 --warmup 3 --full --no-cpu-baseline --no-extra --min-seconds 1 > bench_logs/bench_torchrun1.log 2> bench_logs/bench_torchrun1.err; echo "rc=$?" >> bench_logs/bench_torchrun1.log)
(NCCL_DEBUG=WARN timeout 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29519 bench.py --workload dist --gpus 1 --steps 10 --warmup 3 > bench_logs/bench_dist_torchrun1.log 2> bench_logs/bench_dist_torchrun1.err; echo "rc=$?" >> bench_logs/bench_dist_torchrun1.log)
(timeout 400 python bench.py --workload dist --steps 20 --warmup 3 > bench_logs/bench_dist.log 2>&1; echo "rc=$?" >> bench_logs/bench_dist.log)
python tools/collect_profiles.py $TAG
# gpurun merges at most 64 MiB back: the per-launch traces are not needed once the stats / counter tables exist
find gpurun_out -name "*_kernel_trace.csv" -size +1M -delete; du -sh gpurun_out | tail -1
# the summaries as collected HERE travel too (profiles/ itself is not merged back): cp gpurun_out/profiles_out/* profiles/ at home
rm -rf gpurun_out/profiles_out; mkdir -p gpurun_out/profiles_out; cp profiles/${TAG}_* gpurun_out/profiles_out/
if [ $(du -sm gpurun_out | cut -f1) -gt 55 ]; then rm -rf gpurun_out/prof_* gpurun_out/pmc_*; echo "raw rocprofv3 tables dropped (over the merge limit)"; fi
du -sh gpurun_out | tail -1
