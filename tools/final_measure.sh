# Round-end measurement on the GPU box:  bash tools/final_measure.sh <tag> <output folder>
# everything lands in the output folder (copy what is to be judged into profiles/: tools/publish_profiles.sh, which
# names the folder it copies from in its own first lines)
tag=${1:-final}
R=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
o=$(mkdir -p "${2:?usage: bash tools/final_measure.sh <tag> <output folder>}" && cd "$2" && pwd)
cd $R
python -m pytest tests -m gpu -x -q 2>&1 | tail -4 > $o/${tag}_gputest.log; cat $o/${tag}_gputest.log
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
python tools/pmc_record.py fft ntt ntt_int mb_g3 mb_g4 n1024 ks --tag ${tag} --dir $o > $o/${tag}_pmc.log 2>&1; tail -1 $o/${tag}_pmc.log
# bench.py ties `traffic` to the build through this record: publish it before the bench line is taken
cp $o/pmc_${tag}.json profiles/pmc_latest.json
# the complete line: headline, counter passes, CPU baseline and every datapoint under `extra`
python bench.py --full > $o/${tag}_bench.json 2> $o/${tag}_bench.err; tail -2 $o/${tag}_bench.err; cut -c1-300 $o/${tag}_bench.json
# the multi-rank code path of bench.py at N = 1 (torch.distributed over RCCL, one rank), headline alone
TFHE_BENCH_FORCE_DIST=1 MASTER_ADDR=127.0.0.1 MASTER_PORT=29571 RANK=0 LOCAL_RANK=0 WORLD_SIZE=1 python bench.py --steps 3 > $o/${tag}_bench_dist1.json 2> $o/${tag}_bench_dist1.err; cut -c1-200 $o/${tag}_bench_dist1.json; tail -2 $o/${tag}_bench_dist1.err
# rocprofv3 kernel-trace statistics of the bench command itself
cd /tmp && export TMPDIR=/tmp
rm -rf $o/${tag}_rocprof
# the plain run (headline alone): the average duration of the headline kernel must be that of bench.py's timed launches,
# and the radix datapoint under `extra` launches the same kernel at other batch sizes
rocprofv3 --kernel-trace --stats -d $o/${tag}_rocprof -- python $R/bench.py --steps 5 --warmup 1 > $o/${tag}_rocprof.log 2>&1
rocprofv3 --kernel-trace --stats -d $o/${tag}_rocprof_extra -- python $R/bench.py --steps 5 --warmup 1 --full --no-cpu-baseline --parity-sample 64 > $o/${tag}_rocprof_extra.log 2>&1
cd $R && python tools/rocprof_summary.py $o/${tag}_rocprof $o/${tag}_rocprof_stats.txt | head -14
cd $R && python tools/rocprof_summary.py $o/${tag}_rocprof_extra $o/${tag}_rocprof_extra_stats.txt | head -3
python tools/measure_all.py ks ks32 ks1024 wave n1024 mb mb4 mblat ntt ntt_split sweep > $o/${tag}_measure_all.jsonl 2>&1; cat $o/${tag}_measure_all.jsonl | cut -c1-260
# the multi-GPU form of bench.py on the one GPU of this box (two shards as two streams: logic check, not a scaling number)
TFHE_BENCH_FAKE_MULTI_GPU=1 python bench.py --gpus 2 --steps 3 --full > $o/${tag}_bench_fake2gpu.json 2> $o/${tag}_bench_fake2gpu.err; cut -c1-200 $o/${tag}_bench_fake2gpu.json
# the scaling sweep's form of the command (headline only): eight shards, must stay under two minutes of wall time
( time TFHE_BENCH_FAKE_MULTI_GPU=1 python bench.py --gpus 8 --steps 3 --scale-quick > $o/${tag}_bench_fake8gpu_scale_quick.json 2> $o/${tag}_bench_fake8gpu_scale_quick.err ) 2>&1 | grep real; cut -c1-300 $o/${tag}_bench_fake8gpu_scale_quick.json
# ... and eight shards (the driver's largest N): 8 streams of the one GPU, config 5 through both shardings
TFHE_BENCH_FAKE_MULTI_GPU=1 python bench.py --gpus 8 --steps 2 --full > $o/${tag}_bench_fake8gpu.json 2> $o/${tag}_bench_fake8gpu.err; cut -c1-200 $o/${tag}_bench_fake8gpu.json; tail -2 $o/${tag}_bench_fake8gpu.err
python tools/latency_integer.py classic > $o/${tag}_latency_integer.jsonl 2>&1; python tools/latency_integer.py multibit_g4 >> $o/${tag}_latency_integer.jsonl 2>&1; cut -c1-200 $o/${tag}_latency_integer.jsonl
