# Final per-round evidence: kernel stats + HBM traffic passes + bench line (--full).
R=$(cd "$(dirname "$0")/.." && pwd); O=$R/${TRIAGE_OUT:-triage_out}/final
cd /tmp && export TMPDIR=/tmp
mkdir -p $O
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -o s -- python $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-nms --no-infer > $O/stats_bench.log 2>&1
timeout 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/fetch -o f -- python $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-nms --no-infer > /dev/null 2>&1
timeout 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/write -o w -- python $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-nms --no-infer > /dev/null 2>&1
cd $R && timeout 600 python bench.py --full > $O/bench.json 2> $O/bench.err
tail -c 600 $O/bench.json
ls $O $O/stats $O/fetch $O/write
