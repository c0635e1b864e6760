#!/bin/bash
# full GPU round trip (tag = $1): gpu parity tests, the full bench (with CPU baseline), kernel-trace profile
# (output under $STZS_OUT, default out/)
tag=${1:-x}
out=${STZS_OUT:-out}
mkdir -p $out
timeout -k 10 500 python -u -m pytest tests/ -x -v -s -m gpu -p no:cacheprovider --timeout 120 --timeout-method thread > $out/t_$tag.log 2>&1
rc=$?; echo TEST $rc; grep -E "passed|failed|FAILED|Error" $out/t_$tag.log | tail -8
[ $rc -ne 0 ] && exit $rc
timeout -k 10 400 python -c "import __graft_entry__ as g; g.smoke()" > $out/smoke_$tag.log 2>&1 || exit $?
tail -1 $out/smoke_$tag.log
timeout -k 10 500 python bench.py --full > $out/bench_$tag.log 2>&1 || exit $?
tail -1 $out/bench_$tag.log
bash tools/prof.sh prof_$tag
python3 tools/roofline_check.py $out/prof_$tag/run_kernel_trace.csv $out/prof_$tag.log > $out/roofline_check_$tag.json && cat $out/roofline_check_$tag.json
[ -n "$PMC" ] && bash tools/pmc_bench.sh $tag
exit 0
