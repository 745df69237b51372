#!/bin/bash
# What the driver runs at round end, on one box (tools/round.sh <rNN> <log dir>): the whole -m gpu suite (-x), smoke(),
# bench.py --full.  -> <log dir>/<rNN>_gpu_tests.txt, <log dir>/<rNN>_bench_stdout.txt
R=${1:-r06}
OUT=${2:?usage: tools/round.sh <rNN> <log dir>}
cd /tmp && export TMPDIR=/tmp; cd ${GRAFT_REPO_ROOT:-/root/repo}
mkdir -p "$OUT"
t0=$(date +%s)
timeout 1700 python -m pytest tests/ -x -q -m gpu --durations=12 > "$OUT/${R}_gpu_tests.txt" 2>&1
echo "pytest rc=$? wall=$(( $(date +%s) - t0 ))s" >> "$OUT/${R}_gpu_tests.txt"
tail -22 "$OUT/${R}_gpu_tests.txt"
python -c "from __graft_entry__ import smoke; smoke()" 2>&1 | tail -2
t0=$(date +%s)
python bench.py --full > "$OUT/${R}_bench_stdout.txt" 2> "$OUT/${R}_bench_stderr.txt"
echo "bench rc=$? wall=$(( $(date +%s) - t0 ))s; stdout bytes $(wc -c < "$OUT/${R}_bench_stdout.txt"); last line bytes $(tail -1 "$OUT/${R}_bench_stdout.txt" | wc -c)"
tail -1 "$OUT/${R}_bench_stdout.txt"
