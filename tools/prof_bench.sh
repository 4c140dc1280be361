#!/bin/bash
# usage (on an MI355X): tools/prof_bench.sh <out dir> [bench args...]  -> rocprofv3 kernel trace of bench.py --full + top-kernel table
out="$1"; shift
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p "$out"
rocprofv3 --kernel-trace -d "$out" -o sd -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-graph "$@" > "$out/bench.log" 2>&1
python tools/rocpd_stats.py "$out/sd_results.db" | head -${TOPN:-24} | cut -c1-140
