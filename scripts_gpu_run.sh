#!/bin/bash
# usage: [NL_OUT_DIR=dir] scripts_gpu_run.sh [pytest] [smoke] [bench] [prof]  -- helper run on the GPU machine; logs go to NL_OUT_DIR (run_out/)
ulimit -c 0
export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT" || exit 1
O=${NL_OUT_DIR:-run_out}; mkdir -p "$O"
for what in "$@"; do
  case $what in
    pytest) (timeout 600 python -m pytest tests -m gpu -x -q 2>&1 | tail -15) > "$O/pytest_gpu.log"; cat "$O/pytest_gpu.log";;
    smoke) (timeout 120 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -3) > "$O/smoke.log"; cat "$O/smoke.log";;
    bench) (timeout 600 python bench.py --full 2>&1 | tail -3) > "$O/bench.log"; cat "$O/bench.log";;
    prof) rm -rf "$O/prof"; mkdir -p "$O/prof"
          # headline workload only (--no-secondary skips big and the side configs); big gets its own pass
          NL_NO_GRAPH=1 timeout 250 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof" -o nano -- python3 bench.py --steps 256 --warmup 32 --full --no-cpu-baseline --no-secondary > "$O/bench_prof.log" 2>&1 < /dev/null
          NL_NO_GRAPH=1 timeout 250 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof" -o big -- python3 bench.py --workload big:q4_0 --steps 64 --warmup 8 --no-cpu-baseline > "$O/bench_prof_big.log" 2>&1 < /dev/null
          grep '^{' "$O/bench_prof.log" | tail -1 | cut -c1-300
          for f in "$O/prof/nano_kernel_stats.csv" "$O/prof/big_kernel_stats.csv"; do [ -f "$f" ] && head -12 "$f" | cut -c1-150; done
          rm -f "$O"/prof/*kernel_trace.csv "$O"/prof/*/*kernel_trace.csv;;
  esac
done
