#!/bin/bash
# On-box validation bundle for an MI355X machine: the GPU test tier, the
# smoke run and the full benchmark (headline figure plus the secondary
# mm/staging runs).  Writes logs under the directory given as $1
# (default: validate_out/).  Stops at the first step that fails, so
# nothing more is started on a GPU that a previous step left in trouble.
set -x
out="${1:-validate_out}"
mkdir -p "$out"
export HSA_ENABLE_IPC_MODE_LEGACY=0
timeout -k 10 900 python -m pytest tests -x -q -m gpu > "$out/pytest_gpu.log" 2>&1
rc=$?; echo "pytest rc=$rc"; tail -n 2 "$out/pytest_gpu.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python __graft_entry__.py smoke > "$out/smoke.log" 2>&1
rc=$?; echo "smoke rc=$rc"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full > "$out/bench_default.log" 2>&1
rc=$?; echo "default rc=$rc"; [ $rc -eq 0 ] || exit $rc
grep -h metric "$out/bench_default.log"
