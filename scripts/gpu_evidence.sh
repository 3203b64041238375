#!/bin/bash
# Round evidence on one GPU: the GPU test suite, the full bench line (--full),
# the rocprofv3 kernel-trace summary of the plain command, and the PMC traffic
# passes.  Logs go to $EVIDENCE_DIR (default: evidence/ in the repository).
#   bash scripts/gpu_evidence.sh TAG
set -o pipefail
R="${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}"
TAG=${1:-r01}
cd "$R"
O="${EVIDENCE_DIR:-evidence}"
mkdir -p "$O"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread \
    > "$O/tests_$TAG.log" 2>&1 || { tail -40 "$O/tests_$TAG.log"; exit 1; }
tail -3 "$O/tests_$TAG.log"
timeout -k 10 600 python bench.py --full > "$O/bench_$TAG.log" 2>&1 || { cat "$O/bench_$TAG.log"; exit 1; }
grep '^{' "$O/bench_$TAG.log"
bash scripts/prof_bench.sh > "$O/prof_$TAG.log" 2>&1 || { tail -20 "$O/prof_$TAG.log"; exit 1; }
STEPS=30 bash scripts/pmc_run.sh 256 $TAG > "$O/pmc_$TAG.log" 2>&1 || { tail -20 "$O/pmc_$TAG.log"; exit 1; }
tail -1 "$O/pmc_$TAG.log"
