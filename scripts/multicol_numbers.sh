#!/bin/bash
# The measurements behind BASELINE.md "Several value columns", in one session
# on one machine: count/min/max/avg over 1 column, spread over 2 and over 4
# columns of ONE op, then the same columns through 2, 3 and 4 single-column
# ops pushed back to back (what a user had to do before). Each step is its
# own process under its own time limit; the chain stops at the first step
# that fails. One JSON line per step, also appended to the file given as $1.
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:-/dev/null}
step() {
    timeout -k 10 "$1" python scripts/multicol_numbers.py "${@:2}" | tee -a "$OUT"
}
step 180 --mode multi --cols 1 &&
step 180 --mode multi --cols 2 &&
step 180 --mode multi --cols 4 &&
step 180 --mode split --cols 2 &&
step 180 --mode split --cols 3 &&
step 180 --mode split --cols 4
