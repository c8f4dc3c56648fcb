#!/bin/bash
# The measurements behind BASELINE.md "Intern: int64 keys", in one session on
# one machine: intern ms per launch (int64 and utf8, 10 k and 1 M keys, 8 M-row
# batches), then step-level rows/s of the cfg3 tumbling shape (1 M keys,
# 10 k rows/ms) with dense ids and with int64 keys (and, for scale, utf8 keys)
# interned in the timed region. Each step is its own process under its own time limit; the chain
# stops at the first step that fails. One JSON line per step, also appended
# to the file given as $1.
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:-/dev/null}
step() {
    timeout -k 10 "$1" python scripts/intern_numbers.py "${@:2}" | tee -a "$OUT"
}
step 240 --mode kernel --kind i64 --keys 10000 &&
step 240 --mode kernel --kind utf8 --keys 10000 &&
step 240 --mode kernel --kind i64 --keys 1000000 &&
step 240 --mode kernel --kind utf8 --keys 1000000 &&
step 240 --mode step --kind dense --keys 1000000 --steps 24 &&
step 240 --mode step --kind i64 --keys 1000000 --steps 24 &&
step 240 --mode step --kind utf8 --keys 1000000 --steps 24
