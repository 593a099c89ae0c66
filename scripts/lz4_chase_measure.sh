#!/bin/bash
# The LZ4 chase against the prefix decode of the commit it is compared with
# (DESIGN 12h).  PARENT: a built checkout of that commit; OUT: where the raw
# files go.  The legs alternate, twice each, so that the run-to-run spread of
# either shows beside the difference between them; every GPU step runs under
# its own time limit and the chain stops at the first one that fails.
#   PARENT=/path/to/parent/checkout OUT=profiles/lz4_chase scripts/lz4_chase_measure.sh
set -o pipefail
HERE="$(cd "$(dirname "$0")/.." && pwd)"
PARENT="${PARENT:?a built checkout of the commit to compare against}"
OUT="${OUT:-$HERE/profiles/lz4_chase}"
mkdir -p "$OUT"
cd "$HERE" &&
timeout -k 10 240 python scripts/lz4_chase_rate.py --leg prefix --tree "$PARENT" --out "$OUT/prefix_parent_run1.json" &&
timeout -k 10 240 python scripts/lz4_chase_rate.py --leg chase --out "$OUT/chase_run1.json" &&
timeout -k 10 240 python scripts/lz4_chase_rate.py --leg prefix --tree "$PARENT" --out "$OUT/prefix_parent_run2.json" &&
timeout -k 10 240 python scripts/lz4_chase_rate.py --leg chase --out "$OUT/chase_run2.json"
