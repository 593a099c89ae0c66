#!/bin/bash
# the full bench with and without lone-block byte pieces: the one-call lone legs inside the bench process
cd "$(dirname "$0")/.."; export TMPDIR=/tmp O=${O:-/tmp/bp3}; mkdir -p "$O"
for n in 4 0; do
  JFS_BYTE_PIECES=$n timeout -k 10 900 python bench.py --full > "$O/bp3_$n.json" 2> "$O/bp3_$n.err" || exit 1
  python - "$n" "$O" <<'PY'
import json, sys
n, o = sys.argv[1:3]
d = json.loads([l for l in open(f"{o}/bp3_{n}.json") if l.startswith("{")][-1])["summary"]
print("pieces", n, "lz4 lone", d["oneshot_lz4"]["dec_lone_p50_ms"], "zstd lone", d["oneshot_zstd"]["dec_lone_p50_ms"], "py200", d["oneshot_lz4"]["dec200_GiBs"], "native200", d["oneshot_lz4"]["dec200_native_GiBs"])
PY
done
