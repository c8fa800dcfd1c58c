#!/bin/bash
# serve(jpeg=...) next to the host JPEG path and to plain serve (tools/jpeg_serve_timing.py) -> profiles/jpeg_serve.json.
# Then leg (b) next to (o), the optimised Huffman tables -> <output>_optimized.json.
# Run from the repository root on the GPU host, after the library has been built; one step, under its own time limit.
#   $1  output file (default profiles/jpeg_serve.json)
#   $2  a built checkout of the commit before the encoder (optional): legs (c) and (a) are then also measured there, with this
#       tool copied in, -> <output>_parent.json
set -o pipefail
OUT=${1:-profiles/jpeg_serve.json}
PARENT=${2:-}
timeout -k 10 540 python tools/jpeg_serve_timing.py --reps 3 --wave 16 --out "$OUT" || exit 1
timeout -k 10 300 python tools/jpeg_serve_timing.py --optimize --legs b --reps 3 --wave 16 --out "${OUT%.json}_optimized.json" || exit 1
if [ -n "$PARENT" ]; then
  cp tools/jpeg_serve_timing.py "$PARENT/tools/jpeg_serve_timing.py" || exit 1
  (cd "$PARENT" && timeout -k 10 400 python tools/jpeg_serve_timing.py --host-only --reps 3 --wave 16 --out "$OLDPWD/${OUT%.json}_parent.json")
fi
