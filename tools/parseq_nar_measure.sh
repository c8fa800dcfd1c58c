#!/bin/bash
# The three lines/s measurements of profiles/parseq_nar_lines_per_s.json plus the kernel trace of the new mode: every GPU step
# is a fresh process under its own time limit, chained so that a failing step ends the script.
#   tools/parseq_nar_measure.sh PARENT_TREE OUT_DIR      (PARENT_TREE: a built checkout of the parent commit)
set -o pipefail
parent=${1:?parent tree}
out=${2:?output directory}
mkdir -p "$out"
timeout -k 10 240 python tools/parseq_nar_lines_per_s.py --decode-ar 1 --tree "$parent" --out "$out/parent_ar.json" &&
timeout -k 10 240 python tools/parseq_nar_lines_per_s.py --decode-ar 1 --out "$out/new_ar.json" &&
timeout -k 10 240 python tools/parseq_nar_lines_per_s.py --decode-ar 0 --out "$out/new_nar.json" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$out/trace" -o nar -- python tools/parseq_nar_lines_per_s.py --decode-ar 0 --repeats 1 > "$out/trace.log" 2>&1 &&
grep -h -E "k_nar_cross_attn" "$out"/trace/*kernel_stats.csv "$out"/trace/*/*kernel_stats.csv 2>/dev/null | head -4
