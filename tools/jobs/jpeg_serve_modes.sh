#!/bin/bash
# The encoder's modes through serve(jpeg="high", ...) (tools/jpeg_serve_timing.py, leg (b)) -> profiles/jpeg_serve_modes.json:
# the default, 4:2:2, 4:4:4, grey="auto" on colour pages (what the test costs), grey="auto" on grey-valued pages, and the default
# on grey-valued pages next to that.  Run from the repository root on the GPU host, after the library has been built; every step
# under its own time limit, nothing after a failure.
#   $1  output file (default profiles/jpeg_serve_modes.json)
#   $2  a built checkout of the commit before the modes (optional): the default leg is then measured there three times, with
#       this tool copied in - the spread the default leg of this tree has to sit in
set -o pipefail
OUT=${1:-profiles/jpeg_serve_modes.json}
PARENT=${2:-}
TMP=$(mktemp -d) || exit 1
run() {  # name, then the tool's options
  local name=$1
  shift
  timeout -k 10 240 python tools/jpeg_serve_timing.py --legs b --presets high --reps 3 --wave 16 --out "$TMP/$name.json" "$@" > /dev/null || exit 1
  echo "$name: done"
}
run default
run 422 --subsampling 4:2:2
run 444 --subsampling 4:4:4
run auto_on_colour_pages --grey auto
run auto_on_grey_pages --grey auto --grey-pages
run default_on_grey_pages --grey-pages
if [ -n "$PARENT" ]; then
  cp tools/jpeg_serve_timing.py "$PARENT/tools/jpeg_serve_timing.py" || exit 1
  for k in 1 2 3; do
    (cd "$PARENT" && timeout -k 10 240 python tools/jpeg_serve_timing.py --legs b --presets high --reps 3 --wave 16 --out "$TMP/parent_$k.json" > /dev/null) || exit 1
    echo "parent_$k: done"
  done
fi
python - "$TMP" "$OUT" <<'PY'
import glob, json, os, sys
tmp, out = sys.argv[1:3]
keep = ("pages_per_s_device_jpeg", "pages_per_s_device_jpeg_median", "device_ms_per_wave", "bytes_per_page_device", "bytes_per_page_pillow")
merged = {}
for path in sorted(glob.glob(os.path.join(tmp, "*.json"))):
    run = json.load(open(path))
    merged.setdefault("device", run["device"])
    merged.setdefault("job", {k: run[k] for k in ("pages", "wave", "reps")})
    entry = {k: run["presets"]["high"][k] for k in keep}
    entry.update({k: run[k] for k in ("subsampling", "grey", "grey_pages") if k in run})
    merged[os.path.basename(path)[:-5]] = entry
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    f.write(json.dumps(merged, indent=1) + "\n")
print(json.dumps(merged, indent=1))
PY
