#!/bin/bash
# Writes profiles/channels_rate.txt: the measurements of tools/channels_rate.py on one MI355X, each step a process of its own
# under its own time limit, chained so that a failure ends the run.  The build facts at the head of the file (resource logs
# against the parent's, library size, build time) are not measured here: they are kept from the committed file.
#   bash tools/channels_rate.sh [output file]
set -o pipefail
out=${1:-profiles/channels_rate.txt}
tmp=$(mktemp)
timeout -k 10 300 python tools/channels_rate.py --step kernel --reps 6 | tee -a "$tmp" && echo >> "$tmp" &&
timeout -k 10 300 python tools/channels_rate.py --step device --case C2 --reps 6 | tee -a "$tmp" && echo >> "$tmp" &&
timeout -k 10 300 python tools/channels_rate.py --step device --case C3 --reps 6 | tee -a "$tmp" && echo >> "$tmp" &&
timeout -k 10 540 python tools/channels_rate.py --step file --reps 3 | tee -a "$tmp" || { rc=$?; echo "a step failed ($rc): $out not written" >&2; rm -f "$tmp"; exit $rc; }
if [ -f "$out" ]; then sed -n '/^## Build/,$p' "$out" > "$tmp.build"; fi
cat "$tmp" > "$out.new"
if [ -s "$tmp.build" ]; then { echo; cat "$tmp.build"; } >> "$out.new"; fi
mv "$out.new" "$out"
rm -f "$tmp" "$tmp.build"
