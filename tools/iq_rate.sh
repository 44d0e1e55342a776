#!/bin/bash
# Writes profiles/iq_rate.txt: the measurements of tools/iq_rate.py on one MI355X, each step a process of its own under its own
# time limit, chained so that a failure ends the run.  The build facts at the end of the file (resource logs against the
# parent's, library size, build time) are not measured here: they are kept from the committed file.
#   bash tools/iq_rate.sh [output file]
set -o pipefail
out=${1:-profiles/iq_rate.txt}
tmp=$(mktemp)
timeout -k 10 240 python tools/iq_rate.py --step rows --case fft4096 --reps 6 | tee -a "$tmp" && echo >> "$tmp" &&
timeout -k 10 240 python tools/iq_rate.py --step rows --case mtm4096 --reps 6 | tee -a "$tmp" && echo >> "$tmp" &&
timeout -k 10 240 python tools/iq_rate.py --step rows --case fft1024 --reps 6 | tee -a "$tmp" && echo >> "$tmp" &&
timeout -k 10 240 python tools/iq_rate.py --step batch --reps 6 | tee -a "$tmp" || { rc=$?; echo "a step failed ($rc): $out not written" >&2; rm -f "$tmp"; exit $rc; }
if [ -f "$out" ]; then sed -n '/^## Build/,$p' "$out" > "$tmp.build"; fi
cat "$tmp" > "$out.new"
if [ -s "$tmp.build" ]; then { echo; cat "$tmp.build"; } >> "$out.new"; fi
mv "$out.new" "$out"
rm -f "$tmp" "$tmp.build"
