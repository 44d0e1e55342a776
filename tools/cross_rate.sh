#!/bin/bash
# Writes profiles/cross_rate.txt: the measurements of tools/cross_rate.py on one MI355X, each step a process of its own under its
# own time limit, chained so that a failure ends the run.  The text after the measurements (from "## Reading" on: the reading and
# the build facts) is not measured here: it is kept from the committed file.
#   bash tools/cross_rate.sh [output file]
set -o pipefail
out=${1:-profiles/cross_rate.txt}
tmp=$(mktemp)
timeout -k 10 240 python tools/cross_rate.py --step rows --case mtm4096 --reps 6 | tee -a "$tmp" && echo >> "$tmp" &&
timeout -k 10 240 python tools/cross_rate.py --step rows --case mtm4096o75 --reps 6 | tee -a "$tmp" && echo >> "$tmp" &&
timeout -k 10 240 python tools/cross_rate.py --step rows --case mtm1024 --reps 6 | tee -a "$tmp" && echo >> "$tmp" &&
timeout -k 10 240 python tools/cross_rate.py --step batch --reps 6 | tee -a "$tmp" || { rc=$?; echo "a step failed ($rc): $out not written" >&2; rm -f "$tmp"; exit $rc; }
if [ -f "$out" ]; then sed -n '/^## Reading/,$p' "$out" > "$tmp.keep"; fi
cat "$tmp" > "$out.new"
if [ -s "$tmp.keep" ]; then { echo; cat "$tmp.keep"; } >> "$out.new"; fi
mv "$out.new" "$out"
rm -f "$tmp" "$tmp.keep"
