#!/bin/bash
# Writes the measurements of tools/ddc_rate.py on one MI355X (profiles/ddc_rate.txt keeps them, with the notes written around them),
# each step a process of its own under its own time limit, chained so that a failure ends the run.
#   bash tools/ddc_rate.sh [output file]
set -o pipefail
out=${1:-profiles/ddc_rate_measured.txt}
tmp=$(mktemp)
for fmt in f32 s16; do
  for case in 16x129 64x513 1x1; do
    timeout -k 10 400 python tools/ddc_rate.py --step ddc --case $case --fmt $fmt --reps 6 | tee -a "$tmp" && echo >> "$tmp" ||
      { rc=$?; echo "a step failed ($rc): $out not written" >&2; rm -f "$tmp"; exit $rc; }
  done
done
timeout -k 10 400 python tools/ddc_rate.py --step zoom --reps 6 | tee -a "$tmp" || { rc=$?; echo "a step failed ($rc): $out not written" >&2; rm -f "$tmp"; exit $rc; }
mv "$tmp" "$out"
