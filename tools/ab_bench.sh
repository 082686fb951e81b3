#!/bin/bash
# A/B of experiment builds against the default library, alternating, REPS times (run on the GPU box from the repo root):
#     OUT=<log dir> bash tools/ab_bench.sh "<bench.py flags>" REPS libA.so libB.so ...      (libraries under manga-ocr_amd/manga_ocr/_lib/)
# writes $OUT/ab_<name><rep>.log (OUT defaults to ab_out), one bench --full JSON line each ("def" = the default library).
FLAGS=$1; REPS=$2; shift 2
L=$PWD/manga-ocr_amd/manga_ocr/_lib
OUT=${OUT:-ab_out}
mkdir -p "$OUT"
for i in $(seq 1 "$REPS"); do
    timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-config4 $FLAGS > "$OUT/ab_def$i.log" 2>&1 || exit 1
    for lib in "$@"; do
        n=$(basename "$lib" .so)
        MOCR_LIB=$L/$lib timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-config4 $FLAGS > "$OUT/ab_$n$i.log" 2>&1 || exit 1
    done
done
