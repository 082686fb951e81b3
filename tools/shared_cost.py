#!/usr/bin/env python3
"""What shared encodings save a caller who decodes several rows per crop: wall time per call of a bf16 engine for 64 crops x 8
rows each = 512 rows, generate length 32, scored - once with ``sources=`` (the crops encoded once, include/mocr.h "shared
encodings") and once with the crops physically repeated through the entry point that has always existed (the yardstick: 512
planes, 512 encoder rows).  Also prints mocr_encoded_crops per call: 64 against 512.

    python tools/shared_cost.py [--tree DIR] [--label NAME] [--crops 64] [--per-crop 8] [--max-len 32] [--reps 7]

--tree: the checkout whose package and library are measured (default: this one); pointing it at a checkout of the parent
commit, built, measures the repeated form alone (it has no ``sources=``) - run twice, the parent against itself gives the
run-to-run spread of the yardstick.  Prints one JSON line per form: the median over the repetitions after two warm-ups and
their min .. max, in milliseconds."""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this")
    ap.add_argument("--crops", type=int, default=64)
    ap.add_argument("--per-crop", type=int, default=8)
    ap.add_argument("--max-len", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    for p in (tree, os.path.join(tree, "manga-ocr_amd")):
        sys.path.insert(0, p)
    import numpy as np
    from manga_ocr.engine import Engine
    from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights

    rows = args.crops * args.per_crop
    eng = Engine(synthetic_weights(0), DEFAULT_SPEC, dtype="bf16", device=0, max_batch=rows, lanes=1)
    gray = np.random.RandomState(rows).randint(0, 256, size=(args.crops, 224, 224), dtype=np.uint8)
    source = np.arange(rows) % args.crops
    repeated = np.ascontiguousarray(gray[source])
    forms = [("repeated", lambda: eng.recognize_gray(repeated, args.max_len, scores=True))]
    counter = getattr(eng, "encoded_crops", None)
    if counter is not None:      # (the parent commit has neither sources= nor the counter)
        forms.append(("sources", lambda: eng.recognize_gray(gray, args.max_len, scores=True, sources=source)))
    for form, call in forms:
        for _ in range(2):
            call()
        ms, enc = [], []
        for _ in range(args.reps):
            c0 = counter() if counter else 0
            t0 = time.perf_counter()
            call()
            ms.append(1e3 * (time.perf_counter() - t0))
            enc.append(counter() - c0 if counter else None)
        assert len(set(enc)) == 1, enc
        print(json.dumps(dict(what="shared_cost", build=args.label, form=form, crops=args.crops, rows=rows, max_len=args.max_len,
                              reps=args.reps, ms_per_call=round(statistics.median(ms), 3), spread_ms=[round(min(ms), 3), round(max(ms), 3)],
                              encoded_crops=enc[0])), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
