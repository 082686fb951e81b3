#!/usr/bin/env python3
"""What the run-time target branch of the masked LM-head epilogues costs a batch that has no prefix: HIP-event time per greedy
step of gemm_dec_vocab_m (the engine's own profiler: an instrumented eager pass per repetition) in a constrained, un-prefixed,
scored batch - every row under a random half of the vocabulary.

    python tools/prefix_cost.py [--tree DIR] [--label NAME] [--rows 96,1024] [--max-len 32] [--reps 7]

--tree: the checkout whose package and library are measured (default: this one); pointing it at a checkout of the parent
commit, built, gives the numbers to compare against - measured twice, the parent against itself gives the run-to-run spread.
Prints one JSON line per row count: the median over the repetitions and their min .. max, in microseconds."""
import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this")
    ap.add_argument("--rows", default="96,1024")
    ap.add_argument("--max-len", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    for p in (tree, os.path.join(tree, "manga-ocr_amd")):
        sys.path.insert(0, p)
    import numpy as np
    from manga_ocr.engine import Engine
    from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights

    w = synthetic_weights(0)
    steps = args.max_len - 1
    for rows in [int(r) for r in args.rows.split(",")]:
        eng = Engine(w, DEFAULT_SPEC, dtype="bf16", device=0, max_batch=rows, lanes=1)
        gray = np.random.RandomState(rows).randint(0, 256, size=(rows, 224, 224), dtype=np.uint8)
        half = eng.token_set(np.nonzero(np.random.RandomState(7).rand(DEFAULT_SPEC.vocab) < 0.5)[0])
        call = lambda: eng.recognize_gray(gray, args.max_len, scores=True, token_sets=half)      # noqa: E731
        call()
        call()
        eng.profile_enable(True)
        call()
        head = []
        for _ in range(args.reps):
            eng.profile_reset()
            call()
            st = {s["name"]: s for s in eng.profile_get()}
            s = st["gemm_dec_vocab_m"]
            assert s["launches"] == steps, s
            head.append(1e3 * s["total_ms"] / steps)
        eng.profile_enable(False)
        eng.close()
        print(json.dumps(dict(what="gemm_dec_vocab_m", build=args.label, rows=rows, max_len=args.max_len, reps=args.reps,
                              us_per_step=round(statistics.median(head), 3), spread_us=[round(min(head), 3), round(max(head), 3)])), flush=True)


if __name__ == "__main__":
    main()
