#!/usr/bin/env python3
"""What the token scores cost: HIP-event time per greedy step of the LM head + token kernel, and of the whole decode step,
unscored, scored and scored with token alternatives, each also under token constraints (every row a random half of the vocabulary) and with no-repeat n-grams (n = 3 on every row, whole vocabulary: per-row masks instead of the shared table, rebuilt by the token kernel), for isolated batches (the engine's own profiler: an instrumented eager pass per repetition).

    python tools/score_cost.py [--rows 64,2560] [--max-len 64] [--reps 5] [--unscored-only | --no-alternatives] [--no-constraints] [--no-ngram] [--positions | --no-positions]

With MOCR_LIB pointing at a library built from another commit (--unscored-only when it has no scored exports,
--no-alternatives when it has no alternatives exports, --no-constraints when it has no token-set exports, --no-ngram when it has no n-gram exports) the numbers of the two builds can be compared: the unscored and
the scored kernels are meant to be the same code.
--positions adds the token-positions leg (--no-positions: a library without the exports, e.g. the parent commit's - its
position-less legs above are then the numbers to compare): the wall time of one batch (graph replays, not instrumented) with
positions off and on, interleaved, and an instrumented pass's kernel times of the deferred pass.
Prints one JSON line per (rows, mode): medians over the repetitions and their min .. max spread, in microseconds."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "manga-ocr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

DECODE_PREFIXES = ("gemm_dec", "dec_", "lat_attn", "lat8_attn", "sm_", "compact_rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="64,2560")
    ap.add_argument("--max-len", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--unscored-only", action="store_true")
    ap.add_argument("--no-alternatives", action="store_true")
    ap.add_argument("--no-constraints", action="store_true")
    ap.add_argument("--no-ngram", action="store_true")
    ap.add_argument("--positions", action="store_true")
    ap.add_argument("--no-positions", action="store_true")
    args = ap.parse_args()

    import ctypes as C
    from manga_ocr import _capi
    if args.unscored_only:      # a library without the scored exports: bind what it has
        _capi.SYMBOLS = {k: v for k, v in _capi.SYMBOLS.items() if "_scored" not in k and not k.endswith("_lse")}
    if args.unscored_only or args.no_alternatives:      # ... or without the alternatives exports
        _capi.SYMBOLS = {k: v for k, v in _capi.SYMBOLS.items() if "_alts" not in k and not k.endswith("_topk")}
    constraints = not (args.unscored_only or args.no_alternatives or args.no_constraints)
    if not constraints:         # ... or without the token-set exports
        _capi.SYMBOLS = {k: v for k, v in _capi.SYMBOLS.items() if "token_set" not in k and "_constrained" not in k and not k.endswith("_masked")}
    ngram = constraints and not args.no_ngram
    if not ngram:               # ... or without the n-gram exports
        _capi.SYMBOLS = {k: v for k, v in _capi.SYMBOLS.items() if "_norepeat" not in k and "ngram" not in k}
    if args.no_positions or not ngram:      # ... or without the positions exports
        _capi.SYMBOLS = {k: v for k, v in _capi.SYMBOLS.items() if "_positions" not in k}
    from manga_ocr.engine import Engine
    from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights

    w = synthetic_weights(0)
    steps = args.max_len - 1
    for rows in [int(r) for r in args.rows.split(",")]:
        eng = Engine(w, DEFAULT_SPEC, dtype="bf16", device=0, max_batch=rows, lanes=1)
        gray = np.random.RandomState(rows).randint(0, 256, size=(rows, 224, 224), dtype=np.uint8)
        half = eng.token_set(np.nonzero(np.random.RandomState(7).rand(DEFAULT_SPEC.vocab) < 0.5)[0]) if constraints else 0
        modes = [0] if args.unscored_only else [0, 1] if args.no_alternatives else [0, 1, 2]
        legs = [(m, c, 0) for c in ([False, True] if constraints else [False]) for m in modes] + ([(m, False, 3) for m in modes] if ngram else [])
        for mode, constrained, ng in legs:
            scored = mode >= 1
            kw = dict(token_sets=half) if constrained else dict(no_repeat_ngram=ng) if ng else {}
            call = (lambda: eng.recognize_gray(gray, args.max_len, alternatives=True, **kw)) if mode == 2 else \
                (lambda: eng.recognize_gray(gray, args.max_len, scores=True, **kw)) if mode == 1 else (lambda: eng.recognize_gray(gray, args.max_len, **kw))
            call()                                           # warm: graphs, caches, clocks
            call()
            head, step, per = [], [], {}
            eng.profile_enable(True)
            call()                                           # a warm instrumented pass
            for _ in range(args.reps):
                eng.profile_reset()
                call()
                st = {s["name"]: s for s in eng.profile_get()}
                lm = [s for n, s in st.items() if n in ("gemm_dec_vocab", "gemm_dec_vocab_lse", "gemm_dec_vocab_topk", "sm_vocab", "dec_token", "dec_token_lse",
                                                              "dec_token_topk", "gemm_dec_vocab_m", "dec_token_m", "dec_token_lse_m", "dec_token_topk_m",
                                                              "dec_token_ng", "dec_token_lse_ng", "dec_token_topk_ng")]
                dec = [s for n, s in st.items() if n.startswith(DECODE_PREFIXES) and n != "dec_token_first"]
                assert all(s["launches"] % steps == 0 for s in lm), {n: s["launches"] for n, s in st.items()}
                head.append(1e3 * sum(s["total_ms"] for s in lm) / steps)
                for s in lm:
                    per.setdefault(s["name"], []).append(1e3 * s["total_ms"] / steps)
                step.append(1e3 * sum(s["total_ms"] for s in dec) / steps)
            eng.profile_enable(False)
            print(json.dumps(dict(rows=rows, max_len=args.max_len, scored=scored, alternatives=mode == 2, constrained=constrained, ngram=ng, reps=args.reps,
                                  lm_head_plus_token_us=round(statistics.median(head), 2), lm_head_spread_us=[round(min(head), 2), round(max(head), 2)],
                                  decode_step_us=round(statistics.median(step), 2), decode_step_spread_us=[round(min(step), 2), round(max(step), 2)],
                                  per_kernel_us={n: round(statistics.median(v), 2) for n, v in sorted(per.items())},
                                  lib=os.environ.get("MOCR_LIB", "default"))), flush=True)
        if args.positions and ngram and not args.no_positions:
            import time
            off = lambda: eng.recognize_gray(gray, args.max_len)                       # noqa: E731
            on = lambda: eng.recognize_gray(gray, args.max_len, positions=True)        # noqa: E731
            for f in (off, on, off, on):
                f()                                           # warm: buffers, graphs of both kinds
            t_off, t_on = [], []
            for _ in range(args.reps):
                for f, acc in ((off, t_off), (on, t_on)):
                    t0 = time.perf_counter()
                    f()
                    acc.append(1e3 * (time.perf_counter() - t0))
            eng.profile_enable(True)
            on()
            eng.profile_reset()
            on()
            st = {s["name"]: s for s in eng.profile_get()}
            eng.profile_enable(False)
            names = ("gemm_pos_k", "gemm_pos_q", "attn_positions", "pos_hist_ln")
            print(json.dumps(dict(rows=rows, max_len=args.max_len, positions=True, reps=args.reps,
                                  batch_ms_off=round(statistics.median(t_off), 3), batch_ms_off_spread=[round(min(t_off), 3), round(max(t_off), 3)],
                                  batch_ms_on=round(statistics.median(t_on), 3), batch_ms_on_spread=[round(min(t_on), 3), round(max(t_on), 3)],
                                  pass_kernels_ms={n: round(st[n]["total_ms"], 3) for n in names if n in st},
                                  lib=os.environ.get("MOCR_LIB", "default"))), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
