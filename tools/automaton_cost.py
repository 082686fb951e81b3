#!/usr/bin/env python3
"""What token automata cost the token step: HIP-event time per greedy step of the token kernel (the engine's own profiler: an
instrumented eager pass per repetition), bf16, ids-only batches of 96 and 1024 rows, max_len 32.

    python tools/automaton_cost.py [--lib PATH] [--label NAME] [--modes ngram,trie,universal] [--rows 96,1024] [--reps 7]
    python tools/automaton_cost.py --alternate PARENT_LIB [--runs 3] [--out profiles/automaton_cost.jsonl]

The first form measures one library in this process.  Mode ``ngram``: a plain no-repeat n-gram batch (n = 3, dec_token_ng) -
the mode that exists on the parent commit as well, so --lib pointed at a build of the parent gives the number this commit
must not exceed.  Modes ``trie`` (every row under a lexicon of 8,000 random words of 2 .. 8 of 200 tokens) and ``universal``
(every row under the universal automaton: 6,143 edges per step to look up and to set) run dec_token_am and need this commit.
The second form is the record: it starts the first form in fresh processes, alternating PARENT_LIB (ngram only) and this
tree's library (all three modes) --runs times, appends every line to --out and ends it with the parent's own run-to-run
spread and the conclusion.  Prints one JSON line per (mode, row count): the median over the repetitions and their min ..
max, in microseconds per step."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = {"ngram": "dec_token_ng", "trie": "dec_token_am", "universal": "dec_token_am"}


def trie(words):
    """{state: {token: next}} and the accepting states of a list of token sequences"""
    trans, acc, n = {0: {}}, set(), 1
    for w in words:
        s = 0
        for t in w:
            nxt = trans.setdefault(s, {})
            if t not in nxt:
                nxt[t] = n
                n += 1
            s = nxt[t]
        acc.add(s)
    return trans, acc


def measure(args):
    for p in (ROOT, os.path.join(ROOT, "manga-ocr_amd")):
        sys.path.insert(0, p)
    if args.lib:
        os.environ["MOCR_LIB"] = os.path.abspath(args.lib)
    import numpy as np
    from manga_ocr import _capi
    from manga_ocr.engine import Engine
    from manga_ocr.text import pack_automaton
    from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights

    if args.lib:        # a library of the parent commit lacks the symbols this commit adds: bind what it has
        import ctypes
        lib = ctypes.CDLL(os.environ["MOCR_LIB"])
        _capi.SYMBOLS = {k: v for k, v in _capi.SYMBOLS.items() if hasattr(lib, k)}
    w = synthetic_weights(0)
    steps = args.max_len - 1
    for rows in [int(r) for r in args.rows.split(",")]:
        eng = Engine(w, DEFAULT_SPEC, dtype="bf16", device=0, max_batch=rows, lanes=1)
        gray = np.random.RandomState(rows).randint(0, 256, size=(rows, 224, 224), dtype=np.uint8)
        for mode in args.modes.split(","):
            if mode == "ngram":
                kw = dict(no_repeat_ngram=3)
            elif mode == "universal":
                kw = dict(automata=eng.automaton(*pack_automaton({0: {t: 0 for t in range(DEFAULT_SPEC.vocab) if t != DEFAULT_SPEC.eos_id}}, [0])))
            else:
                rs = np.random.RandomState(11)
                alphabet = rs.choice(np.arange(5, DEFAULT_SPEC.vocab), size=200, replace=False)
                words = [[int(t) for t in alphabet[rs.randint(0, 200, size=rs.randint(2, 9))]] for _ in range(8000)]
                kw = dict(automata=eng.automaton(*pack_automaton(*trie(words))))
            call = lambda: eng.recognize_gray(gray, args.max_len, **kw)      # noqa: E731
            call()
            call()
            eng.profile_enable(True)
            call()
            us, launches = [], []
            for _ in range(args.reps):
                eng.profile_reset()
                lens = call()[1]
                s = {x["name"]: x for x in eng.profile_get()}[KERNEL[mode]]
                us.append(1e3 * s["total_ms"] / s["launches"])
                launches.append(int(s["launches"]))
            eng.profile_enable(False)
            print(json.dumps(dict(what=KERNEL[mode], mode=mode, build=args.label, rows=rows, max_len=args.max_len, reps=args.reps,
                                  steps=sorted(set(launches)), mean_len=round(float(np.mean(lens)), 2), us_per_step=round(statistics.median(us), 3),
                                  spread_us=[round(min(us), 3), round(max(us), 3)])), flush=True)
            assert max(launches) <= steps
        eng.close()


def alternate(args):
    lines = []

    def run(label, lib, modes):
        cmd = [sys.executable, os.path.abspath(__file__), "--label", label, "--modes", modes, "--rows", args.rows, "--reps", str(args.reps),
               "--max-len", str(args.max_len)] + (["--lib", lib] if lib else [])
        out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=args.timeout).stdout
        for ln in out.splitlines():
            if ln.startswith("{"):
                print(ln, flush=True)
                lines.append(json.loads(ln))

    for k in range(1, args.runs + 1):
        run(f"parent_run{k}", args.alternate, "ngram")
        run(f"this_run{k}", None, "ngram,trie,universal")
    text = []
    for rows in [int(r) for r in args.rows.split(",")]:
        med = lambda build, mode: [x["us_per_step"] for x in lines if x["rows"] == rows and x["mode"] == mode and x["build"].startswith(build)]  # noqa: E731
        p, t = med("parent", "ngram"), med("this", "ngram")
        spread = max(p) - min(p)
        slower = statistics.mean(t) - statistics.mean(p)
        verdict = "not slower" if slower <= spread else "SLOWER than the parent's own run-to-run spread allows"
        text.append(f"{rows} rows: plain n-gram batch {min(t):.2f}-{max(t):.2f} us a step against the parent's {min(p):.2f}-{max(p):.2f} "
                    f"(mean {slower:+.2f} us, parent run-to-run spread {spread:.2f} us: {verdict}); trie batch "
                    f"{statistics.median(med('this', 'trie')):.2f} us, universal-automaton batch {statistics.median(med('this', 'universal')):.2f} us "
                    f"(new cost, no threshold)")
        lines.append(dict(what="parent_spread", rows=rows, us=round(spread, 3), ngram_this_minus_parent_us=round(slower, 3)))
    lines.append(dict(what="conclusion", text=f"Medians of {args.reps} instrumented passes per process, {args.runs} alternating processes each. " + "; ".join(text) + "."))
    with open(args.out, "a", encoding="ascii") as f:
        for x in lines:
            f.write(json.dumps(x) + "\n")
    print(lines[-1]["text"], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default="this")
    ap.add_argument("--modes", default="ngram,trie,universal")
    ap.add_argument("--rows", default="96,1024")
    ap.add_argument("--max-len", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--alternate", default=None, metavar="PARENT_LIB")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "automaton_cost.jsonl"))
    args = ap.parse_args()
    alternate(args) if args.alternate else measure(args)


if __name__ == "__main__":
    main()
