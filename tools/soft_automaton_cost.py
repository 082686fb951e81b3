#!/usr/bin/env python3
"""What soft token automata cost a decode step: HIP-event time per greedy step of the token kernel AND of the LM head (the
engine's own profiler: an instrumented eager pass per repetition), bf16, ids-only batches of 96 and 1024 rows, max_len 32.
Modelled on tools/automaton_cost.py.

    python tools/soft_automaton_cost.py [--lib PATH] [--label NAME] [--modes greedy,ngram,hard,glossary,worst] [--rows 96,1024] [--reps 7]
    python tools/soft_automaton_cost.py --alternate PARENT_LIB [--runs 3] [--session NAME] [--out profiles/soft_automaton_cost.jsonl]

The first form measures one library in this process.  The modes that exist on the parent commit as well - ``greedy`` (the
flagship: dec_token / gemm_dec_vocab), ``ngram`` (n = 3: dec_token_ng / gemm_dec_vocab_m) and ``hard`` (every row under a
lexicon of 8,000 random words: dec_token_am / gemm_dec_vocab_m) - give, with --lib pointed at a build of the parent, the
numbers this commit must not exceed beyond the parent's own run-to-run spread.  The new modes need this commit and are
reported without a threshold: ``glossary`` (every row under MangaOcr.glossary's automaton of the 8,000 random words, bonus 2 -
the compact compilation with fallback default edges: dec_token_sw / gemm_dec_vocab_sw) and ``worst`` (every row in one open
state with 6,143 weighted edges).
The second form is the record: it starts the first form in fresh processes, alternating PARENT_LIB (the three old modes) and
this tree's library (all five) --runs times, appends every line to --out and ends it with the parent's spread and the
conclusion.  One JSON line per (mode, kernel, row count): the median over the repetitions and their min .. max, in
microseconds per step.  The committed file holds two records: the protocol as it stands (no session name), and
``--runs 6 --rows 1024 --modes greedy,ngram,hard --session six_processes_1024_rows``, taken because three processes did not
settle the 1024-row masked head."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"greedy": ("dec_token", "gemm_dec_vocab"), "ngram": ("dec_token_ng", "gemm_dec_vocab_m"), "hard": ("dec_token_am", "gemm_dec_vocab_m"),
           "glossary": ("dec_token_sw", "gemm_dec_vocab_sw"), "worst": ("dec_token_sw", "gemm_dec_vocab_sw")}
OLD = "greedy,ngram,hard"


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
    from manga_ocr.text import bias_automaton, pack_automaton
    from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights

    if args.lib:        # a library of the parent commit lacks the symbols this commit adds: bind what it has
        import ctypes
        lib = ctypes.CDLL(os.environ["MOCR_LIB"])
        _capi.SYMBOLS = {k: v for k, v in _capi.SYMBOLS.items() if hasattr(lib, k)}
    w = synthetic_weights(0)
    V, eos = DEFAULT_SPEC.vocab, DEFAULT_SPEC.eos_id
    steps = args.max_len - 1
    rs = np.random.RandomState(11)
    alphabet = rs.choice(np.arange(5, V), size=200, replace=False)
    words = [[int(t) for t in alphabet[rs.randint(0, 200, size=rs.randint(2, 9))]] for _ in range(8000)]
    for rows in [int(r) for r in args.rows.split(",")]:
        eng = Engine(w, DEFAULT_SPEC, dtype="bf16", device=0, max_batch=rows, lanes=1)
        gray = np.random.RandomState(rows).randint(0, 256, size=(rows, 224, 224), dtype=np.uint8)
        for mode in args.modes.split(","):
            if mode == "greedy":
                kw = {}
            elif mode == "ngram":
                kw = dict(no_repeat_ngram=3)
            elif mode == "hard":
                kw = dict(automata=eng.automaton(*pack_automaton(*trie(words))))
            elif mode == "glossary":
                seqs = {tuple(wd[:n]): 2.0 for wd in words[:args.glossary_words] for n in range(2, len(wd) + 1)}
                trans, weights = bias_automaton(seqs, compact=True)
                kw = dict(automata=eng.automaton(*pack_automaton(trans, set(trans), weights=weights, default=0, fallback=True)))
            else:
                edges = [t for t in range(V) if t != eos]
                kw = dict(automata=eng.automaton(*pack_automaton({0: {t: 0 for t in edges}}, [0], weights={0: {t: ((t * 7) % 17 - 8) / 8.0 for t in edges}},
                                                                 default=0)))
            call = lambda: eng.recognize_gray(gray, args.max_len, **kw)      # noqa: E731
            call()
            call()
            eng.profile_enable(True)
            call()
            us = {k: [] for k in KERNELS[mode]}
            launches = []
            for _ in range(args.reps):
                eng.profile_reset()
                lens = call()[1]
                stats = {x["name"]: x for x in eng.profile_get()}
                for k in KERNELS[mode]:
                    us[k].append(1e3 * stats[k]["total_ms"] / stats[k]["launches"])
                launches.append(int(stats[KERNELS[mode][0]]["launches"]))
            eng.profile_enable(False)
            for k in KERNELS[mode]:
                print(json.dumps(dict(what=k, mode=mode, build=args.label, rows=rows, max_len=args.max_len, reps=args.reps, steps=sorted(set(launches)),
                                      mean_len=round(float(np.mean(lens)), 2), us_per_step=round(statistics.median(us[k]), 3),
                                      spread_us=[round(min(us[k]), 3), round(max(us[k]), 3)])), flush=True)
            assert max(launches) <= steps
        eng.close()


def alternate(args):
    lines = []

    def run(label, lib, modes):
        cmd = [sys.executable, os.path.abspath(__file__), "--label", label, "--modes", modes, "--rows", args.rows, "--reps", str(args.reps),
               "--max-len", str(args.max_len), "--glossary-words", str(args.glossary_words)] + (["--lib", lib] if lib else [])
        out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=args.timeout).stdout
        for ln in out.splitlines():
            if ln.startswith("{"):
                print(ln, flush=True)
                lines.append(json.loads(ln))

    for k in range(1, args.runs + 1):
        run(f"parent_run{k}", args.alternate, OLD)
        run(f"this_run{k}", None, args.modes)
    text = []
    for rows in [int(r) for r in args.rows.split(",")]:
        def med(build, mode, kernel):
            return [x["us_per_step"] for x in lines if x.get("rows") == rows and x.get("mode") == mode and x.get("what") == kernel and
                    x.get("build", "").startswith(build)]
        for mode in OLD.split(","):
            for kernel in KERNELS[mode]:
                p, t = med("parent", mode, kernel), med("this", mode, kernel)
                spread = max(p) - min(p)
                slower = statistics.mean(t) - statistics.mean(p)
                verdict = "not slower" if slower <= spread else "SLOWER than the parent's own run-to-run spread allows"
                text.append(f"{rows} rows, {mode}, {kernel}: {min(t):.2f}-{max(t):.2f} us a step against the parent's {min(p):.2f}-{max(p):.2f} "
                            f"(mean {slower:+.2f} us, parent spread {spread:.2f} us: {verdict})")
                lines.append(dict(what="parent_spread", rows=rows, mode=mode, kernel=kernel, us=round(spread, 3), this_minus_parent_us=round(slower, 3)))
        for mode in [m for m in args.modes.split(",") if m not in OLD.split(",")]:
            text.append(f"{rows} rows, {mode} (new cost, no threshold): " +
                        ", ".join(f"{kernel} {statistics.median(med('this', mode, kernel)):.2f} us" for kernel in KERNELS[mode]))
    lines.append(dict(what="conclusion", text=f"Medians of {args.reps} instrumented passes per process, {args.runs} alternating processes each. " + "; ".join(text) + "."))
    with open(args.out, "a", encoding="ascii") as f:
        for x in lines:
            f.write(json.dumps(dict(x, session=args.session) if args.session else x) + "\n")
    print(lines[-1]["text"], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default="this")
    ap.add_argument("--modes", default="greedy,ngram,hard,glossary,worst")
    ap.add_argument("--rows", default="96,1024")
    ap.add_argument("--max-len", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--glossary-words", type=int, default=8000)
    ap.add_argument("--alternate", default=None, metavar="PARENT_LIB")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=300.0)
    ap.add_argument("--session", default=None, help="a name written into every line of this record (a file may hold several)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_automaton_cost.jsonl"))
    args = ap.parse_args()
    alternate(args) if args.alternate else measure(args)


if __name__ == "__main__":
    main()
