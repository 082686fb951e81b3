#!/usr/bin/env python3
"""What a repetition penalty costs a decode step: HIP-event time per greedy step of the token kernel AND of the LM head (the
engine's own profiler: an instrumented eager pass per repetition), bf16, ids-only batches of 96 and 1024 rows, max_len 32.
Modelled on tools/soft_automaton_cost.py.

    python tools/penalty_cost.py [--lib PATH] [--label NAME] [--modes greedy,ngram,penalty,worst] [--rows 96,1024] [--reps 7]
    python tools/penalty_cost.py --alternate PARENT_LIB [--runs 3] [--out profiles/penalty_cost.jsonl]

The first form measures one library in this process.  The modes that exist on the parent commit as well - ``greedy`` (the
flagship: dec_token / gemm_dec_vocab) and ``ngram`` (n = 3, the masked LM head a penalty batch is measured against:
dec_token_ng / gemm_dec_vocab_m) - give, with --lib pointed at a build of the parent, the numbers this commit must not exceed
beyond the parent's own run-to-run spread.  The new mode needs this commit and is reported without a threshold: ``penalty``
(every row at p = 1.3: dec_token_rp / gemm_dec_vocab_rp).  Through the recognise path a row has seen at most max_len tokens,
so the mode ``worst`` times the kernels themselves through the operator hooks (mocr_op_gemm_argmax_penalty,
mocr_op_dec_token_penalty; this commit only): the ids-only masked LM head on the tile the engine takes at that row count
and the token kernel on its candidate and its one-slab path, each in its masked form (``plain``), under p = 1.3 with 32
tokens seen a row (``seen32``) and with a random half of the vocabulary seen (``half``: the worst case).  The leg ``soft_none``
is the SOFT form without a penalty on rows that bring no automaton (state NONE): what the PEN forms pay for being SOFT forms
too, the measured basis of keeping one family instead of splitting off a PEN-only one.
The second form is the record: it starts the first form in fresh processes, alternating PARENT_LIB (the old modes) and this
tree's library (all four) --runs times, appends every line to --out and ends it with the parent's spread and the conclusion.
One JSON line per (mode, kernel, row count): the median over the repetitions and their min .. max, in microseconds per step."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOK_LEGS = ("plain", "soft_none", "seen32", "half")


def measure_hooks(args, eng, rows, np):
    """the ``worst`` mode: one JSON line per (kernel, leg); random bf16 operands, every row its own all-ones mask"""
    import torch
    V, D, MW = 6144, 768, 192
    tile = 64 if rows <= 96 else 128
    nt = V // tile
    rs = np.random.RandomState(rows)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()        # noqa: E731
    A = dev(rs.standard_normal((-(-rows // 128) * 128, D)) * 0.5, np.float32).to(torch.bfloat16)
    W = dev(rs.standard_normal((V, D)) * 0.05, np.float32).to(torch.bfloat16)
    bias = dev(rs.standard_normal(V), np.float32)
    ones = dev(np.full((rows, MW), -1, np.int32), np.int32)
    base = dev(np.full((1, MW), -1, np.int32), np.int32)
    ident, zeros = dev(np.arange(rows), np.int32), dev(np.zeros(rows), np.int32)
    pen = dev(np.full(rows, 1.3), np.float32)

    def seen_words(bits):
        m = np.zeros((rows, V), bool)
        for r in range(rows):
            m[r, rs.choice(V, size=bits, replace=False)] = True
        w = m.reshape(rows, MW, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)
        return dev(w.sum(-1).astype(np.uint32).view(np.int32), np.int32)
    seen = {"seen32": seen_words(32), "half": seen_words(V // 2)}
    # an arena of one state without edges, and every row without an automaton
    none, one0, onem1 = dev(np.full(rows, -1), np.int32), dev([0, 0], np.int32), dev([-1], np.int32)
    acc, w0 = torch.zeros(1, dtype=torch.uint8, device="cuda"), torch.zeros(1, device="cuda")
    cv = torch.zeros((rows, nt), device="cuda")
    ci = torch.zeros((rows, nt), dtype=torch.int32, device="cuda")
    logits = dev(rs.standard_normal((rows, V)) * 3, np.float32)

    def head(leg):
        if leg == "plain":
            eng.op_gemm_argmax_soft(A, W, bias, cv, ci, None, None, None, rows, V, D, tile, ones, ident, ident, None, None, 0, None, None)
        elif leg == "soft_none":
            eng.op_gemm_argmax_soft(A, W, bias, cv, ci, None, None, None, rows, V, D, tile, ones, ident, ident, None, None, 0, None, None,
                                    d_aut_state=none, d_edge_begin=one0, d_edge_token=one0, d_edge_weight=w0)
        else:
            eng.op_gemm_argmax_penalty(A, W, bias, cv, ci, None, None, None, rows, V, D, tile, ones, ident, ident, None, None, 0, None, None,
                                       d_seen_mask=seen[leg], d_penalty_of_row=pen)

    def token(leg, slab):
        d = dict(ids=torch.full((rows, 32), 7, dtype=torch.int32, device="cuda"), step=dev(np.full(rows, 5), np.int32), finished=zeros.clone(),
                 len=dev(np.full(rows, 32), np.int32), n_unfinished=dev([rows, 0], np.int32), rowmap=ident,
                 x_f32=torch.zeros((rows, D), device="cuda"), x_t=torch.zeros((rows, D), device="cuda", dtype=torch.bfloat16))
        kw = dict(slabs=logits, nslab=1, vbias=bias) if slab else dict(cand_val=cv, cand_idx=ci, ncand=nt)
        args_ = (None, None, None, None, None, None, ones, ident, ones, base, zeros, zeros, None, None, 0, None) + (None,) * 8
        if leg == "soft_none":
            eng.op_dec_token_soft(*args_[:16], one0, one0, one0, acc, none, none.clone(), w0, onem1, first=0, n=rows, ids_ld=32, max_len=32, n_real=rows,
                                  **d, **kw)
        elif leg == "plain":
            eng.op_dec_token_soft(*args_, first=0, n=rows, ids_ld=32, max_len=32, n_real=rows, **d, **kw)
        else:
            eng.op_dec_token_penalty(*args_, seen[leg].clone(), pen, first=0, n=rows, ids_ld=32, max_len=32, n_real=rows, **d, **kw)

    legs = [("lm_head_tile%d" % tile, "op_gemm_argmax_masked", head)] + \
           [("token_%s" % ("slab1" if slab else "cand"), None, (lambda leg, slab=slab: token(leg, slab))) for slab in (False, True)]
    head("plain")
    eng.profile_enable(True)
    for what, name, fn in legs:
        for leg in HOOK_LEGS:
            fn(leg)
            us = []
            for _ in range(args.reps):
                eng.profile_reset()
                fn(leg)
                stats = [x for x in eng.profile_get() if x["launches"] > 0 and (x["name"] == name if name else x["name"].startswith("dec_token"))]
                assert len(stats) == 1, stats
                us.append(1e3 * stats[0]["total_ms"] / stats[0]["launches"])
            print(json.dumps(dict(what=what, mode="worst", leg=leg, kernel=stats[0]["name"], build=args.label, rows=rows, reps=args.reps,
                                  us_per_step=round(statistics.median(us), 3), spread_us=[round(min(us), 3), round(max(us), 3)])), flush=True)
    eng.profile_enable(False)


KERNELS = {"greedy": ("dec_token", "gemm_dec_vocab"), "ngram": ("dec_token_ng", "gemm_dec_vocab_m"), "penalty": ("dec_token_rp", "gemm_dec_vocab_rp")}
OLD = "greedy,ngram"


def measure(args):
    for p in (ROOT, os.path.join(ROOT, "manga-ocr_amd")):
        sys.path.insert(0, p)
    if args.lib:
        os.environ["MOCR_LIB"] = os.path.abspath(args.lib)
    import numpy as np
    if "worst" in args.modes.split(","):        # (one HIP runtime per process, torch's: before the engine's library)
        import torch
        torch.cuda.init()
    from manga_ocr import _capi
    from manga_ocr.engine import Engine
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
            if mode == "worst":
                measure_hooks(args, eng, rows, np)
                continue
            if mode == "greedy":
                kw = {}
            elif mode == "ngram":
                kw = dict(no_repeat_ngram=3)
            else:
                kw = dict(penalty=1.3)
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
               "--max-len", str(args.max_len)] + (["--lib", lib] if lib else [])
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
        for what in sorted({x["what"] for x in lines if x.get("mode") == "worst" and x.get("rows") == rows}):
            leg = {g: statistics.median([x["us_per_step"] for x in lines if x.get("mode") == "worst" and x.get("rows") == rows and
                                         x["what"] == what and x["leg"] == g]) for g in HOOK_LEGS}
            text.append(f"{rows} rows, hooks, {what}: plain {leg['plain']:.2f} us, SOFT form on rows without an automaton {leg['soft_none']:.2f} us, p = 1.3 with 32 tokens seen {leg['seen32']:.2f} us, "
                        f"with half the vocabulary seen {leg['half']:.2f} us")
        for mode in [m for m in args.modes.split(",") if m not in OLD.split(",") and m != "worst"]:
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
    ap.add_argument("--modes", default="greedy,ngram,penalty,worst")
    ap.add_argument("--rows", default="96,1024")
    ap.add_argument("--max-len", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--alternate", default=None, metavar="PARENT_LIB")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=300.0)
    ap.add_argument("--session", default=None, help="a name written into every line of this record (a file may hold several)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "penalty_cost.jsonl"))
    args = ap.parse_args()
    alternate(args) if args.alternate else measure(args)


if __name__ == "__main__":
    main()
