#!/usr/bin/env python3
"""What beam search costs: wall time per call of a bf16 engine, 64 crops, generate length 32, for
  (i)   beam search, K = 4 (include/mocr.h "beam search": 256 decode rows over 64 encodings),
  (ii)  the same 64 crops as 256 greedy scored rows through ``sources=`` - the same encoder pass, the same number of decode
        rows, no selection and no cache reorder: (i) / (ii) is the price of those two,
  (iii) plain greedy, 64 rows,
  (iv)  the beam batch of (i) with token scores (``beam_scores=True``) and (v) with token scores under a set of 40 tokens
        (``beam_sets=``): the token form of the selection (include/mocr.h "beam search with token sets and token scores");
        (iv) / (i) is its price - a build without it (the parent commit) runs (i) - (iii) alone, and (i) must agree between
        the two builds within its run-to-run spread (best-of-N, the ``spread_ms`` minimum, is the figure to compare),
  (vi)  the beam batch of (i) with token positions (``beam_positions=True``; include/mocr.h "beam search with token
        positions") and (vii) with token scores and positions: (vi) / (i) is the price of the recorded rows, the trails in the
        selection and the deferred pass.  The lines of (i), (vi) and (vii) are also appended to --positions-out (by default
        profiles/beam_positions_cost.jsonl of this checkout): run it on this build and, with --tree, on a built checkout of
        the parent commit, whose plain beam batch (i) is the yardstick - that build has no (vi) / (vii),
  (viii) the beam batch of (i) with every crop under a trie of 8,000 random words of 2 to 12 tokens and (ix) under the universal
        automaton, the worst case - 6,143 edges to scan per beam and step (include/mocr.h "beam search under a token
        automaton").  The lines of (i), (v), (viii) and (ix) are also appended to --automaton-out (by default
        profiles/beam_automaton_cost.jsonl): on the parent commit's build, which has no (viii) / (ix), (i) and (v) are the
        yardsticks - they launch what they launched and must lie within that build's own min .. max,
  (x)   the beam batch of (i) with every crop under a glossary of 8,000 random names of 2 to 12 tokens over 200 tokens in
        MangaOcr.glossary's compact (fallback) form, bonus 2, and (xi) with every crop in ONE state of 6,143 weighted edges -
        the universal automaton with a weight on every edge, the worst case of the row pass (include/mocr.h "beam search under
        soft token automata").  The lines of (i), (v), (viii), (x) and (xi) are also appended to --soft-out (by default
        profiles/beam_soft_cost.jsonl): on the parent commit's build, which has no (x) / (xi), (i), (v) and (viii) are the
        yardsticks,
and, with --profile, the two new kernels' times from the engine's per-kernel profile at 400 rows.

    python tools/beam_cost.py [--tree DIR] [--label NAME] [--crops 64] [--beams 4] [--max-len 32] [--reps 7] [--profile]
                              [--positions-out profiles/beam_positions_cost.jsonl] [--automaton-out profiles/beam_automaton_cost.jsonl]
                              [--soft-out profiles/beam_soft_cost.jsonl]

--tree: the checkout whose package and library are measured (default: this one); a built checkout of the parent commit runs
(ii) and (iii) alone - they are the yardsticks and must agree between the two builds within their own run-to-run spread.
Prints one JSON line per form: the median over the repetitions after two warm-ups and their min .. max, in milliseconds."""
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
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--max-len", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--positions-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "beam_positions_cost.jsonl"),
                    help="append the plain beam line and the positions lines to this file ('' = nowhere)")
    ap.add_argument("--automaton-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "beam_automaton_cost.jsonl"),
                    help="append the plain beam line, the 40-token-set line and the automaton lines to this file ('' = nowhere)")
    ap.add_argument("--soft-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "beam_soft_cost.jsonl"),
                    help="append the plain beam line, the 40-token-set line, the trie line and the two soft lines to this file ('' = nowhere)")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    for p in (tree, os.path.join(tree, "manga-ocr_amd")):
        sys.path.insert(0, p)
    import numpy as np
    import manga_ocr.engine as me
    from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights

    K = args.beams
    rows = args.crops * K
    w = synthetic_weights(0)
    eng = me.Engine(w, DEFAULT_SPEC, dtype="bf16", device=0, max_batch=rows, lanes=1)
    gray = np.random.RandomState(rows).randint(0, 256, size=(args.crops, 224, 224), dtype=np.uint8)
    source = np.repeat(np.arange(args.crops), K)
    forms = [("greedy_shared_rows", lambda: eng.recognize_gray(gray, args.max_len, scores=True, sources=source)),
             ("greedy", lambda: eng.recognize_gray(gray, args.max_len))]
    beam = getattr(me, "BeamConfig", None)      # (the parent commit has no beam search)
    if beam is not None:
        cfg = beam(K, 2.0, True, 3)
        forms.insert(0, ("beam", lambda: eng.recognize_gray(gray, args.max_len, beam=cfg)))
        if hasattr(eng, "beam_token_state_bytes"):      # (the parent commit has no token form)
            some = eng.token_set(np.random.RandomState(40).choice(np.arange(5, DEFAULT_SPEC.vocab), 40, replace=False).tolist())
            forms.append(("beam_token_scores", lambda: eng.recognize_gray(gray, args.max_len, beam=cfg, beam_scores=True)))
            forms.append(("beam_token_scores_set40", lambda: eng.recognize_gray(gray, args.max_len, beam=cfg, beam_scores=True, beam_sets=some)))
        if hasattr(eng, "beam_position_state_bytes"):   # (the parent commit has no positions for hypotheses)
            forms.append(("beam_positions", lambda: eng.recognize_gray(gray, args.max_len, beam=cfg, beam_positions=True)))
            forms.append(("beam_token_scores_positions", lambda: eng.recognize_gray(gray, args.max_len, beam=cfg, beam_scores=True, beam_positions=True)))
        if hasattr(eng, "op_beam_select_automaton"):    # (the parent commit has no beam search under automata)
            rs = np.random.RandomState(8000)
            trans, accepting, n_states = {0: {}}, set(), 1
            for _ in range(8000):       # a trie of 8,000 random words over 400 tokens: wide at the root, deep below
                s = 0
                for t in rs.randint(5, 405, size=rs.randint(2, 13)):
                    t = int(t) + (1 if int(t) >= DEFAULT_SPEC.eos_id else 0)
                    if t not in trans.setdefault(s, {}):
                        trans[s][t] = n_states
                        n_states += 1
                    s = trans[s][t]
                accepting.add(s)
            from manga_ocr.text import pack_automaton
            trie = eng.automaton(*pack_automaton(trans, accepting))
            uni = eng.automaton(*pack_automaton({0: {t: 0 for t in range(DEFAULT_SPEC.vocab) if t != DEFAULT_SPEC.eos_id}}, [0]))
            forms.append(("beam_automaton_trie8000", lambda: eng.recognize_gray(gray, args.max_len, beam=cfg, beam_automata=trie, beam_states=True)))
            forms.append(("beam_automaton_universal", lambda: eng.recognize_gray(gray, args.max_len, beam=cfg, beam_automata=uni, beam_states=True)))
        if hasattr(eng, "op_beam_select_soft"):         # (the parent commit has no beam search under soft automata)
            from manga_ocr.text import bias_automaton, pack_automaton
            rs = np.random.RandomState(8001)
            seqs = {}
            for _ in range(8000):       # MangaOcr.glossary's sequences: every prefix of two or more tokens of a name, bonus 2
                name = tuple(int(t) + (1 if int(t) >= DEFAULT_SPEC.eos_id else 0) for t in rs.randint(5, 205, size=rs.randint(2, 13)))
                for n in range(2, len(name) + 1):
                    seqs[name[:n]] = 2.0
            trans, weights = bias_automaton(seqs, compact=True)
            gloss = eng.automaton(*pack_automaton(trans, set(trans), weights=weights, default=0, fallback=True))
            every = {t: 0 for t in range(DEFAULT_SPEC.vocab) if t != DEFAULT_SPEC.eos_id}
            heavy = eng.automaton(*pack_automaton({0: every}, [0], weights={0: {t: ((t * 37) % 17 - 8) / 8.0 or 0.125 for t in every}}))
            forms.append(("beam_soft_glossary8000", lambda: eng.recognize_gray(gray, args.max_len, beam=cfg, beam_automata=gloss, beam_states=True,
                                                                                beam_soft=True)))
            forms.append(("beam_soft_weighted6143", lambda: eng.recognize_gray(gray, args.max_len, beam=cfg, beam_automata=heavy, beam_states=True,
                                                                                beam_soft=True)))
    for form, call in forms:
        for _ in range(2):
            call()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            ms.append(1e3 * (time.perf_counter() - t0))
        line = json.dumps(dict(what="beam_cost", build=args.label, form=form, crops=args.crops, beams=K, max_len=args.max_len, reps=args.reps,
                               ms_per_call=round(statistics.median(ms), 3), spread_ms=[round(min(ms), 3), round(max(ms), 3)]))
        print(line, flush=True)
        if args.positions_out and form in ("beam", "beam_positions", "beam_token_scores_positions"):
            os.makedirs(os.path.dirname(os.path.abspath(args.positions_out)), exist_ok=True)
            with open(args.positions_out, "a", encoding="utf-8") as f:
                f.write(line + "\n")
        if args.automaton_out and form in ("beam", "beam_token_scores_set40", "beam_automaton_trie8000", "beam_automaton_universal"):
            os.makedirs(os.path.dirname(os.path.abspath(args.automaton_out)), exist_ok=True)
            with open(args.automaton_out, "a", encoding="utf-8") as f:
                f.write(line + "\n")
        if args.soft_out and form in ("beam", "beam_token_scores_set40", "beam_automaton_trie8000", "beam_soft_glossary8000", "beam_soft_weighted6143"):
            os.makedirs(os.path.dirname(os.path.abspath(args.soft_out)), exist_ok=True)
            with open(args.soft_out, "a", encoding="utf-8") as f:
                f.write(line + "\n")
    eng.close()
    if args.profile and beam is not None:
        n = 400 // K
        eng = me.Engine(w, DEFAULT_SPEC, dtype="bf16", device=0, max_batch=n * K, lanes=1)
        g = np.random.RandomState(7).randint(0, 256, size=(n, 224, 224), dtype=np.uint8)
        kws = [{}] + ([dict(beam_scores=True)] if hasattr(eng, "beam_token_state_bytes") else [])
        kws += [dict(beam_positions=True)] if hasattr(eng, "beam_position_state_bytes") else []
        if hasattr(eng, "op_beam_select_soft"):         # the soft selection, every crop in the state of 6,143 weighted edges
            from manga_ocr.text import pack_automaton
            every = {t: 0 for t in range(DEFAULT_SPEC.vocab) if t != DEFAULT_SPEC.eos_id}
            heavy = eng.automaton(*pack_automaton({0: every}, [0], weights={0: {t: ((t * 37) % 17 - 8) / 8.0 or 0.125 for t in every}}))
            kws += [dict(beam_automata=heavy, beam_states=True, beam_soft=True)]
        for kw in kws:
            eng.recognize_gray(g, args.max_len, beam=cfg, **kw)
            eng.profile_enable(True)
            eng.profile_reset()
            eng.recognize_gray(g, args.max_len, beam=cfg, **kw)
            for s in eng.profile_get():
                if s["name"] in ("beam_select", "beam_select_tok", "beam_select_am", "beam_select_sw", "beam_permute", "beam_init", "dec_attn_self", "latent_self", "gemm_dec_vocab",
                                 "gemm_pos_k", "gemm_pos_q", "attn_positions"):
                    print(json.dumps(dict(what="beam_kernels", build=args.label, rows=n * K, max_len=args.max_len, kernel=s["name"],
                                          launches=s["launches"], total_ms=round(s["total_ms"], 3),
                                          us_per_launch=round(1e3 * s["total_ms"] / max(s["launches"], 1), 2))), flush=True)
            eng.profile_enable(False)
        eng.close()


if __name__ == "__main__":
    main()
