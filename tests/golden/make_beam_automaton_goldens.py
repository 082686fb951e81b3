#!/usr/bin/env python3
"""Generate tests/golden/beam_aut_*.npz from transformers' own beam search under a history-dependent
``prefix_allowed_tokens_fn``: beam search under a token automaton (include/mocr.h).

PROVENANCE SCRIPT, like make_beam_token_goldens.py (whose model, crops and conventions it uses): it imports ``transformers``
(5.15.0), runs once on the build machine and nothing imports it.  Every crop is its own

    generate(num_beams=K, num_return_sequences=K, length_penalty, early_stopping, no_repeat_ngram_size,
             prefix_allowed_tokens_fn=f, output_scores=True, return_dict_in_generate=True)

call.  ``f(batch, ids)`` walks the crop's automaton over the beam's history and returns the state's edge tokens that the
crop's set holds, plus EOS iff the state accepts.  For a history that has left the automaton - the engine's dead beam - it
returns [PAD]: an empty list raises in transformers, and [EOS] would not do.  Such a history is not always a -inf beam: a
candidate that stopped on EOS is carried on at score - 1e9 when fewer than K others are left, and with [EOS] it would stop
again, enter the finished set at about -1e9 / len ^ length_penalty and, under early_stopping = true, end the search before
a real entry has finished.  Under the engine's rule that beam is dead and emits nothing; a PAD continuation never stops
either, and a third PAD falls to the n-gram ban.  The sets of case (b) take an edge away only where a sibling stays, so no
live state is left without a token.

THE -1e9 HYPOTHESES.  Descendants of the padding beams, which under a lexicon reach the finished set whenever it has fewer
real entries than beams, score -1e9 / len ^ length_penalty <= junk_below(length_penalty, max_length); they are stored as
empty slots, as make_beam_token_goldens.py stores them: their order among equals is torch.topk's business.  The tests mask
the engine's in the same way.

Cases (name -> K, length_penalty, early_stopping, no_repeat_ngram_size; automata):
  (a2) (a3) (a4) the published settings at K = 2, 3, 4 under random tries of 6 to 12 entries, 4 to 12 tokens each, every
      node with at most three children and two or three at the root;
  (b) K = 3, no_repeat_ngram_size 2, a token set that removes edges of the trie;
  (c) K = 4, a different automaton per crop: a trie, none, a 2-entry lexicon (fewer entries than beams), another trie;
  (d) K = 3, a loop over three tokens that cannot accept before max_length: the stop by length walks the last token;
  (e0) (e2) length_penalty 0 and 2 with early_stopping true, K = 4 and 3;
  (h2) (h3) (h4) for the bf16 engine: (a)'s settings, only crops whose candidates are at least 2e-2 apart, six per K.
A crop is kept when the float64 reference (tests/beam_automaton_util.py) sees its real candidates at least MIN_GAP (1e-3)
apart; the script asserts that transformers and the reference agree on every crop it writes - ids, lengths and states
exactly, token scores within SCORE_TOL (3e-6) and sequence scores within bau.score_tol: SCORE_TOL, or two fp32 steps of the
score where that is more - transformers' scores ARE fp32 numbers, and under length_penalty 0 a score is a plain sum near -100,
where neighbouring fp32 numbers lie 7.6e-6 apart.  It also runs the greedy ``lexicon=`` reference (tests/automaton_util.py) on every trie crop
and asserts that at least one stored crop's best beam entry is not the greedy entry (``greedy_entry`` / ``beam_entry``).

    python tests/golden/make_beam_automaton_goldens.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "manga-ocr_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import torch  # noqa: E402

import automaton_util as au  # noqa: E402
import beam_automaton_util as bau  # noqa: E402
import beam_util as bu  # noqa: E402
from make_beam_goldens import build_hf, crops, pixel_values_via_hf  # noqa: E402
from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights  # noqa: E402
from oracle.mocr_oracle import Oracle  # noqa: E402

MIN_GAP, BF16_GAP = 1e-3, 2e-2
SCORE_TOL = 3e-6
SET_LD = 64
EARLY_EOS = dict(seed=1, eos_bias=3.0)
LONG_EOS = dict(seed=1, eos_bias=1.5)
SP = DEFAULT_SPEC
POOL = np.setdiff1d(np.arange(5, SP.vocab), [SP.eos_id, SP.start_id, SP.pad_id])


def random_words(seed):
    """6 to 12 words of 4 to 12 tokens over distinct random tokens: every new word forks off an earlier one at a node that
    has fewer than three children; the root gets two or three"""
    rs = np.random.RandomState(seed)
    n_words = int(rs.randint(6, 13))
    toks = iter(int(x) for x in rs.choice(POOL, 200, replace=False))
    words = [[next(toks) for _ in range(int(rs.randint(4, 13)))]]
    kids = {(): 1}
    root = int(rs.randint(2, 4))
    while len(words) < n_words:
        w = words[int(rs.randint(len(words)))]
        d = 0 if kids[()] < root else int(rs.randint(0, len(w)))
        if kids.get(tuple(w[:d]), 1) >= 3:
            continue
        total = int(rs.randint(max(4, d + 1), 13))
        new = w[:d] + [next(toks) for _ in range(total - d)]
        kids[tuple(w[:d])] = kids.get(tuple(w[:d]), 1) + 1
        words.append(new)
    return words


def trie_of(seed):
    return au.trie(random_words(seed))


def thinning_set(aut, seed):
    """the trie's tokens minus one edge of some nodes that have a sibling edge to spare, as a sorted list"""
    rs = np.random.RandomState(seed)
    keep = {t for e in aut.trans.values() for t in e}
    for s, e in sorted(aut.trans.items()):
        if len(e) >= 2 and rs.rand() < 0.6:
            keep.discard(sorted(e)[int(rs.randint(len(e)))])
    return sorted(keep)


# name -> (K, length_penalty, early_stopping, ngram, weights, max_length, crops, min gap, automaton of crop c and seed s)
CASES = {
    "a2": (2, 2.0, True, 3, LONG_EOS, 16, 4, MIN_GAP, lambda c, s: ("trie", s)),
    "a3": (3, 2.0, True, 3, LONG_EOS, 16, 4, MIN_GAP, lambda c, s: ("trie", s)),
    "a4": (4, 2.0, True, 3, LONG_EOS, 16, 4, MIN_GAP, lambda c, s: ("trie", s)),
    "b": (3, 1.0, False, 2, LONG_EOS, 16, 4, MIN_GAP, lambda c, s: ("thin", s)),
    "c": (4, 2.0, True, 3, EARLY_EOS, 24, 4, MIN_GAP, lambda c, s: [("trie", s), ("none", s), ("two", s), ("trie", s)][c]),
    "d": (3, 1.0, False, 0, LONG_EOS, 12, 3, MIN_GAP, lambda c, s: ("loop", s)),
    "e0": (4, 0.0, True, 0, LONG_EOS, 16, 3, MIN_GAP, lambda c, s: ("trie", s)),
    "e2": (3, 2.0, True, 0, LONG_EOS, 16, 3, MIN_GAP, lambda c, s: ("trie", s)),
    "h2": (2, 2.0, True, 3, LONG_EOS, 16, 6, BF16_GAP, lambda c, s: ("trie", s)),
    "h3": (3, 2.0, True, 3, LONG_EOS, 16, 6, BF16_GAP, lambda c, s: ("trie", s)),
    "h4": (4, 2.0, True, 3, LONG_EOS, 16, 6, BF16_GAP, lambda c, s: ("trie", s)),
}
NONE_SEEDS = (100, 106, 117, 124)      # make_beam_token_goldens.py, case (a): free searches with min_gap >= 1e-3 under these settings


def automaton_of(kind, seed, max_length):
    """-> (Automaton or None, {accepting state: entry} or {}, the crop's allowed list or None)"""
    if kind == "none":
        return None, {}, None
    if kind == "loop":
        toks = [int(x) for x in np.random.RandomState(seed).choice(POOL, 3, replace=False)]
        return au.loop(toks, at_least=max_length), {}, None
    if kind == "two":
        words = random_words(seed)
        first = words[0]
        other = next(w for w in words if w[0] != first[0])
        return au.trie([first, other]) + (None,)
    aut, entry = trie_of(seed)
    return aut, entry, thinning_set(aut, seed) if kind == "thin" else None


def mask_of(allowed):
    if allowed is None:
        return np.ones(SP.vocab, bool)
    m = np.zeros(SP.vocab, bool)
    m[allowed] = True
    m[SP.eos_id] = True
    return m


def allowed_fn(aut, mask):
    def f(batch, seq):
        s = 0
        for t in seq[1:].tolist():
            s = aut.next(s, t)                  # (strict: an EOS inside the history has no edge either)
        if s < 0:
            return [SP.pad_id]
        toks = np.nonzero(aut.allowed(s) & mask)[0].tolist()
        assert toks, "a live state without a token: the case's set took too much"
        return toks
    return f


def hf_rows(m, pv, K, lp, es, ngram, max_length, aut, mask):
    ids = np.full((K, max_length), SP.pad_id, np.int32)
    lens = np.zeros(K, np.int32)
    scores = np.full(K, -1e9, np.float32)
    logp = np.zeros((K, max_length), np.float32)
    state = np.full(K, au.NONE, np.int32)
    kw = {}
    if aut is not None:
        kw["prefix_allowed_tokens_fn"] = allowed_fn(aut, mask)
    with torch.no_grad():
        g = m.generate(pixel_values=pv, max_length=max_length, num_beams=K, num_return_sequences=K, length_penalty=lp, early_stopping=es,
                       no_repeat_ngram_size=ngram, do_sample=False, return_dict_in_generate=True, output_scores=True, **kw)
        tr = m.compute_transition_scores(g.sequences, g.scores, g.beam_indices, normalize_logits=False).numpy()
    seq, sc = g.sequences.numpy(), g.sequences_scores.numpy()
    j2 = 0
    for j in range(K):
        if sc[j] <= bau.junk_below(lp, max_length):
            continue
        row = seq[j]
        hit = np.nonzero(row[1:] == SP.eos_id)[0]
        L = int(hit[0]) + 2 if hit.size else row.shape[0]
        assert hit.size or L == max_length, (j, row)
        ids[j2, :L] = row[:L]
        lens[j2] = L
        scores[j2] = sc[j]
        logp[j2, 1:L] = tr[j, :L - 1]
        if aut is not None:
            state[j2] = aut.walk(row[1:L])
        j2 += 1
    return ids, lens, scores, logp, state


def main():
    models, oracles = {}, {}
    differs = 0
    for name, (K, lp, es, ngram, wkw, ML, n_crops, min_gap, pick) in CASES.items():
        key = (tuple(sorted(wkw.items())), ML)
        if key not in models:
            kw = dict(wkw)
            models[key] = build_hf(synthetic_weights(kw.pop("seed"), **kw), ML)
        okey = tuple(sorted(wkw.items()))
        if okey not in oracles:
            kw = dict(wkw)
            oracles[okey] = Oracle(synthetic_weights(kw.pop("seed"), **kw), DEFAULT_SPEC)
        m, o = models[key], oracles[okey]
        cfg = bu.Config(K, lp, es, ngram)
        keys = ("ids", "lens", "scores", "logp", "state", "seeds", "sets", "gaps", "greedy_entry", "beam_entry")
        out = {k: [] for k in keys}
        auts = []
        seed, worst = 200, 0.0
        while len(out["seeds"]) < n_crops:
            c = len(out["seeds"])
            kind, _ = pick(c, seed)
            s = NONE_SEEDS[c] if kind == "none" else seed
            seed += 1
            aut, entry, allowed = automaton_of(kind, s, ML)
            mask = mask_of(allowed)
            gray = crops([s])
            enc = o.encode(o.preprocess_gray(gray))
            r = bau.beam_generate(o, enc, cfg, ML, [aut], mask[None])
            gap = r[5]["min_gap"][0]
            if gap < min_gap:
                assert kind != "none", f"case {name}: the fixed seed {s} has min_gap {gap}"
                print(f"   case {name} crop {c}: seed {s} passed over, min_gap {gap:.2e}", flush=True)
                continue
            want = bau.real_only(*(x[0] for x in r[:5]), lp, ML, SP.pad_id)
            ids, lens, scores, logp, state = hf_rows(m, pixel_values_via_hf(gray), K, lp, es, ngram, ML, aut, mask)
            np.testing.assert_array_equal(lens, want[1], err_msg=f"case {name} seed {s}")
            np.testing.assert_array_equal(ids, want[0], err_msg=f"case {name} seed {s}")
            np.testing.assert_array_equal(state, want[4], err_msg=f"case {name} seed {s}")
            e = max(float((np.abs(scores - want[2]) / bau.score_tol(want[2], SCORE_TOL)).max()),
                    float(np.abs(logp - want[3]).max()) / SCORE_TOL) * SCORE_TOL
            worst = max(worst, e)
            assert e <= SCORE_TOL, f"case {name} seed {s}: scores {e} (in units of the bound) from the float64 reference"
            assert lens[0] > 0 and (aut is None or state[0] >= 0)
            g_entry = b_entry = -1
            if entry:           # the greedy lexicon= answer of the same crop, and the best beam entry
                g_ids, _, _, g_state = au.automaton_generate(o, enc, [aut], mask[None], [0], ML)
                g_len = int(np.nonzero(g_ids[0] == SP.eos_id)[0][0]) + 1 if (g_ids[0] == SP.eos_id).any() else ML
                g_ok = g_ids[0, g_len - 1] == SP.eos_id and int(g_state[0]) in entry
                g_entry = entry[int(g_state[0])] if g_ok else -1
                b_entry = entry.get(int(state[0]), -1) if ids[0, lens[0] - 1] == SP.eos_id else -1
                differs += name[0] in "ah" and g_entry >= 0 and b_entry >= 0 and g_entry != b_entry
            row = np.full(SET_LD, -1, np.int32)
            if allowed is not None:
                assert len(allowed) <= SET_LD
                row[:len(allowed)] = allowed
            auts.append(aut)
            for k, v in zip(keys, (ids, lens, scores, logp, state, s, row, gap, g_entry, b_entry)):
                out[k].append(v)
        packed = au.pack_many([a for a in auts if a is not None]) if any(a is not None for a in auts) else None
        aut_of_crop, i = [], 0
        for a in auts:
            aut_of_crop.append(-1 if a is None else i)
            i += a is not None
        eb, et, en, acc, first = packed
        n_states = [a.n_states for a in auts if a is not None]
        path = os.path.join(HERE, f"beam_aut_{name}.npz")
        np.savez_compressed(path, ids=np.stack(out["ids"]), lens=np.stack(out["lens"]), scores=np.stack(out["scores"]), logp=np.stack(out["logp"]),
                            state=np.stack(out["state"]), crop_seeds=np.array(out["seeds"], np.int64), sets=np.stack(out["sets"]),
                            gaps=np.array(out["gaps"]), greedy_entry=np.array(out["greedy_entry"], np.int64),
                            beam_entry=np.array(out["beam_entry"], np.int64), aut_of_crop=np.array(aut_of_crop, np.int64),
                            edge_begin=eb, edge_token=et, edge_next=en, accepting=acc, aut_first=np.array(first, np.int64),
                            aut_states=np.array(n_states, np.int64), num_beams=np.int64(K), length_penalty=np.float64(lp),
                            early_stopping=np.int64({False: 0, True: 1, "never": 2}[es]), no_repeat_ngram_size=np.int64(ngram),
                            max_length=np.int64(ML), weights_seed=np.int64(wkw["seed"]), eos_bias=np.float64(wkw.get("eos_bias", 0.0)))
        print(f"beam_aut_{name}", os.path.getsize(path), "bytes; seeds", out["seeds"], "lens", np.stack(out["lens"]).tolist(),
              "min_gap", [f"{g:.1e}" for g in out["gaps"]], "greedy/beam entries", list(zip(out["greedy_entry"], out["beam_entry"])),
              f"scores within {worst:.1e} of float64", flush=True)
    assert differs >= 1, "no stored crop's best beam entry differs from the greedy lexicon answer: search more seeds"
    print("crops whose best beam entry is not the greedy entry:", differs)


if __name__ == "__main__":
    main()
