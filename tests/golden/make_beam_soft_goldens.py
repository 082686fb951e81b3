#!/usr/bin/env python3
"""Generate tests/golden/beam_soft_*.npz from transformers' own beam search under ``sequence_bias``: beam search under soft
token automata (include/mocr.h; ``MangaOcr.search``).

PROVENANCE SCRIPT, like make_beam_automaton_goldens.py and make_bias_goldens.py (whose model, crops, sequences and conventions
it uses): it imports ``transformers`` (5.15.0), runs once on the build machine and nothing imports it.  Every crop is its own

    generate(num_beams=K, num_return_sequences=K, length_penalty, early_stopping, no_repeat_ngram_size, sequence_bias=sb,
             output_scores=True, return_dict_in_generate=True)

call; the token scores are compute_transition_scores(normalize_logits=False).  The sequences of a case are made from the free
greedy run of the case's first crop, as make_bias_goldens.py makes them (``sequences_of``): the ``mixed`` set - a negative
one-token sequence, overlapping two- and three-token sequences, a one-token sequence that adds to both - or the ``glossary`` set
in MangaOcr.glossary's form.  All biases are multiples of 1/8; max_length is 16.

Cases (name -> K, length_penalty, early_stopping, no_repeat_ngram_size; weights; sequences):
  (p2) (p3) (p4) the published settings (2.0, true, 3) at K = 2, 3, 4, the ``mixed`` sequences;
  (g) K = 3, the published settings, the ``glossary`` sequences: the reference runs the FLAT and the COMPACT (fallback)
      compilation of text.bias_automaton and the script asserts that they agree; both state columns are stored;
  (n) K = 3, length_penalty 1, no_repeat_ngram_size 2, and a per-crop token set through prefix_allowed_tokens_fn (a random half
      of the vocabulary, the sequences' tokens and EOS kept);
  (e) K = 2 on the early-EOS weights (eos_bias 1.6): rows end after a few tokens - a bias changes which hypotheses finish.
A crop is kept when the float64 reference (tests/beam_soft_util.py) sees its real candidates at least MIN_GAP (1e-3) apart;
up to SCAN seeds are tried per case, CROPS crops are stored, and a case that finds fewer than two fails.  The script asserts
that transformers and the reference agree on every crop it writes - ids, lengths and states exactly, token scores within
SCORE_TOL (3e-6), sequence scores within bau.score_tol - and that the best hypothesis of at least half of the stored crops
differs from the unbiased beam search's (``changed``).

    python tests/golden/make_beam_soft_goldens.py
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

import beam_automaton_util as bau  # noqa: E402
import beam_soft_util as bsu  # noqa: E402
import beam_util as bu  # noqa: E402
import bias_util  # noqa: E402
from make_beam_goldens import build_hf, crops, pixel_values_via_hf  # noqa: E402
from make_bias_goldens import free_run, sequences_of  # noqa: E402
from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights  # noqa: E402
from oracle.mocr_oracle import Oracle  # noqa: E402

MIN_GAP = 1e-3
SCORE_TOL = bias_util.SCORE_TOL
SCAN, CROPS = 400, 4
SEQ_LD = 8
ML = 16
SP = DEFAULT_SPEC
EARLY_EOS = dict(seed=1, eos_bias=1.6)
LONG_EOS = dict(seed=1, eos_bias=1.5)
# name -> (K, length_penalty, early_stopping, ngram, weights, the kind of its sequences, a per-crop token set, first seed)
CASES = {
    "p2": (2, 2.0, True, 3, LONG_EOS, "mixed", False, 400),
    "p3": (3, 2.0, True, 3, LONG_EOS, "mixed", False, 400),
    "p4": (4, 2.0, True, 3, LONG_EOS, "mixed", False, 400),
    "g": (3, 2.0, True, 3, LONG_EOS, "glossary", False, 400),
    "n": (3, 1.0, False, 2, LONG_EOS, "mixed", True, 400),
    "e": (2, 2.0, True, 3, EARLY_EOS, "mixed", False, 400),
}


def set_mask(seed, sb):
    """the crop's token set: a random half of the vocabulary, plus the sequences' tokens and EOS"""
    m = np.random.RandomState(seed).rand(SP.vocab) < 0.5
    for k in sb:
        m[list(k)] = True
    m[SP.eos_id] = True
    return m


def hf_rows(m, pv, K, lp, es, ngram, sb, aut, mask):
    ids = np.full((K, ML), SP.pad_id, np.int32)
    lens = np.zeros(K, np.int32)
    scores = np.full(K, -1e9, np.float32)
    logp = np.zeros((K, ML), np.float32)
    state = np.full(K, bsu.NONE, np.int32)
    kw = {}
    if mask is not None:
        allowed = np.nonzero(mask)[0].tolist()
        kw["prefix_allowed_tokens_fn"] = lambda batch, seq: allowed
    with torch.no_grad():
        g = m.generate(pixel_values=pv, max_length=ML, num_beams=K, num_return_sequences=K, length_penalty=lp, early_stopping=es,
                       no_repeat_ngram_size=ngram, do_sample=False, return_dict_in_generate=True, output_scores=True,
                       sequence_bias={tuple(int(t) for t in k): float(b) for k, b in sb.items()}, **kw)
        tr = m.compute_transition_scores(g.sequences, g.scores, g.beam_indices, normalize_logits=False).numpy()
    seq, sc = g.sequences.numpy(), g.sequences_scores.numpy()
    j2 = 0
    for j in range(K):
        if sc[j] <= bau.junk_below(lp, ML):
            continue
        row = seq[j]
        hit = np.nonzero(row[1:] == SP.eos_id)[0]
        L = int(hit[0]) + 2 if hit.size else row.shape[0]
        assert hit.size or L == ML, (j, row)
        ids[j2, :L] = row[:L]
        lens[j2] = L
        scores[j2] = sc[j]
        logp[j2, 1:L] = tr[j, :L - 1]
        state[j2] = aut.walk(row[1:L])
        j2 += 1
    return ids, lens, scores, logp, state


def main():
    models, oracles = {}, {}
    for name, (K, lp, es, ngram, wkw, kind, with_set, first_seed) in CASES.items():
        okey = tuple(sorted(wkw.items()))
        if okey not in oracles:
            kw = dict(wkw)
            w = synthetic_weights(kw.pop("seed"), **kw)
            models[okey], oracles[okey] = build_hf(w, ML), Oracle(w, DEFAULT_SPEC)
        m, o = models[okey], oracles[okey]
        cfg = bu.Config(K, lp, es, ngram)
        for first in range(first_seed, first_seed + 40):     # the crop the sequences are made from: the first whose free run has three tokens
            with torch.no_grad():
                enc0 = o.encode(o.preprocess_gray(crops([first])))
            ids0, lg0 = free_run(o, enc0, ML)
            if int(bias_util.lengths(ids0, SP.eos_id)[0]) >= 5:
                break
        sb = sequences_of(kind, ids0[0], lg0[0])
        assert all(SP.eos_id not in k for k in sb) and all(float(b) * 8 == int(float(b) * 8) for b in sb.values())
        aut = bias_util.from_sequence_bias(sb)
        compact = bias_util.from_sequence_bias(sb, compact=True) if name == "g" else None
        keys = ("ids", "lens", "scores", "logp", "state", "state_compact", "seeds", "gaps", "set_bits", "changed")
        out = {k: [] for k in keys}
        worst, tried = 0.0, 0
        for seed in range(first_seed, first_seed + SCAN):
            if len(out["seeds"]) >= CROPS:
                break
            tried += 1
            gray = crops([seed])
            mask = set_mask(seed, sb) if with_set else None
            with torch.no_grad():
                enc = o.encode(o.preprocess_gray(gray))
            r = bsu.beam_generate(o, enc, cfg, ML, [aut], None if mask is None else mask[None])
            gap = float(r[5]["min_gap"][0])
            if gap < MIN_GAP:
                continue
            want = bsu.real_only(*(x[0] for x in r[:5]), lp, ML, SP.pad_id)
            st_c = want[4]
            if compact is not None:     # the compact form, walked with the fallback rule: the same search, its own state numbers
                rc = bsu.beam_generate(o, enc, cfg, ML, [compact], None)
                wc = bsu.real_only(*(x[0] for x in rc[:5]), lp, ML, SP.pad_id)
                for a, b in zip(want[:4], wc[:4]):
                    np.testing.assert_array_equal(a, b, err_msg=f"case {name} seed {seed}: flat and compact forms differ")
                st_c = wc[4]
            ids, lens, scores, logp, state = hf_rows(m, pixel_values_via_hf(gray), K, lp, es, ngram, sb, aut, mask)
            np.testing.assert_array_equal(lens, want[1], err_msg=f"case {name} seed {seed}")
            np.testing.assert_array_equal(ids, want[0], err_msg=f"case {name} seed {seed}")
            np.testing.assert_array_equal(state, want[4], err_msg=f"case {name} seed {seed}")
            e = max(float((np.abs(scores - want[2]) / bsu.score_tol(want[2], SCORE_TOL)).max()),
                    float(np.abs(logp - want[3]).max()) / SCORE_TOL) * SCORE_TOL
            worst = max(worst, e)
            assert e <= SCORE_TOL, f"case {name} seed {seed}: scores {e} (in units of the bound) from the float64 reference"
            assert lens[0] > 0 and state[0] >= 0
            free = bau.beam_generate(o, enc, cfg, ML, None, None if mask is None else mask[None])
            changed = not (free[1][0, 0] == lens[0] and np.array_equal(free[0][0, 0, :lens[0]], ids[0, :lens[0]]))
            bits = np.packbits(np.ones(SP.vocab, bool) if mask is None else mask)
            for k, v in zip(keys, (ids, lens, scores, logp, state, st_c, seed, gap, bits, changed)):
                out[k].append(v)
            print(f"   case {name}: seed {seed} kept, min_gap {gap:.2e}, changed {changed}", flush=True)
        n = len(out["seeds"])
        assert n >= 2, f"case {name}: {n} qualifying crops among {tried} seeds"
        assert sum(out["changed"]) * 2 >= n, f"case {name}: only {sum(out['changed'])} of {n} best hypotheses differ from the unbiased search"
        skeys = sorted(sb)
        seq_tok = np.full((len(skeys), SEQ_LD), -1, np.int32)
        for i, k in enumerate(skeys):
            seq_tok[i, :len(k)] = k
        path = os.path.join(HERE, f"beam_soft_{name}.npz")
        np.savez_compressed(path, ids=np.stack(out["ids"]), lens=np.stack(out["lens"]), scores=np.stack(out["scores"]), logp=np.stack(out["logp"]),
                            state=np.stack(out["state"]), state_compact=np.stack(out["state_compact"]),
                            crop_seeds=np.array(out["seeds"], np.int64), gaps=np.array(out["gaps"]), set_bits=np.stack(out["set_bits"]),
                            with_set=np.int64(with_set), changed=np.array(out["changed"], np.int64), seq_tok=seq_tok,
                            seq_len=np.array([len(k) for k in skeys], np.int32), seq_bias=np.array([sb[k] for k in skeys], np.float64),
                            compact=np.int64(compact is not None), num_beams=np.int64(K), length_penalty=np.float64(lp),
                            early_stopping=np.int64({False: 0, True: 1, "never": 2}[es]), no_repeat_ngram_size=np.int64(ngram),
                            max_length=np.int64(ML), weights_seed=np.int64(wkw["seed"]), eos_bias=np.float64(wkw.get("eos_bias", 0.0)))
        print(f"beam_soft_{name}", os.path.getsize(path), "bytes; seeds", out["seeds"], f"of {tried} tried; lens", np.stack(out["lens"]).tolist(),
              "min_gap", [f"{g:.1e}" for g in out["gaps"]], f"{sum(out['changed'])} of {n} best hypotheses differ from the unbiased search;",
              f"scores within {worst:.1e} of float64; {len(sb)} sequences, {aut.n_states} states", flush=True)


if __name__ == "__main__":
    main()
