#!/usr/bin/env python3
"""Generate tests/golden/beam_tok_*.npz from transformers' own beam search under ``prefix_allowed_tokens_fn``, with the
transition scores of every hypothesis.

PROVENANCE SCRIPT, like make_beam_goldens.py (whose model, crops and conventions it uses): it imports ``transformers``
(5.15.0), runs once on the build machine and nothing imports it.  Every crop is its own

    generate(num_beams=K, num_return_sequences=K, length_penalty, early_stopping, no_repeat_ngram_size,
             prefix_allowed_tokens_fn=lambda b, ids: allowed, output_scores=True, return_dict_in_generate=True)

call, and ``compute_transition_scores(sequences, scores, beam_indices, normalize_logits=False)`` gives the processed
log-probability of every token of every returned hypothesis.  EOS is a member of every ``allowed`` list, as the engine
guarantees for its token sets.

Cases (name -> K, length_penalty, early_stopping, no_repeat_ngram_size, sets):
  (a) the published config (4, 2.0, True, 3), no set - the crops of beam_a.npz;
  (b) K = 2 and (c) K = 4 under one random set of 40 tokens;
  (d) K = 3, a set of 12 tokens together with no_repeat_ngram_size = 2;
  (e) K = 3, a different set per crop - 40 tokens, ALL, 12 tokens, another 40 - which the engine decodes in one call.
(b)-(e) run on ``synthetic_weights(1, eos_bias=1.5)``: under a set the EOS bias weighs more (the log_softmax is over the full
row, but only the set's tokens compete with EOS), so searches still end within max_length 16.

Seeds.  A crop is ``RandomState(seed).randint(0, 256, (224, 224))``.  For (b)-(e) the seeds are picked at generation time,
from 100 upwards, by the float64 reference (tests/beam_token_util.py): a crop is taken when its smallest candidate gap
(``min_gap``) is at least 1e-3, the threshold of make_beam_goldens.py; a crop that does not clear it is passed over for the
next seed.  The script then asserts that transformers and the reference agree on every crop it writes.  Seeds and sets are
stored in the files (``crop_seeds``; ``sets`` int32 [n, 40], -1 padded, a row of -1: no set).

    python tests/golden/make_beam_token_goldens.py
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

import beam_token_util as tu  # noqa: E402
import beam_util as bu  # noqa: E402
from make_beam_goldens import build_hf, crops, pixel_values_via_hf  # noqa: E402
from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights  # noqa: E402
from oracle.mocr_oracle import Oracle  # noqa: E402

MIN_GAP = 1e-3
SET_LD = 40
EARLY_EOS = dict(seed=1, eos_bias=3.0)
LONG_EOS = dict(seed=1, eos_bias=1.5)


def random_set(seed, size):
    sp = DEFAULT_SPEC
    pool = np.setdiff1d(np.arange(5, sp.vocab), [sp.eos_id, sp.start_id, sp.pad_id])
    return sorted(int(x) for x in np.random.RandomState(seed).choice(pool, size, replace=False))


S40, S40B, S12 = random_set(40, 40), random_set(41, 40), random_set(12, 12)
# name -> (K, length_penalty, early_stopping, ngram, weights, max_length, the crops' sets in turn (None: no set), crops, fixed seeds)
CASES = {
    "a": (4, 2.0, True, 3, EARLY_EOS, 24, [None], 4, (100, 106, 117, 124)),
    "b": (2, 1.0, False, 0, LONG_EOS, 16, [S40], 4, None),
    "c": (4, 2.0, True, 0, LONG_EOS, 16, [S40], 4, None),
    "d": (3, 1.0, "never", 2, LONG_EOS, 16, [S12], 4, None),
    "e": (3, 1.0, False, 0, LONG_EOS, 16, [S40, None, S12, S40B], 4, None),
}


def mask_of(allowed):
    if allowed is None:
        return np.ones(DEFAULT_SPEC.vocab, bool)
    m = np.zeros(DEFAULT_SPEC.vocab, bool)
    m[allowed] = True
    m[DEFAULT_SPEC.eos_id] = True
    return m


def hf_rows(m, pv, K, lp, es, ngram, max_length, allowed):
    sp = DEFAULT_SPEC
    ids = np.full((K, max_length), sp.pad_id, np.int32)
    lens = np.zeros(K, np.int32)
    scores = np.full(K, -1e9, np.float32)
    logp = np.zeros((K, max_length), np.float32)
    kw = {}
    if allowed is not None:
        full = sorted(set(allowed) | {sp.eos_id})
        kw["prefix_allowed_tokens_fn"] = lambda b, seq: full
    with torch.no_grad():
        g = m.generate(pixel_values=pv, max_length=max_length, num_beams=K, num_return_sequences=K, length_penalty=lp, early_stopping=es,
                       no_repeat_ngram_size=ngram, do_sample=False, return_dict_in_generate=True, output_scores=True, **kw)
        tr = m.compute_transition_scores(g.sequences, g.scores, g.beam_indices, normalize_logits=False).numpy()
    seq, sc = g.sequences.numpy(), g.sequences_scores.numpy()
    for j in range(K):
        if sc[j] <= -1e8:
            continue
        row = seq[j]
        hit = np.nonzero(row[1:] == sp.eos_id)[0]
        L = int(hit[0]) + 2 if hit.size else row.shape[0]
        assert hit.size or L == max_length, (j, row)
        ids[j, :L] = row[:L]
        lens[j] = L
        scores[j] = sc[j]
        logp[j, 1:L] = tr[j, :L - 1]
    return ids, lens, scores, logp


def main():
    models, oracles = {}, {}
    for name, (K, lp, es, ngram, wkw, ML, sets, n_crops, fixed) in CASES.items():
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
        out = dict(ids=[], lens=[], scores=[], logp=[], seeds=[], sets=[], gaps=[])
        seed = 100
        while len(out["seeds"]) < n_crops:
            c = len(out["seeds"])
            s = fixed[c] if fixed else seed
            seed += 1
            allowed = sets[c % len(sets)]
            gray = crops([s])
            enc = o.encode(o.preprocess_gray(gray))
            r_ids, r_lens, r_scores, r_logp, info = tu.beam_generate(o, enc, cfg, ML, mask_of(allowed)[None])
            if info["min_gap"][0] < MIN_GAP:
                assert not fixed, f"case {name}: the fixed seed {s} has min_gap {info['min_gap'][0]}"
                print(f"   case {name} crop {c}: seed {s} passed over, min_gap {info['min_gap'][0]:.2e}", flush=True)
                continue
            ids, lens, scores, logp = hf_rows(m, pixel_values_via_hf(gray), K, lp, es, ngram, ML, allowed)
            np.testing.assert_array_equal(lens, r_lens[0])
            np.testing.assert_array_equal(ids, r_ids[0])
            assert np.abs(scores - r_scores[0]).max() <= 1e-4 and np.abs(logp - r_logp[0]).max() <= 1e-4
            row = np.full(SET_LD, -1, np.int32)
            if allowed is not None:
                row[:len(allowed)] = allowed
            for k, v in zip(("ids", "lens", "scores", "logp", "seeds", "sets", "gaps"), (ids, lens, scores, logp, s, row, info["min_gap"][0])):
                out[k].append(v)
        path = os.path.join(HERE, f"beam_tok_{name}.npz")
        np.savez_compressed(path, ids=np.stack(out["ids"]), lens=np.stack(out["lens"]), scores=np.stack(out["scores"]), logp=np.stack(out["logp"]),
                            crop_seeds=np.array(out["seeds"], np.int64), sets=np.stack(out["sets"]), num_beams=np.int64(K),
                            length_penalty=np.float64(lp), early_stopping=np.int64({False: 0, True: 1, "never": 2}[es]),
                            no_repeat_ngram_size=np.int64(ngram), max_length=np.int64(ML), weights_seed=np.int64(wkw["seed"]),
                            eos_bias=np.float64(wkw.get("eos_bias", 0.0)))
        print(f"beam_tok_{name}", os.path.getsize(path), "bytes; seeds", out["seeds"], "lens", np.stack(out["lens"]).tolist(),
              "min_gap", [f"{g:.1e}" for g in out["gaps"]], flush=True)


if __name__ == "__main__":
    main()
