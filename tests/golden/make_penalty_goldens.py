#!/usr/bin/env python3
"""Generate tests/golden/penalty_*.npz from transformers' own greedy search under ``repetition_penalty``
(include/mocr.h, "repetition penalty"; ``MangaOcr(repetition_penalty=...)``).

PROVENANCE SCRIPT, like make_bias_goldens.py (whose model, crops and conventions it uses): it imports ``transformers``
(5.15.0), runs once on the build machine and nothing imports it.  Every row group is one

    generate(repetition_penalty=p, num_beams=1, do_sample=False, output_scores=True, return_dict_in_generate=True, ...)

call on a batch of crops, for p in 1.3, 2.0 and 0.8, in three files:
  penalty_alone  the penalty alone;
  penalty_ngram  with no_repeat_ngram_size=2: the ban comes AFTER the penalty, a penalised token can still be banned;
  penalty_bias   with a sequence_bias made from the free run of the file's first crop (make_bias_goldens.sequences_of,
                 "mixed"): the bias comes BEFORE the penalty, so a biased, seen token has (logit + bias) penalised.
A crop is kept when the reference loop (tests/penalty_util.py penalty_generate on the oracle's logits) sees the processed,
masked top-2 margin of every step at least MIN_GAP (1e-3) under all three p.  The script asserts that transformers and the
reference agree on every row it writes - ids and lengths exactly, the chosen tokens' log-probabilities (float64 log-softmax
of transformers' processed fp32 scores) within SCORE_TOL (3e-6) - and that on at least half of the crops of every (file, p)
the ids differ from the p = 1 decode of the same call; the share is recorded in the file (``changed`` of ``crops``).

    python tests/golden/make_penalty_goldens.py
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

import bias_util as bu  # noqa: E402
import constraint_util as cu  # noqa: E402
import penalty_util as pu  # noqa: E402
from make_beam_goldens import build_hf, crops, pixel_values_via_hf  # noqa: E402
from make_bias_goldens import sequences_of  # noqa: E402
from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights  # noqa: E402
from oracle.mocr_oracle import Oracle  # noqa: E402

MIN_GAP = 1e-3
SCORE_TOL = bu.SCORE_TOL
SP = DEFAULT_SPEC
SEQ_LD = 8
WEIGHTS = dict(seed=1, eos_bias=1.5)
ML, N_CROPS = 16, 4
PENALTIES = (1.3, 2.0, 0.8)
FIRST_SEED = {"alone": 400, "ngram": 430, "bias": 460}


def reference(o, enc, p, kind, sb_aut):
    B = enc.shape[0]
    return pu.penalty_generate(o, enc, [p] * B, ML, automata=[sb_aut] * B if kind == "bias" else None,
                               ngrams=[2] * B if kind == "ngram" else None)


def min_gap(pl, masks) -> float:
    """[T, V] processed logits and per-step masks -> the smallest top-2 margin among the allowed tokens"""
    x = cu.masked(pl, masks)
    top2 = -np.partition(-x, 1, axis=-1)[..., :2]
    with np.errstate(invalid="ignore"):
        return float(np.where(np.isneginf(top2[..., 1]), np.inf, top2[..., 0] - top2[..., 1]).min())


def main():
    kw = dict(WEIGHTS)
    w = synthetic_weights(kw.pop("seed"), **kw)
    m, o = build_hf(w, ML), Oracle(w, DEFAULT_SPEC)
    for kind, seed in FIRST_SEED.items():
        sb, aut = None, None
        if kind == "bias":
            for first in range(seed, seed + 40):
                with torch.no_grad():
                    enc0 = o.encode(o.preprocess_gray(crops([first])))
                ids0, lg0 = o.generate(enc0, max_len=ML, return_logits=True)
                if int(bu.lengths(np.asarray(ids0), SP.eos_id)[0]) >= 5:
                    break
            sb = sequences_of("mixed", np.asarray(ids0)[0], np.asarray(lg0)[0])
            aut = bu.from_sequence_bias(sb)
        hf_kw = dict(no_repeat_ngram_size=2) if kind == "ngram" else dict(sequence_bias=sb) if kind == "bias" else {}
        # crops: the margins hold under every p, and - the generator condition - the penalty changes the ids of at least
        # half of them under every p
        seeds, changed_of = [], {p: 0 for p in PENALTIES}
        while len(seeds) < N_CROPS:
            with torch.no_grad():
                enc = o.encode(o.preprocess_gray(crops([seed])))
            free = reference(o, enc, 1.0, kind, aut)[0]
            ok, diff = True, {}
            for p in PENALTIES:
                ids, pl, _, masks = reference(o, enc, p, kind, aut)
                L = int(pu.lengths(ids, SP.eos_id)[0])
                ok = ok and min_gap(pl[0, :L - 1], masks[0, :L - 1]) >= MIN_GAP
                diff[p] = ids.shape != free.shape or not np.array_equal(ids, free)
            # keep a crop the penalty leaves alone only while the other crops can still carry the condition
            short = any(changed_of[p] + int(diff[p]) + (N_CROPS - len(seeds) - 1) < (N_CROPS + 1) // 2 for p in PENALTIES)
            if ok and not short:
                seeds.append(seed)
                for p in PENALTIES:
                    changed_of[p] += int(diff[p])
            else:
                print(f"   {kind}: seed {seed} passed over (margins ok: {ok}, changed: {diff})", flush=True)
            seed += 1
        gray = crops(seeds)
        with torch.no_grad():
            enc = o.encode(o.preprocess_gray(gray))
        pv = pixel_values_via_hf(gray)
        B = len(seeds)
        out_ids = np.full((len(PENALTIES), B, ML), SP.pad_id, np.int32)
        out_len = np.zeros((len(PENALTIES), B), np.int32)
        out_logp = np.zeros((len(PENALTIES), B, ML), np.float32)
        changed = np.zeros(len(PENALTIES), np.int64)
        with torch.no_grad():
            g1 = m.generate(pixel_values=pv, max_length=ML, num_beams=1, do_sample=False, return_dict_in_generate=True, **hf_kw)
        free_seq = g1.sequences.numpy()
        free_len = bu.lengths(free_seq, SP.eos_id)
        worst = 0.0
        for k, p in enumerate(PENALTIES):
            want_ids, pl, _, masks = reference(o, enc, p, kind, aut)
            want_len = pu.lengths(want_ids, SP.eos_id)
            with torch.no_grad():
                g = m.generate(pixel_values=pv, max_length=ML, num_beams=1, do_sample=False, repetition_penalty=p, output_scores=True,
                               return_dict_in_generate=True, **hf_kw)
            seq = g.sequences.numpy()
            ids = np.full((B, ML), SP.pad_id, np.int32)
            ids[:, :seq.shape[1]] = seq
            lens = bu.lengths(ids[:, :seq.shape[1]], SP.eos_id).astype(np.int32)
            for t, sc in enumerate(g.scores):
                x = sc.double().numpy()
                mx = x.max(-1, keepdims=True)
                lp = x - (mx + np.log(np.exp(x - mx).sum(-1, keepdims=True)))
                for b in range(B):
                    if t + 1 < lens[b]:
                        out_logp[k, b, t + 1] = lp[b, ids[b, t + 1]]
            for b in range(B):
                ids[b, lens[b]:] = SP.pad_id
            np.testing.assert_array_equal(lens, want_len, err_msg=f"{kind} p={p}")
            for b in range(B):
                np.testing.assert_array_equal(ids[b, :lens[b]], want_ids[b, :lens[b]], err_msg=f"{kind} p={p} crop {b}")
                want_lp = cu.masked_log_softmax64(pl[b, :lens[b] - 1], masks[b, :lens[b] - 1])[np.arange(lens[b] - 1), ids[b, 1:lens[b]]]
                worst = max(worst, float(np.abs(out_logp[k, b, 1:lens[b]] - want_lp).max()))
                changed[k] += int(lens[b] != free_len[b] or not np.array_equal(ids[b, :lens[b]], free_seq[b, :lens[b]]))
            out_ids[k], out_len[k] = ids, lens
        assert worst <= SCORE_TOL, f"{kind}: scores {worst:.2e} from the reference"
        assert (changed * 2 >= B).all(), f"{kind}: only {changed.tolist()} of {B} crops differ from the p = 1 decode"
        extra = {}
        if sb is not None:
            keys = sorted(sb)
            seq_tok = np.full((len(keys), SEQ_LD), -1, np.int32)
            for i, key in enumerate(keys):
                seq_tok[i, :len(key)] = key
            extra = dict(seq_tok=seq_tok, seq_len=np.array([len(key) for key in keys], np.int32), seq_bias=np.array([sb[key] for key in keys], np.float64))
        path = os.path.join(HERE, f"penalty_{kind}.npz")
        np.savez_compressed(path, ids=out_ids, lens=out_len, logp=out_logp, penalties=np.array(PENALTIES, np.float64),
                            crop_seeds=np.array(seeds, np.int64), max_length=np.int64(ML), weights_seed=np.int64(WEIGHTS["seed"]),
                            eos_bias=np.float64(WEIGHTS["eos_bias"]), ngram=np.int64(2 if kind == "ngram" else 0), changed=changed,
                            crops=np.int64(B), **extra)
        print(f"penalty_{kind}", os.path.getsize(path), "bytes; seeds", seeds, "lens", out_len.tolist(),
              f"changed {changed.tolist()} of {B} per p {PENALTIES}; scores within {worst:.1e} of the reference", flush=True)


if __name__ == "__main__":
    main()
