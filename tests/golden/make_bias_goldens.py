#!/usr/bin/env python3
"""Generate tests/golden/bias_*.npz from transformers' own greedy search under ``sequence_bias``: soft token automata
(include/mocr.h, "soft token automata"; ``MangaOcr.sequence_bias``).

PROVENANCE SCRIPT, like make_beam_automaton_goldens.py (whose model, crops and conventions it uses): it imports
``transformers`` (5.15.0), runs once on the build machine and nothing imports it.  Every case is one

    generate(sequence_bias=..., num_beams=1, do_sample=False, output_scores=True, return_dict_in_generate=True)

call on a batch of crops.  The sequences of a case are made from what the unbiased greedy run of its crops emits, so that
they fire: with f the free run of the case's first crop and r(t) the runner-up of its step t,
  (a) a NEGATIVE one-token sequence on the free run's most frequent token; a two-token sequence (f1, r(2)) and a
      three-token sequence that ends in the same two tokens - OVERLAPPING: both complete on the same token, their biases add -
      and a one-token sequence on r(2) that adds to both;
  (b) a glossary in MangaOcr.glossary's form: every prefix of two or more tokens of three "names" made of runner-ups;
  (e) case (a)'s kinds on the early-EOS weights: rows end after a few tokens, one of them because a sequence ends in EOS's
      runner-up position being overtaken - a bias changes WHERE a row ends, too.
All biases are multiples of 1/8.  A crop is kept when the reference loop (tests/bias_util.py soft_generate on the oracle's
logits) sees the weighted top-2 margin of every step at least MIN_GAP (1e-3); the script asserts that transformers and the
reference agree on every row it writes - ids and lengths exactly, the chosen tokens' log-probabilities (float64 log-softmax of
transformers' processed fp32 scores) within SCORE_TOL (3e-6) - and that at least half of the rows differ from their free run.

bias_vectors.npz is the rule itself, frozen: SequenceBiasLogitsProcessor's bias vector (tests/bias_util.py hf_bias_vector)
at every step of a random history, for N_VEC random sets of sequences over 6 tokens - what the CPU test compares
``text.bias_automaton`` with where transformers is not installed.

    python tests/golden/make_bias_goldens.py            (everything)
    python tests/golden/make_bias_goldens.py vectors    (bias_vectors.npz alone)
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
import score_util as su  # noqa: E402
from make_beam_goldens import build_hf, crops, pixel_values_via_hf  # noqa: E402
from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights  # noqa: E402
from oracle.mocr_oracle import Oracle  # noqa: E402

MIN_GAP = 1e-3
SCORE_TOL = bu.SCORE_TOL
SP = DEFAULT_SPEC
SEQ_LD = 8
EARLY_EOS = dict(seed=1, eos_bias=1.6)
LONG_EOS = dict(seed=1, eos_bias=1.5)
# name -> (weights, max_length, crops wanted, the kind of its sequences)
CASES = {"a": (LONG_EOS, 16, 6, "mixed"), "b": (LONG_EOS, 16, 6, "glossary"), "e": (EARLY_EOS, 24, 6, "mixed")}
FIRST_SEED = {"a": 300, "b": 320, "e": 340}


def free_run(o, enc, ML):
    ids, logits = o.generate(enc, max_len=ML, return_logits=True)
    return np.asarray(ids), np.asarray(logits)


def runner_up(logits_row, taken):
    order = np.argsort(-logits_row, kind="stable")
    return int(next(t for t in order if int(t) not in taken))


def sequences_of(kind, ids, logits):
    """the case's sequence_bias from the free run of its first crop (ids [L], logits [L - 1, V])"""
    special = {SP.eos_id, SP.start_id, SP.pad_id, 1, 4}
    L = int(bu.lengths(ids[None], SP.eos_id)[0])
    f = [int(t) for t in ids[1:L] if int(t) != SP.eos_id]
    assert len(f) >= 3, "the free run is too short to make sequences from"
    r = [runner_up(logits[t], special | {f[t] if t < len(f) else -1}) for t in range(min(len(f), 6))]
    if kind == "mixed":
        common = int(np.bincount(f).argmax())
        sb = {(common,): -2.5, (f[0], r[1]): 4.0, (SP.vocab - 7, f[0], r[1]): 1.25, (r[1],): 0.375, (f[0], f[1], r[2]): 3.5}
        sb[(r[1], r[2])] = 2.0
        return sb
    names = [[f[0], r[1], r[2], r[3]], [f[0], r[1], f[2]], [r[0], f[1], r[2]]]
    sb = {}
    for nm in names:
        for n in range(2, len(nm) + 1):
            sb[tuple(nm[:n])] = 3.0
    return sb


def main():
    models, oracles = {}, {}
    for name, (wkw, ML, n_crops, kind) in CASES.items():
        key = (tuple(sorted(wkw.items())), ML)
        if key not in models:
            kw = dict(wkw)
            models[key] = build_hf(synthetic_weights(kw.pop("seed"), **kw), ML)
        okey = tuple(sorted(wkw.items()))
        if okey not in oracles:
            kw = dict(wkw)
            oracles[okey] = Oracle(synthetic_weights(kw.pop("seed"), **kw), DEFAULT_SPEC)
        m, o = models[key], oracles[okey]
        seed = FIRST_SEED[name]
        for first in range(seed, seed + 40):        # the crop the sequences are made from: the first whose free run has three tokens
            with torch.no_grad():
                enc0 = o.encode(o.preprocess_gray(crops([first])))
            ids0, lg0 = free_run(o, enc0, ML)
            if int(bu.lengths(ids0, SP.eos_id)[0]) >= 5:
                break
        sb = sequences_of(kind, ids0[0], lg0[0])
        assert all(SP.eos_id not in k for k in sb) and all(float(b) * 8 == int(float(b) * 8) for b in sb.values())
        aut = bu.from_sequence_bias(sb)
        seeds, worst = [], 0.0
        while len(seeds) < n_crops:
            with torch.no_grad():
                enc = o.encode(o.preprocess_gray(crops([seed])))
            ids, wl, pl, masks, _, _ = bu.soft_generate(o, enc, [aut], np.ones((1, SP.vocab), bool), [0], ML)
            L = int(bu.lengths(ids, SP.eos_id)[0])
            gap = float(cu.masked_gaps(wl[:, :L - 1], masks[:, 0])[0].min())
            if gap >= MIN_GAP:
                seeds.append(seed)
            else:
                print(f"   case {name}: seed {seed} passed over, weighted margin {gap:.2e}", flush=True)
            seed += 1
        gray = crops(seeds)
        with torch.no_grad():
            enc = o.encode(o.preprocess_gray(gray))
        B = len(seeds)
        want_ids, wl, pl, masks, want_state, _ = bu.soft_generate(o, enc, [aut] * B, np.ones((B, SP.vocab), bool), [0] * B, ML)
        free_ids, _ = free_run(o, enc, ML)
        want_len = bu.lengths(want_ids, SP.eos_id)
        with torch.no_grad():
            g = m.generate(pixel_values=pixel_values_via_hf(gray), max_length=ML, num_beams=1, do_sample=False, sequence_bias=sb,
                           output_scores=True, return_dict_in_generate=True)
        seq = g.sequences.numpy()
        ids = np.full((B, ML), SP.pad_id, np.int32)
        ids[:, :seq.shape[1]] = seq
        lens = bu.lengths(ids[:, :seq.shape[1]], SP.eos_id).astype(np.int32)
        logp = np.zeros((B, ML), np.float32)
        for t, sc in enumerate(g.scores):
            lp = su.log_softmax64(sc.numpy())
            for b in range(B):
                if t + 1 < lens[b]:
                    logp[b, t + 1] = lp[b, ids[b, t + 1]]
        for b in range(B):
            ids[b, lens[b]:] = SP.pad_id
        ref = np.full((B, ML), SP.pad_id, np.int64)
        ref[:, :want_ids.shape[1]] = want_ids
        np.testing.assert_array_equal(lens, want_len, err_msg=f"case {name}")
        for b in range(B):
            np.testing.assert_array_equal(ids[b, :lens[b]], ref[b, :lens[b]], err_msg=f"case {name} crop {b}")
            want_lp = su.log_softmax64(wl[b, :lens[b] - 1])[np.arange(lens[b] - 1), ids[b, 1:lens[b]]]
            worst = max(worst, float(np.abs(logp[b, 1:lens[b]] - want_lp).max()))
        assert worst <= SCORE_TOL, f"case {name}: scores {worst:.2e} from the reference"
        L = min(free_ids.shape[1], ML)
        changed = sum(1 for b in range(B) if not np.array_equal(np.pad(free_ids[b, :L], (0, ML - L))[:lens[b]], ids[b, :lens[b]]))
        assert changed * 2 >= B, f"case {name}: only {changed} of {B} rows differ from their free run"
        early = int((lens < ML).sum())
        assert name != "e" or early >= B // 2, "the early-EOS case has no early rows"
        keys = sorted(sb)
        seq_tok = np.full((len(keys), SEQ_LD), -1, np.int32)
        for i, k in enumerate(keys):
            seq_tok[i, :len(k)] = k
        path = os.path.join(HERE, f"bias_{name}.npz")
        np.savez_compressed(path, ids=ids, lens=lens, logp=logp, crop_seeds=np.array(seeds, np.int64), seq_tok=seq_tok,
                            seq_len=np.array([len(k) for k in keys], np.int32), seq_bias=np.array([sb[k] for k in keys], np.float64),
                            state=want_state.astype(np.int32), max_length=np.int64(ML), weights_seed=np.int64(wkw["seed"]),
                            eos_bias=np.float64(wkw.get("eos_bias", 0.0)), changed=np.int64(changed))
        print(f"bias_{name}", os.path.getsize(path), "bytes; seeds", seeds, "lens", lens.tolist(), f"{changed} of {B} rows differ from the free run;",
              f"{early} end early; scores within {worst:.1e} of the reference; {len(sb)} sequences, {aut.n_states} states", flush=True)


N_VEC, VEC_STEPS, VEC_TOKENS, VEC_VOCAB = 60, 12, 6, 64


def vectors():
    rs = np.random.RandomState(17)
    seq_tok = np.full((N_VEC, 8, 4), -1, np.int32)
    seq_bias = np.zeros((N_VEC, 8), np.float64)
    hist = rs.randint(0, VEC_TOKENS, size=(N_VEC, VEC_STEPS)).astype(np.int32)
    vec = np.zeros((N_VEC, VEC_STEPS, VEC_VOCAB), np.float32)
    for k in range(N_VEC):
        sb = {}
        for _ in range(rs.randint(1, 9)):
            sb[tuple(int(t) for t in rs.randint(0, VEC_TOKENS, size=rs.randint(1, 5)))] = int(rs.randint(-40, 41)) / 8.0
        for i, (key, b) in enumerate(sorted(sb.items())):
            seq_tok[k, i, :len(key)] = key
            seq_bias[k, i] = b
        for step in range(VEC_STEPS):
            vec[k, step] = bu.hf_bias_vector(sb, hist[k, :step], VEC_VOCAB)
    path = os.path.join(HERE, "bias_vectors.npz")
    np.savez_compressed(path, seq_tok=seq_tok, seq_bias=seq_bias, hist=hist, vec=vec)
    print("bias_vectors", os.path.getsize(path), "bytes;", N_VEC, "sets,", int(np.count_nonzero(vec.any(-1))), "steps at which a sequence fires", flush=True)


if __name__ == "__main__":
    if sys.argv[1:] != ["vectors"]:
        main()
    vectors()
