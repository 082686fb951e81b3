"""Numpy reference helpers of the repetition-penalty tests (tests/test_penalty_cpu.py, tests/test_gpu_penalty*.py).

The rule is transformers' RepetitionPenaltyLogitsProcessor under greedy search (include/mocr.h, "repetition penalty"), per row
with its own p: at the step that chooses ids[t + 1], every token at positions 0 .. t of the row - the start token, forced
prefix tokens, chosen tokens - has its logit v replaced by v * p where v < 0 and by v / p otherwise.  It sits behind
sequence_bias (tests/bias_util.py: a soft automaton's edge weights) and in front of the bans (token sets, n-gram bans,
automaton sets).  Written here the way transformers writes it - gather the row's tokens, where(), scatter - and not with the
bitmaps of the kernels."""
import numpy as np

import automaton_util as au
import bias_util as bu

V, EOS = au.V, au.EOS
NONE = au.NONE


def pen32(logits, seen, p) -> np.ndarray:
    """the engine's expression: fp32 logits, bool `seen` of the same shape, p broadcastable -> float32, v < 0 ? v * p : v / p
    where seen - one IEEE float32 multiply or divide, which numpy's float32 arithmetic is too"""
    v = np.asarray(logits, np.float32)
    p = np.broadcast_to(np.asarray(p, np.float32), v.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(v < 0, v * p, v / p)
    return np.where(np.asarray(seen, bool), out, v).astype(np.float32)


def penalise(logits, row, p: float, dtype=np.float32) -> np.ndarray:
    """the rule on one step's logits [V] after the row's tokens `row` (start token included), as transformers states it:
    score = gather(logits, row); score = where(score < 0, score * p, score / p); scatter.  dtype float64: the float64 reference"""
    out = np.array(logits, dtype, copy=True)
    toks = np.unique(np.asarray(list(row), np.int64))
    s = out[toks]
    out[toks] = np.where(s < 0, s * dtype(p), s / dtype(p))
    return out


def seen_of(row, vocab: int = V) -> np.ndarray:
    m = np.zeros(vocab, bool)
    m[np.asarray(list(row), np.int64)] = True
    return m


def penalty_generate(o, enc, penalties, max_len: int, automata=None, base_masks=None, ngrams=None, prefixes=None):
    """bias_util.soft_generate with the penalty applied between the edge weights and the masks.  penalties: one p per row;
    automata / base_masks / ngrams / prefixes as there (None: none / everything / 0 / none).
    -> (ids int64 [B, L], the PROCESSED fp32 logits of every step [B, L - 1, V] - weights added, penalised, unmasked -, the raw
    ones, the masks bool [B, L - 1, V])"""
    import torch
    sp = o.spec
    B = enc.shape[0]
    automata = [None] * B if automata is None else list(automata)
    base = np.ones((B, sp.vocab), bool) if base_masks is None else np.asarray(base_masks, bool)
    ngrams = [0] * B if ngrams is None else list(ngrams)
    state = [NONE if a is None else 0 for a in automata]
    with torch.no_grad():
        ckv = o.cross_kv(enc)
        self_kv = [None] * sp.dec_layers
        ids = torch.full((B, 1), sp.start_id, dtype=torch.int64)
        unfinished = torch.ones(B, dtype=torch.int64)
        processed_all, plain_all, masks_all = [], [], []
        t = 0
        while True:
            logits = o.decode_step(ids[:, -1], t, self_kv, ckv)
            plain_all.append(logits)
            hist = ids.numpy()
            pl = torch.from_numpy(np.stack([penalise(bu.step_logits(automata[b], state[b], logits[b].numpy()), hist[b], float(penalties[b]))
                                            for b in range(B)]))
            processed_all.append(pl)
            mk = np.stack([au.step_mask(automata[b], state[b], hist[b], int(ngrams[b]), base[b]) if int(unfinished[b]) else base[b]
                           for b in range(B)])
            masks_all.append(mk)
            nxt = torch.argmax(torch.where(torch.from_numpy(mk), pl, torch.full_like(pl, float("-inf"))), dim=-1)
            if prefixes is not None:
                for b in range(B):
                    if prefixes[b] is not None and t < len(prefixes[b]):
                        nxt[b] = int(prefixes[b][t])
            nxt = nxt * unfinished + sp.pad_id * (1 - unfinished)
            for b in range(B):
                if int(unfinished[b]) and automata[b] is not None and int(nxt[b]) != sp.eos_id:
                    state[b] = automata[b].next(state[b], int(nxt[b]))
            ids = torch.cat((ids, nxt[:, None]), dim=1)
            done = (nxt == sp.eos_id) | (ids.shape[1] >= max_len)
            unfinished = unfinished & (~done).long()
            t += 1
            if int(unfinished.max()) == 0:
                break
    return ids.numpy(), torch.stack(processed_all, dim=1).numpy(), torch.stack(plain_all, dim=1).numpy(), np.stack(masks_all, axis=1)


lengths = bu.lengths
