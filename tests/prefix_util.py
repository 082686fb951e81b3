"""Reference helpers of the forced-prefix tests (tests/test_prefix_cpu.py, tests/test_gpu_prefix.py).

A row with a prefix p[0 .. P-1] holds ids[0] = start, ids[1 + i] = p[i] for i < P and greedy tokens after that (include/mocr.h,
"forced prefixes").  The step that fills ids[t + 1] with t < P runs like any other; only the token that is stored and fed
back differs.  Here: that loop on the fp32 oracle, in the style of ngram_util.ngram_generate, and the float64 score of a
stored token."""
import numpy as np

import constraint_util as cu
import ngram_util as nu

V, EOS = cu.V, cu.EOS


def prefix_generate(o, enc, prefixes, base_masks, ngrams, max_len: int):
    """ngram_util.ngram_generate with forced prefixes: prefixes = per row a sequence of token ids or None, base_masks bool
    [B, V] (None: everything), ngrams int [B] (None: all 0).  A live row's step t < len(prefix) stores prefix[t] instead of the
    arg-max over its effective set; a forced EOS or reaching max_len finishes the row as usual.
    -> (ids int64 [B, L], the fp32 logits of every step [B, L - 1, V] unmasked, the effective sets of every step bool
    [B, L - 1, V])"""
    import torch
    sp = o.spec
    B = enc.shape[0]
    base = np.ones((B, V), bool) if base_masks is None else np.asarray(base_masks, bool)
    ngrams = np.zeros(B, np.int64) if ngrams is None else np.asarray(ngrams)
    pre = [[] if p is None else [int(t) for t in p] for p in prefixes]
    with torch.no_grad():
        ckv = o.cross_kv(enc)
        self_kv = [None] * sp.dec_layers
        ids = torch.full((B, 1), sp.start_id, dtype=torch.int64)
        unfinished = torch.ones(B, dtype=torch.int64)
        logits_all, masks_all = [], []
        t = 0
        while True:
            logits = o.decode_step(ids[:, -1], t, self_kv, ckv)
            logits_all.append(logits)
            hist = ids.numpy()
            mk = np.stack([nu.step_mask(hist[b], int(ngrams[b]), base[b]) if int(unfinished[b]) else base[b] for b in range(B)])
            masks_all.append(mk)
            nxt = torch.argmax(torch.where(torch.from_numpy(mk), logits, torch.full_like(logits, float("-inf"))), dim=-1)
            for b in range(B):
                if t < len(pre[b]):
                    nxt[b] = pre[b][t]
            nxt = nxt * unfinished + sp.pad_id * (1 - unfinished)
            ids = torch.cat((ids, nxt[:, None]), dim=1)
            done = (nxt == sp.eos_id) | (ids.shape[1] >= max_len)
            unfinished = unfinished & (~done).long()
            t += 1
            if int(unfinished.max()) == 0:
                break
    return ids.numpy(), torch.stack(logits_all, dim=1).numpy(), np.stack(masks_all, axis=1)


def stored_logp64(logits, masks, ids, lens) -> np.ndarray:
    """float64 [B, L]: position t + 1 = the masked log-softmax of step t at the STORED token ids[:, t + 1] (-inf when the
    effective set leaves it out), 0 at position 0 and behind a row's end"""
    ids = np.asarray(ids)
    B, L = ids.shape[0], logits.shape[1] + 1
    out = np.zeros((B, L))
    for b in range(B):
        for t in range(1, min(int(lens[b]), L)):
            out[b, t] = cu.masked_log_softmax64(logits[b, t - 1], masks[b, t - 1])[int(ids[b, t])]
    return out


def runner_up(logits, masks=None) -> np.ndarray:
    """[..., V] logits -> the token with the second largest (allowed) logit"""
    x = np.asarray(logits, np.float64) if masks is None else cu.masked(logits, masks)
    return np.argsort(-x, axis=-1, kind="stable")[..., 1]
