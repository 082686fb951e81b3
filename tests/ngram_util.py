"""Float64 / numpy reference helpers of the no-repeat n-gram tests (tests/test_ngram_cpu.py, tests/test_gpu_ngram.py).

The rule is transformers' NoRepeatNGramLogitsProcessor under greedy search (include/mocr.h, "no-repeat n-grams"): with L
tokens in the row, the step that chooses ids[L] bans every token that followed an earlier occurrence of the row's last
n - 1 tokens.  Written here the way transformers writes it - a dictionary from every (n - 1)-gram of the row to the tokens
that followed it, looked up with the last n - 1 tokens - and not with the window arithmetic of the kernel."""
import numpy as np

import constraint_util as cu

V, EOS = cu.V, cu.EOS


def banned_tokens(row, n: int):
    """row: the L tokens the row holds (start token included) -> the sorted token ids banned at the step that chooses
    ids[L]; n = 0: none."""
    row = [int(t) for t in row]
    L = len(row)
    if n <= 0 or L + 1 < n:
        return []
    followers = {}
    for gram in zip(*[row[k:] for k in range(n)]):          # every n-gram of the row, in order
        followers.setdefault(tuple(gram[:-1]), []).append(gram[-1])
    key = tuple(row[L + 1 - n:L])                           # the last n - 1 tokens (empty for n = 1)
    return sorted(set(followers.get(key, [])))


def step_mask(row, n: int, base) -> np.ndarray:
    """the effective set of the step that follows `row`: the row's base set (bool [V]) minus the bans"""
    m = np.array(base, bool, copy=True)
    ban = banned_tokens(row, n)
    if ban:
        m[np.asarray(ban, np.int64)] = False
    return m


def step_masks(ids, lens, ngrams, base_masks) -> np.ndarray:
    """ids [B, L] as a decode emitted them, lens [B] -> bool [B, L - 1, V]: the effective set of every step t (the one that
    chose ids[:, t + 1]); steps behind a row's end keep the base set"""
    ids = np.asarray(ids)
    B, L = ids.shape
    out = np.repeat(np.asarray(base_masks, bool)[:, None, :], L - 1, axis=1)
    for b in range(B):
        for t in range(min(int(lens[b]), L) - 1):
            out[b, t] = step_mask(ids[b, :t + 1], int(ngrams[b]), base_masks[b])
    return out


def first_repeat(row, n: int):
    """the position of the first token that completes an n-gram the row already holds (None: the row repeats none)"""
    seen = set()
    row = [int(t) for t in row]
    for i in range(len(row) - n + 1):
        g = tuple(row[i:i + n])
        if g in seen:
            return i + n - 1
        seen.add(g)
    return None


def ngram_generate(o, enc, base_masks, ngrams, max_len: int):
    """constraint_util.masked_generate with the mask recomputed at every step from the rule above: base_masks bool [B, V],
    ngrams int [B].  -> (ids int64 [B, L], the fp32 logits of every step [B, L - 1, V] unmasked, the masks of every step bool
    [B, L - 1, V])"""
    import torch
    sp = o.spec
    B = enc.shape[0]
    base = np.asarray(base_masks, bool)
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
            mk = np.stack([step_mask(hist[b], int(ngrams[b]), base[b]) if int(unfinished[b]) else base[b] for b in range(B)])
            masks_all.append(mk)
            nxt = torch.argmax(torch.where(torch.from_numpy(mk), logits, torch.full_like(logits, float("-inf"))), dim=-1)
            nxt = nxt * unfinished + sp.pad_id * (1 - unfinished)
            ids = torch.cat((ids, nxt[:, None]), dim=1)
            done = (nxt == sp.eos_id) | (ids.shape[1] >= max_len)
            unfinished = unfinished & (~done).long()
            t += 1
            if int(unfinished.max()) == 0:
                break
    return ids.numpy(), torch.stack(logits_all, dim=1).numpy(), np.stack(masks_all, axis=1)


def lengths(ids, eos=EOS) -> np.ndarray:
    """tokens of every row incl. start and EOS (the row's width when it never emits EOS)"""
    ids = np.asarray(ids)
    return np.array([ids.shape[1] if eos not in r[1:] else 2 + list(r[1:]).index(eos) for r in ids])


def step_gaps(logits, masks) -> np.ndarray:
    """[B, T, V] logits, [B, T, V] per-step masks -> [B, T] top-2 margin among the unbanned tokens"""
    x = cu.masked(logits, masks)
    top2 = -np.partition(-x, 1, axis=-1)[..., :2]
    with np.errstate(invalid="ignore"):
        return np.where(np.isneginf(top2[..., 1]), np.inf, top2[..., 0] - top2[..., 1])
