"""Float64 reference helpers of the token-constraint tests (tests/test_constraints_cpu.py, tests/test_gpu_constraints.py).

A row decoded under a token set behaves as if the logits of every token outside the set were -inf before the argmax and
before the softmax of every step (include/mocr.h, "token constraints").  Here: the bit table the kernels read, the masked
forms of score_util's tile model and of the log-softmax / top four, and the masked greedy loop on the oracle."""
import numpy as np

import score_util as su

V, EOS, K4 = 6144, 3, 4
NO_IDX = 0x7FFFFFFF


def mask_of(ids, vocab=V, eos=EOS) -> np.ndarray:
    """token ids -> bool [vocab], EOS added as the engine adds it"""
    m = np.zeros(vocab, bool)
    m[np.asarray(list(ids), np.int64)] = True
    m[eos] = True
    return m


def pack_sets(masks) -> np.ndarray:
    """bool [S, V] -> uint32 [S, V / 32]: bit (v & 31) of word (v >> 5) = token v is allowed (the engine's table layout)"""
    m = np.asarray(masks, bool)
    w = m.reshape(m.shape[0], -1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)
    return w.sum(-1).astype(np.uint32)


def masked(logits, mask) -> np.ndarray:
    """float64 logits with -inf outside the set; mask broadcasts against logits"""
    return np.where(mask, np.asarray(logits, np.float64), -np.inf)


def masked_log_softmax64(logits, mask) -> np.ndarray:
    """float64 log-softmax over the allowed tokens only (-inf elsewhere); every row keeps an allowed token"""
    x = masked(logits, mask)
    m = x.max(-1, keepdims=True)
    with np.errstate(divide="ignore"):
        return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))


def masked_tile_stats(logits, mask, tile: int, dtype=np.float64):
    """score_util.tile_stats under a set: per tile (max over the allowed columns, its first column, sum over the allowed
    columns of exp(logit - max)).  A tile with no allowed column: (-inf, NO_IDX, 0) - the sum is 0, not exp(-inf - -inf)."""
    x = masked(logits, mask).astype(dtype)
    t = x.reshape(x.shape[:-1] + (x.shape[-1] // tile, tile))
    m = t.max(-1)
    empty = np.isneginf(m)
    idx = np.where(empty, NO_IDX, np.argmax(t, -1) + np.arange(t.shape[-2]) * tile)
    with np.errstate(invalid="ignore"):
        e = np.exp(t - np.where(empty, 0, m)[..., None], dtype=dtype)
    s = np.where(empty, 0, e.sum(-1, dtype=dtype)).astype(dtype)
    return m, idx, s


def masked_merge_tiles(m, s) -> np.ndarray:
    """(tile maxima, tile sums) of masked_tile_stats -> logsumexp over the row's allowed tokens: score_util.merge_tiles,
    where an empty tile's term is 0 x exp(-inf - M) = 0"""
    m, s = np.asarray(m, np.float64), np.asarray(s, np.float64)
    M = m.max(-1, keepdims=True)
    return (M + np.log((s * np.exp(m - M)).sum(-1, keepdims=True)))[..., 0]


def masked_top(logits, mask, k=K4):
    """-> (ids [..., k] of the k best allowed tokens, value descending and the lower id first among equal values, -1 where the
    set has fewer; their masked float64 log-probabilities, -inf there)"""
    x = masked(logits, mask)
    idx = np.argsort(-x, axis=-1, kind="stable")[..., :k]
    lp = np.take_along_axis(masked_log_softmax64(logits, mask), idx, -1)
    return np.where(np.isneginf(np.take_along_axis(x, idx, -1)), -1, idx), lp


def masked_generate(o, enc, masks, max_len: int):
    """Oracle.generate's greedy loop with the logits outside every row's set at -inf before the argmax: masks bool [B, V].
    -> (ids int64 [B, L], the fp32 logits of every step [B, L - 1, V], unmasked)"""
    import torch
    sp = o.spec
    B = enc.shape[0]
    allow = torch.from_numpy(np.asarray(masks, bool))
    with torch.no_grad():
        ckv = o.cross_kv(enc)
        self_kv = [None] * sp.dec_layers
        ids = torch.full((B, 1), sp.start_id, dtype=torch.int64)
        unfinished = torch.ones(B, dtype=torch.int64)
        logits_all = []
        t = 0
        while True:
            logits = o.decode_step(ids[:, -1], t, self_kv, ckv)
            logits_all.append(logits)
            nxt = torch.argmax(torch.where(allow, logits, torch.full_like(logits, float("-inf"))), dim=-1)
            nxt = nxt * unfinished + sp.pad_id * (1 - unfinished)
            ids = torch.cat((ids, nxt[:, None]), dim=1)
            done = (nxt == sp.eos_id) | (ids.shape[1] >= max_len)
            unfinished = unfinished & (~done).long()
            t += 1
            if int(unfinished.max()) == 0:
                break
    return ids.numpy(), torch.stack(logits_all, dim=1).numpy()


def row_masks(free_ids, seed: int, vocab=V) -> np.ndarray:
    """The per-row sets of the end-to-end tests, bool [B, V]: row 0 the whole vocabulary, then alternately a random half
    and "everything but the tokens the free run emitted for this row" (EOS always allowed)."""
    rs = np.random.RandomState(seed)
    B = free_ids.shape[0]
    masks = np.ones((B, vocab), bool)
    for b in range(1, B):
        if b % 2:
            masks[b] = rs.rand(vocab) < 0.5
        else:
            masks[b, np.unique(free_ids[b, 1:])] = False
        masks[b, EOS] = True
    return masks


def first_divergences(got, want, gaps):
    """[(row, token position, the reference's masked top-2 margin at the step that decided it)] of every row's first
    divergence (tests/test_gpu_bf16_parity.py's rule: later tokens of such a row are free)"""
    out = []
    L = min(got.shape[1], want.shape[1])
    for b in range(got.shape[0]):
        neq = np.nonzero(got[b, :L] != want[b, :L])[0]
        if neq.size:
            out.append((b, int(neq[0]), float(gaps[b, int(neq[0]) - 1])))
    return out


def masked_gaps(logits, masks) -> np.ndarray:
    """[B, T, V] logits, [B, V] masks -> [B, T] top-2 margin among the allowed tokens (inf for a one-token set)"""
    x = masked(logits, np.asarray(masks, bool)[:, None, :])
    top2 = -np.partition(-x, 1, axis=-1)[..., :2]
    with np.errstate(invalid="ignore"):
        return np.where(np.isneginf(top2[..., 1]), np.inf, top2[..., 0] - top2[..., 1])

