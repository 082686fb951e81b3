"""Float64 / numpy reference helpers of the token-position tests (tests/test_positions_cpu.py, tests/test_gpu_positions.py).

The definition is include/mocr.h, "token positions": per head the softmax of q_h . K_h / 8 over the 197 encoder keys, the
mean of the twelve probability maps, and of that map centre, spread and mass over the 196 patches (key 0 is CLS)."""
import functools

import numpy as np

from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights

H, DH, KEYS, GRID, FIELDS = 12, 64, 197, 14, 5
# The end-to-end tests scale the last decoder layer's cross-attention query weight and bias by G: synthetic_weights alone
# gives nearly uniform cross-attention (cx = cy = 0.5 everywhere shows nothing).  Chosen on the CPU
# (test_positions_cpu.test_the_scaled_query_spreads_the_positions states the condition); EOS_BIAS makes the rows of CROP_SEED
# end at different lengths below 24 tokens.
G = 64.0         # 8: std(cx) 0.021, 16: 0.046, 32: 0.061, 64: 0.072 over the tokens of the six crops (fp32 oracle)
EOS_BIAS = 1.3   # lengths 24, 17, 24, 17, 24, 13 at max_len 24
WEIGHT_SEED = 1
CROP_SEED = 4321
U = (np.arange(GRID) + 0.5) / GRID


def fields_from_map(a) -> np.ndarray:
    """head-mean map a [..., 197] (float64) -> [..., 5] (cx, cy, sx, sy, mass) by the definition"""
    a = np.asarray(a, np.float64)
    g = a[..., 1:].reshape(a.shape[:-1] + (GRID, GRID))          # [.., grid row i (v), grid column j (u)]
    mass = g.sum(axis=(-1, -2))
    safe = np.where(mass < 1e-20, 1.0, mass)
    cx = (g.sum(axis=-2) * U).sum(-1) / safe
    cy = (g.sum(axis=-1) * U).sum(-1) / safe
    sx = np.sqrt(np.maximum(0.0, (g.sum(axis=-2) * U * U).sum(-1) / safe - cx * cx))
    sy = np.sqrt(np.maximum(0.0, (g.sum(axis=-1) * U * U).sum(-1) / safe - cy * cy))
    none = mass < 1e-20
    out = np.stack([np.where(none, 0.5, cx), np.where(none, 0.5, cy), np.where(none, 0.0, sx), np.where(none, 0.0, sy), mass], axis=-1)
    return out


def head_mean_map(q, K) -> np.ndarray:
    """q [rows, T, 768], K [rows, 197, 768] -> float64 [rows, T, 197]: per head softmax_k(q_h . K_h[k] / 8) with the maximum
    subtracted, then the mean over the 12 heads"""
    q = np.asarray(q, np.float64)
    K = np.asarray(K, np.float64)
    rows, T, _ = q.shape
    qh = q.reshape(rows, T, H, DH)
    kh = K.reshape(rows, KEYS, H, DH)
    s = np.einsum("rthd,rkhd->rthk", qh, kh) / 8.0
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(axis=-1, keepdims=True)
    return p.mean(axis=2)


def ref_positions(q, K, lens):
    """The operator's reference: (map float64 [rows, T, 197], fields float64 [rows, T, 5]); positions at and behind lens[r]
    are 0 in both."""
    a = head_mean_map(q, K)
    f = fields_from_map(a)
    for r, n in enumerate(lens):
        a[r, max(int(n), 0):] = 0.0
        f[r, max(int(n), 0):] = 0.0
    return a, f


def scaled_weights(w: dict, g: float, spec=DEFAULT_SPEC) -> dict:
    """a copy of the weights with the LAST decoder layer's cross-attention query weight and bias scaled by g"""
    out = dict(w)
    p = f"decoder.bert.encoder.layer.{spec.dec_layers - 1}.crossattention.self.query."
    out[p + "weight"] = (np.asarray(w[p + "weight"], np.float32) * np.float32(g)).astype(np.float32)
    out[p + "bias"] = (np.asarray(w[p + "bias"], np.float32) * np.float32(g)).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def pos_weights(g: float = G, eos_bias: float = EOS_BIAS, seed: int = WEIGHT_SEED) -> dict:
    return scaled_weights(synthetic_weights(seed, eos_bias=eos_bias), g)


def forced_cross_probs(o, enc, ids) -> np.ndarray:
    """Teacher-forced decoder loop restating Oracle._dec_layer_step from its public pieces, because Oracle._attn does not
    return its probabilities: ids int [B, T] (ids[:, 0] the start token) -> float64 [B, T, 12, 197], entry t the LAST layer's
    cross-attention probabilities of the step that consumed ids[:, t].  The restatement's logits are checked against
    Oracle.generate(forced_ids=..., return_logits=True) to 1e-5, so it cannot drift from the oracle."""
    import torch
    import torch.nn.functional as F
    ids = np.asarray(ids)
    B, T = ids.shape
    w, sp = o.w, o.spec
    probs, logits = [], []
    with torch.no_grad():
        ckv = o.cross_kv(enc)
        self_kv = [None] * sp.dec_layers
        for t in range(T):
            x = o._dec_embed(torch.from_numpy(ids[:, t].astype(np.int64))[:, None], t)
            for i in range(sp.dec_layers):
                p = f"decoder.bert.encoder.layer.{i}."
                a = p + "attention."
                q = o._heads(F.linear(x, w[a + "self.query.weight"], w[a + "self.query.bias"]))
                k = o._heads(F.linear(x, w[a + "self.key.weight"], w[a + "self.key.bias"]))
                v = o._heads(F.linear(x, w[a + "self.value.weight"], w[a + "self.value.bias"]))
                if self_kv[i] is not None:
                    k = torch.cat((self_kv[i][0], k), dim=2)
                    v = torch.cat((self_kv[i][1], v), dim=2)
                self_kv[i] = (k, v)
                pr = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * (o.dh ** -0.5), dim=-1, dtype=torch.float32)
                ctx = o._merge(torch.matmul(pr, v))
                x = o._ln(F.linear(ctx, w[a + "output.dense.weight"], w[a + "output.dense.bias"]) + x, a + "output.LayerNorm")
                c = p + "crossattention."
                q = o._heads(F.linear(x, w[c + "self.query.weight"], w[c + "self.query.bias"]))
                s = torch.matmul(q, ckv[i][0].transpose(-1, -2)) * (o.dh ** -0.5)           # [B, H, 1, 197]
                pr = torch.softmax(s, dim=-1, dtype=torch.float32)
                if i == sp.dec_layers - 1:
                    s64 = s.double()
                    p64 = torch.softmax(s64, dim=-1)
                    probs.append(p64[:, :, 0, :].numpy())
                ctx = o._merge(torch.matmul(pr, ckv[i][1]))
                x = o._ln(F.linear(ctx, w[c + "output.dense.weight"], w[c + "output.dense.bias"]) + x, c + "output.LayerNorm")
                h = F.gelu(F.linear(x, w[p + "intermediate.dense.weight"], w[p + "intermediate.dense.bias"]))
                h = F.linear(h, w[p + "output.dense.weight"], w[p + "output.dense.bias"])
                x = o._ln(h + x, p + "output.LayerNorm")
            logits.append(o._lm_head(x)[:, 0, :].float().numpy())
        _, want = o.generate(enc, return_logits=True, forced_ids=ids)
    got = np.stack(logits, axis=1)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-5, "the restated decoder step left the oracle's"
    return np.stack(probs, axis=1)


def reference_for_ids(o, gray, ids, lens, enc=None) -> np.ndarray:
    """The end-to-end reference: float64 [B, L, 5], the fields of token t (1 <= t < lens[b]) from the step that consumed
    ids[b, t - 1], teacher-forced on `ids`; 0 elsewhere.  `enc`: the oracle's encoder output of `gray` when the caller has it."""
    ids = np.asarray(ids)
    B, L = ids.shape
    if enc is None:
        enc = o.encode(o.preprocess_gray(gray))
    T = max(int(max(lens)) - 1, 1)
    pr = forced_cross_probs(o, enc, ids[:, :T])                  # [B, T, 12, 197]
    f = fields_from_map(pr.mean(axis=2))                         # [B, T, 5]
    out = np.zeros((B, L, FIELDS), np.float64)
    for b in range(B):
        n = int(lens[b])
        if n > 1:
            out[b, 1:n] = f[b, :n - 1]
    return out
