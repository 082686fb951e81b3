"""Float64 reference helpers of the token-score tests (tests/test_scores_cpu.py, tests/test_gpu_scores.py).

A token's score is the log-probability the decoder gave it: ``logits[id] - logsumexp(logits)`` over the fp32 LM-head
outputs of the step that chose it.  The engine never holds a row of logits: the LM head reduces every 64 / 128-column
tile to (max m_c, its column, s_c = sum over the tile of exp(logit - m_c)) and the token kernel merges the tiles,
``logsumexp = M + log(sum_c s_c exp(m_c - M))`` with ``M = max_c m_c``.  ``tiled_lse`` states that merge in numpy."""
import functools

import numpy as np

from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights

PEAK_SCALE = 8.0      # LM-head weight x 8: chosen-token log-probabilities spread over [-2.7, -0.02] instead of [-5.6, -4.5]


def lse64(logits) -> np.ndarray:
    """float64 logsumexp over the last axis"""
    x = np.asarray(logits, np.float64)
    m = x.max(-1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))[..., 0]


def log_softmax64(logits) -> np.ndarray:
    x = np.asarray(logits, np.float64)
    return x - lse64(x)[..., None]


def tile_stats(logits, tile: int, dtype=np.float64):
    """[..., V] logits -> per tile (max, first column of the max, sum of exp(logit - max)); ``dtype``: the precision the
    tile sums are formed and kept in (np.float32 models the kernel's storage)."""
    x = np.asarray(logits, dtype)
    t = x.reshape(x.shape[:-1] + (x.shape[-1] // tile, tile))
    m = t.max(-1)
    idx = np.argmax(t, -1) + np.arange(t.shape[-2]) * tile
    s = np.exp(t - m[..., None], dtype=dtype).sum(-1, dtype=dtype)
    return m, idx, s


def merge_tiles(m, s) -> np.ndarray:
    """(tile maxima, tile exp sums) -> logsumexp of the row, in float64: M + log(sum_c s_c exp(m_c - M))"""
    m, s = np.asarray(m, np.float64), np.asarray(s, np.float64)
    M = m.max(-1, keepdims=True)
    return (M + np.log((s * np.exp(m - M)).sum(-1, keepdims=True)))[..., 0]


def tiled_lse(logits, tile: int, dtype=np.float64) -> np.ndarray:
    m, _, s = tile_stats(logits, tile, dtype)
    return merge_tiles(m, s)


def f32_lse_error(logits) -> float:
    """max |float32 torch.logsumexp - float64 logsumexp| over the rows of ``logits`` (given as float32 values): what a
    correct fp32 implementation of the same reduction is allowed to lose"""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(logits, np.float32))
    got = torch.logsumexp(x, -1).double().numpy()
    return float(np.abs(got - lse64(x.numpy())).max())


def chosen_logp64(logits, ids) -> np.ndarray:
    """logits [B, T, V] of steps 0 .. T-1, ids [B, >= T + 1] -> float64 [B, T]: log-softmax of step t at ids[:, t + 1]"""
    lp = log_softmax64(logits)
    T = lp.shape[1]
    return np.take_along_axis(lp, np.asarray(ids)[:, 1:T + 1, None].astype(np.int64), -1)[..., 0]


@functools.lru_cache(maxsize=None)
def score_weights(kind: str, seed: int = 0):
    """'wide': the project's widened-margin set (vocab_bias_std 1.0); 'peaked': the same with the LM-head weight x 8;
    'eos': the early-EOS set of tests/test_gpu_compaction.py (seed 1, eos_bias 1.1)"""
    if kind == "wide":
        return synthetic_weights(seed, vocab_bias_std=1.0)
    if kind == "peaked":
        return synthetic_weights(seed, vocab_bias_std=1.0, logit_scale=PEAK_SCALE)
    if kind == "eos":
        return synthetic_weights(1, eos_bias=1.1)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def score_engine(kind: str, dtype: str, max_batch: int = 8, flags: int = 0, seed: int = 0):
    from manga_ocr.engine import Engine
    return Engine(score_weights(kind, seed), DEFAULT_SPEC, dtype=dtype, device=0, max_batch=max_batch, flags=flags, lanes=1)


@functools.lru_cache(maxsize=None)
def score_oracle(kind: str, seed: int = 0):
    from oracle.mocr_oracle import Oracle
    return Oracle(score_weights(kind, seed), DEFAULT_SPEC)


@functools.lru_cache(maxsize=None)
def oracle_run(kind: str, crop_seed: int, n: int, max_len: int, seed: int = 0):
    """(ids [n, L], logits float32 [n, L-1, V]) of the fp32 oracle's greedy decode of crops(crop_seed, n)"""
    import torch
    from gpu_util import crops
    o = score_oracle(kind, seed)
    with torch.no_grad():
        enc = o.encode(o.preprocess_gray(crops(crop_seed, n)))
        ids, logits = o.generate(enc, max_len=max_len, return_logits=True)
    return ids, logits


def lm_head_scale(w) -> float:
    """An upper bound of sum_k |a_k w_jk| for the LM head of weights ``w``, from the weights alone: a = the transform's
    LayerNorm output, |a|_2 <= max|gamma| sqrt(768) + |beta|_2, and sum |a w| <= |a|_2 |w_j|_2 (Cauchy-Schwarz)."""
    g = w["decoder.cls.predictions.transform.LayerNorm.weight"].astype(np.float64)
    b = w["decoder.cls.predictions.transform.LayerNorm.bias"].astype(np.float64)
    wv = w["decoder.cls.predictions.decoder.weight"].astype(np.float64)
    return float((np.abs(g).max() * np.sqrt(g.size) + np.linalg.norm(b)) * np.linalg.norm(wv, axis=1).max())
