"""Helpers shared by the -m gpu tests: engines are expensive to build, so they are cached."""
import functools
import os

import numpy as np

from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights

REPORT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "parity_report.txt")


def report(line: str) -> None:
    print(line, flush=True)
    try:
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        with open(REPORT, "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def crops(seed, n):
    return np.random.RandomState(seed).randint(0, 256, size=(n, 224, 224), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def weights(seed=0, eos_bias=0.0, vocab_bias_std=0.0, hostile=False):
    return synthetic_weights(seed, eos_bias=eos_bias, vocab_bias_std=vocab_bias_std, hostile=hostile)


@functools.lru_cache(maxsize=None)
def engine(dtype="fp32", seed=0, eos_bias=0.0, max_batch=8, flags=0, lanes=1, auto_path=False, vocab_bias_std=0.0, hostile=False):
    """bf16 engines of the tests run the latent attention at every batch size (flag 64) unless they ask for the classic
    kernels (flag 8) or for the product's automatic choice (auto_path: classic up to 256 rows)."""
    from manga_ocr.engine import Engine
    if dtype == "bf16" and not auto_path and not (flags & 8):
        flags |= 64
    return Engine(weights(seed, eos_bias, vocab_bias_std, hostile), DEFAULT_SPEC, dtype=dtype, device=0, max_batch=max_batch, flags=flags, lanes=lanes)


def drop_engines():
    """Engines are cached for speed; a test that needs the HBM back (fat default-sized engines) closes them all."""
    engine.cache_clear()
    import gc
    gc.collect()


@functools.lru_cache(maxsize=None)
def oracle(seed=0, eos_bias=0.0, vocab_bias_std=0.0, hostile=False):
    from oracle.mocr_oracle import Oracle
    return Oracle(weights(seed, eos_bias, vocab_bias_std, hostile), DEFAULT_SPEC)


def bf16_round(a: np.ndarray) -> np.ndarray:
    """float32 -> nearest bfloat16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


BF16_ULP = 2.0 ** -8


def _nan(shape, dtype):
    """NaN-filled output of the engine's storage type ("f32" / "fp32": float32)"""
    import torch
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.bfloat16 if dtype == "bf16" else torch.float32)


def _store(x, dtype):
    """a float64 array as the engine's storage type holds it"""
    return bf16_round(np.asarray(x, np.float32)).astype(np.float64) if dtype == "bf16" else np.asarray(x, np.float32).astype(np.float64)


ACC = 2.0 ** -16                    # fp32 accumulation, relative to the sum of the absolute terms
GELU_SLOPE = 1.13                   # GELU's largest slope
_EPI_SLAB, _EPI_BIAS_GELU = 0, 2


def gelu64(x):
    from scipy.special import erf
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def gemm_bound(dtype, epi, ref_pre, s1, bias, resid=None, out_f32=False):
    """(reference of a GEMM's output, elementwise tolerance) from the float64 product ref_pre = A W^T and S1 = |A| |W|^T:
    |err| <= u |ref| + ACC S1' with S1' = S1 + |bias| (+ |resid|) the sum of the absolute terms, u = 2^-8 for a bf16 output
    and 0 for an fp32 one (slabs, out_f32).  Fused GELU: GELU_SLOPE x the pre-activation bound, + 1e-5 of the row's largest
    |ref| (+ 3e-5 for bf16 outputs) for the device's erf."""
    if epi == _EPI_SLAB:
        return ref_pre, ACC * s1
    u = BF16_ULP if (dtype == "bf16" and not out_f32) else 0.0
    pre, s1b = ref_pre + bias, s1 + np.abs(bias)
    if resid is not None:
        pre, s1b = pre + resid, s1b + np.abs(resid)
    if epi == _EPI_BIAS_GELU:
        ref = gelu64(pre)
        erf_allowance = 1e-5 * np.abs(ref).max(-1, keepdims=True) + (3e-5 if dtype == "bf16" else 0.0)
        return ref, u * np.abs(ref) + GELU_SLOPE * ACC * s1b + erf_allowance
    return pre, u * np.abs(pre) + ACC * s1b


def check_elementwise(got, ref, tol, what):
    """every element within its own tolerance; returns the worst err / tol"""
    assert np.isfinite(got).all(), f"{what}: non-finite output (a tile no block took, or a NaN row of A reached an output)"
    err = np.abs(got - ref)
    bad = np.argwhere(err > tol)
    assert bad.size == 0, f"{what}: {len(bad)} elements out of tolerance, first at {tuple(bad[0])}: got {got[tuple(bad[0])]} want {ref[tuple(bad[0])]}"
    return float((err / tol).max())


def _grid_vals(rs, shape, scale=1.0):
    """values on a 2^-10 grid (|v| < 8 scale): fp32 sums of a few dozen of them are exact in any order"""
    return (np.round(rs.standard_normal(shape) * scale * 256) / 1024).clip(-8 * scale, 8 * scale).astype(np.float32)


def _check_bf16_or_f32(got, ref, scale, dtype, what, extra=0.0):
    """|got - ref| <= (2^-8 |ref| for bf16) + 1e-5 scale + extra; returns the worst ratio err / tol"""
    tol = (BF16_ULP * np.abs(ref) if dtype == "bf16" else 0.0) + 1e-5 * scale + extra
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    ratio = float((err / tol).max())
    bad = np.argwhere(err > tol)
    assert bad.size == 0, f"{what}: {len(bad)} elements out of tolerance, first at {tuple(bad[0])}: got {got[tuple(bad[0])]} want {ref[tuple(bad[0])]}"
    return ratio, float((err / np.broadcast_to(scale, err.shape)).max())


def _ln64(v, g, b, eps=1e-12):
    m = v.mean(-1, keepdims=True)
    var = ((v - m) ** 2).mean(-1, keepdims=True)
    return (v - m) / np.sqrt(var + eps) * g + b, m[..., 0], np.sqrt(var[..., 0])


def e4m3_table():
    """byte -> float for OCP e4m3fn (bias 7, no infinities, 0x7F / 0xFF = NaN)."""
    t = np.zeros(256, np.float64)
    for b in range(256):
        s, e, m = b >> 7, (b >> 3) & 15, b & 7
        if e == 15 and m == 7:
            v = np.nan
        elif e == 0:
            v = m * 2.0 ** -9
        else:
            v = (1 + m / 8.0) * 2.0 ** (e - 7)
        t[b] = -v if s else v
    return t


def e4m3_quant(x):
    """float -> nearest e4m3 value (round half to even), as float64; |x| <= 448 assumed."""
    x = np.asarray(x, np.float64)
    a = np.abs(x)
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -20)))
    e = np.clip(e, -6, 8)
    q = 2.0 ** (e - 3)
    return np.sign(x) * np.round(a / q) * q          # numpy rounds half to even


def assert_ids_match_up_to_ties(got, want, gap_fn, tol, what):
    """Token ids must be identical; the only divergence tolerated is at a step where the ORACLE's
    own top-2 logit gap is below `tol` (a numerical tie no fp32 implementation can be held to).
    gap_fn(row, step) -> oracle top-2 gap at that decision."""
    got, want = np.asarray(got), np.asarray(want)
    L = min(got.shape[1], want.shape[1])
    n_tie = 0
    for b in range(got.shape[0]):
        neq = np.nonzero(got[b, :L] != want[b, :L])[0]
        if neq.size == 0:
            continue
        t = int(neq[0])          # ids[t] was decided at step t-1
        gap = float(gap_fn(b, t - 1))
        report(f"[{what}] row {b}: first divergence at token {t} (oracle top-2 gap {gap:.3e})")
        assert gap < tol, f"{what}: row {b} diverges at token {t} where the oracle's margin is {gap:.3e} >= {tol}"
        n_tie += 1
    return n_tie
