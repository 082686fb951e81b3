"""-m gpu: gemm_pers_kernel (csrc/kernels_gemm_pers.h), the persistent GEMM of the encoder's layers, against float64 - every
schedule (tile list, strips), every epilogue, with and without the folded LayerNorm, in the tile order the encoder uses.

The launches go through mocr_op_gemm_pers (Engine.op_gemm_pers): the GemmCall run_encoder builds, with the column groups of
the tile order (group_n) that mocr_op_gemm never passes; the product's group sizes come from mocr_encoder_groups.
mocr_last_pers_launch says what each launch ran - the grid, strips or tile list, the tiles, group_n - and every case holds
that against the launch it meant (tests/pers_schedule.py restates the host's and the kernel's schedule arithmetic;
tests/test_pers_schedule_cpu.py asserts there that the strip shapes below reach every class of strip and tile).

Operands, two kinds per shape:
  * "exact": A in multiples of 1/2 (|a| <= 4), W in multiples of 1/4 (|w| <= 1), bias and residual in multiples of 1/8 (eight
    columns per 256-column slice with a bias of 40 .. 90, so that every tile holds sums bf16 cannot hold and must round).  Every
    product is a multiple of 1/8 and S1 = sum |a| |w| + |bias| + |resid| stays far below 2^21, so every fp32 partial sum is exact
    in any order (asserted: 8 S1 < 2^24 and ref == float32(ref)).  The fp32 output (bias + residual) must EQUAL the float64
    reference, the bf16 output (bias) its round-to-nearest-even, the bf16 copy of the fold the rounded output and the fold's row
    sums / sums of squares (multiples of 1/8 and 1/64, 64 x the sum of squares < 2^24: exact too) the exact ones.  One dropped,
    doubled or misplaced term, row, column, bias or residual element, or a truncating bf16 store, fails.  GELU is not exact: it
    takes the bound below.
  * "gauss": A ~ N(0, 1), W ~ 0.05 N(0, 1) as bf16, bias and residual ~ N(0, 1) fp32; the elementwise bound of gpu_util.gemm_bound,
    |err| <= u |ref| + 2^-16 S1 (u = 2^-8 for bf16 outputs, 0 for fp32 ones), GELU: 1.13 x the pre-activation part + the erf
    allowance.  Every case reports its worst err / tol.

A holds whole 256-row tiles for the tile list (the kernel stages them) and exactly M rows for the strips (they read no row
behind M); the rows behind M are NaN either way, as are the outputs and the GUARD rows behind them.  Every launch runs twice,
out of place and then in place (out = resid, as the encoder calls the fp32-residual GEMMs)."""
import functools
import os

import numpy as np
import pytest

from gpu_util import ACC, _nan, _store, bf16_round, check_elementwise, engine, gelu64, gemm_bound, report
from pers_schedule import STRIP_SHAPES, strip_grid, strip_wins

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID = 1, 2, 3
GUARD = 3
LIST8, PRODUCT, STRIPS, STRIPS8 = 4097, 4096, 4099, 4100      # tile codes: tile list on 8 blocks, the product's choice, strips, strips on 8 blocks


def _eng():
    """one engine for the file; 64 crops is where QKV and FC1 move to the persistent kernel, so its plan holds their group sizes"""
    return engine("bf16", max_batch=64)


def _cus():
    return max(torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8, 8)


def _round_up(n, q):
    return -(-n // q) * q


def _np(t):
    return t.float().cpu().numpy().astype(np.float64)


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda().to(torch.bfloat16)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@functools.lru_cache(maxsize=2)
def _operands(mode, M, N, K):
    """A [M, K], W [N, K], bias [N], resid [M, N] as float64 values the device holds exactly, and the float64 references:
    the product A W^T and S1 = |A| |W|^T"""
    rs = np.random.RandomState((M * 7919 + N * 31 + K + (mode == "exact")) % (2 ** 31))
    if mode == "exact":
        A = (np.round(rs.standard_normal((M, K)) * 2) / 2).clip(-4, 4)
        W = (np.round(rs.standard_normal((N, K))) / 4).clip(-1, 1)
        bias = np.round(rs.standard_normal(N) * 8) / 8
        # eight columns of every 256-column slice carry a bias of 40 .. 90 in eighths: the sums of a few units are exact in bf16 (8
        # significant bits hold every multiple of 1/8 below 32), these columns' are not - in [32, 64) every other multiple of 1/8 is a
        # tie, in [64, 128) three of four need rounding - so every tile's bf16 store rounds, ties included
        for t in range(N // 256):
            cols = 256 * t + rs.choice(256, 8, replace=False)
            bias[cols] = rs.choice([-1.0, 1.0], 8) * (40 + np.round(rs.rand(8) * 50 * 8) / 8)
        resid = np.round(rs.standard_normal((M, N)) * 8) / 8
        assert np.array_equal(A, _store(A, "bf16")) and np.array_equal(W, _store(W, "bf16"))
    else:
        A = _store(rs.standard_normal((M, K)), "bf16")
        W = _store(rs.standard_normal((N, K)) * 0.05, "bf16")
        bias = rs.standard_normal(N).astype(np.float32).astype(np.float64)
        resid = rs.standard_normal((M, N)).astype(np.float32).astype(np.float64)
    pre, s1 = A @ W.T, np.abs(A) @ np.abs(W).T
    if mode == "exact":
        full = pre + bias + resid
        assert ((s1 + np.abs(bias) + np.abs(resid)) * 8 < 2 ** 24).all(), "the operands are not coarse enough for exact fp32 sums"
        assert np.array_equal(full, full.astype(np.float32)) and np.array_equal(pre + bias, (pre + bias).astype(np.float32))
    for a in (A, W, bias, resid, pre, s1):
        a.setflags(write=False)
    return A, W, bias, resid, pre, s1


class _Dev:
    """the operands of a case on the device"""

    def __init__(self, A, W, bias, resid, padded):
        M, K = A.shape
        self.A = _nan((_round_up(M, 256) if padded else M + GUARD, K), "bf16")
        self.A[:M] = _bf16(A)
        self.W, self.bias = _bf16(W), _f32(bias)
        self.resid = _f32(resid) if resid is not None else None


def _launch(eng, dev, code, M, N, K, epi, *, group_n=0, fold=False, inplace=False, part=None, csum=None):
    """one launch on fresh NaN outputs -> (out [M + GUARD, N], xb, ln_part, the launch's record); fold with EPI_BIAS_RESID: xb and
    ln_part are written (ln_part pre-filled with -7), with the bf16 epilogues: `part` and `csum` are read"""
    out = _nan((M + GUARD, N), "fp32" if epi == EPI_BIAS_RESID else "bf16")
    kw = dict(M=M, N=N, K=K, epilogue=epi, tile=code, group_n=group_n, A=dev.A, W=dev.W, bias=dev.bias, out=out, resid=None, ln_part=None,
              csum=None, xb=None)
    xb = lp = None
    if epi == EPI_BIAS_RESID:
        kw["resid"] = dev.resid
        if inplace:
            out[:M] = dev.resid
            kw["resid"] = out
        if fold:
            xb = _nan((M + GUARD, N), "bf16")
            lp = torch.full((M + GUARD, 4, 2), -7.0, device="cuda", dtype=torch.float32)
            kw.update(ln_part=lp, xb=xb)
    elif fold:
        kw.update(ln_part=part, csum=csum)
    torch.cuda.synchronize()
    eng.op_gemm_pers(**kw)
    rec = eng.last_pers_launch()
    got = _np(out)
    assert np.isnan(got[M:]).all(), "rows behind M were written"
    return got[:M], (_np(xb) if xb is not None else None), (_np(lp) if lp is not None else None), rec


def _slice_sums(x64):
    """[M, N] -> [M, N / 256, 2]: each row's (sum, sum of squares) per 256-column slice"""
    M, N = x64.shape
    seg = x64.reshape(M, N // 256, 256)
    return np.stack([seg.sum(-1), (seg * seg).sum(-1)], -1)


def _verify(mode, epi, fold, got, xb, lp, ops, what):
    """one launch's outputs against the references of its operands; returns the worst err / tol (0.0: compared for equality)"""
    A, W, bias, resid, pre, s1 = ops
    M, N = pre.shape
    worst = 0.0
    if mode == "exact" and epi == EPI_BIAS_RESID:
        ref = pre + bias + resid
        assert np.isfinite(got).all(), f"{what}: non-finite output"
        bad = np.argwhere(got != ref)
        assert bad.size == 0, f"{what}: {len(bad)} elements differ from the exact sum, first at {tuple(bad[0])}: got {got[tuple(bad[0])]} want {ref[tuple(bad[0])]}"
    elif mode == "exact" and epi == EPI_BIAS:
        ref = bf16_round((pre + bias).astype(np.float32)).astype(np.float64)
        assert np.isfinite(got).all(), f"{what}: non-finite output"
        bad = np.argwhere(got != ref)
        assert bad.size == 0, f"{what}: {len(bad)} elements are not the exact sum rounded to nearest even, first at {tuple(bad[0])}: got {got[tuple(bad[0])]} want {ref[tuple(bad[0])]}"
    else:
        ref, tol = gemm_bound("bf16", epi, pre, s1, bias, resid=resid if epi == EPI_BIAS_RESID else None, out_f32=epi == EPI_BIAS_RESID)
        worst = check_elementwise(got, ref, tol, what)
    if fold and epi == EPI_BIAS_RESID:
        ns = N // 256
        assert np.isnan(xb[M:]).all() and (lp[M:] == -7.0).all(), f"{what}: the fold wrote behind row M"
        assert (lp[:M, ns:] == -7.0).all(), f"{what}: statistics written to a slot behind the {ns} column slices"
        assert np.array_equal(xb[:M], bf16_round(got.astype(np.float32)).astype(np.float64)), f"{what}: the bf16 copy is not the rounded fp32 output"
        want = _slice_sums(got)                 # of the rows the kernel wrote (exact mode: the exact rows)
        if mode == "exact":
            assert (want[..., 1] * 64 < 2 ** 24).all(), "the rows are not coarse enough for exact sums of squares"
            assert np.array_equal(lp[:M, :ns], want), f"{what}: the rows' sums / sums of squares are not the exact ones"
        else:
            # 256 fp32 values summed in any order: 255 roundings, each at most 2^-24 of the sum of the absolute terms - 2^-16 of
            # it; the squares carry one rounding more each
            seg = np.abs(got).reshape(M, ns, 256)
            tol = np.stack([ACC * seg.sum(-1), (ACC + 2.0 ** -23) * (seg * seg).sum(-1)], -1)
            worst = max(worst, check_elementwise(lp[:M, :ns], want, tol, what + " fold sums"))
    return worst


def _expect(rec, *, blocks, strips, tiles, group_n, what):
    want = dict(blocks=blocks, strips=strips, tiles=tiles, group_n=group_n)
    assert rec == want, f"{what}: launched {rec}, meant {want}"


# ------------------------------------------------------------------------------------------------ the tile list
# M in {256, 300, 512, 700} x N in {256, 768, 2304, 3072}, K walking {128, 192, 320, 768} (a Latin square: every M, N and K meets
# every other; K = 192 and 320 give 3 and 5 64-deep K-tiles per tile, so the slot of the LDS image alternates from tile to tile),
# and K = 3072 once.  On 8 blocks (4097) that is 1 .. 36 tiles: blocks with 0, 1, 2 and 3 - 5 tiles.
TILE_SHAPES = [(256, 256, 128), (300, 256, 192), (512, 256, 320), (700, 256, 768),
               (256, 768, 192), (300, 768, 320), (512, 768, 768), (700, 768, 128),
               (256, 2304, 320), (300, 2304, 768), (512, 2304, 128), (700, 2304, 192),
               (256, 3072, 768), (300, 3072, 128), (512, 3072, 192), (700, 3072, 320),
               (256, 768, 3072)]


def _plan_group(eng, N):
    """the product's column groups: QKV's for every N but FC1's own"""
    pl = eng.encoder_plan(64)
    assert pl["tile_qkv"] == PRODUCT and pl["tile_fc1"] == PRODUCT, f"64 crops do not run QKV / FC1 on the persistent kernel: {pl}"
    g = eng.encoder_groups(64)
    return g["fc1"] if N == 3072 else g["qkv"]


@pytest.mark.parametrize("mode", ["exact", "gauss"])
@pytest.mark.parametrize("M,N,K", TILE_SHAPES)
def test_tile_list_in_every_tile_order(mode, M, N, K):
    """The tile list on 8 blocks under every column grouping - none, 1, 2, 4, the product's (6: N = 2304 walks 6 + 3, N = 3072
    6 + 6; 4 gives 4 + 4 + 1), the row of tiles itself and a group wider than it - and on the product's grid (one tile per block at
    these sizes) under none and the product's; every epilogue, the fp32-residual one also with the fold's outputs (N <= 1024).
    A tile no block takes stays NaN, one taken for another shows as a wrong sum."""
    eng, cus = _eng(), _cus()
    ntn, ntm = N // 256, _round_up(M, 256) // 256
    ops = _operands(mode, M, N, K)
    dev = _Dev(*ops[:4], padded=True)
    plan = _plan_group(eng, N)
    forms = [(EPI_BIAS_RESID, False)] + ([(EPI_BIAS_RESID, True)] if N <= 1024 else []) + [(EPI_BIAS, False), (EPI_BIAS_GELU, False)]
    worst, launches = 0.0, 0
    for code, groups in ((LIST8, sorted({0, 1, 2, 4, plan, ntn, ntn + 3})), (PRODUCT, sorted({0, plan}))):
        for epi, fold in forms:
            for gn in groups:
                for rep in range(2):
                    what = f"{mode} [{M} x {N} x {K}] code {code} epi {epi}{' fold' if fold else ''} group_n {gn} rep {rep}"
                    got, xb, lp, rec = _launch(eng, dev, code, M, N, K, epi, group_n=gn, fold=fold, inplace=rep == 1)
                    _expect(rec, blocks=strip_grid(M, N, 8 if code == LIST8 else 0, cus), strips=0, tiles=ntm * ntn, group_n=gn, what=what)
                    worst = max(worst, _verify(mode, epi, fold, got, xb, lp, ops, what))
                    launches += 1
    report(f"persistent gemm, tile list, {mode} [{M} x {N} x {K}]: {launches} launches (groups of {plan} = the product's), " +
           ("all equal to float64" if mode == "exact" and worst == 0.0 else f"worst err / tol {worst:.3f}" + (" (GELU; the rest equal)" if mode == "exact" else "")))


# ------------------------------------------------------------------------------------------------ strips
# K per shape: the odd counts of 64-deep K-tiles (192, 320) where a strip has several tiles, every K once
STRIP_K = {(STRIPS8, 4736, 256): 192, (STRIPS8, 3200, 256): 320, (STRIPS8, 4096, 256): 128, (STRIPS8, 896, 256): 192, (STRIPS8, 1664, 256): 768,
           (STRIPS8, 1250, 768): 320, (STRIPS8, 1000, 1024): 192, (STRIPS, 2200, 768): 320, (STRIPS, 1000, 1024): 128}
assert set(STRIP_K) == set(STRIP_SHAPES)


@pytest.mark.parametrize("mode", ["exact", "gauss"])
@pytest.mark.parametrize("code,M,N", list(STRIP_SHAPES), ids=lambda v: str(v))
def test_strip_schedule_every_class(mode, code, M, N):
    """The strip schedule at the shapes of pers_schedule.STRIP_SHAPES (half tiles first, in the middle, last and alone, of exactly
    128 rows; short tiles with their window shifted up or clamped to row 0; whole tiles only; strips inside an XCD's blocks and made
    of the left-over blocks; idle blocks; M no multiple of 16), with every epilogue and the fold's outputs."""
    eng, cus = _eng(), _cus()
    K = STRIP_K[(code, M, N)]
    ops = _operands(mode, M, N, K)
    dev = _Dev(*ops[:4], padded=False)
    grid = strip_grid(M, N, 8 if code == STRIPS8 else 0, cus)
    worst = 0.0
    for epi, fold in ((EPI_BIAS_RESID, False), (EPI_BIAS_RESID, True), (EPI_BIAS, False), (EPI_BIAS_GELU, False)):
        for rep in range(2):
            what = f"{mode} strips [{M} x {N} x {K}] code {code} epi {epi}{' fold' if fold else ''} rep {rep}"
            got, xb, lp, rec = _launch(eng, dev, code, M, N, K, epi, fold=fold, inplace=rep == 1)
            _expect(rec, blocks=grid, strips=1, tiles=_round_up(M, 256) // 256 * (N // 256), group_n=0, what=what)
            worst = max(worst, _verify(mode, epi, fold, got, xb, lp, ops, what))
    report(f"persistent gemm, strips on {grid} blocks, {mode} [{M} x {N} x {K}] code {code}: " +
           ("all equal to float64, " if mode == "exact" else "") + f"worst err / tol {worst:.3f}" + (" (GELU)" if mode == "exact" else ""))


# ------------------------------------------------------------------------------------------------ the product's own choice
@pytest.mark.parametrize("M,strips", [(50432, True), (8900, False)])
def test_the_products_choice_of_schedule(M, strips):
    """Tile code 4096 chooses by the shape (pers_strip_wins): the encoder's N = 768 GEMMs at batch 256 (50,432 rows) run strips on
    every compute unit, at 8,900 rows the tile list.  K = 128 keeps the reference cheap; exact operands, in place.  (The fold's
    outputs under strips are test_strip_schedule_every_class's.)"""
    eng, cus = _eng(), _cus()
    N, K = 768, 128
    ops = _operands.__wrapped__("exact", M, N, K)       # (not cached: a gigabyte of float64)
    dev = _Dev(*ops[:4], padded=True)
    grid = strip_grid(M, N, 0, cus)
    assert strip_wins(M, N // 256, grid) == strips or cus != 256
    for rep in range(2):
        what = f"product's schedule [{M} x {N} x {K}] rep {rep}"
        got, xb, lp, rec = _launch(eng, dev, PRODUCT, M, N, K, EPI_BIAS_RESID, inplace=True)
        _expect(rec, blocks=grid, strips=int(strip_wins(M, N // 256, grid)), tiles=_round_up(M, 256) // 256 * 3, group_n=0, what=what)
        if cus == 256:
            assert (rec["strips"], rec["blocks"]) == ((1, 256) if strips else (0, 112)), rec
        _verify("exact", EPI_BIAS_RESID, False, got, xb, lp, ops, what)
    report(f"persistent gemm, code 4096 [{M} x {N} x {K}]: {'strips' if rec['strips'] else 'tile list'} on {rec['blocks']} blocks, equal to float64")


# ------------------------------------------------------------------------------------------------ the fold's consumer
@functools.lru_cache(maxsize=2)
def _fold_operands(M, N, K):
    """rows x with scales and means of their own and an outlier channel, LayerNorm (g, be), W, b -> what the kernel is given
    (x as bf16, W o g as bf16, b + W be, the column sums, the fp32 partials of the rows' statistics per 256-column slice) and
    the real LN(x) W^T + b in float64"""
    rs = np.random.RandomState((M * 131 + N * 17 + K) % (2 ** 31))
    x = (rs.standard_normal((M, K)) * (0.5 + rs.rand(M, 1) * 3) + rs.standard_normal((M, 1)) * 0.7).astype(np.float32)
    x[:, 5] *= 8.0
    g = (1.0 + 0.2 * rs.standard_normal(K)).astype(np.float32).astype(np.float64)
    be = (0.1 * rs.standard_normal(K)).astype(np.float32).astype(np.float64)
    W = (rs.standard_normal((N, K)) * 0.05).astype(np.float32).astype(np.float64)
    b = rs.standard_normal(N).astype(np.float32).astype(np.float64)
    x64 = x.astype(np.float64)
    Wf = _store(W * g, "bf16")
    csum = Wf.sum(1).astype(np.float32)
    bf = (b + W @ be).astype(np.float32)
    part = np.zeros((M, 4, 2), np.float32)
    for t in range(-(-K // 256)):
        seg = x64[:, 256 * t:256 * (t + 1)]
        part[:, t, 0], part[:, t, 1] = seg.sum(1), (seg * seg).sum(1)
    mean = x64.mean(1, keepdims=True)
    var = ((x64 - mean) ** 2).mean(1, keepdims=True)
    real = ((x64 - mean) / np.sqrt(var + 1e-12) * g + be) @ W.T + b
    return _store(x, "bf16"), Wf, csum, bf, part, real


FOLD_CASES = [(LIST8, 700, 2304, 768, -1), (LIST8, 512, 3072, 192, 4), (LIST8, 300, 768, 320, 0), (PRODUCT, 700, 2304, 768, -1),
              (STRIPS8, 1250, 768, 768, 0), (STRIPS8, 1000, 1024, 320, 0), (STRIPS8, 896, 256, 192, 0), (STRIPS8, 4736, 256, 768, 0),
              (STRIPS, 2200, 768, 768, 0)]


@pytest.mark.parametrize("code,M,N,K,gn", FOLD_CASES)
def test_fold_consumer_against_the_identity(code, M, N, K, gn):
    """EPI_BIAS / EPI_BIAS_GELU behind a folded LayerNorm: A = x as bf16, W = bf16(W o g), bias b' = b + W be, csum = column sums of
    the folded weight, ln_part = the rows' (sum, sum of squares) per 256-column slice; the kernel finishes the statistics (mean,
    one-pass variance, rstd) in fp32 and stores rstd (x_b W_f^T - mean csum) + b'.

    Reference: that identity in float64 on exactly these operands and these float32 partials (mean = sum of the partial sums /
    K, var = sum of the partial squares / K - mean^2, eps = 1e-12).  Tolerance, elementwise, before the activation:
      2^-8 |ref|                                        the bf16 store,
      ACC rstd (sum |x_b| |W_f| + |mean| |csum|)        fp32 accumulation of the K products and of the correction term (ACC = 2^-16
                                                        of the sum of the absolute terms, as for every GEMM here), scaled by rstd,
      |ref - b'| 2^-22 (E[x^2] + mean^2) / var          the one-pass variance: E[x^2] and mean^2 each carry a few fp32 roundings
                                                        (four partials added, the division by K, the square), at most 2^-22
                                                        (E[x^2] + mean^2) together on var; rstd = (var + eps)^-1/2 moves by half
                                                        that relative to var, and so does the term it multiplies, ref - b'; the
                                                        other half covers the roundings of 1 / sqrt and of the two fused
                                                        multiply-adds of the epilogue.
    GELU: gpu_util.gemm_bound's rule on that bound.  M and the K slicing: the tile list reads the statistics of rows < M only
    (the partials behind M are NaN); K = 192 and 320 fill one and two slots, the others are zero.
    Second check, as before: against the real LN(x) W^T + b with the unrounded weight, 2e-2 of its largest value."""
    eng, cus = _eng(), _cus()
    xb, Wf, csum, bf, part, real = _fold_operands(M, N, K)
    if gn < 0:
        gn = _plan_group(eng, N)
    strips = code in (STRIPS, STRIPS8)
    dev = _Dev(xb, Wf, bf, None, padded=not strips)
    d_part = torch.full((M + GUARD, 4, 2), float("nan"), device="cuda", dtype=torch.float32)
    d_part[:M] = torch.from_numpy(part).cuda()
    d_csum = _f32(csum)
    p64, c64, b64 = part.astype(np.float64), csum.astype(np.float64), bf.astype(np.float64)
    mean = p64[:, :, 0].sum(1, keepdims=True) / K
    e2 = p64[:, :, 1].sum(1, keepdims=True) / K
    var = e2 - mean * mean
    rstd = 1.0 / np.sqrt(var + 1e-12)
    lin = rstd * (xb @ Wf.T - mean * c64)                       # ref - b'
    s1 = rstd * (np.abs(xb) @ np.abs(Wf).T + np.abs(mean) * np.abs(c64)) + np.abs(lin) * 2.0 ** -22 * (e2 + mean * mean) / var / ACC
    grid = strip_grid(M, N, 8 if code in (LIST8, STRIPS8) else 0, cus)
    for epi in (EPI_BIAS, EPI_BIAS_GELU):
        ref, tol = gemm_bound("bf16", epi, lin + b64, s1, 0.0)          # (b' is inside the product: the bound above has no term for it)
        for rep in range(2):
            what = f"fold consumer [{M} x {N} x {K}] code {code} epi {epi} group_n {gn} rep {rep}"
            got, _, _, rec = _launch(eng, dev, code, M, N, K, epi, group_n=gn, fold=True, part=d_part, csum=d_csum)
            _expect(rec, blocks=grid, strips=int(strips), tiles=_round_up(M, 256) // 256 * (N // 256), group_n=gn, what=what)
            ratio = check_elementwise(got, ref, tol, what)
        r = real if epi == EPI_BIAS else gelu64(real)
        e_real = np.abs(got - r).max() / np.abs(r).max()
        report(f"persistent gemm, fold consumer [{M} x {N} x {K}] code {code} epi {epi} group_n {gn}: vs the identity err / tol {ratio:.3f}, "
               f"vs LN(x) W^T + b {e_real:.3e} (tol 2e-2)")
        assert e_real <= 2e-2


# ------------------------------------------------------------------------------------------------ refusals
def test_gemm_pers_refusals():
    """what mocr_op_gemm_pers refuses itself and what it passes on to the engine's GEMM call and the kernel's launch, each with the
    message of the check that owns it; nothing is written"""
    from manga_ocr._capi import MocrError
    eng = _eng()
    M, N, K = 300, 256, 128
    dA = torch.zeros((512, K), device="cuda", dtype=torch.bfloat16)
    dW = torch.zeros((N, K), device="cuda", dtype=torch.bfloat16)
    dB = torch.zeros(N, device="cuda", dtype=torch.float32)
    dO = _nan((M, N), "fp32")
    dP = torch.zeros((M, 4, 2), device="cuda", dtype=torch.float32)
    dC = torch.zeros(N, device="cuda", dtype=torch.float32)
    dXb = torch.zeros((M, N), device="cuda", dtype=torch.bfloat16)
    ok = dict(M=M, N=N, K=K, epilogue=EPI_BIAS_RESID, tile=LIST8, group_n=0, A=dA, W=dW, bias=dB, out=dO, resid=dO, ln_part=None, csum=None, xb=None)
    lab = "lab" in os.path.basename(os.environ.get("MOCR_LIB", ""))      # the experiments build has the A/B kernels
    torch.cuda.synchronize()
    cases = [(dict(epilogue=0), "epilogue 1"), (dict(epilogue=5), "epilogue 1"), (dict(tile=128), "persistent kernel only"),
             (dict(tile=4200), "gemm tile must be"), (dict(A=None), "bad argument"), (dict(bias=None), "bad argument"), (dict(resid=None), "bad argument"),
             (dict(group_n=-1), "bad argument"), (dict(M=0), "bad argument"), (dict(csum=dC), "bad argument"), (dict(xb=dXb), "bad argument"),
             (dict(N=200), "not tileable"), (dict(K=96), "not tileable"), (dict(K=64), "K must be a multiple of 64, >= 128"),
             (dict(ln_part=dP), "LayerNorm folding needs"), (dict(epilogue=EPI_BIAS, ln_part=dP), "LayerNorm folding needs"),
             (dict(tile=STRIPS8, M=200), "at least 256 rows"), (dict(tile=STRIPS, M=255), "at least 256 rows")]
    if not lab:
        cases.append((dict(tile=4098), "A/B kernel of the experiments build"))
    for change, msg in cases:
        with pytest.raises(MocrError, match=msg):
            eng.op_gemm_pers(**{**ok, **change})
    with pytest.raises(MocrError, match="bf16 engines only"):
        engine("fp32").op_gemm_pers(**ok)
    torch.cuda.synchronize()
    assert torch.isnan(dO).all(), "a refused GEMM wrote its output"
