"""-m gpu: the latent (absorbed K/V) attention block of the decode step - q -> Qt -> latent attention -> ctx - against float64
numpy, called through mocr_op_latent_block, which launches through the same helper as the decode step and so runs the
variants the product picks: fused or two-launch query, query tile and dec_qqt rows per block by regime rows, the GEMM ring
depth, bf16 or fp8 keys, the 16-key T-kernel or the 32-key tile shape.

Every stage is checked on the kernel's own input to that stage, applying the kernel's rounding points:
  q    = bf16(x Wq^T + bq)                        |err| <= 2^-8 |ref| + 2^-16 S1
  Qt_h = bf16(q_h . wkT_h)                        |err| <= 2^-8 |ref| + 2^-16 S1 (+ on the fused path, where q is internal:
                                                  the q elements whose bf16 rounding the fp32 sum can flip, times |wkT|)
  Et_h = bf16(sum_k P_k X_k / sum_k p_k)          |err| <= 2^-8 |ref| + (u_P + e^(2 ds) - 1) A, A = sum_k p_k |X_k|
         P = bf16(p) (u_P = 2^-8); fp8: P = e4m3(256 p) / 256 normalised by its own sum (u_P = 2^-3), e4m3 keys and a
         per-head e4m3 query (the model of test_latent_attention_fp8_kernel), + 2^-18 sum_k |X_k| for e4m3 subnormals
  ctx  = bf16(Et_h Wv_h^T + bv_h)                 |err| <= 2^-8 |ref| + 2^-16 S1
S1 = the sum of the absolute terms (fp32 accumulation), ds = 2^-16 of the scores' absolute terms.  Each check reports its
measured maximum of err / tol.  Contracts: the outputs' guard rows and heads 12..15 stay NaN, NaN input rows past n reach
no row below n, and the rows behind a self context (cache positions L .. max_len-1, holding huge finite values) change no
bit of any output."""
import numpy as np
import pytest

from gpu_util import bf16_round, e4m3_quant, e4m3_table, engine, report

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

D, H, S, MAX_LEN = 768, 12, 197, 300
NO_FUSED_QQT, LATENT_ALWAYS, FP8, TILE32 = 32, 64, 128, 1024
U8 = 2.0 ** -8                  # bf16 rounding, relative (half an ulp)
ACC = 2.0 ** -16                # fp32 accumulation, relative to the sum of the absolute terms
GUARD = 3                       # NaN rows behind every buffer
SX = 8.0 / 448.0                # fp8 key scale: |x| < 8
ENGINES = {"bf16": LATENT_ALWAYS, "bf16-tile32": LATENT_ALWAYS | TILE32, "fp8": LATENT_ALWAYS | FP8,
           "fp8-tile32": LATENT_ALWAYS | FP8 | TILE32}


def _eng(kind, extra=0):
    return engine("bf16", flags=ENGINES[kind] | extra)


def _bf16_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda().to(torch.bfloat16)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.bfloat16)


def _host(t):
    return t.float().cpu().numpy().astype(np.float64)


def _weights(seed, bk_std=0.0):
    """bf16-representable projections (float32 arrays): scores of std ~2.7, q and Et of std ~1; every head has its own
    weight rows and bias slice"""
    rs = np.random.RandomState(seed)
    w = dict(wq=bf16_round((rs.standard_normal((D, D)) * 0.036).astype(np.float32)),
             bq=(rs.standard_normal(D) * 0.3).astype(np.float32),
             wk=bf16_round((rs.standard_normal((D, D)) * 0.096).astype(np.float32)),
             bk=(rs.standard_normal(D) * bk_std).astype(np.float32),
             wv=bf16_round((rs.standard_normal((D, D)) * 0.036).astype(np.float32)),
             bv=(rs.standard_normal(D) * 0.5).astype(np.float32))
    w["wkT"] = (w["wk"].T / 8).astype(np.float32)                  # exact: the layout transposed_scaled() builds
    return w


def _check(got, ref, tol, what):
    """|got - ref| <= tol elementwise; returns the worst err / tol"""
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    err = np.abs(got - ref)
    bad = np.argwhere(err > tol)
    assert bad.size == 0, (f"{what}: {len(bad)} of {err.size} elements out of tolerance, first at {tuple(bad[0])}: "
                           f"got {got[tuple(bad[0])]} want {ref[tuple(bad[0])]} tol {tol[tuple(bad[0])]}")
    return float((err / tol).max())


def _keys_dev(eng, fp8, slots, per_slot, valid, gen, fill=0.0):
    """[slots][per_slot][768] keys on the device: positions < valid standard normal (bf16, or e4m3 through the engine's own
    quantiser), the rest `fill` (alternating sign by column; e4m3: +-448).  Returns (device keys, function slot -> float64
    key rows [valid][768])."""
    x = torch.randn((slots, per_slot, D), generator=gen, device="cuda", dtype=torch.float32).to(torch.bfloat16)
    if fp8:
        x8 = torch.empty((slots, per_slot, D), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                     # the engine's stream does not wait for torch's: x must be written
        eng.op_quant_fp8(x, x8, x.numel(), 1.0 / SX)
        if valid < per_slot:
            x8[:, valid:, 0::2] = 0x7E if fill else 0
            x8[:, valid:, 1::2] = 0xFE if fill else 0
        tab = e4m3_table() * np.float64(np.float32(SX))
        return x8, lambda s: tab[x8[s, :valid].cpu().numpy()]
    if valid < per_slot:
        x[:, valid:, 0::2] = fill
        x[:, valid:, 1::2] = -fill
    return x, lambda s: _host(x[s, :valid])


def _ref_attention(qt, X, fp8):
    """qt [H][768] (the kernel's Qt of one row), X [L][768] float64 keys -> (Et ref, tol) for one row"""
    if fp8:
        q32 = qt.astype(np.float32)
        amax = np.maximum(np.abs(q32).max(-1, keepdims=True), np.float32(1e-30))
        inv = np.float32(448.0) / amax
        qq = e4m3_quant((q32 * inv).astype(np.float64)) * (amax.astype(np.float64) / 448.0)
        up = 2.0 ** -3
    else:
        qq, up = qt, U8
    s = qq @ X.T                                                       # [H][L]
    ds = ACC * (np.abs(qq) @ np.abs(X).T).max(-1, keepdims=True)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    ref = p @ X
    A = p @ np.abs(X)
    tol = U8 * np.abs(ref) + (up + np.expm1(2 * ds)) * A
    if fp8:
        tol = tol + 2.0 ** -18 * np.abs(X).sum(0)
    return ref, tol


def _run_block(kind, n, regime, mode, L, seed, extra_flags=0, w=None, stale=True):
    """one mocr_op_latent_block call with every contract asserted; returns the worst err / tol of each stage"""
    eng = _eng(kind, extra_flags)
    fp8 = kind.startswith("fp8")
    flags = ENGINES[kind] | extra_flags
    rs = np.random.RandomState(seed)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    w = w or _weights(seed)
    N = (n + 127) // 128 * 128
    R = n + 3                                                          # key slots: three belong to no decode slot
    rowmap = rs.permutation(R)[:n].astype(np.int32)
    xin = np.full((N + GUARD, D), np.nan, np.float32)
    xin[:n] = bf16_round(rs.standard_normal((n, D)).astype(np.float32))
    dx = _bf16_dev(xin)
    dw = {k: _bf16_dev(v) for k, v in w.items() if k.startswith("w")}
    db = {k: torch.from_numpy(v).cuda() for k, v in w.items() if k.startswith("b")}
    if mode == "cross":
        # the decode step's cross launch: layer 1's value projection, read from the cross K/V block [k0; v0; k1; v1]
        ckv = torch.cat([_bf16_dev(rs.standard_normal((D, D)).astype(np.float32) * 0.03) for _ in range(3)] + [dw["wv"]])
        ckv_b = torch.cat([torch.zeros(3 * D, device="cuda"), db["bv"]])
        wv, bv = ckv[3 * D:], ckv_b[3 * D:]
        per_slot, valid = S, S
        keys, key_rows = _keys_dev(eng, fp8, R, S, S, gen)
        keys = torch.cat([keys.reshape(R * S, D), torch.zeros((1, D), dtype=keys.dtype, device="cuda")])   # the row behind the last slot
        step = None
    else:
        wv, bv = dw["wv"], db["bv"]
        per_slot, valid = MAX_LEN, L
        keys, key_rows = _keys_dev(eng, fp8, R, MAX_LEN, L, gen, fill=0.0)
        step = torch.from_numpy(np.full(n, L - 1, np.int32)).cuda()
    drm = torch.from_numpy(rowmap).cuda()

    def call(keys_dev):
        out = dict(q=_nan(N + GUARD, D), qt=_nan(N + GUARD, 16, D), et=_nan(N + GUARD, 16, D), ctx=_nan(n + GUARD, D))
        torch.cuda.synchronize()
        eng.op_latent_block(self=1 if mode == "self" else 0, n=n, regime_rows=regime, fixed_len=S if mode == "cross" else 0,
                            x_in=dx, wq=dw["wq"], bq=db["bq"], wkT=dw["wkT"], wv=wv, bv=bv, keys=keys_dev,
                            key_stride=per_slot * D, step=step, rowmap=drm, sx=SX if fp8 else 0.0, **out)
        return out

    out = call(keys)
    fused = (regime or n) >= 257 and not (flags & NO_FUSED_QQT)
    # ---- contracts on the whole buffers (on the device)
    nan = lambda t: bool(torch.isnan(t.float()).all().item())
    fin = lambda t: bool(torch.isfinite(t.float()).all().item())
    assert nan(out["q"][n:]) and (nan(out["q"]) if fused else fin(out["q"][:n])), "q: written iff the two-launch path runs"
    assert nan(out["qt"][:, H:]) and nan(out["qt"][N:]) and fin(out["qt"][:n, :H]), "Qt: heads 12..15 / guard rows written, or NaN leaked"
    assert nan(out["et"][:, H:]) and nan(out["et"][n:]) and fin(out["et"][:n, :H]), "Et: heads 12..15 / rows >= n written, or NaN leaked"
    assert nan(out["ctx"][n:]) and fin(out["ctx"][:n]), "ctx: guard rows written, or NaN leaked"
    if mode == "self" and stale and L < MAX_LEN:
        # the cache positions behind the context hold huge finite values: not one bit of any output may change
        big, _ = _keys_dev(eng, fp8, R, MAX_LEN, L, gen, fill=3.3e38)
        big[:, :L] = keys[:, :L]
        out2 = call(big)
        for k in out:
            assert torch.equal(out[k].view(torch.int16), out2[k].view(torch.int16)), f"{k}: changed by the rows behind the context"
    # ---- float64 references on a sample of rows (all of a small batch)
    rows = np.arange(n) if n <= 160 else np.unique(np.concatenate([np.arange(48), np.arange(n - 48, n), rs.choice(n, 64)]))
    x = xin[rows].astype(np.float64)
    wq, wkT, wvh = (w[k].astype(np.float64) for k in ("wq", "wkT", "wv"))
    got = {k: _host(v[torch.from_numpy(rows).cuda()]) for k, v in out.items()}
    worst = {}
    ref_q = x @ wq.T + w["bq"]
    s1_q = np.abs(x) @ np.abs(wq).T + np.abs(w["bq"])
    if fused:
        q_in = bf16_round(ref_q.astype(np.float32)).astype(np.float64)
        lo = bf16_round((ref_q - ACC * s1_q).astype(np.float32)).astype(np.float64)
        hi = bf16_round((ref_q + ACC * s1_q).astype(np.float32)).astype(np.float64)
        flip = (hi - lo).reshape(len(rows), H, 64)                      # q elements the fp32 sum can round either way
    else:
        worst["q"] = _check(got["q"], ref_q, U8 * np.abs(ref_q) + ACC * s1_q, f"{kind} q n={n}")
        q_in = got["q"]
        flip = np.zeros((len(rows), H, 64))
    qh, wkh = q_in.reshape(-1, H, 64), wkT.reshape(D, H, 64)
    ref_qt = np.einsum("mhk,ihk->mhi", qh, wkh)
    tol_qt = U8 * np.abs(ref_qt) + ACC * np.einsum("mhk,ihk->mhi", np.abs(qh), np.abs(wkh)) + np.einsum("mhk,ihk->mhi", flip, np.abs(wkh))
    worst["Qt"] = _check(got["qt"][:, :H], ref_qt, tol_qt, f"{kind} Qt n={n} regime={regime}")
    ratios = []
    for j, m in enumerate(rows):
        ref_e, tol_e = _ref_attention(got["qt"][j, :H], key_rows(int(rowmap[m])), fp8)
        ratios.append(_check(got["et"][j, :H], ref_e, tol_e, f"{kind} Et {mode} L={valid} n={n} row {m}"))
    worst["Et"] = max(ratios)
    et = got["et"][:, :H]
    wv3 = wvh.reshape(H, 64, D)
    ref_c = np.einsum("mhd,hjd->mhj", et, wv3).reshape(len(rows), D) + w["bv"]
    s1_c = np.einsum("mhd,hjd->mhj", np.abs(et), np.abs(wv3)).reshape(len(rows), D) + np.abs(w["bv"])
    worst["ctx"] = _check(got["ctx"], ref_c, U8 * np.abs(ref_c) + ACC * s1_c, f"{kind} ctx n={n}")
    report(f"latent block {kind}{' +NO_FUSED_QQT' if extra_flags & NO_FUSED_QQT else ''} {mode} n={n} regime={regime or n} "
           f"L={valid} {'fused' if fused else 'two-launch'}: max err/tol " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return worst


# (n, regime_rows, extra engine flags): every branch of the query path, tile 64 / 128 of gemm_dec_qt, dec_qqt rows per block
# 64 / 128, both GEMM ring depths of gemm_dec_ctx (four slots: n < 1280 and at most one block per CU; two above)
QUERY_CASES = [(5, 5, 0), (200, 200, 0), (257, 257, 0), (1100, 1100, 0), (2560, 2560, 0), (100, 2560, 0), (1100, 1100, NO_FUSED_QQT),
               (77, 77, 0), (1300, 1300, NO_FUSED_QQT)]


@pytest.mark.parametrize("kind", list(ENGINES))
@pytest.mark.parametrize("case", range(len(QUERY_CASES)))
def test_latent_block_cross_query_paths(kind, case):
    n, regime, extra = QUERY_CASES[case]
    _run_block(kind, n, regime, "cross", S, 1000 + case, extra)


# (n, L): L = step[0] + 1 over the tile edges of the 16- and 32-key kernels and the last step at max_len 300; n > 768 (bf16)
# / 512 (fp8): the persistent blocks walk several rows each
SELF_CASES = [(5, L) for L in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 197, 299)] + \
    [(1, 2), (1, 299), (300, 33), (300, 197), (1100, 65), (1100, 299), (2560, 17), (2560, 299)]


@pytest.mark.parametrize("kind", list(ENGINES))
@pytest.mark.parametrize("case", range(len(SELF_CASES)))
def test_latent_block_self(kind, case):
    n, L = SELF_CASES[case]
    _run_block(kind, n, 0, "self", L, 2000 + case)


@pytest.mark.parametrize("n", [64, 300])
def test_absorbed_block_equals_classic_attention_with_key_bias(n):
    """The absorbed form drops the key bias bk: softmax ignores the per-query shift q . bk / 8.  ctx against classic
    attention in float64 - softmax((x Wq^T + bq)(X Wk^T + bk)^T / 8)(X Wv^T + bv) per head - on the same bf16 weights.
    Tolerance, from the rounding points: the scores move by ds <= 2^-8 (|q| . |X Wk^T| / 8 + |Qt| . |X|) (bf16 q and Qt),
    so Et by (e^(2 ds) - 1 + 2^-8) A + 2^-8 |Et|, and ctx by that times |Wv_h| + 2^-8 |ctx|."""
    w = _weights(77, bk_std=1.0)
    eng = _eng("bf16")
    rs = np.random.RandomState(n)
    N = (n + 127) // 128 * 128
    xin = np.full((N + GUARD, D), np.nan, np.float32)
    xin[:n] = bf16_round(rs.standard_normal((n, D)).astype(np.float32))
    X = bf16_round(rs.standard_normal((n * S + 1, D)).astype(np.float32))
    out = dict(q=_nan(N + GUARD, D), qt=_nan(N + GUARD, 16, D), et=_nan(N + GUARD, 16, D), ctx=_nan(n + GUARD, D))
    dw = {k: _bf16_dev(w[k]) for k in ("wq", "wkT", "wv")}
    keep = [torch.from_numpy(w[k]).cuda() for k in ("bq", "bv")]
    dx, dX = _bf16_dev(xin), _bf16_dev(X)
    torch.cuda.synchronize()
    eng.op_latent_block(self=0, n=n, regime_rows=0, fixed_len=S, x_in=dx, wq=dw["wq"], bq=keep[0], wkT=dw["wkT"], wv=dw["wv"],
                        bv=keep[1], keys=dX, key_stride=S * D, **out)
    got = _host(out["ctx"][:n])
    x, wq, wk, wv = (a.astype(np.float64) for a in (xin[:n], w["wq"], w["wk"], w["wv"]))
    q = (x @ wq.T + w["bq"]).reshape(n, H, 64)
    worst = 0.0
    for m in range(n):
        Xm = X[m * S:(m + 1) * S].astype(np.float64)
        K = (Xm @ wk.T + w["bk"]).reshape(S, H, 64)
        K0 = (Xm @ wk.T).reshape(S, H, 64)
        V = (Xm @ wv.T + w["bv"]).reshape(S, H, 64)
        s = np.einsum("hk,shk->hs", q[m], K) / 8
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        ref = np.einsum("hs,shj->hj", p, V).reshape(D)
        qt = np.einsum("hk,shk->hs", np.abs(q[m]), np.abs(K0)) / 8                     # |q| . |X Wk^T| / 8
        qtx = np.abs(np.einsum("hk,ihk->hi", q[m], wk.T.reshape(D, H, 64) / 8)) @ np.abs(Xm).T   # |Qt| . |X|
        ds = (U8 * (qt + qtx)).max(-1, keepdims=True)
        et = p @ Xm
        et_err = (np.expm1(2 * ds) + U8) * (p @ np.abs(Xm)) + U8 * np.abs(et)          # [H][768]
        tol = np.einsum("hd,hjd->hj", et_err, np.abs(wv).reshape(H, 64, D)).reshape(D) + U8 * np.abs(ref) + \
            ACC * (np.einsum("hd,hjd->hj", np.abs(et), np.abs(wv).reshape(H, 64, D)).reshape(D) + np.abs(w["bv"]))
        worst = max(worst, _check(got[m], ref, tol, f"absorbed vs classic attention, row {m}"))
    bk_shift = float(np.abs(np.einsum("mhk,hk->mh", q, w["bk"].reshape(H, 64))).max() / 8)
    report(f"absorbed latent block vs classic attention with key bias (n={n}, max |q . bk| / 8 = {bk_shift:.2f}): max err/tol {worst:.3f}")
    assert bk_shift > 1.0                      # the key bias is far from negligible: dropping it is exact only through softmax


def test_latent_block_rejects_bad_arguments():
    from manga_ocr import _capi
    n, N = 4, 128
    x, q, qt, ctx = _nan(N, D), _nan(N, D), _nan(N, 16, D), _nan(n, D)
    w = torch.zeros((D, D), dtype=torch.bfloat16, device="cuda")
    b = torch.zeros(D, device="cuda")
    keys = torch.zeros((MAX_LEN * (n + 1), D), dtype=torch.bfloat16, device="cuda")
    step = torch.zeros(n, dtype=torch.int32, device="cuda")
    ok = dict(self=1, n=n, x_in=x, wq=w, bq=b, wkT=w, wv=w, bv=b, keys=keys, key_stride=MAX_LEN * D, step=step, q=q, qt=qt, et=qt,
              ctx=ctx)
    eng = _eng("bf16")
    for bad in (dict(struct_size=8), dict(x_in=None), dict(ctx=None), dict(step=None), dict(n=0), dict(self=0, fixed_len=0)):
        with pytest.raises(_capi.MocrError):
            eng.op_latent_block(**{**ok, **bad})
    with pytest.raises(_capi.MocrError):
        _eng("fp8").op_latent_block(**{**ok, "sx": 0.0})
