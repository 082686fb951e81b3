"""-m gpu: the kernels of the greedy decode step against float64 numpy statements of the same op, called through the C
ABI's decode operator hooks (mocr_op_dec_attn / _dec_add_ln / _dec_bias_gelu / _dec_token / _gemm_argmax / _smallm_gemm),
which launch through the same helpers - and so the same kernel variants - as the decode step itself.

The references apply the kernels' own rounding points (bf16 operands, the new self K/V rounded to bf16 before it is
attended to, bf16 normalised rows and GELU outputs in the small-batch GEMM, one bf16 rounding of an output); tolerances
follow from those rounding points alone: ~1e-5 of the row scale for fp32 outputs, one bf16 ulp (2^-8 relative) more for
bf16 outputs, exact for ids, lengths, flags, counters and argmax columns.  Outputs that are written twice are compared
with each other exactly.  Every output sits between NaN guard rows / positions that must stay untouched."""
import numpy as np
import pytest

from gpu_util import BF16_ULP, _check_bf16_or_f32, _grid_vals, _ln64, _nan, _store, bf16_round, e4m3_quant, e4m3_table, engine, report, weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

D, H, DH, V, S = 768, 12, 64, 6144, 197
MAX_LEN = 300                       # the engines' max_len: the K/V and latent caches' position stride
NCKV = 2 * D * 2                    # cross K/V block columns (2 decoder layers)
START, EOS, PAD = 2, 3, 0
SENT = -777                         # guard value of int buffers
GUARD = 2                           # guard rows behind every output


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _t(a, dtype):
    """operand of the engine's storage type"""
    t = _f32(a)
    return t.to(torch.bfloat16) if dtype == "bf16" else t


def _np(t):
    return t.float().cpu().numpy().astype(np.float64) if t.dtype != torch.int32 and t.dtype != torch.uint8 else t.cpu().numpy()


def _gelu(x):
    from scipy.special import erf
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


# ------------------------------------------------------------------------------------------------ decode attention
def _attn_ref(q, keys, vals):
    """q [64], keys / vals [L, 64] float64 -> softmax(q k / 8) v"""
    s = keys @ q * 0.125
    p = np.exp(s - s.max())
    return (p @ vals) / p.sum()


# (lengths of the slots, approx_len, nslab, nt): every NG variant (3 / 5 / 8 / 10) and every split of the keys over the
# four waves, waves without keys included (L <= 33); approx_len = the longest row, as the decode step passes it
SELF_CASES = [
    ([1, 2, 3, 4, 5, 31, 32, 33, 96], 96, 1, 0),
    ([1, 2, 3, 4, 5, 31, 32, 33, 96], 96, 8, 1),
    ([97, 160, 1, 33, 64], 160, 2, 0),
    ([161, 256, 2, 5], 256, 3, 1),
    ([257, 299, 300, 1, 100], 300, 6, 0),
    ([300, 257, 160, 97, 3], 300, 12, 1),
    ([33, 2, 161, 96], 256, 24, -1),
]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", range(len(SELF_CASES)))
def test_self_attention_against_float64(dtype, case):
    Ls, approx, nslab, nt = SELF_CASES[case]
    eng = engine(dtype)
    rs = np.random.RandomState(100 + case)
    n = len(Ls)
    R = n + 3                                                     # cache rows: three belong to no slot
    rowmap = rs.permutation(R)[:n].astype(np.int32) if case % 2 == 0 else np.arange(n, dtype=np.int32)
    step = np.array(Ls, np.int32) - 1
    # K/V cache: positions 0 .. step-1 hold keys, everything else NaN (read = poisoned output, written = caught below)
    kc = np.full((R, H, MAX_LEN, DH), np.nan, np.float32)
    vc = np.full((R, H, MAX_LEN, DH), np.nan, np.float32)
    for s in range(n):
        r, Lc = rowmap[s], step[s]
        kc[r, :, :Lc] = rs.standard_normal((H, Lc, DH))
        vc[r, :, :Lc] = rs.standard_normal((H, Lc, DH))
    kc, vc = _store(kc, dtype).astype(np.float32), _store(vc, dtype).astype(np.float32)
    # q | k | v partial sums on a 2^-10 grid: the slab sums are exact; spread 3 makes scores of std ~ 3 (exp range ~ e^20)
    slabs = _grid_vals(rs, (nslab, n, 3 * D), 3.0 / np.sqrt(nslab))
    bias = _grid_vals(rs, 3 * D, 0.5)
    qkv = slabs.astype(np.float64).sum(0) + bias
    q, k_new, v_new = qkv[:, :D], _store(qkv[:, D:2 * D], dtype), _store(qkv[:, 2 * D:], dtype)
    ref = np.zeros((n, D))
    want_k, want_v = kc.astype(np.float64).copy(), vc.astype(np.float64).copy()
    for s in range(n):
        r, Lc = rowmap[s], step[s]
        for h in range(H):
            c = slice(h * DH, (h + 1) * DH)
            keys = np.concatenate([kc[r, h, :Lc].astype(np.float64), k_new[s, c][None]])
            vals = np.concatenate([vc[r, h, :Lc].astype(np.float64), v_new[s, c][None]])
            ref[s, c] = _attn_ref(q[s, c], keys, vals)
            want_k[r, h, Lc] = k_new[s, c]
            want_v[r, h, Lc] = v_new[s, c]
    dk, dv = _t(kc, dtype), _t(vc, dtype)
    dstep, dmap = _i32(step), _i32(rowmap)
    outs = []
    for al in (approx, MAX_LEN):                                   # approx_len is an upper bound: a larger NG, the same result
        dk.copy_(_t(kc, dtype)); dv.copy_(_t(vc, dtype))
        ctx = _nan((n + GUARD, D), dtype)
        torch.cuda.synchronize()
        eng.op_dec_attn(True, _f32(slabs), nslab, _f32(bias), dk, dv, ctx, n, d_step=dstep,
                        d_rowmap=dmap if case % 2 == 0 else None, approx_len=al, nt=nt)
        got = _np(ctx)
        assert np.isnan(got[n:]).all(), "ctx guard rows written"
        np.testing.assert_array_equal(_np(dk), want_k, err_msg="K cache: the new key must land at position L-1 of row rowmap[s], nothing else may change")
        np.testing.assert_array_equal(_np(dv), want_v, err_msg="V cache: the new value must land at position L-1 of row rowmap[s], nothing else may change")
        np.testing.assert_array_equal(_np(dstep), step)
        outs.append(got[:n])
    scale = np.array([max(np.abs(vc[rowmap[s], :, :step[s]]).max(initial=0), np.abs(v_new[s]).max()) for s in range(n)])[:, None]
    ratio, rel = _check_bf16_or_f32(outs[0], ref, scale, dtype, f"self attention {dtype} L={Ls}")
    # a larger NG issues more (clamped, zero-weighted) loads: the same keys and weights, the fp32 code may contract differently
    ratio2, rel2 = _check_bf16_or_f32(outs[1], ref, scale, dtype, f"self attention {dtype} L={Ls} approx_len={MAX_LEN}")
    report(f"dec_attn self {dtype} L={Ls} approx={approx} nslab={nslab} nt={nt}: max err {rel:.2e} of the value scale "
           f"({ratio:.2f} of tol); approx_len={MAX_LEN}: {rel2:.2e} ({ratio2:.2f} of tol)")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_self_attention_non_temporal_policy_by_rows(dtype):
    """n >= MOCR_ATTN_NT_ROWS (128): the decode step's own choice (nt = -1) streams K/V non-temporally; same values either way"""
    eng = engine(dtype)
    rs = np.random.RandomState(7)
    n, L = 130, 10
    rowmap = rs.permutation(n).astype(np.int32)
    step = np.full(n, L - 1, np.int32)
    kc = _store(rs.standard_normal((n, H, MAX_LEN, DH)).astype(np.float32), dtype).astype(np.float32)
    vc = _store(rs.standard_normal((n, H, MAX_LEN, DH)).astype(np.float32), dtype).astype(np.float32)
    slabs = _grid_vals(rs, (2, n, 3 * D), 2.0)
    bias = _grid_vals(rs, 3 * D, 0.5)
    got = []
    for nt in (-1, 0):
        dk, dv, ctx = _t(kc, dtype), _t(vc, dtype), _nan((n + GUARD, D), dtype)
        torch.cuda.synchronize()
        eng.op_dec_attn(True, _f32(slabs), 2, _f32(bias), dk, dv, ctx, n, d_step=_i32(step), d_rowmap=_i32(rowmap), approx_len=L, nt=nt)
        g = _np(ctx)
        assert np.isnan(g[n:]).all()
        got.append(g[:n])
    np.testing.assert_array_equal(got[0], got[1])
    qkv = slabs.astype(np.float64).sum(0) + bias
    ref = np.zeros((n, D))
    for s in range(0, n, 13):
        r = rowmap[s]
        for h in range(H):
            c = slice(h * DH, (h + 1) * DH)
            keys = np.concatenate([kc[r, h, :L - 1], _store(qkv[s, D:2 * D], dtype)[c][None]])
            vals = np.concatenate([vc[r, h, :L - 1], _store(qkv[s, 2 * D:], dtype)[c][None]])
            ref[s, c] = _attn_ref(qkv[s, c], keys.astype(np.float64), vals.astype(np.float64))
    idx = np.arange(0, n, 13)
    scale = max(np.abs(vc[:, :, :L - 1]).max(), np.abs(_store(qkv[:, 2 * D:], dtype)).max())
    ratio, rel = _check_bf16_or_f32(got[0][idx], ref[idx], scale, dtype, f"self attention nt {dtype}")
    report(f"dec_attn self {dtype} n={n} nt by rows = forced 0 bit-identical; max err {rel:.2e} of the value scale ({ratio:.2f} of tol)")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("nslab,layer", [(1, 0), (3, 1), (8, 0), (24, 1)])
def test_cross_attention_against_float64(dtype, nslab, layer):
    eng = engine(dtype)
    rs = np.random.RandomState(nslab * 10 + layer)
    n, R = 6, 9
    rowmap = rs.permutation(R)[:n].astype(np.int32)
    ckv = _store(rs.standard_normal((R, S, NCKV)).astype(np.float32), dtype).astype(np.float32)
    slabs = _grid_vals(rs, (nslab, n, D), 3.0 / np.sqrt(nslab))
    bias = _grid_vals(rs, D, 0.5)
    q = slabs.astype(np.float64).sum(0) + bias
    ref = np.zeros((n, D))
    for s in range(n):
        kv = ckv[rowmap[s]].astype(np.float64)
        for h in range(H):
            c = slice(h * DH, (h + 1) * DH)
            ref[s, c] = _attn_ref(q[s, c], kv[:, layer * 2 * D + h * DH:layer * 2 * D + (h + 1) * DH],
                                  kv[:, layer * 2 * D + D + h * DH:layer * 2 * D + D + (h + 1) * DH])
    dckv, ctx = _t(ckv, dtype), _nan((n + GUARD, D), dtype)
    torch.cuda.synchronize()
    eng.op_dec_attn(False, _f32(slabs), nslab, _f32(bias), dckv, None, ctx, n, layer=layer, d_rowmap=_i32(rowmap))
    got = _np(ctx)
    assert np.isnan(got[n:]).all(), "ctx guard rows written"
    np.testing.assert_array_equal(_np(dckv), ckv.astype(np.float64), err_msg="cross K/V block modified")
    ratio, rel = _check_bf16_or_f32(got[:n], ref, np.abs(ckv).max(), dtype, f"cross attention {dtype}")
    report(f"dec_attn cross {dtype} nslab={nslab} layer={layer}: max err {rel:.2e} of the value scale ({ratio:.2f} of tol)")


# ------------------------------------------------------------------------------------------------ slab sum + LayerNorm
def _run_add_ln(eng, dtype, slabs, bias, resid, g, b, gelu, with_f32, cache=None, step=None, rowmap=None, inv_sx=0.0):
    rows = slabs.shape[1]
    out_f32 = torch.full((rows + GUARD, D), float("nan"), device="cuda") if with_f32 else None
    out_t = _nan((rows + GUARD, D), dtype)
    torch.cuda.synchronize()
    eng.op_dec_add_ln(_f32(slabs), slabs.shape[0], _f32(bias), None if resid is None else _f32(resid), _f32(g), _f32(b), gelu,
                      out_f32, out_t, rows, d_cache=cache, cache_fp8=cache is not None and cache.dtype == torch.uint8,
                      inv_sx=inv_sx, d_step=step, d_rowmap=rowmap)
    o32 = _np(out_f32) if with_f32 else None
    ot = _np(out_t)
    assert np.isnan(ot[rows:]).all() and (o32 is None or np.isnan(o32[rows:]).all()), "guard rows written"
    return (o32[:rows] if with_f32 else None), ot[:rows]


# nslab x (residual, GELU, fp32 output, cache): the 8-wide slab loads clamp and zero-weight the tail when nslab % 8 != 0
ADD_LN_CASES = [(1, True, False, True, "t"), (2, False, True, True, None), (3, True, False, False, "t"), (6, True, False, True, "e4m3"),
                (8, False, True, False, None), (12, True, False, True, "t"), (13, True, True, True, "e4m3"), (24, False, False, True, "t")]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("nslab,with_resid,gelu,with_f32,cache", ADD_LN_CASES)
def test_add_layernorm_against_float64(dtype, nslab, with_resid, gelu, with_f32, cache):
    if cache == "e4m3" and dtype != "bf16":
        cache = "t"                                  # the fp8 latent cache exists in bf16 engines only
    eng = engine(dtype)
    rs = np.random.RandomState(nslab + 100 * gelu)
    rows, R = 11, 14
    slabs = _grid_vals(rs, (nslab, rows, D), 1.5 / np.sqrt(nslab))
    bias = _grid_vals(rs, D, 0.5)
    resid = rs.standard_normal((rows, D)).astype(np.float32) if with_resid else None
    g = (1 + 0.3 * rs.standard_normal(D)).astype(np.float32)
    b = (0.2 * rs.standard_normal(D)).astype(np.float32)
    v = slabs.astype(np.float64).sum(0) + bias
    gelu_err = 0.0
    if gelu:
        v = _gelu(v)
        gelu_err = 3e-5 if dtype == "bf16" else 0.0             # gelu_fast's bound against the erf form
    if with_resid:
        v = v + resid
    ref, mean, std = _ln64(v, g.astype(np.float64), b.astype(np.float64))
    rowmap = rs.permutation(R)[:rows].astype(np.int32)
    step = rs.randint(0, MAX_LEN, rows).astype(np.int32)
    dcache = None
    inv_sx = 0.0
    if cache == "t":
        dcache = _nan((R, MAX_LEN, D), dtype)
    elif cache == "e4m3":
        dcache = torch.full((R, MAX_LEN, D), 0x7F, dtype=torch.uint8, device="cuda")    # 0x7F = e4m3 NaN
        inv_sx = float(np.float32(400.0 / np.abs(ref).max()))                              # |out * inv_sx| <= 448
    o32, ot = _run_add_ln(eng, dtype, slabs, bias, resid, g, b, gelu, with_f32, dcache,
                          _i32(step) if dcache is not None else None, _i32(rowmap) if dcache is not None else None, inv_sx)
    scale = np.abs(ref).max(-1, keepdims=True)
    extra = gelu_err * (np.abs(g).max() / std)[:, None]
    what = f"dec_add_ln {dtype} nslab={nslab} resid={with_resid} gelu={gelu}"
    if o32 is not None:
        ratio, rel = _check_bf16_or_f32(o32, ref, scale, "fp32", what + " out_f32", extra)
        np.testing.assert_array_equal(ot, _store(o32, dtype), err_msg="out_t must be the storage rounding of out_f32")
    else:
        ratio, rel = _check_bf16_or_f32(ot, ref, scale, dtype, what + " out_t", extra)
    if dcache is not None:
        got_c = _np(dcache)
        if cache == "e4m3":
            got_c = e4m3_table()[got_c]
        written = np.zeros((R, MAX_LEN), bool)
        written[rowmap, step] = True
        assert np.isnan(got_c[~written]).all(), "cache written outside row rowmap[s], position step[s]"
        if cache == "e4m3":
            want = e4m3_quant((o32.astype(np.float32) * np.float32(inv_sx)).astype(np.float64))
            np.testing.assert_array_equal(got_c[rowmap, step], want, err_msg="e4m3 cache row != e4m3(out_f32 * inv_sx)")
        else:
            np.testing.assert_array_equal(got_c[rowmap, step], ot, err_msg="cache row != out_t")
    report(f"{what} cache={cache}: max err {rel:.2e} of the row scale ({ratio:.2f} of tol)")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_add_layernorm_hostile_rows(dtype):
    """a DC offset of ~50 under a spread of ~1e-2 and one outlier channel (the hostile-statistics goldens' rows): the fp32
    row sum carries rounding errors of ~u |mean|; the bound grows with |mean| / std and is applied to these rows only"""
    eng = engine(dtype)
    rs = np.random.RandomState(5)
    rows, nslab = 8, 3
    slabs = (rs.standard_normal((nslab, rows, D)) * 1e-2 / np.sqrt(nslab)).astype(np.float32)
    bias = (rs.standard_normal(D) * 1e-3).astype(np.float32)
    resid = (50.0 + rs.standard_normal((rows, D)) * 1e-2 * rs.uniform(0.5, 2, (rows, 1))).astype(np.float32)
    resid[1::2, 17] += 0.5                                                           # outlier channel on every other row
    g = (1 + 0.3 * rs.standard_normal(D)).astype(np.float32)
    b = (0.2 * rs.standard_normal(D)).astype(np.float32)
    v = slabs.astype(np.float64).sum(0) + bias + resid
    ref, mean, std = _ln64(v, g.astype(np.float64), b.astype(np.float64))
    o32, ot = _run_add_ln(eng, dtype, slabs, bias, resid, g, b, False, True)
    u = 2.0 ** -24
    cond = (np.abs(mean) / std)[:, None]
    # each element of v = fp32(sum + bias + resid) is off by up to u |mean| (u = 2^-24), the fp32 row sum by up to
    # ~log2(768) u |mean| per element: in units of the row's std ~ 16 u |mean| / std, times |gamma| in the output
    extra = 16 * u * cond * np.abs(g).max()
    scale = np.abs(ref).max(-1, keepdims=True)
    ratio, rel = _check_bf16_or_f32(o32, ref, scale, "fp32", f"dec_add_ln hostile {dtype}", extra)
    np.testing.assert_array_equal(ot, _store(o32, dtype))
    report(f"dec_add_ln hostile {dtype}: |mean|/std up to {cond.max():.0f}, max err {rel:.2e} of the row scale "
           f"({ratio:.2f} of the conditioning bound {float((extra / scale).max()):.1e} + 1e-5)")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("rows,N,nslab", [(3, 772, 1), (5, 3072, 2), (7, 3072, 3), (1, 3076, 6)])
def test_bias_gelu_against_float64(dtype, rows, N, nslab):
    """rows x N not a multiple of the 1024 elements a block covers; odd and even slab counts"""
    eng = engine(dtype)
    rs = np.random.RandomState(rows * N + nslab)
    slabs = _grid_vals(rs, (nslab, rows, N), 1.5 / np.sqrt(nslab))
    bias = _grid_vals(rs, N, 0.5)
    ref = _gelu(slabs.astype(np.float64).sum(0) + bias)
    out = _nan((rows * N + 1024,), dtype)
    torch.cuda.synchronize()
    eng.op_dec_bias_gelu(_f32(slabs), nslab, _f32(bias), out, rows, N)
    got = _np(out)
    assert np.isnan(got[rows * N:]).all(), "written past rows x N"
    got = got[:rows * N].reshape(rows, N)
    extra = 3e-5 if dtype == "bf16" else 0.0
    ratio, rel = _check_bf16_or_f32(got, ref, np.abs(ref).max(-1, keepdims=True), dtype, f"dec_bias_gelu {dtype}", extra)
    report(f"dec_bias_gelu {dtype} rows={rows} N={N} nslab={nslab}: max err {rel:.2e} of the row scale ({ratio:.2f} of tol)")


# ------------------------------------------------------------------------------------------------ token step
def _argmax_rule(logits):
    """the kernel's rule: NaN never wins; the lowest column wins a tie; a row without any value above -inf picks 0"""
    out = np.zeros(logits.shape[0], np.int64)
    for i, row in enumerate(logits):
        r = np.where(np.isnan(row), -np.inf, row)
        out[i] = 0 if not (r > -np.inf).any() else int(np.argmax(r))
    return out


def _emb_ref(w, tok, pos):
    d = "decoder.bert.embeddings."
    x = (w[d + "word_embeddings.weight"][tok].astype(np.float64) + w[d + "token_type_embeddings.weight"][0]
         + w[d + "position_embeddings.weight"][pos])
    return _ln64(x, w[d + "LayerNorm.weight"].astype(np.float64), w[d + "LayerNorm.bias"].astype(np.float64))[0]


def _tie_logits(rs, n):
    """integer-valued logits [n, V] (exact fp32 sums in any order) with planted ties and special rows; slot -> description"""
    lg = rs.randint(-1000, 1000, (n, V)).astype(np.float64)
    plan = {}
    def plant(s, cols, what, top=5000):
        lg[s, cols] = top
        plan[s] = what
    plant(0, [4 * 37 + 1, 4 * 37 + 3], "within one thread's float4")
    plant(1, [4 * 77 + 2, 4 * 77 + 2 + 1024], "columns c and c + 1024 of one thread")
    plant(2, [4 * 9 + 1, 4 * 5 + 3], "across lanes of one wave")
    plant(3, [4 * 200, 4 * 10 + 3], "across waves")
    plant(4, [6143, 0], "columns 0 and 6143")
    plant(5, [1024 * 5, 1023], "higher column in the lower thread")
    plant(6, [EOS, 4000], "EOS ties a later column: EOS wins")
    lg[7] = -np.inf; plan[7] = "-inf row"
    lg[8] = -np.inf; lg[8, 2345] = -5.0; plan[8] = "-inf row with one finite column"
    lg[9, rs.choice(V, 50, replace=False)] = np.nan; lg[9, [3001, 3002]] = 7000; lg[9, 3000] = np.nan; plan[9] = "NaN columns never win"
    lg[10] = np.nan; plan[10] = "all-NaN row"
    plant(11, [5000, 5001, 100], "three-way tie")
    return lg, plan


def _token_state(rs, n, R, max_len, ids_ld):
    rowmap = rs.permutation(R)[:n].astype(np.int32)
    step = rs.randint(1, max_len - 2, n).astype(np.int32)
    finished = np.zeros(R, np.int32)
    lens = np.full(R, max_len, np.int32)
    ids = np.full((R + 1, ids_ld), SENT, np.int32)                 # + a guard row
    return rowmap, step, finished, lens, ids


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("path", ["slabs1", "slabs3", "cand64", "cand128"])
def test_token_step_ties_finish_rules_and_embedding(dtype, path):
    eng = engine(dtype)
    w = weights(0)
    rs = np.random.RandomState({"slabs1": 1, "slabs3": 3, "cand64": 64, "cand128": 128}[path])
    n, R, max_len, ids_ld = 20, 24, 40, 40
    lg, plan = _tie_logits(rs, n)
    rowmap, step, finished, lens, ids = _token_state(rs, n, R, max_len, ids_ld)
    # finish rules: slot 12's row is already finished, slot 13 reaches max_len, slot 14 is on the ids_ld guard,
    # slots 15 / 16 emit EOS (16's row was finished before: it must not count twice)
    finished[rowmap[12]] = 1; lens[rowmap[12]] = 17
    step[13] = max_len - 2
    step[14] = ids_ld - 1
    lg[15] = rs.randint(-1000, 1000, V); lg[15, EOS] = 9000; plan[15] = "EOS"
    lg[16] = lg[15]; finished[rowmap[16]] = 1; lens[rowmap[16]] = 9
    n_unf0 = 11
    kw = {}
    if path.startswith("slabs"):
        nslab = int(path[5:])
        bias = rs.randint(-100, 100, V).astype(np.float64)
        parts = rs.randint(-300, 300, (nslab, n, V)).astype(np.float64)
        parts[-1] = np.where(np.isfinite(lg), lg - bias - parts[:-1].sum(0), lg)     # -inf / NaN columns stay -inf / NaN
        kw.update(slabs=_f32(parts), nslab=nslab, vbias=_f32(bias))
    else:
        tile = int(path[4:])
        nc = V // tile
        t = lg.reshape(n, nc, tile)
        tt = np.where(np.isnan(t), -np.inf, t)
        cval = tt.max(-1)
        cidx = np.argmax(tt, -1) + np.arange(nc) * tile
        allnan = np.isnan(t).all(-1)
        cidx[allnan] = 0x7FFFFFFF                                    # what EPI_ARGMAX leaves for a tile without a number
        kw.update(cand_val=_f32(cval), cand_idx=_i32(cidx), ncand=nc)
    best = _argmax_rule(lg)
    d_ids, d_step, d_fin, d_len = _i32(ids), _i32(step), _i32(finished), _i32(lens)
    d_unf, d_map = _i32([n_unf0, SENT]), _i32(rowmap)
    x32 = torch.full((n + GUARD, D), float("nan"), device="cuda")
    xt = _nan((n + GUARD, D), dtype)
    cache = _nan((R, MAX_LEN, D), dtype)
    torch.cuda.synchronize()
    eng.op_dec_token(first=0, n=n, ids=d_ids, step=d_step, finished=d_fin, len=d_len, n_unfinished=d_unf, rowmap=d_map,
                     ids_ld=ids_ld, max_len=max_len, n_real=n, x_f32=x32, x_t=xt, cache=cache, **kw)
    # expected state
    want_ids, want_fin, want_len = ids.copy(), finished.copy(), lens.copy()
    toks = np.zeros(n, np.int64)
    n_unf = n_unf0
    for s in range(n):
        r, t = rowmap[s], step[s]
        fin = finished[r]
        tok = PAD if fin else best[s]
        toks[s] = tok
        if t + 1 < ids_ld:
            want_ids[r, t + 1] = tok
        if not fin and (tok == EOS or t + 2 >= max_len):
            want_fin[r] = 1
            want_len[r] = t + 2
            n_unf -= 1
    got_ids = d_ids.cpu().numpy()
    for s, what in sorted(plan.items()):
        assert got_ids[rowmap[s], step[s] + 1] == want_ids[rowmap[s], step[s] + 1], f"{path} slot {s} ({what})"
    np.testing.assert_array_equal(got_ids, want_ids, err_msg="ids (only ids[rowmap[s], step[s]+1] may change)")
    np.testing.assert_array_equal(d_fin.cpu().numpy(), want_fin, err_msg="finished")
    np.testing.assert_array_equal(d_len.cpu().numpy(), want_len, err_msg="len")
    np.testing.assert_array_equal(d_unf.cpu().numpy(), [n_unf, SENT], err_msg="n_unfinished")
    np.testing.assert_array_equal(d_step.cpu().numpy(), step + 1)
    np.testing.assert_array_equal(d_map.cpu().numpy(), rowmap)
    assert ((toks >= 0) & (toks < V)).all()
    # the chosen token's embedding + LayerNorm at position t + 1: x by slot, the cache by row
    ref = np.stack([_emb_ref(w, toks[s], step[s] + 1) for s in range(n)])
    g32, gt, gc = _np(x32), _np(xt), _np(cache)
    assert np.isnan(g32[n:]).all() and np.isnan(gt[n:]).all(), "x guard rows written"
    ratio, rel = _check_bf16_or_f32(g32[:n], ref, np.abs(ref).max(-1, keepdims=True), "fp32", f"dec_token x_f32 {dtype}")
    np.testing.assert_array_equal(gt[:n], _store(g32[:n], dtype), err_msg="x_t != storage rounding of x_f32")
    written = np.zeros((R, MAX_LEN), bool)
    written[rowmap, step + 1] = True
    assert np.isnan(gc[~written]).all(), "cache written outside row rowmap[s], position step[s] + 1"
    np.testing.assert_array_equal(gc[rowmap, step + 1], gt[:n], err_msg="cache row != x_t")
    report(f"dec_token {dtype} {path}: {len(plan)} planted tie / special rows exact, finish rules exact, "
           f"embedding max err {rel:.2e} of the row scale ({ratio:.2f} of tol)")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_token_step_forced_ids_and_first_step(dtype):
    eng = engine(dtype)
    w = weights(0)
    rs = np.random.RandomState(11)
    n, R, max_len, ids_ld, n_real = 9, 9, 30, 30, 6
    # FIRST: start token, identity rowmap, rows >= n_real born finished, n_unfinished = n_real, position 0
    ids = np.full((R + 1, ids_ld), SENT, np.int32)
    d_ids, d_step, d_fin = _i32(ids), _i32(np.full(n, SENT)), _i32(np.full(R, SENT))
    d_len, d_unf, d_map = _i32(np.full(R, SENT)), _i32([SENT, SENT]), _i32(np.full(n, SENT))
    x32 = torch.full((n + GUARD, D), float("nan"), device="cuda")
    xt = _nan((n + GUARD, D), dtype)
    cache = torch.full((R, MAX_LEN, D), 0x7F, dtype=torch.uint8, device="cuda") if dtype == "bf16" else _nan((R, MAX_LEN, D), dtype)
    inv_sx = 40.0
    torch.cuda.synchronize()
    eng.op_dec_token(first=1, n=n, ids=d_ids, step=d_step, finished=d_fin, len=d_len, n_unfinished=d_unf, rowmap=d_map,
                     ids_ld=ids_ld, max_len=max_len, n_real=n_real, x_f32=x32, x_t=xt, cache=cache,
                     cache_fp8=int(dtype == "bf16"), inv_sx=inv_sx)
    want_ids = ids.copy()
    want_ids[:n, 0] = START
    np.testing.assert_array_equal(d_ids.cpu().numpy(), want_ids)
    np.testing.assert_array_equal(d_step.cpu().numpy(), np.zeros(n))
    np.testing.assert_array_equal(d_fin.cpu().numpy(), (np.arange(R) >= n_real).astype(np.int32))
    np.testing.assert_array_equal(d_len.cpu().numpy(), np.full(R, max_len))
    np.testing.assert_array_equal(d_unf.cpu().numpy(), [n_real, SENT])
    np.testing.assert_array_equal(d_map.cpu().numpy(), np.arange(n))
    ref = np.stack([_emb_ref(w, START, 0)] * n)
    g32 = _np(x32)
    assert np.isnan(g32[n:]).all()
    ratio, rel = _check_bf16_or_f32(g32[:n], ref, np.abs(ref).max(-1, keepdims=True), "fp32", f"dec_token first {dtype}")
    np.testing.assert_array_equal(_np(xt)[:n], _store(g32[:n], dtype))
    gc = _np(cache)
    if dtype == "bf16":
        gc = e4m3_table()[gc]
        np.testing.assert_array_equal(gc[:n, 0], e4m3_quant((g32[:n].astype(np.float32) * np.float32(inv_sx)).astype(np.float64)),
                                      err_msg="e4m3 cache row != e4m3(x_f32 * inv_sx)")
    else:
        np.testing.assert_array_equal(gc[:n, 0], g32[:n])
    assert np.isnan(gc[:, 1:]).all()
    # forced ids override the argmax (and the finish rules): tok = forced[s][t+1], pad beyond forced_T
    T = 12
    forced = rs.randint(4, V, (n, T)).astype(np.int32)
    forced[2, 6] = EOS
    step = np.array([0, 3, 5, 10, 11, 2, 7, 1, 4], np.int32)
    lg = rs.randint(-100, 100, (n, V)).astype(np.float64)
    fin0 = d_fin.cpu().numpy().copy()
    ids1 = d_ids.cpu().numpy().copy()
    d_step.copy_(_i32(step))
    torch.cuda.synchronize()
    eng.op_dec_token(first=0, n=n, slabs=_f32(lg), nslab=1, vbias=_f32(np.zeros(V)), forced=_i32(forced), forced_T=T,
                     ids=d_ids, step=d_step, finished=d_fin, len=d_len, n_unfinished=d_unf, rowmap=d_map,
                     ids_ld=ids_ld, max_len=max_len, n_real=n_real, x_f32=x32, x_t=xt)
    toks = np.array([forced[s, step[s] + 1] if step[s] + 1 < T else PAD for s in range(n)])
    ids1[np.arange(n), step + 1] = toks
    np.testing.assert_array_equal(d_ids.cpu().numpy(), ids1)
    np.testing.assert_array_equal(d_fin.cpu().numpy(), fin0, err_msg="forced steps finish no row")
    np.testing.assert_array_equal(d_unf.cpu().numpy(), [n_real, SENT])
    ref = np.stack([_emb_ref(w, toks[s], step[s] + 1) for s in range(n)])
    _check_bf16_or_f32(_np(x32)[:n], ref, np.abs(ref).max(-1, keepdims=True), "fp32", f"dec_token forced {dtype}")
    report(f"dec_token {dtype}: first step and forced ids exact, start embedding max err {rel:.2e} ({ratio:.2f} of tol)")


# ------------------------------------------------------------------------------------------------ LM-head argmax GEMM
def _tile_argmax(logits, tile):
    M, N = logits.shape
    t = logits.reshape(M, N // tile, tile)
    return t.max(-1), np.argmax(t, -1) + np.arange(N // tile) * tile


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("M", [1, 37, 64, 128, 1000])
def test_fused_argmax_gemm_exact_ties(dtype, tile, M):
    """integer operands (exact fp32 products and sums) with duplicated weight rows: ties inside one 16-column swizzle
    group, across swizzle groups and across the threads of a row are real ties; (value, column) must be exact"""
    eng = engine(dtype)
    rs = np.random.RandomState(M + tile)
    N, K = V, D
    Mp = (M + tile - 1) // tile * tile
    A = np.zeros((Mp, K), np.float32)
    A[:M] = rs.randint(1, 4, (M, K))                                    # positive rows: the all-3 weight row is every row's max
    A[1:M:3] = rs.randint(-3, 4, (len(range(1, M, 3)), K))              # ... except on every third row: natural ties
    W = rs.randint(-3, 3, (N, K)).astype(np.float32)
    bias = rs.randint(-4, 5, N).astype(np.float32)
    top = np.full(K, 3, np.float32)
    nt = N // tile
    for j in range(nt):                                                 # per tile: a tie of the planted kind
        kind = j % 4
        c0 = j * tile + rs.randint(0, 16)
        c1 = {0: (c0 - j * tile) // 16 * 16 + j * tile + (c0 % 16 + 1 + rs.randint(0, 15)) % 16,    # same 16-column group
              1: j * tile + (c0 - j * tile + 16 * rs.randint(1, tile // 16)) % tile,               # another group
              2: j * tile + tile - 1 - rs.randint(0, 4),                                          # another thread
              3: c0}[kind]
        for c in {c0, c1}:
            W[c] = top
            bias[c] = 7
    logits = A[:M].astype(np.float64) @ W.astype(np.float64).T + bias
    want_v, want_i = _tile_argmax(logits, tile)
    cv = torch.full((M + GUARD, nt), float("nan"), device="cuda")
    ci = torch.full((M + GUARD, nt), SENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.op_gemm_argmax(_t(A, dtype), _t(W, dtype), _f32(bias), cv, ci, M, N, K, tile)
    gv, gi = cv.cpu().numpy(), ci.cpu().numpy()
    assert np.isnan(gv[M:]).all() and (gi[M:] == SENT).all(), "guard rows written"
    ties = int(sum((logits.reshape(M, nt, tile) == want_v[..., None]).sum(-1).ravel() > 1))
    np.testing.assert_array_equal(gv[:M], want_v, err_msg="tile maxima")
    np.testing.assert_array_equal(gi[:M], want_i, err_msg="tile argmax columns (lowest column wins a tie)")
    report(f"gemm EPI_ARGMAX {dtype} tile={tile} M={M}: exact over {M * nt} (row, tile) pairs, {ties} of them ties")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("tile,M", [(64, 37), (128, 300)])
def test_fused_argmax_gemm_random_floats(dtype, tile, M):
    eng = engine(dtype)
    rs = np.random.RandomState(3 * M + tile)
    N, K = V, D
    Mp = (M + tile - 1) // tile * tile
    A = rs.standard_normal((Mp, K)).astype(np.float32)
    W = (rs.standard_normal((N, K)) * 0.05).astype(np.float32)
    bias = rs.standard_normal(N).astype(np.float32)
    if dtype == "bf16":
        A, W = bf16_round(A), bf16_round(W)
    logits = A[:M].astype(np.float64) @ W.astype(np.float64).T + bias
    want_v, want_i = _tile_argmax(logits, tile)
    nt = N // tile
    srt = np.sort(logits.reshape(M, nt, tile), -1)
    margin = srt[..., -1] - srt[..., -2]
    cv = torch.full((M + GUARD, nt), float("nan"), device="cuda")
    ci = torch.full((M + GUARD, nt), SENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.op_gemm_argmax(_t(A, dtype), _t(W, dtype), _f32(bias), cv, ci, M, N, K, tile)
    gv, gi = cv.cpu().numpy()[:M].astype(np.float64), ci.cpu().numpy()[:M]
    assert np.isnan(cv.cpu().numpy()[M:]).all() and (ci.cpu().numpy()[M:] == SENT).all()
    clear = margin > 1e-3
    np.testing.assert_array_equal(gi[clear], want_i[clear])
    scale = (np.abs(A[:M]).astype(np.float64) @ np.abs(W).astype(np.float64).T).max()
    err = np.abs(gv - want_v).max() / scale
    assert err <= 1e-5, err
    report(f"gemm EPI_ARGMAX {dtype} tile={tile} M={M} random: columns exact on {int(clear.sum())}/{clear.size} pairs with "
           f"margin > 1e-3, value err {err:.2e} of sum |a w|")


# ------------------------------------------------------------------------------------------------ small-batch GEMM
# (pro, epi, N, K, residual form): the projections decode_step_smallm launches
SMALLM = {
    "qkv0": (0, 0, 3 * D, D, None),
    "qkv_ln": (1, 0, 3 * D, D, None),
    "qc": (1, 0, D, D, None),
    "proj": (0, 1, D, D, "plain"),
    "proj_ln": (0, 1, D, D, "stats"),
    "fc1": (1, 2, 4 * D, D, None),
    "fc2": (0, 1, D, 4 * D, "stats"),
    "transform": (1, 3, D, D, None),
    "vocab": (1, 0, V, D, None),
}
SMALLM_CASES = [(k, r) for k in SMALLM for r in ([1, 17, 32] if k == "vocab" else [1, 2, 15, 16, 17, 31, 32])]


@pytest.mark.parametrize("which,rows", SMALLM_CASES)
def test_smallm_gemm_against_float64(which, rows):
    pro, epi, N, K, rform = SMALLM[which]
    eng = engine("bf16")
    rs = np.random.RandomState(rows * 7 + len(which))
    ldo = N + 16 if rows % 2 else N
    W = bf16_round((rs.standard_normal((N, K)) * 0.05).astype(np.float32))
    bias = rs.standard_normal(N).astype(np.float32)
    kw = dict(pro=pro, epi=epi, rows=rows, K=K, N=N, ldo=ldo, w=_t(W, "bf16"), bias=_f32(bias))
    flip = 0.0
    if pro == 0:
        A = bf16_round(rs.standard_normal((rows, K)).astype(np.float32)).astype(np.float64)
        kw["a_bf16"] = _t(A, "bf16")
    else:
        x = (rs.standard_normal((rows, K)) * rs.uniform(0.5, 3, (rows, 1)) + rs.uniform(-2, 2, (rows, 1))).astype(np.float32)
        g = (1 + 0.3 * rs.standard_normal(K)).astype(np.float32)
        b = (0.2 * rs.standard_normal(K)).astype(np.float32)
        ln, mean, std = _ln64(x.astype(np.float64), g.astype(np.float64), b.astype(np.float64))
        A = bf16_round(ln.astype(np.float32)).astype(np.float64)
        # the kernel rounds its fp32 LayerNorm to bf16: where that lies within fp32 noise of a rounding boundary an element
        # may take the neighbouring bf16 value - one ulp of the largest element times the largest weight
        flip = BF16_ULP * np.abs(A).max() * np.abs(W).max()
        stats = torch.full((32 + GUARD, 2), float("nan"), device="cuda")
        kw.update(a_f32=_f32(x), ln_g=_f32(g), ln_b=_f32(b), stats_out=stats)
    acc = A @ W.astype(np.float64).T
    scale = (np.abs(A) @ np.abs(W).astype(np.float64).T).max(-1, keepdims=True)
    extra = flip
    if epi == 0:
        ref = acc
    elif epi == 1:
        r = rs.standard_normal((rows, N)).astype(np.float32) * 2 + 1
        kw["resid"] = _f32(r)
        if rform == "stats":
            rg = (1 + 0.3 * rs.standard_normal(N)).astype(np.float32)
            rb = (0.2 * rs.standard_normal(N)).astype(np.float32)
            _, m, sd = _ln64(r.astype(np.float64), 0, 0)
            st = np.stack([m, 1 / sd], -1).astype(np.float32)              # distinct (mean, rstd) per row
            kw.update(resid_stats=_f32(st), resid_g=_f32(rg), resid_b=_f32(rb))
            rr = (r - st[:, :1].astype(np.float64)) * st[:, 1:].astype(np.float64) * rg + rb
        else:
            rr = r.astype(np.float64)
        ref = acc + bias + rr
        scale = scale + np.abs(rr).max(-1, keepdims=True)
    else:
        ref = _gelu(acc + bias)
        extra = flip + 3e-5                                               # gelu_fast's bound against the erf form
    out_dtype = "bf16" if epi == 2 else "fp32"
    out = _nan((32 + GUARD, ldo), out_dtype)
    kw["out"] = out
    torch.cuda.synchronize()
    eng.op_smallm_gemm(**kw)
    got = _np(out)
    assert np.isnan(got[rows:]).all(), "rows >= rows written"
    assert np.isnan(got[:rows, N:]).all(), "columns >= N written"
    ratio, rel = _check_bf16_or_f32(got[:rows, :N], ref, scale, out_dtype, f"smallm {which} rows={rows}", extra)
    if pro == 1:
        gs = _np(stats)
        assert np.isnan(gs[rows:]).all(), "stats of rows >= rows written"
        np.testing.assert_allclose(gs[:rows, 0], mean, rtol=0, atol=1e-6 * np.abs(x).max())
        np.testing.assert_allclose(gs[:rows, 1], 1 / std, rtol=1e-5)
    report(f"smallm {which} rows={rows} ldo={ldo}: max err {rel:.2e} of the row scale ({ratio:.2f} of tol)")
