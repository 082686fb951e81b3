"""-m gpu: the encoder's front end, its LayerNorms and its attention against float64 statements of the same op, and the
encoder of a few crops against the oracle in every kernel regime it has.

The kernels are called through the C ABI's operator hooks (mocr_op_embed / _layernorm_slab / _layernorm / _enc_attention),
which launch through the helpers the encoder itself launches through; mocr_encoder_plan (Engine.encoder_plan) says what the
encoder decides from the number of crops - the tile of the patch embedding, the split of O-proj / FC2 over K, the blocks
per head of the attention - so that a test can see which regime it ran.

The references apply the kernels' own rounding points (bf16 operands, one rounding of an output, the attention's
probabilities rounded to bf16 in front of P.V); the tolerances follow from those alone.  Where the inputs lie on a grid
that makes every fp32 sum exact, the result is compared bit for bit.  Every output sits in front of NaN guard rows that
must stay NaN."""
import numpy as np
import pytest

from gpu_util import BF16_ULP, _check_bf16_or_f32, _grid_vals, _ln64, _nan, _store, bf16_round, crops, engine, oracle, report, weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

D, H, DH, S, NP, P, IMG = 768, 12, 64, 197, 196, 16, 224
GUARD = 2                           # guard rows behind every output
U32 = 2.0 ** -24                    # unit roundoff of fp32


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _t(a, dtype):
    """operand of the engine's storage type"""
    t = _f32(a)
    return t.to(torch.bfloat16) if dtype == "bf16" else t


def _np(t):
    return t.float().cpu().numpy().astype(np.float64)


def _plan_str(pl):
    return (f"embed tile {pl['embed_tile']}, tiles {pl['tile_qkv']}/{pl['tile_o']}/{pl['tile_fc1']}/{pl['tile_fc2']}, "
            f"split (O-proj, FC2) ({pl['split_o']}, {pl['split_2']}), fold {pl['fold']}, attention impl {pl['attn_impl']} ysplit {pl['ysplit']}")


# ------------------------------------------------------------------------------------------------ patch embedding
def _planes(n):
    """n = 1: random bytes; 2: random, a ramp that holds every value 0 .. 255; 3: the ramp, all 0, all 255; more: random bytes
    with the ramp, an all-0 and an all-255 plane among them (the all-255 one last)"""
    gray = crops(77 + n, n)
    yy, xx = np.mgrid[0:IMG, 0:IMG]
    ramp = ((xx + 7 * yy) % 256).astype(np.uint8)
    assert len(np.unique(ramp)) == 256
    if n == 2:
        gray[1] = ramp
    elif n == 3:
        gray[0], gray[1], gray[2] = ramp, 0, 255
    elif n > 3:
        gray[n // 4], gray[n // 2], gray[n - 1] = ramp, 0, 255
    return gray


def _lut():
    """(float32(float64(u) / 255) - 0.5f) / 0.5f in float32, as the engine and the reference's image processor compute it"""
    x = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    return ((x - np.float32(0.5)) / np.float32(0.5)).astype(np.float32)


def _embed_weights(dtype):
    w = weights()
    e = "encoder.embeddings."
    wpe = w[e + "patch_embeddings.projection.weight"].astype(np.float64).sum(1).reshape(D, P * P).astype(np.float32)    # [768][ky*16 + kx]
    return dict(wpe=_store(wpe, dtype), bpe=w[e + "patch_embeddings.projection.bias"].astype(np.float64),
                cls=w[e + "cls_token"].reshape(D).astype(np.float32), pos=w[e + "position_embeddings"].reshape(S, D).astype(np.float32))


EMBED_CASES = [(n, tile, 8) for n in (1, 2, 3) for tile in (64, 128)] + [(23, 0, 32)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("n,tile,max_batch", EMBED_CASES)
def test_patch_embedding_against_float64(dtype, n, tile, max_batch):
    """patchify_kernel, cls_rows_kernel and gemm_kernel's EPI_PATCH epilogue as the encoder launches them.  196 patches per crop:
    64-row tiles end in a 4-row tile, 128-row tiles in a 68-row one, and from two crops on tiles straddle crops (the
    epilogue's b = m / 196); 23 crops on a max_batch = 32 engine are where the encoder itself moves to the 128-row tile.
    The patch matrix and the CLS rows are exact; a patch row is within test_gemm_epilogues' bound for fp32 outputs of the
    float64 product of the operands the kernel was given."""
    eng = engine(dtype) if max_batch == 8 else engine(dtype, max_batch=max_batch)
    if tile == 0:
        assert eng.encoder_plan(23)["embed_tile"] == 128 and eng.encoder_plan(3)["embed_tile"] == 64
    gray = _planes(n)
    ew = _embed_weights(dtype)
    A = _store(_lut()[gray].reshape(n, IMG // P, P, IMG // P, P).transpose(0, 1, 3, 2, 4).reshape(n * NP, P * P), dtype)
    rows_a = (n * NP + 127) // 128 * 128
    d_patches = _nan((rows_a, P * P), dtype)
    d_x = _nan((n * S + GUARD, D), "fp32")
    d_gray = torch.from_numpy(gray).cuda()
    torch.cuda.synchronize()
    eng.op_embed(d_gray, n, tile, d_patches, d_x)
    got_a, got_x = _np(d_patches), _np(d_x)
    assert np.isnan(got_a[n * NP:]).all(), "patch rows behind n * 196 were written"
    np.testing.assert_array_equal(got_a[:n * NP], A, err_msg="patch matrix != storage rounding of lut[gray] in [b*196 + py*14 + px][ky*16 + kx] layout")
    assert np.isnan(got_x[n * S:]).all(), "rows behind n * 197 were written"
    x = got_x[:n * S].reshape(n, S, D)
    want_cls = (ew["cls"] + ew["pos"][0]).astype(np.float32).astype(np.float64)
    np.testing.assert_array_equal(x[:, 0], np.broadcast_to(want_cls, (n, D)), err_msg="CLS row != float32(cls + pos[0])")
    ref = (A @ ew["wpe"].T + ew["bpe"]).reshape(n, NP, D) + ew["pos"][1:].astype(np.float64)
    assert np.isfinite(x).all()
    err = np.abs(x[:, 1:] - ref).max() / np.abs(ref).max()
    tol = 2e-6 * np.sqrt(P * P) if dtype == "fp32" else 1e-5
    report(f"patch embedding {dtype} n={n} tile={tile} (max_batch {max_batch}): patches and CLS rows exact, max rel err {err:.3e} ({err / tol:.2f} of tol {tol:.1e})")
    assert err <= tol


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_patch_embedding_refusals(dtype):
    """a tile code the front end does not have, and more crops than the engine was built for: refused, nothing written"""
    from manga_ocr._capi import MocrError
    eng = engine(dtype)
    n = 9                                                                 # max_batch is 8
    d_gray = torch.zeros((n, IMG, IMG), dtype=torch.uint8, device="cuda")
    d_patches = _nan(((n * NP + 127) // 128 * 128, P * P), dtype)
    d_x = _nan((n * S + GUARD, D), "fp32")
    torch.cuda.synchronize()
    with pytest.raises(MocrError, match="tile must be"):
        eng.op_embed(d_gray, 2, 256, d_patches, d_x)
    with pytest.raises(MocrError, match="max_batch"):
        eng.op_embed(d_gray, n, 64, d_patches, d_x)
    with pytest.raises(MocrError, match="max_batch"):
        eng.encoder_plan(n)
    torch.cuda.synchronize()
    assert torch.isnan(d_patches).all() and torch.isnan(d_x).all(), "a refused call wrote its outputs"


# ------------------------------------------------------------------------------------------------ slab sum + LayerNorm
def _run_ln_slab(eng, dtype, x, slabs, bias, g, b):
    """x [M, D], slabs [nslab, M, D] -> (x after the call, out); the slabs lie M * D + 3 * D floats apart, NaN between them"""
    nslab, M = slabs.shape[0], slabs.shape[1]
    stride = M * D + 3 * D
    d_slabs = torch.full((nslab * stride,), float("nan"), device="cuda", dtype=torch.float32)
    for k in range(nslab):
        d_slabs[k * stride:k * stride + M * D] = _f32(slabs[k]).reshape(-1)
    d_x = _nan((M + GUARD, D), "fp32")
    d_x[:M] = _f32(x)
    d_out = _nan((M + GUARD, D), dtype)
    torch.cuda.synchronize()
    eng.op_layernorm_slab(d_x, d_slabs, nslab, stride, _f32(bias), _f32(g), _f32(b), d_out, M)
    gx, go = _np(d_x), _np(d_out)
    assert np.isnan(gx[M:]).all() and np.isnan(go[M:]).all(), "guard rows written"
    return gx[:M], go[:M]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("M", [1, 6, 197, 591])
@pytest.mark.parametrize("nslab", [1, 2, 3, 4, 8])
def test_layernorm_slab_against_float64(dtype, nslab, M):
    """layernorm_slab_kernel, what finishes an encoder GEMM split over K: every slab count the encoder's plans have, all four
    values of M mod 4 (a last block with one to three idle waves).  x, the slabs and the bias lie on the 2^-10 grid and their
    sum stays below 2^7, so it is exact in fp32 in any order: x after the call equals the float64 sum bit for bit."""
    eng = engine(dtype)
    rs = np.random.RandomState(1000 * nslab + M)
    x = _grid_vals(rs, (M, D), 1.0)
    slabs = _grid_vals(rs, (nslab, M, D), 1.5 / np.sqrt(nslab))
    bias = _grid_vals(rs, D, 0.5)
    g = (1 + 0.3 * rs.standard_normal(D)).astype(np.float32)
    b = (0.2 * rs.standard_normal(D)).astype(np.float32)
    v = x.astype(np.float64) + slabs.astype(np.float64).sum(0) + bias
    assert np.abs(v).max() < 2.0 ** 7
    ref, _, _ = _ln64(v, g.astype(np.float64), b.astype(np.float64))
    gx, go = _run_ln_slab(eng, dtype, x, slabs, bias, g, b)
    np.testing.assert_array_equal(gx, v, err_msg="x after the call != x + bias + the slabs")
    scale = np.abs(ref).max(-1, keepdims=True)
    ratio, rel = _check_bf16_or_f32(go, ref, scale, dtype, f"layernorm_slab {dtype} nslab={nslab} M={M}")
    report(f"layernorm_slab {dtype} nslab={nslab} M={M}: x exact, out max err {rel:.2e} of the row scale ({ratio:.2f} of tol)")


def _hostile_rows(rs, M):
    """a DC offset of ~50 under a spread of ~1e-2 and one outlier channel on every other row (test_add_layernorm_hostile_rows)"""
    x = (50.0 + rs.standard_normal((M, D)) * 1e-2 * rs.uniform(0.5, 2, (M, 1))).astype(np.float32)
    x[1::2, 17] += 0.5
    return x


def _conditioning(mean, std, g):
    """the fp32 row sum carries rounding errors of ~log2(768) u |mean| per element: in units of the row's std ~ 16 u |mean| / std,
    times |gamma| in the output (test_add_layernorm_hostile_rows)"""
    cond = (np.abs(mean) / std)[:, None]
    return 16 * U32 * cond * np.abs(g).max(), cond


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_layernorm_slab_hostile_rows(dtype):
    eng = engine(dtype)
    rs = np.random.RandomState(5)
    M, nslab = 8, 3
    slabs = (rs.standard_normal((nslab, M, D)) * 1e-2 / np.sqrt(nslab)).astype(np.float32)
    bias = (rs.standard_normal(D) * 1e-3).astype(np.float32)
    x = _hostile_rows(rs, M)
    g = (1 + 0.3 * rs.standard_normal(D)).astype(np.float32)
    b = (0.2 * rs.standard_normal(D)).astype(np.float32)
    v = x.astype(np.float64) + slabs.astype(np.float64).sum(0) + bias
    ref, mean, std = _ln64(v, g.astype(np.float64), b.astype(np.float64))
    gx, go = _run_ln_slab(eng, dtype, x, slabs, bias, g, b)
    # x: nslab + 1 fp32 additions, each off by up to u of a partial sum no larger than max |v| (+ the others' roundings)
    assert np.abs(gx - v).max() <= (nslab + 1) * U32 * np.abs(v).max() * 1.01
    extra, cond = _conditioning(mean, std, g)
    scale = np.abs(ref).max(-1, keepdims=True)
    ratio, rel = _check_bf16_or_f32(go, ref, scale, dtype, f"layernorm_slab hostile {dtype}", extra)
    report(f"layernorm_slab hostile {dtype}: |mean|/std up to {cond.max():.0f}, max err {rel:.2e} of the row scale "
           f"({ratio:.2f} of the conditioning bound {float((extra / scale).max()):.1e} + 1e-5)")


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("rows", ["benign", "hostile"])
@pytest.mark.parametrize("M", [1, 2, 3, 5, 403])
def test_layernorm_against_float64(dtype, rows, M):
    """layernorm_kernel (the encoder's output, and every LayerNorm of the unfolded regimes), one wave per row: one row, a last
    block with one to three idle waves, many blocks.  Benign rows (offset 0.7, spread 3) and the hostile rows."""
    eng = engine(dtype)
    rs = np.random.RandomState(31 + M)
    x = _hostile_rows(rs, M) if rows == "hostile" else (rs.standard_normal((M, D)) * 3 + 0.7).astype(np.float32)
    g = (1 + 0.3 * rs.standard_normal(D)).astype(np.float32)
    b = (0.2 * rs.standard_normal(D)).astype(np.float32)
    ref, mean, std = _ln64(x.astype(np.float64), g.astype(np.float64), b.astype(np.float64))
    d_out = _nan((M + GUARD, D), dtype)
    torch.cuda.synchronize()
    eng.op_layernorm(_f32(x), _f32(g), _f32(b), d_out, M)
    got = _np(d_out)
    assert np.isnan(got[M:]).all(), "guard rows written"
    extra, cond = _conditioning(mean, std, g)
    if rows == "benign":
        extra = 0.0
    scale = np.abs(ref).max(-1, keepdims=True)
    ratio, rel = _check_bf16_or_f32(got[:M], ref, scale, dtype, f"layernorm {dtype} {rows} M={M}", extra)
    report(f"layernorm {dtype} {rows} M={M}: |mean|/std up to {cond.max():.1f}, max err {rel:.2e} of the row scale ({ratio:.2f} of tol)")


# ------------------------------------------------------------------------------------------------ encoder attention
ATTN_BF16_N = (10, 11, 21, 22)      # the MFMA kernel's four, two (twice) and one block per (crop, head) on 256 CUs
ATTN_CASES = [("bf16", 1, n) for n in ATTN_BF16_N] + [("fp32", 1, 11), ("fp32", 0, 11), ("bf16", 0, 11)]


def _attn_inputs(rs, n, dtype, onehot):
    """qkv [n * S, 3 * H * DH] float32, storable in `dtype` without rounding.

    benign: N(0, 1.5^2) everywhere, the scores' std is ~2 (test_encoder_attention's inputs).
    onehot: a softmax near one-hot behind a large common offset.  q ~ N(0, 8^2) on a 2^-2 grid and k ~ N(0, 1.5^2) on a 2^-3
    grid: the scores q.k / 8 have a std of ~12.  Dim 0 of every head is special: q is 8 there and k is 256 + an even integer,
    i.e. every key is shifted by the vector (256, 0, ...), which moves all scores of a query by 8 * 256 / 8 = 256 and leaves
    the softmax alone - if the kernel subtracts the row maximum.  All values have at most 8 significant bits (bf16 holds
    them) and every product and partial sum is a multiple of 2^-5 below 2^14, so the scores are exact in fp32 in any order:
    what is left are the rounding points of the softmax and of P.V, which the bound names."""
    qkv = (rs.standard_normal((n * S, 3, H, DH)) * 1.5).astype(np.float32)
    if onehot:
        qkv[:, 0] = (np.round(rs.standard_normal((n * S, H, DH)) * 8 * 4) / 4).clip(-31.75, 31.75)
        qkv[:, 1] = (np.round(qkv[:, 1] * 8) / 8).clip(-6, 6)
        qkv[:, 0, :, 0] = 8.0
        qkv[:, 1, :, 0] = 256.0 + 2 * np.round(rs.standard_normal((n * S, H)) * 1.5).clip(-6, 6)
    qkv = qkv.reshape(n * S, 3 * H * DH)
    if dtype == "bf16":
        r = bf16_round(qkv)
        if onehot:
            assert np.array_equal(r[:, :2 * H * DH], qkv[:, :2 * H * DH]), "q / k of the one-hot set must be bf16 values"
        qkv = r
    return qkv


@pytest.mark.parametrize("onehot", [False, True])
@pytest.mark.parametrize("dtype,impl,n", ATTN_CASES)
def test_encoder_attention_against_float64(dtype, impl, n, onehot):
    """The encoder attention kernels elementwise against float64, with the plan's word on how many blocks share a head:
    enc_attn2_kernel (bf16, impl 1) at both ends of each of its three splits, the fp32 MFMA kernel and the VALU kernel of
    both engines at a two-blocks-per-head count.  NaN rows behind qkv (no kernel may read them) and behind ctx.

    Bound, vmax = the largest |v| of the (crop, head): 1e-5 vmax for the fp32 sums (test_encoder_attention's); bf16 adds
    2^-8 |ref| for the output's rounding and 2^-8 vmax for the probabilities rounded to bf16 in front of P.V (each off by
    <= 2^-9 relative, sum of p |v| <= vmax, doubled because the normaliser sums the unrounded ones)."""
    eng = engine(dtype, max_batch=32)
    pl = eng.encoder_plan(n)
    rs = np.random.RandomState(100 * n + 10 * impl + onehot)
    qkv = _attn_inputs(rs, n, dtype, onehot)
    t = torch.from_numpy(qkv).view(n, S, 3, H, DH).permute(2, 0, 3, 1, 4).double()
    s = torch.matmul(t[0], t[1].transpose(-1, -2)) * 0.125
    prob = torch.softmax(s, dim=-1)
    ref = torch.matmul(prob, t[2]).permute(0, 2, 1, 3).reshape(n * S, H * DH).numpy()
    vmax = t[2].abs().amax(dim=(-1, -2))                                         # [n, H]
    vmax = vmax[:, None, :, None].expand(n, S, H, DH).reshape(n * S, H * DH).numpy()
    d_q = torch.cat([_t(qkv, dtype), _nan((256, 3 * H * DH), dtype)]).contiguous()
    d_c = _nan((n * S + GUARD, H * DH), dtype)
    torch.cuda.synchronize()
    eng.op_enc_attention(d_q, d_c, n, impl)
    got = _np(d_c)
    assert np.isnan(got[n * S:]).all(), "rows behind n * 197 were written"
    got = got[:n * S]
    tol = 1e-5 * vmax + ((BF16_ULP * np.abs(ref) + BF16_ULP * vmax) if dtype == "bf16" else 0.0)
    err = np.abs(got - ref)
    finite = np.isfinite(got).all()
    ratio = float((err / tol).max()) if finite else float("inf")
    ysplit = pl["ysplit"] if (dtype == "bf16" and impl == 1) else 1
    report(f"enc attention {dtype} impl{impl} n={n} {'one-hot + offset 256' if onehot else 'benign'}: blocks per head {ysplit}, "
           f"scores std {float(s.std()):.1f} max {float(s.max()):.0f}, mean top probability {float(prob.amax(-1).mean()):.2f}, "
           f"max err {float(err.max()) if finite else float('nan'):.3e} ({ratio:.2f} of the bound)")
    assert finite, "non-finite output"
    bad = np.argwhere(err > tol)
    assert bad.size == 0, f"{len(bad)} elements out of tolerance, first at {tuple(bad[0])}: got {got[tuple(bad[0])]} want {ref[tuple(bad[0])]}"


def test_encoder_attention_cases_cover_every_split():
    """the bf16 cases above ran four, two and one block per (crop, head): the launcher's rule on 256 CUs puts the steps between
    10 and 11 and between 21 and 22 crops"""
    eng = engine("bf16", max_batch=32)
    ys = [eng.encoder_plan(n)["ysplit"] for n in ATTN_BF16_N]
    report(f"enc attention blocks per head at n = {ATTN_BF16_N}: {ys}")
    assert set(ys) == {4, 2, 1}
    assert eng.encoder_plan(11)["attn_impl"] == 1 and engine("fp32", max_batch=32).encoder_plan(11)["ysplit"] == 1


# ------------------------------------------------------------------------------------------------ encoder per regime
REGIME_CASES = [(8, n) for n in (1, 2, 3, 5, 7)] + [(160, n) for n in (5, 6)]


@pytest.fixture(scope="module")
def ref7():
    """the oracle's encodings of seven crops: a crop's reference does not depend on its batch"""
    o = oracle()
    gray = crops(1234, 7)
    return dict(gray=gray, enc=o.encode(o.preprocess_gray(gray)).numpy())


def _regime_engine(dtype, max_batch):
    return engine(dtype) if max_batch == 8 else engine(dtype, max_batch=max_batch)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("max_batch,n", REGIME_CASES)
def test_encoder_of_a_few_crops_matches_oracle_in_every_regime(ref7, dtype, max_batch, n):
    """The encoder splits O-proj / FC2 over K by the number of crops AND by the slab buffer max_batch gives it, so the slab
    count its LayerNorms add up and the summation order of a crop's encoding change with both: every (O-proj, FC2) split the
    plans have - the single crop's (3, 8) among them - against the oracle, within the bounds of
    test_fp32_encoder_matches_oracle_and_golden (2e-4 max abs) and test_bf16_encoder_close_to_oracle (0.25 max, 0.02 mean)."""
    eng = _regime_engine(dtype, max_batch)
    pl = eng.encoder_plan(n)
    d_gray = torch.from_numpy(ref7["gray"][:n]).cuda()
    torch.cuda.synchronize()
    got = eng.encode(d_gray, n)
    d = np.abs(got - ref7["enc"][:n])
    assert np.isfinite(got).all()
    if dtype == "fp32":
        report(f"encoder fp32 n={n} max_batch={max_batch} [{_plan_str(pl)}] vs oracle: max abs err {d.max():.3e} ({d.max() / 2e-4:.2f} of 2e-4)")
        assert d.max() <= 2e-4
    else:
        report(f"encoder bf16 n={n} max_batch={max_batch} [{_plan_str(pl)}] vs oracle: max abs err {d.max():.3e} ({d.max() / 0.25:.2f} of 0.25), "
               f"mean abs err {d.mean():.3e} ({d.mean() / 0.02:.2f} of 0.02)")
        assert d.max() <= 0.25 and d.mean() <= 0.02


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_encoder_regime_cases_cover_every_split(dtype):
    """the plans of the cases above, as the hook reports them: O-proj split 1 and 3 ways, FC2 split 1, 2, 4 and 8 ways"""
    plans = {(mb, n): _regime_engine(dtype, mb).encoder_plan(n) for mb, n in REGIME_CASES}
    splits = {k: (p["split_o"], p["split_2"]) for k, p in plans.items()}
    report(f"encoder plans {dtype}, (max_batch, n) -> (split O-proj, split FC2): {splits}")
    assert {s[0] for s in splits.values()} == {1, 3}
    assert {s[1] for s in splits.values()} == {1, 2, 4, 8}
    assert all(p["embed_tile"] == 64 and p["fold"] == 0 for p in plans.values())
