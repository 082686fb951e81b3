"""-m gpu: what a decode step decides from its row count, and every form of its tile GEMMs against float64.

mocr_decode_plan (Engine.decode_plan) reports the step's choices - path, regime and launch tile, and for each of the five
GEMMs the split over K, the ring depth and the epilogue - from the helpers the step launches through.  (a) pins the plan to a
table derived by hand from the rules, (b) collects the distinct (N, K, tile, split, ring, epilogue) launches of those plans
and runs each once, at the smallest row count that produces it, through mocr_op_gemm_args - the same launch, so the ring is
the product's, which mocr_last_tile_launch confirms - against float64, slab by slab, (c) walks the tile order in column
groups and (d) compares the pairs of forms the code calls bit-identical.

Operands: A ~ N(0, 1) and W ~ 0.05 N(0, 1) rounded to the engine's storage type, fp32 bias.  A holds round_up(M, tile) rows,
the ones behind M NaN (the kernel stages them; they may reach no output).  Outputs are pre-filled with NaN and end in GUARD
rows that must stay NaN; slabs lie (M + GUARD) * ldo floats apart, so every slab has its guard rows and the stride is not
the dense one.

Bound, elementwise: |err| <= u |ref| + 2^-16 S1, S1 = |A| |W|^T (+ |bias|) over the K slice, u = 2^-8 for bf16 outputs and 0
for fp32 ones (test_gpu_latent_block.py's bound for fp32 accumulation).  Fused GELU: 1.13 (GELU's largest slope) x the
pre-activation bound, + 1e-5 of the row's largest |ref| (+ 3e-5 for bf16 outputs) for the device's erf, as
test_bias_gelu_against_float64 allows.  The K 2^-24 S1 widening the worst-case analysis would permit at K = 3072 is not used."""
import functools

import numpy as np
import pytest

from gpu_util import ACC, _nan, _store, engine, report
from gpu_util import check_elementwise as _check, gemm_bound as _bound      # the bound stated above

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPI_SLAB, EPI_BIAS, EPI_BIAS_GELU, EPI_ARGMAX = 0, 1, 2, 6
D, F, V = 768, 3072, 6144
GEMMS = {"qkv": (3 * D, D), "proj": (D, D), "fc1": (F, D), "fc2": (D, F), "vocab": (V, D)}
GUARD = 3
DTYPES = ["fp32", "bf16"]

ROWS = (8, 72, 136, 256, 288, 512, 960, 1024, 1216, 1280, 2304, 2560)
PAIRS = ((2560, 768), (2560, 256), (1024, 512))                       # (regime, rows) of a compacted batch
CASES = tuple((r, r) for r in ROWS) + PAIRS

# (regime, rows) -> launch tile, then (split, ring slots) of QKV, projection, FC1, FC2, vocabulary, on 256 compute units.
# Worked by hand from the rules: tile 128 from 1024 rows; the split doubles while (N-tiles x M-tiles of the REGIME's tile) x
# split stays below the block target (100 up to 128 regime rows, 150 up to 2047, 200 above), the K-tiles (K / 64 for bf16, K /
# 32 for fp32) divide and split x N <= 12288, then triples if that still leaves a third of the target free; four ring slots iff
# rows < 1280, >= 4 K-tiles per slice and (N-tiles x M-tiles of the LAUNCH tile) x split <= compute units.
TABLE = {
    "bf16": {
        (8, 8): (64, (4, 2), (12, 2), (4, 2), (16, 2), (2, 4)),
        (72, 72): (64, (2, 4), (4, 2), (2, 4), (8, 4), (1, 4)),
        (136, 136): (64, (2, 4), (4, 2), (2, 2), (8, 2), (1, 2)),
        (256, 256): (64, (2, 2), (4, 2), (1, 4), (4, 4), (1, 2)),
        (288, 288): (64, (1, 4), (4, 2), (1, 4), (4, 4), (1, 2)),
        (512, 512): (64, (1, 2), (2, 4), (1, 2), (2, 4), (1, 2)),
        (960, 960): (64, (1, 2), (1, 4), (1, 2), (1, 4), (1, 2)),
        (1024, 1024): (128, (2, 2), (4, 2), (1, 4), (4, 4), (1, 2)),
        (1216, 1216): (128, (1, 4), (4, 2), (1, 4), (4, 4), (1, 2)),
        (1280, 1280): (128, (1, 2), (4, 2), (1, 2), (4, 2), (1, 2)),
        (2304, 2304): (128, (1, 2), (2, 2), (1, 2), (2, 2), (1, 2)),
        (2560, 2560): (128, (1, 2), (2, 2), (1, 2), (2, 2), (1, 2)),
        (2560, 768): (64, (1, 2), (2, 2), (1, 2), (2, 2), (1, 2)),
        (2560, 256): (64, (1, 4), (2, 4), (1, 4), (2, 4), (1, 2)),
        (1024, 512): (64, (2, 2), (4, 2), (1, 2), (4, 2), (1, 2)),
    },
    # fp32 walks twice the K-tiles: the projections of 8 .. 136 rows split 8 ways (24 K-tiles divide by 8, 12 do not) and the
    # four-way split projections keep 6 K-tiles per slice, enough for the four-slot ring
    "fp32": {
        (8, 8): (64, (4, 4), (8, 2), (4, 4), (16, 4), (2, 4)),
        (72, 72): (64, (2, 4), (8, 2), (2, 4), (8, 4), (1, 4)),
        (136, 136): (64, (2, 4), (8, 2), (2, 2), (8, 2), (1, 2)),
        (256, 256): (64, (2, 2), (4, 4), (1, 4), (4, 4), (1, 2)),
        (288, 288): (64, (1, 4), (4, 4), (1, 4), (4, 4), (1, 2)),
        (512, 512): (64, (1, 2), (2, 4), (1, 2), (2, 4), (1, 2)),
        (960, 960): (64, (1, 2), (1, 4), (1, 2), (1, 4), (1, 2)),
        (1024, 1024): (128, (2, 2), (4, 4), (1, 4), (4, 4), (1, 2)),
        (1216, 1216): (128, (1, 4), (4, 4), (1, 4), (4, 4), (1, 2)),
        (1280, 1280): (128, (1, 2), (4, 2), (1, 2), (4, 2), (1, 2)),
        (2304, 2304): (128, (1, 2), (2, 2), (1, 2), (2, 2), (1, 2)),
        (2560, 2560): (128, (1, 2), (2, 2), (1, 2), (2, 2), (1, 2)),
        (2560, 768): (64, (1, 2), (2, 2), (1, 2), (2, 2), (1, 2)),
        (2560, 256): (64, (1, 4), (2, 4), (1, 4), (2, 4), (1, 2)),
        (1024, 512): (64, (2, 2), (4, 2), (1, 2), (4, 2), (1, 2)),
    },
}


def _cus():
    """the engine's compute units: the device's, rounded down to a multiple of 8"""
    return max(torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8, 8)


def _ring_rule(dtype, rows, N, K, tile, split, cus):
    """four slots iff rows < 1280, at least 4 K-tiles (128 bytes of a row) per slice and at most one block per compute unit"""
    ktiles = K // split // (64 if dtype == "bf16" else 32)
    blocks = -(-rows // tile) * (N // tile) * split
    return 4 if rows < 1280 and ktiles >= 4 and blocks <= cus else 2


def _round_up(n, q):
    return -(-n // q) * q


# ------------------------------------------------------------------------------------------------ (a) the plan table
@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_plan_equals_the_table(dtype):
    """split, ring and tile of every GEMM at the graph grid's row counts and after a compaction; fused GELU iff FC1 is not
    split, fused LM head iff the vocabulary GEMM is not.  On a device that does not report 256 compute units the ring column
    is recomputed from the stated rule."""
    eng = engine(dtype)
    cus = _cus()
    for regime, rows in CASES:
        pl = eng.decode_plan(rows, 0 if regime == rows else regime)
        want = TABLE[dtype][(regime, rows)]
        tile = want[0]
        assert (pl["regime_tile"], pl["launch_tile"]) == (128 if regime >= 1024 else 64, tile), (regime, rows, pl)
        for (g, (N, K)), (split, ring) in zip(GEMMS.items(), want[1:]):
            if cus != 256:
                ring = _ring_rule(dtype, rows, N, K, tile, split, cus)
            assert (pl[g + "_split"], pl[g + "_ring"]) == (split, ring), f"{dtype} regime {regime} rows {rows} {g}: plan {pl[g + '_split']}/{pl[g + '_ring']}, table {split}/{ring}"
            epi = EPI_BIAS_GELU if (g == "fc1" and split == 1) else EPI_ARGMAX if (g == "vocab" and split == 1) else EPI_SLAB
            assert pl[g + "_epi"] == epi, (regime, rows, g, pl)
        report(f"decode plan {dtype} regime {regime} rows {rows} ({cus} CUs): tile {pl['regime_tile']}/{pl['launch_tile']}, split/ring " +
               " ".join(f"{g} {pl[g + '_split']}/{pl[g + '_ring']}" for g in GEMMS))
    # The graph grid between 1280 and 2560 rows, (projection, FC2): 6 N-tiles x rows / 128 M-tiles against a target of 150
    # blocks below 2048 rows and 200 from there - 60 and 72 tiles double twice, 84 (x 2 = 168) once, 96 (x 2 = 192 < 200) twice,
    # 108 and 120 once.  So two slabs are reached at 1792 rows, left again at 2048 and kept from 2304.
    splits = {r: (eng.decode_plan(r)["proj_split"], eng.decode_plan(r)["fc2_split"]) for r in (1280, 1536, 1792, 2048, 2304, 2560)}
    report(f"decode plan {dtype}: (projection, FC2) split over the graph grid: {splits}")
    assert splits == {1280: (4, 4), 1536: (4, 4), 1792: (2, 2), 2048: (4, 4), 2304: (2, 2), 2560: (2, 2)}


def _check_path_fields(eng, dtype, classic_rows, max_batch, latent, smallm):
    for regime, rows in CASES + ((16, 16), (32, 32), (33, 33), (128, 128), (257, 257), (1281, 1281), (300, 120)):
        pl = eng.decode_plan(rows, 0 if regime == rows else regime)
        is_latent = latent and regime > classic_rows
        is_small = smallm and dtype == "bf16" and regime <= 32 and not is_latent
        assert pl["path"] == ("latent" if is_latent else "small-batch" if is_small else "classic"), (regime, rows, pl)
        assert pl["qkv_tile_gemm"] == int(pl["path"] == "classic")
        fused = is_latent and regime >= 257
        assert pl["fused_query"] == int(fused), (regime, rows, pl)
        assert pl["query_block_rows"] == ((64 if rows <= 1280 else 128) if fused else 0), (regime, rows, pl)
        assert pl["qt_tile"] == ((128 if regime >= 1024 else 64) if is_latent and not fused else 0), (regime, rows, pl)
        assert pl["attn_nt"] == int(not is_latent and regime >= 128), (regime, rows, pl)
        assert pl["chunk_steps"] == (2 if rows <= 16 else 4 if rows <= 128 else 8), (rows, pl)
        q = 1 if rows <= 8 else 8 if rows <= 64 else 32 if rows <= 256 else 64 if rows <= 1024 else 256
        assert pl["graph_rows"] == min(_round_up(rows, q), max_batch), (rows, pl)


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_plan_path_fields(dtype):
    """the rules in the code's own words: latent iff the regime is above the engine's classic_rows (0 on the tests' bf16
    engines, which run the latent path at every size; fp32 engines have no latent path), small-batch iff bf16, <= 32 regime
    rows and not latent, the fused query kernel from 257 regime rows on 64-row blocks up to 1280 rows, chunks of 2 / 4 / 8 steps,
    the graph grid 1 / 8 / 32 / 64 / 256"""
    _check_path_fields(engine(dtype), dtype, 0, 8, dtype == "bf16", True)


def test_decode_plan_path_fields_of_the_product_engine():
    """a bf16 engine that chooses for itself: classic attention up to min(256, max_batch) rows, the small-batch path up to 32"""
    eng = engine("bf16", max_batch=512, auto_path=True)
    _check_path_fields(eng, "bf16", 256, 512, True, True)
    assert eng.decode_plan(256)["path"] == "classic" and eng.decode_plan(257)["path"] == "latent" and eng.decode_plan(32)["path"] == "small-batch"
    # a compacted latent batch stays latent and fused; its query blocks follow the rows it has left
    pl = eng.decode_plan(256, 2560)
    assert (pl["path"], pl["fused_query"], pl["query_block_rows"]) == ("latent", 1, 64)
    assert eng.decode_plan(2560)["query_block_rows"] == 128
    # the per-GEMM fields do not depend on max_batch
    small = engine("bf16")
    for regime, rows in CASES:
        a, b = eng.decode_plan(rows, regime), small.decode_plan(rows, regime)
        for g in GEMMS:
            for f in ("_split", "_ring", "_epi"):
                assert a[g + f] == b[g + f], (regime, rows, g, f)


def test_decode_plan_refusals():
    from manga_ocr._capi import MocrError
    eng = engine("fp32")
    for rows, regime in ((0, 0), (-1, 0), (8, -1)):
        with pytest.raises(MocrError, match="bad argument"):
            eng.decode_plan(rows, regime)


# ------------------------------------------------------------------------------------------------ operands and references
def _dev(a, dtype):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    return t.to(torch.bfloat16) if dtype == "bf16" else t


def _np(t):
    return t.float().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=4)
def _operands(dtype, M, N, K):
    """A [M, K], W [N, K] as the engine stores them (float64 values), bias [N]"""
    rs = np.random.RandomState((M * 7919 + N * 31 + K) % (2 ** 31))
    A = _store(rs.standard_normal((M, K)), dtype)
    W = _store(rs.standard_normal((N, K)) * 0.05, dtype)
    bias = rs.standard_normal(N).astype(np.float32).astype(np.float64)
    for a in (A, W, bias):
        a.setflags(write=False)
    return A, W, bias


@functools.lru_cache(maxsize=2)
def _reference(dtype, M, N, K, split):
    """per K slice: the float64 product [split, M, N] and S1 = |A| |W|^T over the slice"""
    A, W, _ = _operands(dtype, M, N, K)
    ks = K // split
    ref = np.empty((split, M, N))
    s1 = np.empty((split, M, N))
    for z in range(split):
        a, w = A[:, z * ks:(z + 1) * ks], W[:, z * ks:(z + 1) * ks]
        ref[z] = a @ w.T
        s1[z] = np.abs(a) @ np.abs(w).T
    ref.setflags(write=False)
    s1.setflags(write=False)
    return ref, s1


def _device_a(dtype, A, tile, lda):
    """A on the device: round_up(M, tile) rows of lda elements, NaN behind row M and behind column K"""
    M, K = A.shape
    d = _nan((_round_up(M, tile), lda), dtype)
    d[:M, :K] = _dev(A, dtype)
    return d


def _launch(eng, dtype, M, N, K, tile, split, epi, *, lda=0, ldo=0, group_n=0):
    """one launch through mocr_op_gemm_args on fresh NaN outputs; returns (got [split, M, N] float64, the launch's record)"""
    A, W, bias = _operands(dtype, M, N, K)
    lda_, ldo_ = lda or K, ldo or N
    dA, dW = _device_a(dtype, A, tile, lda_), _dev(W, dtype)
    dB = torch.from_numpy(bias.astype(np.float32)).cuda()
    out_dtype = "fp32" if epi == EPI_SLAB else dtype
    stride = (M + GUARD) * ldo_
    dO = _nan((split, M + GUARD, ldo_), out_dtype)
    torch.cuda.synchronize()
    eng.op_gemm_args(M=M, N=N, K=K, epilogue=epi, tile=tile, split_k=split, lda=lda, ldo=ldo, group_n=group_n,
                     slab_stride=stride if epi == EPI_SLAB else 0, A=dA, W=dW, bias=None if epi == EPI_SLAB else dB, out=dO, resid=None)
    rec = eng.last_tile_launch()
    got = _np(dO)
    assert np.isnan(got[:, M:]).all(), "guard rows written"
    assert np.isnan(got[:, :M, N:]).all(), "columns behind N written"
    return got[:, :M, :N], rec


def _forms(eng, dtype):
    """the distinct tile-GEMM launches of the plans of (a): (gemm, N, K, tile, split, ring, epi) -> (rows, regime), the smallest rows"""
    forms = {}
    for regime, rows in sorted(CASES, key=lambda c: c[1]):
        pl = eng.decode_plan(rows, 0 if regime == rows else regime)
        for g, (N, K) in GEMMS.items():
            key = (N, K, pl["launch_tile"], pl[g + "_split"], pl[g + "_ring"], pl[g + "_epi"])
            forms.setdefault(key, (g, rows, regime))
    return forms


def _form_cases(dtype):
    """the forms of TABLE (what the plan reports on 256 compute units), so that the cases can be collected without a device;
    test_forms_are_the_plans_forms holds the list against the plans"""
    forms = {}
    for (regime, rows), want in sorted(TABLE[dtype].items(), key=lambda c: c[0][1]):
        for (g, (N, K)), (split, ring) in zip(GEMMS.items(), want[1:]):
            epi = EPI_BIAS_GELU if (g == "fc1" and split == 1) else EPI_ARGMAX if (g == "vocab" and split == 1) else EPI_SLAB
            forms.setdefault((N, K, want[0], split, ring, epi), (g, rows, regime))
    return [(dtype, g, rows, regime) + key for key, (g, rows, regime) in forms.items()]


FORM_CASES = _form_cases("fp32") + _form_cases("bf16")


def _form_id(c):
    dtype, g, rows, regime, N, K, tile, split, ring, epi = c
    return f"{dtype}-{g}-rows{rows}-regime{regime}-tile{tile}-split{split}-ring{ring}-epi{epi}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_forms_are_the_plans_forms(dtype):
    """the cases of test_every_form_against_float64 are exactly the distinct launches of the plans this device reports"""
    eng = engine(dtype)
    want = {c[4:]: c[1:4] for c in FORM_CASES if c[0] == dtype}
    got = _forms(eng, dtype)
    if _cus() == 256:             # (the case list is the one of 256 compute units; elsewhere each case checks its own launch against the plan)
        assert got == want
    report(f"decode forms {dtype}: {len(got)} distinct (N, K, tile, split, ring, epilogue) launches over {len(CASES)} plans")


# ------------------------------------------------------------------------------------------------ (b) every form
@pytest.mark.parametrize("case", FORM_CASES, ids=_form_id)
def test_every_form_against_float64(case):
    dtype, g, rows, regime, N, K, tile, split, ring, epi = case
    eng = engine(dtype)
    M = rows
    pl = eng.decode_plan(rows, 0 if regime == rows else regime)
    what = f"decode form {dtype} {g} [{M} x {N} x {K}] tile {tile} split {split} ring {ring} epi {epi}"
    ref_pre, s1 = _reference(dtype, M, N, K, split)
    _, _, bias = _operands(dtype, M, N, K)
    if epi == EPI_ARGMAX:
        ratio, rec = _run_lm_head(eng, dtype, M, N, K, tile, ref_pre[0] + bias, s1[0] + np.abs(bias), what)
    else:
        got, rec = _launch(eng, dtype, M, N, K, tile, split, epi)
        ref, tol = _bound(dtype, epi, ref_pre, s1, bias)
        ratio = _check(got, ref, tol, what)
    # the hook launched what the product launches at these rows: the plan's word against the launch's own record
    assert (rec["tile"], rec["split"], rec["ring"]) == (pl["launch_tile"], pl[g + "_split"], pl[g + "_ring"]), (rec, pl)
    if _cus() == 256:
        assert (rec["tile"], rec["split"], rec["ring"]) == (tile, split, ring), rec
    report(f"{what}: launched tile {rec['tile']} ring {rec['ring']} on {rec['blocks']} blocks, max err / tol {ratio:.3f}")


def _run_lm_head(eng, dtype, M, N, K, tile, ref, s1, what):
    """the fused LM head (mocr_op_gemm_argmax; mocr_op_gemm_args refuses it as mocr_op_gemm does): per row and N-tile the winner's
    value within the bound of its own column, and no column of the tile above it by more than both bounds"""
    A, W, bias = _operands(dtype, M, N, K)
    dA, dW = _device_a(dtype, A, tile, K), _dev(W, dtype)
    dB = torch.from_numpy(bias.astype(np.float32)).cuda()
    ntn = N // tile
    d_val = _nan((M + GUARD, ntn), "fp32")
    d_idx = torch.full((M + GUARD, ntn), -7, device="cuda", dtype=torch.int32)
    torch.cuda.synchronize()
    eng.op_gemm_argmax(dA, dW, dB, d_val, d_idx, M, N, K, tile)
    rec = eng.last_tile_launch()
    val, idx = _np(d_val), d_idx.cpu().numpy().astype(np.int64)
    assert np.isnan(val[M:]).all() and (idx[M:] == -7).all(), "guard rows written"
    val, idx = val[:M], idx[:M]
    assert np.isfinite(val).all(), f"{what}: non-finite candidate"
    lo = np.arange(ntn) * tile
    assert ((idx >= lo) & (idx < lo + tile)).all(), f"{what}: a candidate column outside its tile"
    tol = ACC * s1
    rows = np.arange(M)[:, None]
    ratio = np.abs(val - ref[rows, idx]) / tol[rows, idx]
    assert ratio.max() <= 1.0, f"{what}: candidate value off by {ratio.max():.2f} of the bound"
    tile_max = ref.reshape(M, ntn, tile).max(-1)
    slack = tol[rows, idx] + tol.reshape(M, ntn, tile).max(-1)
    assert (ref[rows, idx] >= tile_max - slack).all(), f"{what}: a tile's winner is not its largest column"
    return float(ratio.max()), rec


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["ldo", "lda"])
def test_form_with_padded_rows(dtype, which):
    """rows of out wider than N (the columns behind N stay NaN, in every slab) and rows of A wider than K (NaN behind K, 48 /
    96 bytes: rows no longer start on a 128-byte line): the projection of 72 rows, four (fp32: eight) slabs on 64 x 64 tiles"""
    eng = engine(dtype)
    M, (N, K) = 72, GEMMS["proj"]
    pl = eng.decode_plan(M)
    split = pl["proj_split"]
    got, rec = _launch(eng, dtype, M, N, K, 64, split, EPI_SLAB, **({"ldo": N + 64} if which == "ldo" else {"lda": K + 24}))
    ref_pre, s1 = _reference(dtype, M, N, K, split)
    ratio = _check(got, ref_pre, ACC * s1, f"projection {dtype} {which} padded")
    assert rec["ring"] == pl["proj_ring"]
    report(f"decode form {dtype} proj [{M} x {N} x {K}] split {split} with {which} padded: max err / tol {ratio:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_args_refusals(dtype):
    from manga_ocr._capi import MocrError
    eng = engine(dtype)
    M, N, K = 64, 768, 768
    A, W, bias = _operands(dtype, M, N, K)
    dA, dW, dB = _device_a(dtype, A, 64, K), _dev(W, dtype), torch.from_numpy(bias.astype(np.float32)).cuda()
    dO = _nan((2, M + GUARD, N), "fp32")
    ok = dict(M=M, N=N, K=K, epilogue=EPI_SLAB, tile=64, split_k=2, lda=0, ldo=0, group_n=0, slab_stride=0, A=dA, W=dW, bias=dB, out=dO, resid=None)
    torch.cuda.synchronize()
    for change, msg in ((dict(epilogue=4), "not exposed"), (dict(epilogue=EPI_ARGMAX), "not exposed"), (dict(tile=4096), "tile GEMM only"),
                        (dict(tile=32), "tile GEMM only"), (dict(lda=K - 8), "lda >= K"), (dict(lda=K + 1), "16-byte"), (dict(ldo=N + 2), "16-byte"),
                        (dict(slab_stride=M * N - 4), "slab_stride"), (dict(slab_stride=M * N + 2), "slab_stride"), (dict(A=None), "bad argument"),
                        (dict(epilogue=EPI_BIAS, split_k=1, bias=None), "bad argument"), (dict(epilogue=EPI_BIAS), "not tileable"),
                        (dict(split_k=5), "not tileable"), (dict(N=800), "not tileable"), (dict(group_n=-1), "bad argument")):
        with pytest.raises(MocrError, match=msg):
            eng.op_gemm_args(**{**ok, **change})
    torch.cuda.synchronize()
    assert torch.isnan(dO).all(), "a refused GEMM wrote its output"


# ------------------------------------------------------------------------------------------------ (c) tile order in column groups
GROUP_CASES = [(128, 2304, (0, 9, 5, 18)), (128, 3072, (0, 12, 7)), (64, 768, (0, 5))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [300, 1500])
@pytest.mark.parametrize("tile,N,groups", GROUP_CASES)
def test_tile_order_in_column_groups(dtype, tile, N, groups, M):
    """gemm_tile_of's column groups (9 for the encoder's QKV, 12 for its FC1): groups that divide the N-tiles, a narrower last
    group, a group wider than the row of tiles and none at all.  A tile no block took stays NaN; whatever the order, every
    block computes the same tile the same way, so the outputs are bit-identical."""
    eng = engine(dtype)
    K = 768
    ref_pre, s1 = _reference(dtype, M, N, K, 1)
    _, _, bias = _operands(dtype, M, N, K)
    ref, tol = _bound(dtype, EPI_BIAS, ref_pre, s1, bias)
    first = None
    for gn in groups:
        got, rec = _launch(eng, dtype, M, N, K, tile, 1, EPI_BIAS, group_n=gn)
        ratio = _check(got, ref, tol, f"group_n {gn}")
        report(f"tile order {dtype} [{M} x {N} x {K}] tile {tile} group_n {gn}: {rec['blocks']} blocks, ring {rec['ring']}, max err / tol {ratio:.3f}")
        if first is None:
            first = got
        np.testing.assert_array_equal(got, first, err_msg=f"group_n {gn} and group_n {groups[0]} differ")


# ------------------------------------------------------------------------------------------------ (d) bit-identity
# (N, K, tile, split, epilogue, M with at most 256 blocks, M with more): both below 1280 rows, so the grid decides the ring
RING_PAIRS = [(2304, 768, 64, 1, EPI_SLAB, 448, 512), (768, 3072, 64, 4, EPI_SLAB, 320, 384), (3072, 768, 128, 1, EPI_BIAS_GELU, 1216, 1408)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,K,tile,split,epi,m4,m2", RING_PAIRS)
def test_ring_depth_does_not_touch_the_sums(dtype, N, K, tile, split, epi, m4, m2):
    """tile_launch's comment: "same K order, same sums: bit-identical either way".  The same leading rows of A on a grid of at
    most one block per compute unit (four slots) and on a larger grid or at 1280 rows and more (two slots)."""
    eng = engine(dtype)
    A, W, bias = _operands(dtype, m2, N, K)

    def run(M):
        dA, dW = _device_a(dtype, A[:M], tile, K), _dev(W, dtype)
        dB = torch.from_numpy(bias.astype(np.float32)).cuda()
        dO = _nan((split, M + GUARD, N), "fp32" if epi == EPI_SLAB else dtype)
        torch.cuda.synchronize()
        eng.op_gemm_args(M=M, N=N, K=K, epilogue=epi, tile=tile, split_k=split, lda=0, ldo=0, group_n=0, slab_stride=(M + GUARD) * N,
                         A=dA, W=dW, bias=dB, out=dO, resid=None)
        return _np(dO), eng.last_tile_launch()

    g4, r4 = run(m4)
    g2, r2 = run(m2)
    report(f"ring depth {dtype} [{N} x {K}] tile {tile} split {split} epi {epi}: M {m4} -> ring {r4['ring']} ({r4['blocks']} blocks), M {m2} -> ring {r2['ring']} ({r2['blocks']} blocks)")
    if _cus() == 256:
        assert (r4["ring"], r2["ring"]) == (4, 2), "the pair does not reach both ring depths"
    assert np.isfinite(g4[:, :m4]).all() and np.isnan(g4[:, m4:]).all() and np.isnan(g2[:, m2:]).all()
    np.testing.assert_array_equal(g2[:, :m4], g4[:, :m4])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,K,split,epi,M", [(768, 3072, 4, EPI_SLAB, 320), (2304, 768, 2, EPI_SLAB, 200), (3072, 768, 1, EPI_BIAS_GELU, 200)])
def test_tile_size_does_not_touch_the_sums(dtype, N, K, split, epi, M):
    """dec_launch_tile's comment: "the tile size does not touch a sum (same K-tiles, same order)" - a compacted batch moves from
    128 x 128 to 64 x 64 tiles under the split it started with and its rows' ids must not change"""
    eng = engine(dtype)
    g64, r64 = _launch(eng, dtype, M, N, K, 64, split, epi)
    g128, r128 = _launch(eng, dtype, M, N, K, 128, split, epi)
    assert (r64["tile"], r128["tile"]) == (64, 128)
    report(f"tile size {dtype} [{M} x {N} x {K}] split {split} epi {epi}: 64 x 64 ring {r64['ring']}, 128 x 128 ring {r128['ring']}")
    assert np.isfinite(g64).all()
    np.testing.assert_array_equal(g64, g128)
