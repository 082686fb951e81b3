"""-m gpu: shared encodings - several decode rows per crop from one encoder pass (include/mocr.h, "shared encodings").

Bottom up: the expansion kernel (mocr_op_enc_expand) bit for bit on the shapes that catch a gather in place; the identity
source against the call without one; whole recognitions against the reference loop on the fp32 oracle
(prefix_util.prefix_generate on the oracle's own encodings, gathered by source); the bf16 decode paths, the classic K/V and the
fp8 ones included; more rows than max_batch; early EOS and compaction; images and regions; the argument errors; the product
surface (score_candidates, recognize_nbest).  mocr_encoded_crops is how every test sees that sharing happened.

Tolerances are those of tests/test_gpu_prefix.py and tests/test_gpu_fp8_attention.py (imported, named where used)."""
import ctypes as C

import numpy as np
import pytest

from gpu_util import crops, report

import constraint_util as cu
import ngram_util as nu
import prefix_util as pu
import score_util as su
from test_gpu_constraints import BF16_LOGIT_TOL, FP32_LOGIT_TOL, _i32, fresh_engine  # noqa: F401
from test_gpu_fp8_attention import FP8_LOGIT_TOL
from test_gpu_prefix import BF16_CASES, _assert_same_run, _enc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V, EOS, START = 6144, 3, 2
S, D = 197, 768
LEN = 24
ERR_ARG = -1


# ------------------------------------------------------------------------------------------------ 1. the expansion kernel, exact
EXPAND_CASES = [("fan-out", 3, 7, [2, 0, 2, 1, 1, 0, 2]),      # row 0 reads a source that row 2 overwrites, row 1 one that row 0 overwrites
                ("cycle", 3, 3, [2, 0, 1]),
                ("identity", 3, 3, [0, 1, 2])]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_expansion_kernel_exact(dtype):
    """mocr_op_enc_expand on a buffer of 7 + 2 guard rows of 197 x 768 elements: the rows hold distinct random bits, the guard
    rows a sentinel.  Every output row is bit-identical to its source AS IT WAS BEFORE THE CALL and rows >= n_rows are untouched:
    the smallest shapes that catch a gather in place (a fan-out whose early rows overwrite later rows' sources, a cycle) and a
    write past the end."""
    eng = su.score_engine("wide", dtype)
    row_bytes = S * D * (2 if dtype == "bf16" else 4)
    rows, guard = 7, 2
    rs = np.random.RandomState(5)
    for name, n_src, n_rows, source in EXPAND_CASES:
        before = rs.randint(0, 256, size=(rows + guard, row_bytes), dtype=np.uint8)
        before[rows:] = 0xA5
        assert len({before[r].tobytes() for r in range(rows)}) == rows
        buf = torch.from_numpy(before).cuda()
        d_src = _i32(source)
        torch.cuda.synchronize()
        eng.op_enc_expand(buf, d_src, n_src, n_rows)
        after = buf.cpu().numpy()
        for r in range(n_rows):
            assert after[r].tobytes() == before[source[r]].tobytes(), f"{name}: row {r} is not source {source[r]} as it was before the call"
        np.testing.assert_array_equal(after[n_rows:], before[n_rows:], err_msg=f"{name}: a row >= n_rows was written")
    from manga_ocr._capi import MocrError
    with pytest.raises(MocrError):
        eng.op_enc_expand(buf, _i32([0, 3, 1]), 3, 3)                  # an index outside [0, n_src) never reaches the kernel
    report(f"enc_expand {dtype}: fan-out 3 -> 7, a cycle and the identity bit-exact against the rows as they were before the call; guard rows untouched")


# ------------------------------------------------------------------------------------------------ 2. the identity is the old call
def test_identity_source_is_the_call_without_one():
    """fp32, wide weights, crops(31, 8), length 24, alternatives plus positions: sources = 0 .. 7 is bit-identical in all six
    outputs to the call without sources, and adds no graph.  Profiled: the plain call launches no enc_expand, the shared one
    exactly one."""
    eng = su.score_engine("wide", "fp32")
    gray = crops(31, 8)
    c0 = eng.encoded_crops()
    plain = eng.recognize_gray(gray, LEN, alternatives=True, positions=True)
    g0 = eng.graph_count()
    shared = eng.recognize_gray(gray, LEN, alternatives=True, positions=True, sources=range(8))
    assert eng.graph_count() == g0, "the identity source captured a decode graph of its own"
    assert eng.encoded_crops() == c0 + 16
    assert len(plain) == len(shared) == 6
    _assert_same_run(shared, plain, "sources = 0 .. 7")
    eng.profile_enable(True)
    try:
        seen = []
        for kw in ({}, dict(sources=range(8))):
            eng.profile_reset()
            eng.recognize_gray(gray, LEN, alternatives=True, positions=True, **kw)
            seen.append({s["name"]: s["launches"] for s in eng.profile_get()})
    finally:
        eng.profile_enable(False)
        eng.profile_reset()
    assert "enc_expand" not in seen[0] and seen[1].get("enc_expand") == 1, (seen[0].get("enc_expand"), seen[1].get("enc_expand"))
    rest = {k: v for k, v in seen[1].items() if k != "enc_expand"}
    assert rest == seen[0], "the shared batch launched something else than the plain one plus the expansion"
    report("shared encodings fp32: sources = 0 .. 7 bit-identical to the call without sources in ids, lens, logp, alternatives and positions; "
           "one enc_expand launch, none without sources")


# ------------------------------------------------------------------------------------------------ 3. fp32 against the reference loop
ORDER = (2, 0, 3, 1)


def test_fp32_shared_rows_against_the_reference_loop():
    """fp32, 4 crops crops(31, 4), 16 rows, length 24: four kinds of row, each over the sources in the order (2, 0, 3, 1) - free;
    P = 5 with token 5 replaced by the oracle's runner-up; the first 3 tokens of the oracle's free row; P = 1 with the oracle's
    runner-up of step 0.  The reference is prefix_generate on the oracle's own encodings gathered by source.  On the oracle
    alone: every free-step top-2 margin exceeds 2 x FP32_LOGIT_TOL (two logits each within the tolerance cannot swap; checked
    on the CPU for exactly these inputs: 4.27e-3 against 2e-3).  Then ids and lengths are identical; logp and alt_logp within
    2 x FP32_LOGIT_TOL of the float64 log-softmax (the bound of tests/test_gpu_prefix.py).  mocr_encoded_crops rises by 4 for
    this call and by 16 for the same rows sent as 16 planes."""
    n = 4
    free_ids, free_logits = su.oracle_run("wide", 31, n, LEN)
    o, enc = _enc("wide", 31, n)
    source, pre = [], []
    for kind in range(4):
        for c in ORDER:
            source.append(c)
            if kind == 0:
                pre.append(None)
            elif kind == 1:
                p = free_ids[c, 1:6].tolist()
                p[4] = int(pu.runner_up(free_logits[c, 4]))
                pre.append(p)
            elif kind == 2:
                pre.append(free_ids[c, 1:4].tolist())
            else:
                pre.append([int(pu.runner_up(free_logits[c, 0]))])
    ids_o, logits, masks = pu.prefix_generate(o, enc[source], pre, None, None, LEN)
    lens_o = nu.lengths(ids_o)
    L = ids_o.shape[1]
    gaps = nu.step_gaps(logits, masks)
    free_steps = np.array([[len(pre[b] or []) <= t < lens_o[b] - 1 for t in range(L - 1)] for b in range(16)])
    distinct = [len({tuple(ids_o[r]) for r in range(16) if source[r] == c}) for c in range(n)]
    print(f"shared fp32: smallest free-step margin {gaps[free_steps].min():.2e}, distinct rows per crop {distinct}", flush=True)
    assert gaps[free_steps].min() > 2 * FP32_LOGIT_TOL and min(distinct) >= 3
    eng = su.score_engine("wide", "fp32", max_batch=16)
    gray = crops(31, n)
    c0 = eng.encoded_crops()
    ids, lens, logp, alt_ids, alt_logp = eng.recognize_gray(gray, LEN, alternatives=True, prefixes=pre, sources=source)
    assert eng.encoded_crops() - c0 == 4, "16 rows over 4 crops: the encoder ran on 4"
    live = np.arange(L)[None, :] < lens_o[:, None]
    np.testing.assert_array_equal(np.where(live, ids[:, :L], 0), np.where(live, ids_o, 0), err_msg="ids differ from prefix_generate's")
    np.testing.assert_array_equal(lens, lens_o)
    want = pu.stored_logp64(logits, masks, ids_o, lens_o)
    worst = float(np.abs(logp[:, :L] - want)[live].max())
    for b in range(16):
        for t in range(1, lens[b]):
            w4, lp4 = cu.masked_top(logits[b, t - 1], masks[b, t - 1])
            np.testing.assert_array_equal(alt_ids[b, t], w4)
            worst = max(worst, float(np.abs(alt_logp[b, t] - lp4).max()))
    print(f"shared fp32: max |logp - float64 log-softmax| {worst:.3e} (bound {2 * FP32_LOGIT_TOL:.0e})", flush=True)
    assert worst <= 2 * FP32_LOGIT_TOL
    c1 = eng.encoded_crops()
    ids2, lens2 = eng.recognize_gray(gray[source], LEN, prefixes=pre)
    assert eng.encoded_crops() - c1 == 16, "the same rows as 16 planes: the encoder ran on 16"
    np.testing.assert_array_equal(ids2, ids); np.testing.assert_array_equal(lens2, lens)
    report(f"shared encodings fp32 vs the reference loop: 16 rows of 4 kinds over 4 crops, ids identical (smallest free-step margin "
           f"{gaps[free_steps].min():.1e}), logp / alt_logp within {worst:.2e} (bound {2 * FP32_LOGIT_TOL:.0e}); 4 crops encoded against 16")


# ------------------------------------------------------------------------------------------------ 4. bf16 decode paths
SHARED_BF16_CASES = BF16_CASES + [("classic", 64, 8), ("fp8", 64, 128 | 64)]


@pytest.mark.parametrize("name,rows,flags", SHARED_BF16_CASES)
def test_bf16_shared_paths(name, rows, flags):
    """bf16, the decode paths of tests/test_gpu_prefix.py plus the classic K/V engine (flag 8: the cross-K/V GEMM runs on the
    expanded rows) and the fp8 one (128 | 64: the e4m3 copy is made behind the expansion).  U = rows / 8 crops - crops(31, 8),
    repeated - 8 rows per crop, interleaved (source[r] = r % U).  The prefixes are the oracle's full free ids, so nothing can
    diverge: ids equal the prefix; logp of the rows of the first 8 crops is within 2 x BF16_LOGIT_TOL of the float64
    log-softmax of the oracle's logits (|d(logit - lse)| <= 2 max |d logit|; the fp8 engine: 2 x FP8_LOGIT_TOL, the logit bound
    of tests/test_gpu_fp8_attention.py); mocr_encoded_crops rises by U."""
    n8 = 8
    free_ids, free_logits = su.oracle_run("wide", 31, n8, LEN)
    eng = su.score_engine("wide", "bf16", max_batch=max(64, rows), flags=flags)
    U = rows // 8
    gray = np.concatenate([crops(31, n8)] * ((U + n8 - 1) // n8))[:U]
    source = [r % U for r in range(rows)]
    pre = [free_ids[source[r] % n8, 1:].tolist() for r in range(rows)]
    c0 = eng.encoded_crops()
    ids, lens, logp = eng.recognize_gray(gray, LEN, scores=True, prefixes=pre, sources=source)
    assert eng.encoded_crops() - c0 == U
    np.testing.assert_array_equal(ids[:, :LEN], free_ids[[s % n8 for s in source]])
    assert (lens == LEN).all()
    want = su.chosen_logp64(free_logits, free_ids)
    first = [r for r in range(rows) if source[r] < n8]
    err = float(np.abs(logp[first, 1:LEN] - want[[source[r] for r in first]]).max())
    bound = 2 * (FP8_LOGIT_TOL if flags & 128 else BF16_LOGIT_TOL)
    print(f"bf16 shared {name}: {rows} rows over {U} crops, max |logp - float64 log-softmax of the oracle| {err:.3e} (bound {bound:.0e})", flush=True)
    assert np.isfinite(logp).all() and err <= bound
    report(f"shared encodings bf16 {name} ({rows} rows over {U} crops, flags {flags}): full-text prefix emitted exactly, logp within {err:.2e} "
           f"of the oracle (bound {bound:.0e}), {U} crops encoded")


# ------------------------------------------------------------------------------------------------ 5. more rows than max_batch
def test_more_rows_than_max_batch():
    """fp32, max_batch 8, 3 crops, 20 rows with source[r] = r % 3 and the first 0 / 1 / 3 tokens of the oracle's free rows as
    prefixes, cycled through the rows: the call is cut into three internal batches in row order, every batch encodes the
    crops its own rows name.  ids and lengths equal the oracle's free rows (every free-step margin of those exceeds
    2 x FP32_LOGIT_TOL, asserted on the oracle first); mocr_encoded_crops rises by at least 3 and at most 3 per batch = 9."""
    n, rows = 3, 20
    free_ids, free_logits = su.oracle_run("wide", 31, 8, LEN)
    gaps = nu.step_gaps(free_logits[:n], np.ones_like(free_logits[:n], bool))
    assert gaps.min() > 2 * FP32_LOGIT_TOL, gaps.min()
    eng = su.score_engine("wide", "fp32")
    assert eng.max_batch == 8
    source = [r % n for r in range(rows)]
    pre = [free_ids[source[r], 1:1 + (0, 1, 3)[(r // n) % 3]].tolist() or None for r in range(rows)]
    c0 = eng.encoded_crops()
    ids, lens, logp = eng.recognize_gray(crops(31, 8)[:n], LEN, scores=True, prefixes=pre, sources=source)
    rose = eng.encoded_crops() - c0
    np.testing.assert_array_equal(ids[:, :LEN], free_ids[source]); assert (lens == nu.lengths(free_ids)[source]).all()
    assert 3 <= rose <= 9, rose
    assert np.isfinite(logp).all() and (logp[:, 1:LEN] < 0).all()
    report(f"shared encodings fp32, 20 rows over 3 crops at max_batch 8: three internal batches, ids equal the oracle's free rows, {rose} crops encoded")


# ------------------------------------------------------------------------------------------------ 6. early EOS and compaction
def test_shared_compaction_graphs_and_memory(fresh_engine):
    """Early-EOS weights, bf16, 96 rows from 12 crops (source[r] = r % 12), length 32, mixed prefix lengths as in
    tests/test_gpu_prefix.py (0 / 2 / 5 tokens of the free run, every fourth row ending its prefix in EOS).  The crops are 12
    of crops(4322, 48): the six whose free rows end after 17 tokens on the oracle under these weights (numbers 5, 19, 23, 32,
    34, 39) and six that run to the end, so that with the forced EOS rows two thirds of the batch finish early and its rows
    are compacted (12 arbitrary crops nearly all run to the end: 72 of 96 rows unfinished is no smaller graph).  Compacted equals
    MOCR_FLAG_NO_COMPACTION in ids and lengths; rows were compacted; free HBM is unchanged until the first shared call; a
    repeated identical call adds no graph."""
    from manga_ocr.engine import device_memory
    rows, U, max_len = 96, 12, 32
    gray = crops(4322, 48)[[5, 19, 23, 32, 34, 39, 0, 1, 2, 3, 4, 6]]
    source = [r % U for r in range(rows)]
    eng = fresh_engine("eos", "bf16", max_batch=96)
    free_ids, free_lens = eng.recognize_gray(gray[source], max_len)
    pre = []
    for b in range(rows):
        p = free_ids[b, 1:1 + (0, 2, 5, 2)[b % 4]].tolist()
        p = [t for t in p if t != EOS]
        pre.append(p + [EOS] if b % 4 == 3 else p or None)
    eng.recognize_gray(gray[source], max_len, scores=True, prefixes=pre)          # everything but sharing has its buffers now
    mem0 = device_memory(0)[0]
    eng.recognize_gray(gray[source], max_len)
    assert device_memory(0)[0] == mem0, "a call that shares nothing moved the free HBM"
    c0 = eng.encoded_crops()
    ids, lens, logp = eng.recognize_gray(gray, max_len, scores=True, prefixes=pre, sources=source)
    assert eng.encoded_crops() - c0 == U
    g1 = eng.graph_count()
    ids2, lens2, logp2 = eng.recognize_gray(gray, max_len, scores=True, prefixes=pre, sources=source)
    assert eng.graph_count() == g1, "a repeated call captured another decode graph"
    np.testing.assert_array_equal(ids2, ids); np.testing.assert_array_equal(lens2, lens)
    np.testing.assert_array_equal(logp2.view(np.uint32), logp.view(np.uint32))
    for b in range(rows):
        if pre[b]:
            assert ids[b, 1:1 + len(pre[b])].tolist() == pre[b]
        if b % 4 == 3:
            assert lens[b] == len(pre[b]) + 1 and (ids[b, lens[b]:] == 0).all()
    nc = fresh_engine("eos", "bf16", max_batch=96, flags=2048)          # MOCR_FLAG_NO_COMPACTION
    u_ids, u_lens, _ = nc.recognize_gray(gray, max_len, scores=True, prefixes=pre, sources=source)
    np.testing.assert_array_equal(u_ids, ids); np.testing.assert_array_equal(u_lens, lens)
    assert lens.min() < lens.max() and eng.compaction_count() > 0 and nc.compaction_count() == 0
    report(f"shared encodings bf16 early-EOS 96 rows over 12 crops: compacted == uncompacted, no graph added by a repeat, HBM untouched before the first shared call")


# ------------------------------------------------------------------------------------------------ 7. images and regions
def _three_crops(seed=7):
    """three crops of different sizes, the third RGB and rotated by 90 degrees (seeds 8 and 9 were tried first on the CPU: their
    smallest oracle margins under the two sets below are 3.1e-4 and 9.1e-4, under the 2e-3 the test needs; seed 7 has 4.7e-3)"""
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, size=(60, 90), dtype=np.uint8), rs.randint(0, 256, size=(224, 224), dtype=np.uint8),
            rs.randint(0, 256, size=(130, 40, 3), dtype=np.uint8)], [0, 0, 1]


def test_images_with_sources_equal_the_crops_repeated(fresh_engine):
    """fp32: three crops of different sizes, one of them rotated, each decoded under two different token sets through
    recognize_images(sources=[0, 0, 1, 1, 2, 2]), against the six-image call with the crops repeated.  The planes of both calls
    are bit-equal (mocr_preprocess), and on the oracle every step's top-2 margin inside the row's set exceeds
    2 x FP32_LOGIT_TOL for these planes - asserted first - so the ids and lengths must be equal.  3 crops are preprocessed and
    encoded against 6."""
    eng = fresh_engine("wide", "fp32", max_batch=8)
    imgs, rot = _three_crops()
    source = [0, 0, 1, 1, 2, 2]
    six, rot6 = [imgs[s] for s in source], [rot[s] for s in source]
    planes = eng.preprocess(imgs, rotate=rot)
    np.testing.assert_array_equal(eng.preprocess(six, rotate=rot6), planes[source])
    masks = np.stack([cu.mask_of(np.arange(0, V, 2)), cu.mask_of(np.arange(0, 3000))] * 3)
    o = su.score_oracle("wide")
    with torch.no_grad():
        enc = o.encode(o.preprocess_gray(planes))
    ids_o, logits = cu.masked_generate(o, enc[source], masks, LEN)
    gaps = nu.step_gaps(logits, np.broadcast_to(masks[:, None, :], logits.shape))
    print(f"images with sources: smallest oracle margin {gaps.min():.2e}", flush=True)
    assert gaps.min() > 2 * FP32_LOGIT_TOL, gaps.min()
    sets = [eng.token_set(np.nonzero(m)[0]) for m in masks[:2]] * 3
    eng.set_generate_max_length(LEN)
    c0 = eng.encoded_crops()
    ids, lens, logp = eng.recognize_images(imgs, rotate=rot, scores=True, token_sets=sets, sources=source)
    c1 = eng.encoded_crops()
    ids6, lens6, logp6 = eng.recognize_images(six, rotate=rot6, scores=True, token_sets=sets)
    assert (c1 - c0, eng.encoded_crops() - c1) == (3, 6)
    np.testing.assert_array_equal(ids, ids6); np.testing.assert_array_equal(lens, lens6)
    np.testing.assert_array_equal(ids[:, :LEN], ids_o)
    assert np.abs(logp - logp6).max() <= 2 * 2 * FP32_LOGIT_TOL, "both calls are within 2 x FP32_LOGIT_TOL of the float64 log-softmax"
    assert (ids[0] != ids[1]).any() and (ids[0] != ids[2]).any(), "the rows of a crop differ by their sets, the crops by their pixels"
    report(f"shared encodings, images: 3 crops (one rotated) x 2 token sets through sources= equal the six-image call in ids and lengths "
           f"(smallest oracle margin {gaps.min():.1e}); 3 crops encoded against 6")


def test_regions_with_sources_and_a_sliver(fresh_engine):
    """One page, two regions and a sliver, rows [0, 0, 1, 2, 2]: both rows of the sliver have length 0 - ids all pad, scores 0,
    alternative ids -1 - and ignore their prefixes; the two rows of region 0 are one crop under two prefixes; 2 crops are encoded."""
    eng = fresh_engine("wide", "fp32", max_batch=8)
    page = np.random.RandomState(3).randint(0, 256, size=(300, 400, 3), dtype=np.uint8)
    regions = [(0, 20, 30, 120, 80), (0, 200, 100, 60, 150), (0, 399, 10, 1, 0)]
    source = [0, 0, 1, 2, 2]
    eng.set_generate_max_length(LEN)
    plain = eng.recognize_regions([page], regions)
    assert plain[1][2] == 0 and (plain[1][:2] > 1).all()
    first = eng.recognize_regions([page], regions, alternatives=True, sources=source)
    pre = [None, first[0][0, 1:4].tolist(), None, [5, 6], None]       # row 1: the first tokens of row 0, the same crop's free row
    c0 = eng.encoded_crops()
    ids, lens, logp, alt_ids, alt_logp = eng.recognize_regions([page], regions, alternatives=True, prefixes=pre, sources=source)
    assert eng.encoded_crops() - c0 == 2
    assert (lens[:3] > 1).all() and lens[3:].tolist() == [0, 0] and lens[:3].tolist() == first[1][:3].tolist()
    np.testing.assert_array_equal(ids[[0, 2]], first[0][[0, 2]], err_msg="the free rows moved between two calls of the same shape")
    assert (ids[3:] == 0).all() and (logp[3:] == 0).all() and (alt_ids[3:] == -1).all() and (alt_logp[3:] == 0).all()
    np.testing.assert_array_equal(ids[0], ids[1], err_msg="a self-prefix of the same crop, in the same batch, left the free row")
    assert (ids[0] != ids[2]).any()
    report("shared encodings, regions: rows [0, 0, 1, sliver, sliver] - the sliver's rows have length 0, two crops encoded for three rows")


# ------------------------------------------------------------------------------------------------ 8. argument errors
def test_shared_argument_errors(fresh_engine):
    """every MOCR_ERR_ARG case of the shared-encodings section, through the gray_host and the device entry points; a null
    source with n_rows == n_planes is the prefix call.  Which crop a row read shows in its scores, not in its ids (under these
    weights every crop decodes to the same tokens): rows of one crop in one batch are bit-equal, rows of different crops
    differ by far more than 4 x FP32_LOGIT_TOL (the oracle's rows of crops(1, 3) are >= 4.0e-2 apart, each engine row is within
    2 x FP32_LOGIT_TOL of its own)."""
    eng = fresh_engine("wide", "fp32", max_batch=4)
    gray = crops(1, 3)
    W = eng.spec.max_len
    ids = np.zeros((8, W), np.int32); lens = np.zeros(8, np.int32); lp = np.zeros((8, W), np.float32)
    apart = lambda a, b: float(np.abs(a[1:8] - b[1:8]).max())            # noqa: E731
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)       # noqa: E731
    src = lambda *v: np.array(v, np.int32)                                # noqa: E731

    def host(n_planes, n_rows, source):
        return eng.lib.mocr_recognize_gray_host_shared(eng._h, P(gray), n_planes, n_rows, P(source), 8, P(ids), P(lens), P(lp), *[None] * 7, 0)
    c0 = eng.encoded_crops()
    assert host(3, 5, src(2, 0, 2, 1, 1)) == 0 and lens[:5].tolist() == [8] * 5 and eng.encoded_crops() - c0 == 4, "4 + 1 rows: 3 + 1 crops"
    assert (ids[0] == ids[2]).all() and (lp[0].view(np.uint32) == lp[2].view(np.uint32)).all(), "two rows of one crop in one batch"
    assert min(apart(lp[0], lp[1]), apart(lp[0], lp[3]), apart(lp[1], lp[3])) > 4 * FP32_LOGIT_TOL, "rows of different crops read the same encoding"
    first_lp = lp[:4].copy()
    assert host(3, 5, src(2, 0, 3, 1, 1)) == ERR_ARG and host(3, 5, src(2, 0, -1, 1, 1)) == ERR_ARG, "an index out of range"
    assert host(3, 5, src(2, 0, 2, 0, 0)) == ERR_ARG and "no row names" in eng.lib.mocr_last_error(eng._h).decode(), "an unreferenced plane"
    assert host(3, 0, src(0)) == ERR_ARG and host(3, -1, src(0)) == ERR_ARG, "n_rows < 1"
    assert host(3, 5, None) == ERR_ARG and host(3, 2, None) == ERR_ARG, "source null: n_rows must equal n_planes"
    assert host(3, 3, None) == 0, "source null, n_rows == n_planes: the prefix call"
    plain = eng.recognize_gray(gray, 8)
    np.testing.assert_array_equal(ids[:3], plain[0])
    assert eng.encoded_crops() - c0 == 4 + 3 + 3, "a refused call encoded something"
    dg = torch.from_numpy(gray).cuda()
    d_ids = torch.zeros((8, W), dtype=torch.int32, device="cuda"); d_len = torch.zeros(8, dtype=torch.int32, device="cuda")
    d_lp = torch.zeros((8, W), dtype=torch.float32, device="cuda")

    def dev(n_planes, n_rows, source):
        rc = eng.lib.mocr_recognize_device_shared(eng._h, C.c_void_p(dg.data_ptr()), n_planes, n_rows, P(source), C.c_void_p(d_ids.data_ptr()),
                                                  C.c_void_p(d_len.data_ptr()), C.c_void_p(d_lp.data_ptr()), *[None] * 7, 0)
        eng.synchronize()
        return rc
    eng.set_generate_max_length(8)
    assert dev(3, 4, src(2, 0, 2, 1)) == 0
    got, glp = d_ids.cpu().numpy(), d_lp.cpu().numpy()
    assert d_len.cpu().numpy()[:4].tolist() == [8] * 4 and (got[0] == got[2]).all() and (glp[0].view(np.uint32) == glp[2].view(np.uint32)).all()
    assert min(apart(glp[0], glp[1]), apart(glp[0], glp[3]), apart(glp[1], glp[3])) > 4 * FP32_LOGIT_TOL
    np.testing.assert_array_equal(glp[:4].view(np.uint32), first_lp.view(np.uint32), err_msg="the device call of the host call's first batch")
    assert dev(3, 4, src(2, 0, 3, 1)) == ERR_ARG and dev(3, 4, src(2, 0, 2, 0)) == ERR_ARG and dev(3, 0, src(0)) == ERR_ARG
    assert dev(3, 5, src(2, 0, 2, 1, 1)) == ERR_ARG, "n_rows > max_batch on the device call"
    assert dev(3, 4, None) == ERR_ARG and dev(3, 3, None) == 0
    np.testing.assert_array_equal(d_ids.cpu().numpy()[:3], plain[0])


# ------------------------------------------------------------------------------------------------ 9. the product surface
def _want_branches(rec, count):
    """the selection rule of the issue, restated: (loss, t, j) ascending over the positions before the last"""
    found = []
    for t in range(len(rec.alt_ids) - 1):
        for j in range(1, 4):
            if rec.alt_ids[t, j] >= 0 and np.isfinite(rec.alt_logprobs[t, j]):
                found.append((float(rec.alt_logprobs[t, 0]) - float(rec.alt_logprobs[t, j]), t, j))
    return [(t, j) for _, t, j in sorted(found)[:count]]


def test_product_surface_shared():
    from PIL import Image
    from manga_ocr import MangaOcr
    m = MangaOcr(synthetic_seed=0, dtype="fp32", max_batch=8)
    try:
        img = Image.fromarray(crops(77, 1)[0])
        free = m.recognize_alternatives(img)
        own = free.ids[1:-1].tolist() if free.ids[-1] == EOS else free.ids[1:8].tolist()
        other = own[::-1]
        seen, real = [], m.engine.recognize_images

        def spy(images, *a, **kw):
            seen.append((len(images), len(kw["sources"]) if "sources" in kw else None))
            return real(images, *a, **kw)
        m.engine.recognize_images = spy
        c0 = m.engine.encoded_crops()
        recs = m.score_candidates(img, [own, other])
        assert seen == [(1, 2)] and m.engine.encoded_crops() - c0 == 1, "one engine call of 2 rows and 1 image"
        assert recs[0].ids.tolist() == [START] + own + [EOS] and recs[1].ids.tolist() == [START] + other + [EOS]
        del seen[:]
        one = m.score_text(img, own)
        assert abs(recs[0].logprob - one.logprob) <= 2 * FP32_LOGIT_TOL * (len(own) + 1), (recs[0].logprob, one.logprob)
        assert recs[1].logprob < recs[0].logprob < 0 and recs[0].n_forced == len(own) + 1
        del seen[:]
        c0 = m.engine.encoded_crops()
        best = m.recognize_nbest(img, 4)
        assert m.engine.encoded_crops() - c0 == 2 and seen == [(1, None), (1, 3)], f"one crop per engine call, two calls: {seen}"
        assert len(best) == 4 and any(r.ids.tolist() == free.ids.tolist() for r in best), "the greedy row is among the results"
        lp = [r.logprob for r in best]
        assert lp == sorted(lp, reverse=True)
        branches = [free.branch(t, j) for t, j in _want_branches(free, 3)]
        others = [r for r in best if r.ids.tolist() != free.ids.tolist()]
        assert sorted(r.ids[1:1 + r.n_forced].tolist() for r in others) == sorted(branches), "every other entry starts with its branch(t, j)"
        del seen[:]
        assert [r.ids.tolist() for r in m.recognize_nbest(img, 1)] == [free.ids.tolist()] and seen == [(1, None)], "k = 1: the greedy row, no second call"
    finally:
        m.close()
