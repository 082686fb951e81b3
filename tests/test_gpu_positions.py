"""GPU: token positions (include/mocr.h, "token positions") - the positions kernel against the float64 reference on inputs
each aimed at one mutant, and the engine end to end on every decode path against the teacher-forced oracle."""
import functools

import numpy as np
import pytest

import position_util as pu
from gpu_util import bf16_round, crops, report
from manga_ocr.weights import DEFAULT_SPEC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")      # before the engine's library: one HIP runtime per process, torch's

# The bounds are multiples of the max errors measured on an MI355X (every run reports its figures through gpu_util.report),
# rounded up, each below its ceiling (5e-5 kernel, 2e-3 fp32 engine, half a patch = 3.57e-2 for bf16 cx / cy):
#   kernel, map and fields against float64, both dtypes, all cases: worst 4.34e-7 (fp32 nonsquare; bf16 4.22e-7)    -> 4x
#   fp32 engine, five fields over 113 tokens: cx 3.45e-6 cy 2.52e-6 sx 2.61e-6 sy 1.47e-6 mass 1.77e-6              -> 4x
#   bf16 cx / cy: small-batch 7.4e-3, classic 9.5e-3, latent 1.09e-2 (also compacted on two lanes), with a token set and
#   n-grams 7.1e-3                                                                                                  -> 2x
#   bf16 latent with fp8 attention: cx 1.21e-2, cy 1.34e-2                                                          -> 2x
KERNEL_TOL = 2e-6
FP32_TOL = 1.5e-5
BF16_CXY_TOL = 2.2e-2
FP8_CXY_TOL = 2.7e-2
assert KERNEL_TOL <= 5e-5 and FP32_TOL <= 2e-3 and max(BF16_CXY_TOL, FP8_CXY_TOL) <= 0.5 / 14
LATENT, FP8, NO_COMPACTION = 64, 128, 2048


def _key(i, j):
    return 1 + 14 * i + j


@functools.lru_cache(maxsize=None)
def _engine(dtype, max_batch=8, flags=0, lanes=1):
    from manga_ocr.engine import Engine
    return Engine(pu.pos_weights(), DEFAULT_SPEC, dtype=dtype, device=0, max_batch=max_batch, flags=flags, lanes=lanes)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.mocr_oracle import Oracle
    return Oracle(pu.pos_weights(), DEFAULT_SPEC)


def _gray(n):
    g = crops(pu.CROP_SEED, 6)
    return g[:n] if n <= 6 else np.concatenate([g] + [crops(pu.CROP_SEED + 1 + k, 6) for k in range((n - 1) // 6)])[:n]


@functools.lru_cache(maxsize=None)
def _enc(n):
    """the oracle's encoder output of the first n test crops: computed once, shared by the tests that teacher-force on it"""
    o = _oracle()
    return o.encode(o.preprocess_gray(_gray(n)))


# ---------------------------------------------------------------------------------------------- the kernel
def _inputs(case, T, rng):
    """q [3, T, 768], K [3, 197, 768] float32 for one mutant (see the test's docstring)"""
    rows = 3
    q = np.zeros((rows, T, 768), np.float32)
    K = np.zeros((rows, 197, 768), np.float32)
    lead = np.arange(12) * 64                                # dim 0 of every head
    if case == "extreme":
        # scaled scores reach +-100 (exp(100) overflows fp32 without the maximum subtracted); every value is a multiple of
        # 1/8 and every partial sum below 2^11, so the scores themselves are exact in fp32 and bf16
        q[:] = rng.randint(-4, 5, size=q.shape) / 8.0
        K[:] = rng.randint(-4, 5, size=K.shape) / 8.0
        q[:, :, lead] = 8.0
        K[:, :, lead] = rng.randint(-100, 101, size=(rows, 197, 12))
        K[:, 5, lead] = 100.0
        K[:, 9, lead] = -100.0
    elif case == "one_sharp":
        # head 0 a delta on patch (5, 6), eleven heads flat: averaging the SCORES over the heads instead of the probabilities
        # gives another map
        q[:] = rng.standard_normal(q.shape)
        K[:] = 0.01 * rng.standard_normal(K.shape)
        q[:, :, :64] = 0.0
        q[:, :, 0] = 8.0
        K[:, :, :64] = 0.0
        K[:, _key(5, 6), 0] = 40.0
    elif case == "nonsquare":
        # most mass on patch row 2, column 11: swapped u / v and an off-by-one from CLS both move the centre
        q[:] = 0.1 * rng.standard_normal(q.shape)
        K[:] = 0.1 * rng.standard_normal(K.shape)
        q[:, :, lead] = 8.0
        K[:, :, lead] = 0.0
        K[:, _key(2, 11), lead] = 7.0
    elif case == "delta":
        # every head a delta on one patch: the variance is 0 and must not come out negative (sx NaN)
        q[:] = 0.1 * rng.standard_normal(q.shape)
        K[:] = 0.1 * rng.standard_normal(K.shape)
        q[:, :, lead] = 8.0
        K[:, _key(9, 3), lead] = 60.0
    elif case == "cls":
        # every head on CLS: the mass is below 1e-20 and the guard values come out
        q[:, :, lead] = 8.0
        K[:, 0, lead] = 80.0
    else:
        q[:] = rng.standard_normal(q.shape)
        K[:] = rng.standard_normal(K.shape)
    return q, K


@pytest.mark.parametrize("case", ["extreme", "one_sharp", "nonsquare", "delta", "cls", "random"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_positions_kernel_against_float64(dtype, case):
    """mocr_op_attn_positions, rows = 3, T in {1, 16, 17, 40}, lengths (T, 1, T - 1).  The inputs are rounded to the engine's
    dtype first, so the float64 reference sees the same numbers; the error left is fp32 accumulation and __expf.  In every
    case the K buffer carries 16 further key rows of 1e4 behind the tested extent - an unmasked 13th key tile would read them
    into the last row's softmax - and positions at and behind d_len must be exactly 0."""
    eng = _engine(dtype)
    worst_map = worst_f = 0.0
    for T in (1, 16, 17, 40):
        rng = np.random.RandomState(1000 + T)
        q, K = _inputs(case, T, rng)
        if dtype == "bf16":
            q, K = bf16_round(q), bf16_round(K)
        lens = np.array([T, 1, T - 1], np.int32)
        ref_map, ref_f = pu.ref_positions(q, K, lens)
        tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        d_q = torch.from_numpy(q).cuda().to(tdt)
        Kpad = np.concatenate([K.reshape(-1, 768), np.full((16, 768), 1e4, np.float32)])
        d_k = torch.from_numpy(Kpad).cuda().to(tdt)
        d_len = torch.from_numpy(lens).cuda()
        d_pos = torch.full((3, T, 5), float("nan"), device="cuda")
        d_map = torch.full((3, T, 197), float("nan"), device="cuda")
        eng.op_attn_positions(d_q, d_k, d_len, 3, T, d_pos, d_map)
        got_f, got_map = d_pos.cpu().numpy().astype(np.float64), d_map.cpu().numpy().astype(np.float64)
        d_pos2 = torch.full((3, T, 5), float("nan"), device="cuda")
        eng.op_attn_positions(d_q, d_k, d_len, 3, T, d_pos2, None)           # the map is optional and moves nothing
        np.testing.assert_array_equal(d_pos2.cpu().numpy(), d_pos.cpu().numpy())
        # every row once more on its own, its 197 keys followed directly by 16 key rows of 1e4: the outputs must not change
        for r in range(3):
            Kr = np.concatenate([K[r], np.full((16, 768), 1e4, np.float32)])
            d_kr = torch.from_numpy(Kr).cuda().to(tdt)
            d_pr = torch.full((1, T, 5), float("nan"), device="cuda")
            d_mr = torch.full((1, T, 197), float("nan"), device="cuda")
            eng.op_attn_positions(d_q[r:r + 1].contiguous(), d_kr, d_len[r:r + 1].contiguous(), 1, T, d_pr, d_mr)
            np.testing.assert_array_equal(d_pr.cpu().numpy()[0], d_pos.cpu().numpy()[r])
            np.testing.assert_array_equal(d_mr.cpu().numpy()[0], d_map.cpu().numpy()[r])
        assert np.isfinite(got_f).all() and np.isfinite(got_map).all(), f"{case} T={T}"
        for r in range(3):
            assert (got_f[r, lens[r]:] == 0).all() and (got_map[r, lens[r]:] == 0).all(), f"{case} T={T} row {r}: behind d_len"
        worst_map = max(worst_map, np.abs(got_map - ref_map).max())
        worst_f = max(worst_f, np.abs(got_f - ref_f).max())
        if case == "delta":
            assert (got_f[0, :, 2:4] < 1e-6).all()
        if case == "cls":
            np.testing.assert_array_equal(got_f[0, :, :4], np.tile([0.5, 0.5, 0.0, 0.0], (T, 1)))
        if case == "nonsquare":
            assert abs(got_f[0, 0, 0] - ref_f[0, 0, 0]) < 1e-3 and ref_f[0, 0, 0] > 0.55 and ref_f[0, 0, 1] < 0.45
    report(f"attn_positions {dtype} {case}: max |map - f64| {worst_map:.2e}, max |fields - f64| {worst_f:.2e} (tol {KERNEL_TOL:.1e})")
    assert worst_map <= KERNEL_TOL and worst_f <= KERNEL_TOL


# ---------------------------------------------------------------------------------------------- end to end
def _check_fields(name, pos, ids, lens, n, tol, enc_rows, max_len, enc=None):
    """all tokens of all rows against the oracle teacher-forced on `ids`; position 0 and the pad tail exactly 0"""
    o = _oracle()
    ref = pu.reference_for_ids(o, None, ids[:, :max_len], lens, enc=_enc(enc_rows)[:n] if enc is None else enc)
    err = np.zeros(5)
    cnt = 0
    for b in range(n):
        L = int(lens[b])
        assert (pos[b, 0] == 0).all() and (pos[b, L:] == 0).all(), f"{name}: row {b} outside 1 .. len - 1"
        err = np.maximum(err, np.abs(pos[b, 1:L].astype(np.float64) - ref[b, 1:L]).max(axis=0))
        cnt += L - 1
    sel = np.concatenate([ref[b, 1:int(lens[b])] for b in range(n)])
    report(f"positions {name}: {n} rows, {cnt} tokens, lengths {int(lens.min())}..{int(lens.max())}: max err cx {err[0]:.2e} cy {err[1]:.2e} "
           f"sx {err[2]:.2e} sy {err[3]:.2e} mass {err[4]:.2e} (bound {tol:.2e}); reference std cx {sel[:, 0].std():.3f} cy {sel[:, 1].std():.3f}")
    return err


def test_fp32_engine_positions_match_the_oracle():
    """6 crops, max_len 24, early-EOS weights with the scaled query: ids identical to the oracle's, the five fields within
    FP32_TOL of the reference on those ids"""
    eng, o = _engine("fp32"), _oracle()
    gray = _gray(6)
    want = o.generate(_enc(6), max_len=24)
    ids, lens, pos = eng.recognize_gray(gray, 24, positions=True)
    np.testing.assert_array_equal(ids[:, :want.shape[1]], want)
    assert (ids[:, want.shape[1]:] == 0).all() and len(set(lens.tolist())) >= 3
    err = _check_fields("fp32", pos, ids, lens, 6, FP32_TOL, 6, 24)
    assert err.max() <= FP32_TOL


@pytest.mark.parametrize("name,rows,flags,kernels", [
    ("small-batch", 8, 0, ("sm_qc", "pos_hist_ln", "dec_attn_cross")),
    ("classic (automatic choice at 40 rows)", 40, 0, ("dec_attn_cross", "dec_add_ln")),
    ("latent", 40, LATENT, ("lat_attn_cross", "dec_add_ln")),
    ("latent fp8 attention", 40, LATENT | FP8, ("lat8_attn_cross", "dec_add_ln")),
])
def test_bf16_positions_on_every_decode_path(name, rows, flags, kernels):
    """the recording differs per path (the add/LayerNorm launch's cache store; the small-batch path's row kernel).  The
    reference is teacher-forced on the engine's own ids: bf16 ids may leave the oracle's at near-ties."""
    eng = _engine("bf16", max_batch=rows, flags=flags)
    ids, lens, pos = eng.recognize_gray(_gray(rows), 24, positions=True)
    tol = FP8_CXY_TOL if flags & FP8 else BF16_CXY_TOL
    err = _check_fields(f"bf16 {name}", pos, ids, lens, rows, tol, 40, 24)
    assert max(err[0], err[1]) <= tol and np.isfinite(pos).all()
    # the path this case is about did run: an instrumented (eager) pass names its kernels, and gives the same outputs
    eng.profile_enable(True)
    try:
        eng.profile_reset()
        ids2, lens2, pos2 = eng.recognize_gray(_gray(rows), 24, positions=True)
        ran = {s["name"] for s in eng.profile_get() if s["launches"] > 0}
    finally:
        eng.profile_enable(False)
    others = {"sm_qc", "pos_hist_ln", "dec_attn_cross", "lat_attn_cross", "lat8_attn_cross"} - set(kernels)
    assert set(kernels) <= ran and not (others & ran), sorted(ran)
    assert {"gemm_pos_k", "gemm_pos_q", "attn_positions"} <= ran
    np.testing.assert_array_equal(ids2, ids)
    np.testing.assert_array_equal(pos2, pos)


def test_bf16_positions_survive_compaction_on_two_lanes():
    eng = _engine("bf16", max_batch=40, flags=LATENT, lanes=2)
    base = eng.compaction_count()
    gray = np.tile(_gray(40), (2, 1, 1))                     # every lane the same 40 crops: one encoder pass of the oracle serves both
    ids, lens, pos = eng.recognize_gray(gray, 48, positions=True)
    n_comp = eng.compaction_count() - base
    ids0, lens0 = eng.recognize_gray(gray, 48)
    np.testing.assert_array_equal(ids, ids0)
    np.testing.assert_array_equal(lens, lens0)
    err = _check_fields(f"bf16 latent, 2 lanes x 40 rows, {n_comp} compactions", pos, ids, lens, 80, BF16_CXY_TOL, 40, 48,
                        enc=torch.cat([_enc(40), _enc(40)]))
    assert n_comp > 0 and lens.min() < lens.max()
    assert max(err[0], err[1]) <= BF16_CXY_TOL


@pytest.mark.parametrize("dtype,rows", [("fp32", 3), ("fp32", 40), ("bf16", 3), ("bf16", 40)])
def test_positions_move_no_other_output(dtype, rows):
    """ids, lengths, scores and alternatives with positions are array_equal to those without, calls interleaved on one engine;
    in a batch that mixes jobs with and without positions the rows of the job that did not ask are not written"""
    eng = _engine(dtype, max_batch=40, flags=LATENT if dtype == "bf16" else 0)
    gray = _gray(rows)
    a = eng.recognize_gray(gray, 24, alternatives=True)
    b = eng.recognize_gray(gray, 24, alternatives=True, positions=True)
    c = eng.recognize_gray(gray, 24, alternatives=True)
    for x, y, z in zip(a, b[:5], c):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x, z)
    pos = b[5]
    assert pos.shape == (rows, DEFAULT_SPEC.max_len, 5) and np.abs(pos).max() > 0
    # one batch, two jobs: the first asks, the second does not
    k = (rows + 1) // 2
    d = torch.from_numpy(gray).cuda()
    L = DEFAULT_SPEC.max_len
    out = torch.zeros((rows, L), dtype=torch.int32, device="cuda")
    ln = torch.zeros((rows,), dtype=torch.int32, device="cuda")
    dpos = torch.full((rows, L, 5), float("nan"), device="cuda")
    eng.set_generate_max_length(24)
    try:
        eng.recognize_device(d[:k], k, out[:k], ln[:k], d_out_pos=dpos[:k])
        eng.recognize_device(d[k:], rows - k, out[k:], ln[k:])
        eng.synchronize()
    finally:
        eng.set_generate_max_length(L)
    np.testing.assert_array_equal(out.cpu().numpy(), a[0])
    np.testing.assert_array_equal(ln.cpu().numpy(), a[1])
    got = dpos.cpu().numpy()
    assert np.isnan(got[k:]).all(), "rows of the job that did not ask were written"
    if dtype == "fp32":
        np.testing.assert_array_equal(got[:k], pos[:k])
    else:
        np.testing.assert_allclose(got[:k], pos[:k], atol=1e-6)


def test_region_slivers_follow_padded_rect():
    """the Python restatement of the engine's region cut (regions.padded_rect) decides 'sliver' where the engine does: such a
    region has out_len 0 and a zero positions row; the others are decoded and carry positions"""
    from manga_ocr.regions import padded_rect
    eng = _engine("bf16", max_batch=40, flags=LATENT)
    page = np.random.RandomState(5).randint(0, 256, size=(300, 400, 3), dtype=np.uint8)
    regs = [(0, 20, 30, 100, 60), (0, 403, 10, 50, 50), (0, 10, 10, 0, 0), (0, 396, 0, 50, 40), (0, 100, 303, 40, 40)]
    eng.set_generate_max_length(24)
    try:
        ids, lens, pos = eng.recognize_regions([page], regs, positions=True)
    finally:
        eng.set_generate_max_length(DEFAULT_SPEC.max_len)
    rects = [padded_rect(r[1:], 300, 400) for r in regs]
    assert [r is None for r in rects] == [False, True, True, False, True]
    for i, r in enumerate(rects):
        assert (lens[i] == 0) == (r is None), (i, r, lens[i])
        if r is None:
            assert (pos[i] == 0).all()
        else:
            assert (pos[i, 1:lens[i], 4] > 0).all() and (pos[i, 0] == 0).all() and (pos[i, lens[i]:] == 0).all()


def test_positions_compose_with_a_token_set_and_ngrams():
    eng = _engine("bf16", max_batch=40, flags=LATENT)
    gray = _gray(6)
    half = eng.token_set(np.nonzero(np.random.RandomState(7).rand(DEFAULT_SPEC.vocab) < 0.5)[0])
    ids0, lens0 = eng.recognize_gray(gray, 24, token_sets=half, no_repeat_ngram=2)
    ids, lens, pos = eng.recognize_gray(gray, 24, token_sets=half, no_repeat_ngram=2, positions=True)
    np.testing.assert_array_equal(ids, ids0)
    np.testing.assert_array_equal(lens, lens0)
    err = _check_fields("bf16 latent + token set + ngram 2", pos, ids, lens, 6, BF16_CXY_TOL, 40, 24)
    assert max(err[0], err[1]) <= BF16_CXY_TOL


def test_graph_count_stays_bounded_when_batches_alternate():
    """a batch of 12 rows (16 slots) without compaction replays graphs of 4, 2 (rows are leaving) or 1 (the tail) steps in one
    context bucket: three keys, and three more for the batches that record positions - however often they alternate"""
    eng = _engine("bf16", max_batch=40, flags=LATENT | NO_COMPACTION)
    gray = _gray(12)
    n0 = eng.graph_count()
    for _ in range(4):
        eng.recognize_gray(gray, 24)
        eng.recognize_gray(gray, 24, positions=True)
    assert 2 <= eng.graph_count() - n0 <= 6
