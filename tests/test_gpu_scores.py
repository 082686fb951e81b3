"""-m gpu: token scores - the log-probability of every emitted token, computed inside the LM-head launch.

Layers checked, bottom up: the scored LM-head epilogue (mocr_op_gemm_argmax_lse) and the scored token kernel
(mocr_op_dec_token_scored) against float64 numpy; that asking for scores moves no id on any decode path and that the
decode-graph cache keeps scored and unscored graphs apart; the scores of whole recognitions against the fp32 oracle's
float64 log-softmax (fp32 engine: every id identical; bf16: up to the first id divergence) and against the engine's own
teacher-forced logits; the Python surface (Recognition, MangaOcr.recognize_scored and friends).

Tolerances come from the reference side only (see each test): the GEMM term the existing kernel test grants the fused
arg-max value (1e-5 of sum |a w|), what torch's own float32 logsumexp loses against float64 on the same logits, and the
project's teacher-forced logit tolerances (1e-3 fp32, 1.4e-2 bf16) - a log-softmax moves by at most twice the largest
logit error."""
import threading

import numpy as np
import pytest

from gpu_util import bf16_round, crops, report

import score_util as su

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

D, V = 768, 6144
SENT, GUARD = -777, 2
EOS, PAD = 3, 0
FP32_LOGIT_TOL = 1e-3        # tests/test_gpu_parity.py: fp32 teacher-forced logits
BF16_LOGIT_BOUND = 1.4e-2    # tests/test_gpu_bf16_parity.py: bf16 teacher-forced logits (measured bound)
GEMM_REL = 1e-5              # tests/test_gpu_decode_kernels.py::test_fused_argmax_gemm_random_floats: |cand_val err| / sum |a w|


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _t(a, dtype):
    t = _f32(a)
    return t.to(torch.bfloat16) if dtype == "bf16" else t


# ------------------------------------------------------------------------------------------------ 1. LM-head epilogue
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("M", [1, 37, 128, 300])
def test_scored_lm_head_epilogue_against_float64(dtype, tile, M):
    """cand_val / cand_idx bit-identical to the unscored operator on the same buffers; per row
    max + log(sum_c cand_sum[c] exp(cand_val[c] - max)) against the float64 logsumexp of A(as stored) W(as stored)^T + bias.
    Row 0 spans more than 80 (an un-shifted fp32 exp would overflow); a second launch with a constant bias has a row of
    all-equal logits (A row = 0).  Tolerance per row = 2 x 1e-5 x max_j sum_k |a_k w_jk| (the GEMM term, once for the
    maximum and once for the sum) + 8 x the error of float32 torch.logsumexp on the reference logits."""
    eng = su.score_engine("wide", dtype)
    rs = np.random.RandomState(7 * M + tile)
    N, K = V, D
    Mp = (M + tile - 1) // tile * tile
    nt = N // tile
    A = np.zeros((Mp, K), np.float32)
    A[:M] = rs.standard_normal((M, K))
    A[0] *= 20.0                                                    # logits of row 0: std ~ 22, span > 80
    W = (rs.standard_normal((N, K)) * 0.05).astype(np.float32)
    if dtype == "bf16":
        A, W = bf16_round(A), bf16_round(W)
    dA, dW = _t(A, dtype), _t(W, dtype)
    worst, worst_ratio = 0.0, 0.0
    for case in ("random bias", "constant bias, zero row"):
        if case == "random bias":
            bias = rs.standard_normal(N).astype(np.float32)
            a_case, dA_case = A, dA
        else:
            bias = np.full(N, 0.75, np.float32)
            a_case = A.copy()
            a_case[M - 1] = 0.0                                     # all-equal logits
            dA_case = _t(a_case, dtype)
        logits = a_case[:M].astype(np.float64) @ W.astype(np.float64).T + bias
        if case == "random bias":
            assert logits[0].max() - logits[0].min() > 80
        else:
            assert (logits[M - 1] == 0.75).all()
        cv0 = torch.full((M + GUARD, nt), float("nan"), device="cuda")
        ci0 = torch.full((M + GUARD, nt), SENT, dtype=torch.int32, device="cuda")
        cv, ci, cs = cv0.clone(), ci0.clone(), cv0.clone()
        torch.cuda.synchronize()
        eng.op_gemm_argmax(dA_case, dW, _f32(bias), cv0, ci0, M, N, K, tile)
        eng.op_gemm_argmax_lse(dA_case, dW, _f32(bias), cv, ci, cs, M, N, K, tile)
        gv, gi, gs = cv.cpu().numpy(), ci.cpu().numpy(), cs.cpu().numpy()
        np.testing.assert_array_equal(gv.view(np.uint32), cv0.cpu().numpy().view(np.uint32), err_msg="cand_val moved")
        np.testing.assert_array_equal(gi, ci0.cpu().numpy(), err_msg="cand_idx moved")
        assert np.isnan(gs[M:]).all() and np.isnan(gv[M:]).all() and (gi[M:] == SENT).all(), "guard rows written"
        assert np.isfinite(gs[:M]).all() and (gs[:M] >= 1.0).all() and (gs[:M] <= tile * (1 + 1e-6)).all()
        got = su.merge_tiles(gv[:M], gs[:M])
        ref = su.lse64(logits)
        scale = (np.abs(a_case[:M]).astype(np.float64) @ np.abs(W).astype(np.float64).T).max(-1)
        e32 = su.f32_lse_error(logits.astype(np.float32))
        tol = 2 * GEMM_REL * scale + 8 * e32
        if case != "random bias":
            tol[M - 1] = 8 * max(e32, float(np.spacing(np.float32(ref[M - 1]))))    # no products: the fp32 format alone
        err = np.abs(got - ref)
        print(f"scored epilogue {dtype} tile={tile} M={M} {case}: max err {err.max():.3e}, tol min {tol.min():.3e}, "
              f"f32 logsumexp err {e32:.2e}", flush=True)
        worst, worst_ratio = max(worst, float(err.max())), max(worst_ratio, float((err / tol).max()))
        assert (err <= tol).all(), f"{case}: row {int(np.argmax(err / tol))} err {err.max():.3e}"
        if case != "random bias":
            assert got[M - 1] == pytest.approx(0.75 + np.log(N), abs=tol[M - 1])
    report(f"gemm EPI_ARGMAX_LSE {dtype} tile={tile} M={M}: cand_val / cand_idx bit-identical to EPI_ARGMAX; logsumexp from "
           f"(cand_val, cand_sum) max err {worst:.2e} ({worst_ratio:.3f} of tol) incl. a row spanning > 80 and an all-equal row")


# ------------------------------------------------------------------------------------------------ 2. token kernel
# fp32 evaluation of S = sum of <= 6144 positive terms exp(x), x <= 0, S >= 1: every term carries <= 4 ulp (argument
# scaling, v_exp_f32, the cand_sum product), the block-wide sum adds <= 24 sequential + 8 tree roundings, and a term's
# argument-scaling error |x| 2^-24 is weighted by exp(x) (|x| e^-|x| <= 0.37): |dS| / S <= 40 x 2^-24 = 2.4e-6, which is also
# the absolute error of log S; logf itself adds ~2 ulp of |log S| <= log(6144) = 8.7 -> 1e-6.  Bound: 5e-6.
TOKEN_SCORE_TOL = 5e-6


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("path", ["slabs1", "slabs3", "cand64", "cand128"])
def test_scored_token_step_scores_and_state(dtype, path):
    """Compaction-style (non-identity) rowmap, some rows finished: the score lands at [row][step + 1], finished rows get
    0, nothing else of the score block is written, and ids / step / finished / len / counter / next-input rows are what
    the unscored operator produces from the same inputs."""
    eng = su.score_engine("wide", dtype)
    rs = np.random.RandomState({"slabs1": 1, "slabs3": 3, "cand64": 64, "cand128": 128}[path])
    n, R, max_len, ids_ld = 20, 24, 40, 40
    lg = (np.round(rs.standard_normal((n, V)) * 3 * 256) / 1024 * 4).astype(np.float64)      # 2^-8 grid, |v| < 64
    lg[0] *= 0.0; lg[0] += 1.5                                                              # all equal: log(1 / V)
    lg[1] = np.round(np.linspace(-50, 50, V) * 256) / 256; lg[1, 4321] = 60                # span > 80
    lg[2, 777] = 40.0                                                                        # near-certain: score ~ 0
    lg[3, EOS] = 16.0                                                                        # emits EOS: scored, row finishes
    assert np.delete(lg[3], EOS).max() < 15.5
    lg = lg.astype(np.float32).astype(np.float64)
    rowmap = rs.permutation(R)[:n].astype(np.int32)
    assert (rowmap != np.arange(n)).any()
    step = rs.randint(1, max_len - 3, n).astype(np.int32)
    step[4] = max_len - 2                                                                   # reaches max_len: scored too
    finished = np.zeros(R, np.int32)
    lens = np.full(R, max_len, np.int32)
    for s in (5, 6, 7):
        finished[rowmap[s]] = 1; lens[rowmap[s]] = 9
    ids = np.full((R + 1, ids_ld), SENT, np.int32)
    kw, cand_sum = {}, None
    if path.startswith("slabs"):
        nslab = int(path[5:])
        bias = (rs.randint(-100, 100, V) / 64.0).astype(np.float64)
        parts = (rs.randint(-300, 300, (nslab, n, V)) / 64.0).astype(np.float64)
        parts[-1] = lg - bias - parts[:-1].sum(0)                    # 2^-8 grid values: every fp32 partial sum is exact
        assert (parts.astype(np.float32).astype(np.float64) == parts).all()
        kw.update(slabs=_f32(parts), nslab=nslab, vbias=_f32(bias))
    else:
        tile = int(path[4:])
        m, idx, s = su.tile_stats(lg, tile)
        cand_sum = _f32(s)
        kw.update(cand_val=_f32(m), cand_idx=_i32(idx), ncand=V // tile)
        lse_in = su.merge_tiles(m.astype(np.float32), s.astype(np.float32))        # what the kernel is given, merged in float64
    want_score = -(su.lse64(lg) - lg.max(-1))
    if not path.startswith("slabs"):
        want_score = -(lse_in - lg.max(-1))

    def run(scored):
        d = dict(ids=_i32(ids), step=_i32(step), finished=_i32(finished), len=_i32(lens), n_unfinished=_i32([11, SENT]),
                 rowmap=_i32(rowmap), x_f32=torch.full((n + GUARD, D), float("nan"), device="cuda"),
                 x_t=torch.full((n + GUARD, D), float("nan"), device="cuda", dtype=torch.bfloat16 if dtype == "bf16" else torch.float32))
        sc = torch.full((R + 1, ids_ld), float("nan"), device="cuda")
        torch.cuda.synchronize()
        if scored:
            eng.op_dec_token_scored(cand_sum, sc, first=0, n=n, ids_ld=ids_ld, max_len=max_len, n_real=n, **d, **kw)
        else:
            eng.op_dec_token(first=0, n=n, ids_ld=ids_ld, max_len=max_len, n_real=n, **d, **kw)
        out = {k: v.float().cpu().numpy() if v.dtype == torch.bfloat16 else v.cpu().numpy() for k, v in d.items()}
        return out, sc.cpu().numpy()

    plain, untouched = run(False)
    got, sc = run(True)
    assert np.isnan(untouched).all()
    for k in plain:
        np.testing.assert_array_equal(got[k], plain[k], err_msg=f"{k} differs from the unscored operator")
    written = np.zeros((R + 1, ids_ld), bool)
    written[rowmap, step + 1] = True
    assert np.isnan(sc[~written]).all(), "scores written outside [rowmap[s]][step[s] + 1]"
    val = sc[rowmap, step + 1].astype(np.float64)
    fin = finished[rowmap].astype(bool)
    assert (val[fin] == 0).all(), "finished rows score 0"
    assert plain["ids"][rowmap[3], step[3] + 1] == EOS and plain["finished"][rowmap[3]] == 1 and val[3] < 0
    assert plain["len"][rowmap[4]] == max_len and val[4] < 0
    err = np.abs(val[~fin] - want_score[~fin])
    print(f"scored token step {dtype} {path}: max err {err.max():.3e} (tol {TOKEN_SCORE_TOL:.1e}); scores {val[~fin].min():.4f} .. {val[~fin].max():.2e}", flush=True)
    assert (val <= 0).all() and np.isfinite(val).all()
    assert val[0] == pytest.approx(-np.log(V), abs=TOKEN_SCORE_TOL) and val[2] > -1e-3
    assert err.max() <= TOKEN_SCORE_TOL, f"slot {int(np.argmax(err))}: {err.max():.3e}"
    report(f"dec_token scored {dtype} {path}: scores at [rowmap[s]][step + 1] max err {err.max():.2e} (tol {TOKEN_SCORE_TOL:.0e}), finished rows 0, "
           "ids / step / finished / len / next input identical to the unscored operator")


# ------------------------------------------------------------------------------------------------ 3. ids do not move
CLASSIC, LATENT, FP8, NO_FUSED, NO_GRAPH = 8, 64, 64 | 128, 16, 2
IDS_CASES = [("fp32", 0), ("fp32", NO_FUSED), ("fp32", NO_GRAPH),
             ("bf16", 0), ("bf16", CLASSIC), ("bf16", LATENT), ("bf16", FP8), ("bf16", NO_FUSED), ("bf16", NO_GRAPH)]


@pytest.mark.parametrize("dtype,flags", IDS_CASES)
def test_asking_for_scores_moves_no_id(dtype, flags):
    """Early-EOS weights (batches compact), rows 3 / 40 / 300 on one engine, calls interleaved unscored - scored - unscored
    (3 and 300 rows) and scored - unscored - scored (40 rows): a decode graph captured for one kind must not be replayed
    for the other, and the ids and lengths of every call of a row count are identical."""
    eng = su.score_engine("eos", dtype, max_batch=320, flags=flags)
    for rows in (3, 40, 300):
        gray = np.concatenate([crops(4321, 6), crops(4322, rows)])[:rows]
        order = [True, False, True] if rows == 40 else [False, True, False]
        outs = []
        for scored in order:
            out = eng.recognize_gray(gray, 120, scores=scored)
            assert len(out) == (3 if scored else 2)
            outs.append(out)
        ids0, lens0 = outs[0][0], outs[0][1]
        for out in outs[1:]:
            np.testing.assert_array_equal(out[0], ids0, err_msg=f"{rows} rows: ids moved")
            np.testing.assert_array_equal(out[1], lens0, err_msg=f"{rows} rows: lengths moved")
        logps = [o[2] for o in outs if len(o) == 3]
        for lp in logps:
            _check_layout(ids0, lens0, lp)
            np.testing.assert_array_equal(lp, logps[0], err_msg="scores of two identical scored calls differ")
        assert lens0.min() < lens0.max() or rows == 3
    report(f"{dtype} flags {flags}: scored ids / lengths array_equal to unscored at 3 / 40 / 300 rows (early-EOS weights, interleaved calls), "
           f"{eng.graph_count()} decode graphs")


def _check_layout(ids, lens, logp):
    """column 0 is 0, the pad tail is 0, every score <= 0, every generated position (EOS included) is scored"""
    assert logp.dtype == np.float32 and logp.shape == ids.shape
    assert np.isfinite(logp).all() and (logp <= 0).all()
    assert (logp[:, 0] == 0).all()
    for b in range(len(lens)):
        assert (logp[b, lens[b]:] == 0).all(), f"row {b}: pad tail scored"
        assert (logp[b, 1:lens[b]] < 0).all(), f"row {b}: a generated token without a score"


# ------------------------------------------------------------------------------------------------ 4. fp32 end to end
@pytest.mark.parametrize("kind,max_len,n", [("wide", 32, 8), ("peaked", 32, 8), ("eos", 120, 6)])
def test_fp32_scores_against_the_oracle(kind, max_len, n):
    """fp32 engine vs the fp32 oracle's logits in float64: all ids identical (as the existing fp32 tests hold), every score
    within 2 x the fp32 teacher-forced logit tolerance (1e-3) of log_softmax(logits)[id]."""
    seed = 4321 if kind == "eos" else 11
    ids_o, logits = su.oracle_run(kind, seed, n, max_len)
    eng = su.score_engine(kind, "fp32")
    ids, lens, logp = eng.recognize_gray(crops(seed, n), max_len, scores=True)
    L = ids_o.shape[1]
    np.testing.assert_array_equal(ids[:, :L], ids_o, err_msg="fp32 ids differ from the oracle's")
    assert (ids[:, L:] == PAD).all()
    _check_layout(ids, lens, logp)
    ref = su.chosen_logp64(logits, ids_o)
    worst, cnt = 0.0, 0
    for b in range(n):
        k = lens[b] - 1                                           # generated tokens of row b, EOS included
        d = np.abs(logp[b, 1:lens[b]].astype(np.float64) - ref[b, :k])
        worst, cnt = max(worst, float(d.max())), cnt + k
        if ids[b, lens[b] - 1] == EOS:
            assert logp[b, lens[b] - 1] < 0, "EOS position not scored"
    if kind == "eos":
        assert lens.min() < lens.max() and (ids[np.arange(n), lens - 1] == EOS).any()
    print(f"fp32 scores vs oracle ({kind}): max |logp - ref| {worst:.3e} over {cnt} tokens", flush=True)
    report(f"token scores fp32 vs oracle float64 log-softmax, {kind} weights, {n} crops, max_len {max_len}: ids identical, "
           f"max |logp - ref| {worst:.2e} over {cnt} tokens (bound {2 * FP32_LOGIT_TOL:.0e}); scores {ref.min():.3f} .. {ref.max():.3f}")
    assert worst <= 2 * FP32_LOGIT_TOL


# ------------------------------------------------------------------------------------------------ 5. bf16 end to end
@pytest.mark.parametrize("kind", ["wide", "peaked"])
@pytest.mark.parametrize("rows", [8, 64, 300])
def test_bf16_scores_self_consistent_and_against_the_oracle(kind, rows):
    """bf16 engine, automatic kernel choice: 8 rows (small-batch path), 64 (classic), 300 (latent), max_len 32.
    (a) against the float64 log-softmax of the engine's OWN teacher-forced logits for the ids it just generated: these differ
        by summation order (split-K slabs against the unsplit fused LM head) and exp precision only; tolerance = the rule of
        the epilogue test with the GEMM term applied twice more for the second, differently ordered sum of the same products
        (the split-K allowance): 4 x 1e-5 x an upper bound of sum |a w| from the weights + 8 x the float32 logsumexp error
        measured on the teacher-forced logits.
    (b) widened-margin weights, rows 0..7 (the oracle runs on the CPU) against the oracle on the positions strictly before
        each row's first id divergence: <= 2 x 1.4e-2; at least 75 % of the generated positions must be compared."""
    max_len = 32
    eng = su.score_engine(kind, "bf16", max_batch=320)
    gray = np.concatenate([crops(11, 8), crops(12, rows)])[:rows]
    ids, lens, logp = eng.recognize_gray(gray, max_len, scores=True)
    ids_u, lens_u = eng.recognize_gray(gray, max_len)
    np.testing.assert_array_equal(ids, ids_u)
    np.testing.assert_array_equal(lens, lens_u)
    _check_layout(ids, lens, logp)
    # (a)
    dg = torch.from_numpy(gray).cuda()
    torch.cuda.synchronize()
    T = max_len - 1
    own = eng.decode_logits(dg, rows, ids[:, :T])                  # [rows, T, V]: step t chose ids[:, t + 1]
    assert np.isfinite(own).all()
    ref_own = su.chosen_logp64(own, ids)
    e32 = su.f32_lse_error(own.reshape(-1, V)[:: max(1, rows // 8)])
    scale = su.lm_head_scale(su.score_weights(kind))
    tol_a = 4 * GEMM_REL * scale + 8 * e32
    worst_a, n_pos, top1 = 0.0, 0, 0
    for b in range(rows):
        k = lens[b] - 1
        worst_a = max(worst_a, float(np.abs(logp[b, 1:lens[b]].astype(np.float64) - ref_own[b, :k]).max()))
        top1 += int((own[b, :k].argmax(-1) == ids[b, 1:lens[b]]).sum())
        n_pos += k
    print(f"bf16 scores ({kind}, {rows} rows) vs own teacher-forced logits: max diff {worst_a:.3e}, tol {tol_a:.3e} "
          f"(sum |a w| bound {scale:.1f}, f32 logsumexp err {e32:.2e}); arg-max of the teacher-forced logits = emitted id at {top1}/{n_pos}", flush=True)
    report(f"token scores bf16 {kind} weights, {rows} rows: vs float64 log-softmax of the engine's own teacher-forced logits max diff "
           f"{worst_a:.2e} (tol {tol_a:.2e}) over {n_pos} tokens")
    assert worst_a <= tol_a
    # (b)
    if kind != "wide":
        return
    ids_o, logits_o = su.oracle_run("wide", 11, 8, max_len)
    ref = su.chosen_logp64(logits_o, ids_o)
    worst_b, compared, total = 0.0, 0, 0
    for b in range(8):
        k = lens[b] - 1
        neq = np.nonzero(ids[b, 1:lens[b]] != ids_o[b, 1:lens[b]])[0]
        upto = int(neq[0]) if neq.size else k                      # generated positions strictly before the first divergence
        total += k
        compared += upto
        if upto:
            worst_b = max(worst_b, float(np.abs(logp[b, 1:1 + upto].astype(np.float64) - ref[b, :upto]).max()))
    frac = compared / total
    print(f"bf16 scores (wide, {rows} rows, rows 0..7) vs oracle: max |logp - ref| {worst_b:.3e} on {compared}/{total} positions", flush=True)
    report(f"token scores bf16 wide weights, {rows} rows (rows 0..7 checked) vs oracle float64 log-softmax: max |logp - ref| {worst_b:.2e} "
           f"(bound {2 * BF16_LOGIT_BOUND:.1e}) on {compared}/{total} positions before the first id divergence ({100 * frac:.0f} %)")
    assert frac >= 0.75, f"only {100 * frac:.0f} % of the generated positions precede a divergence"
    assert worst_b <= 2 * BF16_LOGIT_BOUND


# ------------------------------------------------------------------------------------------------ 6. product surface
def test_product_surface_scored_calls():
    from PIL import Image
    from manga_ocr import MangaOcr
    from manga_ocr.ocr import Recognition
    m = MangaOcr(synthetic_seed=1, dtype="fp32", max_batch=8, lanes=1)
    try:
        m.engine.set_generate_max_length(24)
        rs = np.random.RandomState(5)
        imgs = [Image.fromarray(rs.randint(0, 256, (40 + 7 * i, 60 + 5 * i, 3), dtype=np.uint8), "RGB") for i in range(8)]
        texts = [m(im) for im in imgs]
        for im, t in zip(imgs, texts):
            r = m.recognize_scored(im)
            assert isinstance(r, Recognition) and r.text == t
            assert r.logprobs.shape == (len(r.ids) - 1,) and (r.logprobs < 0).all()
            assert r.confidence == pytest.approx(float(np.exp(r.logprobs.astype(np.float64).mean())), rel=1e-12)
            assert r.min_prob == pytest.approx(float(np.exp(r.logprobs.astype(np.float64).min())), rel=1e-12)
            assert 0 < r.min_prob <= r.confidence <= 1
        batch = m.recognize_batch_scored(imgs)
        assert [r.text for r in batch] == texts == m.recognize_batch(imgs)
        bgr = [np.asarray(im)[:, :, ::-1] for im in imgs]
        assert [r.text for r in m.recognize_bgr_scored(bgr)] == m.recognize_bgr(bgr) == texts
        # regions: a sliver gives '' and confidence 0.0
        page = rs.randint(0, 256, (300, 400, 3), dtype=np.uint8)
        regs = [(0, 10, 20, 100, 60), (0, 0, 0, 1, 1), (0, 200, 100, 80, 120)]
        rr = m.recognize_regions_scored([page], regs)
        assert [r.text for r in rr] == m.recognize_regions([page], regs)
        assert rr[1].text == "" and rr[1].confidence == 0.0 and rr[1].ids.size == 0
        assert rr[0].confidence > 0 and rr[2].confidence > 0
        # eight threads mixing __call__ and recognize_scored on one instance
        out = [None] * 8
        def work(i):
            out[i] = m.recognize_scored(imgs[i]) if i % 2 else m(imgs[i])
        th = [threading.Thread(target=work, args=(i,)) for i in range(8)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for i in range(8):
            if i % 2:
                assert isinstance(out[i], Recognition) and out[i].text == texts[i]
                np.testing.assert_allclose(out[i].logprobs, batch[i].logprobs, rtol=0, atol=2 * FP32_LOGIT_TOL)
            else:
                assert isinstance(out[i], str) and out[i] == texts[i]
        report("MangaOcr scored surface: recognize_scored / _batch_scored / _bgr_scored / _regions_scored texts == unscored texts, "
               "confidence == exp(mean logprobs), sliver -> ('', 0.0), 8 mixed threads consistent")
    finally:
        m.close()
