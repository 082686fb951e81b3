"""-m gpu: token alternatives - the four most probable tokens of every position, from the fused LM head.

Layers checked, bottom up: the LM-head epilogue that keeps four candidates per tile (mocr_op_gemm_topk) and the token kernel
that merges them (mocr_op_dec_token_topk) against float64 numpy, with exact-arithmetic inputs for the order and its tie
rule; that asking for alternatives moves no id, no length and no score on any decode path and that the decode-graph cache
keeps the three kinds of step apart; whole recognitions against the fp32 oracle (fp32 engine) and against the engine's own
teacher-forced logits (bf16 engine); the Python surface.

The order everywhere: logit descending, equal logits the lower id first - numpy's stable argsort of the negated values.
Tolerances come from the reference side only and are the ones the token-score tests use (tests/test_gpu_scores.py)."""
import threading

import numpy as np
import pytest

from gpu_util import bf16_round, crops, report

import score_util as su

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

D, V, K4 = 768, 6144, 4
SENT, GUARD = -777, 2
EOS, PAD = 3, 0
FP32_LOGIT_TOL = 1e-3        # tests/test_gpu_parity.py: fp32 teacher-forced logits
GEMM_REL = 1e-5              # tests/test_gpu_decode_kernels.py::test_fused_argmax_gemm_random_floats: |cand_val err| / sum |a w|
TOKEN_SCORE_TOL = 5e-6       # tests/test_gpu_scores.py: the fp32 evaluation of log(sum exp(x - max)) over <= 6144 terms
NO_IDX = 0x7FFFFFFF


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _t(a, dtype):
    t = _f32(a)
    return t.to(torch.bfloat16) if dtype == "bf16" else t


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lex_top(x, k=K4):
    """[..., n] -> columns [..., k] of the k largest values, value descending, the lower column first among equal values"""
    return np.argsort(-np.asarray(x), axis=-1, kind="stable")[..., :k]


def lex_top_sparse(x, k):
    """lex_top for long rows: the 16 largest by partition, then the stable order among those (more than 16 - k equal
    values at the top of a row do not occur in the logits this is used on)"""
    x = np.asarray(x)
    out = np.empty(x.shape[:-1] + (k,), np.int64)
    for lo in range(0, x.shape[0], 1024):                                          # (bounded temporaries: x may hold 9000 rows)
        c = x[lo:lo + 1024]
        cand = np.sort(np.argpartition(-c, 16, axis=-1)[..., :16], axis=-1)        # ascending columns: the stable sort keeps them so
        order = np.argsort(-np.take_along_axis(c, cand, -1), axis=-1, kind="stable")[..., :k]
        out[lo:lo + 1024] = np.take_along_axis(cand, order, -1)
    return out


# ------------------------------------------------------------------------------------------------ 1. LM-head epilogue
def _run_topk(eng, dA, dW, bias, M, N, K, tile):
    """the three operators on the same inputs, guard rows behind every output"""
    nt = N // tile
    nan2 = lambda: torch.full((M + GUARD, nt), float("nan"), device="cuda")
    sent2 = lambda: torch.full((M + GUARD, nt), SENT, dtype=torch.int32, device="cuda")
    cv0, ci0 = nan2(), sent2()
    cv1, ci1, cs1 = nan2(), sent2(), nan2()
    cv, ci, cs = nan2(), sent2(), nan2()
    tv = torch.full((M + GUARD, nt, K4), float("nan"), device="cuda")
    ti = torch.full((M + GUARD, nt, K4), SENT, dtype=torch.int32, device="cuda")
    db = _f32(bias)
    torch.cuda.synchronize()
    eng.op_gemm_argmax(dA, dW, db, cv0, ci0, M, N, K, tile)
    eng.op_gemm_argmax_lse(dA, dW, db, cv1, ci1, cs1, M, N, K, tile)
    eng.op_gemm_topk(dA, dW, db, cv, ci, cs, tv, ti, M, N, K, tile)
    gv, gi, gs, gtv, gti = (x.cpu().numpy() for x in (cv, ci, cs, tv, ti))
    np.testing.assert_array_equal(_bits(gv), _bits(cv0.cpu().numpy()), err_msg="cand_val differs from mocr_op_gemm_argmax")
    np.testing.assert_array_equal(gi, ci0.cpu().numpy(), err_msg="cand_idx differs from mocr_op_gemm_argmax")
    np.testing.assert_array_equal(_bits(gs), _bits(cs1.cpu().numpy()), err_msg="cand_sum differs from mocr_op_gemm_argmax_lse")
    np.testing.assert_array_equal(_bits(gv), _bits(cv1.cpu().numpy()))
    np.testing.assert_array_equal(gi, ci1.cpu().numpy())
    np.testing.assert_array_equal(_bits(gtv[..., 0]), _bits(gv), err_msg="top_val[..., 0] is not cand_val")
    np.testing.assert_array_equal(gti[..., 0], gi, err_msg="top_idx[..., 0] is not cand_idx")
    assert np.isnan(gv[M:]).all() and (gi[M:] == SENT).all() and np.isnan(gs[M:]).all(), "guard rows of the candidates written"
    assert np.isnan(gtv[M:]).all() and (gti[M:] == SENT).all(), "guard rows of top_val / top_idx written"
    return gtv[:M], gti[:M]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("M", [1, 37, 300])
def test_topk_lm_head_epilogue_against_float64(dtype, tile, M):
    """mocr_op_gemm_topk, N 6144, K 768.  The candidate arrays are bit-identical to the two existing operators' and entry 0 of
    the lists equals them; guard rows untouched (every launch).
    Random floats: every top_val[k] within 1e-5 x max sum |a w| of the float64 logit at top_idx[k] and of the float64 k-th
    largest of the tile; columns inside the tile and distinct; values non-increasing.
    Exact arithmetic (A in {-1, 0, 1}, W in {-1, 0, 1}, integer bias: every sum exact in fp32, ties everywhere): top_idx and
    top_val equal numpy's lexicographic top four exactly - with a random bias, with a constant bias and a zero row (a row
    of all-equal logits: every tile's four best are equal), and with spikes on that row (a tile whose four best are equal
    and apart, and a tile with five equal maxima)."""
    eng = su.score_engine("wide", dtype)
    rs = np.random.RandomState(11 * M + tile)
    N, K = V, D
    Mp = (M + tile - 1) // tile * tile
    nt = N // tile
    tile_lo = (np.arange(nt) * tile)[None, :, None]
    # ---- random floats
    A = np.zeros((Mp, K), np.float32)
    A[:M] = rs.standard_normal((M, K))
    W = (rs.standard_normal((N, K)) * 0.05).astype(np.float32)
    bias = rs.standard_normal(N).astype(np.float32)
    if dtype == "bf16":
        A, W = bf16_round(A), bf16_round(W)
    dW = _t(W, dtype)
    tv, ti = _run_topk(eng, _t(A, dtype), dW, bias, M, N, K, tile)
    logits = A[:M].astype(np.float64) @ W.astype(np.float64).T + bias
    allow = GEMM_REL * (np.abs(A[:M]).astype(np.float64) @ np.abs(W).astype(np.float64).T).max()
    assert ((ti >= tile_lo) & (ti < tile_lo + tile)).all(), "a column outside its tile"
    srt = np.sort(ti, -1)
    assert (srt[..., 1:] != srt[..., :-1]).all(), "a column twice in one list"
    assert np.isfinite(tv).all() and (tv[..., 1:] <= tv[..., :-1]).all(), "values increase along a list"
    at = np.take_along_axis(logits, ti.reshape(M, -1).astype(np.int64), -1).reshape(M, nt, K4)
    e_at = float(np.abs(tv - at).max())
    kth = -np.sort(-logits.reshape(M, nt, tile), -1)[..., :K4]
    e_kth = float(np.abs(tv - kth).max())
    print(f"topk epilogue {dtype} tile={tile} M={M} random: |top_val - logit[top_idx]| {e_at:.3e}, |top_val - k-th largest| {e_kth:.3e}, "
          f"allowance {allow:.3e}", flush=True)
    assert e_at <= allow and e_kth <= allow
    # ---- exact arithmetic
    Ai = np.zeros((Mp, K), np.float32)
    Ai[:M] = rs.choice([-1.0, 0.0, 1.0], size=(M, K), p=[0.05, 0.9, 0.05])
    Wi = rs.randint(-1, 2, size=(N, K)).astype(np.float32)
    dWi = _t(Wi, dtype)
    Az = Ai.copy()
    Az[M - 1] = 0.0
    spikes = np.full(N, 1.0, np.float32)
    t1, t2 = 1 * tile, 2 * tile
    spikes[[t1 + 5, t1 + tile // 2 - 1, t1 + tile // 2 + 2, t1 + tile - 1]] = 9.0                 # four equal, in every thread's share of the row
    spikes[[t2 + tile - 2, t2 + 3, t2 + tile // 4, t2 + tile // 2, t2 + 3 * tile // 4 + 1]] = 7.0   # five equal: the lowest four
    n_ties = 0
    for case, a_case, b_case in (("random bias", Ai, rs.randint(-3, 4, size=N).astype(np.float32)),
                                 ("constant bias, zero row", Az, np.full(N, 2.0, np.float32)),
                                 ("spikes, zero row", Az, spikes)):
        tv, ti = _run_topk(eng, _t(a_case, dtype), dWi, b_case, M, N, K, tile)
        lg = a_case[:M].astype(np.float64) @ Wi.astype(np.float64).T + b_case
        assert (lg == lg.astype(np.float32)).all() and np.abs(lg).max() < 2 ** 20
        t3 = lg.reshape(M, nt, tile)
        want_i = lex_top(t3) + tile_lo
        want_v = np.take_along_axis(t3, want_i - tile_lo, -1)
        n_ties += int((want_v[..., 1:] == want_v[..., :-1]).sum())
        np.testing.assert_array_equal(ti, want_i, err_msg=f"{case}: top_idx is not the lexicographic top four")
        np.testing.assert_array_equal(tv.astype(np.float64), want_v, err_msg=f"{case}: top_val")
        if case == "constant bias, zero row":
            assert (lg[M - 1] == 2.0).all()
            np.testing.assert_array_equal(ti[M - 1], tile_lo[0] + np.arange(K4))
        if case == "spikes, zero row":
            np.testing.assert_array_equal(ti[M - 1, 1], [t1 + 5, t1 + tile // 2 - 1, t1 + tile // 2 + 2, t1 + tile - 1])
            np.testing.assert_array_equal(ti[M - 1, 2], [t2 + 3, t2 + tile // 4, t2 + tile // 2, t2 + 3 * tile // 4 + 1])
            assert (tv[M - 1, 1] == 9.0).all() and (tv[M - 1, 2] == 7.0).all()
    assert n_ties > M * nt // 4, "the exact-arithmetic inputs were meant to tie"
    report(f"gemm EPI_TOPK {dtype} tile={tile} M={M}: cand_val / cand_idx / cand_sum bit-identical to EPI_ARGMAX / EPI_ARGMAX_LSE, entry 0 = "
           f"the candidate; random floats |top_val - logit[top_idx]| {e_at:.2e}, |top_val - k-th largest| {e_kth:.2e} (allowance {allow:.2e}); "
           f"exact inputs: top_idx == lexicographic top four incl. {n_ties} ties, an all-equal row, 4 and 5 equal maxima in a tile")


# ------------------------------------------------------------------------------------------------ 2. token kernel
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("path", ["cand64", "cand128", "slabs1", "slabs3"])
def test_topk_token_step_against_float64(dtype, path):
    """mocr_op_dec_token_topk: the inputs are the fp32 logits themselves (2^-8 grid), so the order is exact and alt_ids must
    equal numpy's lexicographic top four of the row; alt_logp within 5e-6 + 2^-23 |ref| of the float64 log-softmax (the
    token-score bound plus the one rounding of val_k - max); entry 0 bit-identical to mocr_op_dec_token_scored's score;
    every state array identical to the scored operator's; the finished row reads -1 / 0; nothing else is written.
    Slots: 0 all four winners in one tile, 1 winners in four tiles, 2 five equal maxima in five tiles, 3 six equal maxima
    spread over the four waves' columns (slab path: thread t holds columns 4 t + 1024 j .. + 3) and over tiles 64 columns
    and 64 tiles apart (candidate path: thread c holds tile c), 4 two equal pairs that interleave, 5 an all-equal row,
    6 finished; the rest random."""
    eng = su.score_engine("wide", dtype)
    rs = np.random.RandomState({"slabs1": 11, "slabs3": 13, "cand64": 164, "cand128": 228}[path])
    n, R, max_len, ids_ld = 10, 13, 40, 40
    lg = (np.round(rs.standard_normal((n, V)) * 3 * 256) / 256).astype(np.float64)          # 2^-8 grid, |v| < 20
    assert np.abs(lg).max() < 20
    lg[0, [133, 130, 150, 129]] = [50, 49, 48, 47]
    lg[1, [6000, 5, 3000, 1000]] = [44, 43, 42, 41]
    lg[2, [10, 200, 4000, 5000, 6100]] = 40
    lg[3, [3, 263, 513, 770, 4101, 2000]] = 30
    lg[4, [6000, 900]] = 30; lg[4, [5, 4101, 300]] = 29
    lg[5] = 1.5
    lg = lg.astype(np.float32).astype(np.float64)
    want_ids = lex_top(lg)
    np.testing.assert_array_equal(want_ids[:6], [[133, 130, 150, 129], [6000, 5, 3000, 1000], [10, 200, 4000, 5000], [3, 263, 513, 770],
                                                 [900, 6000, 5, 300], [0, 1, 2, 3]])
    want_lp = np.take_along_axis(su.log_softmax64(lg), want_ids, -1)
    rowmap = rs.permutation(R)[:n].astype(np.int32)
    assert (rowmap != np.arange(n)).any()
    step = rs.randint(1, max_len - 3, n).astype(np.int32)
    finished = np.zeros(R, np.int32)
    lens = np.full(R, max_len, np.int32)
    finished[rowmap[6]] = 1; lens[rowmap[6]] = 9
    ids = np.full((R + 1, ids_ld), SENT, np.int32)
    kw, cand_sum, top_val, top_idx = {}, None, None, None
    if path.startswith("slabs"):
        nslab = int(path[5:])
        bias = (rs.randint(-100, 100, V) / 64.0).astype(np.float64)
        parts = (rs.randint(-300, 300, (nslab, n, V)) / 64.0).astype(np.float64)
        parts[-1] = lg - bias - parts[:-1].sum(0)                    # 2^-8 grid values: every fp32 partial sum is exact
        assert (parts.astype(np.float32).astype(np.float64) == parts).all()
        kw.update(slabs=_f32(parts), nslab=nslab, vbias=_f32(bias))
    else:
        tile = int(path[4:])
        nt = V // tile
        m, idx, s = su.tile_stats(lg, tile)
        t3 = lg.reshape(n, nt, tile)
        ti = lex_top(t3)
        cand_sum, top_val = _f32(s), _f32(np.take_along_axis(t3, ti, -1))
        top_idx = _i32(ti + (np.arange(nt) * tile)[None, :, None])
        kw.update(cand_val=_f32(m), cand_idx=_i32(idx), ncand=nt)

    def run(topk):
        d = dict(ids=_i32(ids), step=_i32(step), finished=_i32(finished), len=_i32(lens), n_unfinished=_i32([11, SENT]),
                 rowmap=_i32(rowmap), x_f32=torch.full((n + GUARD, D), float("nan"), device="cuda"),
                 x_t=torch.full((n + GUARD, D), float("nan"), device="cuda", dtype=torch.bfloat16 if dtype == "bf16" else torch.float32))
        sc = torch.full((R + 1, ids_ld), float("nan"), device="cuda")
        ai = torch.full((R + 1, ids_ld, K4), SENT, dtype=torch.int32, device="cuda")
        al = torch.full((R + 1, ids_ld, K4), float("nan"), device="cuda")
        torch.cuda.synchronize()
        if topk:
            eng.op_dec_token_topk(cand_sum, sc, top_val, top_idx, ai, al, first=0, n=n, ids_ld=ids_ld, max_len=max_len, n_real=n, **d, **kw)
        else:
            eng.op_dec_token_scored(cand_sum, sc, first=0, n=n, ids_ld=ids_ld, max_len=max_len, n_real=n, **d, **kw)
        out = {k: v.float().cpu().numpy() if v.dtype == torch.bfloat16 else v.cpu().numpy() for k, v in d.items()}
        return out, sc.cpu().numpy(), ai.cpu().numpy(), al.cpu().numpy()

    scored, sc0, ai0, al0 = run(False)
    assert (ai0 == SENT).all() and np.isnan(al0).all()
    got, sc, ai, al = run(True)
    for k in scored:
        np.testing.assert_array_equal(got[k], scored[k], err_msg=f"{k} differs from the scored operator")
    np.testing.assert_array_equal(_bits(sc), _bits(sc0), err_msg="scores differ from the scored operator")
    written = np.zeros((R + 1, ids_ld), bool)
    written[rowmap, step + 1] = True
    assert (ai[~written] == SENT).all() and np.isnan(al[~written]).all(), "alternatives written outside [rowmap[s]][step[s] + 1]"
    gi, gl = ai[rowmap, step + 1], al[rowmap, step + 1]
    live = np.arange(n) != 6
    assert (gi[6] == -1).all() and (gl[6] == 0).all() and sc[rowmap[6], step[6] + 1] == 0, "the finished row reads -1 / 0"
    np.testing.assert_array_equal(gi[live], want_ids[live], err_msg="alt_ids is not the lexicographic top four")
    np.testing.assert_array_equal(gi[live, 0], got["ids"][rowmap, step + 1][live])
    np.testing.assert_array_equal(_bits(gl[live, 0]), _bits(sc[rowmap, step + 1][live]), err_msg="entry 0 is not the score, bit for bit")
    tol = TOKEN_SCORE_TOL + 2.0 ** -23 * np.abs(want_lp)
    err = np.abs(gl.astype(np.float64) - want_lp)
    print(f"topk token step {dtype} {path}: max |alt_logp - ref| {err[live].max():.3e} (tol >= {TOKEN_SCORE_TOL:.1e}), "
          f"alt_logp {gl[live].min():.3f} .. {gl[live].max():.2e}", flush=True)
    assert (err[live] <= tol[live]).all(), f"slot {int(np.argmax((err / tol)[live].max(-1)))}: {err[live].max():.3e}"
    assert (gl[live][:, 1:] <= gl[live][:, :-1]).all()
    assert np.abs(gl[5] + np.log(V)).max() <= TOKEN_SCORE_TOL + 2.0 ** -23 * np.log(V)
    report(f"dec_token topk {dtype} {path}: alt_ids == lexicographic top four (one tile, four tiles, ties across tiles and waves, all-equal row), "
           f"alt_logp max err {err[live].max():.2e} (tol 5e-6 + 2^-23 |ref|), entry 0 bit-identical to the score, state identical to the scored "
           "operator, finished row -1 / 0, nothing else written")


# ------------------------------------------------------------------------------------------------ 3. ids do not move
CLASSIC, LATENT, FP8, NO_FUSED, NO_GRAPH = 8, 64, 64 | 128, 16, 2
IDS_CASES = [("fp32", 0), ("fp32", NO_FUSED), ("fp32", NO_GRAPH),
             ("bf16", 0), ("bf16", CLASSIC), ("bf16", LATENT), ("bf16", FP8), ("bf16", NO_FUSED), ("bf16", NO_GRAPH)]
ORDERS = {3: (0, 2, 1, 2), 40: (2, 0, 2, 1), 300: (1, 2, 0, 2)}          # 0 unscored, 1 scored, 2 scored with alternatives


def _call(eng, gray, max_len, kind):
    out = eng.recognize_gray(gray, max_len) if kind == 0 else eng.recognize_gray(gray, max_len, scores=True) if kind == 1 else \
        eng.recognize_gray(gray, max_len, alternatives=True)
    assert len(out) == (2, 3, 5)[kind]
    return out


def _check_alt_layout(ids, lens, logp, alt_ids, alt_logp):
    """position 0 and the pad tail read -1 / 0; a generated position holds four distinct ids of the vocabulary, entry 0 the
    emitted one with the score's very bits, log-probabilities <= 0 and non-increasing"""
    assert alt_ids.dtype == np.int32 and alt_logp.dtype == np.float32
    assert alt_ids.shape == ids.shape + (K4,) and alt_logp.shape == ids.shape + (K4,)
    gen = (np.arange(ids.shape[1])[None, :] >= 1) & (np.arange(ids.shape[1])[None, :] < lens[:, None])
    assert (alt_ids[~gen] == -1).all() and (alt_logp[~gen] == 0).all(), "position 0 / the pad tail is not -1 / 0"
    gi, gl = alt_ids[gen], alt_logp[gen]
    assert ((gi >= 0) & (gi < V)).all()
    np.testing.assert_array_equal(gi[:, 0], ids[gen], err_msg="entry 0 is not the emitted id")
    np.testing.assert_array_equal(_bits(gl[:, 0]), _bits(logp[gen]), err_msg="entry 0 is not the score, bit for bit")
    srt = np.sort(gi, -1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "an id twice at one position"
    assert np.isfinite(gl).all() and (gl <= 0).all() and (gl[:, 1:] <= gl[:, :-1]).all()


@pytest.mark.parametrize("dtype,flags", IDS_CASES)
def test_asking_for_alternatives_moves_no_id(dtype, flags):
    """The flag matrix of test_asking_for_scores_moves_no_id: early-EOS weights (batches compact), 3 / 40 / 300 rows on one
    engine, the three kinds of call interleaved.  ids and lengths array_equal across kinds, logp array_equal between the
    scored and the alternatives call, two alternatives calls identical; repeating every kind captures no further graph."""
    eng = su.score_engine("eos", dtype, max_batch=320, flags=flags)
    grays = {rows: np.concatenate([crops(4321, 6), crops(4322, rows)])[:rows] for rows in ORDERS}
    for rows, order in ORDERS.items():
        outs = [(kind, _call(eng, grays[rows], 120, kind)) for kind in order]
        ids0, lens0 = outs[0][1][0], outs[0][1][1]
        for kind, out in outs[1:]:
            np.testing.assert_array_equal(out[0], ids0, err_msg=f"{rows} rows, kind {kind}: ids moved")
            np.testing.assert_array_equal(out[1], lens0, err_msg=f"{rows} rows, kind {kind}: lengths moved")
        logp1 = [o[2] for k, o in outs if k == 1][0]
        alts = [o for k, o in outs if k == 2]
        for o in alts:
            np.testing.assert_array_equal(_bits(o[2]), _bits(logp1), err_msg=f"{rows} rows: logp differs between the scored and the alternatives call")
            _check_alt_layout(ids0, lens0, o[2], o[3], o[4])
        np.testing.assert_array_equal(alts[0][3], alts[1][3], err_msg="alt_ids of two identical calls differ")
        np.testing.assert_array_equal(_bits(alts[0][4]), _bits(alts[1][4]), err_msg="alt_logp of two identical calls differ")
        assert lens0.min() < lens0.max() or rows == 3
    graphs = eng.graph_count()
    for rows, order in ORDERS.items():
        for kind in sorted(set(order)):
            _call(eng, grays[rows], 120, kind)
    assert eng.graph_count() == graphs, "a repeated call captured another decode graph"
    assert (graphs == 0) == bool(flags & NO_GRAPH)
    report(f"{dtype} flags {flags}: ids / lengths array_equal across unscored / scored / alternatives calls at 3 / 40 / 300 rows (early-EOS "
           f"weights, interleaved), logp array_equal scored vs alternatives, {graphs} decode graphs, none added by repeats")


# ------------------------------------------------------------------------------------------------ 4. / 5. end to end
def _rank_reference(logits, ids, lens):
    """logits float32 [B, T, V] of steps 0 .. T-1 (step t chose ids[:, t + 1]) -> for the generated positions, in row order:
    (row, position), the reference's five best ids [P, 5], their float64 log-probabilities [P, 5], and a function giving the
    float64 log-probability of any ids [P, 4] at those positions"""
    B, T, _ = logits.shape
    where = [(b, t) for b in range(B) for t in range(1, min(int(lens[b]), T + 1))]
    bb, tt = np.array([w[0] for w in where]), np.array([w[1] for w in where])
    x = np.ascontiguousarray(logits[bb, tt - 1], np.float32)     # [P, V]; the float32 values are the reference's inputs
    lse = np.concatenate([su.lse64(x[lo:lo + 1024]) for lo in range(0, len(x), 1024)])
    top5 = lex_top_sparse(x, 5)
    lp_at = lambda idx: np.take_along_axis(x, idx.astype(np.int64), -1).astype(np.float64) - lse[:, None]
    return bb, tt, top5, lp_at(top5), lp_at


def _compare_ranks(alt_ids, alt_logp, bb, tt, top5, lp5, lp_at, tol, gap_tol):
    """-> (max |alt_logp - reference log-softmax at alt_ids|, max |alt_logp[k] - reference k-th largest|, (position, rank)
    pairs whose bordering reference gaps all exceed gap_tol, how many of those have the reference's id)"""
    gi, gl = alt_ids[bb, tt], alt_logp[bb, tt].astype(np.float64)
    e_at = float(np.abs(gl - lp_at(gi)).max())
    e_kth = float(np.abs(gl - lp5[:, :K4]).max())
    gaps = lp5[:, :-1] - lp5[:, 1:]                              # [P, 4]: gap below rank k
    clear = gaps > gap_tol
    clear[:, 1:] &= gaps[:, :-1] > gap_tol                       # ... and the gap above it
    same = gi == top5[:, :K4]
    return e_at, e_kth, clear, int((same & clear).sum())


@pytest.mark.parametrize("kind", ["wide", "peaked"])
def test_fp32_alternatives_against_the_oracle(kind):
    """fp32 engine vs the fp32 oracle's logits in float64, 8 crops, max_len 32: all ids identical; with tol = 2 x 1e-3 (the
    project's fp32 logit tolerance, twice: a log-softmax moves by at most twice the largest logit error) every alt_logp[k]
    within tol of the float64 log-softmax at alt_ids[k] and of the oracle's k-th largest log-probability; alt_ids[k] equal
    to the oracle's rank k wherever the oracle's gaps on both sides of rank k exceed 2e-3 - at least 90 % of the
    (position, rank) pairs (measured on the oracle: at most 2 % of the positions have such a small gap at any one rank)."""
    n, max_len = 8, 32
    tol = 2 * FP32_LOGIT_TOL
    ids_o, logits = su.oracle_run(kind, 11, n, max_len)
    eng = su.score_engine(kind, "fp32")
    ids, lens, logp, alt_ids, alt_logp = eng.recognize_gray(crops(11, n), max_len, alternatives=True)
    L = ids_o.shape[1]
    np.testing.assert_array_equal(ids[:, :L], ids_o, err_msg="fp32 ids differ from the oracle's")
    _check_alt_layout(ids, lens, logp, alt_ids, alt_logp)
    bb, tt, top5, lp5, lp_at = _rank_reference(logits, ids_o, lens)
    e_at, e_kth, clear, same = _compare_ranks(alt_ids, alt_logp, bb, tt, top5, lp5, lp_at, tol, tol)
    share = clear.mean()
    print(f"fp32 alternatives vs oracle ({kind}): |alt_logp - ref at alt_ids| {e_at:.3e}, |alt_logp - ref k-th| {e_kth:.3e} (tol {tol:.0e}); "
          f"{int(clear.sum())}/{clear.size} (position, rank) pairs clear of a {tol:.0e} gap ({100 * share:.1f} %), {same} of them exact", flush=True)
    report(f"token alternatives fp32 vs oracle, {kind} weights, {n} crops, max_len {max_len}: ids identical, alt_logp within {e_at:.2e} of the float64 "
           f"log-softmax at alt_ids and {e_kth:.2e} of the oracle's k-th largest (bound {tol:.0e}); alt_ids == oracle rank on {same}/{int(clear.sum())} "
           f"pairs with gaps > {tol:.0e} ({100 * share:.1f} % of {clear.size})")
    assert e_at <= tol and e_kth <= tol
    assert same == int(clear.sum()), "an alternative differs from the oracle's rank where the oracle's gaps are clear"
    assert share >= 0.90


@pytest.mark.parametrize("kind", ["wide", "peaked"])
@pytest.mark.parametrize("rows", [8, 64, 300])
def test_bf16_alternatives_against_own_teacher_forced_logits(kind, rows):
    """bf16 engine, automatic kernel choice: 8 rows (small-batch path), 64 (classic), 300 (latent), max_len 32.  Reference:
    the float64 log-softmax of the engine's OWN teacher-forced logits for the ids it emitted; tolerance tol_a of the bf16
    score test (4e-5 x the LM head's sum |a w| bound + 8 x the measured float32 logsumexp error).  The two value checks of
    the fp32 test, no exemptions; peaked weights only: alt_ids[k] equal to the own logits' rank k wherever their gaps on
    both sides exceed 2 x tol_a, at least 75 % of the pairs."""
    max_len = 32
    eng = su.score_engine(kind, "bf16", max_batch=320)
    gray = np.concatenate([crops(11, 8), crops(12, rows)])[:rows]
    ids, lens, logp, alt_ids, alt_logp = eng.recognize_gray(gray, max_len, alternatives=True)
    _check_alt_layout(ids, lens, logp, alt_ids, alt_logp)
    dg = torch.from_numpy(gray).cuda()
    torch.cuda.synchronize()
    T = max_len - 1
    own = eng.decode_logits(dg, rows, ids[:, :T])                  # [rows, T, V]: step t chose ids[:, t + 1]
    assert np.isfinite(own).all()
    e32 = su.f32_lse_error(own.reshape(-1, V)[:: max(1, rows // 8)])
    scale = su.lm_head_scale(su.score_weights(kind))
    tol_a = 4 * GEMM_REL * scale + 8 * e32
    bb, tt, top5, lp5, lp_at = _rank_reference(own, ids, lens)
    e_at, e_kth, clear, same = _compare_ranks(alt_ids, alt_logp, bb, tt, top5, lp5, lp_at, tol_a, 2 * tol_a)
    share = clear.mean()
    print(f"bf16 alternatives ({kind}, {rows} rows) vs own teacher-forced logits: |alt_logp - ref at alt_ids| {e_at:.3e}, |alt_logp - ref k-th| "
          f"{e_kth:.3e}, tol_a {tol_a:.3e}; {int(clear.sum())}/{clear.size} pairs clear of a {2 * tol_a:.2e} gap ({100 * share:.1f} %), {same} exact", flush=True)
    report(f"token alternatives bf16 {kind} weights, {rows} rows vs the engine's own teacher-forced logits: alt_logp within {e_at:.2e} at alt_ids, "
           f"{e_kth:.2e} of the k-th largest (tol {tol_a:.2e}); compared share {100 * share:.1f} % of {clear.size} pairs, {same}/{int(clear.sum())} exact")
    assert e_at <= tol_a and e_kth <= tol_a
    if kind == "peaked":
        assert same == int(clear.sum()), "an alternative differs from the own logits' rank where their gaps are clear"
        assert share >= 0.75, f"only {100 * share:.0f} % of the pairs have clear gaps"


# ------------------------------------------------------------------------------------------------ 6. product surface
def test_product_surface_alternatives_calls():
    from PIL import Image
    from manga_ocr import MangaOcr
    from manga_ocr.ocr import Recognition
    m = MangaOcr(synthetic_seed=1, dtype="fp32", max_batch=8, lanes=1)
    try:
        m.engine.set_generate_max_length(24)
        rs = np.random.RandomState(5)
        imgs = [Image.fromarray(rs.randint(0, 256, (40 + 7 * i, 60 + 5 * i, 3), dtype=np.uint8), "RGB") for i in range(8)]
        arrs = [np.asarray(im) for im in imgs]
        ids, lens, logp, alt_ids, alt_logp = m.engine.recognize_images(arrs, alternatives=True)
        _check_alt_layout(ids, lens, logp, alt_ids, alt_logp)
        batch_blocks = (ids, lens, logp, alt_ids, alt_logp)
        texts = m.recognize_batch(imgs)

        def same_as_engine(r, i, blocks=None):
            """r against row i of the engine's blocks for the same batch (default: the eight crops in one call)"""
            ids, lens, logp, alt_ids, alt_logp = blocks or batch_blocks
            assert isinstance(r, Recognition) and r.text == texts[i]
            i = 0 if blocks else i                                   # (blocks: of crop i alone)
            np.testing.assert_array_equal(r.ids, ids[i, :lens[i]])
            np.testing.assert_array_equal(r.logprobs, logp[i, 1:lens[i]])
            assert r.alt_ids.shape == (lens[i] - 1, K4) and r.alt_logprobs.shape == (lens[i] - 1, K4)
            np.testing.assert_array_equal(r.alt_ids, alt_ids[i, 1:lens[i]])
            np.testing.assert_array_equal(r.alt_logprobs, alt_logp[i, 1:lens[i]])
            for k in (0, len(r.logprobs) - 1):
                c = r.candidates(k)
                assert len(c) == K4 and c[0][0] == m.vocab.tokens[r.ids[k + 1]], "candidates(k)[0] is not the emitted token"
                assert c[0][1] == pytest.approx(float(np.exp(np.float64(r.logprobs[k]))), rel=1e-12)
                assert [p for _, p in c] == sorted([p for _, p in c], reverse=True) and 0 < sum(p for _, p in c) <= 1 + 1e-6

        for i, r in enumerate(m.recognize_batch_alternatives(imgs)):
            same_as_engine(r, i)
        for i, r in enumerate(m.recognize_bgr_alternatives([a[:, :, ::-1] for a in arrs])):
            same_as_engine(r, i)
        # a single-crop call is a batch of one: against the engine's call for that crop alone (a row's last bits may
        # depend on the batch it is decoded in - the kernels are chosen by row count - so not against the batch of eight)
        for i in (0, 5):
            one = m.engine.recognize_images([arrs[i]], alternatives=True)
            np.testing.assert_array_equal(one[0][0], ids[i], err_msg="ids of a crop alone differ from its ids in the batch")
            same_as_engine(m.recognize_alternatives(imgs[i]), i, one)
        # regions: a sliver is all -1 / 0 at the engine and empty in the Recognition
        page = rs.randint(0, 256, (300, 400, 3), dtype=np.uint8)
        regs = [(0, 10, 20, 100, 60), (0, 0, 0, 1, 1), (0, 200, 100, 80, 120)]
        e_ids, e_lens, e_logp, e_ai, e_al = m.engine.recognize_regions([page], regs, True, alternatives=True)
        assert e_lens[1] == 0 and (e_ai[1] == -1).all() and (e_al[1] == 0).all() and (e_logp[1] == 0).all()
        _check_alt_layout(e_ids, e_lens, e_logp, e_ai, e_al)
        rr = m.recognize_regions_alternatives([page], regs)
        assert [r.text for r in rr] == m.recognize_regions([page], regs)
        assert rr[1].text == "" and rr[1].confidence == 0.0 and rr[1].alt_ids.shape == (0, K4) and rr[1].alt_logprobs.shape == (0, K4)
        for j in (0, 2):
            np.testing.assert_array_equal(rr[j].alt_ids, e_ai[j, 1:e_lens[j]])
            np.testing.assert_array_equal(rr[j].alt_logprobs, e_al[j, 1:e_lens[j]])
            assert rr[j].candidates(0)[0][0] == m.vocab.tokens[rr[j].ids[1]]
        # the device entry point: the same blocks into device buffers
        gray = m.engine.preprocess(arrs)
        d = dict(g=torch.from_numpy(gray).cuda(), ids=torch.zeros(ids.shape, dtype=torch.int32, device="cuda"),
                 lens=torch.zeros(8, dtype=torch.int32, device="cuda"), logp=torch.zeros(ids.shape, device="cuda"),
                 ai=torch.zeros(alt_ids.shape, dtype=torch.int32, device="cuda"), al=torch.ones(alt_ids.shape, device="cuda"))
        torch.cuda.synchronize()
        m.engine.recognize_device(d["g"], 8, d["ids"], d["lens"], d["logp"], d["ai"], d["al"])
        m.engine.synchronize()
        np.testing.assert_array_equal(d["ids"].cpu().numpy(), ids)
        np.testing.assert_array_equal(d["ai"].cpu().numpy(), alt_ids)
        np.testing.assert_array_equal(_bits(d["al"].cpu().numpy()), _bits(alt_logp))
        # nine threads mixing the three kinds of single-crop call on one instance
        out = [None] * 9
        def work(i):
            im = imgs[i % 8]
            out[i] = m.recognize_alternatives(im) if i % 3 == 2 else m.recognize_scored(im) if i % 3 == 1 else m(im)
        th = [threading.Thread(target=work, args=(i,)) for i in range(9)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for i in range(9):
            if i % 3 == 0:
                assert isinstance(out[i], str) and out[i] == texts[i % 8]
            else:
                assert isinstance(out[i], Recognition) and out[i].text == texts[i % 8]
                assert (out[i].alt_ids is None) == (i % 3 == 1)
                if i % 3 == 2:
                    np.testing.assert_array_equal(out[i].alt_ids[:, 0], out[i].ids[1:])
                    np.testing.assert_allclose(out[i].alt_logprobs, alt_logp[i % 8, 1:lens[i % 8]], rtol=0, atol=2 * FP32_LOGIT_TOL)
        report("MangaOcr alternatives surface: recognize_alternatives / _batch_alternatives / _bgr_alternatives / _regions_alternatives == Engine "
               "blocks, candidates(k)[0] = the emitted token, sliver -> -1 / 0 and empty, device entry point identical, 9 mixed threads consistent")
    finally:
        m.close()
