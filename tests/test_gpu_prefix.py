"""-m gpu: forced prefixes - caller-given tokens scored and continued inside the masked, scored LM-head step.

Bottom up: the target column of the masked LM-head epilogues (mocr_op_gemm_argmax_target) against the same operator under a
singleton set, bit for bit; the token kernel (mocr_op_dec_token_prefix) on every kind of row; whole recognitions against the
reference loop on the fp32 oracle (prefix_util.prefix_generate); the bf16 decode paths; sets and n-grams together; compaction,
graphs, memory and the argument errors; positions; the Python surface.

Tolerances are those of tests/test_gpu_constraints.py (imported, named where used)."""
import threading

import numpy as np
import pytest

from gpu_util import bf16_round, crops, report

import constraint_util as cu
import ngram_util as nu
import prefix_util as pu
import score_util as su
from test_gpu_constraints import (BF16_LOGIT_TOL, FP32_LOGIT_TOL, TOKEN_SCORE_TOL, _bits, _f32, _i32, _t, _u32, fresh_engine,  # noqa: F401
                                  kernel_masks, lex_top)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

D, V, K4, EOS, START = 768, 6144, 4, 3, 2
NO_IDX = cu.NO_IDX
GUARD = 2
SENT = -777


# ------------------------------------------------------------------------------------------------ 1. the target epilogue, exact
def _head(eng, dA, dW, db, M, tile, table, sor, rowmap, target=None):
    """the alternatives form of the masked LM head, with (target = (prefix, prefix_len, ld, step, tgt_val)) or without the
    target column; guard rows behind every output -> (cand_val, cand_idx, cand_sum, top_val, top_idx) [M] rows each"""
    nt = V // tile
    cv = torch.full((M + GUARD, nt), float("nan"), device="cuda")
    ci = torch.full((M + GUARD, nt), SENT, dtype=torch.int32, device="cuda")
    cs = cv.clone()
    tv = torch.full((M + GUARD, nt, K4), float("nan"), device="cuda")
    ti = torch.full((M + GUARD, nt, K4), SENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if target is None:
        eng.op_gemm_argmax_masked(dA, dW, db, cv, ci, cs, tv, ti, M, V, D, tile, table, sor, rowmap)
    else:
        eng.op_gemm_argmax_target(dA, dW, db, cv, ci, cs, tv, ti, M, V, D, tile, table, sor, rowmap, *target)
    out = [x.cpu().numpy() for x in (cv, ci, cs, tv, ti)]
    for x in out:
        assert (np.isnan(x[M:]) if x.dtype == np.float32 else x[M:] == SENT).all(), "guard rows written"
    return [x[:M] for x in out]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("tile", [64, 128])
def test_target_epilogue_exact(dtype, tile):
    """mocr_op_gemm_argmax_target, M = 70 (two 64-row tiles / one 128-row tile, a ragged last one) with guard rows behind it,
    N 6144, K 768.  GEMM row m is slot m of a permuted rowmap over M + 3 rows; the prefix arrays are by row, step and tgt_val by
    slot.  Slot kinds (m % 7): no prefix; column 0; column 6143; a column of a middle tile; a column outside the row's set;
    step >= prefix_len; a random column.  Expected: tgt_val[m] is bit-identical to cand_val[m][target's tile] of
    mocr_op_gemm_argmax_masked run under the singleton set {target} - the same operator, so no float reference is needed -
    and -inf where the row's set leaves the target out; untouched where there is no target and in the guard rows; the
    candidate, sum and top arrays bit-identical to mocr_op_gemm_argmax_masked's."""
    eng = su.score_engine("wide", dtype)
    M, ld = 70, 9
    rs = np.random.RandomState(100 + tile)
    Mp = (M + tile - 1) // tile * tile
    R = M + 3
    rowmap = rs.permutation(R)[:M].astype(np.int32)
    A = np.zeros((Mp, D), np.float32)
    A[:M] = rs.standard_normal((M, D))
    W = (rs.standard_normal((V, D)) * 0.05).astype(np.float32)
    if dtype == "bf16":
        A, W = bf16_round(A), bf16_round(W)
    bias = rs.standard_normal(V).astype(np.float32)
    logits = A[:M].astype(np.float64) @ W.astype(np.float64).T + bias
    masks7 = kernel_masks(logits, tile, 2 * tile)
    kind = np.arange(M) % 7
    set_of_row = np.zeros(R, np.int32)
    set_of_row[rowmap] = np.where(kind == 4, 1, np.array([0, 1, 3])[np.arange(M) % 3])      # by ROW
    step = rs.randint(0, 4, size=M).astype(np.int32)
    prefix = rs.randint(0, V, size=(R + 1, ld)).astype(np.int32)
    prefix_len = np.zeros(R + 1, np.int32)
    banned1 = np.nonzero(~masks7[1])[0]
    target = np.full(M, -1)
    for m in range(M):
        row, k = rowmap[m], kind[m]
        prefix_len[row] = 0 if k == 0 else step[m] if k == 5 else step[m] + 1 + rs.randint(0, 3)
        if k in (0, 5):
            continue
        target[m] = {1: 0, 2: V - 1, 3: 3000 + m, 4: int(banned1[m % banned1.size]), 6: int(rs.randint(0, V))}[k]
        prefix[row, step[m]] = target[m]
    prefix_len[R] = 5                                                # a row no slot decodes
    assert (prefix_len[:R] <= ld).all() and (rowmap != np.arange(M)).any(), "a kernel reading the prefix by slot must fail"
    has = target >= 0
    allowed = np.array([has[m] and masks7[set_of_row[rowmap[m]], target[m]] for m in range(M)])
    assert has.sum() == 50 and (has & ~allowed)[kind == 4].all() and allowed[kind == 1].any() and allowed[kind == 2].any()
    dA, dW, db = _t(A, dtype), _t(W, dtype), _f32(bias)
    table, d_sor, d_map = _u32(cu.pack_sets(masks7)), _i32(set_of_row), _i32(rowmap)
    want = _head(eng, dA, dW, db, M, tile, table, d_sor, d_map)
    junk = rs.standard_normal(M + GUARD).astype(np.float32)
    d_tgt = _f32(junk)
    got = _head(eng, dA, dW, db, M, tile, table, d_sor, d_map, (_i32(prefix), _i32(prefix_len), ld, _i32(step), d_tgt))
    for name, g, w_ in zip(("cand_val", "cand_idx", "cand_sum", "top_val", "top_idx"), got, want):
        np.testing.assert_array_equal(g.view(np.uint32), w_.view(np.uint32), err_msg=f"{name} differs from mocr_op_gemm_argmax_masked")
    tgt = d_tgt.cpu().numpy()
    np.testing.assert_array_equal(_bits(tgt[M:]), _bits(junk[M:]), err_msg="guard rows of tgt_val written")
    np.testing.assert_array_equal(_bits(tgt[:M][~has]), _bits(junk[:M][~has]), err_msg="tgt_val of a row without a target written")
    assert np.isneginf(tgt[:M][has & ~allowed]).all(), "a masked target is not -inf"
    # the singleton sets: set m = {target[m]} (no EOS added: the table is the caller's), slot m decodes under it by the identity
    single = np.zeros((M, V), bool)
    single[np.nonzero(has)[0], target[has]] = True
    single[~has, EOS] = True
    one = _head(eng, dA, dW, db, M, tile, _u32(cu.pack_sets(single)), _i32(np.arange(M)), None)
    ref = one[0][np.arange(M), np.maximum(target, 0) // tile]
    assert np.isfinite(ref[has]).all() and (one[1][np.arange(M), np.maximum(target, 0) // tile][has] == target[has]).all()
    np.testing.assert_array_equal(_bits(tgt[:M][allowed]), _bits(ref[allowed]), err_msg="tgt_val is not the cand_val of the singleton set")
    d64 = np.abs(ref[has] - logits[np.nonzero(has)[0], target[has]]).max()
    report(f"target epilogue {dtype} tile {tile}: 50 targets of 70 rows (columns 0, 6143, middle, masked, random; permuted rowmap), tgt_val "
           f"bit-identical to the singleton-set cand_val (|that - float64 logit| <= {d64:.2e}), -inf where masked, untouched elsewhere; "
           f"candidates / sums / top four bit-identical to the masked operator")


# ------------------------------------------------------------------------------------------------ 2. the token step, exact
# slot -> (row, kind, step, finished): the row kinds of the issue
STEP_SLOTS = [(5, "forced", 3, False), (2, "free", 2, False), (7, "finished", 6, True), (0, "forced_eos", 4, False),
              (3, "forced_last", 14, False), (6, "forced_argmax", 1, False), (1, "forced_masked", 5, False)]
TOP = [30.0, 29.0, 28.0, 27.0]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("path", ["cand64", "cand128", "slabs1", "slabs3"])
def test_prefix_token_step_exact(dtype, path):
    """mocr_op_dec_token_prefix, alternatives form, candidate and slab path: 7 slots over 8 rows through a permuted rowmap,
    ids_ld = max_len = 16, a different step per slot.  Row kinds: forced (the token is not the arg-max); free (prefix shorter
    than the step); finished (emits pad, scores 0, although its prefix is longer); a forced EOS (finishes, len = t + 2); a
    forced token at t + 2 == max_len (finishes there); a forced token equal to the arg-max under a set that leaves S = 1 (the
    score's bits equal the free step's, -0 included); a forced token outside the row's set (scores -inf, still emitted).
    Expected exactly: ids, step, finished, len, n_unfinished, and - against the same launch WITHOUT a prefix - the alternatives
    (ids and bits) of every slot and the scores of the free, finished and forced-arg-max slots.  The forced scores: within
    TOKEN_SCORE_TOL (tests/test_gpu_scores.py: the fp32 evaluation of -log S) + 2^-23 |score| (one fp32 rounding of the final
    add; v - gmax is exact for these logits, multiples of 1/256 below 64) of the float64 masked log-softmax."""
    eng = su.score_engine("wide", dtype)
    n, R, ids_ld, max_len, ld = len(STEP_SLOTS), 8, 16, 16, 15
    rowmap = np.array([s[0] for s in STEP_SLOTS], np.int32)
    step = np.array([s[2] for s in STEP_SLOTS], np.int32)
    rs = np.random.RandomState({"slabs1": 31, "slabs3": 33, "cand64": 364, "cand128": 428}[path])
    lg = (np.round(rs.standard_normal((n, V)) * 3 * 256) / 256)
    lg = np.clip(lg, -20, 20)
    tops = [[100 + 10 * s + k for k in range(4)] for s in range(n)]
    for s in range(n):
        lg[s, tops[s]] = TOP
    lg[:, EOS] = -8.0
    forced_tok = {0: 2500, 3: EOS, 4: 4100, 5: tops[5][0], 6: 777}                 # slot -> its forced token
    lg[0, 2500], lg[4, 4100], lg[6, 777] = 25.5, 26.25, 29.5
    lg[5, EOS] = -200.0                                                              # exp(-230) = 0 in fp32: S = 1, score -0
    lg = lg.astype(np.float32).astype(np.float64)
    masks = np.ones((4, V), bool)                                                    # sets: 0 all, 1 {arg-max of slot 5, EOS}, 2 without 777
    masks[1] = cu.mask_of([tops[5][0]])
    masks[2, 777] = False
    set_of_row = np.zeros(R, np.int32)
    set_of_row[6], set_of_row[1] = 1, 2
    mk = masks[set_of_row[rowmap]]                                                   # [n, V] by slot
    ids = np.full((R + 1, ids_ld), 4000, np.int32)
    finished = np.zeros(R, np.int32)
    lens = np.full(R, max_len, np.int32)
    prefix = rs.randint(5, V, size=(R + 1, ld)).astype(np.int32)
    prefix_len = np.zeros(R + 1, np.int32)
    for s, (row, kind, t, fin) in enumerate(STEP_SLOTS):
        ids[row, 0] = START
        prefix_len[row] = 2 if kind == "free" else 10 if kind == "finished" else t + 1 if kind in ("forced_eos", "forced_last") else t + 3
        if s in forced_tok:
            prefix[row, t] = forced_tok[s]
        if fin:
            finished[row], lens[row] = 1, 5
    prefix_len[4] = 9                                                                # a row no slot decodes
    assert len(set(step.tolist())) == n and (prefix_len[:R] <= ld).all()

    def inputs():
        if path.startswith("slabs"):
            nslab = int(path[5:])
            r2 = np.random.RandomState(5)
            bias = (r2.randint(-100, 100, V) / 64.0).astype(np.float64)
            parts = (r2.randint(-300, 300, (nslab, n, V)) / 64.0).astype(np.float64)
            parts[-1] = lg - bias - parts[:-1].sum(0)
            assert (parts.astype(np.float32).astype(np.float64) == parts).all()
            return dict(slabs=_f32(parts), nslab=nslab, vbias=_f32(bias)), None, None, None, None
        tile = int(path[4:])
        nt = V // tile
        m, idx, s_ = cu.masked_tile_stats(lg, mk, tile)
        t3 = cu.masked(lg, mk).reshape(n, nt, tile)
        ti = lex_top(t3)
        tv = np.take_along_axis(t3, ti, -1)
        ti = np.where(np.isneginf(tv), NO_IDX, ti + (np.arange(nt) * tile)[None, :, None])
        tgt = np.full(n + GUARD, np.nan, np.float32)                                 # what the target epilogue leaves: forced slots only
        for s, tok in forced_tok.items():
            tgt[s] = lg[s, tok] if mk[s, tok] else -np.inf
        return dict(cand_val=_f32(m), cand_idx=_i32(idx), ncand=nt), _f32(s_), _f32(tv), _i32(ti), _f32(tgt)

    def run(with_prefix):
        kw, cand_sum, top_val, top_idx, tgt = inputs()
        d = dict(ids=_i32(ids), step=_i32(step), finished=_i32(finished), len=_i32(lens), n_unfinished=_i32([6, SENT]),
                 rowmap=_i32(rowmap), x_f32=torch.full((n + GUARD, D), float("nan"), device="cuda"),
                 x_t=torch.full((n + GUARD, D), float("nan"), device="cuda", dtype=torch.bfloat16 if dtype == "bf16" else torch.float32))
        sc = torch.full((R + 1, ids_ld), float("nan"), device="cuda")
        ai = torch.full((R + 1, ids_ld, K4), SENT, dtype=torch.int32, device="cuda")
        al = torch.full((R + 1, ids_ld, K4), float("nan"), device="cuda")
        torch.cuda.synchronize()
        pre = (_i32(prefix), _i32(prefix_len), ld, tgt) if with_prefix else (None, None, 0, None)
        eng.op_dec_token_prefix(cand_sum, sc, top_val, top_idx, ai, al, _u32(cu.pack_sets(masks)), _i32(set_of_row), None, None, None, None,
                                *pre, first=0, n=n, ids_ld=ids_ld, max_len=max_len, n_real=n, **d, **kw)
        o = {k: v.float().cpu().numpy() if v.dtype == torch.bfloat16 else v.cpu().numpy() for k, v in d.items()}
        return o, sc.cpu().numpy(), ai.cpu().numpy(), al.cpu().numpy()

    free, f_sc, f_ai, f_al = run(False)
    got, sc, ai, al = run(True)
    argmax = np.argmax(cu.masked(lg, mk), -1)
    assert argmax.tolist() == [tops[s][0] for s in range(n)] and argmax[5] == forced_tok[5]
    want_tok = [forced_tok.get(s, int(argmax[s])) for s in range(n)]
    want_tok[2] = 0                                                                  # the finished row pads
    at = (rowmap, step + 1)
    assert got["ids"][at].tolist() == want_tok, got["ids"][at].tolist()
    assert free["ids"][at].tolist() == [0 if s == 2 else int(argmax[s]) for s in range(n)]
    want_ids = ids.copy(); want_ids[at] = want_tok
    np.testing.assert_array_equal(got["ids"], want_ids, err_msg="ids written elsewhere")
    np.testing.assert_array_equal(got["step"], step + 1)
    want_fin, want_len = finished.copy(), lens.copy()
    for s in (3, 4):                                                                 # the forced EOS, the forced token at max_len
        want_fin[rowmap[s]], want_len[rowmap[s]] = 1, step[s] + 2
    np.testing.assert_array_equal(got["finished"], want_fin); np.testing.assert_array_equal(got["len"], want_len)
    assert got["n_unfinished"].tolist() == [4, SENT] and free["n_unfinished"].tolist() == [5, SENT], "the free run finishes slot 4 only"
    assert want_len[rowmap[4]] == max_len and step[4] + 2 == max_len
    # the alternatives of a forced step are the step's own: everything but the forced scores equals the un-prefixed launch
    np.testing.assert_array_equal(ai, f_ai); np.testing.assert_array_equal(_bits(al), _bits(f_al))
    assert (ai[at][[0, 1, 3, 4, 5, 6], 0] == argmax[[0, 1, 3, 4, 5, 6]]).all(), "entry 0 is what the model would have chosen"
    keep = np.ones_like(sc, bool); keep[rowmap[[0, 3, 4, 6]], step[[0, 3, 4, 6]] + 1] = False
    np.testing.assert_array_equal(_bits(sc[keep]), _bits(f_sc[keep]), err_msg="a free / finished / forced-arg-max score moved")
    assert _bits(sc[at][5:6])[0] == 0x80000000 == _bits(f_sc[at][5:6])[0], "the forced arg-max keeps the free step's -0"
    assert sc[at][2] == 0.0 and np.isneginf(sc[at][6]) and got["ids"][at][6] == 777
    worst = 0.0
    for s in (0, 3, 4):
        ref = cu.masked_log_softmax64(lg[s], mk[s])[forced_tok[s]]
        err = abs(float(sc[at][s]) - ref)
        print(f"slot {s}: forced score {sc[at][s]:.7f}, float64 {ref:.7f}, |diff| {err:.2e}", flush=True)
        assert err <= TOKEN_SCORE_TOL + 2.0 ** -23 * abs(ref), (s, err)
        worst = max(worst, err)
    # the forced token is what the next step consumes: its embedding row equals the one a free step emits for that token
    lg2 = lg.copy()
    for s, tok in forced_tok.items():
        if mk[s, tok]:
            lg2[s, tok] = 40.0
    lg_keep, lg = lg, lg2
    again, _, _, _ = run(False)
    lg = lg_keep
    same = [s for s, tok in forced_tok.items() if mk[s, tok]]
    assert again["ids"][at][same].tolist() == [forced_tok[s] for s in same]
    np.testing.assert_array_equal(_bits(got["x_f32"][same]), _bits(again["x_f32"][same]), err_msg="the embedding fed back is not the forced token's")
    report(f"dec_token prefix {dtype} {path}: forced / free / finished / forced EOS / forced at max_len / forced arg-max (-0) / forced masked (-inf) "
           f"exact in ids, step, finished, len, n_unfinished; alternatives bit-identical to the un-prefixed launch; forced scores within {worst:.1e}")


# ------------------------------------------------------------------------------------------------ 3. fp32 against the reference loop
N_E2E, LEN_E2E = 8, 24
SELF_LENS = (0, 1, 3, 5, 11, 23, 23, 0)


def _enc(kind, seed, n):
    o = su.score_oracle(kind)
    with torch.no_grad():
        return o, o.encode(o.preprocess_gray(crops(seed, n)))


def _assert_same_run(a, b, what):
    """(ids, lens, logp, alt_ids, alt_logp[, pos]) twice: bit-identical"""
    for x, y, name in zip(a, b, ("ids", "lens", "logp", "alt_ids", "alt_logp", "positions")):
        np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32), err_msg=f"{what}: {name}")


def test_fp32_self_prefix_is_bit_identical():
    """(a) fp32, wide weights, crops(31, 8), max_len 24: prefixes = the engine's own free ids cut to (0, 1, 3, 5, 11, 23, 23, 0)
    tokens.  ids, lengths, scores and alternatives are bit-identical to the free run; so is a batch of all-empty prefixes."""
    eng = su.score_engine("wide", "fp32")
    gray = crops(31, N_E2E)
    free = eng.recognize_gray(gray, LEN_E2E, alternatives=True)
    pre = [free[0][b, 1:1 + P].tolist() for b, P in enumerate(SELF_LENS)]
    got = eng.recognize_gray(gray, LEN_E2E, alternatives=True, prefixes=pre)
    _assert_same_run(got, free, "self-prefix")
    _assert_same_run(eng.recognize_gray(gray, LEN_E2E, alternatives=True, prefixes=[None] * N_E2E), free, "empty prefixes")
    i0, l0 = eng.recognize_gray(gray, LEN_E2E, prefixes=pre)
    np.testing.assert_array_equal(i0, free[0]); np.testing.assert_array_equal(l0, free[1])
    report("forced prefixes fp32: a self-prefix of 0 / 1 / 3 / 5 / 11 / 23 tokens reproduces the free run bit for bit (ids, lens, logp, alternatives)")


def test_fp32_perturbed_prefix_against_the_reference_loop():
    """(b) P = 5 and token 5 replaced by the oracle's runner-up.  On the oracle alone: every continuation differs from the free
    run, and every free-step margin of the reference exceeds 2 x FP32_LOGIT_TOL (two logits each within tol cannot swap).  Then:
    ids and lengths identical to prefix_generate; forced and free logp and the alternatives within 2 x FP32_LOGIT_TOL of the
    float64 log-softmax (the bound of the constraints tests); alt_ids entry 0 of a forced step is the model's own pick."""
    P = 5
    free_ids, free_logits = su.oracle_run("wide", 31, N_E2E, LEN_E2E)
    o, enc = _enc("wide", 31, N_E2E)
    pre = [free_ids[b, 1:1 + P].tolist() for b in range(N_E2E)]
    for b in range(N_E2E):
        pre[b][P - 1] = int(pu.runner_up(free_logits[b, P - 1]))
        assert pre[b][P - 1] != free_ids[b, P] and pre[b][P - 1] != EOS
    ids_o, logits, masks = pu.prefix_generate(o, enc, pre, None, None, LEN_E2E)
    lens_o = nu.lengths(ids_o)
    L = ids_o.shape[1]
    differ = [(ids_o[b, P + 1:] != free_ids[b, P + 1:L]).any() for b in range(N_E2E)]
    gaps = nu.step_gaps(logits, masks)
    free_steps = np.array([[P <= t < lens_o[b] - 1 for t in range(L - 1)] for b in range(N_E2E)])
    print(f"perturbed prefix: {sum(differ)} of {N_E2E} continuations differ from the free run, smallest free-step margin {gaps[free_steps].min():.2e}", flush=True)
    assert all(differ), differ
    assert gaps[free_steps].min() > 2 * FP32_LOGIT_TOL
    eng = su.score_engine("wide", "fp32")
    ids, lens, logp, alt_ids, alt_logp = eng.recognize_gray(crops(31, N_E2E), LEN_E2E, alternatives=True, prefixes=pre)
    live = np.arange(L)[None, :] < lens_o[:, None]
    np.testing.assert_array_equal(np.where(live, ids[:, :L], 0), np.where(live, ids_o, 0), err_msg="ids differ from prefix_generate's")
    np.testing.assert_array_equal(lens, lens_o)
    assert (ids[:, 1:P + 1] == np.array(pre)).all()
    want = pu.stored_logp64(logits, masks, ids_o, lens_o)
    worst = float(np.abs(logp[:, :L] - want)[live].max())
    for b in range(N_E2E):
        for t in range(1, lens[b]):
            w4, lp4 = cu.masked_top(logits[b, t - 1], masks[b, t - 1])
            np.testing.assert_array_equal(alt_ids[b, t], w4)
            worst = max(worst, float(np.abs(alt_logp[b, t] - lp4).max()))
            if t > P:
                assert alt_ids[b, t, 0] == ids[b, t] and _bits(alt_logp[b, t, :1])[0] == _bits(logp[b, t:t + 1])[0]
        assert alt_ids[b, P, 0] == free_ids[b, P] != ids[b, P], "entry 0 of the perturbed step is what the model would have chosen"
    print(f"perturbed prefix: max |logp - float64 log-softmax| {worst:.3e} (bound {2 * FP32_LOGIT_TOL:.0e})", flush=True)
    assert worst <= 2 * FP32_LOGIT_TOL
    report(f"forced prefixes fp32 vs the reference loop: P = 5 with token 5 perturbed, 8 of 8 continuations differ from the free run, ids identical "
           f"(smallest free-step margin {gaps[free_steps].min():.1e}), logp / alt_logp within {worst:.2e} (bound {2 * FP32_LOGIT_TOL:.0e})")


def test_fp32_text_scoring():
    """(c) early-EOS weights: the prefix is the oracle's greedy row through EOS (P generated tokens + EOS): the length is P + 2
    tokens with the start token, the ids equal the prefix, and the sum of logp is within P x 2 x FP32_LOGIT_TOL of the float64
    sequence log-probability.  A second prefix with EOS forced after two tokens: the row ends there."""
    n, max_len = 8, 32
    free_ids, free_logits = su.oracle_run("eos", 4321, n, max_len)
    lens_o = nu.lengths(free_ids)
    assert 2 <= (lens_o < max_len).sum() < n, "some rows were meant to end in EOS, some at max_len"
    pre = [free_ids[b, 1:lens_o[b]].tolist() for b in range(n)]
    eng = su.score_engine("eos", "fp32")
    ids, lens, logp = eng.recognize_gray(crops(4321, n), max_len, scores=True, prefixes=pre)
    np.testing.assert_array_equal(lens, lens_o)
    worst = 0.0
    for b in range(n):
        np.testing.assert_array_equal(ids[b, :lens[b]], free_ids[b, :lens[b]]); assert (ids[b, lens[b]:] == 0).all() and (logp[b, lens[b]:] == 0).all()
        ref = su.chosen_logp64(free_logits[b:b + 1], free_ids[b:b + 1])[0, :lens[b] - 1].sum()
        err = abs(float(logp[b].astype(np.float64).sum()) - ref)
        assert err <= (lens[b] - 1) * 2 * FP32_LOGIT_TOL, (b, err)
        worst = max(worst, err)
    early = [free_ids[b, 1:3].tolist() + [EOS] for b in range(n)]
    ids2, lens2, logp2 = eng.recognize_gray(crops(4321, n), max_len, scores=True, prefixes=early)
    assert (lens2 == 4).all() and (ids2[:, 3] == EOS).all() and (ids2[:, 4:] == 0).all() and (logp2[:, 4:] == 0).all()
    np.testing.assert_array_equal(_bits(logp2[:, 1:3]), _bits(logp[:, 1:3]))
    ref3 = su.log_softmax64(free_logits[:, 2])[:, EOS]
    assert np.abs(logp2[:, 3] - ref3).max() <= 2 * FP32_LOGIT_TOL
    report(f"text scoring fp32: sum of logp of the oracle's own rows within {worst:.2e} of the float64 sequence log-probability; a forced early EOS ends the row")


# ------------------------------------------------------------------------------------------------ 4. bf16 paths
BF16_CASES = [("small", 8, 0), ("latent", 64, 64), ("fused64", 96, 0), ("nofused", 96, 16), ("fused128", 1024, 0)]


@pytest.mark.parametrize("name,rows,flags", BF16_CASES)
def test_bf16_prefix_paths(name, rows, flags):
    """bf16; the first 8 rows are crops(31, 8), the others repeat them.  Full-text prefix: the prefixes are the oracle's free
    ids (23 tokens), so nothing can diverge - ids equal the prefix exactly and every logp of the first 8 rows is within
    2 x BF16_LOGIT_TOL (the 3e-2 of tests/test_gpu_bf16_parity.py; |d(logit - lse)| <= 2 max |d logit|) of the float64
    log-softmax of the oracle's logits on those ids.  Self-prefix: bit-identity with the free run at the same row count."""
    free_ids, free_logits = su.oracle_run("wide", 31, N_E2E, LEN_E2E)
    eng = su.score_engine("wide", "bf16", max_batch=max(64, rows), flags=flags)
    gray = np.concatenate([crops(31, N_E2E)] * (rows // N_E2E))
    pre = [free_ids[b % N_E2E, 1:].tolist() for b in range(rows)]
    ids, lens, logp = eng.recognize_gray(gray, LEN_E2E, scores=True, prefixes=pre)
    np.testing.assert_array_equal(ids[:, :LEN_E2E], np.concatenate([free_ids] * (rows // N_E2E)))
    assert (lens == LEN_E2E).all()
    want = su.chosen_logp64(free_logits, free_ids)
    err = float(np.abs(logp[:N_E2E, 1:LEN_E2E] - want).max())
    print(f"bf16 {name}: max |logp - float64 log-softmax of the oracle| {err:.3e} (bound {2 * BF16_LOGIT_TOL:.0e})", flush=True)
    assert np.isfinite(logp).all() and err <= 2 * BF16_LOGIT_TOL
    free = eng.recognize_gray(gray, LEN_E2E, alternatives=True)
    own = [free[0][b, 1:1 + SELF_LENS[b % N_E2E]].tolist() for b in range(rows)]
    _assert_same_run(eng.recognize_gray(gray, LEN_E2E, alternatives=True, prefixes=own), free, f"bf16 {name} self-prefix")
    report(f"forced prefixes bf16 {name} ({rows} rows, flags {flags}): full-text prefix emitted exactly, logp within {err:.2e} of the oracle "
           f"(bound {2 * BF16_LOGIT_TOL:.0e}); self-prefix bit-identical to the free run")


# ------------------------------------------------------------------------------------------------ 5. sets and n-grams together
def test_prefix_with_sets_and_ngrams(fresh_engine):
    """fp32, 8 crops, max_len 24, n = 3 on every row.  Rows 0-3: a prefix a b c a b c - its last token completes a held 3-gram
    and scores -inf at that position, is emitted, and later bans honour the prefix history (no further repeated 3-gram is
    generated).  Rows 4-5: a 2-token prefix whose second token is outside the row's set: -inf, emitted, decoding goes on inside
    the set.  Rows 6-7: P = 0.  Ids equal prefix_generate's; the P = 0 rows are bit-identical to the un-prefixed run."""
    eng = fresh_engine("wide", "fp32", max_batch=8)
    o, enc = _enc("wide", 31, N_E2E)
    free_ids, _ = su.oracle_run("wide", 31, N_E2E, LEN_E2E)
    base = np.ones((N_E2E, V), bool)
    pre = [None] * N_E2E
    for b in range(4):
        a3 = [5500 + 3 * b, 5501 + 3 * b, 5502 + 3 * b]
        pre[b] = a3 + a3
    for b in (4, 5):
        out = 2000 + b
        base[b, out] = False
        pre[b] = [int(free_ids[b, 1]), out]
    ngr = np.full(N_E2E, 3, np.int32)
    handles = [0 if m.all() else eng.token_set(np.nonzero(m)[0]) for m in base]
    ids_o, logits, masks = pu.prefix_generate(o, enc, pre, base, ngr, LEN_E2E)
    lens_o = nu.lengths(ids_o)
    L = ids_o.shape[1]
    # on the oracle alone, as in the perturbed-prefix test: every free step of the reference is decided by more than two logit
    # tolerances (checked on the CPU for exactly these tokens: the smallest margin is 4.8e-3), so the ids cannot differ
    gaps = nu.step_gaps(logits, masks)
    free_steps = np.array([[len(pre[b] or []) <= t < lens_o[b] - 1 for t in range(L - 1)] for b in range(N_E2E)])
    assert gaps[free_steps].min() > 2 * FP32_LOGIT_TOL, gaps[free_steps].min()
    ids, lens, logp, alt_ids, alt_logp = eng.recognize_gray(crops(31, N_E2E), LEN_E2E, alternatives=True, token_sets=handles,
                                                            no_repeat_ngram=ngr, prefixes=pre)
    live = np.arange(L)[None, :] < lens_o[:, None]
    np.testing.assert_array_equal(np.where(live, ids[:, :L], 0), np.where(live, ids_o, 0)); np.testing.assert_array_equal(lens, lens_o)
    want = pu.stored_logp64(logits, masks, ids_o, lens_o)
    for b in range(4):
        assert np.isneginf(logp[b, 6]) and np.isneginf(want[b, 6]) and np.isfinite(logp[b, 1:6]).all() and ids[b, 6] == pre[b][5]
        assert pre[b][5] not in alt_ids[b, 6].tolist(), "the banned token among the step's alternatives"
        assert nu.first_repeat(ids[b, 4:lens[b]], 3) is None, "a 3-gram repeated behind the prefix"
    for b in (4, 5):
        assert np.isneginf(logp[b, 2]) and ids[b, 2] == pre[b][1] and base[b][ids[b, 3:lens[b]]].all() and np.isfinite(logp[b, 3:lens[b]]).all()
    fin = np.isfinite(want) & live
    assert (np.isneginf(logp[:, :L]) == (np.isneginf(want) & live)).all()
    worst = float(np.abs(logp[:, :L] - want)[fin].max())
    assert worst <= 2 * FP32_LOGIT_TOL, worst
    plain = eng.recognize_gray(crops(31, N_E2E), LEN_E2E, alternatives=True, token_sets=handles, no_repeat_ngram=ngr)
    _assert_same_run([x[6:] for x in (ids, lens, logp, alt_ids, alt_logp)], [x[6:] for x in plain], "P = 0 rows")
    report(f"forced prefixes with sets and 3-grams: a prefix completing a held 3-gram and a token outside the set score -inf and are emitted, "
           f"ids equal the reference loop, finite logp within {worst:.2e}, P = 0 rows bit-identical to the un-prefixed run")


# ------------------------------------------------------------------------------------------------ 6. compaction, graphs, memory, errors
def test_compaction_graphs_and_memory(fresh_engine):
    """Early-EOS weights, bf16, 96 rows, max_len 32: mixed prefix lengths (0 / 2 / 5 tokens of the free run, every fourth row
    ending its prefix in EOS).  Compacted equals MOCR_FLAG_NO_COMPACTION in ids and lengths; mocr_graph_count is unchanged by a
    second identical call; free HBM is unchanged until the first prefixed call."""
    from manga_ocr.engine import device_memory
    n, max_len = 96, 32
    gray = np.concatenate([crops(4321, 6), crops(4322, n)])[:n]
    eng = fresh_engine("eos", "bf16", max_batch=96)
    free_ids, free_lens = eng.recognize_gray(gray, max_len)
    eng.recognize_gray(gray, max_len, scores=True, token_sets=np.zeros(n, np.int32))
    pre = []
    for b in range(n):
        p = free_ids[b, 1:1 + (0, 2, 5, 2)[b % 4]].tolist()
        p = [t for t in p if t != EOS]
        pre.append(p + [EOS] if b % 4 == 3 else p or None)
    mem0 = device_memory(0)[0]
    eng.recognize_gray(gray, max_len)
    assert device_memory(0)[0] == mem0, "an un-prefixed call moved the free HBM"
    g0 = eng.graph_count()
    ids, lens, logp = eng.recognize_gray(gray, max_len, scores=True, prefixes=pre)
    g1 = eng.graph_count()
    assert g1 > g0, "the prefixed batch did not capture graphs of its own"
    ids2, lens2, logp2 = eng.recognize_gray(gray, max_len, scores=True, prefixes=pre)
    assert eng.graph_count() == g1, "a repeated call captured another decode graph"
    np.testing.assert_array_equal(ids2, ids); np.testing.assert_array_equal(_bits(logp2), _bits(logp))
    for b in range(n):
        if pre[b]:
            assert ids[b, 1:1 + len(pre[b])].tolist() == pre[b]
        if b % 4 == 3:
            assert lens[b] == len(pre[b]) + 1 and (ids[b, lens[b]:] == 0).all()
    z = np.array([p is None for p in pre])
    np.testing.assert_array_equal(ids[z], free_ids[z]); np.testing.assert_array_equal(lens[z], free_lens[z])
    nc = fresh_engine("eos", "bf16", max_batch=96, flags=2048)          # MOCR_FLAG_NO_COMPACTION
    u_ids, u_lens, u_lp = nc.recognize_gray(gray, max_len, scores=True, prefixes=pre)
    np.testing.assert_array_equal(u_ids, ids); np.testing.assert_array_equal(u_lens, lens)
    fin = np.isfinite(u_lp)
    # (the scores are not bit-identical across a compaction - the LM head's tile goes by the rows a batch has left, see
    # tests/test_gpu_constraints.py: both runs evaluate -log S within TOKEN_SCORE_TOL, and a forced score adds one fp32 rounding)
    assert (fin == np.isfinite(logp)).all() and (np.abs(u_lp[fin] - logp[fin]) <= 2 * TOKEN_SCORE_TOL + 2.0 ** -23 * np.abs(logp[fin])).all()
    assert lens.min() < lens.max() and eng.compaction_count() > 0 and nc.compaction_count() == 0
    report(f"forced prefixes bf16 early-EOS 96 rows: compacted == uncompacted, graphs {g0} -> {g1}, none added by a repeat, HBM untouched before the first prefix")


def test_argument_errors(fresh_engine):
    """every MOCR_ERR_ARG case of the forced-prefix section, through the gray_host and the device entry points"""
    import ctypes as C
    from manga_ocr._capi import MocrError
    eng = fresh_engine("wide", "fp32", max_batch=8)
    gray = crops(1, 2)
    ok = eng.recognize_gray(gray, 8, prefixes=[[5, 6], None])
    assert ok[0][0, 1:3].tolist() == [5, 6]
    for bad, why in (([[5] * 8, None], "prefix_len"),            # P = L: outside 0 .. L - 1
                     ([[V], None], "vocabulary"), ([[-1], None], "vocabulary"),
                     ([[EOS, 5], None], "EOS"), ([None, [5, EOS, EOS]], "EOS")):
        with pytest.raises(MocrError, match=why):
            eng.recognize_gray(gray, 8, prefixes=bad)
    assert eng.recognize_gray(gray, 8, prefixes=[[5] * 7, [5, EOS]])[1].tolist() == [8, 3], "P = L - 1 and a final EOS are fine"
    ids = np.zeros((2, eng.spec.max_len), np.int32); lens = np.zeros(2, np.int32)
    pre = np.array([[5, 6], [7, 8]], np.int32); plen = np.array([2, 2], np.int32)
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)       # noqa: E731
    call = lambda p, q, ld: eng.lib.mocr_recognize_gray_host_prefix(eng._h, P(gray), 2, 8, P(ids), P(lens), *[None] * 6, P(p), P(q), ld)  # noqa: E731
    assert call(pre, plen, 2) == 0 and ids[1, 1:3].tolist() == [7, 8]
    assert call(pre, None, 2) != 0 and call(None, plen, 2) != 0, "exactly one of prefix / prefix_len null"
    assert call(pre, plen, 1) != 0, "prefix_len above prefix_ld"
    assert call(pre, np.array([-1, 0], np.int32), 2) != 0
    assert call(None, None, 0) == 0, "both null: the positions call"
    dg = torch.from_numpy(gray).cuda()
    d_ids = torch.zeros((2, eng.spec.max_len), dtype=torch.int32, device="cuda"); d_len = torch.zeros(2, dtype=torch.int32, device="cuda")
    eng.set_generate_max_length(8)
    with pytest.raises(MocrError, match="prefix_len"):
        eng.recognize_device(dg, 2, d_ids, d_len, prefixes=[[5] * 8, None])
    eng.recognize_device(dg, 2, d_ids, d_len, prefixes=[[5, 6], None])
    eng.synchronize()
    eng.set_generate_max_length(eng.spec.max_len)
    np.testing.assert_array_equal(d_ids.cpu().numpy(), ok[0])
    with pytest.raises(ValueError):
        eng.recognize_gray(gray, 8, prefixes=[[5]])


# ------------------------------------------------------------------------------------------------ 7. positions
def test_positions_of_a_self_prefixed_run():
    eng = su.score_engine("wide", "fp32")
    gray = crops(31, N_E2E)
    free = eng.recognize_gray(gray, LEN_E2E, alternatives=True, positions=True)
    pre = [free[0][b, 1:1 + P].tolist() for b, P in enumerate(SELF_LENS)]
    got = eng.recognize_gray(gray, LEN_E2E, alternatives=True, positions=True, prefixes=pre)
    _assert_same_run(got, free, "self-prefix with positions")
    assert np.abs(got[5][:, 1:LEN_E2E]).sum() > 0


# ------------------------------------------------------------------------------------------------ 8. the product surface
def test_product_surface_prefix():
    from PIL import Image
    from manga_ocr import MangaOcr
    m = MangaOcr(synthetic_seed=0, dtype="fp32", max_batch=8, lanes=1, batch_timeout_ms=2000)
    try:
        imgs = [Image.fromarray(g) for g in crops(77, 4)]
        free = m.recognize_batch_alternatives(imgs)
        # branch() fed back as a prefix: the row up to position 2, then the runner-up of position 2
        br = free[0].branch(2, 1)
        assert br == free[0].ids[1:3].tolist() + [int(free[0].alt_ids[2, 1])]
        re = m.recognize_batch_alternatives(imgs, prefix=[br, None, None, None])
        assert re[0].ids[1:4].tolist() == br and re[0].n_forced == 3 and re[1].n_forced == 0
        assert re[0].alt_ids[2, 0] == free[0].ids[3], "entry 0 of the forced step is the model's own pick"
        assert abs(re[0].logprobs[2] - free[0].alt_logprobs[2, 1]) <= 2 * FP32_LOGIT_TOL
        assert [r.text for r in re[1:]] == [r.text for r in free[1:]]
        own = free[1].ids[1:-1].tolist() if free[1].ids[-1] == EOS else free[1].ids[1:8].tolist()
        ch = next(t for t in (m.vocab.tokens[i] for i in free[3].ids[1:]) if len(t) == 1)
        with pytest.raises(ValueError):
            m.recognize_batch(imgs, prefix=[br])
        # what the engine is asked per batch: (crops, whether prefixes= was passed)
        seen, real = [], m.engine.recognize_images

        def spy(images, *a, **kw):
            seen.append((len(images), "prefixes" in kw))
            return real(images, *a, **kw)
        m.engine.recognize_images = spy
        # the plain callers' solo calls, each a batch of its own through the batcher (window 0 for these: nothing to wait for)
        m._batcher.timeout = 0.0
        solo = {k: m.recognize_scored(imgs[k]) for k in (1, 2, 3)}
        assert seen == [(1, False)] * 3, seen
        m._batcher.timeout = 2.0
        del seen[:]
        # ONE batch of eight threaded single-crop callers (it fills max_batch, so nobody waits for the window): prefixed and plain
        calls = [lambda: m.score_text(imgs[1], own), lambda: m.recognize_scored(imgs[0], prefix=br), lambda: m.recognize_scored(imgs[2]),
                 lambda: m.recognize(imgs[3]), lambda: m.recognize(imgs[0], prefix=br), lambda: m.recognize_alternatives(imgs[1]),
                 lambda: m(imgs[2]), lambda: m.recognize_scored(imgs[3], prefix=ch)]
        out = [None] * len(calls)

        def work(k):
            try:
                out[k] = calls[k]()
            except BaseException as exc:
                out[k] = exc
        ts = [threading.Thread(target=work, args=(k,)) for k in range(len(calls))]
        for t in ts:
            t.start()
        for t in ts:
            t.join(120)
        for o_ in out:
            assert o_ is not None and not isinstance(o_, BaseException), out
        assert seen == [(8, True)], f"the eight callers did not share one prefixed batch: {seen}"
        sc = out[0]                          # score_text: the row is the text plus EOS, all of it forced
        assert sc.ids.tolist() == [START] + own + [EOS] and sc.n_forced == len(own) + 1 and np.isfinite(sc.logprob) and sc.logprob < 0
        both = m.score_texts(imgs[:2], [own, own])
        assert abs(both[1].logprob - sc.logprob) <= 2 * FP32_LOGIT_TOL * (len(own) + 1) and both[0].n_forced == len(own) + 1
        assert out[1].ids.tolist() == re[0].ids.tolist() and out[1].n_forced == 3 and out[4] == re[0].text
        # the plain callers of the mixed batch get the ids of their solo calls (a text is a function of its ids)
        assert out[2].ids.tolist() == solo[2].ids.tolist() and out[5].ids.tolist() == solo[1].ids.tolist()
        assert out[6] == solo[2].text and out[3] == solo[3].text
        assert out[7].ids[1] == m.vocab.encode_chars(ch)[0] and out[7].n_forced == 1
    finally:
        m.close()
