"""-m gpu: the kernels of the repetition penalty (include/mocr.h, "repetition penalty"), exactly.

Everything runs through the new operator hooks - mocr_op_gemm_argmax_penalty, mocr_op_dec_token_penalty,
mocr_op_penalty_init - on operands coarse enough that every fp32 sum is exact (the practice of
tests/test_gpu_soft_automaton_kernels.py).  The penalty itself is one IEEE fp32 multiply or divide, which numpy's float32
arithmetic mirrors bit for bit (tests/penalty_util.py: pen32), so candidates, four best, target values and tokens are compared
exactly; the exp sums go through the merged logsumexp within the exact-input tolerance of tests/test_gpu_constraints.py."""
import numpy as np
import pytest

from gpu_util import report

import bias_util as bu
import constraint_util as cu
import ngram_util as nu
import penalty_util as pu
import score_util as su
from test_gpu_automaton import FILL, GUARD, SENT
from test_gpu_constraints import _f32, _i32, _t, _u32, lex_top
from test_gpu_ngram import _unpack

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

D, V, K4, EOS, START = 768, 6144, 4, 3, 2
MW = V // 32
NO_IDX = cu.NO_IDX
NONE = -1
P_OF_KIND = np.array([2.0, 1.3, 0.8, 2.0, 1.0, 1.3, 2.0, 1.3], np.float32)


# ------------------------------------------------------------------------------------------------ 1. the LM head
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("tile", [64, 128])
def test_penalty_lm_head_exact(dtype, tile):
    """mocr_op_gemm_argmax_penalty, M 40, N 256, K 768, ids / scored / alternatives forms, with and without a target column.
    GEMM row m is slot m of a permuted rowmap over M + 3 rows, so `seen` and p are read by ROW; M = 40 leaves rows >= M in the
    tile and has every swizzle phase (row >> 2) & 3.  Columns 100 (50.0), 200 (40.0), 37 (25.0), 150 (0.0) and 210 (-30.0) are
    constructed; every row also has a random half of the vocabulary seen, and the first and last column of every tile and both
    sides of a word boundary (0, 31, 32, 63, 64, 127, 128, 255).  Row kinds r % 8:
      0 p = 2, 100 and 200 seen: 25.0 ties with the unseen 37, 200 falls to 20 - the lower column wins;
      1 p = 1.3, 100 seen: the unpenalised winner falls below 200;
      2 p = 0.8, 200 seen: 40 / 0.8 = 50.0 ties with 100 - a tie made by a reward, the lower column wins;
      3 p = 2, 100 and 37 seen: 200 wins;
      4 p = 1: nothing changes;
      5 p = 1.3, 100 seen and outside the row's set: it stays -inf, nothing is NaN;
      6 p = 2, 100 seen with an edge weight of +32 on it: (50 + 32) / 2 = 41 wins, the order sequence_bias -> penalty;
      7 p = 1.3, a random half.
    cand_val / cand_idx, the four best and tgt_val equal the numpy mirror bit for bit; with p = 1 on every row every output
    is bit-identical to mocr_op_gemm_argmax_soft's; soft = NULL runs a penalty without any automaton."""
    N, M = 256, 40
    rs = np.random.RandomState(100 + tile)
    Mp = (M + tile - 1) // tile * tile
    nt, R = N // tile, M + 3
    rowmap = rs.permutation(R)[:M].astype(np.int32)
    kind = np.arange(R) % 8
    assert (kind[rowmap] != kind[:M]).any(), "a kernel reading seen / p by slot must fail"
    assert set(((np.arange(M) >> 2) & 3).tolist()) == {0, 1, 2, 3}
    A = np.zeros((Mp, D), np.float32)
    A[:M, :8] = rs.randint(-1, 2, size=(M, 8))
    W = np.zeros((N, D), np.float32)
    W[:, :8] = rs.randint(-2, 3, size=(N, 8)) / 4.0
    bias = (rs.randint(-16, 17, size=N) / 8.0).astype(np.float32)
    for c, b in ((100, 50.0), (200, 40.0), (37, 25.0), (150, 0.0), (210, -30.0)):
        W[c] = 0
        bias[c] = b
    logits = A[:M].astype(np.float64) @ W.astype(np.float64).T + bias
    assert (logits.astype(np.float32).astype(np.float64) == logits).all()
    corners = [0, 31, 32, 63, 64, 127, 128, 255, 150, 210]
    seen = rs.rand(R, N) < 0.5
    seen[:, corners] = True
    seen[:, [100, 200, 37]] = False
    seen[np.isin(kind, [0, 1, 3, 5, 6]), 100] = True
    seen[np.isin(kind, [0, 2]), 200] = True
    seen[kind == 3, 37] = True
    p = P_OF_KIND[kind]
    masks = np.ones((2, N), bool)
    masks[1] = rs.rand(N) < 0.5
    masks[1, [EOS, 200, 37, 0, 255]] = True
    masks[1, 100] = False
    set_of_row = (kind == 5).astype(np.int32)
    # one automaton of one state with an edge on 100 (+32) and one on 255 (-4); rows of kind 6 are in it
    aut = bu.SoftAutomaton({0: {100: 0, 255: 0}}, [0], {0: {100: 32.0, 255: -4.0}}, 0, 1)
    eb, et, en, acc, ew, dn, first = bu.pack_many([aut])
    state = np.where(kind == 6, first[0], NONE).astype(np.int32)
    ld = 1
    prefix = np.array([100, 0, 255, 150])[np.arange(R) % 4][:, None].astype(np.int32)
    plen = (np.arange(R) % 3 != 0).astype(np.int32)
    step = np.zeros(M, np.int32)

    rows = rowmap

    def reference(pp, with_soft):
        wl = logits + (np.where(kind[rows] == 6, 1.0, 0.0)[:, None] * bu.bias_of(aut, 0)[:N].astype(np.float64) if with_soft else 0.0)
        assert (wl.astype(np.float32).astype(np.float64) == wl).all()
        return pu.pen32(wl.astype(np.float32), seen[rows], pp[rows][:, None]).astype(np.float64)

    mask = masks[set_of_row[rows]]
    pl = reference(p, True)
    assert np.isfinite(pl).all()
    win = np.argmax(cu.masked(pl, mask), -1)
    free = np.argmax(cu.masked(logits, mask), -1)
    k_of = kind[rows]
    assert (free[k_of != 5] == 100).all()
    assert (win[k_of == 0] == 37).all() and (pl[k_of == 0][:, 100] == 25.0).all(), "kind 0: a tie made by the penalty, the lower column"
    assert (win[k_of == 1] == 200).all() and (win[k_of == 3] == 200).all()
    assert (win[k_of == 2] == 100).all() and (pl[k_of == 2][:, 200] == 50.0).all(), "kind 2: p < 1 lifts 200 to a tie, the lower column"
    assert (win[k_of == 4] == 100).all() and (win[k_of == 5] == 200).all() and not mask[k_of == 5][:, 100].any()
    assert (win[k_of == 6] == 100).all() and (pl[k_of == 6][:, 100] == 41.0).all(), "kind 6: (50 + 32) / 2, not 50 / 2 + 32"
    assert (pl[:, 150] == 0.0).all() and (pl[k_of == 0][:, 210] == -60.0).all() and (pl[k_of == 2][:, 210] == -24.0).all()

    eng = su.score_engine("wide", dtype)
    dA, dW, db = _t(A, dtype), _t(W, dtype), _f32(bias)
    table, d_sor, d_rowmap = _u32(cu.pack_sets(masks)), _i32(set_of_row), _i32(rowmap)
    tabs = dict(d_aut_state=_i32(state), d_edge_begin=_i32(eb), d_edge_token=_i32(et), d_edge_weight=_f32(ew))
    d_seen = _u32(cu.pack_sets(seen))

    def run(variant, target, pp=None, soft=True):
        cv = torch.full((M + GUARD, nt), float("nan"), device="cuda")
        ci = torch.full((M + GUARD, nt), SENT, dtype=torch.int32, device="cuda")
        cs = cv.clone() if variant >= 1 else None
        tv = torch.full((M + GUARD, nt, K4), float("nan"), device="cuda") if variant == 2 else None
        ti = torch.full((M + GUARD, nt, K4), SENT, dtype=torch.int32, device="cuda") if variant == 2 else None
        tg = torch.full((M + GUARD,), float("nan"), device="cuda") if target else None
        pre = (_i32(prefix), _i32(plen), ld, _i32(step), tg) if target else (None, None, 0, None, None)
        torch.cuda.synchronize()
        if pp is None:
            eng.op_gemm_argmax_soft(dA, dW, db, cv, ci, cs, tv, ti, M, N, D, tile, table, d_sor, d_rowmap, *pre, **(tabs if soft else {}))
        else:
            eng.op_gemm_argmax_penalty(dA, dW, db, cv, ci, cs, tv, ti, M, N, D, tile, table, d_sor, d_rowmap, *pre, **(tabs if soft else {}),
                                       d_seen_mask=d_seen, d_penalty_of_row=_f32(pp))
        out = [None if x is None else x.cpu().numpy() for x in (cv, ci, cs, tv, ti, tg)]
        for x in out:
            if x is not None:
                assert (np.isnan(x[M:]) if x.dtype == np.float32 else x[M:] == SENT).all(), "rows >= M written"
        return [None if x is None else x[:M] for x in out]

    tgt_rows = np.nonzero(plen[rows] > 0)[0]
    assert any(seen[rows[m], prefix[rows[m], 0]] and p[rows[m]] != 1 for m in tgt_rows), "a seen target column"
    worst = 0.0
    for with_soft in (True, False):
        pl = reference(p, with_soft)
        m64, idx64, s64 = cu.masked_tile_stats(pl, mask, tile)
        t3 = cu.masked(pl, mask).reshape(M, nt, tile)
        tile_lo = (np.arange(nt) * tile)[None, :, None]
        want_i = lex_top(t3) + tile_lo
        want_v = np.take_along_axis(t3, want_i - tile_lo, -1)
        want_i = np.where(np.isneginf(want_v), NO_IDX, want_i)
        want_tgt = np.full(M, np.nan)
        for m in tgt_rows:
            c = int(prefix[rows[m], 0])
            want_tgt[m] = pl[m, c] if mask[m, c] else -np.inf
        for variant in (0, 1, 2):
            for target in ((False,) if variant == 0 else (False, True)):
                gv, gi, gs, gtv, gti, gtg = run(variant, target, p, with_soft)
                what = f"form {variant} soft={with_soft}"
                assert not np.isnan(gv).any(), f"{what}: NaN"
                np.testing.assert_array_equal(gv.astype(np.float64), m64, err_msg=f"{what}: cand_val")
                np.testing.assert_array_equal(gi, idx64, err_msg=f"{what}: cand_idx")
                if variant == 2:
                    np.testing.assert_array_equal(gti, want_i, err_msg=f"{what}: top_idx")
                    np.testing.assert_array_equal(gtv.astype(np.float64), want_v, err_msg=f"{what}: top_val")
                if variant >= 1:
                    got_lse, ref_lse = cu.masked_merge_tiles(gv, gs), cu.masked_merge_tiles(m64, s64)
                    e32 = su.f32_lse_error(np.where(mask, pl, -1e30).astype(np.float32))
                    tol = 8 * np.maximum(e32, np.spacing(np.abs(ref_lse).astype(np.float32)).astype(np.float64))
                    err = np.abs(got_lse - ref_lse)
                    print(f"penalty LM head {dtype} tile={tile} {what}: logsumexp max err {err.max():.3e}, tol min {tol.min():.3e}", flush=True)
                    assert (err <= tol).all()
                    worst = max(worst, float((err / tol).max()))
                if target:
                    np.testing.assert_array_equal(gtg[tgt_rows].astype(np.float64), want_tgt[tgt_rows], err_msg=f"{what}: tgt_val")
                    assert np.isnan(gtg[plen[rows] == 0]).all(), "a row without a target had tgt_val written"
                # p = 1 on every row: the hook it extends, bit for bit
                ones = run(variant, target, np.ones(R, np.float32), with_soft)
                plain = run(variant, target, None, with_soft)
                for g, w_ in zip(ones, plain):
                    if g is not None:
                        np.testing.assert_array_equal(g.view(np.uint32), w_.view(np.uint32), err_msg=f"{what}: p = 1 differs from the _soft hook")
    report(f"gemm EPI_*_M PEN {dtype} tile={tile} M={M} N={N}: ids / scored / alternatives, with and without a target column, with and without "
           f"soft tables: candidates, four best and tgt_val == the numpy fp32 mirror bit for bit (winner that loses, negative, zero, ties made by "
           f"p = 2 and p = 0.8, seen column outside the set, tile and word corners, every swizzle phase, permuted rowmap, weight and penalty on "
           f"one column, seen target), logsumexp err / tol {worst:.3f}; p = 1 == the _soft hook bit for bit; rows >= M untouched")


# ------------------------------------------------------------------------------------------------ 2. the start of a batch
def test_penalty_init_kernel_exact():
    """mocr_op_penalty_init: every row's 192 words zero but the start token's bit; the row behind the batch untouched."""
    eng = su.score_engine("wide", "fp32")
    R = 5
    junk = np.random.RandomState(4).randint(0, 2 ** 32, size=(R + 1, MW), dtype=np.uint64).astype(np.uint32)
    d = _u32(junk)
    torch.cuda.synchronize()
    eng.op_penalty_init(d, R)
    got = d.cpu().numpy().view(np.uint32)
    want = np.zeros((R, V), bool)
    want[:, eng.spec.start_id] = True
    np.testing.assert_array_equal(got[:R], cu.pack_sets(want))
    np.testing.assert_array_equal(got[R], junk[R], err_msg="the row behind the batch was written")


# ------------------------------------------------------------------------------------------------ 3. the token kernel
# slot -> (row, p, n, the row's tokens so far, finished, prefix)
SLOTS = [
    (4, 2.0, 0, [START], False, None),              # free: 4001 (30) wins step 1; step 2 its 30 / 2 = 15 loses to 4002 (29)
    (0, 1.3, 0, [START], False, [4001, 4005]),      # forced 4001 then 4005: their bits are set although the picks differ
    (5, 1.0, 0, [START], False, None),              # p = 1 beside them: 4001 twice
    (2, 2.0, 0, [START, 50, EOS, 0], True, None),   # finished before: its words stay
    (1, 0.8, 1, [START, 60], False, None),          # p < 1 with n = 1: the reward cannot bring back a banned token
    (6, 2.0, 0, [START, 70], False, None),          # a seen negative winner-to-be and a seen zero (below)
]
TOP = [
    ([4001, 4002, 4003, 4004], [4001, 4002, 4003, 4004]),
    ([4002, 4001, 4003, 4004], [4001, 4005, 4003, 4004]),
    ([4001, 4002, 4003, 4004], [4001, 4002, 4003, 4004]),
    ([100, 101, 102, 103], [100, 101, 102, 103]),
    ([60, 4002, 4003, 4004], [60, 4002, 4003, 4004]),
    ([70, 4002, 4003, 4004], [4002, 70, 4003, 4004]),
]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_penalty_token_step_exact(dtype):
    """mocr_op_dec_token_penalty without any automaton, two consecutive steps, the alternatives form (with the forced
    prefixes) on the slab path (one slab) and on the candidate path (tile 64: its inputs are the tile statistics of the
    penalised, masked logits, as the PEN LM head leaves them), and the ids form on the slab path.  Six slots over seven rows
    through a permuted rowmap; the rows' first seen words come from mocr_op_penalty_init.  ids, steps, finished, lengths, the
    192 mask words and the 192 seen words of every row are exact against numpy and equal on both paths; the second step's pick
    reflects the first step's bit; a forced token's bit is set; a finished row's words are unchanged; with p = 1 on every row
    every output is bit-identical to mocr_op_dec_token_soft's."""
    eng = su.score_engine("wide", dtype)
    n, R, ids_ld, max_len = len(SLOTS), 7, 8, 8
    rowmap = np.array([s[0] for s in SLOTS], np.int32)
    base = np.ones((1, V), bool)
    ngr, pen = np.zeros(R + 1, np.int32), np.ones(R + 1, np.float32)
    ids = np.full((R + 1, ids_ld), FILL, np.int32)
    step, finished, lens = np.zeros(n, np.int32), np.zeros(R + 1, np.int32), np.full(R + 1, max_len, np.int32)
    ld = 4
    prefix, plen = np.zeros((R + 1, ld), np.int32), np.zeros(R + 1, np.int32)
    rs = np.random.RandomState(77)
    junk = rs.randint(0, 2 ** 32, size=(R + 1, MW), dtype=np.uint64).astype(np.uint32)
    d_seen0 = _u32(junk)
    torch.cuda.synchronize()
    eng.op_penalty_init(d_seen0, R)
    seen0 = d_seen0.cpu().numpy().view(np.uint32).copy()
    rm0 = junk.copy()
    for s, (row, p_, g, hist, fin, pre) in enumerate(SLOTS):
        pen[row], ngr[row] = p_, g
        ids[row, :len(hist)] = hist
        step[s] = len(hist) - 1
        for tok in hist[1:]:
            if tok != 0:
                seen0[row, tok >> 5] |= np.uint32(1 << (tok & 31))
        if fin:
            finished[row] = 1; lens[row] = hist.index(EOS) + 1
        else:
            rm0[row] = cu.pack_sets(nu.step_mask(hist, g, base[0])[None])[0]
        if pre:
            prefix[row, len(hist) - 1:len(hist) - 1 + len(pre)] = pre; plen[row] = len(hist) - 1 + len(pre)
    for tok in (5000, 5001):                                 # row 6 has also seen a negative and a zero logit
        seen0[6, tok >> 5] |= np.uint32(1 << (tok & 31))
    seen_fin = seen0[2].copy()

    def logits(k):
        lg = (np.round(rs.standard_normal((n, V)) * 3 * 256) / 256)
        for s in range(n):
            lg[s, TOP[s][k]] = [30.0, 29.0, 28.0, 27.0]
        lg[5, 5000], lg[5, 5001] = -7.5, 0.0
        return lg.astype(np.float32)

    def forced_of(state):
        _, step_, fin_, _, _, _ = state
        return {s: int(prefix[rowmap[s], step_[s]]) for s in range(n) if step_[s] < plen[rowmap[s]] and not fin_[rowmap[s]]}

    def penalised(lg, state, pp):
        return pu.pen32(lg, _unpack(state[5][rowmap]), pp[rowmap][:, None])

    def inputs(path, lg, pl, mk, forced):
        tgt = np.full(n + GUARD, np.nan, np.float32)
        if path == "slabs1":                                 # the kernel penalises itself: raw logits in
            r2 = np.random.RandomState(5)
            bias = (r2.randint(-100, 100, V) / 64.0).astype(np.float64)
            parts = (lg.astype(np.float64) - bias)[None]
            assert (parts.astype(np.float32).astype(np.float64) == parts).all()
            return dict(slabs=_f32(parts), nslab=1, vbias=_f32(bias)), None, None, None, _f32(tgt)
        tile = 64
        nt = V // tile
        m, idx, s_ = cu.masked_tile_stats(pl.astype(np.float64), mk, tile)
        t3 = cu.masked(pl.astype(np.float64), mk).reshape(n, nt, tile)
        ti = lex_top(t3)
        tv = np.take_along_axis(t3, ti, -1)
        ti = np.where(np.isneginf(tv), NO_IDX, ti + (np.arange(nt) * tile)[None, :, None])
        for s, tok in forced.items():
            tgt[s] = pl[s, tok] if mk[s, tok] else -np.inf
        return dict(cand_val=_f32(m), cand_idx=_i32(idx), ncand=nt), _f32(s_), _f32(tv), _i32(ti), _f32(tgt)

    def run(path, variant, lg, state, pp, hook="penalty"):
        ids_, step_, fin_, len_, rm_, seen_ = state
        kw, cand_sum, top_val, top_idx, tgt = inputs(path, lg, penalised(lg, state, pp), _unpack(rm_[rowmap]), forced_of(state) if variant == 2 else {})
        d = dict(ids=_i32(ids_), step=_i32(step_), finished=_i32(fin_), len=_i32(len_), n_unfinished=_i32([8, SENT]),
                 rowmap=_i32(rowmap), x_f32=torch.full((n + GUARD, D), float("nan"), device="cuda"),
                 x_t=torch.full((n + GUARD, D), float("nan"), device="cuda", dtype=torch.bfloat16 if dtype == "bf16" else torch.float32))
        sc = torch.full((R + 1, ids_ld), float("nan"), device="cuda") if variant == 2 else None
        ai = torch.full((R + 1, ids_ld, K4), SENT, dtype=torch.int32, device="cuda") if variant == 2 else None
        al = torch.full((R + 1, ids_ld, K4), float("nan"), device="cuda") if variant == 2 else None
        d_rm, d_seen = _u32(rm_), _u32(seen_)
        pre = (_i32(prefix), _i32(plen), ld, tgt) if variant == 2 else (None, None, 0, None)
        args = (cand_sum if variant == 2 else None, sc, top_val if variant == 2 else None, top_idx if variant == 2 else None, ai, al, d_rm,
                _i32(np.arange(R + 1)), d_rm, _u32(cu.pack_sets(base)), _i32(np.zeros(R + 1)), _i32(ngr), *pre) + (None,) * 8
        torch.cuda.synchronize()
        if hook == "penalty":
            eng.op_dec_token_penalty(*args, d_seen, _f32(pp), first=0, n=n, ids_ld=ids_ld, max_len=max_len, n_real=n, **d, **kw)
        else:
            eng.op_dec_token_soft(*args, first=0, n=n, ids_ld=ids_ld, max_len=max_len, n_real=n, **d, **kw)
        o = {k: v.cpu().numpy() for k, v in d.items() if k in ("ids", "step", "finished", "len", "x_f32")}
        return ((o["ids"], o["step"], o["finished"], o["len"], d_rm.cpu().numpy().view(np.uint32), d_seen.cpu().numpy().view(np.uint32)),
                None if ai is None else ai.cpu().numpy(), None if sc is None else sc.cpu().numpy(),
                None if al is None else al.cpu().numpy(), o["x_f32"])

    def reference(state, lg, pp, with_prefix):
        ids_, step_, fin_, len_, rm_, seen_ = (a.copy() for a in state)
        pl = penalised(lg, state, pp).astype(np.float64)
        forced = forced_of(state) if with_prefix else {}
        want4, want_lp = np.full((n, K4), -1), np.full(n, np.nan)
        for s in range(n):
            row, t = rowmap[s], step_[s]
            eff = _unpack(rm_[row])
            was = bool(fin_[row])
            tok = 0 if was else int(np.argmax(np.where(eff, pl[s], -np.inf)))
            if not was:
                want4[s] = cu.masked_top(pl[s], eff)[0]
            tok = forced.get(s, tok)
            ids_[row, t + 1] = tok
            step_[s] = t + 1
            if was:
                continue
            want_lp[s] = cu.masked_log_softmax64(pl[s], eff)[tok]
            seen_[row, tok >> 5] |= np.uint32(1 << (tok & 31))
            if tok == EOS or t + 2 >= max_len:
                fin_[row] = 1; len_[row] = t + 2
            elif ngr[row] > 0:
                rm_[row] = cu.pack_sets(nu.step_mask(ids_[row, :t + 2], int(ngr[row]), base[0])[None])[0]
        return (ids_, step_, fin_, len_, rm_, seen_), want4, want_lp

    names = ("ids", "step", "finished", "len", "row_mask", "seen_mask")
    LG = [logits(0), logits(1)]
    state2 = state0 = (ids, step, finished, lens, rm0, seen0)
    ones = np.ones(R + 1, np.float32)
    for k in range(2):
        want2, want4, want_lp = reference(state2, LG[k], pen, True)
        want0, _, _ = reference(state0, LG[k], pen, False)
        got2, ai, sc, al, x2 = run("slabs1", 2, LG[k], state2, pen)
        got2c, aic, scc, alc, x2c = run("cand64", 2, LG[k], state2, pen)
        got0, _, _, _, _ = run("slabs1", 0, LG[k], state0, pen)
        for name, g2, gc, w2, g0, w0 in zip(names, got2, got2c, want2, got0, want0):
            np.testing.assert_array_equal(g2, w2, err_msg=f"step {k + 1}, alternatives form, slab path: {name}")
            np.testing.assert_array_equal(gc, w2, err_msg=f"step {k + 1}, alternatives form, candidate path: {name}")
            np.testing.assert_array_equal(g0, w0, err_msg=f"step {k + 1}, ids form: {name}")
        np.testing.assert_array_equal(x2[:n].view(np.uint32), x2c[:n].view(np.uint32), err_msg="the two paths feed back different embeddings")
        live = state2[2][rowmap] == 0
        for a4, lp, path in ((ai, sc, "slab"), (aic, scc, "candidate")):
            a4 = a4[rowmap, state2[1] + 1]
            np.testing.assert_array_equal(a4[live], want4[live], err_msg=f"{path} path: alt_ids is not the top four of the penalised, masked row")
            assert (a4[~live] == -1).all()
            got_lp = lp[rowmap, state2[1] + 1].astype(np.float64)
            print(f"penalty token step {dtype} {path} step {k + 1}: score max err {np.abs(got_lp[live] - want_lp[live]).max():.3e}", flush=True)
            assert np.abs(got_lp[live] - want_lp[live]).max() <= 5e-6, "the stored token's log-probability of the penalised, masked row (TOKEN_SCORE_TOL)"
        # p = 1 on every row: the hook it extends, bit for bit, on both paths and in both forms
        for path, variant, st_ in (("slabs1", 2, state2), ("cand64", 2, state2), ("slabs1", 0, state0)):
            a, b = run(path, variant, LG[k], st_, ones), run(path, variant, LG[k], st_, ones, hook="soft")
            for name, ga, gb in zip(names[:5], a[0], b[0]):
                np.testing.assert_array_equal(ga, gb, err_msg=f"p = 1, {path} form {variant}: {name} differs from the _soft hook")
            for ga, gb in zip(a[1:], b[1:]):
                if ga is not None:
                    np.testing.assert_array_equal(ga.view(np.uint32), gb.view(np.uint32), err_msg=f"p = 1, {path} form {variant}: differs from the _soft hook")
        state2, state0 = got2, got0
    ids2, _, fin2, len2, rm2, seen2 = state2
    bit = lambda row, tok: bool((seen2[row, tok >> 5] >> np.uint32(tok & 31)) & np.uint32(1))
    assert ids2[4, 1:3].tolist() == [4001, 4002], "slot 0: the second step's pick reflects the first step's bit"
    assert ids2[0, 1:3].tolist() == [4001, 4005] and bit(0, 4001) and bit(0, 4005) and not bit(0, 4002), "slot 1: forced tokens' bits, not the picks'"
    assert ids2[5, 1:3].tolist() == [4001, 4001] and state0[0][0, 1:3].tolist() == [4002, 4001], "p = 1 repeats; the ids form has no prefix"
    np.testing.assert_array_equal(seen2[2], seen_fin, err_msg="a finished row's seen words were rewritten")
    np.testing.assert_array_equal(seen2[R], junk[R], err_msg="the seen row behind the batch was written")
    np.testing.assert_array_equal(seen2[3], seen0[3], err_msg="a row no slot decodes had its seen words written")
    assert ids2[1, 2:4].tolist() == [4002, 4003], "slot 4: n = 1 bans 60 whatever p < 1 makes of it"
    assert ids2[6, 2:4].tolist() == [4002, 4003], "slot 5: 70 / 2 loses, then 4002 / 2 loses"
    assert bit(4, START) and bit(4, 4001) and bit(4, 4002) and int(sum(bin(int(w)).count("1") for w in seen2[4])) == 3
    report(f"dec_token PEN {dtype}: two consecutive steps, slab and candidate path, alternatives and ids form: ids, states, mask and seen words of "
           f"7 rows exact against the numpy fp32 mirror and equal on both paths (free and forced tokens' bits, finished row untouched, n = 1 "
           f"beside p < 1, negative and zero seen logits); p = 1 == mocr_op_dec_token_soft bit for bit; penalty_init leaves the start bit")
