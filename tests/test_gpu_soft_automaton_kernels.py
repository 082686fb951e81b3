"""-m gpu: the kernels of the soft token automata (include/mocr.h, "soft token automata"), exactly.

Everything runs through the new operator hooks - mocr_op_gemm_argmax_soft, mocr_op_dec_token_soft,
mocr_op_automaton_init_soft - on operands coarse enough that every fp32 sum is exact (small integers and dyadic fractions, the
practice of tests/test_gpu_automaton.py), so the outputs are compared bit for bit with numpy (tests/bias_util.py: an automaton
is a dictionary of dictionaries).  The one output that is not a sum - the LM head's exp sums - is compared through the merged
logsumexp, within the tolerance tests/test_gpu_constraints.py uses for exact inputs."""
import numpy as np
import pytest

from gpu_util import report

import automaton_util as au
import bias_util as bu
import constraint_util as cu
import score_util as su
from test_gpu_automaton import FILL, GUARD, K_LOOP, SENT, _u8
from test_gpu_constraints import _bits, _f32, _i32, _t, _u32, lex_top
from test_gpu_ngram import _unpack

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

D, V, K4, EOS, START = 768, 6144, 4, 3, 2
MW = V // 32
NO_IDX = cu.NO_IDX
NONE, DEAD = au.NONE, au.DEAD
LAST = V - 1                        # the last non-EOS column


# ------------------------------------------------------------------------------------------------ 1. the LM head
def _head_automata():
    """one-state automata of the LM-head test behind each other (the head reads a state's edges and weights, nothing else):
    0 no edge; 1 one edge; 2 300 edges; 3 all 6,143 edges; 4 edges on the first and last column of a thread's group (16
    columns on the 64 tile, 64 on the 128 tile), of a tile, on column 0 and on the last column; 5 a negative weight on the
    unweighted winner (column 1000) that moves the winner to column 3000, another tile; 6 a weight on column 2000, which set
    1 leaves out"""
    rs = np.random.RandomState(11)

    def one(edges):
        return bu.SoftAutomaton({0: {t: 0 for t in edges}}, [0], {0: {t: float(w) for t, w in edges.items()}}, 0, 1)
    e300 = {int(t): int(w) / 8.0 for t, w in zip(sorted(rs.choice(np.setdiff1d(np.arange(V), [EOS]), 300, replace=False)), rs.randint(-64, 65, 300))}
    eall = {t: int(w) / 8.0 for t, w in zip(range(V), rs.randint(-80, 81, V)) if t != EOS}
    corners = {0: 60.0, 15: 61.0, 16: -3.5, 63: 59.0, 64: 58.5, 127: 62.0, 128: 57.0, 6080: 56.0, 6143 - 16: 55.5, LAST: 100.0}
    auts = [one({}), one({4321: 70.0}), one(e300), one(eall), one(corners), one({1000: -64.0}), one({2000: 100.0})]
    return auts, bu.pack_many(auts)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("M", [70, 130])
def test_soft_lm_head_exact(dtype, tile, M):
    """mocr_op_gemm_argmax_soft, N 6144, K 768, ids / scored / alternatives forms, with and without a target column.  GEMM row
    m is slot m of a permuted rowmap over M + 3 rows; row r is in the state of automaton r % 9 of _head_automata (7: no
    automaton, 8: dead), under set 1 (column 2000 and a random half banned) when r % 9 == 6 or r % 4 == 0.  M = 70 / 130 leaves
    one ragged tile, so rows >= M exist and every swizzle phase (row >> 2) & 3 occurs.  Integer operands: logits and weights are
    dyadic, every sum exact.  cand_val / cand_idx, the four best and tgt_val equal numpy's on logit + weight bit for bit; the
    merged logsumexp is within the exact-input tolerance of tests/test_gpu_constraints.py; with every state NONE, and with
    the tables null, every output is bit-identical to mocr_op_gemm_argmax_target's."""
    eng = su.score_engine("wide", dtype)
    auts, (eb, et, en, acc, ew, dn, first) = _head_automata()
    rs = np.random.RandomState(17 * M + tile)
    Mp = (M + tile - 1) // tile * tile
    nt, R = V // tile, M + 3
    rowmap = rs.permutation(R)[:M].astype(np.int32)
    kind = np.arange(R) % 9
    state = np.array([first[k] if k < 7 else (NONE if k == 7 else DEAD) for k in kind], np.int32)
    set_of_row = ((kind == 6) | (np.arange(R) % 4 == 0)).astype(np.int32)
    assert (kind[rowmap] != kind[:M]).any(), "a kernel reading the state by slot must fail"
    A = np.zeros((Mp, D), np.float32)
    A[:M, :8] = rs.randint(-1, 2, size=(M, 8))
    W = np.zeros((V, D), np.float32)
    W[:, :8] = rs.randint(-2, 3, size=(V, 8)) / 4.0
    bias = (rs.randint(-16, 17, size=V) / 8.0).astype(np.float32)
    bias[1000], bias[3000] = 50.0, 40.0                       # every row's unweighted winner and runner-up
    logits = A[:M].astype(np.float64) @ W.astype(np.float64).T + bias
    assert (logits.astype(np.float32).astype(np.float64) == logits).all() and np.abs(logits).max() < 64
    masks = np.ones((2, V), bool)
    masks[1] = rs.rand(V) < 0.5
    masks[1, [EOS, 1000, 3000, 15, LAST, 4321]] = True
    masks[1, 2000] = False
    # forced targets: slot m with step < prefix_len has target prefix[row][step]; 15 and LAST carry a weight in state 4
    ld = 2
    prefix = np.stack([np.array([15, LAST, 1000, 2000])[np.arange(R) % 4], np.full(R, 77)], 1).astype(np.int32)
    plen = (np.arange(R) % 3 != 0).astype(np.int32)
    step = np.zeros(M, np.int32)
    # the reference: logit + weight in fp32 (exact), masked
    rows = rowmap
    wl = np.stack([logits[m] + (auts[kind[r]].bias(0).astype(np.float64) if kind[r] < 7 else 0.0) for m, r in enumerate(rows)])
    assert (wl.astype(np.float32).astype(np.float64) == wl).all()
    mask = masks[set_of_row[rows]]
    m64, idx64, s64 = cu.masked_tile_stats(wl, mask, tile)
    t3 = cu.masked(wl, mask).reshape(M, nt, tile)
    tile_lo = (np.arange(nt) * tile)[None, :, None]
    want_i = lex_top(t3) + tile_lo
    want_v = np.take_along_axis(t3, want_i - tile_lo, -1)
    want_i = np.where(np.isneginf(want_v), NO_IDX, want_i)
    tgt_rows = np.nonzero(plen[rows] > 0)[0]
    want_tgt = np.full(M, np.nan)
    for m in tgt_rows:
        c = int(prefix[rows[m], 0])
        want_tgt[m] = wl[m, c] if mask[m, c] else -np.inf
    # what the table proves
    free = np.argmax(cu.masked(logits, mask), -1)
    got_w = np.argmax(cu.masked(wl, mask), -1)
    assert (free == 1000).all() and (got_w[kind[rows] == 5] == 3000).all() and 1000 // tile != 3000 // tile
    assert (got_w[kind[rows] == 6] == 1000).all() and not mask[kind[rows] == 6][:, 2000].any(), "the weighted masked column stays out"
    assert (got_w[kind[rows] == 4] == LAST).all() and (got_w[kind[rows] == 1] == 4321).all()
    assert any(kind[rows[m]] == 4 and prefix[rows[m], 0] in (15, LAST) for m in tgt_rows), "a target column that carries a weight"
    ks = set(kind[rows[:tile]].tolist())                     # NONE and DEAD rows share a tile with soft rows
    assert {7, 8} <= ks and {2, 3, 4} <= ks

    dA, dW, db = _t(A, dtype), _t(W, dtype), _f32(bias)
    table, d_sor, d_rowmap = _u32(cu.pack_sets(masks)), _i32(set_of_row), _i32(rowmap)
    tabs = dict(d_edge_begin=_i32(eb), d_edge_token=_i32(et), d_edge_weight=_f32(ew))

    def run(variant, target, states, soft=True):
        cv = torch.full((M + GUARD, nt), float("nan"), device="cuda")
        ci = torch.full((M + GUARD, nt), SENT, dtype=torch.int32, device="cuda")
        cs = cv.clone() if variant >= 1 else None
        tv = torch.full((M + GUARD, nt, K4), float("nan"), device="cuda") if variant == 2 else None
        ti = torch.full((M + GUARD, nt, K4), SENT, dtype=torch.int32, device="cuda") if variant == 2 else None
        tg = torch.full((M + GUARD,), float("nan"), device="cuda") if target else None
        pre = (_i32(prefix), _i32(plen), ld, _i32(step), tg) if target else (None, None, 0, None, None)
        torch.cuda.synchronize()
        if soft:
            eng.op_gemm_argmax_soft(dA, dW, db, cv, ci, cs, tv, ti, M, V, D, tile, table, d_sor, d_rowmap, *pre, d_aut_state=_i32(states), **tabs)
        else:
            eng.op_gemm_argmax_target(dA, dW, db, cv, ci, cs, tv, ti, M, V, D, tile, table, d_sor, d_rowmap, *pre)
        out = [None if x is None else x.cpu().numpy() for x in (cv, ci, cs, tv, ti, tg)]
        for x in out:
            if x is not None:
                assert (np.isnan(x[M:]) if x.dtype == np.float32 else x[M:] == SENT).all(), "guard rows written"
        return [None if x is None else x[:M] for x in out]

    worst = 0.0
    for variant in (0, 1, 2):
        for target in ((False,) if variant == 0 else (False, True)):
            gv, gi, gs, gtv, gti, gtg = run(variant, target, state)
            np.testing.assert_array_equal(gv.astype(np.float64), m64, err_msg=f"form {variant}: cand_val")
            np.testing.assert_array_equal(gi, idx64, err_msg=f"form {variant}: cand_idx")
            if variant == 2:
                np.testing.assert_array_equal(gti, want_i, err_msg="top_idx is not the lexicographic top four of logit + weight")
                np.testing.assert_array_equal(gtv.astype(np.float64), want_v)
            if variant >= 1:
                got_lse, ref_lse = cu.masked_merge_tiles(gv, gs), cu.masked_merge_tiles(m64, s64)
                e32 = su.f32_lse_error(np.where(mask, wl, -1e30).astype(np.float32))
                tol = 8 * np.maximum(e32, np.spacing(np.abs(ref_lse).astype(np.float32)).astype(np.float64))
                err = np.abs(got_lse - ref_lse)
                print(f"soft LM head {dtype} tile={tile} M={M} form {variant}: logsumexp max err {err.max():.3e}, tol min {tol.min():.3e}", flush=True)
                assert (err <= tol).all()
                worst = max(worst, float((err / tol).max()))
            if target:
                np.testing.assert_array_equal(gtg[tgt_rows].astype(np.float64), want_tgt[tgt_rows], err_msg="tgt_val")
                assert np.isnan(gtg[plen[rows] == 0]).all(), "a row without a target had tgt_val written"
            # no state at all, and no tables at all: the call below it, bit for bit
            plain = run(variant, target, None, soft=False)
            for name, states, soft in (("every state NONE", np.full(R, NONE), True), ("tables null", None, False)):
                if name == "tables null":
                    eng_out = [None] * 6
                    cv = torch.full((M + GUARD, nt), float("nan"), device="cuda")
                    ci = torch.full((M + GUARD, nt), SENT, dtype=torch.int32, device="cuda")
                    cs = cv.clone() if variant >= 1 else None
                    tv = torch.full((M + GUARD, nt, K4), float("nan"), device="cuda") if variant == 2 else None
                    ti = torch.full((M + GUARD, nt, K4), SENT, dtype=torch.int32, device="cuda") if variant == 2 else None
                    tg = torch.full((M + GUARD,), float("nan"), device="cuda") if target else None
                    pre = (_i32(prefix), _i32(plen), ld, _i32(step), tg) if target else (None, None, 0, None, None)
                    eng.op_gemm_argmax_soft(dA, dW, db, cv, ci, cs, tv, ti, M, V, D, tile, table, d_sor, d_rowmap, *pre)
                    eng_out = [None if x is None else x.cpu().numpy()[:M] for x in (cv, ci, cs, tv, ti, tg)]
                else:
                    eng_out = run(variant, target, states)
                for g, w_ in zip(eng_out, plain):
                    if g is not None:
                        np.testing.assert_array_equal(g.view(np.uint32), w_.view(np.uint32), err_msg=f"{name}: differs from the _target hook")
    report(f"gemm EPI_*_M SOFT {dtype} tile={tile} M={M}: ids / scored / alternatives, with and without a target column: candidates, four best and "
           f"tgt_val == numpy on logit + weight bit for bit (no edge, 1, 300, 6,143 edges, group / tile corners, winner moved to another tile, "
           f"weighted masked column, weighted target, NONE / DEAD rows in every tile, permuted rowmap), logsumexp err / tol {worst:.3f}; "
           f"states NONE and tables null == the _target hook bit for bit")


# ------------------------------------------------------------------------------------------------ 2. the start of a batch
def _token_automata():
    """the automata of the init and token-step tests behind each other:
    0 three states, 0 and 1 open (default 0), 2 closed, accepting, without edges: weights +12 on 100 (-> 1), -60 on 101 in
      state 0, +35 on 102 (-> 2) in state 1;
    1 the closed digit loop of tests/test_gpu_automaton.py, no weights: a hard automaton inside a soft launch;
    2 the universal open automaton (one accepting open state, no edge);
    3 one open state with 300 weighted edges on the tokens 1000 .. 1299 - four in a row of every float4 a thread holds;
    4 one open state that does not accept: A = everything but EOS;
    5 three open accepting states whose default edges carry MOCR_DEFAULT_FALLBACK (default 0): 0 -100-> 1, 0 -300-> 2,
      1 -102-> 0, state 2 without edges - a token without an edge is looked up in state 0's edges"""
    a0 = bu.SoftAutomaton({0: {100: 1, 101: 0}, 1: {102: 2}}, [0, 2], {0: {100: 12.0, 101: -60.0}, 1: {102: 35.0}}, {0: 0, 1: 0}, 3)
    a3 = bu.SoftAutomaton({0: {t: 0 for t in range(1000, 1300)}}, [0], {0: {t: ((t * 7) % 33 - 16) / 8.0 for t in range(1000, 1300)}}, 0, 1)
    a3.weights[0][1100] = 8.0
    a5 = bu.SoftAutomaton({0: {100: 1, 300: 2}, 1: {102: 0}}, [0, 1, 2], None, 0, 3, fallback=True)
    auts = [a0, au.loop(K_LOOP), bu.universal_open(), a3, bu.SoftAutomaton({}, [], None, 0, 1), a5]
    return auts, bu.pack_many(auts)


def test_soft_automaton_init_kernel_exact():
    """mocr_op_automaton_init_soft, 9 rows (the last under a start state whose default edge carries MOCR_DEFAULT_FALLBACK:
    open like any other) and a guard row: open start states (accepting and not) under both base sets and
    n = 0 / 1, the closed loop, a row without an automaton, the dead-end rule on an open state ({200} minus nothing is fine,
    a set of EOS alone under a non-accepting open state is empty -> {EOS}); with d_default_next null it is
    mocr_op_automaton_init.  Masks and states exact."""
    eng = su.score_engine("wide", "fp32")
    auts, (eb, et, en, acc, ew, dn, first) = _token_automata()
    R = 9
    base3 = np.ones((3, V), bool)
    base3[1] = np.random.RandomState(3).rand(V) < 0.5
    base3[1, [START, EOS]] = True
    base3[2] = cu.mask_of([])                               # EOS alone
    which = [0, 2, 2, None, 1, 4, 4, 3, 5]
    sor = np.array([0, 1, 0, 1, 0, 2, 1, 0, 1], np.int32)
    ngr = np.array([0, 0, 1, 1, 2, 0, 1, 3, 0], np.int32)
    assert dn[first[5]] == (first[5] | bu.FALLBACK)
    abase = np.array([-1 if k is None else first[k] for k in which] + [first[0]], np.int32)
    junk = np.random.RandomState(4).randint(0, 2 ** 32, size=(R + 1, MW), dtype=np.uint64).astype(np.uint32)
    want = np.stack([au.step_mask(None if k is None else auts[k], 0, [START], int(ngr[r]), base3[sor[r]]) for r, k in enumerate(which)])
    for soft in (True, False):
        d_rm, d_state = _u32(junk), _i32(np.full(R + 1, SENT))
        torch.cuda.synchronize()
        eng.op_automaton_init_soft(d_rm, _u32(cu.pack_sets(base3)), _i32(sor), _i32(ngr), R, _i32(eb), _i32(et), _u8(acc), _i32(abase), d_state,
                                   _i32(dn) if soft else None)
        got, state = d_rm.cpu().numpy().view(np.uint32), d_state.cpu().numpy()
        if soft:
            np.testing.assert_array_equal(got[:R], cu.pack_sets(want))
        else:       # the hard reading of the same tables: an open state is a state with its edges alone
            hard = [None if k is None else au.Automaton(auts[k].trans, auts[k].accepting, auts[k].n_states) for k in which]
            np.testing.assert_array_equal(got[:R], cu.pack_sets(np.stack([au.step_mask(hard[r], 0, [START], int(ngr[r]), base3[sor[r]])
                                                                          for r in range(R)])))
        np.testing.assert_array_equal(got[R], junk[R], err_msg="the mask row behind the batch was written")
        np.testing.assert_array_equal(state, [NONE if k is None else first[k] for k in which] + [SENT])
    assert want[0].sum() == V and want[1].sum() == base3[1].sum() and want[2].sum() == V - 1 and not want[2, START]
    assert want[5].sum() == 1 and want[5, EOS], "row 5: a non-accepting open state under {EOS} -> the dead-end rule"
    assert want[6].sum() == base3[1].sum() - 2 and not want[6, EOS] and want[4].sum() == len(K_LOOP)
    assert want[8].sum() == base3[1].sum(), "row 8: the fallback bit leaves the start state open"


# ------------------------------------------------------------------------------------------------ 3. the token kernel
def _token_case():
    auts, packed = _token_automata()
    # slot -> (row, automaton, n, base set, the row's tokens so far, finished, prefix)
    slots = [
        (5, 0, 0, 0, [START], False, None),                       # weights decide: 100 (+12) beats the unweighted winner, then 102 (+35), then {EOS}
        (2, 0, 1, 0, [START, 50], False, None),                   # the unweighted winner 101 loses 60: 5000 wins and walks the default edge; n = 1
        (7, 1, 0, 0, [START], False, [100, 4000]),                # the closed loop: forced onto an edge, then off it -> DEAD, {EOS}
        (0, 2, 2, 1, [START, 60, 61, 60], False, None),           # universal open, base set 1, n = 2: 61 is banned behind 60
        (9, 2, 3, 0, [START, 70, 71, 72, 70, 71], False, None),   # ... n = 3: 72 is banned behind 70 71
        (1, 0, 0, 0, [START, 100], False, [4000]),                # state 1, forced a token without an edge: the default edge, not DEAD
        (8, 1, 0, 0, [START, 100, EOS, 0], True, None),           # finished: untouched
        (6, None, 0, 1, [START, 20], False, None),                # no automaton, n = 0: the mask is left alone
        (3, 4, 1, 2, [START, 200], False, None),                  # open, not accepting, set {200, EOS}, n = 1: nothing left -> {EOS}
        (10, 3, 0, 0, [START], False, None),                      # 300 weighted edges: 1100 (+8) wins
        (11, 5, 0, 0, [START, 100], False, None),                 # fallback HIT: state 1 has no edge on 300, state 0 has: -> 2; 100 from 2 -> 1; 300 -> 2
        (12, 5, 0, 0, [START, 100], False, None),                 # fallback MISS: 4001 has no edge in 1 nor in 0 -> 0; 102 from 0: again -> 0; 300 -> 2
    ]
    top = [
        ([4001, 4002, 4003, 100], [4002, 102, 4003, 4004], [4001, 4002, 4003, 4004]),
        ([101, 5000, 4002, 4003], [5000, 101, 5001, 4003], [5002, 5000, 101, 50]),
        ([101, 102, 103, 100], [101, 102, 103, 100], [101, 102, 103, 100]),
        ([61, 62, 63, 64], [62, 60, 63, 64], [99, 61, 63, 64]),
        ([72, 73, 74, 75], [70, 74, 75, 76], [71, 74, 75, 76]),
        ([4005, 102, 4003, 4004], [4001, 100, 4003, 4004], [4001, 4002, 102, 4004]),
        ([100, 101, 102, 103], [100, 101, 102, 103], [100, 101, 102, 103]),
        ([21, 22, 23, 24], [22, 23, 24, 25], [99, 22, 23, 24]),
        ([200, 4001, 4002, 4003], [200, 4001, 4002, 4003], [200, 4001, 4002, 4003]),
        ([4001, 4002, 1100, 4003], [4001, 4002, 1100, 4003], [4001, 1100, 4002, 4003]),
        ([300, 4001, 4002, 4003], [100, 4001, 4002, 4003], [300, 4001, 4002, 4003]),
        ([4001, 4002, 4003, 4004], [102, 4001, 4002, 4003], [300, 4001, 4002, 4003]),
    ]
    return auts, packed, slots, top


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("path", ["cand64", "cand128", "slabs1", "slabs3"])
def test_soft_token_step_exact(dtype, path):
    """mocr_op_dec_token_soft, three consecutive steps, alternatives form (with the forced prefixes) and ids form, candidate
    and slab path: the rows of _token_case, 12 slots over 13 rows through a permuted rowmap.  The reference adds the state's
    weights to the step's logits (on the candidate path the inputs are the tile statistics of logit + weight, as the SOFT LM
    head leaves them; on the slab path the kernel adds the weights itself), picks over the effective set, walks the state -
    an edge, else the default edge (with MOCR_DEFAULT_FALLBACK: the default state's edge on the token, if it has one), else DEAD -
    and rebuilds the mask, an open state from all ones.  ids, steps, finished,
    lengths, states and the 192 mask words of every row exact; then, on the rows that bring no soft automaton, the same launch
    through mocr_op_dec_token_automaton gives the same outputs bit for bit."""
    eng = su.score_engine("wide", dtype)
    auts, (eb, et, en, acc, ew, dn, first), slots, top = _token_case()
    n, R, ids_ld, max_len = len(slots), 13, 16, 16
    rowmap = np.array([s[0] for s in slots], np.int32)
    base3 = np.ones((3, V), bool)
    base3[1, [21, 99, 62, 3000]] = False
    base3[2] = cu.mask_of([200])
    aut_of_row, ngr, bsor = [None] * (R + 1), np.zeros(R + 1, np.int32), np.zeros(R + 1, np.int32)
    ids = np.full((R + 1, ids_ld), FILL, np.int32)
    step, finished, lens = np.zeros(n, np.int32), np.zeros(R + 1, np.int32), np.full(R + 1, max_len, np.int32)
    ld = 4
    prefix, plen = np.zeros((R + 1, ld), np.int32), np.zeros(R + 1, np.int32)
    rel = np.full(R + 1, SENT, np.int64)
    for s, (row, k, g, bs, hist, fin, pre) in enumerate(slots):
        aut_of_row[row], ngr[row], bsor[row] = k, g, bs
        ids[row, :len(hist)] = hist
        step[s] = len(hist) - 1
        rel[row] = NONE if k is None else auts[k].walk(hist[1:hist.index(EOS)] if EOS in hist else hist[1:])
        if fin:
            finished[row] = 1; lens[row] = hist.index(EOS) + 1
        if pre:
            prefix[row, len(hist) - 1:len(hist) - 1 + len(pre)] = pre; plen[row] = len(hist) - 1 + len(pre)
    aut_of_row[4], ngr[4] = 0, 2                            # a row no slot decodes: whatever it holds stays
    abase = np.array([-1 if k is None else first[k] for k in aut_of_row], np.int32)
    rs = np.random.RandomState({"slabs1": 41, "slabs3": 43, "cand64": 464, "cand128": 528}[path])
    junk = rs.randint(0, 2 ** 32, size=(R + 1, MW), dtype=np.uint64).astype(np.uint32)

    def glob(rel_):
        return np.array([r + first[aut_of_row[i]] if r >= 0 else r for i, r in enumerate(rel_)], np.int32)

    def logits(k):
        lg = (np.round(rs.standard_normal((n, V)) * 3 * 256) / 256)
        for s in range(n):
            lg[s, top[s][k]] = [30.0, 29.0, 28.0, 27.0]
        return lg.astype(np.float32).astype(np.float64)

    def weighted(lg, state):
        """the step's logits as the rule sees them: + the weights of the state every slot's row is in"""
        rel_, fin_ = state[5], state[2]
        out = lg.copy()
        for s in range(n):
            k = aut_of_row[rowmap[s]]
            if k is not None and rel_[rowmap[s]] >= 0:
                out[s] += bu.bias_of(auts[k], int(rel_[rowmap[s]])).astype(np.float64)
        assert (out.astype(np.float32).astype(np.float64) == out).all()
        return out

    def forced_of(state, with_prefix):
        _, step_, fin_, _, _, _ = state
        return {s: int(prefix[rowmap[s], step_[s]]) for s in range(n)
                if with_prefix and step_[s] < plen[rowmap[s]] and not fin_[rowmap[s]]}

    def inputs(lg, wl, mk, forced):
        tgt = np.full(n + GUARD, np.nan, np.float32)
        if path.startswith("slabs"):                                     # the kernel adds the weights itself: plain logits in
            nslab = int(path[5:])
            r2 = np.random.RandomState(5)
            bias = (r2.randint(-100, 100, V) / 64.0).astype(np.float64)
            parts = (r2.randint(-300, 300, (nslab, n, V)) / 64.0).astype(np.float64)
            parts[-1] = lg - bias - parts[:-1].sum(0)
            assert (parts.astype(np.float32).astype(np.float64) == parts).all()
            return dict(slabs=_f32(parts), nslab=nslab, vbias=_f32(bias)), None, None, None, _f32(tgt)
        tile = int(path[4:])
        nt = V // tile
        m, idx, s_ = cu.masked_tile_stats(wl, mk, tile)                  # what the SOFT LM head leaves
        t3 = cu.masked(wl, mk).reshape(n, nt, tile)
        ti = lex_top(t3)
        tv = np.take_along_axis(t3, ti, -1)
        ti = np.where(np.isneginf(tv), NO_IDX, ti + (np.arange(nt) * tile)[None, :, None])
        for s, tok in forced.items():
            tgt[s] = wl[s, tok] if mk[s, tok] else -np.inf
        return dict(cand_val=_f32(m), cand_idx=_i32(idx), ncand=nt), _f32(s_), _f32(tv), _i32(ti), _f32(tgt)

    def run(variant, lg, state, soft=True, hard_rows=None):
        ids_, step_, fin_, len_, rm_, rel_ = state
        kw, cand_sum, top_val, top_idx, tgt = inputs(lg, weighted(lg, state) if soft else lg, _unpack(rm_[rowmap]), forced_of(state, variant == 2))
        d = dict(ids=_i32(ids_), step=_i32(step_), finished=_i32(fin_), len=_i32(len_), n_unfinished=_i32([8, SENT]),
                 rowmap=_i32(rowmap), x_f32=torch.full((n + GUARD, D), float("nan"), device="cuda"),
                 x_t=torch.full((n + GUARD, D), float("nan"), device="cuda", dtype=torch.bfloat16 if dtype == "bf16" else torch.float32))
        sc = torch.full((R + 1, ids_ld), float("nan"), device="cuda") if variant == 2 else None
        ai = torch.full((R + 1, ids_ld, K4), SENT, dtype=torch.int32, device="cuda") if variant == 2 else None
        al = torch.full((R + 1, ids_ld, K4), float("nan"), device="cuda") if variant == 2 else None
        ab = abase if hard_rows is None else np.where(hard_rows, abase, -1).astype(np.int32)
        d_rm, d_state = _u32(rm_), _i32(glob(rel_))
        pre = (_i32(prefix), _i32(plen), ld, tgt) if variant == 2 else (None, None, 0, None)
        args = (cand_sum if variant == 2 else None, sc, top_val if variant == 2 else None, top_idx if variant == 2 else None, ai, al, d_rm,
                _i32(np.arange(R + 1)), d_rm, _u32(cu.pack_sets(base3)), _i32(bsor), _i32(ngr), *pre, _i32(eb), _i32(et), _i32(en), _u8(acc),
                _i32(ab), d_state)
        torch.cuda.synchronize()
        if soft:
            eng.op_dec_token_soft(*args, _f32(ew), _i32(dn), first=0, n=n, ids_ld=ids_ld, max_len=max_len, n_real=n, **d, **kw)
        else:
            eng.op_dec_token_automaton(*args, first=0, n=n, ids_ld=ids_ld, max_len=max_len, n_real=n, **d, **kw)
        o = {k: v.cpu().numpy() for k, v in d.items() if k in ("ids", "step", "finished", "len", "x_f32")}
        g = d_state.cpu().numpy()
        back = np.array([int(x) - first[aut_of_row[i]] if x >= 0 and aut_of_row[i] is not None else int(x) for i, x in enumerate(g)], np.int64)
        return ((o["ids"], o["step"], o["finished"], o["len"], d_rm.cpu().numpy().view(np.uint32), back),
                None if ai is None else ai.cpu().numpy(), None if sc is None else sc.cpu().numpy(),
                None if al is None else al.cpu().numpy(), o["x_f32"])

    def reference(state, lg, with_prefix):
        ids_, step_, fin_, len_, rm_, rel_ = (a.copy() for a in state)
        wl = weighted(lg, state)
        forced = forced_of(state, with_prefix)
        want4 = np.full((n, K4), -1)
        for s in range(n):
            row, t = rowmap[s], step_[s]
            eff = _unpack(rm_[row])
            was = bool(fin_[row])
            tok = 0 if was else int(np.argmax(np.where(eff, wl[s], -np.inf)))
            if not was:
                want4[s] = cu.masked_top(wl[s], eff)[0]
            tok = forced.get(s, tok)
            ids_[row, t + 1] = tok
            step_[s] = t + 1
            if not was and (tok == EOS or t + 2 >= max_len):
                fin_[row] = 1; len_[row] = t + 2
            a = None if aut_of_row[row] is None else auts[aut_of_row[row]]
            if was:
                continue
            if a is not None and tok != EOS:
                rel_[row] = a.next(int(rel_[row]), tok)
            if not fin_[row] and (a is not None or ngr[row] > 0):
                rm_[row] = cu.pack_sets(au.step_mask(a, int(rel_[row]), ids_[row, :t + 2], int(ngr[row]), base3[bsor[row]])[None])[0]
        return (ids_, step_, fin_, len_, rm_, rel_), want4

    LG = [logits(0), logits(1), logits(2)]
    rm0 = junk.copy()
    for s, (row, k, g, bs, hist, fin, pre) in enumerate(slots):
        if not fin:
            rm0[row] = cu.pack_sets(au.step_mask(None if k is None else auts[k], int(rel[row]), hist, g, base3[bs])[None])[0]
    names = ("ids", "step", "finished", "len", "row_mask", "state")
    state2 = state0 = (ids, step, finished, lens, rm0, rel)
    hard_rows = np.array([k in (None, 1) for k in aut_of_row])        # the rows that bring no soft automaton
    hard_slots = hard_rows[rowmap]
    for k in range(3):
        want2, want4 = reference(state2, LG[k], True)
        want0, _ = reference(state0, LG[k], False)
        got2, ai, sc, al, x2 = run(2, LG[k], state2)
        got0, _, _, _, x0 = run(0, LG[k], state0)
        for name, g2, w2, g0, w0 in zip(names, got2, want2, got0, want0):
            np.testing.assert_array_equal(g2, w2, err_msg=f"step {k + 1}, alternatives form: {name}")
            np.testing.assert_array_equal(g0, w0, err_msg=f"step {k + 1}, ids form: {name}")
        a4 = ai[rowmap, state2[1] + 1]
        live = state2[2][rowmap] == 0
        np.testing.assert_array_equal(a4[live], want4[live], err_msg="alt_ids is not the top four of the effective set on logit + weight")
        assert (a4[~live] == -1).all()
        # the rows without a soft automaton, in a launch of the hook below that knows only them: the same outputs bit for bit
        # (on the candidate path its inputs are those rows' own unweighted statistics, which is what theirs were)
        h2, hai, hsc, hal, hx2 = run(2, LG[k], state2, soft=False, hard_rows=hard_rows)
        h0, _, _, _, hx0 = run(0, LG[k], state0, soft=False, hard_rows=hard_rows)
        rows_h = np.nonzero(hard_rows[:R])[0]
        for name, g2, hh2, g0, hh0 in zip(names, got2, h2, got0, h0):
            if name == "step":
                np.testing.assert_array_equal(g2[hard_slots], hh2[hard_slots]); np.testing.assert_array_equal(g0[hard_slots], hh0[hard_slots])
            else:
                np.testing.assert_array_equal(g2[rows_h], hh2[rows_h], err_msg=f"hard rows, alternatives form: {name}")
                np.testing.assert_array_equal(g0[rows_h], hh0[rows_h], err_msg=f"hard rows, ids form: {name}")
        for g, h in ((ai, hai), (sc, hsc), (al, hal)):
            np.testing.assert_array_equal(g[rows_h].view(np.uint32), h[rows_h].view(np.uint32), err_msg="hard rows: scores / alternatives")
        np.testing.assert_array_equal(x2[:n][hard_slots].view(np.uint32), hx2[:n][hard_slots].view(np.uint32))
        np.testing.assert_array_equal(x0[:n][hard_slots].view(np.uint32), hx0[:n][hard_slots].view(np.uint32))
        if k == 1:
            assert np.isneginf(sc[7, state2[1][2] + 1]), "the loop's forced token without an edge is outside the effective set: -inf"
        state2, state0 = got2, got0
    ids3, _, fin3, len3, rm3, rel3 = state2
    assert ids3[5, 1:4].tolist() == [100, 102, EOS] and rel3[5] == 2 and len3[5] == 4, "slot 0: the weights decide, the closed accepting state ends the row"
    assert ids3[2, 2:5].tolist() == [5000, 5001, 5002] and rel3[2] == 0, "slot 1: -60 on the unweighted winner; default edges; n = 1 bans"
    assert ids3[7, 1:4].tolist() == [100, 4000, EOS] and rel3[7] == DEAD and fin3[7] == 1, "slot 2: the closed loop dies beside the open rows"
    assert state0[5][7] >= 0, "... and lives in the ids form"
    assert ids3[0, 4:7].tolist() == [63, 60, 64] and rel3[0] == 0, "slot 3: open state, base set 1 lacks 62 and 99, n = 2 bans 61 and 63 behind 60"
    assert ids3[9, 6:9].tolist() == [73, 70, 71], "slot 4: n = 3 bans 72 behind 70 71"
    assert ids3[1, 2] == 4000 and rel3[1] == 2 and ids3[1, 3:5].tolist() == [100, 102], "slot 5: forced along the default edge to state 0, then 100, then 102"
    assert ids3[3, 2:4].tolist() == [EOS, 0] and len3[3] == 3, "slot 8: the dead-end rule on an open state"
    assert ids3[10, 1:4].tolist() == [1100, 1100, 1100] and rel3[10] == 0, "slot 9: +8 on 1100 among 300 edges"
    for untouched in (4, 8, R):
        np.testing.assert_array_equal(rm3[untouched], junk[untouched], err_msg=f"row {untouched}: mask rewritten")
    assert rel3[8] == 1 and rel3[4] == SENT and rel3[R] == SENT and (rm3[6] == rm0[6]).all()
    assert ids3[11, 2:5].tolist() == [300, 100, 300] and rel3[11] == 2, "slot 10: the fallback walk finds state 0's edges (without it: 0, 1, 0)"
    assert ids3[12, 2:5].tolist() == [4001, 102, 300] and rel3[12] == 2, "slot 11: no edge in the default state either: the default state itself"
    report(f"dec_token SOFT {dtype} {path}: three consecutive steps, ids, states and the 192 mask words of 13 rows exact against numpy on logit + weight "
           f"(weights decide, default walk, closed DEAD beside it, open rebuild with a base set and n = 1, 2, 3, dead end, forced default edge, fallback hit and miss, "
           f"finished, none, 300 edges); rows without a soft automaton == mocr_op_dec_token_automaton bit for bit")
