"""-m gpu: greedy decoding with no_repeat_ngram_size - the per-row effective masks the token kernel rebuilds on the device.

Bottom up: the NGRAM token kernel (mocr_op_dec_token_ngram) and the start-of-batch kernel (mocr_op_ngram_init) against numpy,
exactly (ids and mask words); whole recognitions against the reference loop on the fp32 oracle (ngram_util.ngram_generate: the
masked greedy loop with the mask recomputed at every step from a dictionary of n-grams); the bf16 decode paths under the
first-divergence rule; scores and alternatives under bans; token sets and bans together; compaction; the Python surface.

Tolerances are those of tests/test_gpu_constraints.py (named where used); the bf16 gap bound is imported."""
import threading

import numpy as np
import pytest

from gpu_util import crops, report

import constraint_util as cu
import ngram_util as nu
import score_util as su
from test_gpu_bf16_parity import BF16_GAP_TOL
from test_gpu_constraints import FP32_LOGIT_TOL, _bits, _f32, _i32, _u32, lex_top

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

D, V, K4, EOS, START = 768, 6144, 4, 3, 2
MW = V // 32
NO_IDX = cu.NO_IDX
GUARD = 2
FILL = 4000                  # what the unwritten tail of an ids row holds in the kernel test: a valid token, so that a window
                             # read past the row's L tokens shows up as a ban of it


def _unpack(words):
    """uint32 [..., V / 32] -> bool [..., V]"""
    w = np.asarray(words).view(np.uint32)
    return ((w[..., :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(w.shape[:-1] + (V,))


# ------------------------------------------------------------------------------------------------ 1. the kernels, exact
# slot -> (row, n, base set, the row's tokens so far, finished)
KERNEL_SLOTS = [
    (5, 3, 0, [START, 10, 11, 12, 13, 10, 11], False),      # key (10, 11) -> 12 banned; then key (11, 13): nothing; then (13, 10) -> 11
    (2, 2, 1, [START, 20, 20], False),                      # "a a": the match is the LAST window (i = L - n); base set 1 lacks 21
    (7, 1, 0, [START, 30, 31, 35], False),                     # n = 1: every token of the row, the start token too
    (0, 5, 0, [START, 40, 41], False),                      # L + 1 < n, then L + 1 = n: nothing banned
    (3, 3, 1, [START, 50, 51, 50, 51, EOS, 0], True),       # finished: emits pad, its mask is left alone
]
# the tokens with the four largest logits of every slot, largest first, for the two consecutive steps
KERNEL_TOP = [
    ([12, 13, 14, 15], [10, 16, 17, 18]),                   # step 1: 12 is banned -> 13; step 2: free -> 10, then 11 is banned
    ([20, 21, 22, 23], [20, 24, 25, 26]),                   # step 1: 20 banned, 21 outside the base set -> 22; step 2: free -> 20
    ([30, START, 31, 32], [32, 30, 33, 34]),                # step 1: 30, start, 31 banned -> 32; step 2: 32, 30 banned -> 33
    ([40, 41, 42, 43], [41, 40, 42, 43]),                   # nothing banned: 40, then 41
    ([50, 51, 52, 53], [51, 50, 52, 53]),
]
KERNEL_WANT = [(13, 10), (22, 20), (32, 33), (40, 41), (0, 0)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("path", ["cand64", "cand128", "slabs1", "slabs3"])
def test_ngram_token_step_exact(dtype, path):
    """mocr_op_dec_token_ngram, two consecutive steps (the second on the first one's outputs), alternatives form and ids form,
    candidate and slab path.  5 slots over 8 rows through a permuted rowmap, ids_ld 16, a different step per slot, n per row
    from {0, 1, 2, 3, 5}, two base sets, one finished row; in the first step the largest logit of every slot that has a ban is a banned token.
    Expected, exactly: the emitted id = the argmax over the row's effective set; after every step row_mask[row] = the row's
    base set minus the bans of the NEXT step for every live row with n > 0 (numpy, ngram_util.step_mask), every other row's
    words untouched; alt_ids entry 0 = the id and no banned token among the four.  Then the same first step with n = 0 on
    slot 0's row: that row's mask is left alone."""
    eng = su.score_engine("wide", dtype)
    n, R, ids_ld, max_len = 5, 8, 16, 16
    rowmap = np.array([s[0] for s in KERNEL_SLOTS], np.int32)
    ngram_of_row = np.zeros(R, np.int32)
    base_set_of_row = np.zeros(R, np.int32)
    base2 = np.ones((2, V), bool)
    base2[1, [21, 99, 3000]] = False
    ids = np.full((R + 1, ids_ld), FILL, np.int32)
    step = np.zeros(n, np.int32)
    finished = np.zeros(R, np.int32)
    lens = np.full(R, max_len, np.int32)
    for s, (row, g, bs, hist, fin) in enumerate(KERNEL_SLOTS):
        ngram_of_row[row], base_set_of_row[row] = g, bs
        ids[row, :len(hist)] = hist
        step[s] = len(hist) - 1
        if fin:
            finished[row] = 1; lens[row] = hist.index(EOS) + 1
    ngram_of_row[[1, 4, 6]] = [2, 3, 1]                     # rows no slot decodes: whatever they hold stays
    assert sorted(set(ngram_of_row[rowmap].tolist())) == [1, 2, 3, 5] and len(set(step.tolist())) >= 3
    rs = np.random.RandomState({"slabs1": 21, "slabs3": 23, "cand64": 264, "cand128": 328}[path])
    junk = rs.randint(0, 2 ** 32, size=(R + 1, MW), dtype=np.uint64).astype(np.uint32)      # rows 1, 4, 6, the finished row, the guard row

    def logits(k):
        lg = (np.round(rs.standard_normal((n, V)) * 3 * 256) / 256)
        for s in range(n):
            lg[s, KERNEL_TOP[s][k]] = [30.0, 29.0, 28.0, 27.0]
        return lg.astype(np.float32).astype(np.float64)

    def inputs(lg, mk):
        if path.startswith("slabs"):
            nslab = int(path[5:])
            r2 = np.random.RandomState(5)
            bias = (r2.randint(-100, 100, V) / 64.0).astype(np.float64)
            parts = (r2.randint(-300, 300, (nslab, n, V)) / 64.0).astype(np.float64)
            parts[-1] = lg - bias - parts[:-1].sum(0)
            assert (parts.astype(np.float32).astype(np.float64) == parts).all()
            return dict(slabs=_f32(parts), nslab=nslab, vbias=_f32(bias)), None, None, None
        tile = int(path[4:])
        nt = V // tile
        m, idx, s_ = cu.masked_tile_stats(lg, mk, tile)                  # what the masked LM head leaves for these sets
        t3 = cu.masked(lg, mk).reshape(n, nt, tile)
        ti = lex_top(t3)
        tv = np.take_along_axis(t3, ti, -1)
        ti = np.where(np.isneginf(tv), NO_IDX, ti + (np.arange(nt) * tile)[None, :, None])
        return dict(cand_val=_f32(m), cand_idx=_i32(idx), ncand=nt), _f32(s_), _f32(tv), _i32(ti)

    def run(variant, lg, state, ngr):
        """one step on `state` (ids, step, finished, len, row_mask words): -> the state after it, alt_ids"""
        ids_, step_, fin_, len_, rm_ = state
        kw, cand_sum, top_val, top_idx = inputs(lg, _unpack(rm_[rowmap]))
        d = dict(ids=_i32(ids_), step=_i32(step_), finished=_i32(fin_), len=_i32(len_), n_unfinished=_i32([4, -777]),
                 rowmap=_i32(rowmap), x_f32=torch.full((n + GUARD, D), float("nan"), device="cuda"),
                 x_t=torch.full((n + GUARD, D), float("nan"), device="cuda", dtype=torch.bfloat16 if dtype == "bf16" else torch.float32))
        sc = torch.full((R + 1, ids_ld), float("nan"), device="cuda") if variant == 2 else None
        ai = torch.full((R + 1, ids_ld, K4), -777, dtype=torch.int32, device="cuda") if variant == 2 else None
        al = torch.full((R + 1, ids_ld, K4), float("nan"), device="cuda") if variant == 2 else None
        d_rm = _u32(rm_)
        torch.cuda.synchronize()
        eng.op_dec_token_ngram(cand_sum if variant == 2 else None, sc, top_val if variant == 2 else None,
                               top_idx if variant == 2 else None, ai, al, d_rm, _i32(np.arange(R + 1)), d_rm,
                               _u32(cu.pack_sets(base2)), _i32(base_set_of_row), _i32(ngr),
                               first=0, n=n, ids_ld=ids_ld, max_len=max_len, n_real=n, **d, **kw)
        o = {k: v.cpu().numpy() for k, v in d.items() if k in ("ids", "step", "finished", "len", "n_unfinished")}
        return (o["ids"], o["step"], o["finished"], o["len"], d_rm.cpu().numpy().view(np.uint32)), None if ai is None else ai.cpu().numpy()

    def reference(state, k, ngr):
        """numpy: the state after step k on `state`"""
        ids_, step_, fin_, len_, rm_ = (a.copy() for a in state)
        want4 = np.full((n, K4), -1)
        lg = LG[k]
        for s in range(n):
            row, t = rowmap[s], step_[s]
            eff = _unpack(rm_[row])
            tok = 0 if fin_[row] else int(np.argmax(np.where(eff, lg[s], -np.inf)))
            if not fin_[row]:
                want4[s] = cu.masked_top(lg[s], eff)[0]
            ids_[row, t + 1] = tok
            step_[s] = t + 1
            if not fin_[row] and ngr[row] > 0:
                rm_[row] = cu.pack_sets(nu.step_mask(ids_[row, :t + 2], int(ngr[row]), base2[base_set_of_row[row]])[None])[0]
        return (ids_, step_, fin_, len_, rm_), want4

    LG = [logits(0), logits(1)]
    # the masks the batch would hold before these steps: the effective set of every live row's current step
    rm0 = junk.copy()
    for s, (row, g, bs, hist, fin) in enumerate(KERNEL_SLOTS):
        if not fin:
            rm0[row] = cu.pack_sets(nu.step_mask(hist, g, base2[bs])[None])[0]
    state = (ids, step, finished, lens, rm0)
    for k in (0, 1):
        want, want4 = reference(state, k, ngram_of_row)
        got2, ai = run(2, LG[k], state, ngram_of_row)
        got0, _ = run(0, LG[k], state, ngram_of_row)
        emitted = got2[0][rowmap, state[1] + 1]
        assert emitted.tolist() == [w[k] for w in KERNEL_WANT], f"step {k + 1}: emitted {emitted.tolist()}"
        for name, g2, g0, w_ in zip(("ids", "step", "finished", "len", "row_mask"), got2, got0, want):
            np.testing.assert_array_equal(g2, w_, err_msg=f"step {k + 1}, alternatives form: {name}")
            np.testing.assert_array_equal(g0, w_, err_msg=f"step {k + 1}, ids form: {name}")
        a4 = ai[rowmap, state[1] + 1]
        np.testing.assert_array_equal(a4[:4], want4[:4], err_msg="alt_ids is not the top four of the effective set")
        assert (a4[:4, 0] == emitted[:4]).all() and (a4[4] == -1).all()
        for s in range(4):
            assert _unpack(state[4][rowmap[s]])[a4[s]].all(), f"slot {s}: a banned token among the four"
        state = got2
    # what the two steps proved about the rebuilt masks (so that the table above cannot rot)
    after1 = _unpack(reference((ids, step, finished, lens, rm0), 0, ngram_of_row)[0][4])
    after2 = _unpack(state[4])
    assert after1[5].all() and not after2[5, 11] and after2[5, 12] and after2[5].sum() == V - 1, "row 5: the ban of 12 is gone, 11 is banned"
    assert after1[2].sum() == V - 3 and not after2[2, 20] and not after2[2, 22] and after2[2].sum() == V - 5, "row 2: base set 1, then 20 and 22"
    assert after2[7].sum() == V - 6 and not after2[7, START], "row 7 (n = 1): start, 30, 31, 35, 32, 33"
    assert after1[0].all() and after2[0].all(), "row 0 (n = 5): L + 1 <= n"
    np.testing.assert_array_equal(state[4][[1, 3, 4, 6, 8]], junk[[1, 3, 4, 6, 8]], err_msg="a row no live slot decodes was rewritten")
    # n = 0 on slot 0's row: its mask is left alone (and still applies to the step)
    ng0 = ngram_of_row.copy(); ng0[5] = 0
    got, _ = run(2, LG[0], (ids, step, finished, lens, rm0), ng0)
    np.testing.assert_array_equal(got[4][5], rm0[5]); assert got[0][5, step[0] + 1] == 13
    report(f"dec_token NGRAM {dtype} {path}: two consecutive steps, ids and the 192 mask words of 8 rows exact against numpy "
           f"(n = 1, 2, 3, 5 and 0, two base sets, permuted rowmap, a finished row, the largest logit of every slot with a ban banned)")


def test_ngram_init_kernel_exact():
    eng = su.score_engine("wide", "fp32")
    R = 8
    base2 = np.ones((2, V), bool)
    base2[1] = np.random.RandomState(3).rand(V) < 0.5
    base2[1, [START, EOS]] = True
    sor = np.array([0, 1, 1, 0, 1, 0, 0, 1], np.int32)
    ngr = np.array([1, 1, 3, 0, 2, 5, 1, 0], np.int32)
    junk = np.random.RandomState(4).randint(0, 2 ** 32, size=(R + 1, MW), dtype=np.uint64).astype(np.uint32)
    d_rm = _u32(junk)
    torch.cuda.synchronize()
    eng.op_ngram_init(d_rm, _u32(cu.pack_sets(base2)), _i32(sor), _i32(ngr), R)
    got = d_rm.cpu().numpy().view(np.uint32)
    want = base2[sor].copy()
    want[ngr == 1, START] = False
    np.testing.assert_array_equal(got[:R], cu.pack_sets(want))
    np.testing.assert_array_equal(got[R], junk[R], err_msg="the row behind the batch was written")
    assert (_unpack(got[:R]).sum(-1) == base2[sor].sum(-1) - (ngr == 1)).all()


# ------------------------------------------------------------------------------------------------ 2 .. 4. end to end
N_E2E, LEN_E2E = 8, 32
MIXED = np.array([0, 1, 2, 3] * 2, np.int32)


def _reference(case):
    """case: 3, 2 or "mixed" -> (ngrams [8], ids, logits, per-step masks) of the reference loop on the fp32 oracle, widened-margin
    weights, crops(31, 8), max_len 32; computed once"""
    if case not in _reference.cache:
        o = su.score_oracle("wide")
        with torch.no_grad():
            enc = o.encode(o.preprocess_gray(crops(31, N_E2E)))
        ngr = MIXED if case == "mixed" else np.full(N_E2E, case, np.int32)
        _reference.cache[case] = (ngr,) + nu.ngram_generate(o, enc, np.ones((N_E2E, V), bool), ngr, LEN_E2E)
    return _reference.cache[case]


_reference.cache = {}


def _no_repeats(ids, lens, ngr):
    for b in range(ids.shape[0]):
        if ngr[b] > 0:
            assert nu.first_repeat(ids[b, :lens[b]], int(ngr[b])) is None, f"row {b} repeats a {ngr[b]}-gram: {ids[b, :lens[b]].tolist()}"


@pytest.mark.parametrize("case", [3, 2, "mixed"])
def test_fp32_ngram_against_the_reference_loop(case):
    """fp32 engine, 8 crops, max_len 32, n = 3 / n = 2 on every row / (0, 1, 2, 3) repeating.  First, on the oracle alone: the
    free greedy run of every row holds a repeated n-gram before position 32, so the bans fire (and the ids differ from the free
    run's: this test fails without the feature).  Then: ids and lengths identical to the reference loop; scores and alternatives
    within 2 x 1e-3 of the float64 masked log-softmax of the oracle's logits under the per-step masks (the fp32 bound of
    tests/test_gpu_constraints.py for its masked scores); alt_ids entry 0 = the id, no banned token among the four; no emitted
    row repeats an n-gram; the ids-only and scored calls give the same ids; n = 0 rows bit-identical to an unconstrained run."""
    free_ids, _ = su.oracle_run("wide", 31, N_E2E, LEN_E2E)
    ngr, ids_o, logits, masks = _reference(case)
    for b in range(N_E2E):
        for g in (2, 3):
            f = nu.first_repeat(free_ids[b], g)
            assert f is not None and f < LEN_E2E, f"row {b}: the free run repeats no {g}-gram"
        if ngr[b] > 0:
            assert (free_ids[b] != ids_o[b, :free_ids.shape[1]]).any(), f"row {b}: the bans changed nothing"
    lens_o = nu.lengths(ids_o)
    _no_repeats(ids_o, lens_o, ngr)
    L = ids_o.shape[1]
    eng = su.score_engine("wide", "fp32")
    gray = crops(31, N_E2E)
    ids, lens, logp, alt_ids, alt_logp = eng.recognize_gray(gray, LEN_E2E, alternatives=True, no_repeat_ngram=ngr)
    live = np.arange(L)[None, :] < lens_o[:, None]
    gaps = nu.step_gaps(logits, masks)
    print(f"fp32 n-gram ({case}): smallest unbanned top-2 margin of the reference {gaps[live[:, 1:]].min():.2e}", flush=True)
    np.testing.assert_array_equal(np.where(live, ids[:, :L], 0), np.where(live, ids_o, 0), err_msg="fp32 ids differ from the reference loop's")
    np.testing.assert_array_equal(lens, lens_o)
    assert (ids[:, L:] == 0).all()
    _no_repeats(ids, lens, ngr)
    tol = 2 * FP32_LOGIT_TOL
    worst = 0.0
    for b in range(N_E2E):
        for t in range(1, lens[b]):
            ref = cu.masked_log_softmax64(logits[b, t - 1], masks[b, t - 1])
            a = alt_ids[b, t]
            assert a[0] == ids[b, t] and (a >= 0).all() and masks[b, t - 1][a].all(), f"row {b} token {t}: alternatives {a.tolist()}"
            want4, lp4 = cu.masked_top(logits[b, t - 1], masks[b, t - 1])
            worst = max(worst, abs(float(logp[b, t]) - ref[ids[b, t]]), float(np.abs(alt_logp[b, t] - ref[a]).max()),
                        float(np.abs(alt_logp[b, t].astype(np.float64) - lp4).max()))
            np.testing.assert_array_equal(_bits(alt_logp[b, t, :1]), _bits(logp[b, t:t + 1]))
    print(f"fp32 n-gram ({case}): max |logp - float64 masked log-softmax| {worst:.3e} (bound {tol:.0e})", flush=True)
    assert worst <= tol, worst
    i0, l0 = eng.recognize_gray(gray, LEN_E2E, no_repeat_ngram=ngr)
    i1, l1, p1 = eng.recognize_gray(gray, LEN_E2E, scores=True, no_repeat_ngram=ngr)
    np.testing.assert_array_equal(i0, ids); np.testing.assert_array_equal(i1, ids); np.testing.assert_array_equal(l0, lens)
    np.testing.assert_array_equal(_bits(p1), _bits(logp))
    z = np.nonzero(ngr == 0)[0]
    if z.size:
        fi, fl, fp, fa, fal = eng.recognize_gray(gray, LEN_E2E, alternatives=True)
        np.testing.assert_array_equal(fi[z], ids[z], err_msg="an n = 0 row differs from the unconstrained run")
        np.testing.assert_array_equal(fl[z], lens[z]); np.testing.assert_array_equal(_bits(fp[z]), _bits(logp[z]))
        np.testing.assert_array_equal(fa[z], alt_ids[z]); np.testing.assert_array_equal(_bits(fal[z]), _bits(alt_logp[z]))
    report(f"no-repeat n-grams fp32 vs the reference loop, n = {case}, 8 crops, max_len 32: ids identical (smallest unbanned margin "
           f"{gaps[live[:, 1:]].min():.1e}), logp / alt_logp within {worst:.2e} (bound {tol:.0e})")


# (name, rows, engine flags).  NO_FUSED_ARGMAX = 16.  bf16, engine.hip decode_step: up to 32 rows the small-batch step (its LM
# head leaves one slab: the slab form of the token kernel); 96 rows (max_batch 96) the generic step with the fused masked
# epilogue on 64-column tiles (candidate path), or through the slab GEMM with NO_FUSED_ARGMAX; from 1024 rows (dec_tile) the
# 128-column tiles - the smallest row count that takes them.
BF16_CASES = [("small", 8, 0), ("fused64", 96, 0), ("nofused", 96, 16), ("fused128", 1024, 0)]


@pytest.mark.parametrize("name,rows,flags", BF16_CASES)
def test_bf16_ngram_paths(name, rows, flags):
    """bf16, n = 3 on every row; the first 8 rows are the crops of the fp32 test, the others repeat them.  Every row of the
    batch: no repeated 3-gram, alt_ids entry 0 = the id, the three kinds of call give the same ids.  The first 8 rows against
    the reference loop on the fp32 oracle under the first-divergence rule of tests/test_gpu_bf16_parity.py: a row may leave the
    reference only at a step whose reference margin among the UNBANNED tokens is below that file's BF16_GAP_TOL; at least half
    of the rows match the reference to their end."""
    ngr8, ids_o, logits, masks = _reference(3)
    eng = su.score_engine("wide", "bf16", max_batch=max(64, rows), flags=flags)
    gray = np.concatenate([crops(31, N_E2E)] * (rows // N_E2E))
    ngr = np.full(rows, 3, np.int32)
    ids, lens, logp, alt_ids, alt_logp = eng.recognize_gray(gray, LEN_E2E, alternatives=True, no_repeat_ngram=ngr)
    _no_repeats(ids, lens, ngr)
    for b in range(rows):
        np.testing.assert_array_equal(alt_ids[b, 1:lens[b], 0], ids[b, 1:lens[b]])
    assert np.isfinite(logp).all() and (logp <= 0).all()
    i0, l0 = eng.recognize_gray(gray, LEN_E2E, no_repeat_ngram=3)
    i1, l1, p1 = eng.recognize_gray(gray, LEN_E2E, scores=True, no_repeat_ngram=ngr)
    np.testing.assert_array_equal(i0, ids); np.testing.assert_array_equal(i1, ids); np.testing.assert_array_equal(l1, lens)
    np.testing.assert_array_equal(_bits(p1), _bits(logp))
    fi, _ = eng.recognize_gray(gray, LEN_E2E)
    assert all(nu.first_repeat(fi[b], 3) is not None for b in range(N_E2E)), "the free bf16 run was meant to loop"
    L = ids_o.shape[1]
    div = cu.first_divergences(ids[:N_E2E, :L], ids_o, nu.step_gaps(logits, masks))
    for b, t, g in div:
        report(f"[bf16 n-gram {name}] row {b}: first divergence at token {t} (reference margin among the unbanned tokens {g:.3e})")
    assert all(g < BF16_GAP_TOL for _, _, g in div), div
    assert len(div) <= N_E2E // 2, f"{len(div)} of {N_E2E} rows leave the reference"
    report(f"no-repeat n-grams bf16 {name} ({rows} rows, flags {flags}): no row repeats a 3-gram, ids / logp equal across the three kinds "
           f"of call, {len(div)} first divergences of 8, all below the unbanned margin {BF16_GAP_TOL}")


# ------------------------------------------------------------------------------------------------ 5. sets and bans together
def test_token_set_and_ngram_together():
    """A digits-like set of 4 tokens (plus EOS, which the engine adds) and n = 2, fp32, 8 crops, max_len 32.  Every generated
    token but the first completes a bigram inside the set, none may repeat, and 4 symbols have 16 bigrams: a row holds at most
    17 tokens of the set; then every one of them is banned, EOS - never banned - is the only token left, and the row ends by
    EOS with at most 1 + 17 + 1 = 19 tokens, well before max_len.  Every id inside the set, none banned at its step, no
    repeated bigram; identical to the reference loop."""
    o = su.score_oracle("wide")
    free_ids, _ = su.oracle_run("wide", 31, N_E2E, LEN_E2E)
    digits = np.unique(free_ids[:, 1:])[:4]
    base = np.repeat(cu.mask_of(digits)[None], N_E2E, 0)
    ngr = np.full(N_E2E, 2, np.int32)
    with torch.no_grad():
        enc = o.encode(o.preprocess_gray(crops(31, N_E2E)))
    ids_o, logits, masks = nu.ngram_generate(o, enc, base, ngr, LEN_E2E)
    eng = su.score_engine("wide", "fp32")
    h = eng.token_set(digits)
    ids, lens, logp, alt_ids, alt_logp = eng.recognize_gray(crops(31, N_E2E), LEN_E2E, alternatives=True, token_sets=h, no_repeat_ngram=2)
    L = ids_o.shape[1]
    lens_o = nu.lengths(ids_o)
    live = np.arange(L)[None, :] < lens_o[:, None]
    np.testing.assert_array_equal(np.where(live, ids[:, :L], 0), np.where(live, ids_o, 0))
    np.testing.assert_array_equal(lens, lens_o)
    _no_repeats(ids, lens, ngr)
    for b in range(N_E2E):
        assert ids[b, lens[b] - 1] == EOS and lens[b] <= 19, f"row {b} did not end by EOS: {ids[b, :lens[b]].tolist()}"
        for t in range(1, lens[b]):
            assert base[b, ids[b, t]] and masks[b, t - 1][ids[b, t]], f"row {b} token {t}: outside the set or banned"
            a = alt_ids[b, t]
            assert masks[b, t - 1][a[a >= 0]].all() and a[0] == ids[b, t]
            np.testing.assert_array_equal((a >= 0).sum(), min(K4, int(masks[b, t - 1].sum())))
    report(f"token set of 4 + EOS with n = 2, fp32: ids identical to the reference loop, lengths {lens.tolist()}, every row ends by EOS")


# ------------------------------------------------------------------------------------------------ 6. compaction
def test_ngram_compacted_equals_uncompacted():
    """Early-EOS weights, 96 rows shaped as tests/test_gpu_compaction.py shapes them (the six golden crops first), max_len 120,
    n = (0, 1, 2, 3) repeating: rows finish at different steps, the batch is compacted, and ids and lengths equal those of the
    same crops on an engine that never compacts.  The masks are indexed by row, so a compaction moves none."""
    n, max_len = 96, 120
    gray = np.concatenate([crops(4321, 6), crops(4322, n)])[:n]
    ngr = np.array([0, 1, 2, 3] * (n // 4), np.int32)
    eng = su.score_engine("eos", "bf16", max_batch=96)
    nc = su.score_engine("eos", "bf16", max_batch=96, flags=2048)          # MOCR_FLAG_NO_COMPACTION
    base = eng.compaction_count()
    ids, lens = eng.recognize_gray(gray, max_len, no_repeat_ngram=ngr)
    assert eng.compaction_count() - base > 0 and eng.compaction_count() > 0
    u_ids, u_lens = nc.recognize_gray(gray, max_len, no_repeat_ngram=ngr)
    assert nc.compaction_count() == 0
    np.testing.assert_array_equal(ids, u_ids); np.testing.assert_array_equal(lens, u_lens)
    assert lens.min() < lens.max(), "rows were meant to finish at different steps"
    _no_repeats(ids, lens, ngr)
    f_ids, _ = eng.recognize_gray(gray, max_len)
    z = ngr == 0
    np.testing.assert_array_equal(ids[z], f_ids[z])
    assert (ids[~z] != f_ids[~z]).any()
    report(f"no-repeat n-grams bf16 early-EOS 96 rows, lengths {int(lens.min())}..{int(lens.max())}: compacted == uncompacted, "
           f"n = 0 rows == the free run")


# ------------------------------------------------------------------------------------------------ 7. surface
def test_graphs_memory_and_errors():
    """An engine never asked allocates nothing for the feature (free device memory unchanged by unconstrained calls after the
    warm one); the first n-gram batch allocates and captures graphs of its own, a repeat adds none and the unconstrained
    graphs are not captured again; sizes outside 0 .. max_len are refused."""
    from manga_ocr._capi import MocrError
    from manga_ocr.engine import device_memory
    eng = su.score_engine.__wrapped__("wide", "bf16", max_batch=64)
    try:
        gray = crops(5, 40)
        want, want_l = eng.recognize_gray(gray, 16)
        eng.recognize_gray(gray, 16, scores=True)
        g1 = eng.graph_count()
        torch.cuda.synchronize()
        free0 = device_memory(0)[0]
        eng.recognize_gray(gray, 16); eng.recognize_gray(gray, 16, scores=True)
        eng.recognize_gray(gray, 16, no_repeat_ngram=0); eng.recognize_gray(gray, 16, no_repeat_ngram=np.zeros(40, np.int32))
        assert eng.graph_count() == g1 and device_memory(0)[0] == free0, "an engine nobody asked grew"
        ids, lens = eng.recognize_gray(gray, 16, no_repeat_ngram=3)
        g2 = eng.graph_count()
        free1 = device_memory(0)[0]
        assert g2 > g1, "the first n-gram batch captures graphs of its own"
        assert free0 - free1 <= 16 << 20, "the masks of 64 rows and the set table are well under a megabyte"
        eng.recognize_gray(gray, 16, no_repeat_ngram=3); eng.recognize_gray(gray, 16, no_repeat_ngram=[2] * 40)
        b_ids, b_lens = eng.recognize_gray(gray, 16)
        assert eng.graph_count() == g2 and device_memory(0)[0] == free1, "a repeated call captured a graph or allocated"
        assert g2 - g1 <= g1, "the n-gram graphs are the ids-mode ones only"
        np.testing.assert_array_equal(b_ids, want); np.testing.assert_array_equal(b_lens, want_l)
        with pytest.raises(ValueError):
            eng.recognize_gray(gray, 16, no_repeat_ngram=[3] * 39)
        with pytest.raises(ValueError):
            eng.recognize_gray(gray, 16, no_repeat_ngram=-1)
        sizes = np.zeros(40, np.int32); sizes[7] = eng.spec.max_len + 1
        ids_ = np.zeros((40, eng.spec.max_len), np.int32); lens_ = np.zeros(40, np.int32)
        rc = eng.lib.mocr_recognize_gray_host_norepeat(eng._h, gray.ctypes.data, 40, 16, ids_.ctypes.data, lens_.ctypes.data, None, None,
                                                       None, None, sizes.ctypes.data)
        assert rc != 0, "a size above max_len must be MOCR_ERR_ARG"
        with pytest.raises(MocrError):
            eng._check(rc)
    finally:
        eng.close()


def test_product_surface_no_repeat_ngram():
    from PIL import Image
    from manga_ocr import MangaOcr
    imgs = [Image.fromarray(g) for g in crops(77, 4)]
    m = MangaOcr(synthetic_seed=0, dtype="fp32", max_batch=8, lanes=1, batch_timeout_ms=2000.0)
    try:
        assert m.no_repeat_ngram_size is None and m.ignored_generation_config == {}
        free = m.recognize_batch_alternatives(imgs)
        got3 = m.recognize_batch_alternatives(imgs, no_repeat_ngram=3)
        got2 = m.recognize_batch(imgs, no_repeat_ngram=2)
        for r in got3:
            assert nu.first_repeat(r.ids, 3) is None and (r.alt_ids[:, 0] == r.ids[1:]).all()
        per = m.recognize_batch(imgs, no_repeat_ngram=[3, 0, 2, 3])
        assert per == [got3[0].text, free[1].text, got2[2], got3[3].text]
        # concurrent single-crop callers with different n land in one batch (the batcher's window is 2 s) and each gets its own
        before = m.engine.decode_slot_steps()
        sizes = [3, 0, 2, 3]
        out = [None] * 4
        ths = [threading.Thread(target=lambda i=i: out.__setitem__(i, m.recognize(imgs[i], no_repeat_ngram=sizes[i]))) for i in range(4)]
        [t.start() for t in ths]; [t.join() for t in ths]
        assert out == per
        one = m.engine.decode_slot_steps() - before
        before = m.engine.decode_slot_steps()
        m.recognize_batch(imgs, no_repeat_ngram=sizes)
        assert one == m.engine.decode_slot_steps() - before, "the four callers were not decoded as one batch"
        assert m(imgs[1]) == free[1].text and m.recognize_scored(imgs[0], no_repeat_ngram=3).text == got3[0].text
    finally:
        m.close()
    m = MangaOcr(synthetic_seed=0, dtype="fp32", max_batch=8, lanes=1, no_repeat_ngram_size=3)
    try:
        assert m.no_repeat_ngram_size == 3
        assert m.recognize_batch(imgs) == [r.text for r in got3] and m(imgs[0]) == got3[0].text
        assert m.recognize_batch(imgs, no_repeat_ngram=0) == [r.text for r in free]
    finally:
        m.close()
