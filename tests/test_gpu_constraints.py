"""-m gpu: token constraints - per-crop allowed-token sets applied inside the fused LM head.

Bottom up: the masked LM-head epilogue (mocr_op_gemm_argmax_masked) and the masked token kernel (mocr_op_dec_token_masked)
against float64 numpy on the kernels' own inputs, with a permuted rowmap and a different set per row; whole recognitions
against a masked greedy loop on the fp32 oracle (constraint_util.masked_generate); the invariants on every decode path
(nothing outside a row's set, set-0 rows bit-identical to an unconstrained run, the feature off moves nothing); merged
jobs, graph keys, error paths, the Python surface.

Tolerances are the ones of tests/test_gpu_scores.py and tests/test_gpu_alternatives.py, derived there."""
import numpy as np
import pytest

from gpu_util import bf16_round, crops, report

import constraint_util as cu
import score_util as su

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

D, V, K4, EOS = 768, 6144, 4, 3
SENT, GUARD = -777, 2
NO_IDX = cu.NO_IDX
FP32_LOGIT_TOL = 1e-3        # tests/test_gpu_parity.py: fp32 teacher-forced logits
GEMM_REL = 1e-5              # tests/test_gpu_decode_kernels.py: |cand_val err| / sum |a w|
TOKEN_SCORE_TOL = 5e-6       # tests/test_gpu_scores.py: the fp32 evaluation of log(sum exp(x - max)) over <= 6144 terms
BF16_LOGIT_TOL = 3e-2        # tests/test_gpu_bf16_parity.py: teacher-forced bf16 logits
BF16_GAP_TOL = 1.5e-2        # tests/test_gpu_bf16_parity.py: a first divergence only below this reference margin


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def _t(a, dtype):
    t = _f32(a)
    return t.to(torch.bfloat16) if dtype == "bf16" else t


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lex_top(x, k=K4):
    return np.argsort(-np.asarray(x), axis=-1, kind="stable")[..., :k]


def kernel_masks(logits, tile_lo, tile_hi):
    """The seven sets of the kernel tests for logits [n, V] (a set per row kind, applied to row r as set r % 7):
    0 everything, 1 a random half, 2 EOS only, 3 columns [tile_lo, tile_hi) banned, 4 three tokens, 5 every row's free
    argmax banned, 6 every row's lowest-id maximum banned (the rows' ties: see the callers)."""
    rs = np.random.RandomState(77)
    m = np.ones((7, V), bool)
    m[1] = rs.rand(V) < 0.5
    m[2] = cu.mask_of([])
    m[3, tile_lo:tile_hi] = False
    m[4] = cu.mask_of([1500, 5000])
    m[5, np.argmax(logits, -1)] = False
    m[6, np.argmax(logits, -1)] = False
    m[:, EOS] = True
    return m


# ------------------------------------------------------------------------------------------------ 1. LM-head epilogue
def _run_masked_gemm(eng, dA, dW, bias, M, tile, table, set_of_row, rowmap, variant):
    """variant 0 ids, 1 scored, 2 alternatives; table None = the unmasked hooks.  Guard rows behind every output."""
    nt = V // tile
    cv = torch.full((M + GUARD, nt), float("nan"), device="cuda")
    ci = torch.full((M + GUARD, nt), SENT, dtype=torch.int32, device="cuda")
    cs = cv.clone() if variant >= 1 else None
    tv = torch.full((M + GUARD, nt, K4), float("nan"), device="cuda") if variant == 2 else None
    ti = torch.full((M + GUARD, nt, K4), SENT, dtype=torch.int32, device="cuda") if variant == 2 else None
    torch.cuda.synchronize()
    if table is None:
        eng.op_gemm_topk(dA, dW, bias, cv, ci, cs, tv, ti, M, V, D, tile)
    else:
        eng.op_gemm_argmax_masked(dA, dW, bias, cv, ci, cs, tv, ti, M, V, D, tile, table, set_of_row, rowmap)
    out = [None if x is None else x.cpu().numpy() for x in (cv, ci, cs, tv, ti)]
    assert np.isnan(out[0][M:]).all() and (out[1][M:] == SENT).all(), "guard rows of the candidates written"
    for x in out[2:]:
        if x is not None:
            assert (np.isnan(x[M:]) if x.dtype == np.float32 else x[M:] == SENT).all(), "guard rows written"
    return [None if x is None else x[:M] for x in out]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("M", [1, 5, 64, 130])
def test_masked_lm_head_epilogue_against_float64(dtype, tile, M):
    """mocr_op_gemm_argmax_masked, N 6144, K 768, the ids / scored / alternatives forms.  GEMM row m is slot m of a permuted
    rowmap over M + 3 rows; row r decodes under set r % 7 (kernel_masks; set 3 bans exactly tile 1).
    All rows under set 0: every output bit-identical to the unmasked operators'.
    Random floats: the three forms agree bit for bit on what they share; every winner lies in its row's set; cand_val within
    1e-5 x sum |a w| of the float64 masked tile maximum; the merged logsumexp within the scored test's tolerance
    (2 x 1e-5 x sum |a w| + 8 x the fp32 logsumexp error) of the float64 one over the allowed tokens; a tile with no allowed
    column reads (-inf, no index, sum exactly 0, list entries (-inf, no index)); nothing is NaN.
    Exact arithmetic (zero activations: logit = integer bias, ties everywhere, every row the same logits): cand_idx / top_idx
    equal numpy's lexicographic masked top four exactly - incl. the sets that ban the free argmax and the lower id of a tie."""
    eng = su.score_engine("wide", dtype)
    rs = np.random.RandomState(13 * M + tile)
    Mp = (M + tile - 1) // tile * tile
    nt = V // tile
    R = M + 3
    rowmap = rs.permutation(R)[:M].astype(np.int32)
    set_of_row = (np.arange(R) % 7).astype(np.int32)
    sets_m = set_of_row[rowmap]                                      # the set GEMM row m decodes under
    assert M == 1 or (sets_m != set_of_row[:M]).any(), "a kernel reading the set by slot must fail"
    A = np.zeros((Mp, D), np.float32)
    A[:M] = rs.standard_normal((M, D))
    W = (rs.standard_normal((V, D)) * 0.05).astype(np.float32)
    if dtype == "bf16":
        A, W = bf16_round(A), bf16_round(W)
    bias_r = rs.standard_normal(V).astype(np.float32)
    bias_i = rs.randint(-3, 4, size=V).astype(np.float32)
    bias_i[[700, 900]] = 9.0                                         # the row maximum twice: an exact tie, lower id 700
    dW, d_rowmap, d_sor = _t(W, dtype), _i32(rowmap), _i32(set_of_row)
    tile_lo = (np.arange(nt) * tile)[None, :]
    worst = {}
    for case, a_case, bias in (("random", A, bias_r), ("exact", np.zeros_like(A), bias_i)):
        dA, db = _t(a_case, dtype), _f32(bias)
        logits = a_case[:M].astype(np.float64) @ W.astype(np.float64).T + bias
        masks7 = kernel_masks(logits[:1] if case == "exact" else logits, tile, 2 * tile)
        if case == "random":                                         # sets 5 / 6 ban every row's argmax: keep the sets non-trivial
            assert masks7[5].sum() >= V - M
        table = _u32(cu.pack_sets(masks7))
        # ---- all rows under set 0: bit-identical to the unmasked hooks
        zeros = _i32(np.zeros(R))
        for variant in (0, 1, 2):
            want = _run_masked_gemm(eng, dA, dW, db, M, tile, None, None, None, variant)
            got = _run_masked_gemm(eng, dA, dW, db, M, tile, table, zeros, d_rowmap, variant)
            for g, w_ in zip(got, want):
                if g is not None:
                    np.testing.assert_array_equal(g.view(np.uint32), w_.view(np.uint32), err_msg=f"{case}: set 0 differs from the unmasked operator")
        # ---- a set per row
        o0, o1, o2 = (_run_masked_gemm(eng, dA, dW, db, M, tile, table, d_sor, d_rowmap, v) for v in (0, 1, 2))
        for a, b in ((o0[0], o2[0]), (o1[0], o2[0]), (o1[2], o2[2])):
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"{case}: the three forms disagree")
        np.testing.assert_array_equal(o0[1], o2[1]); np.testing.assert_array_equal(o1[1], o2[1])
        gv, gi, gs, gtv, gti = o2
        mask = masks7[sets_m]                                        # [M, V]
        m64, idx64, s64 = cu.masked_tile_stats(logits, mask, tile)
        empty = np.isneginf(m64)
        assert empty[sets_m == 2].sum() == (sets_m == 2).sum() * (nt - 1) and empty[sets_m == 3].sum() == (sets_m == 3).sum()
        assert not np.isnan(gv).any() and not np.isnan(gs).any() and not np.isnan(gtv).any(), "NaN"
        assert np.isneginf(gv[empty]).all() and (gi[empty] == NO_IDX).all(), "a tile with no allowed column has a winner"
        assert (gs[empty] == 0).all(), "the exp sum of a tile with no allowed column is not exactly 0"
        assert np.isneginf(gtv[empty]).all() and (gti[empty] == NO_IDX).all()
        assert np.isfinite(gv[~empty]).all() and (gs[~empty] >= 1).all()
        np.testing.assert_array_equal(_bits(gtv[..., 0]), _bits(gv)); np.testing.assert_array_equal(gti[..., 0], gi)
        real = gti != NO_IDX
        assert ((gti >= tile_lo[..., None]) & (gti < tile_lo[..., None] + tile))[real].all(), "a column outside its tile"
        rows3 = np.broadcast_to(np.arange(M)[:, None, None], gti.shape)
        assert mask[rows3[real], gti[real]].all(), "a column outside its row's set"
        assert np.isneginf(gtv[~real]).all() and np.isfinite(gtv[real]).all(), "a -inf entry with a real column"
        n_allowed = mask.reshape(M, nt, tile).sum(-1)
        np.testing.assert_array_equal(real.sum(-1), np.minimum(n_allowed, K4), err_msg="entries per tile")
        scale = (np.abs(a_case[:M]).astype(np.float64) @ np.abs(W).astype(np.float64).T).max(-1)
        e32 = su.f32_lse_error(np.where(mask, logits, -1e30).astype(np.float32))
        if case == "random":
            allow = GEMM_REL * scale.max()
            e_val = float(np.abs(gv[~empty] - m64[~empty]).max())
            at = np.take_along_axis(logits, np.where(real, gti, 0).reshape(M, -1).astype(np.int64), -1).reshape(gti.shape)
            e_at = float(np.abs(gtv - at)[real].max())
            assert e_val <= allow and e_at <= allow, (e_val, e_at, allow)
            tol = 2 * GEMM_REL * scale + 8 * e32
        else:
            t3 = cu.masked(logits, mask).reshape(M, nt, tile)
            want_i = lex_top(t3) + tile_lo[..., None]
            want_v = np.take_along_axis(t3, want_i - tile_lo[..., None], -1)
            want_i = np.where(np.isneginf(want_v), NO_IDX, want_i)
            np.testing.assert_array_equal(gti, want_i, err_msg="top_idx is not the lexicographic masked top four")
            np.testing.assert_array_equal(gtv.astype(np.float64), want_v)
            assert (want_v[..., 1:] == want_v[..., :-1])[np.isfinite(want_v[..., 1:])].sum() > M * nt // 4, "meant to tie"
            for r in np.nonzero(sets_m >= 5)[0]:                     # the free argmax = the lower id of the tie is banned
                assert gi[r, 700 // tile] != 700 and gi[r, 900 // tile] == 900 and gv[r, 900 // tile] == 9.0
            for r in np.nonzero(sets_m == 0)[0]:
                assert gi[r, 700 // tile] == 700
        got_lse = cu.masked_merge_tiles(gv, gs)
        ref_lse = cu.masked_merge_tiles(m64, s64)
        if case == "exact":                                          # no products: the fp32 format alone, per row
            tol = 8 * np.maximum(e32, np.spacing(np.abs(ref_lse).astype(np.float32)).astype(np.float64))
        err = np.abs(got_lse - ref_lse)
        print(f"masked epilogue {dtype} tile={tile} M={M} {case}: logsumexp max err {err.max():.3e}, tol min {tol.min():.3e}", flush=True)
        assert (err <= tol).all(), f"{case}: row {int(np.argmax(err / tol))} err {err.max():.3e}"
        worst[case] = float((err / tol).max())
    report(f"gemm EPI_*_M {dtype} tile={tile} M={M}: set 0 bit-identical to the unmasked operators (ids / scored / alternatives); per-row sets "
           f"through a permuted rowmap: winners inside the sets, empty tiles (-inf, no index, sum 0), masked logsumexp err / tol "
           f"{worst['random']:.3f} (random) {worst['exact']:.3f} (exact), exact inputs == lexicographic masked top four incl. banned argmax / tie")


# ------------------------------------------------------------------------------------------------ 2. token kernel
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("path", ["cand64", "cand128", "slabs1", "slabs3"])
def test_masked_token_step_against_float64(dtype, path):
    """mocr_op_dec_token_masked, the ids / scored / alternatives forms on the candidate and the slab path (one slab = the
    small-batch step's form).  Logits on a 2^-8 grid, so the order is exact.  Slot s decodes row rowmap[s] (a permutation of
    13 rows) under set row % 7 of kernel_masks (set 3 bans columns 1024 .. 2047: a whole column block of every thread on
    the slab path, 8 / 16 whole tiles on the candidate path); slot 6's row is finished.  Every slot's row maximum sits twice,
    at columns 700 and 900.
    Expected: ids = the lowest allowed id of the masked maximum; alt_ids = the lexicographic masked top four, -1 / -inf beyond
    the set's size; scores / alt_logp within 5e-6 + 2^-23 |ref| of the float64 masked log-softmax; the three forms agree bit
    for bit; all rows under set 0: bit-identical to mocr_op_dec_token_topk."""
    eng = su.score_engine("wide", dtype)
    rs = np.random.RandomState({"slabs1": 21, "slabs3": 23, "cand64": 264, "cand128": 328}[path])
    n, R, max_len, ids_ld = 10, 13, 40, 40
    lg = (np.round(rs.standard_normal((n, V)) * 3 * 256) / 256).astype(np.float64)
    lg[:, [700, 900]] = 25.0
    lg = lg.astype(np.float32).astype(np.float64)
    rowmap = rs.permutation(R)[:n].astype(np.int32)
    set_of_row = (np.arange(R) % 7).astype(np.int32)
    sets_s = set_of_row[rowmap]
    assert (sets_s != set_of_row[:n]).any() and len(set(sets_s.tolist())) >= 5
    masks7 = kernel_masks(lg[:1], 1024, 2048)
    assert not masks7[5, 700] and not masks7[6, 700] and masks7[5, 900]
    mask = masks7[sets_s]
    want_ids, want_lp = cu.masked_top(lg, mask)
    assert (want_ids[sets_s == 2] == [EOS, -1, -1, -1]).all() and (want_ids[sets_s == 4][:, 3] == -1).all()
    assert (want_ids[sets_s >= 5][:, 0] == 900).all() and (want_ids[sets_s == 0][:, :2] == [700, 900]).all()
    step = rs.randint(1, max_len - 3, n).astype(np.int32)
    finished = np.zeros(R, np.int32)
    lens = np.full(R, max_len, np.int32)
    finished[rowmap[6]] = 1; lens[rowmap[6]] = 9
    ids = np.full((R + 1, ids_ld), SENT, np.int32)
    table_np = cu.pack_sets(masks7)

    def inputs(mk):
        """the token kernel's inputs for the sets mk [n, V] (the slab path's do not depend on them)"""
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
        m, idx, s = cu.masked_tile_stats(lg, mk, tile)
        t3 = cu.masked(lg, mk).reshape(n, nt, tile)
        ti = lex_top(t3)
        tv = np.take_along_axis(t3, ti, -1)
        ti = np.where(np.isneginf(tv), NO_IDX, ti + (np.arange(nt) * tile)[None, :, None])
        return dict(cand_val=_f32(m), cand_idx=_i32(idx), ncand=nt), _f32(s), _f32(tv), _i32(ti)

    def run(variant, mk, sor, use_mask=True):
        kw, cand_sum, top_val, top_idx = inputs(mk)
        d = dict(ids=_i32(ids), step=_i32(step), finished=_i32(finished), len=_i32(lens), n_unfinished=_i32([11, SENT]),
                 rowmap=_i32(rowmap), x_f32=torch.full((n + GUARD, D), float("nan"), device="cuda"),
                 x_t=torch.full((n + GUARD, D), float("nan"), device="cuda", dtype=torch.bfloat16 if dtype == "bf16" else torch.float32))
        sc = torch.full((R + 1, ids_ld), float("nan"), device="cuda") if variant >= 1 else None
        ai = torch.full((R + 1, ids_ld, K4), SENT, dtype=torch.int32, device="cuda") if variant == 2 else None
        al = torch.full((R + 1, ids_ld, K4), float("nan"), device="cuda") if variant == 2 else None
        common = dict(first=0, n=n, ids_ld=ids_ld, max_len=max_len, n_real=n, **d, **kw)
        torch.cuda.synchronize()
        if use_mask:
            eng.op_dec_token_masked(cand_sum if variant >= 1 else None, sc, top_val if variant == 2 else None,
                                    top_idx if variant == 2 else None, ai, al, _u32(table_np), _i32(sor), **common)
        else:
            eng.op_dec_token_topk(cand_sum if variant >= 1 else None, sc, top_val if variant == 2 else None,
                                  top_idx if variant == 2 else None, ai, al, **common)
        out = {k: v.float().cpu().numpy() if v.dtype == torch.bfloat16 else v.cpu().numpy() for k, v in d.items()}
        return out, *(None if x is None else x.cpu().numpy() for x in (sc, ai, al))

    # ---- all rows under set 0: the unmasked operator, bit for bit
    ones = np.ones((n, V), bool)
    for variant in (0, 1, 2):
        want = run(variant, ones, np.zeros(R), use_mask=False)
        got = run(variant, ones, np.zeros(R))
        for k in want[0]:
            np.testing.assert_array_equal(got[0][k], want[0][k], err_msg=f"{k}: set 0 differs from the unmasked operator")
        for g, w_ in zip(got[1:], want[1:]):
            if g is not None:
                np.testing.assert_array_equal(g.view(np.uint32), w_.view(np.uint32), err_msg="set 0 differs from the unmasked operator")
    # ---- a set per row
    r0, r1, r2 = (run(v, mask, set_of_row) for v in (0, 1, 2))
    for k in r2[0]:
        np.testing.assert_array_equal(r0[0][k], r2[0][k], err_msg=f"{k}: ids form vs alternatives form")
        np.testing.assert_array_equal(r1[0][k], r2[0][k], err_msg=f"{k}: scored form vs alternatives form")
    np.testing.assert_array_equal(_bits(r1[1]), _bits(r2[1]), err_msg="scores: scored form vs alternatives form")
    got, sc, ai, al = r2
    written = np.zeros((R + 1, ids_ld), bool)
    written[rowmap, step + 1] = True
    assert (ai[~written] == SENT).all() and np.isnan(al[~written]).all() and np.isnan(sc[~written]).all()
    gi, gl, gs = ai[rowmap, step + 1], al[rowmap, step + 1], sc[rowmap, step + 1]
    live = np.arange(n) != 6
    assert (gi[6] == -1).all() and (gl[6] == 0).all() and gs[6] == 0, "the finished row reads -1 / 0"
    assert got["ids"][rowmap[6], step[6] + 1] == 0
    np.testing.assert_array_equal(gi[live], want_ids[live], err_msg="alt_ids is not the lexicographic masked top four")
    np.testing.assert_array_equal(got["ids"][rowmap, step + 1][live], want_ids[live, 0], err_msg="ids is not the masked argmax")
    np.testing.assert_array_equal(_bits(gl[live, 0]), _bits(gs[live]), err_msg="entry 0 is not the score, bit for bit")
    assert not np.isnan(gl).any() and not np.isnan(gs).any(), "NaN"
    missing = want_ids == -1
    assert np.isneginf(gl[missing & live[:, None]]).all(), "a missing entry's log-probability is not -inf"
    ok = live[:, None] & ~missing
    tol = TOKEN_SCORE_TOL + 2.0 ** -23 * np.abs(np.where(ok, want_lp, 0))
    err = np.abs(np.where(ok, gl.astype(np.float64) - np.where(ok, want_lp, 0), 0))
    print(f"masked token step {dtype} {path}: max |alt_logp - ref| {err.max():.3e} (tol >= {TOKEN_SCORE_TOL:.1e})", flush=True)
    assert (err <= tol).all(), f"slot {int(np.argmax((err / tol).max(-1)))} (set {sets_s[int(np.argmax((err / tol).max(-1)))]}): {err.max():.3e}"
    assert (gs[(sets_s == 2) & live] == 0).all(), "a row whose set is EOS alone scores exactly log 1"
    report(f"dec_token MASK {dtype} {path}: set 0 bit-identical to the unmasked operator; per-row sets through a permuted rowmap: ids = masked "
           f"argmax (tie at the banned lower id -> 900), alt_ids == lexicographic masked top four with -1 / -inf beyond the set, "
           f"max err {err.max():.2e} (tol 5e-6 + 2^-23 |ref|), three forms agree, finished row -1 / 0")


# ------------------------------------------------------------------------------------------------ 3. end to end
N_E2E, LEN_E2E = 8, 16


def _e2e_reference(kind):
    """free run, per-row sets (constraint_util.row_masks), the masked oracle run: (free ids, masks, ids, logits)"""
    if kind not in _e2e_reference.cache:
        o = su.score_oracle(kind)
        free_ids, _ = su.oracle_run(kind, 31, N_E2E, LEN_E2E)
        masks = cu.row_masks(free_ids, 9)
        with torch.no_grad():
            enc = o.encode(o.preprocess_gray(crops(31, N_E2E)))
        ids, logits = cu.masked_generate(o, enc, masks, LEN_E2E)
        _e2e_reference.cache[kind] = (free_ids, masks, ids, logits)
    return _e2e_reference.cache[kind]


_e2e_reference.cache = {}


@pytest.fixture
def fresh_engine():
    """engines of the test's own, closed after it: their set tables start empty however often the test runs"""
    made = []

    def make(kind, dtype, **kw):
        made.append(su.score_engine.__wrapped__(kind, dtype, **kw))
        return made[-1]
    yield make
    for e in made:
        e.close()


def _handles(eng, masks):
    """a token set per row of masks (set 0 for an all-true row)"""
    return [0 if m.all() else eng.token_set(np.nonzero(m)[0]) for m in masks]


def _check_inside_sets(masks, ids, lens, alt_ids=None, alt_logp=None):
    """no emitted id and no alternative outside its row's set; -1 entries score -inf"""
    for b in range(ids.shape[0]):
        gen = ids[b, 1:lens[b]]
        assert masks[b][gen].all(), f"row {b}: an emitted id outside its set"
        if alt_ids is not None:
            a, l = alt_ids[b, 1:lens[b]], alt_logp[b, 1:lens[b]]
            assert masks[b][a[a >= 0]].all(), f"row {b}: an alternative outside its set"
            assert np.isneginf(l[a < 0]).all() and np.isfinite(l[a >= 0]).all()
            np.testing.assert_array_equal(a[:, 0], gen)
            np.testing.assert_array_equal((a >= 0).sum(-1), np.minimum(int(masks[b].sum()), K4))


@pytest.mark.parametrize("kind", ["wide", "eos"])
def test_fp32_constrained_against_the_masked_oracle(kind):
    """fp32 engine, 8 crops, max_len 16, per-row sets (row 0 set 0, then a random half / the free run's own tokens banned):
    ids identical to the masked greedy loop on the oracle, every constrained row differs from the free run, row 0 does not;
    scores and alternatives within 2 x 1e-3 of the float64 masked log-softmax of the oracle's logits (the scored / alternatives
    tests' fp32 bound); set-0 row bit-identical to an unconstrained run; the ids-only and scored calls give the same ids."""
    free_ids, masks, ids_o, logits = _e2e_reference(kind)
    gaps = cu.masked_gaps(logits, masks)
    L = ids_o.shape[1]
    pad = lambda a: np.pad(a, ((0, 0), (0, LEN_E2E - a.shape[1])))
    assert (pad(ids_o)[0] == pad(free_ids)[0]).all(), "row 0 decodes under set 0"
    for b in range(1, N_E2E):
        assert (pad(ids_o)[b] != pad(free_ids)[b]).any(), f"row {b}: the set changed nothing"
    eng = su.score_engine(kind, "fp32")
    gray = crops(31, N_E2E)
    hs = _handles(eng, masks)
    ids, lens, logp, alt_ids, alt_logp = eng.recognize_gray(gray, LEN_E2E, alternatives=True, token_sets=hs)
    lens_o = np.array([L if EOS not in r[1:] else 2 + list(r[1:]).index(EOS) for r in ids_o])
    live = np.arange(L)[None, :] < lens_o[:, None]
    print(f"fp32 constrained ({kind}): smallest masked top-2 margin of the oracle {gaps[live[:, 1:]].min():.2e}", flush=True)
    np.testing.assert_array_equal(np.where(live, ids[:, :L], 0), np.where(live, ids_o, 0), err_msg="fp32 ids differ from the masked oracle's")
    np.testing.assert_array_equal(lens, lens_o)
    _check_inside_sets(masks, ids, lens, alt_ids, alt_logp)
    tol = 2 * FP32_LOGIT_TOL
    worst = 0.0
    for b in range(N_E2E):
        for t in range(1, lens[b]):
            ref = cu.masked_log_softmax64(logits[b, t - 1], masks[b])
            a = alt_ids[b, t]
            worst = max(worst, abs(float(logp[b, t]) - ref[ids[b, t]]), float(np.abs(alt_logp[b, t][a >= 0] - ref[a[a >= 0]]).max()))
            want4, lp4 = cu.masked_top(logits[b, t - 1], masks[b])
            worst = max(worst, float(np.abs(alt_logp[b, t][a >= 0].astype(np.float64) - lp4[a >= 0]).max()))
    assert worst <= tol, worst
    i0, l0 = eng.recognize_gray(gray, LEN_E2E, token_sets=hs)
    i1, l1, p1 = eng.recognize_gray(gray, LEN_E2E, scores=True, token_sets=hs)
    np.testing.assert_array_equal(i0, ids); np.testing.assert_array_equal(i1, ids); np.testing.assert_array_equal(l0, lens)
    np.testing.assert_array_equal(_bits(p1), _bits(logp))
    fi, fl, fp, fa, fal = eng.recognize_gray(gray, LEN_E2E, alternatives=True)
    np.testing.assert_array_equal(fi[0], ids[0]); np.testing.assert_array_equal(_bits(fp[0]), _bits(logp[0]))
    np.testing.assert_array_equal(fa[0], alt_ids[0]); np.testing.assert_array_equal(_bits(fal[0]), _bits(alt_logp[0]))
    report(f"token constraints fp32 vs the masked oracle, {kind} weights, 8 crops, max_len 16: ids identical (smallest masked margin "
           f"{gaps[live[:, 1:]].min():.1e}), logp / alt_logp within {worst:.2e} (bound {tol:.0e}), set-0 row bit-identical to the free run")


# (name, rows, engine flags).  LATENT_ALWAYS = 64, NO_FUSED_ARGMAX = 16, FP8_ATTENTION = 128.  What the LM head of each does
# (engine.hip decode_step / pick_split, bf16, 64-column tiles): up to 32 rows the small-batch step, whose LM head leaves one
# slab; 64 rows are 96 tiles, below the split-K target of 100: two slabs; 96 rows (max_batch 96: the classic generic step)
# are 192 tiles: no split, so the fused masked epilogue and the candidate path - unless NO_FUSED_ARGMAX sends the same batch
# through the slab GEMM (one slab), which is where that flag changes anything.
BF16_CASES = [("small", 8, 0), ("latent", 64, 64), ("fused", 96, 0), ("nofused", 96, 16), ("fp8", 64, 64 | 128)]


@pytest.mark.parametrize("name,rows,flags", BF16_CASES)
def test_bf16_constrained_paths(name, rows, flags):
    """bf16: 8 rows (small-batch path: the slab form with one slab), 64 rows (latent attention; split-K LM head: two slabs),
    96 rows on the generic step with the fused masked epilogue (candidate path) and with MOCR_FLAG_NO_FUSED_ARGMAX (the same
    step through the slab GEMM), and the fp8-attention engine.  The first 8 rows carry the sets of the fp32 test, the others
    repeat them.  Invariants on every path: nothing outside a row's set, set-0 rows bit-identical to an unconstrained run of the
    same size and kind, the three kinds of constrained call give the same ids.  Not fp8: the first-divergence rule of
    tests/test_gpu_bf16_parity.py on the MASKED margins of the oracle, and the engine's own teacher-forced logits (not
    constrained) within that file's tolerance of the oracle's for the ids the engine emitted."""
    free_ids, masks8, ids_o, logits_o = _e2e_reference("wide")
    eng = su.score_engine("wide", "bf16", max_batch=max(64, rows), flags=flags)
    gray = np.concatenate([crops(31, N_E2E)] * (rows // N_E2E))
    masks = np.concatenate([masks8] * (rows // N_E2E))
    hs = _handles(eng, masks)
    ids, lens, logp, alt_ids, alt_logp = eng.recognize_gray(gray, LEN_E2E, alternatives=True, token_sets=hs)
    _check_inside_sets(masks, ids, lens, alt_ids, alt_logp)
    i0, l0 = eng.recognize_gray(gray, LEN_E2E, token_sets=hs)
    i1, l1, p1 = eng.recognize_gray(gray, LEN_E2E, scores=True, token_sets=hs)
    np.testing.assert_array_equal(i0, ids); np.testing.assert_array_equal(i1, ids); np.testing.assert_array_equal(l1, lens)
    np.testing.assert_array_equal(_bits(p1), _bits(logp))
    fi, fl, fp, fa, fal = eng.recognize_gray(gray, LEN_E2E, alternatives=True)
    z = np.nonzero(np.array(hs) == 0)[0]
    np.testing.assert_array_equal(fi[z], ids[z], err_msg="a set-0 row differs from the unconstrained run")
    np.testing.assert_array_equal(_bits(fp[z]), _bits(logp[z])); np.testing.assert_array_equal(fa[z], alt_ids[z])
    np.testing.assert_array_equal(_bits(fal[z]), _bits(alt_logp[z]))
    assert (ids[8 - 1] != fi[8 - 1]).any(), "the constrained rows were meant to differ from the free run"
    n_div = 0
    if name != "fp8":
        gaps = cu.masked_gaps(logits_o, masks8)
        L = ids_o.shape[1]
        div = cu.first_divergences(ids[:N_E2E, :L], ids_o, gaps)
        n_div = len(div)
        for b, t, g in div:
            report(f"[bf16 constrained {name}] row {b}: first divergence at token {t} (masked oracle margin {g:.3e})")
        assert all(g < BF16_GAP_TOL for _, _, g in div), div
        dg = torch.from_numpy(np.ascontiguousarray(gray[:N_E2E])).cuda()
        torch.cuda.synchronize()
        same = [b for b in range(N_E2E) if b not in {d[0] for d in div}]
        own = eng.decode_logits(dg, N_E2E, ids[:N_E2E, :L - 1])
        d = np.abs(own[same].astype(np.float64) - logits_o[same])
        keep = np.arange(L - 1)[None, :] < (lens[same, None] - 1)
        assert np.isfinite(own).all() and d[keep].max() <= BF16_LOGIT_TOL, d[keep].max()
    report(f"token constraints bf16 {name} ({rows} rows, flags {flags}): nothing outside the sets, set-0 rows bit-identical to the free run, "
           f"ids / logp equal across the three kinds of call; {n_div} first divergences, all below the masked margin {BF16_GAP_TOL}")


def test_feature_off_and_compaction_and_merged_jobs_and_graphs(fresh_engine):
    """Early-EOS weights, 96 rows, max_len 120.  An engine that has created sets and decoded constrained batches gives, for an
    unconstrained call, the ids it gave before it had heard of sets (the feature off); token_sets=None, all-zero handles and
    set-0 rows agree bit for bit; compacted equals uncompacted under constraints (ids and lengths exactly; the scores within twice the
    token-score bound, see below); two jobs with different sets merged into one
    batch equal the same rows decoded alone; constrained and unconstrained decode graphs are kept apart."""
    n, max_len = 96, 120
    gray = np.concatenate([crops(4321, 6), crops(4322, n)])[:n]
    eng = fresh_engine("eos", "bf16", max_batch=96)                     # an engine of its own: no set exists yet
    assert eng.token_set_count() == 1
    g0 = eng.graph_count()
    want_ids, want_lens = eng.recognize_gray(gray, max_len)             # before the engine has heard of sets
    g1 = eng.graph_count()
    rs = np.random.RandomState(2)
    half = eng.token_set(np.nonzero(rs.rand(V) < 0.5)[0])
    ban = eng.token_set(np.setdiff1d(np.arange(V), np.unique(want_ids[:, 1:3])))
    assert (half, ban) == (1, 2) and eng.token_set_count() == 3
    assert eng.token_set(np.nonzero(np.random.RandomState(2).rand(V) < 0.5)[0][::-1]) == half, "the same content gives the same handle"
    hs = np.array([0, half, ban, 0] * (n // 4), np.int32)
    c_ids, c_lens = eng.recognize_gray(gray, max_len, token_sets=hs)
    g2 = eng.graph_count()
    assert g2 > g1 > g0, "the constrained batch did not capture graphs of its own"
    z = hs == 0
    np.testing.assert_array_equal(c_ids[z], want_ids[z]); np.testing.assert_array_equal(c_lens[z], want_lens[z])
    assert (c_ids[~z] != want_ids[~z]).any()
    # the feature off: after sets and constrained batches, unconstrained calls are the parent's
    for kw in ({}, dict(token_sets=None), dict(token_sets=np.zeros(n, np.int32)), dict(token_sets=0)):
        b_ids, b_lens = eng.recognize_gray(gray, max_len, **kw)
        np.testing.assert_array_equal(b_ids, want_ids); np.testing.assert_array_equal(b_lens, want_lens)
    eng.recognize_gray(gray, max_len, token_sets=hs)
    assert eng.graph_count() == g2, "a repeated call captured another decode graph"
    assert c_lens.min() < c_lens.max(), "rows were meant to finish at different steps"
    # compacted == uncompacted
    nc = fresh_engine("eos", "bf16", max_batch=96, flags=2048)          # MOCR_FLAG_NO_COMPACTION
    assert (nc.token_set(np.nonzero(np.random.RandomState(2).rand(V) < 0.5)[0]), nc.token_set(np.setdiff1d(np.arange(V), np.unique(want_ids[:, 1:3])))) == (1, 2)
    u_ids, u_lens, u_lp = nc.recognize_gray(gray, max_len, scores=True, token_sets=hs)
    k_ids, k_lens, k_lp = eng.recognize_gray(gray, max_len, scores=True, token_sets=hs)
    np.testing.assert_array_equal(u_ids, c_ids); np.testing.assert_array_equal(k_ids, c_ids)
    np.testing.assert_array_equal(u_lens, c_lens); np.testing.assert_array_equal(k_lens, c_lens)
    # The scores are NOT bit-identical across a compaction, with or without sets: the LM head's tile (64 / 128 columns) goes by
    # the rows a batch has LEFT (engine.hip dec_launch_tile), which leaves every logit and id alone but groups the exp sums
    # differently.  Both runs evaluate log(sum exp) of the same fp32 logits, each within TOKEN_SCORE_TOL of the exact value.
    f_u, f_k = nc.recognize_gray(gray, max_len, scores=True)[2], eng.recognize_gray(gray, max_len, scores=True)[2]
    d_free, d_con = float(np.abs(f_u - f_k).max()), float(np.abs(u_lp - k_lp).max())
    print(f"compacted vs uncompacted logp: unconstrained max diff {d_free:.3e} ({int((_bits(f_u) != _bits(f_k)).sum())} words differ), "
          f"constrained {d_con:.3e} ({int((_bits(u_lp) != _bits(k_lp)).sum())} words differ); bound {2 * TOKEN_SCORE_TOL:.0e}", flush=True)
    assert np.isfinite(u_lp).all() and np.isfinite(k_lp).all() and d_con <= 2 * TOKEN_SCORE_TOL
    assert eng.compaction_count() > 0 and nc.compaction_count() == 0
    # two jobs with different sets, merged by the scheduler into one batch (device entry point: asynchronous submissions)
    dg = torch.from_numpy(gray).cuda()
    L = eng.spec.max_len
    h = n // 2
    outs = [(torch.zeros((h, L), dtype=torch.int32, device="cuda"), torch.zeros(h, dtype=torch.int32, device="cuda")) for _ in range(2)]
    eng.set_generate_max_length(max_len)
    torch.cuda.synchronize()
    eng.recognize_device(dg[:h], h, outs[0][0], outs[0][1], token_sets=hs[:h])
    eng.recognize_device(dg[h:], h, outs[1][0], outs[1][1], token_sets=ban)
    eng.synchronize()
    eng.set_generate_max_length(L)
    np.testing.assert_array_equal(outs[0][0].cpu().numpy(), c_ids[:h])
    ban_ids, _ = eng.recognize_gray(gray, max_len, token_sets=ban)      # the same 96-row regime, every row under `ban`
    np.testing.assert_array_equal(outs[1][0].cpu().numpy(), ban_ids[h:])
    report(f"token constraints bf16 early-EOS 96 rows: feature off == an engine without sets, set-0 rows bit-identical, compacted == uncompacted, "
           f"two merged jobs == alone, graphs {g0} -> {g1} (free) -> {g2} (constrained), none added by repeats")


def test_error_paths_and_full_table(fresh_engine):
    from manga_ocr._capi import MocrError
    eng = fresh_engine("wide", "fp32", max_batch=8, flags=2)            # an engine of its own: the table gets filled
    gray = crops(1, 2)
    for bad in ([], [V], [-1], [5, V + 3]):
        with pytest.raises(MocrError):
            eng.token_set(bad)
    with pytest.raises(MocrError, match="unknown token set"):
        eng.recognize_gray(gray, 8, token_sets=[0, 1])                  # no set created yet
    with pytest.raises(MocrError, match="unknown token set"):
        eng.recognize_gray(gray, 8, token_sets=[-1, 0])
    with pytest.raises(ValueError):
        eng.recognize_gray(gray, 8, token_sets=[0])
    assert eng.token_set([EOS]) == eng.token_set([EOS, EOS]) == 1       # duplicates are fine, EOS is added anyway
    assert eng.token_set([7]) == eng.token_set([EOS, 7, 7]) == 2
    for h in range(3, 256):
        assert eng.token_set([h + 100]) == h
    assert eng.token_set_count() == 256
    with pytest.raises(MocrError, match="full"):
        eng.token_set([4000])
    assert eng.token_set([255 + 100]) == 255, "an existing set is still found when the table is full"
    ids, lens = eng.recognize_gray(gray, 8, token_sets=[255, 1])
    assert set(ids[0, 1:lens[0]].tolist()) <= {EOS, 355} and ids[1, 1] == EOS and lens[1] == 2
    with pytest.raises(MocrError, match="unknown token set"):
        eng.recognize_gray(gray, 8, token_sets=[256, 0])


def test_product_surface_allowed():
    from PIL import Image
    from manga_ocr import MangaOcr
    m = MangaOcr(synthetic_seed=0, dtype="fp32", max_batch=8, lanes=1)
    try:
        imgs = [Image.fromarray(g) for g in crops(77, 4)]
        free = m.recognize_batch_alternatives(imgs)
        used = "".join(sorted({ch for r in free for ch in r.text}))
        keep = m.token_set(chars=used[: len(used) // 2])
        assert m.token_set(chars=used[: len(used) // 2]) is keep and keep.handle >= 1
        drop = m.token_set(exclude_chars=used)
        allowed = set(m.vocab.ids_for_chars(used[: len(used) // 2])) | {EOS}
        got = m.recognize_batch_alternatives(imgs, allowed=keep)
        for r in got:
            assert set(r.ids[1:].tolist()) <= allowed and set(r.alt_ids[r.alt_ids >= 0].tolist()) <= allowed
            assert all(len(r.candidates(k)) == min(4, len(allowed)) for k in range(len(r.logprobs)))
        for r in m.recognize_batch_scored(imgs, allowed=drop):
            assert not (set(r.text) & set(used))
        per = m.recognize_batch(imgs, allowed=[keep, 0, drop, keep])
        assert per[0] == got[0].text and per[3] == got[3].text and per[1] == free[1].text
        assert m.recognize(imgs[0], allowed=keep) == got[0].text and m.recognize_scored(imgs[2], allowed=drop).text == per[2]
        assert m.recognize_alternatives(imgs[0], allowed=keep).alt_ids[:, 0].tolist() == got[0].alt_ids[:, 0].tolist()
        assert m(imgs[1]) == free[1].text and m.recognize_batch(imgs) == [r.text for r in free]
        with pytest.raises(ValueError):
            m.recognize_batch(imgs, allowed=[keep])
    finally:
        m.close()
