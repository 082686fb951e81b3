"""-m gpu: every tile form of the fused LM head on the ring it ships with, exactly.

TileFamily (csrc/engine.hip) builds gemm_kernel's vocabulary epilogues in 72 forms per storage type (tests/lm_head_forms_util.py
states the list; tests/test_lm_head_forms_cpu.py holds it against tile_forms()'s rule), and tile_launch gives every small launch
four ring slots - so the kernel tests of the masked, scored, soft and penalised heads ran four-slot forms, while a batch of 136
rows and more runs two-slot ones, on 128 x 128 tiles from 1024 rows: there the fp32 epilogue tile is the WHOLE ring (64 KiB).
Here one case is one (storage type, tile, ring): N 6144, K 768, M the smallest row count that gets the ring on this device with
a ragged last M-tile of one row (ring 2: one M-tile more than one block per compute unit holds - 641 / 129 rows on 256 units;
ring 4: tile + 1 rows), and its 18 forms run on shared operands through the seven mocr_op_gemm_argmax* / _topk hooks.  After
every launch mocr_last_tile_launch must report the case's (tile, ring): the test proves it ran the form it names.

Operands (lm_head_forms_util.build): dyadic and live in every K-tile, so every sum is exact and a K-tile dropped, doubled or
read from the wrong slot changes it; permuted rowmap, ten row kinds in every M-tile, seen and banned columns on tile and word
corners.  cand_val / cand_idx, the four best and tgt_val equal the numpy fp32 mirror bit for bit (ties: the lowest column);
the logsumexp merged from cand_val and cand_sum is within 8 x max(fp32 logsumexp's own error, spacing of the reference) of
the float64 one (the exact-input rule of tests/test_gpu_constraints.py); rows behind M stay untouched.  On the ring-2 shapes
also: PEN with p = 1 == the SOFT hook, SOFT with every state NONE or with null tables == the target / masked hook, and the
first M-tile's rows == a launch of those rows alone, which is a four-slot one - all bit for bit."""
import functools
import types

import numpy as np
import pytest

from gpu_util import report

import constraint_util as cu
import lm_head_forms_util as fu
import score_util as su
from test_gpu_constraints import _f32, _i32, _t, _u32
from test_gpu_decode_regimes import _cus

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

D, V, K4 = fu.D, fu.V, fu.K4
SENT, GUARD = -777, 3
NAMES = ("cand_val", "cand_idx", "cand_sum", "top_val", "top_idx", "tgt_val")
CASES = [(dtype, tile, ring) for dtype in ("fp32", "bf16") for tile in fu.TILES for ring in fu.RINGS]


@functools.lru_cache(maxsize=2)
def _device_weights(dtype):
    W, bias = fu.weights()
    return _t(W.copy(), dtype), _f32(bias.copy())      # (the cached arrays are read-only)


def _device_case(c, dtype):
    eb, et, ew = c.tables
    dW, db = _device_weights(dtype)
    return types.SimpleNamespace(
        A=_t(c.A, dtype), W=dW, bias=db, table=_u32(cu.pack_sets(c.masks)), sor=_i32(c.set_of_row), rowmap=_i32(c.rowmap),
        prefix=_i32(c.prefix), plen=_i32(c.plen), step=_i32(c.step), state=_i32(c.state), none=_i32(np.full(c.R, fu.NONE)),
        tabs=dict(d_edge_begin=_i32(eb), d_edge_token=_i32(et), d_edge_weight=_f32(ew)), seen=_u32(cu.pack_sets(c.seen)), p=_f32(c.p),
        ones=_f32(np.ones(c.R)))


def _launch(eng, c, d, v, want_ring, *, rows=None, hook=None, tables=True, state=None, pen=None):
    """one launch of variant v's outputs through its hook (or `hook`) on fresh NaN / sentinel outputs with GUARD rows behind
    them -> the six outputs' first `rows` rows (None where the form has none); the launch's record must name the tile and ring"""
    M, nt, tile = rows or c.M, c.nt, c.tile
    name, given = fu.hook_of(v)
    name = hook or name
    cv = torch.full((M + GUARD, nt), float("nan"), device="cuda")
    ci = torch.full((M + GUARD, nt), SENT, dtype=torch.int32, device="cuda")
    cs = cv.clone() if given["cs"] else None
    tv = torch.full((M + GUARD, nt, K4), float("nan"), device="cuda") if given["top"] else None
    ti = torch.full((M + GUARD, nt, K4), SENT, dtype=torch.int32, device="cuda") if given["top"] else None
    tg = torch.full((M + GUARD,), float("nan"), device="cuda") if given["target"] else None
    pre = (d.prefix, d.plen, c.ld, d.step, tg) if given["target"] else (None, None, 0, None, None)
    head = (d.A, d.W, d.bias, cv, ci)
    sets = (d.table, d.sor, d.rowmap)
    soft = dict(d_aut_state=d.state if state is None else state, **d.tabs) if tables else {}
    torch.cuda.synchronize()
    if name == "op_gemm_argmax":
        eng.op_gemm_argmax(*head, M, V, D, tile)
    elif name == "op_gemm_argmax_lse":
        eng.op_gemm_argmax_lse(*head, cs, M, V, D, tile)
    elif name == "op_gemm_topk":
        eng.op_gemm_topk(*head, cs, tv, ti, M, V, D, tile)
    elif name == "op_gemm_argmax_masked":
        eng.op_gemm_argmax_masked(*head, cs, tv, ti, M, V, D, tile, *sets)
    elif name == "op_gemm_argmax_target":
        eng.op_gemm_argmax_target(*head, cs, tv, ti, M, V, D, tile, *sets, *pre)
    elif name == "op_gemm_argmax_soft":
        eng.op_gemm_argmax_soft(*head, cs, tv, ti, M, V, D, tile, *sets, *pre, **soft)
    else:
        assert name == "op_gemm_argmax_penalty", name
        eng.op_gemm_argmax_penalty(*head, cs, tv, ti, M, V, D, tile, *sets, *pre, **soft, d_seen_mask=d.seen,
                                   d_penalty_of_row=d.p if pen is None else pen)
    rec = eng.last_tile_launch()
    assert (rec["tile"], rec["ring"], rec["split"]) == (tile, want_ring, 1), f"{name} {fu.form_name(fu.Form(*v, tile, want_ring))} M={M}: launched {rec}"
    out = [None if x is None else x.cpu().numpy() for x in (cv, ci, cs, tv, ti, tg)]
    for n_, x in zip(NAMES, out):
        if x is not None:
            assert (np.isnan(x[M:]) if x.dtype == np.float32 else x[M:] == SENT).all(), f"{name}: rows >= M of {n_} written"
    return [None if x is None else x[:M] for x in out]


def _same(got, want, what, rows=None, which=slice(None)):
    """bit for bit: the outputs `which` of two launches, over their first `rows` rows"""
    for n_, g, w_ in zip(NAMES[which], got[which], want[which]):
        assert (g is None) == (w_ is None), (what, n_)
        if g is not None:
            np.testing.assert_array_equal(g[:rows].view(np.uint32), w_[:rows].view(np.uint32), err_msg=f"{what}: {n_}")


def _check(out, ref, c, v, what) -> float:
    """the exact outputs against the mirror; -> the worst logsumexp err / tol (0 for the ids forms)"""
    gv, gi, gs, gtv, gti, gtg = out
    assert not np.isnan(gv).any(), f"{what}: NaN"
    np.testing.assert_array_equal(gv.astype(np.float64), ref.cand_val, err_msg=f"{what}: cand_val")
    np.testing.assert_array_equal(gi, ref.cand_idx, err_msg=f"{what}: cand_idx")
    if gtv is not None:
        np.testing.assert_array_equal(gti, ref.top_idx, err_msg=f"{what}: top_idx is not the lexicographic top four")
        np.testing.assert_array_equal(gtv.astype(np.float64), ref.top_val, err_msg=f"{what}: top_val")
    if gtg is not None:
        np.testing.assert_array_equal(gtg[c.has_tgt].astype(np.float64), ref.tgt[c.has_tgt], err_msg=f"{what}: tgt_val")
        assert np.isnan(gtg[~c.has_tgt]).all(), f"{what}: a row without a target had tgt_val written"
    if gs is None:
        return 0.0
    assert not np.isnan(gs).any() and (gs[np.isfinite(gv)] >= 1).all() and (gs[np.isneginf(gv)] == 0).all(), f"{what}: cand_sum"
    err = np.abs(cu.masked_merge_tiles(gv, gs) - ref.lse)
    ratio = float((err / ref.tol).max())
    print(f"{what}: logsumexp max err {err.max():.3e}, tol min {ref.tol.min():.3e}, err / tol {ratio:.3f}", flush=True)
    assert (err <= ref.tol).all(), f"{what}: logsumexp of row {int(np.argmax(err / ref.tol))} off by {err.max():.3e}"
    return ratio


@pytest.mark.parametrize("dtype,tile,ring", CASES, ids=[fu.case_id(*c) for c in CASES])
def test_every_lm_head_form_exact(dtype, tile, ring):
    """the 18 forms of one (tile, ring) - fu.variants() - on the case's shared operands; PEN also without tables (the same form:
    a penalty without any automaton).  Ring 2 only: the degenerate riches and the first M-tile alone on four slots."""
    eng = su.score_engine("wide", dtype)
    cus = _cus()
    M = fu.rows_for(tile, ring, cus)
    if fu.ring_rule(dtype, M, tile, cus) != ring or M <= tile or M % tile != 1:
        pytest.skip(f"{cus} compute units: no row count with a full and a one-row M-tile gets ring {ring} on the {tile} tile "
                    f"({M} rows: ring {fu.ring_rule(dtype, M, tile, cus)})")
    c = fu.build(tile, M)
    d = _device_case(c, dtype)
    tag = f"LM head forms {fu.case_id(dtype, tile, ring)} M={M}"
    outs, worst = {}, 0.0
    for v in fu.variants():
        what = f"{tag} {fu.form_name(fu.Form(*v, tile, ring))}"
        outs[v] = _launch(eng, c, d, v, ring)
        worst = max(worst, _check(outs[v], fu.reference(c, v.masked, v.rich), c, v, what))
        if v.rich == "pen":
            bare = _launch(eng, c, d, v, ring, tables=False)
            worst = max(worst, _check(bare, fu.reference(c, True, "pen", False), c, v, what + " without tables"))
    # the forms agree bit for bit on what they share: candidates of the three levels, exp sums of scored and alternatives,
    # everything but tgt_val with and without a target column
    for v in fu.variants():
        what = f"{tag} {fu.form_name(fu.Form(*v, tile, ring))}"
        _same(outs[v], outs[fu.Variant("ids", v.masked, False, v.rich)], f"{what} against the ids form", which=slice(0, 2))
        if v.level == "alternatives":
            _same(outs[v], outs[v._replace(level="scored")], f"{what} against the scored form", which=slice(2, 3))
        if v.tgt:
            _same(outs[v], outs[v._replace(tgt=False)], f"{what} against the form without a target", which=slice(0, 5))
    extra = ""
    if ring == 2:
        for level, tgt in (("ids", False), ("scored", False), ("scored", True), ("alternatives", False), ("alternatives", True)):
            plain, soft, pen = (fu.Variant(level, True, tgt, rich) for rich in fu.RICHES)
            name = f"{tag} {level}{' TGT' if tgt else ''}"
            _same(_launch(eng, c, d, pen, ring, pen=d.ones), outs[soft], f"{name}: PEN with p = 1 against the _soft hook")
            _same(_launch(eng, c, d, soft, ring, state=d.none), outs[plain], f"{name}: SOFT with every state NONE against the hook below")
            _same(_launch(eng, c, d, plain, ring, hook="op_gemm_argmax_soft", tables=False), outs[plain], f"{name}: the _soft hook with null tables")
        # the first M-tile's rows alone: at most one block per compute unit, so four slots - same K order, same sums
        alone = 4 if cus == 256 else fu.ring_rule(dtype, tile, tile, cus)
        for v in fu.variants():
            one = _launch(eng, c, d, v, alone, rows=tile)
            _same(one, outs[v], f"{tag} {fu.form_name(fu.Form(*v, tile, ring))}: the first M-tile against its own ring-{alone} launch", rows=tile)
        extra = f"; PEN p = 1 == _soft, SOFT all NONE / null tables == _target / _masked, first M-tile == its own ring-{alone} launch, bit for bit"
    report(f"{tag}: mocr_last_tile_launch confirmed tile {tile} ring {ring} on {-(-M // tile) * c.nt} blocks ({cus} CUs) for all 18 forms "
           f"(+ 5 PEN without tables): candidates, four best and tgt_val == the numpy fp32 mirror bit for bit, rows >= M untouched, "
           f"worst logsumexp err / tol {worst:.3f}{extra}")
