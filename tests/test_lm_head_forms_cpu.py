"""The fused LM head's tile forms without a device: the case list of tests/test_gpu_lm_head_forms.py is TileFamily's (csrc/engine.hip
tile_forms(): 72 vocabulary forms per storage type), every form has one hook call that asks for it, and the operand builder's
construction asserts hold at the shapes a device of 256 compute units gives."""
import collections

import pytest

import lm_head_forms_util as fu

CUS = 256


def test_case_list_is_the_families():
    forms = fu.forms()
    assert len(forms) == 72 and len(set(forms)) == 72
    per = collections.Counter((f.tile, f.ring) for f in forms)
    assert per == {(t, r): 18 for t in fu.TILES for r in fu.RINGS}
    for f in forms:
        assert not f.tgt or (f.masked and f.level in ("scored", "alternatives")), f
        assert f.rich == "plain" or f.masked, f
    # tile_forms()'s own count: per (tile, ring) 3 unmasked, EPI_ARGMAX_M in 3 riches, the two scored ones in 2 x 3
    assert collections.Counter(fu.EPI_NAME[(f.level, f.masked)] for f in forms if (f.tile, f.ring) == (64, 2)) == {
        "EPI_ARGMAX": 1, "EPI_ARGMAX_LSE": 1, "EPI_TOPK": 1, "EPI_ARGMAX_M": 3, "EPI_ARGMAX_LSE_M": 6, "EPI_TOPK_M": 6}
    new = fu.untested_before()
    assert len(new) == 24 and len(set(new)) == 24 and set(new) <= set(forms)
    on128 = [f for f in new if f.tile == 128]
    assert len(on128) == 17 and all(f.ring == 2 for f in new)
    assert collections.Counter(fu.EPI_NAME[(f.level, f.masked)] for f in on128) == {
        "EPI_ARGMAX_LSE": 1, "EPI_TOPK": 1, "EPI_ARGMAX_M": 3, "EPI_ARGMAX_LSE_M": 6, "EPI_TOPK_M": 6}
    assert sorted(fu.form_name(f) for f in new if f.tile == 64) == sorted([
        "EPI_ARGMAX_M PEN", "EPI_ARGMAX_LSE_M PEN", "EPI_ARGMAX_LSE_M TGT PEN", "EPI_TOPK_M PEN", "EPI_TOPK_M TGT PEN",
        "EPI_ARGMAX_LSE_M TGT", "EPI_TOPK_M TGT"])


def test_every_form_has_its_hook_call():
    """what a hook is given makes launch_gemm_tile's key the form's: 18 distinct keys, one per form of a (tile, ring)"""
    keys = {}
    for v in fu.variants():
        hook, given = fu.hook_of(v)
        assert hook in ("op_gemm_argmax", "op_gemm_argmax_lse", "op_gemm_topk", "op_gemm_argmax_masked", "op_gemm_argmax_target",
                        "op_gemm_argmax_soft", "op_gemm_argmax_penalty")
        assert fu.key_of(hook, given) == (fu.EPI_NAME[(v.level, v.masked)], v.tgt, v.rich != "plain", v.rich == "pen"), v
        keys[fu.key_of(hook, given)] = v
        if v.rich == "pen":       # without tables: the same form
            assert fu.key_of(hook, dict(given, tables=False)) == fu.key_of(hook, given)
    assert len(keys) == 18


def test_rows_reach_the_ring_on_256_units():
    want = {(128, 2): (641, 6, 288), (64, 2): (129, 3, 288), (128, 4): (129, 2, 96), (64, 4): (65, 2, 192)}
    for (tile, ring), (M, ntm, blocks) in want.items():
        assert fu.rows_for(tile, ring, CUS) == M
        assert (-(-M // tile), -(-M // tile) * (fu.V // tile)) == (ntm, blocks)
        for dtype in ("fp32", "bf16"):
            assert fu.ring_rule(dtype, M, tile, CUS) == ring
            if ring == 2:         # the smallest such shape: one M-tile less is a four-slot launch, which is the first tile's own launch
                assert fu.ring_rule(dtype, M - tile, tile, CUS) == 4 and fu.ring_rule(dtype, tile, tile, CUS) == 4


@pytest.mark.parametrize("tile,ring", [(t, r) for t in fu.TILES for r in fu.RINGS])
def test_operands_hold_what_the_cases_are_for(tile, ring):
    """fu.build asserts, on the reference: exact fp32 logits below 64 that are live in every K-tile, by-ROW arrays that differ from
    their by-slot reading in every M-tile, every row kind in every full M-tile, the ragged tile's row under mask, weight,
    penalty and target, targets that are seen / banned / absent; and the mirror of every (masked, rich) is finite where allowed"""
    c = fu.build(tile, fu.rows_for(tile, ring, CUS))
    assert c.A.shape == (c.Mp, fu.D) and c.Mp % tile == 0 and c.Mp - c.M == tile - 1
    import numpy as np
    assert np.isnan(c.A[c.M:]).all() and np.isfinite(c.A[:c.M]).all()
    for masked, rich, tables in ((False, "plain", True), (True, "plain", True), (True, "soft", True), (True, "pen", True), (True, "pen", False)):
        r = fu.reference(c, masked, rich, tables)
        assert np.isfinite(r.lse).all() and (r.tol > 0).all() and not np.isnan(r.cand_val).any()
        assert (r.top_idx[..., 0] == r.cand_idx).all() and (r.top_val[..., 0] == r.cand_val).all()
        assert (np.isnan(r.tgt) == ~c.has_tgt).all()
        if masked:
            assert np.isneginf(r.tgt[c.has_tgt]).any() and np.isfinite(r.tgt[c.has_tgt]).any()
