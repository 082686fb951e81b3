"""CPU: the token-score feature's host side - the scored exports exist and are declared, the ABI did not move, the
``Recognition`` aggregation, the multi-device refusal, and a numpy model of the tile-wise log-sum-exp merge the kernels
implement (guards the formula independently of any GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
from manga_ocr import _capi, text
from manga_ocr.ocr import MangaOcr, Recognition

import score_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORED = ["mocr_recognize_images_scored", "mocr_recognize_regions_scored", "mocr_recognize_device_scored",
          "mocr_recognize_gray_host_scored", "mocr_op_gemm_argmax_lse", "mocr_op_dec_token_scored"]


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return _capi.load_library()


def test_scored_symbols_are_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, "include", "mocr.h")).read()
    for name in SCORED:
        assert name in _capi.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in mocr.h"
        assert getattr(lib, name) is not None
    # each scored twin = the unscored signature plus pointer arguments
    for plain, scored, extra in [("mocr_recognize_images", "mocr_recognize_images_scored", 1),
                                 ("mocr_recognize_regions", "mocr_recognize_regions_scored", 1),
                                 ("mocr_recognize_device", "mocr_recognize_device_scored", 1),
                                 ("mocr_recognize_gray_host", "mocr_recognize_gray_host_scored", 1),
                                 ("mocr_op_dec_token", "mocr_op_dec_token_scored", 2)]:
        a, b = _capi.SYMBOLS[plain][1], _capi.SYMBOLS[scored][1]
        assert b[:len(a)] == a and b[len(a):] == [C.c_void_p] * extra, scored


def test_abi_version_and_token_args_size_are_unchanged(lib):
    assert lib.mocr_abi_version() == 2
    hdr = open(os.path.join(ROOT, "include", "mocr.h")).read()
    assert re.search(r"#define\s+MOCR_ABI_VERSION\s+2\b", hdr)
    # mocr_token_args as ABI 2 shipped it (11 int32 / float and 14 pointers with their padding): 25 fields, 160 bytes on LP64
    assert C.sizeof(_capi.MocrTokenArgs) == 160
    assert len(_capi.MocrTokenArgs._fields_) == 25 and _capi.MocrTokenArgs._fields_[-1][0] == "inv_sx"
    body = hdr[hdr.index("typedef struct mocr_token_args {"):hdr.index("} mocr_token_args;")]
    assert "cand_sum" not in body and "scores" not in body
    # null handles are refused before anything is dereferenced: the scored entry points are real functions
    assert lib.mocr_recognize_images_scored(None, None, 1, None, None, None) == -1
    assert lib.mocr_op_gemm_argmax_lse(None, None, None, None, None, None, None, 1, 64, 64, 64) == -1


def test_recognition_aggregates_hand_made_rows():
    v = text.Vocab.synthetic(6144)
    ids = np.array([2, 5, 6, 3, 0, 0], np.int32)
    logp = np.array([0.0, np.log(0.5), np.log(0.25), np.log(0.5), 0.0, 0.0], np.float32)
    r = Recognition.from_row(v, ids, logp, 4)
    assert r.text == text.ids_to_text(v, [2, 5, 6, 3]) == "一丁"
    np.testing.assert_array_equal(r.ids, [2, 5, 6, 3])
    assert r.logprobs.dtype == np.float32 and r.logprobs.shape == (3,)          # generated tokens only, start dropped
    np.testing.assert_allclose(r.logprobs, np.log([0.5, 0.25, 0.5]), rtol=1e-6)
    assert r.confidence == pytest.approx((0.5 * 0.25 * 0.5) ** (1 / 3), rel=1e-6)   # geometric mean
    assert r.confidence == pytest.approx(float(np.exp(r.logprobs.astype(np.float64).mean())), rel=1e-12)
    assert r.min_prob == pytest.approx(0.25, rel=1e-6)
    # a certain row; a sliver region (length 0); a row that is the start token alone
    sure = Recognition.from_row(v, ids, np.zeros(6, np.float32), 4)
    assert sure.confidence == 1.0 and sure.min_prob == 1.0
    empty = Recognition.from_row(v, np.zeros(6, np.int32), np.zeros(6, np.float32), 0)
    assert empty.text == "" and empty.confidence == 0.0 and empty.min_prob == 0.0 and empty.ids.size == 0 and empty.logprobs.size == 0
    lone = Recognition.from_row(v, ids, logp, 1)
    assert lone.confidence == 0.0 and lone.logprobs.size == 0
    with pytest.raises(Exception):
        r.text = "x"                                                             # frozen


def test_scored_calls_refuse_several_devices_without_spawning_workers():
    from manga_ocr.multi import MultiGpuEngine
    eng = object.__new__(MultiGpuEngine)          # no __init__: no child process, no GPU
    with pytest.raises(NotImplementedError, match="several devices"):
        eng.recognize_images([np.zeros((8, 8), np.uint8)], scores=True)
    with pytest.raises(NotImplementedError, match="several devices"):
        eng.recognize_regions([np.zeros((8, 8, 3), np.uint8)], [(0, 0, 0, 4, 4)], scores=True)
    ocr = object.__new__(MangaOcr)
    ocr.engine = eng
    ocr.vocab = text.Vocab.synthetic(6144)
    from PIL import Image
    for call in (lambda: ocr.recognize_scored(Image.new("L", (8, 8))),
                 lambda: ocr.recognize_batch_scored([Image.new("L", (8, 8))]),
                 lambda: ocr.recognize_bgr_scored([np.zeros((8, 8, 3), np.uint8)]),
                 lambda: ocr.recognize_regions_scored([np.zeros((8, 8, 3), np.uint8)], [(0, 0, 0, 4, 4)])):
        with pytest.raises(NotImplementedError, match="several devices"):
            call()


def test_tiled_merge_equals_float64_logsumexp_on_peaked_oracle_logits():
    """-log sum_c s_c exp(m_c - M) is the chosen token's log-probability: the tile-wise merge in float64 equals the
    float64 logsumexp of the whole row to rounding, for both tile widths; with the tile sums formed in float32 (the
    kernels' storage) it stays within 8 x what torch's own float32 logsumexp loses."""
    ids, logits = su.oracle_run("peaked", 11, 4, 12)
    ref = su.lse64(logits)
    chosen = su.chosen_logp64(logits, ids)
    assert chosen.max() <= 0 and chosen.min() < -0.5 and chosen.max() > -0.5        # the peaked set spreads the scores
    e32 = su.f32_lse_error(logits)
    assert 0 < e32 < 1e-5
    for tile in (64, 128):
        np.testing.assert_allclose(su.tiled_lse(logits, tile), ref, rtol=0, atol=1e-12)
        assert np.abs(su.tiled_lse(logits, tile, np.float32) - ref).max() <= 8 * e32
        m, idx, s = su.tile_stats(logits, tile)
        assert (s >= 1).all()
        # greedy: the chosen id is the arg-max, its logit is M, so the score is -log(sum_c s_c exp(m_c - M))
        M = m.max(-1)
        np.testing.assert_array_equal(np.take_along_axis(logits, ids[:, 1:, None], -1)[..., 0], M.astype(np.float32))
        np.testing.assert_allclose(-(su.merge_tiles(m, s) - M), chosen, rtol=0, atol=1e-12)
    # rows that would overflow an un-shifted fp32 exp, and a row of equal logits
    hard = np.zeros((2, 6144), np.float32)
    hard[0] = np.linspace(-60, 60, 6144)
    hard[1] = 3.25
    np.testing.assert_allclose(su.tiled_lse(hard, 64), su.lse64(hard), rtol=0, atol=1e-12)
    assert su.tiled_lse(hard, 128)[1] == pytest.approx(3.25 + np.log(6144), abs=1e-12)
