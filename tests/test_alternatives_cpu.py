"""CPU: the token-alternatives feature's host side - the new exports exist, are declared and mirrored, the ABI did not
move, ``Recognition`` keeps its old constructions and names candidates, the multi-device refusal, the batcher's dispatch of
mixed request kinds on a fake engine, and a numpy statement of the merge the kernels rely on: the four best of a row are the
four best of the union of its tiles' four best."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
from manga_ocr import _capi, text
from manga_ocr.ocr import MangaOcr, Recognition, _Batcher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mocr_recognize_images_alts", "mocr_recognize_regions_alts", "mocr_recognize_device_alts", "mocr_recognize_gray_host_alts",
       "mocr_op_gemm_topk", "mocr_op_dec_token_topk"]
P = C.c_void_p


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return _capi.load_library()


def test_alternatives_symbols_are_exported_declared_and_mirrored(lib):
    hdr = open(os.path.join(ROOT, "include", "mocr.h")).read()
    for name in NEW:
        assert name in _capi.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in mocr.h"
        assert getattr(lib, name) is not None
    # every recognise twin = the scored signature plus the two pointers; the token hook = the scored hook plus four
    for scored, alts, extra in [("mocr_recognize_images_scored", "mocr_recognize_images_alts", 2),
                                ("mocr_recognize_regions_scored", "mocr_recognize_regions_alts", 2),
                                ("mocr_recognize_device_scored", "mocr_recognize_device_alts", 2),
                                ("mocr_recognize_gray_host_scored", "mocr_recognize_gray_host_alts", 2),
                                ("mocr_op_dec_token_scored", "mocr_op_dec_token_topk", 4)]:
        a, b = _capi.SYMBOLS[scored][1], _capi.SYMBOLS[alts][1]
        assert b[:len(a)] == a and b[len(a):] == [P] * extra, alts
        assert _capi.SYMBOLS[alts][0] is C.c_int
    # the GEMM hook = the arguments of mocr_op_gemm_argmax_lse with d_top_val, d_top_idx in front of the four sizes
    a, b = _capi.SYMBOLS["mocr_op_gemm_argmax_lse"][1], _capi.SYMBOLS["mocr_op_gemm_topk"][1]
    assert b == a[:-4] + [P, P] + a[-4:] and a[-4:] == [C.c_int32] * 4
    m = re.search(r"#define\s+MOCR_ALTERNATIVES\s+(\d+)\b", hdr)
    assert m and int(m.group(1)) == 4 == _capi.ALTERNATIVES


def test_abi_version_and_token_args_are_unchanged(lib):
    assert lib.mocr_abi_version() == 2
    assert C.sizeof(_capi.MocrTokenArgs) == 160 and len(_capi.MocrTokenArgs._fields_) == 25
    hdr = open(os.path.join(ROOT, "include", "mocr.h")).read()
    body = hdr[hdr.index("typedef struct mocr_token_args {"):hdr.index("} mocr_token_args;")]
    assert "top_" not in body and "alt_" not in body
    # null handles are refused before anything is dereferenced: the new entry points are real functions
    assert lib.mocr_recognize_images_alts(None, None, 1, None, None, None, None, None) == -1
    assert lib.mocr_recognize_regions_alts(None, None, 1, None, 1, None, None, None, None, None) == -1
    assert lib.mocr_recognize_device_alts(None, None, 1, None, None, None, None, None) == -1
    assert lib.mocr_recognize_gray_host_alts(None, None, 1, 8, None, None, None, None, None) == -1
    assert lib.mocr_op_gemm_topk(None, None, None, None, None, None, None, None, None, 1, 64, 64, 64) == -1
    assert lib.mocr_op_dec_token_topk(None, None, None, None, None, None, None, None) == -1


def test_recognition_defaults_and_candidates():
    v = text.Vocab.synthetic(6144)
    ids = np.array([2, 5, 6, 3, 0, 0], np.int32)
    logp = np.array([0.0, np.log(0.5), np.log(0.25), np.log(0.5), 0.0, 0.0], np.float32)
    # the constructions that existed keep working and carry no alternatives
    old = Recognition("x", ids[:4], logp[1:4], 0.5, 0.25)
    assert old.alt_ids is None and old.alt_logprobs is None
    r = Recognition.from_row(v, ids, logp, 4)
    assert r.alt_ids is None and r.alt_logprobs is None and r.text == "一丁"
    with pytest.raises(ValueError, match="no alternatives"):
        r.candidates(0)
    # with the two blocks: rows 1 .. len - 1, row k belongs to ids[k + 1]
    alt_ids = np.full((6, 4), -1, np.int32)
    alt_logp = np.zeros((6, 4), np.float32)
    alt_ids[1:4] = [[5, 9, 7, 8], [6, 5, 11, 10], [3, 6, 5, 12]]
    alt_logp[1:4] = np.log([[0.5, 0.25, 0.125, 0.0625], [0.25, 0.25, 0.125, 0.0625], [0.5, 0.2, 0.1, 0.05]])
    a = Recognition.from_row(v, ids, logp, 4, alt_ids, alt_logp)
    assert a.text == r.text and a.confidence == r.confidence and a.min_prob == r.min_prob
    np.testing.assert_array_equal(a.logprobs, r.logprobs)
    assert a.alt_ids.dtype == np.int32 and a.alt_ids.shape == (3, 4) and a.alt_logprobs.dtype == np.float32 and a.alt_logprobs.shape == (3, 4)
    np.testing.assert_array_equal(a.alt_ids[:, 0], a.ids[1:])
    np.testing.assert_array_equal(a.alt_logprobs[:, 0], a.logprobs)
    c = a.candidates(0)
    assert [t for t, _ in c] == [v.tokens[5], v.tokens[9], v.tokens[7], v.tokens[8]] and c[0][0] == "一"
    assert [p for _, p in c] == pytest.approx([0.5, 0.25, 0.125, 0.0625], rel=1e-6)
    assert a.candidates(2)[0] == (v.tokens[3], pytest.approx(0.5, rel=1e-6))          # the EOS position names the EOS token
    assert a.candidates(-1) == a.candidates(2)
    with pytest.raises(IndexError):
        a.candidates(3)
    # a sliver region (length 0) and a lone start token: empty blocks of the right shape
    for n in (0, 1):
        e = Recognition.from_row(v, np.zeros(6, np.int32), np.zeros(6, np.float32), n, alt_ids, alt_logp)
        assert e.alt_ids.shape == (0, 4) and e.alt_logprobs.shape == (0, 4) and e.confidence == 0.0
    with pytest.raises(Exception):
        a.alt_ids = None                                                             # frozen


def test_alternatives_calls_refuse_several_devices_without_spawning_workers():
    """(this package has no CPU path to refuse on: MangaOcr(force_cpu=True) raises at construction)"""
    from manga_ocr.multi import MultiGpuEngine
    eng = object.__new__(MultiGpuEngine)          # no __init__: no child process, no GPU
    with pytest.raises(NotImplementedError, match="several devices"):
        eng.recognize_images([np.zeros((8, 8), np.uint8)], alternatives=True)
    with pytest.raises(NotImplementedError, match="several devices"):
        eng.recognize_regions([np.zeros((8, 8, 3), np.uint8)], [(0, 0, 0, 4, 4)], alternatives=True)
    ocr = object.__new__(MangaOcr)
    ocr.engine = eng
    ocr.vocab = text.Vocab.synthetic(6144)
    from PIL import Image
    for call in (lambda: ocr.recognize_alternatives(Image.new("L", (8, 8))),
                 lambda: ocr.recognize_batch_alternatives([Image.new("L", (8, 8))]),
                 lambda: ocr.recognize_bgr_alternatives([np.zeros((8, 8, 3), np.uint8)]),
                 lambda: ocr.recognize_regions_alternatives([np.zeros((8, 8, 3), np.uint8)], [(0, 0, 0, 4, 4)])):
        with pytest.raises(NotImplementedError, match="token alternatives.*several devices"):
            call()
    with pytest.raises(RuntimeError, match="no CPU path"):
        MangaOcr(force_cpu=True)


class _FakeEngine:
    """recognize_images as Engine answers it: every crop 'decodes' to [2, its first pixel, 3]; logs the kind of each call"""
    L = 6

    def __init__(self):
        self.calls = []

    def recognize_images(self, images, bgr=False, rotate=None, *, scores=False, alternatives=False):
        self.calls.append((len(images), 2 if alternatives else 1 if scores else 0))
        n = len(images)
        ids = np.zeros((n, self.L), np.int32)
        ids[:, 0], ids[:, 1], ids[:, 2] = 2, [int(g[0, 0]) for g in images], 3
        lens = np.full(n, 3, np.int32)
        if not (scores or alternatives):
            return ids, lens
        logp = np.zeros((n, self.L), np.float32)
        logp[:, 1:3] = -0.5
        if not alternatives:
            return ids, lens, logp
        alt_ids = np.full((n, self.L, 4), -1, np.int32)
        alt_logp = np.zeros((n, self.L, 4), np.float32)
        alt_ids[:, 1:3] = ids[:, 1:3, None] + np.arange(4)
        alt_logp[:, 1:3] = -0.5 - np.arange(4)
        return ids, lens, logp, alt_ids, alt_logp


def test_batcher_makes_the_richest_call_and_hands_each_caller_its_kind():
    eng = _FakeEngine()
    b = _Batcher(eng, max_batch=6, timeout_ms=60_000.0)          # the batch leaves when it is full, not by the clock
    try:
        kinds = [0, 1, 2, 0, 2, 1]
        futs = [b.submit(np.full((4, 4), 10 + i, np.uint8), scored=k == 1, alternatives=k == 2) for i, k in enumerate(kinds)]
        res = [f.result(timeout=30) for f in futs]
        assert eng.calls == [(6, 2)], "one engine call, in the richest mode asked"
        for i, (k, r) in enumerate(zip(kinds, res)):
            if k == 0:
                assert isinstance(r, np.ndarray)
                np.testing.assert_array_equal(r, [2, 10 + i, 3])
                continue
            assert isinstance(r, tuple) and len(r) == (2 if k == 1 else 4)
            np.testing.assert_array_equal(r[0], [2, 10 + i, 3])
            np.testing.assert_array_equal(r[1], np.float32([0, -0.5, -0.5]))
            if k == 2:
                assert r[2].shape == (3, 4) and r[3].shape == (3, 4)
                np.testing.assert_array_equal(r[2][1], 10 + i + np.arange(4))
                np.testing.assert_array_equal(r[3][2], np.float32(-0.5 - np.arange(4)))
                rec = Recognition.from_row(text.Vocab.synthetic(6144), r[0], r[1], len(r[0]), r[2], r[3])
                assert rec.alt_ids.shape == (2, 4) and rec.alt_ids[0, 0] == 10 + i
        # a batch nobody asked alternatives of does not pay for them
        for want, flags in (((6, 1), dict(scored=True)), ((6, 0), {})):
            futs = [b.submit(np.full((4, 4), 7, np.uint8), **(flags if i == 3 else {})) for i in range(6)]
            [f.result(timeout=30) for f in futs]
            assert eng.calls[-1] == want
    finally:
        b.close()


def test_row_top_four_is_the_top_four_of_the_tiles_top_fours():
    """value descending, the lower column first among equal values - on a row with many ties, for both tile widths"""
    rs = np.random.RandomState(3)
    x = rs.randint(-6, 7, size=(16, 6144)).astype(np.float64)
    x[1] = 2.0
    x[2, [100, 101, 102, 103, 6000]] = 50
    top = lambda a: np.argsort(-a, axis=-1, kind="stable")[..., :4]
    want = top(x)
    for tile in (64, 128):
        t3 = x.reshape(16, -1, tile)
        ti = top(t3) + (np.arange(6144 // tile) * tile)[None, :, None]
        tv = np.take_along_axis(x, ti.reshape(16, -1), -1)                      # the union, tile by tile: columns ascend within equal values
        cols = ti.reshape(16, -1)
        order = np.lexsort((cols, -tv), axis=-1)[:, :4]
        np.testing.assert_array_equal(np.take_along_axis(cols, order, -1), want)
    np.testing.assert_array_equal(want[1], [0, 1, 2, 3])
    np.testing.assert_array_equal(want[2], [100, 101, 102, 103])
