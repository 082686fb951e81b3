"""CPU: the forced-prefix feature's host side - ``Vocab.encode_chars``, the normalisation of ``prefix=`` and its errors,
``Recognition.branch`` / ``n_forced`` / ``logprob``, the routing of ``prefix=`` through the batcher on a fake engine (only a
batch with a prefixed request passes ``prefixes=``), the packing of ``prefixes=`` into one int32 block, the multi-device
refusal, and the library's new exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
from manga_ocr import _capi, text
from manga_ocr.engine import Engine
from manga_ocr.ocr import MangaOcr, Recognition, _Batcher, _prefix_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mocr_recognize_images_prefix", "mocr_recognize_regions_prefix", "mocr_recognize_device_prefix",
       "mocr_recognize_gray_host_prefix", "mocr_op_dec_token_prefix", "mocr_op_gemm_argmax_target"]
P = C.c_void_p


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return _capi.load_library()


def _vocab():
    toks = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "a", "##b", "ab", "c", "##c", "あ", " d "]
    return text.Vocab(toks) if not hasattr(text.Vocab, "from_tokens") else text.Vocab.from_tokens(toks)


def test_encode_chars():
    v = _vocab()
    assert v.encode_chars("abc") == [5, 6, 8], "one token per character: 'ab' is never used, '##b' spells b, the lowest id wins for c"
    assert v.encode_chars("あ d") == [10, 11], "whitespace in the text is skipped, whitespace in a token's text is stripped"
    assert v.encode_chars("") == []
    with pytest.raises(ValueError, match="'z'"):
        v.encode_chars("az")
    with pytest.raises(ValueError, match=r"\["):
        v.encode_chars("[")                                      # special tokens never count, and '[' alone is no token
    ids = v.ids_for_chars("abcあd")
    assert set(v.encode_chars("abcあd")) <= set(ids)


def test_prefix_normalisation_and_errors():
    v = _vocab()
    assert _prefix_rows(None, 3, v) is None
    assert _prefix_rows("ab", 2, v) == [[5, 6], [5, 6]]
    assert _prefix_rows([7, 8], 2, v) == [[7, 8], [7, 8]], "a flat int sequence applies to every crop"
    assert _prefix_rows(np.array([7, 8]), 3, v) == [[7, 8]] * 3
    assert _prefix_rows(["a", None, [9, 3]], 3, v) == [[5], None, [9, 3]]
    assert _prefix_rows([None, (np.int64(4),)], 2, v) == [None, [4]]
    assert _prefix_rows([None, None], 2, v) is None and _prefix_rows("", 2, v) is None and _prefix_rows([[], None], 2, v) is None
    with pytest.raises(ValueError, match="2 crops but 3"):
        _prefix_rows(["a", "b", "c"], 2, v)
    with pytest.raises(ValueError, match="'z'"):
        _prefix_rows(["a", "z"], 2, v)
    for bad in (5, 2.5, True, b"ab", [1.5, 2], [[1.5], None], [True, False], [["a"], None]):
        with pytest.raises(TypeError):
            _prefix_rows(bad, 2, v)


def test_engine_packs_prefixes_into_one_block():
    block, plen, ld = Engine._prefixes([[5, 6, 7], None, (), np.array([9])], 4)
    assert block.dtype == np.int32 and plen.dtype == np.int32 and block.flags["C_CONTIGUOUS"]
    assert ld == 3 and block.tolist() == [[5, 6, 7], [0, 0, 0], [0, 0, 0], [9, 0, 0]] and plen.tolist() == [3, 0, 0, 1]
    block, plen, ld = Engine._prefixes([None, None], 2)
    assert ld == 1 and block.shape == (2, 1) and plen.tolist() == [0, 0]
    with pytest.raises(ValueError, match="3 crops but 2"):
        Engine._prefixes([None, [1]], 3)
    with pytest.raises(TypeError):
        Engine._prefixes([[1.5]], 1)
    with pytest.raises(TypeError):
        Engine._prefixes([[[1, 2]]], 1)


def test_recognition_branch_and_n_forced():
    v = _vocab()
    ids = np.array([2, 5, 6, 8, 3], np.int32)
    lp = np.log(np.array([0.0, 0.5, 0.25, 0.5, 1.0], np.float32), where=np.arange(5) > 0, out=np.zeros(5, np.float32))
    alt_ids = np.full((5, 4), -1, np.int32)
    alt_ids[1:5] = [[5, 7, 8, 9], [6, 9, 5, -1], [8, 10, 5, 6], [3, 5, 6, 7]]
    r = Recognition.from_row(v, ids, lp, 5, alt_ids, np.zeros((5, 4), np.float32))
    assert r.n_forced == 0
    assert r.branch(0, 1) == [7] and r.branch(2, 1) == [5, 6, 10] and r.branch(3, 0) == [5, 6, 8, 3]
    assert r.branch(1, 0) == r.ids[1:3].tolist(), "candidate 0 is the row itself"
    with pytest.raises(ValueError, match="no candidate"):
        r.branch(1, 3)
    with pytest.raises(IndexError):
        r.branch(4, 0)
    with pytest.raises(IndexError):
        r.branch(0, 4)
    with pytest.raises(ValueError, match="no alternatives"):
        Recognition.from_row(v, ids, lp, 5).branch(0, 0)
    assert abs(r.logprob - np.log(0.5 * 0.25 * 0.5)) < 1e-6
    marked = MangaOcr._mark_forced([r, r, r], [[5, 6], None, [5, 6, 8, 3, 9, 9]])
    assert [m.n_forced for m in marked] == [2, 0, 4], "a row that finished inside its prefix counts what it took"
    assert MangaOcr._mark_forced([r], None)[0] is r


class _FakeEngine:
    """recognize_images as Engine answers it; logs the keywords of each call.  A crop 'decodes' to [2, its prefix or its first
    pixel, 3]."""
    L = 8

    def __init__(self):
        self.calls = []

    def recognize_images(self, images, bgr=False, rotate=None, *, scores=False, alternatives=False, **kw):
        assert set(kw) <= {"token_sets", "no_repeat_ngram", "prefixes"}
        self.calls.append((len(images), 1 if scores else 0, dict(kw)))
        n = len(images)
        pre = kw.get("prefixes") or [None] * n
        ids = np.zeros((n, self.L), np.int32)
        lens = np.zeros(n, np.int32)
        for i, im in enumerate(images):
            row = [2] + (list(pre[i]) if pre[i] else [int(im.flat[0])]) + [3]
            ids[i, :len(row)] = row
            lens[i] = len(row)
        if scores:
            return ids, lens, np.zeros((n, self.L), np.float32)
        return ids, lens


def test_prefix_is_routed_through_the_batcher_only_when_asked():
    eng = _FakeEngine()
    b = _Batcher(eng, max_batch=4, timeout_ms=60_000.0)
    try:
        pres = [None, [40, 41], None, (50,)]
        futs = [b.submit(np.full((4, 4), 10 + i, np.uint8), scored=i == 3, prefix=p) for i, p in enumerate(pres)]
        res = [f.result(timeout=30) for f in futs]
        assert eng.calls == [(4, 1, dict(prefixes=[None, [40, 41], None, [50]]))], "one engine call, one prefix per crop in queue order"
        np.testing.assert_array_equal(res[0], [2, 10, 3]); np.testing.assert_array_equal(res[1], [2, 40, 41, 3])
        np.testing.assert_array_equal(res[3][0], [2, 50, 3])
        # nobody asked: the call of before, without the keyword
        futs = [b.submit(np.full((4, 4), 7, np.uint8), prefix=None if i else []) for i in range(4)]
        [f.result(timeout=30) for f in futs]
        assert eng.calls[-1] == (4, 0, {})
    finally:
        b.close()
    ocr = object.__new__(MangaOcr)
    ocr.engine, ocr.no_repeat_ngram_size, ocr.vocab = eng, None, _vocab()
    assert ocr._decode_kw(None, None, 2) == {} and ocr._single(None, None) == {}
    assert ocr._decode_kw(None, None, 2, "ab") == dict(prefixes=[[5, 6], [5, 6]])
    assert ocr._decode_kw(3, 2, 2, [None, [9]]) == dict(token_sets=[3, 3], no_repeat_ngram=[2, 2], prefixes=[None, [9]])
    assert ocr._decode_kw(None, None, 2, [None, None]) == {}, "no crop has a prefix: the call the method always made"
    assert ocr._single(None, None, "c") == dict(prefix=[8]) and ocr._single(None, None, []) == {}
    n0 = len(eng.calls)
    out = ocr.recognize_ids([np.full((4, 4), 9, np.uint8)] * 2, prefix=[[30, 31], None])
    assert [o.tolist() for o in out] == [[2, 30, 31, 3], [2, 9, 3]] and eng.calls[n0][2] == dict(prefixes=[[30, 31], None])
    ocr.recognize_ids([np.full((4, 4), 9, np.uint8)] * 2)
    assert eng.calls[-1][2] == {}
    recs = ocr.recognize_bgr_scored([np.full((4, 4, 3), 9, np.uint8)] * 2, prefix=[[30, 31], None])
    assert [r.n_forced for r in recs] == [2, 0]


def test_prefixes_refuse_several_devices_without_spawning_workers():
    from manga_ocr.multi import MultiGpuEngine
    eng = object.__new__(MultiGpuEngine)          # no __init__: no child process, no GPU
    assert "forced prefixes" in MultiGpuEngine.NO_PREFIX
    with pytest.raises(NotImplementedError, match="forced prefixes.*several devices"):
        eng.recognize_images([np.zeros((8, 8), np.uint8)], prefixes=[[5]])
    with pytest.raises(NotImplementedError, match="forced prefixes.*several devices"):
        eng.recognize_regions([np.zeros((8, 8, 3), np.uint8)], [(0, 0, 0, 4, 4)], prefixes=[None])
    ocr = object.__new__(MangaOcr)
    ocr.engine, ocr.no_repeat_ngram_size, ocr.vocab = eng, None, _vocab()
    for call in (lambda: ocr.recognize_ids([np.zeros((8, 8), np.uint8)], prefix="a"),
                 lambda: ocr.recognize_bgr([np.zeros((8, 8, 3), np.uint8)], prefix=[[5]]),
                 lambda: ocr.recognize_regions([np.zeros((8, 8, 3), np.uint8)], [(0, 0, 0, 4, 4)], prefix=[5])):
        with pytest.raises(NotImplementedError, match="forced prefixes.*several devices"):
            call()


def test_prefix_symbols_are_exported_declared_and_mirrored(lib):
    hdr = open(os.path.join(ROOT, "include", "mocr.h")).read()
    for name in NEW:
        assert name in _capi.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in mocr.h"
        assert getattr(lib, name) is not None
    I = C.c_int32
    for kind in ("images", "regions", "device", "gray_host"):
        pos, pre = f"mocr_recognize_{kind}_positions", f"mocr_recognize_{kind}_prefix"
        assert _capi.SYMBOLS[pre][1] == _capi.SYMBOLS[pos][1] + [P, P, I], pre        # the _positions twin plus the three arguments
    assert _capi.SYMBOLS["mocr_op_dec_token_prefix"][1] == _capi.SYMBOLS["mocr_op_dec_token_ngram"][1] + [P, P, I, P]
    assert _capi.SYMBOLS["mocr_op_gemm_argmax_target"][1] == _capi.SYMBOLS["mocr_op_gemm_argmax_masked"][1] + [P, P, I, P, P]
    assert "forced prefixes" in hdr
    # the ABI did not move; null handles are refused before anything is dereferenced
    assert lib.mocr_abi_version() == 2
    assert C.sizeof(_capi.MocrTokenArgs) == 160 and len(_capi.MocrTokenArgs._fields_) == 25, "mocr_token_args did not grow"
    assert lib.mocr_recognize_images_prefix(None, None, 1, *[None] * 10, 0) == -1
    assert lib.mocr_recognize_regions_prefix(None, None, 1, None, 1, *[None] * 10, 0) == -1
    assert lib.mocr_recognize_device_prefix(None, None, 1, *[None] * 10, 0) == -1
    assert lib.mocr_recognize_gray_host_prefix(None, None, 1, 8, *[None] * 10, 0) == -1
    assert lib.mocr_op_dec_token_prefix(None, *[None] * 15, 0, None) == -1
    assert lib.mocr_op_gemm_argmax_target(None, *[None] * 8, 1, 1, 1, 64, *[None] * 5, 0, None, None) == -1
