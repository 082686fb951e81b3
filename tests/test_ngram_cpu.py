"""CPU: the no-repeat n-gram feature's host side - the reference ban function (ngram_util.banned_tokens, the dictionary
form transformers uses) on hand-written cases, argument validation, the multi-device refusal, the resolution of
``MangaOcr(no_repeat_ngram_size="checkpoint")`` on a synthetic model directory, the routing of ``no_repeat_ngram=`` through
the batcher on a fake engine, and the library's new exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import ngram_util as nu
from manga_ocr import _capi, text
from manga_ocr.engine import Engine
from manga_ocr.ocr import MangaOcr, _Batcher, _ngram_sizes, resolve_no_repeat_ngram
from manga_ocr.weights import DEFAULT_SPEC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mocr_recognize_images_norepeat", "mocr_recognize_regions_norepeat", "mocr_recognize_device_norepeat",
       "mocr_recognize_gray_host_norepeat", "mocr_op_dec_token_ngram", "mocr_op_ngram_init"]
P = C.c_void_p


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return _capi.load_library()


def test_banned_tokens_on_hand_written_cases():
    a, b, c, d, s = 10, 11, 12, 13, 2
    # n = 0: off
    assert nu.banned_tokens([s, a, a, a], 0) == []
    # n = 1: the key is empty - every token of the row, the start token too
    assert nu.banned_tokens([s], 1) == [s]
    assert nu.banned_tokens([s, b, a, b], 1) == [s, a, b]
    # n = 2: the followers of the last token's earlier occurrences
    assert nu.banned_tokens([s], 2) == []                       # L + 1 = n: no complete bigram yet
    assert nu.banned_tokens([s, a], 2) == []
    assert nu.banned_tokens([s, a, b, a], 2) == [b]
    assert nu.banned_tokens([s, a, b, a, c, a], 2) == [b, c], "a key that occurs twice with different followers: both"
    assert nu.banned_tokens([s, a, a], 2) == [a], "the last complete window (i = L - n) counts"
    # n = 3
    assert nu.banned_tokens([s], 3) == [] and nu.banned_tokens([s, a], 3) == [], "L + 1 <= n: nothing"
    assert nu.banned_tokens([s, a, b], 3) == []
    assert nu.banned_tokens([s, a, b, c, a, b], 3) == [c]
    assert nu.banned_tokens([s, a, b, c, a, b, d, a, b], 3) == [c, d]
    assert nu.banned_tokens([s, a, b, c, b, a], 3) == [], "the key is ordered"
    # overlapping repeats
    assert nu.banned_tokens([s, a, a], 3) == []
    assert nu.banned_tokens([s, a, a, a], 3) == [a]
    assert nu.banned_tokens([s, a, a, a, a], 3) == [a] and nu.banned_tokens([s, a, a, a, a], 2) == [a]
    assert nu.banned_tokens([s, a, a, a, a], 5) == [] and nu.banned_tokens([s, a, a, a, a, a], 5) == [a]
    # L + 1 < n
    assert nu.banned_tokens([s, a, a], 5) == [] and nu.banned_tokens([s, a, b, a], 6) == []
    # the effective set: the base set minus the bans; first_repeat: where a free row first completes a repeated n-gram
    base = np.ones(nu.V, bool); base[c] = False
    m = nu.step_mask([s, a, b, a, c, a], 2, base)
    assert not m[b] and not m[c] and m[a] and m.sum() == nu.V - 2
    assert nu.first_repeat([s, a, b, c, a, b, c], 3) == 6 and nu.first_repeat([s, a, b, c, a, b], 3) is None
    assert nu.first_repeat([s, a, a, a], 2) == 3 and nu.first_repeat([s, a, a], 1) == 2
    # a row decoded under the rule holds no repeated n-gram, and step_masks states every step's set
    ids = np.array([[s, a, b, a, c, nu.EOS, 0, 0]])
    sm = nu.step_masks(ids, [6], [2], np.ones((1, nu.V), bool))
    assert sm.shape == (1, 7, nu.V) and sm[0, :3].all() and not sm[0, 3, b] and sm[0, 3].sum() == nu.V - 1
    assert sm[0, 4:].all(), "the key (c) has no earlier occurrence; steps behind the row's end keep the base set"


def test_the_golden_free_runs_repeat_ngrams():
    """what the feature is for: the golden ids of the widened-margin synthetic weights loop (tests/golden/bf16_parity.npz:
    every row completes a repeated 3-gram at position 4), and most rows of the seed-0 weights do"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "bf16_parity.npz"))
    assert [nu.first_repeat(r, 3) for r in g["ids_wide"]] == [4] * 32
    firsts = [nu.first_repeat(r, 3) for r in g["ids_seed0"]]
    assert sum(f is not None for f in firsts) == 252 and min(f for f in firsts if f is not None) == 35


def test_argument_validation():
    eng = object.__new__(Engine)                 # no __init__: no library, no GPU
    eng.spec = DEFAULT_SPEC
    np.testing.assert_array_equal(eng._ngram(3, 4), [3, 3, 3, 3])
    assert eng._ngram(3, 4).dtype == np.int32
    np.testing.assert_array_equal(eng._ngram([0, 1, 2, DEFAULT_SPEC.max_len], 4), [0, 1, 2, DEFAULT_SPEC.max_len])
    np.testing.assert_array_equal(eng._ngram(np.array([2, 0], np.int64), 2), [2, 0])
    with pytest.raises(ValueError, match="3 crops but 2 sizes"):
        eng._ngram([1, 2], 3)
    for bad in (-1, DEFAULT_SPEC.max_len + 1, [0, -2], [1, 10 ** 6]):
        with pytest.raises(ValueError, match="0 .. max_len"):
            eng._ngram(bad, 2)
    for bad in (True, "3", [1.5, 2.0]):
        with pytest.raises(TypeError):
            eng._ngram(bad, 2)
    # the MangaOcr side: a call's value overrides the constructor's
    assert _ngram_sizes(None, None, 3) is None and _ngram_sizes(None, 3, 2) == [3, 3]
    assert _ngram_sizes(0, 3, 2) == [0, 0] and _ngram_sizes([1, 0], 3, 2) == [1, 0]
    with pytest.raises(ValueError, match="2 crops but 1 sizes"):
        _ngram_sizes([1], None, 2)
    with pytest.raises(ValueError):
        _ngram_sizes(-1, None, 2)
    with pytest.raises(TypeError):
        _ngram_sizes("checkpoint", None, 2)


def test_checkpoint_resolution_on_a_synthetic_model_directory(tmp_path):
    """config.json of tests/hf_dir.py carries num_beams=4, no_repeat_ngram_size=3, length_penalty=2.0: "checkpoint" takes the 3
    and leaves the beam settings ignored; the RuntimeWarning of the loader stays."""
    from hf_dir import write_hf_dir
    from manga_ocr.weights import load_checkpoint
    d = str(tmp_path / "manga-ocr-base")
    write_hf_dir(d, seed=3)
    with pytest.warns(RuntimeWarning, match="greedy"):
        spec, _ = load_checkpoint(d)
    ignored = dict(spec.ignored_generation)
    assert ignored["no_repeat_ngram_size"] == 3 and ignored["num_beams"] == 4 and ignored["length_penalty"] == 2.0
    n, left = resolve_no_repeat_ngram("checkpoint", ignored, spec.max_len)
    assert n == 3 and "no_repeat_ngram_size" not in left and left["num_beams"] == 4 and left["length_penalty"] == 2.0
    assert ignored["no_repeat_ngram_size"] == 3, "the caller's dictionary is not touched"
    # None: today's behaviour; an int: that size, the checkpoint's own value stays listed as ignored
    assert resolve_no_repeat_ngram(None, ignored, 300) == (None, ignored)
    assert resolve_no_repeat_ngram(2, ignored, 300) == (2, ignored)
    assert resolve_no_repeat_ngram(0, ignored, 300) == (0, ignored)
    # a greedy checkpoint (synthetic weights): "checkpoint" is 0
    assert resolve_no_repeat_ngram("checkpoint", {}, 300) == (0, {})
    for bad in (-1, 301):
        with pytest.raises(ValueError):
            resolve_no_repeat_ngram(bad, {}, 300)
    with pytest.raises(ValueError):
        resolve_no_repeat_ngram("config", {}, 300)
    for bad in (True, 2.0):
        with pytest.raises(TypeError):
            resolve_no_repeat_ngram(bad, {}, 300)


class _FakeEngine:
    """recognize_images as Engine answers it; logs the keywords of each call.  A crop under size g 'decodes' to
    [2, first pixel + 100 g, 3]."""
    L = 6

    def __init__(self):
        self.calls = []

    def recognize_images(self, images, bgr=False, rotate=None, *, scores=False, alternatives=False, **kw):
        assert set(kw) <= {"token_sets", "no_repeat_ngram"}
        self.calls.append((len(images), 1 if scores else 0, {k: list(v) for k, v in kw.items()}))
        n = len(images)
        g = kw.get("no_repeat_ngram") or [0] * n
        ids = np.zeros((n, self.L), np.int32)
        ids[:, 0], ids[:, 2] = 2, 3
        ids[:, 1] = [int(im[0, 0]) + 100 * g[i] for i, im in enumerate(images)]
        lens = np.full(n, 3, np.int32)
        if scores:
            return ids, lens, np.zeros((n, self.L), np.float32)
        return ids, lens


def test_no_repeat_ngram_is_routed_through_the_batcher():
    eng = _FakeEngine()
    b = _Batcher(eng, max_batch=5, timeout_ms=60_000.0)
    try:
        sizes = [0, 3, 2, 0, 1]
        sets = [0, 0, 4, 0, 0]
        futs = [b.submit(np.full((4, 4), 10 + i, np.uint8), scored=i == 1, token_set=h, no_repeat_ngram=g)
                for i, (g, h) in enumerate(zip(sizes, sets))]
        res = [f.result(timeout=30) for f in futs]
        assert eng.calls == [(5, 1, dict(token_sets=sets, no_repeat_ngram=sizes))], "one engine call, one size per crop in queue order"
        for i, (g, r) in enumerate(zip(sizes, res)):
            np.testing.assert_array_equal(r[0] if i == 1 else r, [2, 10 + i + 100 * g, 3])
        # nobody asked: the call of before, without the keyword
        futs = [b.submit(np.full((4, 4), 7, np.uint8)) for _ in range(5)]
        [f.result(timeout=30) for f in futs]
        assert eng.calls[-1] == (5, 0, {})
    finally:
        b.close()
    # MangaOcr: the constructor's size is every call's default, a call's own value overrides it, 0 switches it off
    ocr = object.__new__(MangaOcr)
    ocr.engine, ocr.no_repeat_ngram_size = eng, 3
    assert ocr._decode_kw(None, None, 2) == dict(no_repeat_ngram=[3, 3])
    assert ocr._decode_kw(None, 0, 2) == {} and ocr._decode_kw(None, [0, 2], 2) == dict(no_repeat_ngram=[0, 2])
    assert ocr._single(None, None) == dict(no_repeat_ngram=3) and ocr._single(None, 0) == {}
    ocr.no_repeat_ngram_size = None
    assert ocr._decode_kw(None, None, 2) == {} and ocr._single(None, None) == {}
    assert ocr._decode_kw(5, 2, 1) == dict(token_sets=[5], no_repeat_ngram=[2])


def test_ngrams_refuse_several_devices_without_spawning_workers():
    from manga_ocr.multi import MultiGpuEngine
    eng = object.__new__(MultiGpuEngine)          # no __init__: no child process, no GPU
    with pytest.raises(NotImplementedError, match="no-repeat n-grams.*several devices"):
        eng.recognize_images([np.zeros((8, 8), np.uint8)], no_repeat_ngram=3)
    with pytest.raises(NotImplementedError, match="no-repeat n-grams.*several devices"):
        eng.recognize_regions([np.zeros((8, 8, 3), np.uint8)], [(0, 0, 0, 4, 4)], no_repeat_ngram=[2])
    ocr = object.__new__(MangaOcr)
    ocr.engine, ocr.no_repeat_ngram_size = eng, None
    ocr.vocab = text.Vocab.synthetic(6144)
    for call in (lambda: ocr.recognize_ids([np.zeros((8, 8), np.uint8)], no_repeat_ngram=3),
                 lambda: ocr.recognize_bgr([np.zeros((8, 8, 3), np.uint8)], no_repeat_ngram=[2]),
                 lambda: ocr.recognize_regions([np.zeros((8, 8, 3), np.uint8)], [(0, 0, 0, 4, 4)], no_repeat_ngram=3)):
        with pytest.raises(NotImplementedError, match="no-repeat n-grams.*several devices"):
            call()
    with pytest.raises(NotImplementedError, match="no-repeat n-grams.*several devices"):
        MangaOcr(synthetic_seed=0, devices=[0, 1], no_repeat_ngram_size=3)      # refused before any worker starts


def test_ngram_symbols_are_exported_declared_and_mirrored(lib):
    hdr = open(os.path.join(ROOT, "include", "mocr.h")).read()
    for name in NEW:
        assert name in _capi.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in mocr.h"
        assert getattr(lib, name) is not None
    for con, nr in [("mocr_recognize_images_constrained", "mocr_recognize_images_norepeat"),
                    ("mocr_recognize_regions_constrained", "mocr_recognize_regions_norepeat"),
                    ("mocr_recognize_device_constrained", "mocr_recognize_device_norepeat"),
                    ("mocr_recognize_gray_host_constrained", "mocr_recognize_gray_host_norepeat")]:
        assert _capi.SYMBOLS[nr][1] == _capi.SYMBOLS[con][1] + [P], nr          # the _constrained twin plus `ngram`
    assert _capi.SYMBOLS["mocr_op_dec_token_ngram"][1] == _capi.SYMBOLS["mocr_op_dec_token_masked"][1] + [P, P, P, P]
    # the ABI did not move; null handles are refused before anything is dereferenced
    assert lib.mocr_abi_version() == 2
    assert C.sizeof(_capi.MocrTokenArgs) == 160 and len(_capi.MocrTokenArgs._fields_) == 25
    assert lib.mocr_recognize_images_norepeat(None, None, 1, None, None, None, None, None, None, None) == -1
    assert lib.mocr_recognize_regions_norepeat(None, None, 1, None, 1, None, None, None, None, None, None, None) == -1
    assert lib.mocr_recognize_device_norepeat(None, None, 1, None, None, None, None, None, None, None) == -1
    assert lib.mocr_recognize_gray_host_norepeat(None, None, 1, 8, None, None, None, None, None, None, None) == -1
    assert lib.mocr_op_dec_token_ngram(None, None, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert lib.mocr_op_ngram_init(None, None, None, None, None, 1) == -1
