"""CPU: the host side of shared encodings (include/mocr.h, "shared encodings") - the library's new exports, the header and
the ctypes mirror; ``sources=`` of the ``Engine`` methods on a fake library (kinds, per-row sizes, the symbol and the arguments
of every call); the branch selection of ``MangaOcr.recognize_batch_nbest`` and ``score_candidates`` on a fake engine that
answers hand-written alternatives; the multi-device refusal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
from manga_ocr import _capi, text
from manga_ocr.engine import Engine
from manga_ocr.ocr import MangaOcr
from manga_ocr.weights import DEFAULT_SPEC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED = ["mocr_recognize_images_shared", "mocr_recognize_regions_shared", "mocr_recognize_device_shared", "mocr_recognize_gray_host_shared"]
NEW = SHARED + ["mocr_op_enc_expand", "mocr_encoded_crops"]
P, I = C.c_void_p, C.c_int32
L = DEFAULT_SPEC.max_len
START, EOS = 2, 3


# ------------------------------------------------------------------------------------------------ 1. exports
def test_shared_symbols_are_exported_declared_and_mirrored():
    entry.build()
    lib = _capi.load_library()
    hdr = open(os.path.join(ROOT, "include", "mocr.h")).read()
    for name in NEW:
        assert name in _capi.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in mocr.h"
        assert getattr(lib, name) is not None
    # the *_shared calls are the *_prefix twins plus n_rows and source, behind the count of images / regions / planes
    for kind, at in (("images", 3), ("regions", 5), ("device", 3), ("gray_host", 3)):
        pre = _capi.SYMBOLS[f"mocr_recognize_{kind}_prefix"][1]
        assert _capi.SYMBOLS[f"mocr_recognize_{kind}_shared"][1] == pre[:at] + [I, P] + pre[at:], kind
    assert _capi.SYMBOLS["mocr_encoded_crops"] == (C.c_int64, [P]) and _capi.SYMBOLS["mocr_op_enc_expand"][1] == [P, P, P, I, I]
    assert hdr.index("---- forced prefixes") < hdr.index("---- shared encodings") < hdr.index("mocr_recognize_images_shared")
    assert lib.mocr_abi_version() == 2
    # null handles are refused before anything is dereferenced
    assert lib.mocr_recognize_images_shared(None, None, 1, 1, *[None] * 11, 0) == -1
    assert lib.mocr_recognize_regions_shared(None, None, 1, None, 1, 1, *[None] * 11, 0) == -1
    assert lib.mocr_recognize_device_shared(None, None, 1, 1, *[None] * 11, 0) == -1
    assert lib.mocr_recognize_gray_host_shared(None, None, 1, 1, None, 8, *[None] * 10, 0) == -1
    assert lib.mocr_op_enc_expand(None, None, None, 1, 1) == -1 and lib.mocr_encoded_crops(None) == 0


# ------------------------------------------------------------------------------------------------ 2. Engine argument checks
class _FakeLib:
    """every symbol answers MOCR_OK and logs (name, arguments); `peek` = {argument index: count}: the int32 arrays read
    through those pointers DURING the next call (the caller's arrays need not outlive it) land in `seen`"""

    def __init__(self):
        self.calls, self.peek, self.seen = [], {}, {}

    def __getattr__(self, name):
        if not name.startswith("mocr_"):
            raise AttributeError(name)

        def call(*args):
            self.seen = {i: _ints(args[i], n) for i, n in self.peek.items()}
            self.peek = {}
            self.calls.append((name, args))
            return _capi.MOCR_OK
        return call


@pytest.fixture
def eng():
    e = object.__new__(Engine)          # no __init__: no library, no GPU
    e.lib, e.spec, e._h = _FakeLib(), DEFAULT_SPEC, C.c_void_p(0)
    return e


def _ints(p, n):
    return np.ctypeslib.as_array((C.c_int32 * n).from_address(p.value)).tolist()


def _null(p):
    return isinstance(p, C.c_void_p) and not p.value


def test_sources_kinds_and_values():
    assert Engine._sources([2, 0, 2, 1], 3).tolist() == [2, 0, 2, 1] and Engine._sources(np.array([0, 0]), 1).dtype == np.int32
    assert Engine._sources(range(3), 3).tolist() == [0, 1, 2] and Engine._sources((np.int64(0),), 1).tolist() == [0]
    for bad in (3, "012", b"01", True, [0.0, 1.0], [[0, 1]], [], [None, 0], np.int32(1)):
        with pytest.raises(TypeError):
            Engine._sources(bad, 2)
    for bad, why in (([0, 2], "in \\[0, 2\\)"), ([-1, 0, 1], "in \\[0, 2\\)"), ([0, 0], "must be named"), ([1], "must be named")):
        with pytest.raises(ValueError, match=why):
            Engine._sources(bad, 2)


def test_gray_with_sources_calls_the_shared_symbol_with_row_sized_blocks(eng):
    gray = np.zeros((3, 224, 224), np.uint8)
    src = [2, 0, 2, 1, 1]
    eng.lib.peek = {4: 5, 11: 5, 12: 5, 14: 10, 15: 5}
    out = eng.recognize_gray(gray, 24, alternatives=True, positions=True, sources=src, token_sets=[0, 1, 0, 1, 0], no_repeat_ngram=2,
                             prefixes=[[5, 6], None, [7], None, None])
    assert [o.shape for o in out] == [(5, L), (5,), (5, L), (5, L, 4), (5, L, 4), (5, L, 5)], "the output blocks have len(sources) rows"
    (name, a), = eng.lib.calls
    assert name == "mocr_recognize_gray_host_shared" and len(a) == len(_capi.SYMBOLS[name][1])
    seen = eng.lib.seen
    assert (a[2], a[3], a[5]) == (3, 5, 24) and seen[4] == src
    assert seen[11] == [0, 1, 0, 1, 0] and seen[12] == [2] * 5
    assert a[16] == 2 and seen[14] == [5, 6, 0, 0, 7, 0, 0, 0, 0, 0] and seen[15] == [2, 0, 1, 0, 0]
    # the per-row arrays are checked against len(sources), not against the planes
    for kw, why in ((dict(token_sets=[0, 1, 0]), "5 crops but 3 set handles"), (dict(no_repeat_ngram=[1, 2, 3]), "5 crops but 3 sizes"),
                    (dict(prefixes=[None] * 3), "5 crops but 3 prefixes")):
        with pytest.raises(ValueError, match=why):
            eng.recognize_gray(gray, 24, sources=src, **kw)
    with pytest.raises(TypeError):
        eng.recognize_gray(gray, 24, sources=1)
    with pytest.raises(ValueError, match="must be named"):
        eng.recognize_gray(gray, 24, sources=[0, 1, 1])
    assert len(eng.lib.calls) == 1, "a refused call reached the library"
    # without prefixes the shared call passes them null
    eng.recognize_gray(gray, 24, sources=src)
    a = eng.lib.calls[-1][1]
    assert _null(a[14]) and _null(a[15]) and a[16] == 0 and _null(a[8]) and _null(a[11])


def test_images_regions_and_device_with_sources(eng):
    imgs = [np.zeros((20, 30), np.uint8), np.zeros((40, 10, 3), np.uint8)]
    eng.lib.peek = {4: 3}
    ids, lens, logp = eng.recognize_images(imgs, scores=True, sources=[1, 0, 1])
    assert ids.shape == (3, L) and logp.shape == (3, L)
    name, a = eng.lib.calls[-1]
    assert name == "mocr_recognize_images_shared" and len(a) == len(_capi.SYMBOLS[name][1]) and (a[2], a[3]) == (2, 3) and eng.lib.seen[4] == [1, 0, 1]
    page = np.zeros((100, 100, 3), np.uint8)
    eng.lib.peek = {6: 5, 12: 5}
    ids, lens = eng.recognize_regions([page], [(0, 1, 1, 20, 20), (0, 30, 30, 20, 20)], sources=[0, 0, 1, 1, 1], token_sets=[0, 1, 0, 1, 0])
    assert ids.shape == (5, L) and lens.shape == (5,)
    name, a = eng.lib.calls[-1]
    assert name == "mocr_recognize_regions_shared" and len(a) == len(_capi.SYMBOLS[name][1])
    assert (a[2], a[4], a[5]) == (1, 2, 5) and eng.lib.seen[6] == [0, 0, 1, 1, 1] and eng.lib.seen[12] == [0, 1, 0, 1, 0]
    with pytest.raises(ValueError, match="5 crops but 2 set handles"):
        eng.recognize_regions([page], [(0, 1, 1, 20, 20), (0, 30, 30, 20, 20)], sources=[0, 0, 1, 1, 1], token_sets=[0, 1])
    eng.lib.peek = {4: 4, 14: 4}
    eng.recognize_device(1000, 2, 2000, 3000, sources=[0, 1, 1, 0], prefixes=[[9]] * 4)
    name, a = eng.lib.calls[-1]
    assert name == "mocr_recognize_device_shared" and len(a) == len(_capi.SYMBOLS[name][1])
    assert (a[1].value, a[2], a[3], a[5].value, a[6].value) == (1000, 2, 4, 2000, 3000) and eng.lib.seen[4] == [0, 1, 1, 0] and eng.lib.seen[14] == [1] * 4
    with pytest.raises(ValueError, match="4 crops but 2"):
        eng.recognize_device(1000, 2, 2000, 3000, sources=[0, 1, 1, 0], no_repeat_ngram=[1, 1])
    eng.op_enc_expand(10, 20, 3, 7)
    assert eng.lib.calls[-1][0] == "mocr_op_enc_expand" and eng.lib.calls[-1][1][3:] == (3, 7)
    assert eng.encoded_crops() == 0 and eng.lib.calls[-1][0] == "mocr_encoded_crops"


def test_without_sources_the_old_symbols_get_the_old_arguments(eng):
    gray = np.zeros((3, 224, 224), np.uint8)
    imgs = [np.zeros((20, 30), np.uint8)] * 2
    page = np.zeros((100, 100, 3), np.uint8)
    eng.recognize_gray(gray, 24, scores=True)
    eng.recognize_gray(gray, 24, prefixes=[[5], None, None])
    eng.recognize_images(imgs)
    eng.recognize_images(imgs, prefixes=[None, [5]])
    eng.recognize_regions([page], [(0, 1, 1, 20, 20)])
    eng.recognize_regions([page], [(0, 1, 1, 20, 20)], prefixes=[[5]])
    eng.recognize_device(1000, 2, 2000, 3000)
    eng.recognize_device(1000, 2, 2000, 3000, prefixes=[None, [4]])
    names = [n for n, _ in eng.lib.calls]
    assert names == ["mocr_recognize_gray_host_positions", "mocr_recognize_gray_host_prefix", "mocr_recognize_images_positions",
                     "mocr_recognize_images_prefix", "mocr_recognize_regions_positions", "mocr_recognize_regions_prefix",
                     "mocr_recognize_device_positions", "mocr_recognize_device_prefix"]
    for name, a in eng.lib.calls:
        assert len(a) == len(_capi.SYMBOLS[name][1]), name
    assert eng.lib.calls[0][1][2:4] == (3, 24) and eng.lib.calls[2][1][2] == 2 and eng.lib.calls[6][1][2] == 2


# ------------------------------------------------------------------------------------------------ 3. n-best selection
def _vocab():
    toks = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [chr(ord("a") + i) for i in range(26)] + [f"t{i}" for i in range(69)]
    return text.Vocab(toks) if not hasattr(text.Vocab, "from_tokens") else text.Vocab.from_tokens(toks)


NINF = float("-inf")
# Hand-written alternatives of two crops (first pixel 0 / 1): per generated position the four candidates and their
# log-probabilities; entry 0 is the greedy token.
ALTS = {
    0: dict(ids=[START, 10, 11, 12, EOS],
            alt_ids=[[10, 20, 21, -1], [11, 22, 23, 24], [12, 25, 26, 27], [EOS, 28, 29, 30]],
            alt_lp=[[-0.5, -1.5, -2.5, -0.6],        # losses 1.0 (t0 j1), 2.0 (t0 j2); j3 has no token (id -1): skipped
                    [-0.25, -1.25, NINF, -3.25],     # losses 1.0 (t1 j1: ties with t0 j1, the lower t first), 3.0 (t1 j3); j2 -inf: skipped
                    [-1.0, -1.5, -1.5, -9.0],        # losses 0.5 (t2 j1), 0.5 (t2 j2: the lower j first), 8.0
                    [-0.1, -0.11, -0.12, -0.13]]),   # the last position: never a branch point, however cheap
    1: dict(ids=[START, 40, 41, EOS],
            alt_ids=[[40, 50, 51, 52], [41, 53, 54, 55], [EOS, 56, 57, 58]],
            alt_lp=[[-0.2, -4.2, -5.2, -6.2], [-0.3, -0.4, -7.0, -8.0], [-0.1, -0.2, -0.3, -0.4]]),
}
# what a continuation 'decodes' to, by its prefix: (tokens behind the prefix, total log-probability of the row)
CONT = {(10, 11, 25): ([60, EOS], -3.0), (10, 11, 26): ([EOS], -1.0), (20,): ([11, 12, EOS], -9.0),
        (10, 22): ([12, EOS], -0.1 - 0.25 - 1.0 - 0.5),       # rejoins ... a different row from the greedy one
        (40, 53): ([EOS], -0.7), (50,): ([41, EOS], -4.6)}


class _NbestEngine:
    """recognize_images as Engine answers it, from the tables above; logs every call"""
    W = 8

    def __init__(self):
        self.calls = []

    def recognize_images(self, images, bgr=False, rotate=None, *, scores=False, alternatives=False, **kw):
        assert set(kw) <= {"token_sets", "no_repeat_ngram", "prefixes", "sources"}
        self.calls.append(dict(n=len(images), scores=scores, alternatives=alternatives, first=[int(im.flat[0]) for im in images], **kw))
        src = kw.get("sources") or list(range(len(images)))
        n = len(src)
        ids, lens, logp = np.zeros((n, self.W), np.int32), np.zeros(n, np.int32), np.zeros((n, self.W), np.float32)
        alt_ids, alt_lp = np.full((n, self.W, 4), -1, np.int32), np.zeros((n, self.W, 4), np.float32)
        for r in range(n):
            crop = int(images[src[r]].flat[0])
            if alternatives:
                a = ALTS[crop]
                row = a["ids"]
                alt_ids[r, 1:len(row)] = a["alt_ids"]
                alt_lp[r, 1:len(row)] = a["alt_lp"]
                logp[r, 1:len(row)] = [x[0] for x in a["alt_lp"]]
            else:
                pre = tuple(kw["prefixes"][r])
                tail, total = CONT[pre]
                row = [START] + list(pre) + tail
                logp[r, 1] = total
                assert ALTS[crop]["ids"][1:len(pre)] == list(pre[:-1]), "the prefix is not a branch of ITS crop's row"
            ids[r, :len(row)] = row
            lens[r] = len(row)
        return (ids, lens, logp, alt_ids, alt_lp) if alternatives else (ids, lens, logp)


def _ocr(engine):
    ocr = object.__new__(MangaOcr)
    ocr.engine, ocr.no_repeat_ngram_size, ocr.vocab, ocr.spec = engine, None, _vocab(), DEFAULT_SPEC
    return ocr


def _img(v):
    from PIL import Image
    return Image.fromarray(np.full((4, 4), v, np.uint8))


def test_nbest_selection_sources_duplicates_and_order():
    eng = _NbestEngine()
    ocr = _ocr(eng)
    # crop 0: the three smallest losses are 0.5 (t2 j1), 0.5 (t2 j2), 1.0 (t0 j1 before t1 j1: the lower t); the -1 and -inf
    # entries and every candidate of the last position are never taken.  crop 1: 0.1 (t1 j1), 4.0 (t0 j1), 5.0 (t0 j2) - its
    # last position's 0.1 / 0.2 / 0.3 would all have won.
    want = [[10, 11, 25], [10, 11, 26], [20], [40, 53], [50], [51]]
    CONT[(51,)] = ([41, EOS], -5.6)
    try:
        out = ocr.recognize_batch_nbest([_img(0), _img(1)], k=4, allowed=[7, 9], no_repeat_ngram=[0, 3])
    finally:
        del CONT[(51,)]
    first, second = eng.calls
    assert first["alternatives"] and first["n"] == 2 and "sources" not in first and "prefixes" not in first
    assert first["token_sets"] == [7, 9] and first["no_repeat_ngram"] == [0, 3]
    assert second["prefixes"] == want and second["sources"] == [0, 0, 0, 1, 1, 1] and second["first"] == [0, 1]
    assert second["scores"] and not second["alternatives"], "the continuations are a scored call"
    assert second["token_sets"] == [7, 7, 7, 9, 9, 9] and second["no_repeat_ngram"] == [0, 0, 0, 3, 3, 3], "the crop's set and size, per row"
    recs0 = ocr._recognitions_alt(*_NbestEngine().recognize_images([np.zeros((4, 4), np.uint8)], alternatives=True))[0]
    assert want[:3] == [recs0.branch(2, 1), recs0.branch(2, 2), recs0.branch(0, 1)], "the prefixes are Recognition.branch(t, j)"
    # sorted by logprob, descending: greedy -1.85, then -1.0, -3.0, -9.0
    assert [r.ids.tolist() for r in out[0]] == [[START, 10, 11, 26, EOS], [START, 10, 11, 12, EOS], [START, 10, 11, 25, 60, EOS], [START, 20, 11, 12, EOS]]
    lp = [r.logprob for r in out[0]]
    assert lp == sorted(lp, reverse=True) and abs(lp[1] - (-0.5 - 0.25 - 1.0 - 0.1)) < 1e-6
    assert [r.n_forced for r in out[0]] == [3, 0, 3, 1]
    assert [r.ids.tolist() for r in out[1]] == [[START, 40, 41, EOS], [START, 40, 53, EOS], [START, 50, 41, EOS], [START, 51, 41, EOS]]


def test_nbest_drops_equal_rows_keeps_ties_in_order_and_k1_makes_one_call():
    eng = _NbestEngine()
    ocr = _ocr(eng)
    # k = 3 on crop 0: branches (t2 j1), (t2 j2).  Make the second continuation spell the greedy row again: dropped, the
    # first occurrence (the greedy row) kept; and give the first continuation the greedy row's own logprob: the tie keeps
    # the order of construction, greedy first
    keep = dict(CONT)
    ALTS[0]["alt_lp"][3][0] = -0.125         # the greedy row's logprob: -0.5 - 0.25 - 1.0 - 0.125, exact in float32
    CONT[(10, 11, 25)] = ([EOS], -1.875)
    ALTS[0]["alt_ids"][2][2] = 12            # candidate 2 of position 2 spells the greedy token: its branch IS the greedy row
    try:
        CONT[(10, 11, 12)] = ([EOS], -7.0)
        out = ocr.recognize_nbest(_img(0), 3)
    finally:
        ALTS[0]["alt_ids"][2][2], ALTS[0]["alt_lp"][3][0] = 26, -0.1
        CONT.clear(); CONT.update(keep)
    assert out[0].logprob == out[1].logprob == -1.875
    assert eng.calls[1]["prefixes"] == [[10, 11, 25], [10, 11, 12]] and eng.calls[1]["sources"] == [0, 0]
    assert [r.ids.tolist() for r in out] == [[START, 10, 11, 12, EOS], [START, 10, 11, 25, EOS]], "the equal row is dropped, the tie keeps the greedy row first"
    assert len(eng.calls) == 2
    # k = 1: the greedy row, no second call; a row without a deviation (two tokens) sends nothing either
    eng.calls.clear()
    one = ocr.recognize_nbest(_img(1), 1)
    assert len(eng.calls) == 1 and [r.ids.tolist() for r in one] == [[START, 40, 41, EOS]]
    for bad in (0, -1, 2.5, True, "3"):
        with pytest.raises(ValueError):
            ocr.recognize_nbest(_img(1), bad)
    assert ocr.recognize_batch_nbest([], 3) == []
    # fewer branches than k - 1: everything there is, at most k entries
    eng.calls.clear()
    CONT[(50,)], CONT[(51,)], CONT[(52,)] = [([41, EOS], -5.0 - i) for i in range(3)]
    CONT[(40, 54)], CONT[(40, 55)] = ([EOS], -7.5), ([EOS], -8.5)
    try:
        many = ocr.recognize_nbest(_img(1), 50)
    finally:
        CONT.clear(); CONT.update(keep)
    assert len(eng.calls[1]["prefixes"]) == 6 and len(many) == 7, "3 candidates at each of the 2 positions before the last"


def test_score_candidates_is_one_shared_call():
    class Eng(_NbestEngine):
        def recognize_images(self, images, *a, **kw):
            self.calls.append(dict(n=len(images), **kw))
            n = len(kw["sources"])
            ids, lens, logp = np.zeros((n, 8), np.int32), np.zeros(n, np.int32), np.zeros((n, 8), np.float32)
            for r, p in enumerate(kw["prefixes"]):
                ids[r, :len(p) + 1] = [START] + list(p)
                lens[r] = len(p) + 1
                logp[r, 1:len(p) + 1] = -1.0 - r
            return ids, lens, logp
    eng = Eng()
    ocr = _ocr(eng)
    recs = ocr.score_candidates(_img(0), ["ab", [7, 8, 9], ""])
    (call,) = eng.calls
    assert call["n"] == 1 and call["scores"] and call["sources"] == [0, 0, 0]
    assert call["prefixes"] == [[5, 6, EOS], [7, 8, 9, EOS], [EOS]], "every text is forced through EOS, as score_text does it"
    assert [r.ids.tolist() for r in recs] == [[START, 5, 6, EOS], [START, 7, 8, 9, EOS], [START, EOS]], "results in the order given"
    assert [r.n_forced for r in recs] == [3, 4, 1] and abs(recs[1].logprob - (-8.0)) < 1e-6
    assert ocr.score_candidates(_img(0), []) == [] and len(eng.calls) == 1
    with pytest.raises(ValueError, match="'#'"):
        ocr.score_candidates(_img(0), ["a#"])


def test_shared_features_refuse_several_devices_without_spawning_workers():
    from manga_ocr.multi import MultiGpuEngine
    ocr = _ocr(object.__new__(MultiGpuEngine))          # no __init__: no child process, no GPU
    for call in (lambda: ocr.score_candidates(_img(0), ["a"]), lambda: ocr.recognize_nbest(_img(0), 2),
                 lambda: ocr.recognize_batch_nbest([_img(0)], 1)):
        with pytest.raises(NotImplementedError, match="several devices"):
            call()
