"""CPU: Engine's four recognise methods on a fake library that records its calls - whatever is asked for, a method prepares
its blocks once and makes ONE C call, to its source kind's richest symbol, with every output nobody asked for passed as null,
and shapes the return value as its docstring promises."""
import ctypes as C
import itertools

import numpy as np
import pytest

from manga_ocr import _capi
from manga_ocr.engine import Engine
from manga_ocr.weights import DEFAULT_SPEC

N = 3
COMBOS = list(itertools.product([False, True], repeat=5))      # scores, alternatives, token_sets, no_repeat_ngram, positions


class _FakeLib:
    """every symbol answers MOCR_OK and logs (name, arguments)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("mocr_"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or _capi.MOCR_OK


@pytest.fixture
def eng():
    e = object.__new__(Engine)          # no __init__: no library, no GPU
    e.lib, e.spec, e._h = _FakeLib(), DEFAULT_SPEC, C.c_void_p(0)
    return e


def _null(p):
    return isinstance(p, C.c_void_p) and not p.value


def _check_call(eng, symbol, scores, alternatives, sets, ngram, positions):
    """one call, to `symbol`; its last nine arguments are ids, lens and the optional blocks"""
    assert [name for name, _ in eng.lib.calls] == [symbol], eng.lib.calls
    ids, lens, logp, alt_ids, alt_logp, p_sets, p_ngram, pos = eng.lib.calls[0][1][-8:]
    assert not _null(ids) and not _null(lens)
    assert _null(logp) == (not (scores or alternatives))
    assert _null(alt_ids) == _null(alt_logp) == (not alternatives)
    assert _null(p_sets) == (not sets) and _null(p_ngram) == (not ngram) and _null(pos) == (not positions)


def _check_result(out, n, scores, alternatives, positions):
    L = DEFAULT_SPEC.max_len
    want = [(n, L), (n,)] + ([(n, L)] if scores or alternatives else []) + ([(n, L, 4), (n, L, 4)] if alternatives else []) + \
           ([(n, L, 5)] if positions else [])
    assert isinstance(out, tuple) and [a.shape for a in out] == want
    assert out[0].dtype == np.int32 and out[1].dtype == np.int32 and all(a.dtype == np.float32 for a in out[2:3] + out[4:])
    if alternatives:
        assert out[3].dtype == np.int32 and (out[3] == -1).all()


def _kw(scores, alternatives, sets, ngram, positions, n=N):
    kw = dict(scores=scores, alternatives=alternatives, positions=positions)
    if sets:
        kw["token_sets"] = [1, 0, 2][:n] if n else 1
    if ngram:
        kw["no_repeat_ngram"] = 3
    return kw


@pytest.mark.parametrize("scores,alternatives,sets,ngram,positions", COMBOS)
def test_recognize_images_makes_one_call(eng, scores, alternatives, sets, ngram, positions):
    out = eng.recognize_images([np.zeros((8, 9), np.uint8)] * N, **_kw(scores, alternatives, sets, ngram, positions))
    _check_call(eng, "mocr_recognize_images_positions", scores, alternatives, sets, ngram, positions)
    assert eng.lib.calls[0][1][2] == N
    _check_result(out, N, scores, alternatives, positions)
    # no crops: no call at all, token_sets / no_repeat_ngram are not looked at, the same arity
    eng.lib.calls.clear()
    _check_result(eng.recognize_images([], **_kw(scores, alternatives, sets, ngram, positions, n=0)), 0, scores, alternatives, positions)
    assert eng.lib.calls == []


@pytest.mark.parametrize("scores,alternatives,sets,ngram,positions", COMBOS)
def test_recognize_regions_makes_one_call(eng, scores, alternatives, sets, ngram, positions):
    pages = [np.zeros((32, 48, 3), np.uint8)]
    out = eng.recognize_regions(pages, [(0, 1, 2, 8, 8)] * N, **_kw(scores, alternatives, sets, ngram, positions))
    _check_call(eng, "mocr_recognize_regions_positions", scores, alternatives, sets, ngram, positions)
    assert eng.lib.calls[0][1][2] == 1 and eng.lib.calls[0][1][4] == N
    _check_result(out, N, scores, alternatives, positions)
    eng.lib.calls.clear()
    _check_result(eng.recognize_regions(pages, [], **_kw(scores, alternatives, sets, ngram, positions, n=0)), 0, scores, alternatives, positions)
    assert eng.lib.calls == []


@pytest.mark.parametrize("scores,alternatives,sets,ngram,positions", COMBOS)
def test_recognize_gray_makes_one_call(eng, scores, alternatives, sets, ngram, positions):
    out = eng.recognize_gray(np.zeros((N, 224, 224), np.uint8), max_len=8, **_kw(scores, alternatives, sets, ngram, positions))
    _check_call(eng, "mocr_recognize_gray_host_positions", scores, alternatives, sets, ngram, positions)
    assert eng.lib.calls[0][1][2:4] == (N, 8)
    _check_result(out, N, scores, alternatives, positions)


@pytest.mark.parametrize("scores,alternatives,sets,ngram,positions", COMBOS)
def test_recognize_device_makes_one_call(eng, scores, alternatives, sets, ngram, positions):
    kw = _kw(scores, alternatives, sets, ngram, positions)
    out = eng.recognize_device(0x1000, N, 0x2000, 0x3000, 0x4000 if scores or alternatives else None,
                               0x5000 if alternatives else None, 0x6000 if alternatives else None,
                               token_sets=kw.get("token_sets"), no_repeat_ngram=kw.get("no_repeat_ngram"),
                               d_out_pos=0x7000 if positions else None)
    assert out is None
    _check_call(eng, "mocr_recognize_device_positions", scores, alternatives, sets, ngram, positions)
    assert [p.value for p in eng.lib.calls[0][1][3:5]] == [0x2000, 0x3000]


def test_the_argument_errors_come_before_any_call(eng):
    crops = [np.zeros((8, 9), np.uint8)] * N
    with pytest.raises(ValueError, match="token_sets"):
        eng.recognize_images(crops, token_sets=[1, 2])
    with pytest.raises(ValueError, match="no_repeat_ngram"):
        eng.recognize_gray(np.zeros((N, 224, 224), np.uint8), no_repeat_ngram=[1, 2])
    with pytest.raises(TypeError, match="no_repeat_ngram"):
        eng.recognize_regions([np.zeros((32, 48, 3), np.uint8)], [(0, 1, 2, 8, 8)] * N, no_repeat_ngram=True)
    with pytest.raises(ValueError, match="max_len"):
        eng.recognize_device(0x1000, N, 0x2000, 0x3000, no_repeat_ngram=DEFAULT_SPEC.max_len + 1)
    with pytest.raises(ValueError, match="no_repeat_ngram"):       # the sizes are checked before the sets
        eng.recognize_images(crops, token_sets=[1, 2], no_repeat_ngram=-1)
    assert eng.lib.calls == []
    # half an alternatives pair is the engine's to refuse: it is passed on as it came
    eng.recognize_device(0x1000, N, 0x2000, 0x3000, 0x4000, 0x5000, None)
    args = eng.lib.calls[0][1]
    assert args[6].value == 0x5000 and _null(args[7])
