"""GPU: the 24 exported mocr_recognize_* symbols, called through the library directly.  Engine (manga_ocr/engine.py) reaches
the *_positions symbol of every source kind only, so this is what keeps the other twenty honest: each is its kind's richest
call with nulls for what it does not take (include/mocr.h), bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import position_util as pu
from gpu_util import crops
from manga_ocr import _capi
from manga_ocr.weights import DEFAULT_SPEC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")      # before the engine's library: one HIP runtime per process, torch's

N, T, L = 3, 8, DEFAULT_SPEC.max_len
KINDS = ["device", "gray_host", "images", "regions"]
# rung -> how many of the optional arguments (logp, alt_ids, alt_logp, sets, ngram, pos) its symbols take
RUNGS = {"": 0, "_scored": 1, "_alts": 3, "_constrained": 4, "_norepeat": 5, "_positions": 6}
ERR_ARG = -1
# 96 x 128 page, three regions, the middle one a sliver (empty: nothing to pad)
REGIONS = [(0, 10, 12, 60, 40), (0, 50, 40, 0, 0), (0, 40, 50, 70, 30)]


@functools.lru_cache(maxsize=None)
def _engine():
    from manga_ocr.engine import Engine
    eng = Engine(pu.pos_weights(), DEFAULT_SPEC, dtype="fp32", device=0, max_batch=8, lanes=1)
    eng.set_generate_max_length(T)
    return eng


@functools.lru_cache(maxsize=None)
def _inputs():
    gray = crops(pu.CROP_SEED, N)
    page = np.ascontiguousarray(np.random.RandomState(pu.CROP_SEED + 7).randint(0, 256, size=(96, 128, 3), dtype=np.uint8))
    return gray, page


@functools.lru_cache(maxsize=None)
def _per_crop():
    """(sets, ngram) that engage the masked LM head and the n-gram token kernel on rows 0 and 2 without moving an id: a set of
    the whole vocabulary but one token no row emits (greedy never chose it), and n = T, which a row of T tokens cannot repeat"""
    emitted = set(np.concatenate([_plain(kind)[0].ravel() for kind in KINDS]).tolist())
    unused = next(t for t in range(DEFAULT_SPEC.vocab - 1, -1, -1) if t not in emitted)
    h = _engine().token_set([t for t in range(DEFAULT_SPEC.vocab) if t != unused])
    assert h != _capi.TOKEN_SET_ALL
    return np.array([h, 0, h], np.int32), np.array([T, 0, T], np.int32)


def _call(kind, rung, nargs=None, sets=None, half_pair=False):
    """Call mocr_recognize_<kind><rung> with fresh output blocks: the first `nargs` optional arguments given (default: all
    the rung takes), the rest of what the symbol takes null.  Returns (rc, [ids, lens, logp, alt_ids, alt_logp, pos] as
    host arrays, None where not given)."""
    eng = _engine()
    gray, page = _inputs()
    takes = RUNGS[rung]
    nargs = takes if nargs is None else nargs
    dev = kind == "device"

    def block(shape, dtype, fill=0):
        return torch.full(shape, fill, dtype=getattr(torch, dtype), device="cuda") if dev else np.full(shape, fill, dtype=dtype)

    outs = [block((N, L), "int32", -7), block((N,), "int32", -7), block((N, L), "float32"), block((N, L, 4), "int32", -1),
            block((N, L, 4), "float32"), block((N, L, 5), "float32")]
    p_sets, p_ngram = _per_crop() if nargs >= 4 else (None, None)
    opt = [outs[2], outs[3], outs[4], p_sets if sets is None else sets, p_ngram, outs[5]]
    opt = [a if i < nargs else None for i, a in enumerate(opt)]
    if half_pair:
        opt[2] = None
    from manga_ocr.engine import _ptr
    tail = [_ptr(outs[0]), _ptr(outs[1])] + [_ptr(a) for a in opt[:takes]]
    fn = getattr(eng.lib, f"mocr_recognize_{kind}{rung}")
    if kind == "device":
        d_gray = torch.from_numpy(gray).cuda()
        rc = fn(eng._h, _ptr(d_gray), N, *tail)
        eng.synchronize()
    elif kind == "gray_host":
        rc = fn(eng._h, _ptr(gray), N, T, *tail)
    elif kind == "images":
        descs, keep = eng._image_descs(list(gray))
        rc = fn(eng._h, descs, N, *tail)
    else:
        descs, keep = eng._image_descs([page], True)
        arr = (_capi.MocrRegion * N)()
        for i, (pg, x, y, w, h) in enumerate(REGIONS):
            arr[i].page, arr[i].x, arr[i].y, arr[i].width, arr[i].height = pg, x, y, w, h
        rc = fn(eng._h, descs, 1, arr, N, *tail)
    given = [True, True] + [opt[0] is not None, opt[1] is not None, opt[2] is not None, opt[5] is not None]
    return rc, [(o.cpu().numpy() if dev else o) if g else None for o, g in zip(outs, given)]


@functools.lru_cache(maxsize=None)
def _plain(kind):
    rc, out = _call(kind, "")
    assert rc == _capi.MOCR_OK
    return out


@pytest.mark.parametrize("rung", list(RUNGS))
@pytest.mark.parametrize("kind", KINDS)
def test_a_twin_is_the_richest_call_with_nulls(kind, rung):
    rc, got = _call(kind, rung)
    rc2, want = _call(kind, "_positions", nargs=RUNGS[rung])
    assert rc == _capi.MOCR_OK and rc2 == _capi.MOCR_OK
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert g.tobytes() == w.tobytes()
    assert sum(g is not None for g in got) == 2 + min(RUNGS[rung], 3) + (RUNGS[rung] == 6)
    # ... and the ids and lengths are those of every other rung of the kind
    ids, lens = _plain(kind)[:2]
    assert got[0].tobytes() == ids.tobytes() and got[1].tobytes() == lens.tobytes()
    assert (lens[[0, 2]] >= 2).all() and (ids != -7).all()
    if kind == "regions":
        assert lens[1] == 0 and (ids[1] == DEFAULT_SPEC.pad_id).all(), "the sliver"
        for blk, fill in zip(got[2:], (0, -1, 0, 0)):
            assert blk is None or (blk[1] == fill).all()
    if RUNGS[rung] >= 1:
        assert (got[2][[0, 2], 1:2] < 0).all(), "scores were written"
    if RUNGS[rung] == 6:
        assert (got[5][[0, 2], 1, 4] > 0).all(), "positions were written"


@pytest.mark.parametrize("kind", KINDS)
def test_the_twins_keep_the_argument_checks(kind):
    rc, _ = _call(kind, "_constrained", sets=np.array([0, 999, 0], np.int32))
    assert rc == ERR_ARG, "an unknown token set handle"
    rc, _ = _call(kind, "_alts", half_pair=True)
    assert rc == ERR_ARG, "half an alternatives pair"
    eng = _engine()
    assert b"both null or both set" in eng.lib.mocr_last_error(eng._h)
