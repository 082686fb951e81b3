#!/usr/bin/env python3
"""Record what the Python recognise surface does with its arguments: tests/golden/surface.json.

A characterisation of ``manga_ocr/engine.py`` and ``manga_ocr/ocr.py`` on fakes - no library, no GPU.  ``record()`` drives

* ``Engine``'s four recognise methods on a fake library that logs, per C call, the symbol and every argument (null or not,
  scalars by value, the descriptor / region / beam structs by field, the per-row int arrays by content), plus the shapes,
  dtypes and fill of what the method returns;
* every public recognise / score method of ``MangaOcr`` on a fake engine that takes any keywords, logs the method, the
  positional arguments (as ``Engine`` names them, one left out by its default) reduced to shapes and scalars and the exact
  keyword dict, and answers with deterministic arrays
  of the arity the keywords ask for; the texts, ids, ``n_forced`` and array shapes that come back are logged too;
* the refusals: a ``MultiGpuEngine`` made with ``object.__new__`` under every method, short ``orientations`` lists,
  arguments that are no image - exception type and message.

surface.json holds one digest per method (``digest``: the scenarios in full are half a megabyte; ``--show GROUP`` prints a
group's, to compare two commits with).  It was written by this script at the commit BEFORE the request path of the two files was folded into one
(``Engine._recognize``, ``MangaOcr._run``); tests/test_surface_cpu.py runs ``record()`` again and asserts equality, so the
file is only ever regenerated when the surface is meant to change:

    python tests/golden/make_surface_golden.py [--show GROUP]

Imports the package, numpy and Pillow (``MangaOcr.recognize`` takes a PIL image or a path, nothing else).
"""
import ctypes as C
import json
import os
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if os.path.join(ROOT, "manga-ocr_amd") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "manga-ocr_amd"))

from manga_ocr import _capi  # noqa: E402
from manga_ocr.engine import BeamConfig, Engine  # noqa: E402
from manga_ocr.ocr import MangaOcr, Recognition, TokenSet, _Batcher  # noqa: E402
from manga_ocr.text import Vocab  # noqa: E402
from manga_ocr.weights import DEFAULT_SPEC  # noqa: E402

PATH = os.path.join(HERE, "surface.json")
START, EOS = int(DEFAULT_SPEC.start_id), int(DEFAULT_SPEC.eos_id)


# ------------------------------------------------------------------------------------------------ rendering
def _plain(v):
    """anything -> JSON: arrays by shape, dtype and content (larger ones: their sum); a Recognition by the fields it has"""
    if isinstance(v, Recognition):
        out = {"text": v.text, "ids": v.ids.tolist(), "logprobs": v.logprobs.tolist(), "confidence": round(v.confidence, 6),
               "min_prob": round(v.min_prob, 6), "n_forced": v.n_forced, "alt_ids": _plain(v.alt_ids), "alt_logprobs": _plain(v.alt_logprobs),
               "positions": _plain(v.positions), "rect": _plain(v.rect), "sequence_score": v.sequence_score, "has_vocab": v._vocab is not None or None}
        return {k: x for k, x in out.items() if x is not None}
    if isinstance(v, np.ndarray):
        if v.size <= 12:
            return {"shape": list(v.shape), "dtype": str(v.dtype), "values": v.tolist()}
        return {"shape": list(v.shape), "dtype": str(v.dtype), "sum": float(v.astype(np.float64).sum())}
    if isinstance(v, (BeamConfig, TokenSet)):
        return repr(v)
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v)
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, tuple):
        return {"tuple": [_plain(x) for x in v]}
    if isinstance(v, list):
        return [_plain(x) for x in v]
    if v is None or isinstance(v, str):
        return v
    return f"<{type(v).__name__}>"


def _attempt(fn):
    """the call's outcome: what it returned, or the exception's type and message"""
    try:
        return {"returns": _plain(fn())}
    except Exception as exc:       # noqa: BLE001 - the refusals are what is recorded
        return {"raises": [type(exc).__name__, str(exc)]}


# ------------------------------------------------------------------------------------------------ Engine on a fake library
# where a symbol of a source kind holds its row count, and (shared) its sources array
_ROWS_AT = {"images": (2, 3), "regions": (4, 5), "gray_host": (2, 3), "device": (2, 3)}
_SRC_AT = {"images": 4, "regions": 6, "gray_host": 4, "device": 4}


def _ints(p, n):
    return np.ctypeslib.as_array((C.c_int32 * n).from_address(p.value)).tolist() if n and p.value else []


class RecordingLib:
    """every mocr_* symbol answers MOCR_OK and logs (symbol, rendered arguments)"""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _arg(a):
        if isinstance(a, C.c_void_p):
            return "null" if not a.value else (hex(a.value) if a.value < 0x100000 else "ptr")     # (the fake device addresses are small)
        if isinstance(a, C.Array) and a._type_ is _capi.MocrImage:
            return ["images"] + [[d.height, d.width, d.row_stride, d.channels, d.rotate] for d in a]
        if isinstance(a, C.Array) and a._type_ is _capi.MocrRegion:
            return ["regions"] + [[r.page, r.x, r.y, r.width, r.height] for r in a]
        if hasattr(a, "_obj"):          # byref(struct)
            return {"byref": {name: _plain(getattr(a._obj, name)) for name, _ in a._obj._fields_}}
        return _plain(a)

    def __getattr__(self, name):
        if not name.startswith("mocr_"):
            raise AttributeError(name)

        def call(*args):
            entry = {"symbol": name, "args": [self._arg(a) for a in args]}
            kind = next((k for k in _ROWS_AT if name.startswith(f"mocr_recognize_{k}_")), None)
            variant = name.rsplit("_", 1)[1]
            if kind and variant in ("positions", "prefix", "shared"):
                rows = args[_ROWS_AT[kind][variant == "shared"]]
                tail = args[-8:] if variant == "positions" else args[-11:]
                entry["sets"], entry["ngram"] = _ints(tail[5], rows), _ints(tail[6], rows)
                if variant != "positions":
                    entry["prefix_len"], entry["prefix"] = _ints(tail[9], rows), _ints(tail[8], rows * tail[10])
                if variant == "shared":
                    entry["sources"] = _ints(args[_SRC_AT[kind]], rows)
            self.calls.append(entry)
            return _capi.MOCR_OK
        return call


def _fill(out):
    """shapes, dtypes and the (constant) fill of the arrays a recognise method returns"""
    if out is None:
        return None
    return [{"shape": list(a.shape), "dtype": str(a.dtype), "fill": sorted({float(x) for x in np.unique(a)})} for a in out]


ENGINE_KW = {
    "plain": {}, "scores": dict(scores=True), "alternatives": dict(alternatives=True), "positions": dict(positions=True),
    "scores+positions": dict(scores=True, positions=True), "alternatives+positions": dict(alternatives=True, positions=True),
    "sets_one": dict(token_sets=3), "sets_each": dict(token_sets=[1, 0, 2]), "ngram_one": dict(no_repeat_ngram=2),
    "ngram_each": dict(no_repeat_ngram=[0, 3, 1]), "prefixes": dict(prefixes=[[7, 8], None, [9]]),
    "everything": dict(alternatives=True, positions=True, token_sets=[1, 0, 2], no_repeat_ngram=2, prefixes=[None, [5, 6, 7], []]),
    "sources": dict(sources=[2, 0, 1, 2]), "sources+scores": dict(scores=True, sources=[0, 1, 2]),
    "sources+everything": dict(alternatives=True, positions=True, sources=[2, 0, 1, 2, 0], token_sets=[1, 0, 2, 0, 1], no_repeat_ngram=[0, 1, 2, 3, 4],
                               prefixes=[[7], None, [8, 9], None, []]),
    "beam": dict(beam=BeamConfig(3, 2.0, True, 3)), "beam_defaults": dict(beam=BeamConfig()),
    # the refusals and their order
    "beam+scores": dict(beam=BeamConfig(2), scores=True), "beam+sources+sets": dict(beam=BeamConfig(2), sources=[0, 1, 2], token_sets=1),
    "beam_not_a_config": dict(beam=4), "beam_too_many": dict(beam=BeamConfig(4)), "beam+bad_sources": dict(beam=BeamConfig(2), sources=7),
    "sources_bad_type": dict(sources=1), "sources_unnamed": dict(sources=[0, 1, 1]), "sources_range": dict(sources=[0, 1, 2, 3]),
    "sets_short": dict(token_sets=[1, 2]), "ngram_short": dict(no_repeat_ngram=[1, 2]), "ngram_bool": dict(no_repeat_ngram=True),
    "ngram_long": dict(no_repeat_ngram=DEFAULT_SPEC.max_len + 1), "prefixes_short": dict(prefixes=[[1]]), "prefixes_nested": dict(prefixes=[[[1]], None, None]),
    "ngram_before_sets": dict(token_sets=[1, 2], no_repeat_ngram=-1), "sets_before_prefixes": dict(token_sets=[1, 2], prefixes=[[1]]),
    "sources_before_ngram": dict(sources=[0, 0], no_repeat_ngram=-1), "ngram_before_prefixes": dict(no_repeat_ngram=[1], prefixes=[[1]]),
    "sources+sets_short": dict(sources=[2, 0, 1, 2], token_sets=[1, 0, 2]), "sources+prefixes_short": dict(sources=[2, 0, 1, 2], prefixes=[None] * 3),
}
# zero sources: nothing is looked at in recognize_images / recognize_regions; recognize_gray and recognize_device make the call
ENGINE_KW_EMPTY = {
    "plain": {}, "alternatives+positions": dict(alternatives=True, positions=True), "sets_one": dict(token_sets=1), "sets_short": dict(token_sets=[1, 2]),
    "ngram_bool": dict(no_repeat_ngram=True), "prefixes_short": dict(prefixes=[[1]]), "prefixes_none": dict(prefixes=[]), "beam": dict(beam=BeamConfig(2)),
    "beam+scores": dict(beam=BeamConfig(2), scores=True), "sources": dict(sources=[0]), "sources_empty": dict(sources=[]),
}


def _device_call(eng, n, kw):
    """recognize_device takes buffers where the host kinds take flags"""
    kw = dict(kw)
    scores, alts, pos = kw.pop("scores", False), kw.pop("alternatives", False), kw.pop("positions", False)
    if "beam" in kw:
        kw["d_out_score"] = 0x8000
    return eng.recognize_device(0x1000, n, 0x2000, 0x3000, 0x4000 if scores or alts else None, 0x5000 if alts else None, 0x6000 if alts else None,
                                d_out_pos=0x7000 if pos else None, **kw)


def record_engine() -> dict:
    eng = object.__new__(Engine)          # no __init__: no library, no GPU
    eng.lib, eng.spec, eng._h, eng.max_batch = RecordingLib(), DEFAULT_SPEC, C.c_void_p(0), 9
    page = np.zeros((32, 48, 3), np.uint8)
    crops = [np.zeros((8, 8), np.uint8), np.zeros((8, 8, 3), np.uint8), page[2:10, 4:12]]       # the last: a view with a row stride
    regs = [(0, 1, 2, 8, 8), (1, 3, 4, 8, 8), (0, 5, 6, 8, 8)]
    kinds = {
        "images": lambda n, kw: eng.recognize_images(crops[:n], **kw),
        "images_bgr_rotate": lambda n, kw: eng.recognize_images(crops[:n], True, [0, 1, 2][:n], **kw),
        "regions": lambda n, kw: eng.recognize_regions([page, page], regs[:n], **kw),
        "regions_rgb": lambda n, kw: eng.recognize_regions([page, page], iter(regs[:n]), False, **kw),
        "gray": lambda n, kw: eng.recognize_gray(np.zeros((n, 224, 224), np.uint8), **kw),
        "gray_max_len": lambda n, kw: eng.recognize_gray(np.zeros((n, 224, 224), np.uint8), 8, **kw),
        "device": lambda n, kw: _device_call(eng, n, kw),
    }
    out = {}
    for kind, call in kinds.items():
        for n, table in ((3, ENGINE_KW), (0, ENGINE_KW_EMPTY)):
            if n == 0 and kind in ("images_bgr_rotate", "regions_rgb", "gray_max_len"):
                continue
            for name, kw in table.items():
                eng.lib.calls = []
                try:
                    entry = {"returns": _fill(call(n, kw))}
                except Exception as exc:       # noqa: BLE001
                    entry = {"raises": [type(exc).__name__, str(exc)]}
                entry["calls"] = eng.lib.calls
                out[f"{kind}[{n}] {name}"] = entry
    return out


# ------------------------------------------------------------------------------------------------ MangaOcr on a fake engine
class RecordingEngine:
    """recognize_images / recognize_regions as Engine answers them: logs (method, positional arguments, keywords) and returns
    deterministic blocks of the arity the keywords ask for.  Row r reads START, its prefix, 10 + r, 20 + r, EOS; a region of width
    0 is a sliver (length 0); beam slot j of crop i reads START, 10 + i, 30 + j, EOS and the last slot is empty."""
    L = 12

    def __init__(self):
        self.calls = []

    def token_set(self, ids):
        self.calls.append(["token_set", len(list(ids))])
        return 7

    def recognize_images(self, images, bgr=False, rotate=None, **kw):
        return self._answer("recognize_images", (images, bgr, rotate), kw, [False] * len(images))

    def recognize_regions(self, pages, regions, bgr=True, **kw):
        return self._answer("recognize_regions", (pages, regions, bgr), kw, [int(r[3]) == 0 for r in regions])

    def _answer(self, method, args, kw, sliver):
        self.calls.append([method, _plain(list(args)), _plain(kw)])
        L = self.L
        if "beam" in kw:
            n, K = len(sliver), kw["beam"].num_beams
            ids, lens, sc = np.zeros((n, K, L), np.int32), np.zeros((n, K), np.int32), np.full((n, K), -1e9, np.float32)
            for i in range(n):
                for j in range(K - 1):
                    if not sliver[i]:
                        ids[i, j, :4], lens[i, j], sc[i, j] = [START, 10 + i, 30 + j, EOS], 4, -(i + 0.25 * j)
            return ids, lens, sc
        src = kw.get("sources")
        src = list(range(len(sliver))) if src is None else list(src)
        n = len(src)
        ids, lens, logp = np.zeros((n, L), np.int32), np.zeros(n, np.int32), np.zeros((n, L), np.float32)
        alt_ids, alt_logp = np.full((n, L, 4), -1, np.int32), np.zeros((n, L, 4), np.float32)
        pos = np.zeros((n, L, 5), np.float32)
        for r in range(n):
            if sliver[src[r]]:
                continue
            pre = (kw.get("prefixes") or [None] * n)[r] or []
            row = ([START] + [int(t) for t in pre] + [10 + r, 20 + r, EOS])[:L]
            ids[r, :len(row)], lens[r] = row, len(row)
            for t in range(1, len(row)):
                logp[r, t] = -(0.125 * t + r)
                alt_ids[r, t] = [row[t], row[t] + 30, row[t] + 31, -1]
                alt_logp[r, t] = [logp[r, t], logp[r, t] - 0.5 * t, logp[r, t] - 4.0, 0.0]
                pos[r, t] = [t / 16.0, (r + 1) / 16.0, 1 / 32.0, 1 / 64.0, 1.0]
        out = (ids, lens)
        if kw.get("scores") or kw.get("alternatives"):
            out += (logp,)
        if kw.get("alternatives"):
            out += (alt_ids, alt_logp)
        if kw.get("positions"):
            out += (pos,)
        return out


VOCAB = Vocab.synthetic(64)         # ids 5 .. 63 spell one ideograph each: no half-width text, whatever converter is installed
CH = [chr(0x4E00 + i) for i in range(8)]


def _ocr(engine, *, minimal=False, ngram=None, beam=None, max_batch=4):
    """a MangaOcr without __init__; ``minimal``: only ``engine`` and ``vocab`` set"""
    ocr = object.__new__(MangaOcr)
    ocr.engine, ocr.vocab = engine, VOCAB
    if not minimal:
        ocr.spec, ocr.max_batch, ocr.no_repeat_ngram_size, ocr.beam = DEFAULT_SPEC, max_batch, ngram, beam
        ocr._token_sets, ocr._token_sets_lock = {}, threading.Lock()
        ocr._batcher = _Batcher(engine, max_batch, 0.0)      # no window: every single-crop call is its own batch
    return ocr


def _img(v=0, mode="L"):
    from PIL import Image
    a = np.full((8, 8), v, np.uint8) if mode == "L" else np.full((8, 8, 3), v, np.uint8)
    return Image.fromarray(a)


def _decode_keywords(n: int) -> dict:
    """the allowed= / no_repeat_ngram= / prefix= combinations a method with ``n`` crops is run under"""
    each = dict(allowed=[TokenSet(1, 10), 0, 2][:n], no_repeat_ngram=[0, 3, 1][:n], prefix=[[7, 8], None, CH[2]][:n])
    return {
        "nothing": {}, "allowed": dict(allowed=3), "allowed_set": dict(allowed=TokenSet(5, 10)), "ngram": dict(no_repeat_ngram=2),
        "ngram_off": dict(no_repeat_ngram=0), "prefix_str": dict(prefix=CH[0] + CH[1]), "prefix_ids": dict(prefix=[7, 8, 9]), "prefix_empty": dict(prefix=[]),
        "all": dict(allowed=3, no_repeat_ngram=2, prefix=CH[0]),
        "allowed_each": dict(allowed=each["allowed"]), "ngram_each": dict(no_repeat_ngram=each["no_repeat_ngram"]), "prefix_each": dict(prefix=each["prefix"]),
        "all_each": each,
        "allowed_short": dict(allowed=[1] * (n + 1)), "ngram_bool": dict(no_repeat_ngram=True), "ngram_negative": dict(no_repeat_ngram=-1),
        "prefix_scalar": dict(prefix=5), "prefix_unknown_char": dict(prefix="#"), "prefix_short": dict(prefix=[None] * (n + 1) if n != 0 else [None]),
    }


EMPTY_COMBOS = ("nothing", "all", "all_each", "allowed_short")      # what the methods are run under with no crops


def _surface(ocr, n: int) -> dict:
    """name -> callable(**decode keywords) for the methods that take allowed= / no_repeat_ngram= / prefix=; with one crop
    only the single-crop methods (the batch methods run with three crops and with none)"""
    page = np.zeros((32, 48, 3), np.uint8)
    crops = [np.zeros((8, 8, 3), np.uint8), np.zeros((6, 8, 3), np.uint8), np.zeros((8, 6, 3), np.uint8)][:n]
    regs = [(0, 1, 2, 8, 8), (1, 3, 4, 0, 8), (0, 5, 6, 8, 8)][:n]          # the middle one: a sliver
    ori = ["Vertical", "Vertical", "Horizontal"][:n]
    out = {}
    if n == 1:
        out["__call__"] = lambda **kw: ocr(_img(), **kw)
    for sfx in ("", "_scored", "_alternatives", "_positions"):
        if n == 1:
            out["recognize" + sfx] = lambda sfx=sfx, **kw: getattr(ocr, "recognize" + sfx)(_img(3, "RGB"), **kw)
        if n == 1:
            continue
        out["recognize_batch" + sfx] = lambda sfx=sfx, **kw: getattr(ocr, "recognize_batch" + sfx)([_img(i) for i in range(n)], **kw)
        out["recognize_bgr" + sfx] = lambda sfx=sfx, **kw: getattr(ocr, "recognize_bgr" + sfx)(crops, **kw)
        out["recognize_bgr" + sfx + " orientations"] = lambda sfx=sfx, **kw: getattr(ocr, "recognize_bgr" + sfx)(iter(crops) if sfx else crops, ori, **kw)
        out["recognize_regions" + sfx] = lambda sfx=sfx, **kw: getattr(ocr, "recognize_regions" + sfx)([page, page], iter(regs), **kw)
    if n == 1:
        return out
    out["recognize_ids"] = lambda **kw: ocr.recognize_ids(crops, **kw)
    out["recognize_ids bgr rotate"] = lambda **kw: ocr.recognize_ids(iter(crops), True, [0, 1, 2][:n], **kw)
    out["recognize_batch_arrays"] = lambda **kw: ocr.recognize_batch_arrays(iter(crops), **kw)
    return out


def _run(engine, fn, **kw):
    engine.calls = []
    entry = _attempt(lambda: fn(**kw))
    entry["engine"] = engine.calls
    return entry


def record_ocr() -> dict:
    out = {}
    eng = RecordingEngine()
    ocr = _ocr(eng)
    try:
        for n in (1, 3, 0):
            for method, fn in _surface(ocr, n).items():
                for name, kw in _decode_keywords(n).items():
                    if (method == "__call__" and kw) or (n == 0 and name not in EMPTY_COMBOS):
                        continue
                    out[f"{method}[{n}] {name}"] = _run(eng, fn, **kw)
        # the n-best and scoring methods, the beam forms
        imgs = [_img(i) for i in range(3)]
        page = np.zeros((32, 48, 3), np.uint8)
        crops = [np.zeros((8, 8, 3), np.uint8), np.zeros((6, 8, 3), np.uint8), np.zeros((8, 6, 3), np.uint8)]
        regs = [(0, 1, 2, 8, 8), (1, 3, 4, 0, 8), (0, 5, 6, 8, 8)]
        more = {
            "score_text str": lambda: ocr.score_text(_img(), CH[0] + CH[1]), "score_text ids": lambda: ocr.score_text(_img(), [7, 8]),
            "score_text empty": lambda: ocr.score_text(_img(), ""), "score_text too long": lambda: ocr.score_text(_img(), [7] * DEFAULT_SPEC.max_len),
            "score_text unknown char": lambda: ocr.score_text(_img(), "#"),
            "score_texts": lambda: ocr.score_texts(imgs, [CH[0], [7, 8], ""]), "score_texts none": lambda: ocr.score_texts([], []),
            "score_texts mismatch": lambda: ocr.score_texts(imgs, [CH[0]]),
            "score_candidates": lambda: ocr.score_candidates(_img(), [CH[0] + CH[1], [7, 8, 9], ""]), "score_candidates none": lambda: ocr.score_candidates(5, []),
            "score_candidates unknown char": lambda: ocr.score_candidates(5, ["#"]),
            "token_set": lambda: [ocr.token_set(chars=CH[:3]), ocr.token_set(chars=CH[:3]), ocr.token_set(ids=[5, 6], exclude_chars=CH[0])],
        }
        for k in (1, 2, 4):
            more[f"recognize_nbest k={k}"] = lambda k=k: ocr.recognize_nbest(_img(), k)
            more[f"recognize_batch_nbest k={k}"] = lambda k=k: ocr.recognize_batch_nbest(imgs, k)
            more[f"recognize_batch_nbest k={k} keywords"] = lambda k=k: ocr.recognize_batch_nbest(imgs, k, allowed=[1, 0, 2], no_repeat_ngram=[0, 3, 1])
        more["recognize_batch_nbest none"] = lambda: ocr.recognize_batch_nbest([], 3)
        more["recognize_batch_nbest bad k"] = lambda: ocr.recognize_batch_nbest(imgs, True)
        more["recognize_nbest allowed"] = lambda: ocr.recognize_nbest(_img(), 3, allowed=TokenSet(4, 9), no_repeat_ngram=2)
        for name, bkw in (("defaults", {}), ("config", dict(num_beams=3, length_penalty=2.0, early_stopping="never", no_repeat_ngram=3)),
                          ("bad num_beams", dict(num_beams=5)), ("bad early_stopping", dict(early_stopping="no"))):
            more[f"recognize_beam {name}"] = lambda bkw=bkw: ocr.recognize_beam(_img(), **bkw)
            more[f"recognize_batch_beam {name}"] = lambda bkw=bkw: ocr.recognize_batch_beam(imgs, **bkw)
            more[f"recognize_bgr_beam {name}"] = lambda bkw=bkw: ocr.recognize_bgr_beam(crops, **bkw)
            more[f"recognize_bgr_beam orientations {name}"] = lambda bkw=bkw: ocr.recognize_bgr_beam(iter(crops), ["Vertical", "Vertical", "Horizontal"], **bkw)
            more[f"recognize_regions_beam {name}"] = lambda bkw=bkw: ocr.recognize_regions_beam([page, page], iter(regs), **bkw)
        more["recognize_batch_beam none"] = lambda: ocr.recognize_batch_beam([])
        more["recognize_bgr_beam none"] = lambda: ocr.recognize_bgr_beam([], [])
        more["recognize_regions_beam none"] = lambda: ocr.recognize_regions_beam([page], [])
        for name, fn in more.items():
            out[name] = _run(eng, fn)
    finally:
        ocr._batcher.close()

    # constructor-level no_repeat_ngram_size and beam, and the instance with nothing but engine and vocab
    for tag, make in (("ngram_size=3", lambda e: _ocr(e, ngram=3)), ("ngram_size=0", lambda e: _ocr(e, ngram=0)),
                      ("beam", lambda e: _ocr(e, beam=BeamConfig(2, 2.0, True, 3))), ("minimal", lambda e: _ocr(e, minimal=True))):
        eng = RecordingEngine()
        ocr = make(eng)
        try:
            for n in (1, 3, 0):
                for method, fn in _surface(ocr, n).items():
                    if tag == "minimal" and (method == "__call__" or method.startswith("recognize ") or method in
                                             ("recognize", "recognize_scored", "recognize_alternatives", "recognize_positions")):
                        continue        # (the single-crop methods need the batcher)
                    if "_alternatives" in method or ("_positions" in method and "regions" not in method):
                        continue        # (the runner-up kinds differ from the scored one in nothing these settings touch)
                    for name in ("nothing", "allowed", "ngram_off", "all_each"):
                        kw = _decode_keywords(n)[name]
                        if (method == "__call__" and kw) or (n == 0 and name not in EMPTY_COMBOS):
                            continue
                        out[f"<{tag}> {method}[{n}] {name}"] = _run(eng, fn, **kw)
            if tag != "minimal":
                imgs = [_img(i) for i in range(3)]
                out[f"<{tag}> recognize_batch_nbest"] = _run(eng, lambda: ocr.recognize_batch_nbest(imgs, 2))
                out[f"<{tag}> score_texts"] = _run(eng, lambda: ocr.score_texts(imgs, [CH[0], [7, 8], ""]))
                out[f"<{tag}> score_candidates"] = _run(eng, lambda: ocr.score_candidates(imgs[0], [CH[0], [7, 8]]))
                out[f"<{tag}> recognize_batch_beam"] = _run(eng, lambda: ocr.recognize_batch_beam(imgs, 2))
                out[f"<{tag}> recognize_beam"] = _run(eng, lambda: ocr.recognize_beam(imgs[0], 3))
        finally:
            if hasattr(ocr, "_batcher"):
                ocr._batcher.close()
    return out


# ------------------------------------------------------------------------------------------------ the refusals
def record_errors() -> dict:
    from manga_ocr.multi import MultiGpuEngine
    out = {}
    page = np.zeros((32, 48, 3), np.uint8)
    crops = [np.zeros((8, 8, 3), np.uint8)] * 3
    regs = [(0, 1, 2, 8, 8)] * 3
    # several devices: the refusal comes before the image is opened or any argument is looked at (5 is no image, the
    # orientations are short).  No worker: whatever gets past the refusal fails on an attribute __init__ would have set.
    ocr = _ocr(object.__new__(MultiGpuEngine))       # no __init__: no child process, no GPU
    multi = {"token_set": lambda: ocr.token_set(chars="a"), "score_text": lambda: ocr.score_text(5, "#"), "score_texts": lambda: ocr.score_texts([5], ["#"]),
             "score_candidates": lambda: ocr.score_candidates(5, ["#"]), "recognize_nbest k=1": lambda: ocr.recognize_nbest(5, 1),
             "recognize_nbest k=2": lambda: ocr.recognize_nbest(5, 2), "recognize_batch_nbest k=1": lambda: ocr.recognize_batch_nbest([5], 1),
             "recognize_batch_nbest k=2": lambda: ocr.recognize_batch_nbest([5], 2), "recognize_batch_nbest bad k": lambda: ocr.recognize_batch_nbest([5], 0)}
    for sfx in ("_scored", "_alternatives", "_positions", "_beam"):
        multi["recognize" + sfx] = lambda sfx=sfx: getattr(ocr, "recognize" + sfx)(5)
        multi["recognize_batch" + sfx] = lambda sfx=sfx: getattr(ocr, "recognize_batch" + sfx)([5])
        multi["recognize_bgr" + sfx] = lambda sfx=sfx: getattr(ocr, "recognize_bgr" + sfx)(crops, ["Vertical"])
        multi["recognize_regions" + sfx] = lambda sfx=sfx: getattr(ocr, "recognize_regions" + sfx)([page], regs)
    for kname, kw in (("allowed", dict(allowed=1)), ("ngram", dict(no_repeat_ngram=2)), ("prefix", dict(prefix=[7])),
                      ("all", dict(allowed=1, no_repeat_ngram=2, prefix=[7])), ("ngram_off", dict(no_repeat_ngram=0))):
        for sfx in ("", "_scored", "_alternatives", "_positions"):
            if sfx and kname != "all":
                continue
            multi[f"recognize{sfx} {kname}"] = lambda sfx=sfx, kw=kw: getattr(ocr, "recognize" + sfx)(_img(), **kw)
            multi[f"recognize_batch{sfx} {kname}"] = lambda sfx=sfx, kw=kw: getattr(ocr, "recognize_batch" + sfx)([_img()], **kw)
            multi[f"recognize_bgr{sfx} {kname}"] = lambda sfx=sfx, kw=kw: getattr(ocr, "recognize_bgr" + sfx)(crops[:1], **kw)
            multi[f"recognize_regions{sfx} {kname}"] = lambda sfx=sfx, kw=kw: getattr(ocr, "recognize_regions" + sfx)([page], regs[:1], **kw)
        if kname != "ngram_off":
            multi[f"recognize_ids {kname}"] = lambda kw=kw: ocr.recognize_ids(crops[:1], **kw)
            multi[f"recognize_batch_arrays {kname}"] = lambda kw=kw: ocr.recognize_batch_arrays(crops[:1], **kw)
    ocr.no_repeat_ngram_size = 3        # (the constructor refuses this; the calls still must)
    multi["recognize_batch <ngram_size=3>"] = lambda: ocr.recognize_batch([_img()])
    multi["recognize_regions <ngram_size=3> ngram_off"] = lambda: ocr.recognize_regions_scored([page], regs[:1], no_repeat_ngram=0)
    try:
        for name, fn in multi.items():
            out["multi " + name] = _attempt(fn)
    finally:
        ocr._batcher.close()

    # one device: short orientations and arguments that are no image, before any engine call; the order of the checks
    for tag, okw in (("greedy", {}), ("beam", dict(beam=BeamConfig(2)))):
        eng = RecordingEngine()
        ocr = _ocr(eng, **okw)
        try:
            one = {}
            for sfx in ("", "_scored", "_alternatives", "_positions", "_beam"):
                one[f"recognize_bgr{sfx} short orientations"] = lambda sfx=sfx: getattr(ocr, "recognize_bgr" + sfx)(crops, ["Vertical", "Horizontal"])
                one[f"recognize_bgr{sfx} long orientations"] = lambda sfx=sfx: getattr(ocr, "recognize_bgr" + sfx)(crops[:1], ["Vertical", "Horizontal"])
                one[f"recognize{sfx} no image"] = lambda sfx=sfx: getattr(ocr, "recognize" + sfx)(5)
                one[f"recognize{sfx} no image, array"] = lambda sfx=sfx: getattr(ocr, "recognize" + sfx)(np.zeros((8, 8), np.uint8))
                if sfx != "_beam":
                    one[f"recognize{sfx} no image, bad keywords"] = lambda sfx=sfx: getattr(ocr, "recognize" + sfx)(5, allowed=[1, 2], no_repeat_ngram=True, prefix=5)
                    one[f"recognize_bgr{sfx} short orientations, bad keywords"] = \
                        lambda sfx=sfx: getattr(ocr, "recognize_bgr" + sfx)(crops, ["Vertical"], allowed=[1], no_repeat_ngram=True)
                else:
                    one["recognize_bgr_beam short orientations, bad config"] = lambda: ocr.recognize_bgr_beam(crops, ["Vertical"], num_beams=9)
                    one["recognize_beam no image, bad config"] = lambda: ocr.recognize_beam(5, num_beams=9)
            one["__call__ no image"] = lambda: ocr(5)
            one["score_text no image"] = lambda: ocr.score_text(5, CH[0])
            one["score_text no image, unknown char"] = lambda: ocr.score_text(5, "#")
            one["score_candidates no image"] = lambda: ocr.score_candidates(5, [CH[0]])
            one["recognize_nbest no image"] = lambda: ocr.recognize_nbest(5, 2)
            one["recognize_nbest no image, bad k"] = lambda: ocr.recognize_nbest(5, 0)
            one["recognize_batch no image"] = lambda: ocr.recognize_batch([5])
            one["recognize_regions bad region"] = lambda: ocr.recognize_regions_positions([page], [(3, 1, 2, 8, 8)])
            for name, fn in one.items():
                out[f"{tag} {name}"] = _run(eng, fn)
        finally:
            ocr._batcher.close()
    return out


def record() -> dict:
    return {"engine": record_engine(), "ocr": record_ocr(), "errors": record_errors()}


def group(name: str) -> str:
    """the method (in front, its instance: "<beam>", "multi", ...) a scenario belongs to, whatever the number of crops"""
    words = name.split(" ")
    return " ".join(words[:2] if words[0].startswith("<") or words[0] in ("multi", "greedy", "beam") else words[:1]).split("[")[0]


def digest(rec: dict) -> dict:
    """section -> group -> [scenarios, sha256 of their canonical JSON (16 hex digits)]: what surface.json holds.  The scenarios
    themselves would be half a megabyte; ``--show GROUP`` prints a group's in full, to compare two commits with."""
    import hashlib
    out = {}
    for section, entries in rec.items():
        groups = {}
        for name, entry in entries.items():
            groups.setdefault(group(name), []).append([name, entry])
        out[section] = {g: [len(rows), hashlib.sha256(json.dumps(rows, sort_keys=True, ensure_ascii=True).encode()).hexdigest()[:16]]
                        for g, rows in groups.items()}
    return out


def dump(rec: dict) -> str:
    """one group per line, in the order recorded"""
    parts = []
    for section, groups in digest(rec).items():
        rows = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in groups.items())
        parts.append(f" {json.dumps(section)}: {{\n{rows}\n }}")
    return "{\n" + ",\n".join(parts) + "\n}\n"


if __name__ == "__main__":
    if sys.argv[1:2] == ["--show"]:
        for section, entries in record().items():
            for name, entry in entries.items():
                if group(name) == sys.argv[2]:
                    print(json.dumps(name), json.dumps(entry, sort_keys=True))
        sys.exit(0)
    text = dump(record())
    with open(PATH, "w", encoding="ascii") as f:
        f.write(text)
    print(PATH, len(text), "bytes;", {k: [len(v), sum(n for n, _ in v.values())] for k, v in json.loads(text).items()}, "[groups, scenarios]")
