"""CPU: the token-position feature's host side - the float64 reference (position_util) on hand cases, the condition on the
end-to-end tests' weights (the scaled query spreads the positions), Recognition.boxes under both device rotations against
numpy.rot90, the regions mapping, the batcher merging requests with and without positions on a fake engine, the
multi-device refusal and the library's new exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import position_util as pu
from manga_ocr import _capi, text
from manga_ocr.ocr import MangaOcr, Recognition, _Batcher
from manga_ocr.regions import padded_rect
from manga_ocr.weights import DEFAULT_SPEC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mocr_recognize_images_positions", "mocr_recognize_regions_positions", "mocr_recognize_device_positions",
       "mocr_recognize_gray_host_positions", "mocr_op_attn_positions"]
P = C.c_void_p


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return _capi.load_library()


def _key(i, j):
    return 1 + 14 * i + j


def test_the_reference_on_hand_cases():
    a = np.zeros(197)
    a[_key(3, 10)] = 1.0
    np.testing.assert_allclose(pu.fields_from_map(a), [10.5 / 14, 3.5 / 14, 0.0, 0.0, 1.0], atol=1e-9)
    a = np.zeros(197)
    a[0] = 1.0                                              # all weight on CLS: the guard values
    np.testing.assert_array_equal(pu.fields_from_map(a), [0.5, 0.5, 0.0, 0.0, 0.0])
    a = np.full(197, 1.0 / 197)
    sd = np.sqrt((((np.arange(14) + 0.5) / 14 - 0.5) ** 2).mean())              # the grid's standard deviation
    np.testing.assert_allclose(pu.fields_from_map(a), [0.5, 0.5, sd, sd, 196.0 / 197], atol=1e-12)
    # two patches in one grid row: the centre between them, spread in u only
    a = np.zeros(197)
    a[_key(2, 4)] = a[_key(2, 8)] = 0.25                    # half the mass on CLS
    a[0] = 0.5
    np.testing.assert_allclose(pu.fields_from_map(a), [6.5 / 14, 2.5 / 14, 2.0 / 14, 0.0, 0.5], atol=1e-9)
    # head_mean_map: the softmax per head FIRST, then the mean - one sharp head and eleven flat ones
    q = np.zeros((1, 1, 768))
    K = np.zeros((1, 197, 768))
    q[0, 0, :64] = 1.0
    K[0, _key(5, 6), :64] = 100.0                           # head 0: a delta on patch (5, 6); heads 1 .. 11: uniform
    m = pu.head_mean_map(q, K)[0, 0]
    want = np.full(197, 11.0 / 12 / 197)
    want[_key(5, 6)] += 1.0 / 12
    np.testing.assert_allclose(m, want, atol=1e-12)
    m2, f2 = pu.ref_positions(np.repeat(q, 3, axis=1), K, [2])
    assert (m2[0, 2] == 0).all() and (f2[0, 2] == 0).all() and f2[0, 1, 4] > 0.9


@pytest.fixture(scope="module")
def spread_case():
    from gpu_util import crops
    from oracle.mocr_oracle import Oracle, row_lengths
    o = Oracle(pu.pos_weights(), DEFAULT_SPEC)
    gray = crops(pu.CROP_SEED, 6)
    ids = o.generate(o.encode(o.preprocess_gray(gray)), max_len=24)
    lens = row_lengths(ids)
    return ids, lens, pu.reference_for_ids(o, gray, ids, lens)


def test_the_scaled_query_spreads_the_positions(spread_case):
    """the condition of the end-to-end tests: with G and the test crops the reference cx and cy each vary over the tokens with
    a standard deviation of at least 0.05 and the mass stays above 0.5 (synthetic_weights alone: ~0.003, nothing to see)"""
    ids, lens, ref = spread_case
    sel = np.concatenate([ref[b, 1:lens[b]] for b in range(len(lens))])
    assert sel[:, 0].std() >= 0.05 and sel[:, 1].std() >= 0.05, (sel[:, 0].std(), sel[:, 1].std())
    assert sel[:, 4].min() > 0.5
    assert len(set(lens.tolist())) >= 3 and lens.min() < 24, "the rows end at different lengths (early EOS)"
    for b in range(len(lens)):
        assert (ref[b, 0] == 0).all() and (ref[b, lens[b]:] == 0).all()


def _rec(pos, rect=None):
    pos = np.asarray(pos, np.float32)
    n = pos.shape[0]
    return Recognition("x", np.zeros(n, np.int32), np.zeros(n - 1, np.float32), 1.0, 1.0, positions=pos, rect=rect)


@pytest.mark.parametrize("rotate,k", [(0, 0), (1, -1), (2, 1)])
def test_boxes_map_back_through_the_device_rotation(rotate, k):
    """an H x W crop with one marked pixel; the encoder sees numpy.rot90(crop, k) (k = -1: clockwise); the position of the
    marked pixel in THAT plane must come back as the pixel's own rectangle on the crop"""
    Hc, Wc, y0, x0 = 30, 50, 7, 41
    img = np.zeros((Hc, Wc), np.uint8)
    img[y0, x0] = 1
    seen = np.rot90(img, k)
    ys, xs = np.nonzero(seen)
    hs, ws = seen.shape
    cx, cy = (xs[0] + 0.5) / ws, (ys[0] + 0.5) / hs
    sx, sy = 0.5 / ws / 2.0, 0.5 / hs / 2.0                 # k = 2 spreads: exactly the pixel
    r = _rec([[0, 0, 0, 0, 0], [cx, cy, sx, sy, 1.0]])
    b = r.boxes(Wc, Hc, rotate=rotate)
    assert b.shape == (2, 4) and (b[0] == 0).all()
    np.testing.assert_allclose(b[1], [x0, y0, x0 + 1, y0 + 1], atol=1e-5)
    # clipped to the crop; k scales the spread
    wide = _rec([[0, 0, 0, 0, 0], [0.1, 0.9, 0.2, 0.2, 1.0]]).boxes(100, 200, k=1.0)
    np.testing.assert_allclose(wide[1], [0.0, 140.0, 30.0, 200.0], atol=1e-4)
    with pytest.raises(ValueError):
        Recognition("x", np.zeros(1, np.int32), np.zeros(0, np.float32), 0.0, 0.0).boxes(10, 10)
    with pytest.raises(ValueError):
        r.boxes(10, 10, rotate=3)


def test_regions_map_into_page_pixels_through_the_padded_rectangle():
    # the rule of the engine's region cut: grown by int(max(w, h) * 0.08), clipped to the page; a sliver is not decoded
    assert padded_rect((100, 50, 200, 100), 1000, 800) == (84, 34, 232, 132)
    assert padded_rect((0, 0, 50, 100), 120, 55) == (0, 0, 55, 108)
    assert padded_rect((790, 10, 50, 50), 1000, 800) == (786, 6, 14, 58)
    assert padded_rect((803, 10, 50, 50), 1000, 800) is None and padded_rect((10, 10, 0, 0), 100, 100) is None
    r = _rec([[0, 0, 0, 0, 0], [0.5, 0.25, 0.05, 0.1, 0.9]], rect=(84, 34, 232, 132))
    np.testing.assert_allclose(r.page_boxes()[1], [84 + 0.4 * 232, 34 + 0.05 * 132, 84 + 0.6 * 232, 34 + 0.45 * 132], atol=1e-3)
    assert (r.page_boxes()[0] == 0).all()
    with pytest.raises(ValueError):
        _rec([[0, 0, 0, 0, 0]]).page_boxes()
    # from_row: row 0 zeros, [len, 5]; a sliver has no rows
    pos = np.arange(6 * 5, dtype=np.float32).reshape(6, 5)
    pos[0] = 0
    rec = Recognition.from_row(text.Vocab.synthetic(6144), np.array([2, 9, 3, 0, 0, 0]), np.zeros(6, np.float32), 3, pos_row=pos, rect=(1, 2, 3, 4))
    assert rec.positions.shape == (3, 5) and (rec.positions[0] == 0).all() and rec.rect == (1, 2, 3, 4)
    np.testing.assert_array_equal(rec.positions[1:], pos[1:3])
    sl = Recognition.from_row(text.Vocab.synthetic(6144), np.zeros(6, np.int32), np.zeros(6, np.float32), 0, pos_row=np.zeros((6, 5), np.float32))
    assert sl.positions.shape == (0, 5) and sl.text == ""


class _FakeEngine:
    """recognize_images as Engine answers it; logs the keywords of each call.  Position row t of crop i is filled with
    first pixel + t."""
    L = 6

    def __init__(self):
        self.calls = []

    def recognize_images(self, images, bgr=False, rotate=None, *, scores=False, alternatives=False, **kw):
        assert set(kw) <= {"token_sets", "no_repeat_ngram", "positions"}
        self.calls.append((len(images), 1 if scores else 0, dict(kw)))
        n = len(images)
        ids = np.zeros((n, self.L), np.int32)
        ids[:, 0], ids[:, 2] = 2, 3
        ids[:, 1] = [int(im[0, 0]) for im in images]
        lens = np.full(n, 3, np.int32)
        out = (ids, lens, np.zeros((n, self.L), np.float32)) if scores else (ids, lens)
        if kw.get("positions"):
            pos = np.zeros((n, self.L, 5), np.float32)
            for i, im in enumerate(images):
                pos[i] = (int(im[0, 0]) + np.arange(self.L))[:, None]
            out = out + (pos,)
        return out


def test_the_batcher_merges_requests_with_and_without_positions():
    eng = _FakeEngine()
    b = _Batcher(eng, max_batch=4, timeout_ms=60_000.0)
    try:
        futs = [b.submit(np.full((4, 4), 10 + i, np.uint8), scored=i in (1, 2), positions=i in (2, 3)) for i in range(4)]
        res = [f.result(timeout=30) for f in futs]
        assert eng.calls == [(4, 1, dict(positions=True))], "one engine call: scored, with positions"
        np.testing.assert_array_equal(res[0], [2, 10, 3])                          # plain: ids
        assert len(res[1]) == 2 and len(res[2]) == 3 and len(res[3]) == 2           # scored; scored + positions; ids + positions
        np.testing.assert_array_equal(res[2][2], (12 + np.arange(3))[:, None] * np.ones((1, 5)))
        np.testing.assert_array_equal(res[3][0], [2, 13, 3])
        np.testing.assert_array_equal(res[3][1][:, 0], [13, 14, 15])
        # nobody asked: the call of before, without the keyword
        futs = [b.submit(np.full((4, 4), 7, np.uint8)) for _ in range(4)]
        [f.result(timeout=30) for f in futs]
        assert eng.calls[-1] == (4, 0, {})
    finally:
        b.close()


def test_positions_refuse_several_devices_without_spawning_workers():
    from manga_ocr.multi import MultiGpuEngine
    eng = object.__new__(MultiGpuEngine)          # no __init__: no child process, no GPU
    with pytest.raises(NotImplementedError, match="token positions.*several devices"):
        eng.recognize_images([np.zeros((8, 8), np.uint8)], positions=True)
    with pytest.raises(NotImplementedError, match="token positions.*several devices"):
        eng.recognize_regions([np.zeros((8, 8, 3), np.uint8)], [(0, 0, 0, 4, 4)], positions=True)
    ocr = object.__new__(MangaOcr)
    ocr.engine, ocr.no_repeat_ngram_size = eng, None
    ocr.vocab = text.Vocab.synthetic(6144)
    for call in (lambda: ocr.recognize_batch_positions([]), lambda: ocr.recognize_bgr_positions([np.zeros((8, 8, 3), np.uint8)]),
                 lambda: ocr.recognize_regions_positions([np.zeros((8, 8, 3), np.uint8)], [(0, 0, 0, 4, 4)])):
        with pytest.raises(NotImplementedError, match="token positions.*several devices"):
            call()


def test_position_symbols_are_exported_declared_and_mirrored(lib):
    hdr = open(os.path.join(ROOT, "include", "mocr.h")).read()
    for name in NEW:
        assert name in _capi.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in mocr.h"
        assert getattr(lib, name) is not None
    for nr, ps in [("mocr_recognize_images_norepeat", "mocr_recognize_images_positions"),
                   ("mocr_recognize_regions_norepeat", "mocr_recognize_regions_positions"),
                   ("mocr_recognize_device_norepeat", "mocr_recognize_device_positions"),
                   ("mocr_recognize_gray_host_norepeat", "mocr_recognize_gray_host_positions")]:
        assert _capi.SYMBOLS[ps][1] == _capi.SYMBOLS[nr][1] + [P], ps             # the _norepeat twin plus out_pos
    assert _capi.SYMBOLS["mocr_op_attn_positions"][1] == [P, P, P, P, C.c_int32, C.c_int32, P, P]
    assert re.search(r"#define\s+MOCR_POSITION_FIELDS\s+5\b", hdr) and _capi.POSITION_FIELDS == 5
    # the ABI did not move; null handles are refused before anything is dereferenced
    assert lib.mocr_abi_version() == 2
    assert lib.mocr_recognize_images_positions(None, None, 1, None, None, None, None, None, None, None, None) == -1
    assert lib.mocr_recognize_regions_positions(None, None, 1, None, 1, None, None, None, None, None, None, None, None) == -1
    assert lib.mocr_recognize_device_positions(None, None, 1, None, None, None, None, None, None, None, None) == -1
    assert lib.mocr_recognize_gray_host_positions(None, None, 1, 8, None, None, None, None, None, None, None, None) == -1
    assert lib.mocr_op_attn_positions(None, None, None, None, 1, 1, None, None) == -1
