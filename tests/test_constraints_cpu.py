"""CPU: the token-constraint feature's host side - ``Vocab.ids_for_chars`` on a hand-written vocabulary, a numpy model of
the masked tile merge the kernels rely on (tiles with no allowed column, sets of one to three tokens) against the float64
masked log-softmax, the new exports, the routing of ``allowed=`` through the batcher on a fake engine, ``candidates()``
skipping the entries a small set leaves empty, and the multi-device refusal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import constraint_util as cu
import score_util as su
from manga_ocr import _capi, text
from manga_ocr.ocr import MangaOcr, Recognition, TokenSet, _Batcher, _set_handles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mocr_token_set_create", "mocr_token_set_count", "mocr_recognize_images_constrained", "mocr_recognize_regions_constrained",
       "mocr_recognize_device_constrained", "mocr_recognize_gray_host_constrained", "mocr_op_gemm_argmax_masked",
       "mocr_op_dec_token_masked"]
P = C.c_void_p


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return _capi.load_library()


def test_ids_for_chars_on_a_hand_written_vocabulary():
    toks = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "1", "2", "##3", "12", "1a", "##", " ", "", "あ", "##あい", "ア", "１", "1 2", "[", "##[U"]
    v = text.Vocab(toks)
    assert v.ids_for_chars("0123456789") == [5, 6, 7, 8, 17]          # "##3" by its body, "1 2" with its whitespace stripped
    assert v.ids_for_chars(["12", "3"]) == [5, 6, 7, 8, 17]           # any iterable of strings
    assert v.ids_for_chars("1") == [5]
    assert v.ids_for_chars("あい") == [13, 14]
    assert v.ids_for_chars("１") == [16], "raw token text: the full-width digit is its own character"
    assert v.ids_for_chars("[]UNKPADCLSEMa") == [18, 19], "special tokens never count, whatever their letters"
    assert v.ids_for_chars("") == [] and v.ids_for_chars("xyz") == []
    everything = v.ids_for_chars("".join(toks))
    assert 10 not in everything and 11 not in everything and 12 not in everything, "'##', ' ' and '' have no text"
    assert not (set(everything) & v.special_ids)


def test_masked_tile_merge_equals_the_float64_masked_log_softmax():
    """score_util.tile_stats under a set (constraint_util.masked_tile_stats), tiles 64 and 128, float64 and float32 tile
    sums: the merged logsumexp equals the float64 one over the allowed tokens; tiles with no allowed column read
    (-inf, no index, sum exactly 0) and the merge stays finite; sets of 1, 2 and 3 tokens."""
    rs = np.random.RandomState(5)
    x = (rs.standard_normal((8, cu.V)) * 4).astype(np.float32)
    masks = np.ones((8, cu.V), bool)
    masks[1] = rs.rand(cu.V) < 0.5
    masks[2] = cu.mask_of([])                                         # EOS only
    masks[3] = cu.mask_of([4000])                                     # two tokens, two tiles
    masks[4] = cu.mask_of([200, 6100])                                # three
    masks[5, 128:256] = False                                         # one 128-tile = two 64-tiles without a column
    masks[6] = cu.mask_of(range(1000, 1064))                          # one full 64-tile + EOS
    masks[7, np.argmax(x[7])] = False                                 # the free argmax banned
    masks[:, cu.EOS] = True
    ref = cu.masked_log_softmax64(x, masks)
    assert np.isneginf(ref[~masks]).all() and np.isfinite(ref[masks]).all()
    np.testing.assert_allclose(np.exp(ref).sum(-1), 1.0, rtol=1e-12)
    assert ref[2, cu.EOS] == 0.0
    lse_ref = np.where(masks, x.astype(np.float64), -np.inf)
    lse_ref = np.array([su.lse64(r[np.isfinite(r)]) for r in lse_ref])
    for tile in (64, 128):
        for dtype, tol in ((np.float64, 1e-12), (np.float32, 4e-6)):
            m, idx, s = cu.masked_tile_stats(x, masks, tile, dtype)
            empty = ~masks.reshape(8, -1, tile).any(-1)
            assert empty[5].sum() == 128 // tile and empty[2].sum() == cu.V // tile - 1
            assert np.isneginf(m[empty]).all() and (idx[empty] == cu.NO_IDX).all() and (s[empty] == 0).all()
            assert not np.isnan(s).any() and (s[~empty] >= 1).all()
            assert masks[np.arange(8)[:, None], np.where(empty, cu.EOS, idx)].all(), "a tile's winner outside the set"
            got = cu.masked_merge_tiles(m, s)
            assert np.isfinite(got).all()
            np.testing.assert_allclose(got, lse_ref, rtol=0, atol=tol)
            # the row's winner and its score, as the token kernel forms them
            M = m.max(-1)
            win = idx[np.arange(8), np.argmax(m, -1)]
            np.testing.assert_array_equal(win, np.argmax(np.where(masks, x, -np.inf), -1))
            np.testing.assert_allclose(M - got, ref[np.arange(8), win], rtol=0, atol=tol)
    ids, lp = cu.masked_top(x, masks)
    assert (ids[2] == [cu.EOS, -1, -1, -1]).all() and lp[2, 0] == 0 and np.isneginf(lp[2, 1:]).all()
    assert sorted(ids[3, :2]) == [cu.EOS, 4000] and (ids[3, 2:] == -1).all()
    assert sorted(ids[4, :3]) == [cu.EOS, 200, 6100] and ids[4, 3] == -1 and np.isneginf(lp[4, 3])
    assert np.argmax(x[7]) not in ids[7]
    # an exact tie whose lower id is banned resolves to the lowest ALLOWED id
    y = np.zeros((1, cu.V)); y[0, [10, 20, 30]] = 5.0
    mk = np.ones((1, cu.V), bool); mk[0, 10] = False
    assert cu.masked_top(y, mk)[0][0, :2].tolist() == [20, 30]
    # the bit table: bit (v & 31) of word (v >> 5)
    tab = cu.pack_sets(masks)
    assert tab.dtype == np.uint32 and tab.shape == (8, cu.V // 32) and (tab[0] == 0xFFFFFFFF).all()
    assert tab[2].tolist().count(0) == cu.V // 32 - 1 and tab[2, 0] == 1 << cu.EOS
    v = np.arange(cu.V)
    np.testing.assert_array_equal((tab[1][v >> 5] >> (v & 31)) & 1, masks[1])


def test_constraint_symbols_are_exported_declared_and_mirrored(lib):
    hdr = open(os.path.join(ROOT, "include", "mocr.h")).read()
    for name in NEW:
        assert name in _capi.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in mocr.h"
        assert getattr(lib, name) is not None
    for alts, con in [("mocr_recognize_images_alts", "mocr_recognize_images_constrained"),
                      ("mocr_recognize_regions_alts", "mocr_recognize_regions_constrained"),
                      ("mocr_recognize_device_alts", "mocr_recognize_device_constrained"),
                      ("mocr_recognize_gray_host_alts", "mocr_recognize_gray_host_constrained")]:
        a, b = _capi.SYMBOLS[alts][1], _capi.SYMBOLS[con][1]
        assert b == a + [P], con                                   # the _alts twin plus `sets`
    assert _capi.SYMBOLS["mocr_op_dec_token_masked"][1] == _capi.SYMBOLS["mocr_op_dec_token_topk"][1] + [P, P]
    assert _capi.SYMBOLS["mocr_op_gemm_argmax_masked"][1] == _capi.SYMBOLS["mocr_op_gemm_topk"][1] + [P, P, P]
    for macro, val in (("MOCR_MAX_TOKEN_SETS", 256), ("MOCR_TOKEN_SET_ALL", 0)):
        m = re.search(r"#define\s+%s\s+(\d+)\b" % macro, hdr)
        assert m and int(m.group(1)) == val
    assert _capi.MAX_TOKEN_SETS == 256 and _capi.TOKEN_SET_ALL == 0
    # the ABI did not move; null handles are refused before anything is dereferenced
    assert lib.mocr_abi_version() == 2
    assert C.sizeof(_capi.MocrTokenArgs) == 160 and len(_capi.MocrTokenArgs._fields_) == 25
    out = C.c_int32(-5)
    assert lib.mocr_token_set_create(None, None, 1, C.byref(out)) == -1 and out.value == -5
    assert lib.mocr_token_set_count(None) == 0
    assert lib.mocr_recognize_images_constrained(None, None, 1, None, None, None, None, None, None) == -1
    assert lib.mocr_recognize_regions_constrained(None, None, 1, None, 1, None, None, None, None, None, None) == -1
    assert lib.mocr_recognize_device_constrained(None, None, 1, None, None, None, None, None, None) == -1
    assert lib.mocr_recognize_gray_host_constrained(None, None, 1, 8, None, None, None, None, None, None) == -1
    assert lib.mocr_op_gemm_argmax_masked(None, None, None, None, None, None, None, None, None, 1, 128, 64, 64, None, None, None) == -1
    assert lib.mocr_op_dec_token_masked(None, None, None, None, None, None, None, None, None, None) == -1


class _FakeEngine:
    """recognize_images as Engine answers it; logs (crops, kind, token_sets) of each call.  A crop under set h 'decodes'
    to [2, first pixel + 100 h, 3]."""
    L = 6

    def __init__(self):
        self.calls = []

    def recognize_images(self, images, bgr=False, rotate=None, *, scores=False, alternatives=False, **kw):
        assert set(kw) <= {"token_sets"}
        sets = kw.get("token_sets")
        self.calls.append((len(images), 2 if alternatives else 1 if scores else 0, None if sets is None else list(sets), "token_sets" in kw))
        n = len(images)
        ids = np.zeros((n, self.L), np.int32)
        ids[:, 0], ids[:, 2] = 2, 3
        ids[:, 1] = [int(g[0, 0]) + 100 * (sets[i] if sets else 0) for i, g in enumerate(images)]
        lens = np.full(n, 3, np.int32)
        if not (scores or alternatives):
            return ids, lens
        logp = np.zeros((n, self.L), np.float32)
        logp[:, 1:3] = -0.5
        if not alternatives:
            return ids, lens, logp
        alt_ids = np.full((n, self.L, 4), -1, np.int32)
        alt_logp = np.zeros((n, self.L, 4), np.float32)
        alt_ids[:, 1:3, 0] = ids[:, 1:3]
        alt_logp[:, 1:3] = [-0.5, -np.inf, -np.inf, -np.inf]
        return ids, lens, logp, alt_ids, alt_logp


def test_allowed_is_routed_through_the_batcher():
    eng = _FakeEngine()
    b = _Batcher(eng, max_batch=6, timeout_ms=60_000.0)
    try:
        kinds = [0, 1, 2, 0, 2, 1]
        sets = [0, 3, 0, 7, 2, 0]
        futs = [b.submit(np.full((4, 4), 10 + i, np.uint8), scored=k == 1, alternatives=k == 2, token_set=h)
                for i, (k, h) in enumerate(zip(kinds, sets))]
        res = [f.result(timeout=30) for f in futs]
        assert eng.calls == [(6, 2, sets, True)], "one engine call, the richest kind, one handle per crop in queue order"
        for i, (k, h, r) in enumerate(zip(kinds, sets, res)):
            got = r if k == 0 else r[0]
            np.testing.assert_array_equal(got, [2, 10 + i + 100 * h, 3])
            assert (isinstance(r, np.ndarray) if k == 0 else len(r) == (2 if k == 1 else 4))
        # nobody constrained: the calls of before, without the keyword
        for want_kind, flags in ((1, dict(scored=True)), (0, {})):
            futs = [b.submit(np.full((4, 4), 7, np.uint8), **(flags if i == 3 else {})) for i in range(6)]
            [f.result(timeout=30) for f in futs]
            assert eng.calls[-1] == (6, want_kind, None, False)
    finally:
        b.close()


def test_set_handles_and_candidates_skip_missing_entries():
    ts = TokenSet(5, 11)
    assert _set_handles(None, 3) is None
    assert _set_handles(ts, 3) == [5, 5, 5] and _set_handles(2, 2) == [2, 2]
    assert _set_handles([ts, 0, TokenSet(9, 1)], 3) == [5, 0, 9]
    with pytest.raises(ValueError, match="3 crops but 2 token sets"):
        _set_handles([ts, ts], 3)
    v = text.Vocab.synthetic(6144)
    ids = np.array([2, 5, 3, 0], np.int32)
    logp = np.array([0, np.log(0.75), 0, 0], np.float32)
    alt_ids = np.full((4, 4), -1, np.int32)
    alt_logp = np.zeros((4, 4), np.float32)
    alt_ids[1] = [5, 3, -1, -1]; alt_logp[1] = [np.log(0.75), np.log(0.25), -np.inf, -np.inf]
    alt_ids[2] = [3, -1, -1, -1]; alt_logp[2] = [0, -np.inf, -np.inf, -np.inf]
    r = Recognition.from_row(v, ids, logp, 3, alt_ids, alt_logp)
    assert r.candidates(0) == [(v.tokens[5], pytest.approx(0.75)), (v.tokens[3], pytest.approx(0.25))]
    assert r.candidates(1) == [(v.tokens[3], 1.0)]


def test_constraints_refuse_several_devices_without_spawning_workers():
    from manga_ocr.multi import MultiGpuEngine
    eng = object.__new__(MultiGpuEngine)          # no __init__: no child process, no GPU
    with pytest.raises(NotImplementedError, match="several devices"):
        eng.token_set([5, 6])
    with pytest.raises(NotImplementedError, match="several devices"):
        eng.recognize_images([np.zeros((8, 8), np.uint8)], token_sets=[0])
    with pytest.raises(NotImplementedError, match="several devices"):
        eng.recognize_regions([np.zeros((8, 8, 3), np.uint8)], [(0, 0, 0, 4, 4)], token_sets=[0])
    ocr = object.__new__(MangaOcr)
    ocr.engine = eng
    ocr.vocab = text.Vocab.synthetic(6144)
    with pytest.raises(NotImplementedError, match="token constraints.*several devices"):
        ocr.token_set(chars="一")
    for call in (lambda: ocr.recognize_ids([np.zeros((8, 8), np.uint8)], allowed=1),
                 lambda: ocr.recognize_bgr([np.zeros((8, 8, 3), np.uint8)], allowed=[TokenSet(1, 2)]),
                 lambda: ocr.recognize_regions([np.zeros((8, 8, 3), np.uint8)], [(0, 0, 0, 4, 4)], allowed=1)):
        with pytest.raises(NotImplementedError, match="token constraints.*several devices"):
            call()
