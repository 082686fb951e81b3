"""CPU: token positions for beam-search hypotheses (include/mocr.h, "beam search with token positions") - the numpy restatement
of the beam-index trail (tests/beam_position_util.py) against replay, the precondition the GPU tests rely on (the inputs tell a
dropped trail from a kept one), the Python surface over a fake library and a stub engine, and the exported symbols."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import beam_position_util as bp
import beam_token_util as tu
import beam_util as bu
import position_util as pu
from manga_ocr import _capi
from manga_ocr.engine import BeamConfig, Engine
from manga_ocr.ocr import MangaOcr, Recognition, TokenSet, _Batcher
from manga_ocr.weights import DEFAULT_SPEC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16_CXY_TOL = 2.2e-2        # tests/test_gpu_positions.py (a GPU module: not imported here)
NEW_SYMBOLS = ["mocr_recognize_images_beam_positions", "mocr_recognize_regions_beam_positions", "mocr_recognize_gray_host_beam_positions",
               "mocr_recognize_device_beam_positions", "mocr_op_beam_select_positions", "mocr_op_attn_positions_gathered",
               "mocr_beam_position_state_bytes"]


# ------------------------------------------------------------------------------------------------ (a) the trail's bookkeeping
def _random_search(seed, K, max_len, steps, eos_every, base):
    """a search on random logits (a few strong tokens per beam, EOS among them every `eos_every` steps) with the trails and
    the recorder -> (state, trails, hist)"""
    rs = np.random.RandomState(seed)
    cfg = bu.Config(K, 1.0, False, 0)
    st = (tu.State if base is tu.step else bu.State)(K, 2)
    tr, rec = bp.Trails(K), bp.Recorder()
    for s in range(steps):
        if st.done:
            break
        rec.record(st)
        logits = rs.standard_normal((K, bu.V)) * 0.1
        for k in range(K):
            logits[k, rs.randint(5, bu.V, size=3)] += rs.uniform(2.0, 6.0, size=3)
        if s % eos_every == eos_every - 1:
            logits[rs.randint(0, K), bu.EOS] += 7.0
        acc = tu.processed(logits, st, cfg) if base is tu.step else bu.accumulate(logits, st, cfg)
        bp.step(acc, st, tr, cfg, max_len, bu.EOS, base=base)
    return st, tr, rec.hist


@pytest.mark.parametrize("base", [bu.step, tu.step], ids=["beam_util.step", "beam_token_util.step"])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_the_trail_replays_every_hypothesis(K, base):
    """random searches: the running beams' trails and the finished set's replay to their histories at every step count, the
    beams change rows (a trail that is not constant) and hypotheses are inserted ahead of existing ones"""
    moved = inserted = finished = 0
    for seed in range(6):
        for steps in (1, 2, 5, 11):
            st, tr, hist = _random_search(100 * K + seed, K, 12, steps, 3, base)
            hist = hist + [[list(s) for s in st.seqs]]
            for k in range(K):
                if not st.done:      # (a crop that ended keeps the candidates of its last step as "beams": nothing reads them)
                    assert bp.replay(st.seqs[k], tr.trail[k], hist), (seed, steps, k)
                    moved += len(set(tr.trail[k][1:])) > 1
            for j in range(K):
                assert len(tr.hyp_trail[j]) == len(st.hyp_seq[j])
                if st.hyp_seq[j]:
                    finished += 1
                    assert tr.hyp_trail[j][0] == 0 and all(0 <= b < K for b in tr.hyp_trail[j])
                    assert bp.replay(st.hyp_seq[j], tr.hyp_trail[j], hist), (seed, steps, j)
            lens = [len(h) for h in st.hyp_seq if h]
            inserted += any(a > b for a, b in zip(lens, lens[1:]))          # a later (longer) hypothesis ranks ahead of an earlier one
    assert moved > 0 and inserted > 0 and finished > 10


def test_a_wrong_trail_does_not_replay():
    st, tr, hist = _random_search(7, 4, 12, 11, 3, bu.step)
    j = next(j for j in range(4) if len(st.hyp_seq[j]) > 3 and len(set(tr.hyp_trail[j][1:])) > 1)
    good = tr.hyp_trail[j]
    assert bp.replay(st.hyp_seq[j], good, hist)
    assert not bp.replay(st.hyp_seq[j], [0] + [j] * (len(good) - 1), hist), "the hypothesis' own slot is not its trail"
    assert not bp.replay(st.hyp_seq[j], good[:-1], hist)


# ------------------------------------------------------------------------------------------------ (b) the inputs' precondition
@functools.lru_cache(maxsize=None)
def _reference():
    from gpu_util import crops
    from oracle.mocr_oracle import Oracle
    o = Oracle(pu.pos_weights(bp.G, bp.EOS_BIAS, bp.WEIGHT_SEED), DEFAULT_SPEC)
    enc = o.encode(o.preprocess_gray(crops(bp.CROP_SEED, 6)))
    return (o, enc) + bp.beam_generate(o, enc, bu.Config(*bp.PUBLISHED), bp.MAX_LEN)


def test_the_reference_search_replays():
    o, enc, ids, lens, scores, trails, info = _reference()
    plain = bu.beam_generate(o, enc[:2], bu.Config(*bp.PUBLISHED), bp.MAX_LEN)
    np.testing.assert_array_equal(plain[0], ids[:2])          # the wrapper moves nothing of the search
    np.testing.assert_array_equal(plain[1], lens[:2])
    for c in range(6):
        for j in range(4):
            L = int(lens[c, j])
            assert (trails[c, j, L:] == 0).all() and trails[c, j, 0] == 0
            if L:
                assert bp.replay(ids[c, j, :L].tolist(), trails[c, j, :L].tolist(), info["hist"][c])


def test_the_inputs_tell_a_dropped_trail():
    """The published configuration at max_len 24 on the position tests' weights and crops: hypotheses with a trail that is not
    constant exist, and for one of them the float64 fields taken from the hypothesis' OWN row's recordings (the trail
    dropped) leave the correct ones by more than 10 x BF16_CXY_TOL in cx or cy - so the GPU tests, whose widest bound is
    2 x BF16_CXY_TOL, cannot pass with the trail dropped.  Measured: all 24 hypotheses change rows; the largest
    difference per hypothesis is 0.13 .. 0.31."""
    o, enc, ids, lens, scores, trails, info = _reference()
    ref = bp.reference_fields(o, enc, ids, lens)
    changing = [(c, j) for c in range(6) for j in range(4) if lens[c, j] > 1 and len(set(trails[c, j, 1:lens[c, j]].tolist())) > 1]
    assert changing, "no returned hypothesis changes rows: pick another weight seed or eos_bias (beam_position_util)"
    worst = 0.0
    for c, j in changing[:8]:
        L = int(lens[c, j])
        own = bp.own_row_fields(o, enc[c:c + 1], j, L, info["hist"][c])
        worst = max(worst, float(np.abs(own[1:L, :2] - ref[c, j, 1:L, :2]).max()))
        same = [t for t in range(1, L) if info["hist"][c][t - 1][j] == ids[c, j, :t].tolist()]
        assert np.abs(own[same] - ref[c, j][same]).max() <= 1e-9, "where the row held the hypothesis' own history the two agree"
    print(f"dropped trail: {len(changing)} hypotheses change rows; cx / cy move by up to {worst:.3f} (needed > {10 * BF16_CXY_TOL:.3f})")
    assert worst > 10 * BF16_CXY_TOL


# ------------------------------------------------------------------------------------------------ (c) the Python surface
class _FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("mocr_"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or _capi.MOCR_OK


@pytest.fixture
def eng():
    e = object.__new__(Engine)          # no __init__: no library, no GPU
    e.lib, e.spec, e._h, e.max_batch = _FakeLib(), DEFAULT_SPEC, C.c_void_p(0), 16
    return e


def test_beam_positions_go_to_the_positions_symbol(eng):
    beam = BeamConfig(3, 2.0, True, 3)
    L = DEFAULT_SPEC.max_len
    crops = [np.zeros((8, 9), np.uint8)] * 4
    # positions alone: a fourth block, out_logp and sets null
    out = eng.recognize_images(crops, beam=beam, beam_positions=True)
    assert [a.shape for a in out] == [(4, 3, L), (4, 3), (4, 3), (4, 3, L, 5)] and out[3].dtype == np.float32 and (out[3] == 0).all()
    name, args = eng.lib.calls[-1]
    assert name == "mocr_recognize_images_beam_positions" and len(args) == 10
    assert args[-1].value == out[3].ctypes.data and args[-2].value is None and args[-3].value is None
    # with token scores and sets: logp fourth, pos LAST
    out = eng.recognize_regions([np.zeros((32, 48, 3), np.uint8)], [(0, 1, 2, 8, 8)] * 4, beam=beam, beam_scores=True, beam_sets=5, beam_positions=True)
    assert [a.shape for a in out] == [(4, 3, L), (4, 3), (4, 3), (4, 3, L), (4, 3, L, 5)]
    name, args = eng.lib.calls[-1]
    assert name == "mocr_recognize_regions_beam_positions" and len(args) == 12
    assert args[-1].value == out[4].ctypes.data and args[-3].value == out[3].ctypes.data
    out = eng.recognize_gray(np.zeros((4, 224, 224), np.uint8), max_len=8, beam=beam, beam_positions=True, beam_sets=[1, 0, 2, 0])
    assert len(out) == 4 and out[3].shape == (4, 3, L, 5)
    name, args = eng.lib.calls[-1]
    assert name == "mocr_recognize_gray_host_beam_positions" and len(args) == 11 and args[3] == 8 and args[-3].value is None
    # the device twin: buffers in, nothing out
    assert eng.recognize_device(0x1000, 4, 0x2000, 0x3000, beam=beam, d_out_score=0x4000, d_out_beam_pos=0x6000) is None
    name, args = eng.lib.calls[-1]
    assert name == "mocr_recognize_device_beam_positions" and [p.value for p in args[-6:]] == [0x2000, 0x3000, 0x4000, None, None, 0x6000]
    eng.recognize_device(0x1000, 4, 0x2000, 0x3000, beam=beam, d_out_score=0x4000, d_out_beam_logp=0x5000, d_out_beam_pos=0x6000)
    assert [p.value for p in eng.lib.calls[-1][1][-3:]] == [0x5000, None, 0x6000]
    # without the keyword every call is the one it was
    eng.lib.calls.clear()
    assert len(eng.recognize_images(crops, beam=beam)) == 3 and len(eng.recognize_images(crops, beam=beam, beam_scores=True, beam_positions=False)) == 4
    eng.recognize_device(0x1000, 4, 0x2000, 0x3000, beam=beam, d_out_score=0x4000)
    assert [n for n, _ in eng.lib.calls] == ["mocr_recognize_images_beam", "mocr_recognize_images_beam_tokens", "mocr_recognize_device_beam"]
    # no crops: the shapes, no call
    eng.lib.calls.clear()
    out = eng.recognize_images([], beam=beam, beam_positions=True)
    assert [a.shape for a in out] == [(0, 3, L), (0, 3), (0, 3), (0, 3, L, 5)] and eng.lib.calls == []


def test_what_is_refused_before_any_call(eng):
    beam = BeamConfig(2)
    crops = [np.zeros((8, 9), np.uint8)] * 3
    for call in (lambda: eng.recognize_images(crops, beam_positions=True),
                 lambda: eng.recognize_gray(np.zeros((3, 224, 224), np.uint8), beam_positions=True, positions=True),
                 lambda: eng.recognize_device(0x1000, 3, 0x2000, 0x3000, d_out_beam_pos=0x6000)):
        with pytest.raises(ValueError, match="beam="):
            call()
    # the greedy keyword stays refused with beam=
    with pytest.raises(ValueError, match="does not combine with positions"):
        eng.recognize_images(crops, beam=beam, positions=True, beam_positions=True)
    with pytest.raises(ValueError, match="3 crops but 2 set handles"):
        eng.recognize_images(crops, beam=beam, beam_positions=True, beam_sets=[1, 2])
    with pytest.raises(ValueError, match="max_batch"):
        eng.recognize_images([crops[0]] * 9, beam=beam, beam_positions=True)
    assert eng.lib.calls == []


class _FakeEngine:
    """recognize_images / recognize_regions as Engine answers a beam call; logs (crops, keywords) of each call"""
    L = 6

    def __init__(self):
        self.calls = []

    def recognize_images(self, images, bgr=False, rotate=None, **kw):
        self.calls.append((len(images), dict(kw)))
        n, K = len(images), kw["beam"].num_beams
        ids = np.zeros((n, K, self.L), np.int32)
        ids[:, :, 0], ids[:, :, 1], ids[:, :, 2] = 2, 10 + np.arange(n)[:, None], 3
        lens = np.full((n, K), 3, np.int32)
        lens[:, K - 1] = 0                              # the last slot is empty
        out = (ids, lens, np.full((n, K), -0.5, np.float32) - 0.125 * np.arange(K, dtype=np.float32))
        if kw.get("beam_scores"):
            logp = np.zeros((n, K, self.L), np.float32)
            logp[:, :, 1], logp[:, :, 2] = -0.25, -0.75
            out += (logp,)
        if kw.get("beam_positions"):
            pos = np.zeros((n, K, self.L, 5), np.float32)
            pos[:, :, 1:3] = [0.25, 0.75, 0.05, 0.1, 0.9]
            pos[:, :, 1:3, 0] += 0.01 * np.arange(K, dtype=np.float32)[None, :, None]
            out += (pos,)
        return out

    def recognize_regions(self, pages, regions, bgr=True, **kw):
        out = self.recognize_images(list(regions), **kw)
        out[1][[i for i, r in enumerate(regions) if r[3] == 0]] = 0      # an empty region is a sliver: no hypotheses
        return out


def test_the_batcher_carries_positions_per_crop():
    fe = _FakeEngine()
    b = _Batcher(fe, max_batch=8, timeout_ms=200.0)
    try:
        gray = np.zeros((4, 4), np.uint8)
        beam4, beam2 = BeamConfig(4), BeamConfig(2)
        futs = [b.submit(gray, beam=beam4), b.submit(gray, beam=beam4, beam_positions=True), b.submit(gray, beam=beam2, beam_scores=True, beam_positions=True),
                b.submit(gray, beam=beam2), b.submit(gray, beam=beam4, beam_scores=True)]
        res = [f.result(timeout=10) for f in futs]
    finally:
        b.close()
    assert [len(r) for r in res] == [3, 4, 5, 3, 4], "only the caller that asked gets its positions, last"
    assert res[1][3].shape == (4, 6, 5) and res[2][4].shape == (2, 6, 5) and res[2][3].shape == (2, 6) and res[4][3].shape == (4, 6)
    for n, kw in fe.calls:
        assert set(kw) <= {"beam", "beam_scores", "beam_positions"} and n <= 8 // kw["beam"].num_beams
    assert any("beam_positions" in kw for _, kw in fe.calls)


class _Vocab:
    tokens = [f"[{i}]" for i in range(64)]
    special = set()

    def __len__(self):
        return len(self.tokens)


def _ocr(engine, max_batch=4, beam=None):
    ocr = object.__new__(MangaOcr)
    ocr.engine, ocr.spec, ocr.max_batch, ocr.beam = engine, DEFAULT_SPEC, max_batch, beam
    ocr.beam_positions = beam is not None           # as MangaOcr.__init__ sets it
    ocr.vocab = _Vocab()
    return ocr


@pytest.fixture
def plain_text(monkeypatch):
    import manga_ocr.ocr as ocr_mod
    monkeypatch.setattr(ocr_mod, "ids_to_text", lambda vocab, ids: " ".join(str(int(i)) for i in ids))
    monkeypatch.setattr(ocr_mod, "to_pixels", lambda im: im)


def test_hypotheses_carry_positions_of_their_own_length(plain_text):
    fe = _FakeEngine()
    ocr = _ocr(fe)
    imgs = [np.zeros((8, 8), np.uint8)] * 3
    hyps = ocr.recognize_batch_beam(imgs, 2, positions=True)
    assert [kw for _, kw in fe.calls] == [dict(beam=BeamConfig(2), beam_positions=True)] * 2
    assert [len(h) for h in hyps] == [1, 1, 1], "the empty slot is dropped"
    for h in (x[0] for x in hyps):
        assert isinstance(h, Recognition) and h.positions.shape == (3, 5) and h.positions.dtype == np.float32 and h.rect is None
        assert (h.positions[0] == 0).all() and h.positions[1].tolist() == pytest.approx([0.25, 0.75, 0.05, 0.1, 0.9])
        assert len(h.logprobs) == 0 and h.sequence_score == -0.5
        b = h.boxes(100, 50)
        assert b.shape == (3, 4) and (b[0] == 0).all() and b[1].tolist() == pytest.approx([15.0, 27.5, 35.0, 47.5])
    # with token scores: both, through from_row
    fe.calls.clear()
    hyps = ocr.recognize_batch_beam(imgs[:1], 3, token_scores=True, allowed=TokenSet(5, 12), positions=True)
    assert [kw for _, kw in fe.calls] == [dict(beam=BeamConfig(3), beam_scores=True, beam_positions=True, beam_sets=[5])]
    assert [h.positions.shape for h in hyps[0]] == [(3, 5)] * 2 and hyps[0][1].positions[1, 0] == pytest.approx(0.26)
    assert hyps[0][0].logprobs.tolist() == [-0.25, -0.75]
    # regions: every hypothesis carries its region's rect, a sliver has none
    fe.calls.clear()
    page = np.zeros((100, 200, 3), np.uint8)
    regs = [(0, 10, 10, 50, 40), (0, 100, 20, 40, 40), (0, 0, 0, 0, 0)]
    hyps = ocr.recognize_regions_beam([page], regs, 2, positions=True)
    assert [len(h) for h in hyps] == [1, 1, 0]
    from manga_ocr.regions import padded_rect
    for h, r in zip(hyps[:2], regs):
        assert h[0].rect == tuple(padded_rect(r[1:], 100, 200)) and h[0].page_boxes().shape == (3, 4)
        assert (h[0].page_boxes()[1, :2] >= np.array(h[0].rect[:2])).all()
    # nobody asking makes the call it always made, and the hypotheses carry no positions
    fe.calls.clear()
    plain = ocr.recognize_batch_beam(imgs, 2)
    assert [kw for _, kw in fe.calls] == [dict(beam=BeamConfig(2))] * 2 and all(h[0].positions is None for h in plain)
    with pytest.raises(ValueError, match="no positions"):
        plain[0][0].boxes(10, 10)
    with pytest.raises(TypeError):
        ocr.recognize_batch_beam(imgs, 2, 1.0, False, 0, False, None, True)         # keyword-only


def test_positions_methods_of_a_beam_manga_ocr_return_the_best_hypothesis(plain_text):
    fe = _FakeEngine()
    ocr = _ocr(fe, beam=BeamConfig(4, 2.0, True, 3))
    imgs = [np.zeros((8, 8), np.uint8)] * 2
    recs = ocr.recognize_batch_positions(imgs)
    assert [kw for _, kw in fe.calls] == [dict(beam=BeamConfig(4, 2.0, True, 3), beam_scores=True, beam_positions=True)] * 2
    for i, r in enumerate(recs):
        assert r.text == "2 10 3" and r.sequence_score == -0.5 and r.positions.shape == (3, 5)
        assert r.logprobs.tolist() == [-0.25, -0.75] and r.positions[1, 0] == pytest.approx(0.25), "hypothesis 0, the best"
        assert r.boxes(10, 10).shape == (3, 4)
    # regions: rect, and a sliver gives what the greedy method gives
    regs = [(0, 10, 10, 50, 40), (0, 0, 0, 0, 0)]
    recs = ocr.recognize_regions_positions([np.zeros((100, 200, 3), np.uint8)], regs)
    assert recs[0].rect is not None and recs[0].page_boxes().shape == (3, 4)
    assert recs[1].text == "" and len(recs[1].ids) == 0 and recs[1].positions.shape == (0, 5) and recs[1].rect is None
    # the per-call keywords stay refused, as for the plain methods
    ts = TokenSet(5, 12)
    for kw in (dict(allowed=ts), dict(no_repeat_ngram=2), dict(prefix=[5, 6])):
        with pytest.raises(ValueError, match="do not combine"):
            ocr.recognize_batch_positions(imgs, **kw)
        with pytest.raises(ValueError, match="do not combine"):
            ocr.recognize_bgr_positions([np.zeros((8, 8, 3), np.uint8)], **kw)
    # a greedy MangaOcr is untouched: its positions methods make the greedy call
    class _Greedy:
        def __init__(self):
            self.calls = []

        def recognize_images(self, images, bgr=False, rotate=None, **kw):
            self.calls.append(dict(kw))
            n = len(images)
            return np.zeros((n, 6), np.int32), np.zeros(n, np.int32), np.zeros((n, 6), np.float32), np.zeros((n, 6, 5), np.float32)
    g = _Greedy()
    _ocr(g).recognize_batch_positions(imgs)
    assert g.calls == [dict(scores=True, positions=True)]
    # the switch is the constructor's ``beam_positions``: an instance that holds ``beam`` alone (tests/golden/surface.json
    # records such instances) keeps its greedy positions rows, while its plain methods decode with the beams
    g = _Greedy()
    half = _ocr(g, beam=BeamConfig(2))
    del half.beam_positions
    half.recognize_batch_positions(imgs)
    assert g.calls == [dict(scores=True, positions=True)]


def test_require_beam_positions(plain_text):
    from manga_ocr.multi import MultiGpuEngine
    assert "positions" in MultiGpuEngine.NO_BEAM_POSITIONS

    class _Refuses:
        NO_BEAM_POSITIONS = "no beam positions here"
    ocr = _ocr(_Refuses(), beam=BeamConfig(2))
    with pytest.raises(NotImplementedError, match="no beam positions here"):
        ocr._require("BEAM_POSITIONS")
    with pytest.raises(NotImplementedError, match="no beam positions here"):
        ocr.recognize_batch_beam([np.zeros((8, 8), np.uint8)], 2, positions=True)
    with pytest.raises(NotImplementedError, match="no beam positions here"):
        ocr.recognize_batch_positions([np.zeros((8, 8), np.uint8)])
    multi = _ocr(object.__new__(MultiGpuEngine))
    with pytest.raises(NotImplementedError):
        multi.recognize_bgr_beam([np.zeros((8, 8, 3), np.uint8)], None, 2, positions=True)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mocr.h")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\s*\(", header), f"{sym} is not declared in include/mocr.h"
        assert sym in _capi.SYMBOLS, f"{sym} has no ctypes signature"
    for kind in ("images", "regions", "gray_host", "device"):
        tok, pos = _capi.SYMBOLS[f"mocr_recognize_{kind}_beam_tokens"], _capi.SYMBOLS[f"mocr_recognize_{kind}_beam_positions"]
        assert pos[0] is tok[0] and pos[1][:len(tok[1])] == tok[1] and len(pos[1]) == len(tok[1]) + 1, "the _beam_tokens twin plus out_pos"
    assert len(_capi.SYMBOLS["mocr_op_beam_select_positions"][1]) == len(_capi.SYMBOLS["mocr_op_beam_select_tokens"][1]) + 2
    assert len(_capi.SYMBOLS["mocr_op_attn_positions_gathered"][1]) == len(_capi.SYMBOLS["mocr_op_attn_positions"][1]) + 3
    assert "carries no prefixes, positions" not in header and "decode with the beams too" in MangaOcr.__init__.__doc__
    import __graft_entry__ as entry
    entry.build()
    lib = _capi.load_library()
    for sym in NEW_SYMBOLS:
        assert getattr(lib, sym) is not None, f"{sym} is not exported"
    assert lib.mocr_abi_version() == 2
