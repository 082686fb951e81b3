"""CPU: beam search with token sets and token scores - the float64 reference of the GPU tests (tests/beam_token_util.py)
against transformers' own constrained beam search and transition scores (tests/golden/beam_tok_*.npz, written by
tests/golden/make_beam_token_goldens.py), the margin the fp32 GPU test relies on, the Python surface over a fake library,
and the exported symbols."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import beam_token_util as tu
import beam_util as bu
from manga_ocr import _capi
from manga_ocr.engine import BeamConfig, Engine
from manga_ocr.ocr import MangaOcr, Recognition, TokenSet, _Batcher
from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = ["a", "b", "c", "d", "e"]
ES = {0: False, 1: True, 2: "never"}
NEW_SYMBOLS = ["mocr_recognize_images_beam_tokens", "mocr_recognize_regions_beam_tokens", "mocr_recognize_gray_host_beam_tokens",
               "mocr_recognize_device_beam_tokens", "mocr_op_beam_select_tokens"]


def golden(name):
    g = np.load(os.path.join(GOLD, f"beam_tok_{name}.npz"))
    return {k: g[k] for k in g.files}


def golden_masks(g):
    """bool [n, V]: the crops' sets with EOS added, a row of -1 in the file = no set"""
    m = np.zeros((g["sets"].shape[0], DEFAULT_SPEC.vocab), bool)
    for c, row in enumerate(g["sets"]):
        if (row < 0).all():
            m[c] = True
        else:
            m[c, row[row >= 0]] = True
            m[c, DEFAULT_SPEC.eos_id] = True
    return m


def golden_config(g):
    return bu.Config(int(g["num_beams"]), float(g["length_penalty"]), ES[int(g["early_stopping"])], int(g["no_repeat_ngram_size"]))


@functools.lru_cache(maxsize=None)
def reference(name):
    """beam_token_util's search of case `name` on the golden's crops, weights and sets (computed once, shared)"""
    from test_beam_cpu import _oracle_enc
    g = golden(name)
    o, enc = _oracle_enc(int(g["weights_seed"]), float(g["eos_bias"]), tuple(int(s) for s in g["crop_seeds"]))
    return tu.beam_generate(o, enc, golden_config(g), int(g["max_length"]), golden_masks(g))


@pytest.mark.parametrize("name", CASES)
def test_the_reference_is_transformers_constrained_beam_search(name):
    g = golden(name)
    ids, lens, scores, logp, info = reference(name)
    np.testing.assert_array_equal(lens, g["lens"])
    np.testing.assert_array_equal(ids, g["ids"])
    assert np.abs(scores - g["scores"]).max() <= 1e-4
    assert np.abs(logp - g["logp"]).max() <= 1e-4, "compute_transition_scores(normalize_logits=False)"
    assert (info["min_gap"] >= 1e-3).all(), info["min_gap"]      # the condition the fp32 GPU test relies on


def test_the_goldens_are_the_cases_they_claim():
    for name in CASES:
        g = golden(name)
        masks, K = golden_masks(g), int(g["num_beams"])
        assert 3 <= g["ids"].shape[0] <= 6 and g["ids"].shape[1] == K
        for c in range(g["ids"].shape[0]):
            for j in range(K):
                L = int(g["lens"][c, j])
                assert masks[c, g["ids"][c, j, 1:L]].all(), "every token behind the start token is a member of its crop's set"
                assert g["logp"][c, j, 0] == 0 and (g["logp"][c, j, L:] == 0).all() and (g["logp"][c, j, 1:L] < 0).all()
                if L:       # the identity of include/mocr.h, in the reference's own arithmetic
                    assert abs(float(g["logp"][c, j, 1:L].astype(np.float64).sum()) / float(L - 1) ** float(g["length_penalty"]) - float(g["scores"][c, j])) <= 1e-4
    sizes = {name: [int((r >= 0).sum()) for r in golden(name)["sets"]] for name in CASES}
    assert set(sizes["a"]) == {0} and set(sizes["b"]) == set(sizes["c"]) == {40} and set(sizes["d"]) == {12}
    assert 0 in sizes["e"] and len(set(map(tuple, golden("e")["sets"]))) >= 3, "(e): different sets in one call, one of them ALL"
    assert (int(golden("b")["num_beams"]), int(golden("c")["num_beams"])) == (2, 4) and int(golden("d")["no_repeat_ngram_size"]) == 2
    a = golden("a")
    assert (int(a["num_beams"]), float(a["length_penalty"]), int(a["early_stopping"]), int(a["no_repeat_ngram_size"])) == (4, 2.0, 1, 3)
    # a set changes the search: under the set the hypotheses are not those of the unconstrained search on the same crops
    from test_beam_cpu import _oracle_enc
    g = golden("c")
    o, enc = _oracle_enc(int(g["weights_seed"]), float(g["eos_bias"]), tuple(int(s) for s in g["crop_seeds"]))
    free = tu.beam_generate(o, enc[:1], golden_config(g), int(g["max_length"]))
    assert not np.array_equal(free[0][0], g["ids"][0])


def test_dead_candidates_in_the_reference():
    """a set of one token and EOS at K = 4 with that token banned in three beams: 5 finite scores of 24576, the other winners
    are dead, in the order of their flat index; nothing dead is kept"""
    K, a = 4, 700
    cfg = bu.Config(K, 1.0, False, 2)
    st = tu.State(K, 2)
    st.seqs = [[2, 51, 52, 53]] + [[2, 50, a, 50] for _ in range(K - 1)]
    st.logp = [[0.0, -1.0, -1.0, -1.0] for _ in range(K)]
    st.run = np.array([-1.0, -1.5, -2.0, -2.5])
    logits = np.zeros((K, bu.V))
    mask = np.zeros(bu.V, bool)
    mask[[a, bu.EOS]] = True
    logits[:, a], logits[:, bu.EOS] = 3.0, [2.0, 1.75, 1.5, 1.25]
    cv, cpar, ctok, stop, clp = tu.step(tu.processed(logits, st, cfg, mask), st, cfg, 16)
    assert np.isfinite(cv).sum() == K + 1 and np.isinf(cv[K + 1:]).all() and np.isinf(clp[K + 1:]).all()
    flat = cpar[K + 1:] * bu.V + ctok[K + 1:]
    assert flat.tolist() == [0, 1, 2], "among -inf the lower flat index first"
    assert np.isfinite(st.hyp_score).all() and np.isfinite(st.run).all()
    assert [len(s) for s in st.hyp_seq] == [5, 5, 5, 0] and all(len(lp) == len(s) for lp, s in zip(st.hyp_logp, st.hyp_seq))
    assert st.run[0] == cv[0] and (st.run[1:] < -1e8).all(), "the stopped candidates' - 1e9 outranks the dead ones"


# ------------------------------------------------------------------------------------------------ the Python surface
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


def _ints(p, n):
    return np.ctypeslib.as_array((C.c_int32 * n).from_address(p.value)).tolist()


def test_beam_scores_and_sets_go_to_the_tokens_symbol(eng):
    beam = BeamConfig(3, 2.0, True, 3)
    L = DEFAULT_SPEC.max_len
    crops = [np.zeros((8, 9), np.uint8)] * 4
    page = [np.zeros((32, 48, 3), np.uint8)]
    regs = [(0, 1, 2, 8, 8)] * 4
    # token scores: a fourth block, out_logp set and sets null
    out = eng.recognize_images(crops, beam=beam, beam_scores=True)
    assert [a.shape for a in out] == [(4, 3, L), (4, 3), (4, 3), (4, 3, L)] and [a.dtype for a in out] == [np.int32, np.int32, np.float32, np.float32]
    assert (out[3] == 0).all()
    name, args = eng.lib.calls[-1]
    assert name == "mocr_recognize_images_beam_tokens" and len(args) == 9
    assert args[-2].value == out[3].ctypes.data and args[-1].value is None and args[-3].value == out[2].ctypes.data
    # one set for all crops: three blocks, out_logp null and sets [4]
    out = eng.recognize_regions(page, regs, beam=beam, beam_sets=5)
    assert [a.shape for a in out] == [(4, 3, L), (4, 3), (4, 3)]
    name, args = eng.lib.calls[-1]
    assert name == "mocr_recognize_regions_beam_tokens" and len(args) == 11 and args[-2].value is None and _ints(args[-1], 4) == [5] * 4
    # one set per crop, with the scores
    out = eng.recognize_gray(np.zeros((4, 224, 224), np.uint8), max_len=8, beam=beam, beam_scores=True, beam_sets=[1, 0, 2, 0])
    assert len(out) == 4 and out[3].shape == (4, 3, L)
    name, args = eng.lib.calls[-1]
    assert name == "mocr_recognize_gray_host_beam_tokens" and len(args) == 10 and args[3] == 8
    assert args[-2].value == out[3].ctypes.data and _ints(args[-1], 4) == [1, 0, 2, 0]
    # the device twin: buffers in, nothing out
    assert eng.recognize_device(0x1000, 4, 0x2000, 0x3000, beam=beam, d_out_score=0x4000, d_out_beam_logp=0x5000, beam_sets=[3, 3, 0, 1]) is None
    name, args = eng.lib.calls[-1]
    assert name == "mocr_recognize_device_beam_tokens" and [p.value for p in args[-5:-1]] == [0x2000, 0x3000, 0x4000, 0x5000]
    assert _ints(args[-1], 4) == [3, 3, 0, 1]
    assert eng.recognize_device(0x1000, 4, 0x2000, 0x3000, beam=beam, d_out_score=0x4000, beam_sets=2) is None
    assert eng.lib.calls[-1][0] == "mocr_recognize_device_beam_tokens" and eng.lib.calls[-1][1][-2].value is None
    # without either keyword every call is the one it was
    eng.lib.calls.clear()
    assert len(eng.recognize_images(crops, beam=beam)) == 3 and len(eng.recognize_images(crops, beam=beam, beam_scores=False, beam_sets=None)) == 3
    eng.recognize_device(0x1000, 4, 0x2000, 0x3000, beam=beam, d_out_score=0x4000)
    assert [n for n, _ in eng.lib.calls] == ["mocr_recognize_images_beam"] * 2 + ["mocr_recognize_device_beam"]
    # no crops: the shapes, no call
    eng.lib.calls.clear()
    out = eng.recognize_images([], beam=beam, beam_scores=True)
    assert [a.shape for a in out] == [(0, 3, L), (0, 3), (0, 3), (0, 3, L)] and eng.lib.calls == []


def test_what_is_refused_before_any_call(eng):
    beam = BeamConfig(2)
    crops = [np.zeros((8, 9), np.uint8)] * 3
    gray = np.zeros((3, 224, 224), np.uint8)
    for call in (lambda: eng.recognize_images(crops, beam_scores=True), lambda: eng.recognize_images(crops, beam_sets=1),
                 lambda: eng.recognize_regions([np.zeros((32, 48, 3), np.uint8)], [(0, 1, 2, 8, 8)], beam_sets=[1]),
                 lambda: eng.recognize_gray(gray, beam_scores=True, scores=True),
                 lambda: eng.recognize_device(0x1000, 3, 0x2000, 0x3000, d_out_beam_logp=0x5000),
                 lambda: eng.recognize_device(0x1000, 3, 0x2000, 0x3000, beam_sets=[0, 1, 2])):
        with pytest.raises(ValueError, match="beam="):
            call()
    with pytest.raises(ValueError, match="3 crops but 2 set handles"):
        eng.recognize_images(crops, beam=beam, beam_sets=[1, 2])
    # the greedy keywords stay refused with beam=, the new ones do not lift that
    with pytest.raises(ValueError, match="does not combine with scores"):
        eng.recognize_images(crops, beam=beam, scores=True, beam_scores=True)
    with pytest.raises(ValueError, match="does not combine with token_sets"):
        eng.recognize_gray(gray, beam=beam, token_sets=1, beam_sets=1)
    with pytest.raises(ValueError, match="max_batch"):
        eng.recognize_images([crops[0]] * 9, beam=beam, beam_scores=True)
    assert eng.lib.calls == []


class _FakeEngine:
    """recognize_images as Engine answers a beam call; logs (crops, keywords) of each call"""
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
        out = (ids, lens, np.full((n, K), -0.5, np.float32))
        if kw.get("beam_scores"):
            logp = np.zeros((n, K, self.L), np.float32)
            logp[:, :, 1], logp[:, :, 2] = -0.25, -0.75
            out += (logp,)
        return out


def test_the_batcher_carries_scores_and_sets_per_crop():
    fe = _FakeEngine()
    b = _Batcher(fe, max_batch=8, timeout_ms=200.0)
    try:
        gray = np.zeros((4, 4), np.uint8)
        beam4, beam2 = BeamConfig(4), BeamConfig(2)
        futs = [b.submit(gray, beam=beam4), b.submit(gray, beam=beam4, beam_scores=True), b.submit(gray, beam=beam2, beam_set=7),
                b.submit(gray, beam=beam2), b.submit(gray, beam=beam4)]
        res = [f.result(timeout=10) for f in futs]
    finally:
        b.close()
    assert [len(r) for r in res] == [3, 4, 3, 3, 3], "only the caller that asked gets its logp"
    assert res[1][3].shape == (4, 6) and res[1][3][0, 1] == np.float32(-0.25)
    for n, kw in fe.calls:
        assert set(kw) <= {"beam", "beam_scores", "beam_sets"} and n <= 8 // kw["beam"].num_beams
        if "beam_sets" in kw:
            assert kw["beam"] == beam2 and len(kw["beam_sets"]) == n and 7 in kw["beam_sets"]
    assert any("beam_scores" in kw for _, kw in fe.calls) and any(set(kw) == {"beam"} for _, kw in fe.calls)
    assert all(kw["beam"] == beam4 for _, kw in fe.calls if "beam_scores" in kw), "requests of different configurations never merge"


class _Vocab:
    tokens = [f"[{i}]" for i in range(64)]
    special = set()

    def __len__(self):
        return len(self.tokens)


def _ocr(engine, max_batch=4):
    ocr = object.__new__(MangaOcr)
    ocr.engine, ocr.spec, ocr.max_batch, ocr.beam = engine, DEFAULT_SPEC, max_batch, None
    ocr.vocab = _Vocab()
    return ocr


def test_hypotheses_carry_token_logp_of_their_own_length(monkeypatch):
    import manga_ocr.ocr as ocr_mod
    monkeypatch.setattr(ocr_mod, "ids_to_text", lambda vocab, ids: " ".join(str(int(i)) for i in ids))
    monkeypatch.setattr(ocr_mod, "to_pixels", lambda im: im)
    fe = _FakeEngine()
    ocr = _ocr(fe)
    imgs = [np.zeros((8, 8), np.uint8)] * 3
    ts = TokenSet(5, 12)
    hyps = ocr.recognize_batch_beam(imgs, 2, token_scores=True, allowed=ts)
    assert [kw for _, kw in fe.calls] == [dict(beam=BeamConfig(2), beam_scores=True, beam_sets=[5, 5]), dict(beam=BeamConfig(2), beam_scores=True, beam_sets=[5])]
    assert [len(h) for h in hyps] == [1, 1, 1], "the empty slot is dropped"
    for h in (x[0] for x in hyps):
        assert isinstance(h, Recognition) and len(h.logprobs) == len(h.ids) - 1 == 2 and len(h.token_logp) == len(h.ids)
        assert h.token_logp.tolist() == [0.0, -0.25, -0.75]
        assert h.logprobs.tolist() == [-0.25, -0.75] and h.sequence_score == -0.5
        assert h.confidence == pytest.approx(np.exp(-0.5)) and h.min_prob == pytest.approx(np.exp(-0.75))
    # one set per crop; a wrong number of them is refused before any call; nobody asking makes the plain beam call
    fe.calls.clear()
    ocr.recognize_batch_beam(imgs, 2, allowed=[ts, TokenSet(0, 64), TokenSet(9, 3)])
    assert [kw for _, kw in fe.calls] == [dict(beam=BeamConfig(2), beam_sets=[5, 0]), dict(beam=BeamConfig(2), beam_sets=[9])]
    fe.calls.clear()
    with pytest.raises(ValueError, match="3 crops but 2 token sets"):
        ocr.recognize_batch_beam(imgs, 2, allowed=[ts, ts])
    with pytest.raises(TypeError):
        ocr.recognize_batch_beam(imgs, 2, 1.0, False, 0, True)         # keyword-only
    assert fe.calls == []
    plain = ocr.recognize_batch_beam(imgs, 2)
    assert [kw for _, kw in fe.calls] == [dict(beam=BeamConfig(2))] * 2
    assert all(len(h[0].logprobs) == 0 and h[0].confidence == 0.0 and h[0].sequence_score == -0.5 for h in plain)
    assert all(len(h[0].token_logp) == 1 for h in plain), "a plain hypothesis carries no token scores (its start token's 0 alone)"


def test_several_devices_refuse_through_no_beam():
    from manga_ocr.multi import MultiGpuEngine
    ocr = _ocr(object.__new__(MultiGpuEngine))
    with pytest.raises(NotImplementedError):
        ocr.recognize_bgr_beam([np.zeros((8, 8, 3), np.uint8)], None, 2, token_scores=True, allowed=TokenSet(1, 3))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mocr.h")).read()
    for sym in NEW_SYMBOLS + ["mocr_beam_token_state_bytes"]:
        assert re.search(r"\b" + sym + r"\s*\(", header), f"{sym} is not declared in include/mocr.h"
        assert sym in _capi.SYMBOLS, f"{sym} has no ctypes signature"
    for kind in ("images", "regions", "gray_host", "device"):
        plain, tok = _capi.SYMBOLS[f"mocr_recognize_{kind}_beam"], _capi.SYMBOLS[f"mocr_recognize_{kind}_beam_tokens"]
        assert tok[0] is plain[0] and tok[1][:len(plain[1])] == plain[1] and len(tok[1]) == len(plain[1]) + 2, "the _beam twin plus (out_logp, sets)"
    assert len(_capi.SYMBOLS["mocr_op_beam_select_tokens"][1]) == len(_capi.SYMBOLS["mocr_op_beam_select"][1]) + 4
    assert "no token sets" not in header and "renormalis" in header.split("mocr_recognize_images_beam_tokens")[0].split("beam search")[-1]
    import __graft_entry__ as entry
    entry.build()
    lib = _capi.load_library()
    for sym in NEW_SYMBOLS + ["mocr_beam_token_state_bytes"]:
        assert getattr(lib, sym) is not None, f"{sym} is not exported"
    assert lib.mocr_abi_version() == 2
