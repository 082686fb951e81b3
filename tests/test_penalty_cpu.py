"""CPU: the repetition penalty's host side - the reference rule (penalty_util) against transformers'
RepetitionPenaltyLogitsProcessor and against the goldens of tests/golden/make_penalty_goldens.py (transformers' generate under
the penalty alone, with no_repeat_ngram_size=2 and with a sequence_bias: the order of the processors), argument validation, the
travel of ``repetition_penalty=`` through the batcher and the request path on fake engines, the beam refusals, the resolution
of ``MangaOcr(repetition_penalty="checkpoint")``, and the library's new exports."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import bias_util as bu
import constraint_util as cu
import penalty_util as pu
from manga_ocr import _capi, text
from manga_ocr.engine import BeamConfig, Engine
from manga_ocr.ocr import MangaOcr, _Batcher, _penalties, resolve_repetition_penalty
from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
V, EOS, START = 6144, 3, 2
P = C.c_void_p
NEW = ["mocr_recognize_images_penalty", "mocr_recognize_regions_penalty", "mocr_recognize_device_penalty",
       "mocr_recognize_gray_host_penalty", "mocr_op_dec_token_penalty", "mocr_op_gemm_argmax_penalty", "mocr_op_penalty_init"]


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return _capi.load_library()


@pytest.fixture(scope="module")
def rec():
    spec = importlib.util.spec_from_file_location("make_surface_golden", os.path.join(GOLDEN, "make_surface_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ the rule
def test_the_rule_on_hand_written_cases():
    lg = np.array([4.0, -4.0, 0.0, 3.0, -0.0, 1.0], np.float32)
    out = pu.penalise(lg, [0, 1, 2, 4, 0], 2.0)
    np.testing.assert_array_equal(out, np.array([2.0, -8.0, 0.0, 3.0, -0.0, 1.0], np.float32))
    assert np.signbit(out[4]) and not np.signbit(out[2]), "v == 0 divides: the zero keeps its sign"
    np.testing.assert_array_equal(pu.penalise(lg, [0, 1], 0.5), np.array([8.0, -2.0, 0.0, 3.0, -0.0, 1.0], np.float32))
    np.testing.assert_array_equal(pu.penalise(lg, [0, 1, 2, 3, 4, 5], 1.0).view(np.uint32), lg.view(np.uint32))
    seen = pu.seen_of([0, 1, 2, 4], 6)
    np.testing.assert_array_equal(pu.pen32(lg, seen, 2.0).view(np.uint32), out.view(np.uint32))
    # a division, not a multiplication by the reciprocal: they differ in fp32
    v, p = np.float32(7.0), np.float32(1.3)
    assert pu.pen32(np.array([v]), [True], p)[0] == v / p and any(np.float32(x) / p != np.float32(x) * (np.float32(1) / p) for x in range(1, 50))


def test_the_rule_is_transformers_processor():
    """RepetitionPenaltyLogitsProcessor on random fp32 scores and histories with repeats, p = 1.3, 2.0, 0.8: bit for bit."""
    torch = pytest.importorskip("torch")
    tr = pytest.importorskip("transformers")
    rs = np.random.RandomState(5)
    for p in (1.3, 2.0, 0.8):
        proc = tr.RepetitionPenaltyLogitsProcessor(penalty=p)
        hist = rs.randint(0, 64, size=(6, 9))
        scores = (rs.standard_normal((6, 64)) * 4).astype(np.float32)
        scores[0, hist[0, 0]] = 0.0
        want = proc(torch.from_numpy(hist).long(), torch.from_numpy(scores.copy())).numpy()
        got = np.stack([pu.penalise(scores[b], hist[b], p) for b in range(6)])
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"p = {p}")
        np.testing.assert_array_equal(np.stack([pu.pen32(scores[b], pu.seen_of(hist[b], 64), p) for b in range(6)]).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("kind", ["alone", "ngram", "bias"])
def test_the_reference_loop_reproduces_transformers_goldens(kind):
    """tests/golden/penalty_<kind>.npz - transformers' generate(repetition_penalty=p[, no_repeat_ngram_size=2 | sequence_bias]) -
    against penalty_util.penalty_generate on the oracle's logits: ids and lengths exactly, the token scores within
    bias_util.SCORE_TOL.  The sequence_bias file shows the order bias -> penalty, the n-gram file penalty -> ban."""
    import torch
    from oracle.mocr_oracle import Oracle
    g = np.load(os.path.join(GOLDEN, f"penalty_{kind}.npz"))
    o = Oracle(synthetic_weights(int(g["weights_seed"]), eos_bias=float(g["eos_bias"])), DEFAULT_SPEC)
    gray = np.stack([np.random.RandomState(int(s)).randint(0, 256, size=(224, 224), dtype=np.uint8) for s in g["crop_seeds"]])
    ML, B = int(g["max_length"]), len(gray)
    aut = None
    if kind == "bias":
        sb = {tuple(int(t) for t in g["seq_tok"][i, :g["seq_len"][i]]): float(g["seq_bias"][i]) for i in range(len(g["seq_len"]))}
        aut = bu.from_sequence_bias(sb)
    with torch.no_grad():
        enc = o.encode(o.preprocess_gray(gray))
    assert int(g["crops"]) == B and (g["changed"] * 2 >= B).all(), "the generator condition: at least half of the crops leave the p = 1 decode"
    worst = 0.0
    for k, p in enumerate(g["penalties"]):
        ids, pl, raw, masks = pu.penalty_generate(o, enc, [float(p)] * B, ML, automata=None if aut is None else [aut] * B,
                                                  ngrams=[int(g["ngram"])] * B)
        lens = pu.lengths(ids, EOS)
        np.testing.assert_array_equal(lens, g["lens"][k])
        for b in range(B):
            np.testing.assert_array_equal(ids[b, :lens[b]], g["ids"][k, b, :lens[b]])
            lp = cu.masked_log_softmax64(pl[b, :lens[b] - 1], masks[b, :lens[b] - 1])[np.arange(lens[b] - 1), ids[b, 1:lens[b]]]
            worst = max(worst, float(np.abs(lp - g["logp"][k, b, 1:lens[b]]).max()))
    assert worst <= bu.SCORE_TOL, worst


# ------------------------------------------------------------------------------------------------ host logic
def test_argument_validation():
    assert _penalties(None, 1.0, 3) is None and _penalties(1.0, 1.0, 2) is None and _penalties([1, 1.0], 1.0, 2) is None
    assert _penalties(None, 1.3, 2) == [1.3, 1.3] and _penalties(1.0, 1.3, 2) is None, "a call's own value overrides the default"
    assert _penalties([1.0, 0.8], 1.0, 2) == [1.0, 0.8] and _penalties(2, 1.0, 1) == [2.0]
    for bad in (0, 0.0, -1.5, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            _penalties(bad, 1.0, 2)
        with pytest.raises(ValueError):
            Engine._penalty([1.0, bad], 2)
        with pytest.raises(ValueError):
            resolve_repetition_penalty(bad, {})
    for bad in (True, "1.3", [1.0, "x"], [None, 1.0]):
        with pytest.raises(TypeError):
            _penalties(bad, 1.0, 2)
    with pytest.raises(ValueError):
        _penalties([1.3], 1.0, 2)
    with pytest.raises(ValueError):
        Engine._penalty([1.3], 2)
    with pytest.raises(TypeError):
        Engine._penalty("checkpoint", 2)
    a = Engine._penalty(1.3, 3)
    assert a.dtype == np.float32 and a.tolist() == [np.float32(1.3)] * 3 and Engine._penalty([1, 0.8], 2).tolist() == [1.0, np.float32(0.8)]


def test_checkpoint_resolution_on_a_synthetic_model_directory(tmp_path):
    """a config.json with repetition_penalty = 1.2: the loader's warning and ignored_generation are what they were;
    "checkpoint" takes the 1.2 and leaves the rest ignored; the default stays 1.0."""
    import json
    from hf_dir import write_hf_dir
    from manga_ocr.weights import load_checkpoint
    d = str(tmp_path / "manga-ocr-base")
    write_hf_dir(d, seed=3)
    cfg_path = os.path.join(d, "config.json")
    cfg = json.load(open(cfg_path))
    cfg["repetition_penalty"] = 1.2
    json.dump(cfg, open(cfg_path, "w"))
    with pytest.warns(RuntimeWarning, match="greedy"):
        spec, _ = load_checkpoint(d)
    ignored = dict(spec.ignored_generation)
    assert ignored["repetition_penalty"] == 1.2 and ignored["num_beams"] == 4
    p, left = resolve_repetition_penalty("checkpoint", ignored)
    assert p == 1.2 and "repetition_penalty" not in left and left["num_beams"] == 4 and ignored["repetition_penalty"] == 1.2
    assert resolve_repetition_penalty(1.0, ignored) == (1.0, ignored) and resolve_repetition_penalty(2, ignored) == (2.0, ignored)
    assert resolve_repetition_penalty("checkpoint", {}) == (1.0, {})
    with pytest.raises(ValueError):
        resolve_repetition_penalty("config", {})
    with pytest.raises(TypeError):
        resolve_repetition_penalty(None, {})


def test_engine_makes_the_penalty_call_only_when_asked(rec):
    """Engine.recognize_* on a recording library: without penalty= the symbols are the ones of before; with it the symbol is
    mocr_recognize_<kind>_penalty - the _automaton argument list plus one pointer, automata / out_state null unless given;
    a beam call refuses it before anything else is looked at."""
    eng = object.__new__(Engine)
    eng.lib, eng.spec, eng._h, eng.max_batch = rec.RecordingLib(), DEFAULT_SPEC, C.c_void_p(0), 9
    crops = [np.zeros((8, 8), np.uint8)] * 3
    eng.recognize_images(crops, no_repeat_ngram=2)
    assert eng.lib.calls[-1]["symbol"] == "mocr_recognize_images_positions"
    eng.recognize_images(crops, penalty=1.3)
    call = eng.lib.calls[-1]
    assert call["symbol"] == "mocr_recognize_images_penalty" and len(call["args"]) == len(_capi.SYMBOLS["mocr_recognize_images_penalty"][1])
    assert call["args"][-1] == "ptr" and call["args"][-3:-1] == ["null", "null"] and call["args"][3] == 3
    eng.recognize_gray(np.zeros((3, 224, 224), np.uint8), 8, penalty=[1.0, 2.0, 0.8], automata=[0, 1, 0], states=True, scores=True)
    call = eng.lib.calls[-1]
    assert call["symbol"] == "mocr_recognize_gray_host_penalty" and call["args"][-3:] == ["ptr", "ptr", "ptr"]
    eng.recognize_regions([np.zeros((32, 48, 3), np.uint8)], [(0, 1, 2, 8, 8)], penalty=2.0)
    assert eng.lib.calls[-1]["symbol"] == "mocr_recognize_regions_penalty"
    eng.recognize_device(0x1000, 3, 0x2000, 0x3000, penalty=[1.3] * 3)
    assert eng.lib.calls[-1]["symbol"] == "mocr_recognize_device_penalty" and len(eng.lib.calls[-1]["args"]) == 19
    n = len(eng.lib.calls)
    with pytest.raises(ValueError, match="beam search does not combine with penalty"):
        eng.recognize_images(crops, beam=BeamConfig(2), penalty=1.3)
    with pytest.raises(ValueError):
        eng.recognize_images(crops, penalty=[1.3, 1.0])
    assert len(eng.lib.calls) == n, "a refused call reached the library"


class _FakeEngine:
    """recognize_images as Engine answers it; logs the keywords of each call.  A crop under p 'decodes' to
    [2, first pixel + round(100 p), 3]."""
    L = 6

    def __init__(self):
        self.calls = []

    def recognize_images(self, images, bgr=False, rotate=None, *, scores=False, alternatives=False, **kw):
        assert set(kw) <= {"token_sets", "no_repeat_ngram", "penalty"}
        self.calls.append((len(images), 1 if scores else 0, {k: list(v) for k, v in kw.items()}))
        n = len(images)
        p = kw.get("penalty") or [0.0] * n
        ids = np.zeros((n, self.L), np.int32)
        ids[:, 0], ids[:, 2] = 2, 3
        ids[:, 1] = [int(im[0, 0]) + int(round(100 * p[i])) for i, im in enumerate(images)]
        lens = np.full(n, 3, np.int32)
        if scores:
            return ids, lens, np.zeros((n, self.L), np.float32)
        return ids, lens


def test_repetition_penalty_is_routed_through_the_batcher_and_the_surface():
    eng = _FakeEngine()
    b = _Batcher(eng, max_batch=4, timeout_ms=60_000.0)
    try:
        pens = [1.0, 1.3, 2.0, 0.8]
        futs = [b.submit(np.full((4, 4), 10 + i, np.uint8), scored=i == 1, penalty=p) for i, p in enumerate(pens)]
        res = [f.result(timeout=30) for f in futs]
        assert eng.calls == [(4, 1, dict(penalty=pens))], "one engine call, one p per crop in queue order"
        for i, (p, r) in enumerate(zip(pens, res)):
            np.testing.assert_array_equal(r[0] if i == 1 else r, [2, 10 + i + int(round(100 * p)), 3])
        futs = [b.submit(np.full((4, 4), 7, np.uint8)) for _ in range(4)]       # nobody asked: the call of before
        [f.result(timeout=30) for f in futs]
        assert eng.calls[-1] == (4, 0, {})
    finally:
        b.close()
    ocr = object.__new__(MangaOcr)
    ocr.engine, ocr.no_repeat_ngram_size, ocr.repetition_penalty, ocr.beam = eng, None, 1.3, None
    ocr.vocab = text.Vocab.synthetic(6144)
    crops = [np.full((8, 8), 5, np.uint8)] * 2
    ocr.recognize_ids(crops)
    assert eng.calls[-1] == (2, 0, dict(penalty=[1.3, 1.3])), "the reader's default"
    ocr.recognize_ids(crops, repetition_penalty=1.0)
    assert eng.calls[-1] == (2, 0, {}), "a call's own 1.0 switches it off: the call of before"
    ocr.recognize_ids(crops, repetition_penalty=[1.0, 2.0], no_repeat_ngram=2)
    assert eng.calls[-1] == (2, 0, dict(no_repeat_ngram=[2, 2], penalty=[1.0, 2.0]))
    ocr.recognize_batch_scored([__import__("PIL.Image").Image.fromarray(c) for c in crops], repetition_penalty=0.8)
    assert eng.calls[-1] == (2, 1, dict(penalty=[0.8, 0.8]))
    assert ocr._decode_kw(None, None, 2) == {}, "the n-best and text-scoring paths take no penalty, not even the reader's"
    ocr.repetition_penalty = 1.0
    ocr.recognize_ids(crops)
    assert eng.calls[-1] == (2, 0, {})
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            ocr.recognize_ids(crops, repetition_penalty=bad)
    with pytest.raises(TypeError):
        ocr.recognize_nbest(crops[0], repetition_penalty=1.3)
    with pytest.raises(TypeError):
        ocr.match(crops[0], None, repetition_penalty=1.3)
    with pytest.raises(TypeError):
        ocr.search(crops[0], None, repetition_penalty=1.3)


def test_beams_and_several_devices_refuse_the_penalty():
    from manga_ocr.multi import MultiGpuEngine
    ocr = object.__new__(MangaOcr)
    ocr.engine, ocr.no_repeat_ngram_size, ocr.repetition_penalty, ocr.beam = _FakeEngine(), None, 1.0, BeamConfig(2)
    ocr.beam_positions = True
    ocr.vocab = text.Vocab.synthetic(6144)
    crops = [np.zeros((8, 8), np.uint8)]
    for call in (lambda: ocr.recognize_ids(crops, repetition_penalty=1.3), lambda: ocr.recognize_ids(crops, repetition_penalty=1.0),
                 lambda: ocr.recognize_batch_scored([], repetition_penalty=2.0)):
        with pytest.raises(ValueError, match="beam search takes no repetition_penalty"):
            call()
    assert ocr.engine.calls == []
    with pytest.raises(ValueError, match="repetition_penalty does not combine with num_beams"):
        MangaOcr(synthetic_seed=0, num_beams=2, repetition_penalty=1.3)
    multi = object.__new__(MultiGpuEngine)          # no __init__: no child process, no GPU
    ocr = object.__new__(MangaOcr)
    ocr.engine, ocr.no_repeat_ngram_size, ocr.repetition_penalty, ocr.beam = multi, None, 1.0, None
    ocr.vocab = text.Vocab.synthetic(6144)
    with pytest.raises(NotImplementedError, match="repetition penalty.*several devices"):
        ocr.recognize_ids(crops, repetition_penalty=1.3)
    with pytest.raises(NotImplementedError, match="repetition penalty.*several devices"):
        MangaOcr(synthetic_seed=0, devices=[0, 1], repetition_penalty=1.3)      # refused before any worker starts


def test_penalty_symbols_are_exported_declared_and_mirrored(lib):
    hdr = open(os.path.join(ROOT, "include", "mocr.h")).read()
    for name in NEW:
        assert name in _capi.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in mocr.h"
        assert getattr(lib, name) is not None
    for kind in ("images", "regions", "device", "gray_host"):
        assert _capi.SYMBOLS[f"mocr_recognize_{kind}_penalty"][1] == _capi.SYMBOLS[f"mocr_recognize_{kind}_automaton"][1] + [P]
    assert _capi.SYMBOLS["mocr_op_dec_token_penalty"][1] == _capi.SYMBOLS["mocr_op_dec_token_soft"][1] + [P, P]
    assert _capi.SYMBOLS["mocr_op_gemm_argmax_penalty"][1] == _capi.SYMBOLS["mocr_op_gemm_argmax_soft"][1] + [P, P]
    # the ABI did not move; null handles are refused before anything is dereferenced
    assert lib.mocr_abi_version() == 2
    assert lib.mocr_op_penalty_init(None, None, 1) == -1
