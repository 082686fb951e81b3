"""CPU: beam search - the reference of the GPU tests (tests/beam_util.py) against transformers' own beam search
(tests/golden/beam_*.npz, written by tests/golden/make_beam_goldens.py), what the goldens exercise, the condition on the
inputs the fp32 GPU test relies on (every crop's min_gap >= 1e-3), and the argument handling of the Python layers."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import beam_util as bu
import ngram_util as ngu
from manga_ocr import _capi
from manga_ocr.engine import BeamConfig, Engine
from manga_ocr.ocr import _Batcher, resolve_num_beams
from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = ["a", "b", "c", "d", "la", "lb", "lc"]      # (la)-(lc): one crop, long searches
ES = {0: False, 1: True, 2: "never"}


def golden(name):
    g = np.load(os.path.join(GOLD, f"beam_{name}.npz"))
    return {k: g[k] for k in g.files}


def golden_crops(g):
    return np.stack([np.random.RandomState(int(s)).randint(0, 256, size=(224, 224), dtype=np.uint8) for s in g["crop_seeds"]])


@functools.lru_cache(maxsize=None)
def _oracle_enc(weights_seed, eos_bias, crop_seeds):
    from oracle.mocr_oracle import Oracle
    o = Oracle(synthetic_weights(weights_seed, **({"eos_bias": eos_bias} if eos_bias else {})), DEFAULT_SPEC)
    gray = np.stack([np.random.RandomState(s).randint(0, 256, size=(224, 224), dtype=np.uint8) for s in crop_seeds])
    return o, o.encode(o.preprocess_gray(gray))


@functools.lru_cache(maxsize=None)
def reference(name):
    """beam_util's search of config `name` on the golden's crops and weights (computed once, shared)"""
    g = golden(name)
    o, enc = _oracle_enc(int(g["weights_seed"]), float(g["eos_bias"]), tuple(int(s) for s in g["crop_seeds"]))
    cfg = bu.Config(int(g["num_beams"]), float(g["length_penalty"]), ES[int(g["early_stopping"])], int(g["no_repeat_ngram_size"]))
    return bu.beam_generate(o, enc, cfg, int(g["max_length"])) + (o, enc)


@pytest.mark.parametrize("name", CONFIGS)
def test_the_reference_is_transformers_beam_search(name):
    g = golden(name)
    ids, lens, scores, info, _, _ = reference(name)
    np.testing.assert_array_equal(lens, g["lens"])
    np.testing.assert_array_equal(ids, g["ids"])
    assert np.abs(scores - g["scores"]).max() <= 1e-4
    assert (lens > 0).all(), "every slot of these goldens holds a hypothesis"


@pytest.mark.parametrize("name", CONFIGS)
def test_every_crop_has_a_margin_of_1e_3(name):
    """the condition the fp32 GPU test relies on: a condition on the inputs, so it is checked here"""
    info = reference(name)[3]
    assert (info["min_gap"] >= 1e-3).all(), info["min_gap"]


def test_the_goldens_exercise_what_they_must():
    ids_a, lens_a, _, info_a, o, enc = reference("a")
    _, lens_b, _, info_b, _, _ = reference("b")
    ga = golden("a")
    ML = int(ga["max_length"])
    # (a): beam search does not return the greedy n-gram row
    base = np.ones((enc.shape[0], bu.V), bool)
    greedy, _, _ = ngu.ngram_generate(o, enc, base, [3] * enc.shape[0], ML)
    glen = ngu.lengths(greedy)
    differs = [not (lens_a[c, 0] == glen[c] and np.array_equal(ids_a[c, 0, :glen[c]], greedy[c, :glen[c]])) for c in range(enc.shape[0])]
    assert any(differs)
    every = [reference(n) for n in CONFIGS]
    # a hypothesis that finished before the last step its crop ran (a hypothesis of L tokens finishes in step L - 2)
    assert any((r[1][c] - 2 < r[3]["steps"][c] - 1).any() for r in every for c in range(r[1].shape[0]))
    # hypotheses of different lengths within one crop
    assert any(len(set(r[1][c].tolist())) > 1 for r in every for c in range(r[1].shape[0]))
    # (a) and (b) end a crop at different steps
    assert (info_a["steps"] != info_b["steps"]).any()
    # (la)-(lc): searches of many steps; under (la) and (lc) the n-gram rule bans tokens of real histories
    for n in ("la", "lb", "lc"):
        assert (reference(n)[3]["steps"] >= 16).all()
    assert all(st.n_banned > 0 for n in ("la", "lc") for st in reference(n)[3]["states"])
    # (d): nothing ends by EOS, every hypothesis ends on the length rule
    ids_d, lens_d = reference("d")[:2]
    assert (lens_d == int(golden("d")["max_length"])).all() and not (ids_d == DEFAULT_SPEC.eos_id).any()


# ------------------------------------------------------------------------------------------------ argument handling
CKPT = {"num_beams": 4, "length_penalty": 2.0, "early_stopping": True, "no_repeat_ngram_size": 3, "do_sample": True}


def test_resolve_num_beams():
    assert resolve_num_beams(None, CKPT) == (None, CKPT)
    cfg, left = resolve_num_beams("checkpoint", CKPT)
    assert cfg == BeamConfig(4, 2.0, True, 3) and left == {"do_sample": True}
    assert CKPT["num_beams"] == 4, "the caller's dictionary is not touched"
    cfg, left = resolve_num_beams(2, CKPT)
    assert cfg == BeamConfig(2, 2.0, True, 3) and left == {"do_sample": True}
    # no_repeat_ngram_size="checkpoint" took the size out before: it comes as the default
    cfg, left = resolve_num_beams("checkpoint", {k: v for k, v in CKPT.items() if k != "no_repeat_ngram_size"}, 3)
    assert cfg == BeamConfig(4, 2.0, True, 3)
    # a greedy checkpoint: "checkpoint" changes nothing; an int gives the defaults
    assert resolve_num_beams("checkpoint", {}) == (None, {})
    assert resolve_num_beams(3, {})[0] == BeamConfig(3, 1.0, False, 0)
    for bad in (1, 5, 0, -2):
        with pytest.raises(ValueError, match="2 .. 4"):
            resolve_num_beams(bad, CKPT)
    with pytest.raises(ValueError):
        resolve_num_beams("config", CKPT)
    for bad in (True, 2.0):
        with pytest.raises(TypeError):
            resolve_num_beams(bad, CKPT)


def test_beam_config_checks():
    assert BeamConfig().key() == (4, 1.0, False, 0)
    s = BeamConfig(3, 2.0, "never", 2).as_struct()
    assert (s.num_beams, s.length_penalty, s.early_stopping, s.no_repeat_ngram_size) == (3, 2.0, 2, 2)
    for kw in (dict(num_beams=1), dict(num_beams=5), dict(early_stopping="always"), dict(no_repeat_ngram=-1)):
        with pytest.raises(ValueError):
            BeamConfig(**kw)
    with pytest.raises(TypeError):
        BeamConfig(num_beams=True)


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


def _check_beam_result(out, n, K):
    L = DEFAULT_SPEC.max_len
    assert [a.shape for a in out] == [(n, K, L), (n, K), (n, K)]
    assert out[0].dtype == np.int32 and out[1].dtype == np.int32 and out[2].dtype == np.float32
    assert (out[1] == 0).all() and (out[2] == np.float32(-1e9)).all()


def test_a_beam_call_is_one_call_to_the_beam_symbol(eng):
    beam = BeamConfig(3, 2.0, True, 3)
    crops = [np.zeros((8, 9), np.uint8)] * 4
    _check_beam_result(eng.recognize_images(crops, beam=beam), 4, 3)
    _check_beam_result(eng.recognize_regions([np.zeros((32, 48, 3), np.uint8)], [(0, 1, 2, 8, 8)] * 4, beam=beam), 4, 3)
    _check_beam_result(eng.recognize_gray(np.zeros((4, 224, 224), np.uint8), max_len=8, beam=beam), 4, 3)
    assert eng.recognize_device(0x1000, 4, 0x2000, 0x3000, beam=beam, d_out_score=0x4000) is None
    names = [name for name, _ in eng.lib.calls]
    assert names == ["mocr_recognize_images_beam", "mocr_recognize_regions_beam", "mocr_recognize_gray_host_beam", "mocr_recognize_device_beam"]
    assert [p.value for p in eng.lib.calls[3][1][-3:]] == [0x2000, 0x3000, 0x4000]
    # what does not fit one batch, and what does not combine, is refused before any call
    eng.lib.calls.clear()
    with pytest.raises(ValueError, match="max_batch"):
        eng.recognize_images([np.zeros((8, 9), np.uint8)] * 6, beam=beam)
    with pytest.raises(ValueError, match="scores"):
        eng.recognize_images(crops, beam=beam, scores=True)
    with pytest.raises(ValueError, match="sources"):
        eng.recognize_gray(np.zeros((4, 224, 224), np.uint8), beam=beam, sources=[0, 1, 2, 3])
    with pytest.raises(TypeError):
        eng.recognize_images(crops, beam=4)
    assert eng.lib.calls == []


class _FakeEngine:
    """recognize_images as Engine answers it; logs (crops, keywords) of each call"""
    L = 6

    def __init__(self):
        self.calls = []

    def recognize_images(self, images, bgr=False, rotate=None, **kw):
        self.calls.append((len(images), dict(kw)))
        n = len(images)
        if "beam" in kw:
            K = kw["beam"].num_beams
            return np.full((n, K, self.L), 7, np.int32), np.full((n, K), 3, np.int32), np.zeros((n, K), np.float32)
        return np.full((n, self.L), 5, np.int32), np.full(n, 2, np.int32)


def test_the_batcher_never_merges_beam_and_greedy_requests():
    fe = _FakeEngine()
    b = _Batcher(fe, max_batch=8, timeout_ms=200.0)
    try:
        gray = np.zeros((4, 4), np.uint8)
        beam4, beam2 = BeamConfig(4), BeamConfig(2)
        futs = [b.submit(gray), b.submit(gray), b.submit(gray, beam=beam4), b.submit(gray, beam=beam4), b.submit(gray, beam=beam4),
                b.submit(gray, beam=beam2), b.submit(gray)]
        res = [f.result(timeout=10) for f in futs]
    finally:
        b.close()
    assert all(isinstance(r, np.ndarray) and r.shape == (2,) for r in (res[0], res[1], res[6]))
    assert all(isinstance(r, tuple) and r[0].shape == (4, 6) and r[1].shape == (4,) for r in res[2:5])
    assert res[5][0].shape == (2, 6)
    # no call mixes: every call is all greedy (no beam keyword at all) or one beam configuration, at most max_batch // K crops
    assert sum(n for n, _ in fe.calls) == 7
    for n, kw in fe.calls:
        if "beam" in kw:
            assert set(kw) == {"beam"} and n <= 8 // kw["beam"].num_beams
        else:
            assert kw == {}
    order = [kw.get("beam") for _, kw in fe.calls]
    assert [o for i, o in enumerate(order) if i == 0 or o != order[i - 1]][:1] == [None]
    assert beam4 in order and beam2 in order
