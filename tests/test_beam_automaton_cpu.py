"""CPU: beam search under token automata (include/mocr.h, "beam search under a token automaton") - the float64 reference
(tests/beam_automaton_util.py) against transformers' goldens and its reductions to the token form, the prototypes, the Engine
keywords on a recording library, the ``match*`` methods of MangaOcr on a fake engine, and the refusals that stay."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import automaton_util as au
import beam_automaton_util as bau
import beam_token_util as btu
import beam_util as bu
import constraint_util as cu
from manga_ocr import _capi
from manga_ocr.engine import BeamConfig, Engine
from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights

V, EOS, START, PAD = au.V, au.EOS, 2, DEFAULT_SPEC.pad_id
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ES = {0: False, 1: True, 2: "never"}
CASES = ["a2", "a3", "a4", "b", "c", "d", "e0", "e2", "h2", "h3", "h4"]


@pytest.fixture(scope="module")
def rec():
    """the surface recorder's fakes"""
    spec = importlib.util.spec_from_file_location("make_surface_golden", os.path.join(GOLDEN, "make_surface_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_ORACLES = {}


def _oracle(seed, eos_bias):
    from oracle.mocr_oracle import Oracle
    key = (int(seed), float(eos_bias))
    if key not in _ORACLES:
        _ORACLES[key] = Oracle(synthetic_weights(key[0], eos_bias=key[1]), DEFAULT_SPEC)
    return _ORACLES[key]


def _golden(name, prefix="beam_aut"):
    g = np.load(os.path.join(GOLDEN, f"{prefix}_{name}.npz"))
    return {k: g[k] for k in g.files}


def _crops(g, rows=None):
    seeds = g["crop_seeds"] if rows is None else g["crop_seeds"][rows]
    return np.stack([np.random.RandomState(int(s)).randint(0, 256, size=(224, 224), dtype=np.uint8) for s in seeds])


def _automata(g):
    auts = []
    for i in g["aut_of_crop"]:
        if i < 0:
            auts.append(None)
            continue
        s0, ns = int(g["aut_first"][i]), int(g["aut_states"][i])
        eb = g["edge_begin"][s0:s0 + ns + 1]
        auts.append(au.unpack(eb - eb[0], g["edge_token"][eb[0]:eb[-1]], g["edge_next"][eb[0]:eb[-1]] - s0, g["accepting"][s0:s0 + ns]))
    return auts


def _masks(g):
    out = np.ones((len(g["sets"]), V), bool)
    for c, row in enumerate(g["sets"]):
        if (row >= 0).any():
            out[c] = cu.mask_of(row[row >= 0].tolist())
    return out


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("name", CASES)
def test_the_reference_returns_the_transformers_hypotheses(name):
    """every golden crop: ids, lengths and states exactly, token scores within 3e-6, sequence scores within
    beam_automaton_util.score_tol(3e-6) - the generator's own assertion, from the files"""
    g = _golden(name)
    K, lp, ML = int(g["num_beams"]), float(g["length_penalty"]), int(g["max_length"])
    cfg = bu.Config(K, lp, ES[int(g["early_stopping"])], int(g["no_repeat_ngram_size"]))
    o = _oracle(g["weights_seed"], g["eos_bias"])
    enc = o.encode(o.preprocess_gray(_crops(g)))
    auts = _automata(g)
    ids, lens, scores, logp, state, info = bau.beam_generate(o, enc, cfg, ML, auts, _masks(g))
    assert (info["min_gap"] >= (2e-2 if name[0] == "h" else 1e-3)).all() and np.allclose(info["min_gap"], g["gaps"], rtol=1e-3)
    assert name[0] != "h" or len(auts) >= 6
    for c in range(len(auts)):
        w = bau.real_only(ids[c], lens[c], scores[c], logp[c], state[c], lp, ML, PAD)
        np.testing.assert_array_equal(w[1], g["lens"][c])
        np.testing.assert_array_equal(w[0], g["ids"][c])
        np.testing.assert_array_equal(w[4], g["state"][c])
        assert (np.abs(w[2] - g["scores"][c]) <= bau.score_tol(w[2], 3e-6)).all() and np.abs(w[3] - g["logp"][c]).max() <= 3e-6
        assert g["lens"][c, 0] > 0 and (auts[c] is None or g["state"][c, 0] >= 0)
    if name == "c":
        assert auts[1] is None and (g["state"][1] == au.NONE).all() and (g["lens"][2] > 0).sum() == 2, "a crop without one; fewer entries than beams"
    if name == "d":
        assert (g["lens"] == ML).all() and (g["state"] == ML - 1).all(), "the stop by length walks the last token"
    if name == "b":
        assert all((row >= 0).any() for row in g["sets"])


def test_the_goldens_hold_a_crop_where_beam_and_greedy_disagree():
    n = 0
    for name in ("a2", "a3", "a4"):
        g = _golden(name)
        n += int(((g["greedy_entry"] >= 0) & (g["beam_entry"] >= 0) & (g["greedy_entry"] != g["beam_entry"])).sum())
    assert n >= 1
    # ... and the float64 greedy reference really reads that entry: one crop, end to end
    g = _golden("a4")
    c = int(np.nonzero(g["greedy_entry"] != g["beam_entry"])[0][0])
    o = _oracle(g["weights_seed"], g["eos_bias"])
    enc = o.encode(o.preprocess_gray(_crops(g, [c])))
    aut = _automata(g)[c]
    _, _, _, st = au.automaton_generate(o, enc, [aut], np.ones((1, V), bool), [0], int(g["max_length"]))
    assert int(st[0]) in aut.accepting and int(st[0]) != int(g["state"][c, 0])


@pytest.mark.parametrize("name", ["b", "d"])
def test_a_one_state_automaton_is_the_token_set(name):
    """the crops of tests/golden/beam_tok_*.npz: the set as a one-state automaton (and nothing through the set), the set
    under the universal automaton, and the set alone give the same search - ids, lengths, scores and token scores to the bit
    of the float64 reference"""
    g = _golden(name, "beam_tok")
    K, ML = int(g["num_beams"]), int(g["max_length"])
    cfg = bu.Config(K, float(g["length_penalty"]), ES[int(g["early_stopping"])], int(g["no_repeat_ngram_size"]))
    o = _oracle(g["weights_seed"], g["eos_bias"])
    rows = [0, 1]
    enc = o.encode(o.preprocess_gray(_crops(g, rows)))
    masks = np.stack([cu.mask_of(g["sets"][c][g["sets"][c] >= 0].tolist()) for c in rows])
    want = btu.beam_generate(o, enc, cfg, ML, masks)
    as_aut = bau.beam_generate(o, enc, cfg, ML, [bau.set_automaton(m) for m in masks], None)
    uni = bau.beam_generate(o, enc, cfg, ML, [au.universal()] * len(rows), masks)
    none = bau.beam_generate(o, enc, cfg, ML, None, masks)
    for got, what in ((as_aut, "one-state automaton"), (uni, "universal automaton"), (none, "no automaton")):
        for i in range(4):
            np.testing.assert_array_equal(got[i], want[i], err_msg=f"{what}: block {i}")
    np.testing.assert_array_equal(want[0][:, :, :ML], g["ids"][rows])
    assert (as_aut[4][as_aut[1] > 0] == 0).all() and (none[4] == au.NONE).all()


def test_the_step_of_the_reference():
    """the rule in small: the mask of a state, the dead beam, the walk on reorder, the state a hypothesis keeps"""
    K, cfg = 2, bu.Config(2, 1.0, False, 0)
    aut = au.Automaton({0: {10: 1, 11: 2}, 1: {12: 3}}, [2, 3])
    st = bau.State(K, START, aut)
    lg = np.zeros((K, V))
    lg[:, 10], lg[:, 11], lg[:, EOS] = 3.0, 2.0, 9.0
    m = bau.beam_masks(st, cfg)
    assert sorted(np.nonzero(m[0])[0]) == [10, 11] and not m[0, EOS], "EOS is banned where the state does not accept"
    cv, cpar, ctok, stop, clp, cst = bau.step(bau.processed(lg, st, cfg), st, cfg, 8, EOS)
    assert list(ctok[:2]) == [10, 11] and list(cpar[:2]) == [0, 0] and st.ast == [1, 2], "two beams from one parent, two states"
    assert cv[2] == -1e9 and cv[3] == -1e9, "the padding beam's children are -1e9f, whatever their log-probability"
    lg2 = np.zeros((K, V))
    lg2[0, 12], lg2[1, EOS] = 1.0, 1.0
    bau.step(bau.processed(lg2, st, cfg), st, cfg, 8, EOS)
    assert st.hyp_seq[0] == [START, 11, EOS] and st.hyp_state[0] == 2, "stopped on EOS: the parent's state"
    assert st.seqs[0] == [START, 10, 12] and st.ast[0] == 3
    assert st.ast[1] == au.DEAD and st.run[1] == -1e9, "the stopped candidate carried on: EOS is no edge"
    lp = bau.processed(np.zeros((K, V)), st, cfg)
    assert np.isinf(lp[1]).all() and np.isfinite(lp[0, EOS]) and np.isinf(lp[0, 12]), "a DEAD beam allows nothing; a leaf allows EOS"
    # a set that meets no edge: a dead beam, no dead-end rule
    st2 = bau.State(K, START, aut)
    assert np.isinf(bau.processed(lg, st2, cfg, cu.mask_of([500]))).all()
    assert bau.junk_below(2.0, 16) == -1e9 / 256 and bau.junk_below(0.0, 16) == -1e9


# ------------------------------------------------------------------------------------------------ the prototypes
def test_the_prototypes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "mocr.h")).read()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    names = [f"mocr_recognize_{k}_beam_automaton" for k in ("images", "regions", "gray_host", "device")] + ["mocr_op_beam_select_automaton"]
    for name in names:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared"
        want = []
        for p in m.group(1).replace("\n", " ").split(","):
            p = p.strip()
            if "mocr_engine" in p or ("*" in p and not any(s in p for s in ("mocr_image", "mocr_region", "mocr_beam_config", "mocr_token_args"))):
                want.append(_capi._P)
            elif "*" in p:
                struct = {"mocr_image": _capi.MocrImage, "mocr_region": _capi.MocrRegion, "mocr_beam_config": _capi.MocrBeamConfig,
                          "mocr_token_args": _capi.MocrTokenArgs}[next(s for s in ("mocr_image", "mocr_region", "mocr_beam_config", "mocr_token_args") if s in p)]
                want.append(C.POINTER(struct))
            else:
                want.append(ctype[p.split()[0]])
        res, args = _capi.SYMBOLS[name]
        assert res is C.c_int and args == want, name
    # the twins are the *_beam_positions calls plus two pointers
    for k in ("images", "regions", "gray_host", "device"):
        assert _capi.SYMBOLS[f"mocr_recognize_{k}_beam_automaton"][1] == _capi.SYMBOLS[f"mocr_recognize_{k}_beam_positions"][1] + [_capi._P] * 2
    assert _capi.SYMBOLS["mocr_op_beam_select_automaton"][1] == _capi.SYMBOLS["mocr_op_beam_select_positions"][1] + [_capi._P] * 7
    assert "beam search under a token automaton" in hdr and "Beam search is out of scope" not in hdr


# ------------------------------------------------------------------------------------------------ Engine on a recording library
def test_engine_keywords_reach_the_beam_automaton_symbols_only_when_asked(rec):
    eng = object.__new__(Engine)
    eng.lib, eng.spec, eng._h, eng.max_batch = rec.RecordingLib(), DEFAULT_SPEC, C.c_void_p(0), 12
    gray = np.zeros((3, 224, 224), np.uint8)
    cfg = BeamConfig(3)
    eng.recognize_gray(gray, 16, beam=cfg)
    eng.recognize_gray(gray, 16, beam=cfg, beam_scores=True)
    eng.recognize_gray(gray, 16, beam=cfg, beam_positions=True)
    assert [c["symbol"] for c in eng.lib.calls] == ["mocr_recognize_gray_host_beam", "mocr_recognize_gray_host_beam_tokens",
                                                    "mocr_recognize_gray_host_beam_positions"], "nobody asked: the calls of before"
    eng.lib.calls.clear()
    out = eng.recognize_gray(gray, 16, beam=cfg, beam_automata=[4, None, 5], beam_states=True)
    assert len(out) == 4 and out[3].dtype == np.int32 and out[3].shape == (3, 3) and (out[3] == -1).all()
    call, = eng.lib.calls
    assert call["symbol"] == "mocr_recognize_gray_host_beam_automaton" and len(call["args"]) == 13
    assert call["args"][2:4] == [3, 16] and call["args"][8:11] == ["null", "null", "null"], "n, max_len; no logp, sets, pos"
    assert call["args"][-2:] == ["ptr", "ptr"]
    eng.lib.calls.clear()
    out = eng.recognize_images([np.zeros((8, 8), np.uint8)] * 2, beam=cfg, beam_automata=7, beam_scores=True, beam_sets=[0, 1], beam_positions=True)
    assert len(out) == 5 and out[3].shape == (2, 3, DEFAULT_SPEC.max_len) and out[4].shape == (2, 3, DEFAULT_SPEC.max_len, 5)
    call, = eng.lib.calls
    assert call["symbol"] == "mocr_recognize_images_beam_automaton" and call["args"][-5:] == ["ptr", "ptr", "ptr", "ptr", "null"]
    eng.lib.calls.clear()
    out = eng.recognize_regions([np.zeros((32, 48, 3), np.uint8)], [(0, 1, 2, 8, 8)], beam=cfg, beam_states=True, beam_positions=True)
    assert len(out) == 5 and out[3].ndim == 4 and out[4].shape == (1, 3), "positions, then states last"
    eng.recognize_device(0x1000, 2, 0x2000, 0x3000, beam=cfg, d_out_score=0x8000, beam_automata=[1, 2], d_out_beam_state=0x9000)
    eng.recognize_device(0x1000, 2, 0x2000, 0x3000, beam=cfg, d_out_score=0x8000, beam_automata=[1, 2])
    assert [c["symbol"] for c in eng.lib.calls] == ["mocr_recognize_regions_beam_automaton"] + ["mocr_recognize_device_beam_automaton"] * 2
    assert eng.lib.calls[0]["args"][-2:] == ["null", "ptr"] and eng.lib.calls[1]["args"][-2:] == ["ptr", "0x9000"]
    assert eng.lib.calls[2]["args"][-2:] == ["ptr", "null"]
    eng.lib.calls.clear()
    for bad, exc in ((dict(beam_automata=[1, 2, 3]), ValueError), (dict(beam_states=True), ValueError),
                     (dict(beam=cfg, beam_automata=[1, 2]), ValueError), (dict(beam=cfg, beam_automata="x"), TypeError),
                     (dict(beam=cfg, beam_automata=[1.5, 2, 3]), TypeError), (dict(beam=cfg, beam_automata=True), TypeError),
                     (dict(beam=cfg, beam_automata=1, scores=True), ValueError),
                     # the old keywords keep raising with beam=
                     (dict(beam=cfg, automata=[1, 2, 3]), ValueError), (dict(beam=cfg, states=True), ValueError),
                     (dict(beam=cfg, automata=[1, 2, 3], beam_automata=[1, 2, 3]), ValueError)):
        with pytest.raises(exc):
            eng.recognize_gray(gray, 16, **bad)
    assert not eng.lib.calls, "a refused call reached the library"

    class HookLib:
        def mocr_op_beam_select_automaton(self, *a):
            self.seen = a
            return _capi.MOCR_OK
    eng.lib = HookLib()
    eng.op_beam_select_automaton(cfg, 1, 2, 3, 4, 5, 6, d_aut_state=7, n=4)
    assert len(eng.lib.seen) == 22 and eng.lib.seen[-2].value == 7 and eng.lib.seen[-1].value is None


# ------------------------------------------------------------------------------------------------ MangaOcr on a fake engine
def _fake_engine(rec):
    class MatchEngine(rec.RecordingEngine):
        """the recorder's engine plus automata under beams.  A beam call with ``beam_automata`` answers, for crop i and K = 4:
        slot 0 START, 10 + i, 20, EOS (score -1 - i), slot 1 START, 10 + i, EOS (-2 - i), slot 2 slot 0 again at -1e9 / 3 - a
        padding beam's duplicate -, slot 3 START, 11, 21 without EOS (-5); with K = 3 the first three, with K = 2 the first two.
        The states are the walks"""

        def __init__(self):
            super().__init__()
            self.auts = [None]

        def automaton(self, eb, et, en, acc):
            self.auts.append(au.unpack(*(np.asarray(x) for x in (eb, et, en, acc))))
            return len(self.auts) - 1

        def _answer(self, method, args, kw, sliver):
            if "beam_automata" not in kw:
                return super()._answer(method, args, kw, sliver)
            self.calls.append([method, len(sliver), {k: (v if not isinstance(v, BeamConfig) else v.key()) for k, v in kw.items()}])
            n, K, L = len(sliver), kw["beam"].num_beams, self.L
            ids, lens, sc = np.zeros((n, K, L), np.int32), np.zeros((n, K), np.int32), np.full((n, K), -1e9, np.float32)
            logp, pos, state = np.zeros((n, K, L), np.float32), np.zeros((n, K, L, 5), np.float32), np.full((n, K), -1, np.int32)
            for i, h in enumerate(kw["beam_automata"]):
                if sliver[i]:
                    continue
                rows = [([START, 10 + i, 20, EOS], -1.0 - i), ([START, 10 + i, EOS], -2.0 - i), ([START, 10 + i, 20, EOS], -1e9 / 3),
                        ([START, 11, 21], -5.0)][:K]
                for j, (row, s) in enumerate(rows):
                    ids[i, j, :len(row)], lens[i, j], sc[i, j] = row, len(row), s
                    logp[i, j, 1:len(row)] = -0.5
                    if h:
                        state[i, j] = self.auts[h].walk(row[1:])
            out = (ids, lens, sc)
            if kw.get("beam_scores"):
                out += (logp,)
            if kw.get("beam_positions"):
                out += (pos,)
            return out + ((state,) if kw.get("beam_states") else ())
    return MatchEngine()


def test_match_on_a_fake_engine(rec):
    eng = _fake_engine(rec)
    ocr = rec._ocr(eng, max_batch=16)
    try:
        tok = lambda i: ocr.vocab.tokens[i]
        texts = [tok(10) + tok(20), tok(10), tok(11) + tok(20), tok(11) + tok(21), tok(12) + tok(20)]
        lx = ocr.lexicon(texts)
        imgs = [rec._img(i) for i in range(3)]
        got = ocr.match_batch(imgs, lx)
        call = eng.calls[-1]
        assert call[0] == "recognize_images" and call[2]["beam"] == (4, 1.0, 0, 0) and call[2]["beam_automata"] == [lx.handle] * 3 and call[2]["beam_states"]
        assert "beam_scores" not in call[2] and "beam_sets" not in call[2] and "beam_positions" not in call[2], "only what was asked"
        # crop 0: two entries in score order; the duplicate at -1e9 / 3 and the hypothesis without EOS are dropped
        assert [r.text for r in got[0]] == [texts[0], texts[1]] and [r.entry for r in got[0]] == [0, 1]
        assert all(r.accepted and r.state in lx.accepting for r in got[0]) and [r.sequence_score for r in got[0]] == [-1.0, -2.0]
        assert [r.entry for r in got[1]] == [2] and got[1][0].text == texts[2], "crop 1: '11' alone is no entry"
        assert [r.entry for r in got[2]] == [4]
        raw = ocr.match_batch(imgs, lx, raw=True)
        assert [len(r) for r in raw] == [4, 4, 4] and [r.accepted for r in raw[0]] == [True, True, True, False]
        assert raw[0][3].entry is None and raw[0][3].state in lx.accepting, "an entry's tokens without EOS: its state, not accepted"
        assert [r.accepted for r in raw[1]] == [True, False, True, False] and raw[1][1].entry is None
        # fewer beams; the keywords travel
        got = ocr.match_batch(imgs, lx, k=2, length_penalty=2.0, early_stopping=True, no_repeat_ngram=3, token_scores=True, positions=True)
        assert eng.calls[-1][2]["beam"] == (2, 2.0, 1, 3) and eng.calls[-1][2]["beam_scores"] and eng.calls[-1][2]["beam_positions"]
        assert len(got[0]) == 2 and got[0][0].positions is not None and len(got[0][0].logprobs) == 3
        # per-crop lexicons: a crop without one keeps nothing, and everything with raw=True
        one = ocr.lexicon([texts[1]])
        per = ocr.match_batch(imgs, [lx, None, one])
        assert eng.calls[-1][2]["beam_automata"] == [lx.handle, 0, one.handle]
        assert [r.entry for r in per[0]] == [0, 1] and per[1] == [] and per[2] == []
        rawp = ocr.match_batch(imgs, [lx, None, one], raw=True)
        assert all(r.state == -1 and not r.accepted for r in rawp[1]) and rawp[2][0].state == au.DEAD
        # a pattern: distinct accepted hypotheses without entries
        pat = ocr.automaton({0: {10: 1}, 1: {20: 2}}, [1, 2])
        assert [(r.text, r.entry, r.state) for r in ocr.match_batch(imgs[:1], pat)[0]] == [(texts[0], None, 2), (texts[1], None, 1)]
        # one crop goes through the batcher; bgr crops and regions
        single = ocr.match(imgs[0], lx, k=3)
        assert [r.entry for r in single] == [0, 1] and eng.calls[-1][2]["beam_automata"] == [lx.handle] and eng.calls[-1][2]["beam"][0] == 3
        assert [r.entry for r in ocr.match_bgr([np.zeros((8, 8, 3), np.uint8)], lx)[0]] == [0, 1]
        page = np.zeros((32, 48, 3), np.uint8)
        regs = ocr.match_regions([page], [(0, 1, 2, 8, 8), (0, 3, 4, 0, 8)], lx)
        assert eng.calls[-1][0] == "recognize_regions" and [r.entry for r in regs[0]] == [0, 1] and regs[1] == []
        # an allowed= set travels as beam_sets
        ts = ocr.token_set(ids=[10, 20])
        ocr.match_batch(imgs, lx, allowed=ts)
        assert eng.calls[-1][2]["beam_sets"] == [ts.handle] * 3
        # refusals: before the engine is reached
        before = len(eng.calls)
        for bad, exc in ((dict(lexicon=None), ValueError), (dict(lexicon=[lx]), ValueError), (dict(lexicon=3), TypeError),
                         (dict(lexicon=lx, k=5), ValueError), (dict(lexicon=lx, k=1), ValueError), (dict(lexicon=lx, early_stopping="no"), ValueError)):
            with pytest.raises(exc):
                ocr.match_batch(imgs, **bad)
        assert len(eng.calls) == before
        # the old refusals still refuse, and name the new methods
        for name, args in (("recognize_beam", (imgs[0],)), ("recognize_batch_beam", (imgs,)), ("recognize_bgr_beam", ([np.zeros((8, 8, 3), np.uint8)],)),
                           ("recognize_regions_beam", ([page], [(0, 1, 2, 8, 8)]))):
            with pytest.raises(ValueError, match="lexicon") as e:
                getattr(ocr, name)(*args, lexicon=lx)
            assert "match" in str(e.value)
        # a plain beam call and a greedy lexicon= call make the calls they made
        ocr.recognize_batch_beam(imgs, 2)
        assert "beam_automata" not in eng.calls[-1][2] and "beam_states" not in eng.calls[-1][2]
    finally:
        ocr._batcher.close()

    class Multi(type(eng)):
        NO_LEXICON = "token automata are not implemented for several devices"
        NO_BEAM = "beam search is not implemented for several devices"
    ocr = rec._ocr(Multi())
    try:
        for name, args in (("match", (rec._img(0), None)), ("match_batch", ([rec._img(0)], None)), ("match_bgr", ([], None)),
                           ("match_regions", ([], [], None))):
            with pytest.raises(NotImplementedError):
                getattr(ocr, name)(*args)
    finally:
        ocr._batcher.close()
