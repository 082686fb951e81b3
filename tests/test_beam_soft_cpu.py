"""CPU: beam search under soft token automata (include/mocr.h, "beam search under soft token automata") - the float64
reference (tests/beam_soft_util.py) against transformers' goldens, its identities on random logits, the carried-on-EOS clause
and the fp32 running score on constructed steps, the prototypes, the Engine keyword on a recording library, and the ``search*``
methods of MangaOcr on a fake engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import automaton_util as au
import beam_automaton_util as bau
import beam_soft_util as bsu
import beam_util as bu
import bias_util
from manga_ocr import _capi
from manga_ocr.engine import BeamConfig, Engine
from manga_ocr.weights import DEFAULT_SPEC
from test_beam_automaton_cpu import ES, _crops, _fake_engine, _oracle, rec  # noqa: F401  (rec: the surface recorder's fakes, a fixture)

V, EOS, START, PAD = au.V, au.EOS, 2, DEFAULT_SPEC.pad_id
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ["p2", "p3", "p4", "g", "n", "e"]


def _golden(name):
    g = np.load(os.path.join(GOLDEN, f"beam_soft_{name}.npz"))
    return {k: g[k] for k in g.files}


def _bias(g):
    return {tuple(int(t) for t in row[:n]): float(b) for row, n, b in zip(g["seq_tok"], g["seq_len"], g["seq_bias"])}


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("name", CASES)
def test_the_reference_returns_the_transformers_hypotheses(name):
    """every golden crop: ids, lengths and states exactly, token scores within 3e-6, sequence scores within score_tol(3e-6) - the
    generator's own assertion, from the files; the compact (fallback) compilation gives the same search"""
    g = _golden(name)
    K, lp, ML = int(g["num_beams"]), float(g["length_penalty"]), int(g["max_length"])
    cfg = bu.Config(K, lp, ES[int(g["early_stopping"])], int(g["no_repeat_ngram_size"]))
    o = _oracle(g["weights_seed"], g["eos_bias"])
    enc = o.encode(o.preprocess_gray(_crops(g)))
    sb = _bias(g)
    assert all(b * 8 == int(b * 8) for b in sb.values()) and ML == 16 and 2 <= len(g["crop_seeds"]) <= 4
    masks = np.unpackbits(g["set_bits"], axis=1)[:, :V].astype(bool) if int(g["with_set"]) else None
    n = len(g["crop_seeds"])
    for compact in ([False, True] if int(g["compact"]) else [False]):
        aut = bias_util.from_sequence_bias(sb, compact=compact)
        ids, lens, scores, logp, state, info = bsu.beam_generate(o, enc, cfg, ML, [aut] * n, masks)
        assert (info["min_gap"] >= 1e-3).all() and np.allclose(info["min_gap"], g["gaps"], rtol=1e-2)
        for c in range(n):
            w = bsu.real_only(ids[c], lens[c], scores[c], logp[c], state[c], lp, ML, PAD)
            np.testing.assert_array_equal(w[1], g["lens"][c])
            np.testing.assert_array_equal(w[0], g["ids"][c])
            np.testing.assert_array_equal(w[4], g["state_compact" if compact else "state"][c])
            assert (np.abs(w[2] - g["scores"][c]) <= bsu.score_tol(w[2], 3e-6)).all() and np.abs(w[3] - g["logp"][c]).max() <= 3e-6
            assert g["lens"][c, 0] > 0 and g["state"][c, 0] >= 0
    assert int(g["changed"].sum()) * 2 >= n, "the biases change the best hypothesis of at least half of the crops"
    if name == "e":
        assert (g["lens"] < ML).all(), "the early-EOS case ends early"
    if name == "n":
        assert int(g["no_repeat_ngram_size"]) == 2 and not masks.all()


def _random_search(seed, K, aut, base=None, soft=True, ngram=2, steps=7):
    """a search on random logits (a function of the beams' histories, so that two searches that decide alike see the same rows)"""
    cfg = bu.Config(K, 1.0, False, ngram)

    def logits_of(seqs, parents, t):
        rows = []
        for s in seqs:
            rs = np.random.RandomState(abs(hash((seed, tuple(s)))) % (2 ** 31))
            lg = rs.standard_normal(V) * 3.0
            lg[EOS] += 1.0
            rows.append(lg)
        return np.stack(rows)
    return (bsu if soft else bau).search(logits_of, K, cfg, steps + 1, aut, base, START, EOS)


def _same_search(a, b, states=True):
    assert a.hyp_seq == b.hyp_seq and a.hyp_logp == b.hyp_logp and list(a.hyp_score) == list(b.hyp_score) and a.steps == b.steps
    if states:
        assert a.hyp_state == b.hyp_state


@pytest.mark.parametrize("K", [2, 3, 4])
def test_the_identities_on_random_logits(K):
    rs = np.random.RandomState(K)
    toks = [int(x) for x in rs.choice(np.arange(5, V), 40, replace=False)]
    hard = au.Automaton({0: {t: 1 for t in toks[:20]}, 1: {t: 0 for t in toks[10:40]}}, [0, 1])
    zero = bias_util.SoftAutomaton(hard.trans, hard.accepting, {s: {t: 0.0 for t in e} for s, e in hard.trans.items()}, None, hard.n_states)
    # a hard automaton under the soft rule is beam_automaton_util's search; all-zero weights change nothing
    _same_search(_random_search(1, K, hard), _random_search(1, K, hard, soft=False))
    _same_search(_random_search(1, K, zero), _random_search(1, K, hard, soft=False))
    # the universal-open automaton is no automaton (its one state apart)
    base = np.ones(V, bool)
    base[rs.choice(np.arange(5, V), 3000, replace=False)] = False
    base[EOS] = True
    for m in (None, base):
        u, none = _random_search(2, K, bias_util.universal_open(), m), _random_search(2, K, None, m, soft=False)
        _same_search(u, none, states=False)
        assert all(s == 0 for s, seq in zip(u.hyp_state, u.hyp_seq) if seq) and all(s == au.NONE for s in none.hyp_state)
    # ... and a weight does move the search
    w = bias_util.from_sequence_bias({(t,): 6.0 for t in toks[:3]})
    moved, free = _random_search(2, K, w), _random_search(2, K, None, soft=False)
    assert moved.hyp_seq != free.hyp_seq and any(t in seq for seq in moved.hyp_seq for t in toks[:3])


def test_the_step_of_the_rule():
    """the rule in small: the weight behind the log_softmax and without renormalising, a masked token stays -inf, an open state
    masks EOS unless it accepts, running' = s + running in fp32, and the carried-on-EOS clause"""
    K, cfg = 2, bu.Config(2, 1.0, False, 0)
    aut = bias_util.SoftAutomaton({0: {10: 1, 11: 0}, 1: {12: 1}}, [1], {0: {10: 2.5, 11: -1.0}, 1: {12: 0.125}}, {0: 0, 1: 0}, fallback=True)
    st = bsu.State(K, START, aut)
    rs = np.random.RandomState(0)
    lg = rs.standard_normal((K, V))
    lg[:, EOS], lg[:, 10] = 9.0, 6.0
    lp = bu.log_softmax64(lg)
    p = bsu.processed(lg, st, cfg)
    assert p[0, 10] == lp[0, 10] + 2.5 and p[0, 11] == lp[0, 11] - 1.0 and p[0, 500] == lp[0, 500], "lp + w: gmax and logS never see a weight"
    assert np.isinf(p[0, EOS]) and np.isfinite(p[0, 1:][np.arange(1, V) != EOS]).all(), "state 0 is open and does not accept: EOS is masked"
    base = np.ones(V, bool)
    base[10] = False
    assert np.isinf(bsu.processed(lg, st, cfg, base)[0, 10]), "a weight never revives a masked token"
    # running' = s + running in fp32: the engine's token score is the ranked fp32 value
    cv, cpar, ctok, stop, clp, cst = bsu.step(p, st, cfg, 8, EOS)
    assert int(ctok[0]) == 10 and int(cst[0]) == 1 and st.ast[0] == 1
    s32, run32 = np.float32(clp[0]), np.float32(0.0)
    assert np.float32(s32 + run32) == np.float32(cv[0]) and abs(float(s32) - (lp[0, 10] + 2.5)) < 1e-6
    # the carried-on EOS: beam 0 (state 1: open, accepting) stops on EOS; with fewer than K candidates left that did not stop, the
    # stopped one is carried on at score - 1e9, and its state follows the default edge (fallback: the default state, 0)
    st2 = bsu.State(K, START, aut)
    st2.ast = [1, 1]
    st2.run = np.array([0.0, -np.inf])
    lg2 = np.full((K, V), -30.0)
    lg2[:, EOS], lg2[:, 12] = 5.0, 4.0
    base2 = np.zeros(V, bool)
    base2[[EOS, 12]] = True
    cv, cpar, ctok, stop, clp, cst = bsu.step(bsu.processed(lg2, st2, cfg, base2), st2, cfg, 8, EOS)
    assert [int(t) for t in ctok[:2]] == [EOS, 12] and list(stop[:2]) == [True, False]
    assert st2.hyp_seq[0] == [START, EOS] and st2.hyp_state[0] == 1, "a hypothesis that stopped on EOS keeps its parent's state"
    assert st2.seqs == [[START, 12], [START, EOS]] and st2.run[1] <= -1e8, "the stopped candidate is carried on at score - 1e9"
    assert st2.ast == [1, 0], "... in the default state: EOS is never an edge, the suffix match restarts"
    hard = au.Automaton({0: {12: 0}}, [0])
    st3 = bsu.State(K, START, hard)
    st3.run = np.array([0.0, -np.inf])
    bsu.step(bsu.processed(lg2, st3, cfg, base2), st3, cfg, 8, EOS)
    assert st3.ast == [0, au.DEAD], "in a closed state it is DEAD, as before"


# ------------------------------------------------------------------------------------------------ the prototypes
def test_the_prototypes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "mocr.h")).read()
    for k in ("images", "regions", "gray_host", "device"):
        assert re.search(r"\bint\s+mocr_recognize_" + k + r"_beam_soft\s*\(", hdr)
        assert _capi.SYMBOLS[f"mocr_recognize_{k}_beam_soft"] == _capi.SYMBOLS[f"mocr_recognize_{k}_beam_automaton"]
    m = re.search(r"\bint\s+mocr_op_beam_select_soft\s*\(([^;]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == len(_capi.SYMBOLS["mocr_op_beam_select_soft"][1])
    assert _capi.SYMBOLS["mocr_op_beam_select_soft"][1] == _capi.SYMBOLS["mocr_op_beam_select_automaton"][1] + [_capi._P] * 2
    assert "beam search under soft token automata" in hdr and "beam_select_sw" in hdr
    src = open(os.path.join(ROOT, "manga-ocr_amd", "csrc", "kernels_beam.h")).read()
    assert "bool AUT = false, bool SOFT = false>" in src and "struct BeamSoftAutomata : BeamAutomata" in src


# ------------------------------------------------------------------------------------------------ Engine on a recording library
def test_beam_soft_picks_the_soft_symbols_and_nothing_else_moves(rec):  # noqa: F811
    eng = object.__new__(Engine)
    eng.lib, eng.spec, eng._h, eng.max_batch = rec.RecordingLib(), DEFAULT_SPEC, C.c_void_p(0), 12
    gray = np.zeros((3, 224, 224), np.uint8)
    cfg = BeamConfig(3)
    eng.recognize_gray(gray, 16, beam=cfg, beam_automata=[4, None, 5], beam_states=True)
    out = eng.recognize_gray(gray, 16, beam=cfg, beam_automata=[4, None, 5], beam_states=True, beam_soft=True)
    assert len(out) == 4 and out[3].shape == (3, 3)
    a, b = eng.lib.calls
    assert a["symbol"] == "mocr_recognize_gray_host_beam_automaton" and b["symbol"] == "mocr_recognize_gray_host_beam_soft"
    assert len(a["args"]) == len(b["args"]) == 13 and [type(x) for x in a["args"]] == [type(x) for x in b["args"]]
    eng.lib.calls.clear()
    eng.recognize_images([np.zeros((8, 8), np.uint8)] * 2, beam=cfg, beam_automata=7, beam_soft=True)
    eng.recognize_regions([np.zeros((32, 48, 3), np.uint8)], [(0, 1, 2, 8, 8)], beam=cfg, beam_soft=True)
    eng.recognize_device(0x1000, 2, 0x2000, 0x3000, beam=cfg, d_out_score=0x8000, beam_automata=[1, 2], beam_soft=True)
    assert [c["symbol"] for c in eng.lib.calls] == [f"mocr_recognize_{k}_beam_soft" for k in ("images", "regions", "device")]
    assert eng.lib.calls[1]["args"][-2:] == ["null", "null"], "the flag alone: the soft symbol with nothing asked"
    eng.lib.calls.clear()
    with pytest.raises(ValueError):
        eng.recognize_gray(gray, 16, beam_soft=True)
    with pytest.raises(ValueError):
        eng.recognize_gray(gray, 16, beam=cfg, beam_soft=True, automata=[1, 2, 3])
    assert not eng.lib.calls, "a refused call reached the library"

    class HookLib:
        def mocr_op_beam_select_soft(self, *a):
            self.seen = a
            return _capi.MOCR_OK
    eng.lib = HookLib()
    eng.op_beam_select_soft(cfg, 1, 2, 3, 4, 5, 6, d_edge_weight=7, d_default_next=8, n=4)
    assert len(eng.lib.seen) == 24 and eng.lib.seen[-2].value == 7 and eng.lib.seen[-1].value == 8


# ------------------------------------------------------------------------------------------------ MangaOcr on a fake engine
def test_search_on_a_fake_engine(rec):  # noqa: F811
    eng = _fake_engine(rec)
    soft_made = []
    hard_automaton = eng.automaton

    def automaton(eb, et, en, acc, edge_weight=None, default_next=None):
        h = hard_automaton(eb, et, en, acc)
        if edge_weight is not None or default_next is not None:
            soft_made.append(h)
        return h
    eng.automaton = automaton
    ocr = rec._ocr(eng, max_batch=16)
    try:
        from manga_ocr.ocr import MangaOcr
        assert not [m for m in ("search", "search_batch", "search_bgr", "search_regions") if not hasattr(MangaOcr, m)]
        tok = lambda i: ocr.vocab.tokens[i]
        gl = ocr.glossary([tok(10) + tok(20), tok(11) + tok(21)], bonus=2.0)
        assert gl.soft and soft_made == [gl.handle]
        imgs = [rec._img(i) for i in range(3)]
        got = ocr.search_batch(imgs, gl)
        call = eng.calls[-1]
        assert call[0] == "recognize_images" and call[2]["beam"] == (4, 1.0, 0, 0) and call[2]["beam_automata"] == [gl.handle] * 3
        assert call[2]["beam_states"] and call[2]["beam_soft"] is True
        assert "beam_scores" not in call[2] and "beam_sets" not in call[2] and "beam_positions" not in call[2], "only what was asked"
        assert [len(r) for r in got] == [4, 4, 4], "the hypotheses as the engine delivered them"
        assert all(h.accepted is None and h.entry is None and h.state is not None for r in got for h in r)
        assert [h.sequence_score for h in got[0][:2]] == [-1.0, -2.0] and gl.find(got[0][0].ids) == [(1, 0)]
        # a hard Lexicon is allowed and marks its hypotheses as match does; per-crop lexicons; the keywords travel
        lx = ocr.lexicon([tok(10) + tok(20), tok(10)])
        per = ocr.search_batch(imgs, [lx, None, gl], k=3, length_penalty=2.0, early_stopping=True, no_repeat_ngram=3, token_scores=True, positions=True)
        call = eng.calls[-1]
        assert call[2]["beam"] == (3, 2.0, 1, 3) and call[2]["beam_automata"] == [lx.handle, 0, gl.handle] and call[2]["beam_soft"] is True
        assert call[2]["beam_scores"] and call[2]["beam_positions"] and len(per[2][0].logprobs) == 3 and per[2][0].positions is not None
        assert all(h.accepted is False and h.state == -1 for h in per[1]) and [h.accepted for h in per[0]][:2] == [True, True]
        assert [h.entry for h in per[0]][:2] == [0, 1] and all(h.accepted is None for h in per[2])
        # one crop goes through the batcher with the flag; bgr crops and regions
        one = ocr.search(imgs[0], gl, k=2)
        assert len(one) == 2 and eng.calls[-1][2]["beam_soft"] is True and eng.calls[-1][2]["beam_automata"] == [gl.handle]
        assert len(ocr.search_bgr([np.zeros((8, 8, 3), np.uint8)], gl)[0]) == 4
        regs = ocr.search_regions([np.zeros((32, 48, 3), np.uint8)], [(0, 1, 2, 8, 8), (0, 3, 4, 0, 8)], gl)
        assert eng.calls[-1][0] == "recognize_regions" and len(regs[0]) == 4 and regs[1] == []
        # match keeps refusing the soft lexicon and names search; match on a hard one makes the call it made
        before = len(eng.calls)
        with pytest.raises(ValueError, match="search"):
            ocr.match_batch(imgs, gl)
        with pytest.raises(ValueError):
            ocr.search_batch(imgs, None)
        assert len(eng.calls) == before
        ocr.match_batch(imgs, lx)
        assert "beam_soft" not in eng.calls[-1][2]
        ocr.match(imgs[0], lx)
        assert "beam_soft" not in eng.calls[-1][2]
    finally:
        ocr._batcher.close()
