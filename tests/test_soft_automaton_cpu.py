"""CPU: soft token automata (include/mocr.h, "soft token automata") - the dictionary-of-dictionaries reference of
tests/bias_util.py, the Aho-Corasick compilation of manga_ocr/text.py (``bias_automaton``) against transformers' own
``SequenceBiasLogitsProcessor``, the goldens of tests/golden/make_bias_goldens.py against the reference loop on the oracle, the
``glossary`` construction and ``Lexicon.find``, the refusals, and - against a recording engine, as tests/test_surface_cpu.py
does - that with default arguments ``pack_automaton``, ``Engine.automaton`` and ``MangaOcr.automaton`` make the calls they made."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import automaton_util as au
import bias_util as bu
import constraint_util as cu
import score_util as su
from manga_ocr import _capi
from manga_ocr.engine import Engine
from manga_ocr.ocr import Lexicon
from manga_ocr.text import bias_automaton, pack_automaton
from manga_ocr.weights import DEFAULT_SPEC, spec_from_hf_config, synthetic_weights

V, EOS, START = au.V, au.EOS, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def rec():
    spec = importlib.util.spec_from_file_location("make_surface_golden", os.path.join(GOLDEN, "make_surface_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ the reference
def test_open_states_weights_and_the_walk():
    a = bu.SoftAutomaton({0: {100: 1, 101: 0}, 1: {102: 2}}, [0, 2], {0: {100: 1.5, 101: -6.0}, 1: {102: 0.25}}, {0: 0, 1: 0}, 3)
    assert a.is_open(0) and a.is_open(1) and not a.is_open(2) and not a.is_open(bu.DEAD)
    assert a.allowed(0).sum() == V and a.allowed(1).sum() == V - 1 and not a.allowed(1)[EOS], "open: every token, EOS iff accepting"
    assert a.allowed(2).sum() == 1 and a.allowed(2)[EOS] and not a.allowed(bu.DEAD).any(), "closed: its edges, as before"
    assert a.next(0, 100) == 1 and a.next(0, 7) == 0 and a.next(1, 7) == 0 and a.next(2, 7) == bu.DEAD and a.next(bu.DEAD, 100) == bu.DEAD
    assert a.walk([100, 102]) == 2 and a.walk([100, 5, 100, EOS]) == 1 and a.walk([100, 102, 100]) == bu.DEAD
    lg = np.zeros(V, np.float32)
    w = bu.step_logits(a, 0, lg)
    assert w.dtype == np.float32 and w[100] == 1.5 and w[101] == -6.0 and np.count_nonzero(w) == 2
    assert not bu.step_logits(a, 2, lg).any() and not bu.step_logits(a, bu.DEAD, lg).any() and not bu.step_logits(None, bu.NONE, lg).any()
    # the effective set: A(s) AND the base set, minus the bans, {EOS} if empty - au.step_mask on the open A(s)
    base = cu.mask_of([100, 200])
    assert au.step_mask(a, 0, [START, 100], 1, base).tolist() == cu.mask_of([200]).tolist()
    assert au.step_mask(a, 1, [START, 100, 200], 1, base).sum() == 1, "nothing left under a non-accepting open state: {EOS}"
    # the packer: CSR plus the two arrays, global numbers behind another automaton
    eb, et, en, acc, ew, dn = bu.pack(a)
    assert et.tolist() == [100, 101, 102] and ew.tolist() == [1.5, -6.0, 0.25] and dn.tolist() == [0, 0, -1] and ew.dtype == np.float32
    many = bu.pack_many([au.loop([5, 6]), a])
    assert many[5].tolist() == [-1, -1, -1, 3, 3, -1] and many[4].tolist() == [0.0] * 6 + [1.5, -6.0, 0.25] and many[6] == [0, 3]
    u = bu.universal_open()
    assert u.allowed(0).all() and u.next(0, 9) == 0 and not u.bias(0).any()
    # manga_ocr.text.pack_automaton is the same form, and with the defaults the form it always was
    mine = pack_automaton(a.trans, a.accepting, weights=a.weights, default=a.default)
    for got, want in zip(mine, bu.pack(a)):
        assert list(got) == want.tolist()
    assert pack_automaton(a.trans, a.accepting) == tuple(x.tolist() for x in au.pack(a)) and len(pack_automaton(a.trans, a.accepting)) == 4
    assert pack_automaton({0: {9: 1, 5: 1}}, [1]) == ([0, 2, 2], [5, 9], [1, 1], [0, 1])
    assert pack_automaton({0: {5: 0}}, [0], default=0)[4:] == ([0.0], [0]) and pack_automaton({}, [0], weights={})[4:] == ([], [-1])
    for bad in (dict(weights={0: {7: 1.0}}), dict(default={0: 5}, n_states=2), dict(default=True), dict(default=1.5)):
        with pytest.raises(ValueError):
            pack_automaton({0: {5: 0}}, [0], **bad)


def _random_bias(rs, vocab):
    sb = {}
    for _ in range(rs.randint(1, 9)):
        sb[tuple(int(t) for t in rs.randint(0, vocab, size=rs.randint(1, 5)))] = int(rs.randint(-40, 41)) / 8.0
    return sb


def test_bias_automaton_is_transformers_sequence_bias():
    """300 random sets of one to eight sequences over 6 tokens (so that they overlap and nest), biases multiples of 1/8,
    walked for 12 random steps: at every step the state's weights ARE SequenceBiasLogitsProcessor's bias vector, exactly."""
    pytest.importorskip("transformers")
    rs = np.random.RandomState(5)
    fired = 0
    for trial in range(300):
        sb = _random_bias(rs, 6)
        a = bu.from_sequence_bias(sb)
        assert all(a.is_open(s) and s in a.accepting for s in range(a.n_states)), "every state open and accepting"
        hist, s = [], 0
        for step in range(12):
            want = bu.hf_bias_vector(sb, hist, 64)
            got = a.bias(s)[:64]
            np.testing.assert_array_equal(got, want, err_msg=f"{sb} after {hist}")
            fired += int(np.count_nonzero(want) > 0)
            t = int(rs.randint(0, 6))
            hist.append(t)
            s = a.next(s, t)
            assert s >= 0
    assert fired > 2000


def test_bias_automaton_is_the_frozen_processor_vectors():
    """The same comparison without transformers: tests/golden/bias_vectors.npz holds SequenceBiasLogitsProcessor's vectors for 60
    random sets at every step of a random history (tests/golden/make_bias_goldens.py vectors).  Flat and compact form."""
    g = np.load(os.path.join(GOLDEN, "bias_vectors.npz"))
    fired = 0
    for k in range(len(g["hist"])):
        sb = {tuple(int(t) for t in row if t >= 0): float(b) for row, b in zip(g["seq_tok"][k], g["seq_bias"][k]) if row[0] >= 0}
        for compact in (False, True):
            a = bu.from_sequence_bias(sb, compact=compact)
            s = 0
            for step, t in enumerate(g["hist"][k]):
                np.testing.assert_array_equal(a.bias(s)[:64], g["vec"][k, step], err_msg=f"{sb} after {g['hist'][k, :step]} (compact={compact})")
                fired += int(g["vec"][k, step].any())
                s = a.next(s, int(t))
    assert fired > 800


def test_compact_bias_automaton_is_the_flat_one_with_fewer_edges():
    """bias_automaton(compact=True) under the fallback walk (MOCR_DEFAULT_FALLBACK: a token without an edge takes the default
    state's edge) against the flat form under the plain walk: the same state numbers, the same next state for every (state,
    token), the same weights; its edges are a subset of the flat ones, and an edge it leaves out weighs nothing.  Then the size
    that matters: 8,000 random words over 200 first tokens - the flat form would need states x 200 edges, beyond the engine's
    2^22; the compact one, which keeps the weighted continuations a state inherits (here every token is some word's first, so
    a state inherits the ~40 children of its last token's node), takes less than a quarter of that and of the arena."""
    rs = np.random.RandomState(9)
    for trial in range(200):
        sb = _random_bias(rs, 6)
        flat, comp = bu.from_sequence_bias(sb), bu.from_sequence_bias(sb, compact=True)
        assert comp.fallback and not flat.fallback and comp.n_states == flat.n_states
        for s in range(flat.n_states):
            assert set(comp.trans.get(s, {}).items()) <= set(flat.trans[s].items())
            assert all(flat.weights[s].get(t, 0.0) == 0.0 for t in set(flat.trans[s]) - set(comp.trans.get(s, {})))
            np.testing.assert_array_equal(comp.bias(s), flat.bias(s))
            for t in range(7):
                assert comp.next(s, t) == flat.next(s, t), (sb, s, t)
        if trial == 0:
            assert (bu.pack(comp)[5] == bu.FALLBACK).all() and (bu.pack(flat)[5] == 0).all()
            mine = pack_automaton(comp.trans, comp.accepting, weights=comp.weights, default=0, fallback=True)
            assert list(mine[5]) == bu.pack(comp)[5].tolist() and bu.pack_many([au.loop([5]), comp])[5][3] == (3 | bu.FALLBACK)
    alphabet = rs.choice(np.arange(5, V), size=200, replace=False)
    words = [tuple(int(t) for t in alphabet[rs.randint(0, 200, size=rs.randint(2, 9))]) for _ in range(8000)]
    trans, weights = bias_automaton({w[:n]: 2.0 for w in words for n in range(2, len(w) + 1)}, compact=True)
    edges = sum(len(e) for e in trans.values())
    assert len(trans[0]) == 200 and len(trans) * 200 > _capi.MAX_AUTOMATON_EDGES > 4 * edges and len(trans) * 200 > 4 * edges, (len(trans), edges)


def test_bias_automaton_sums_in_float64_and_rounds_once():
    sb = {(7,): 0.1, (5, 7): 0.2, (6, 5, 7): 0.3}
    trans, weights = bias_automaton(sb)
    s = 0
    for t in (6, 5):
        s = trans[s].get(t, 0)
    assert weights[s][7] == 0.1 + 0.2 + 0.3 or weights[s][7] == (0.3 + 0.2) + 0.1, "three overlapping sequences add"
    assert np.float32(weights[s][7]) == np.float32(0.6000000000000001)
    assert weights[0] == {7: 0.1} and weights[trans[0][5]][7] == pytest.approx(0.3)
    with pytest.raises(ValueError):
        bias_automaton({(): 1.0})


# ------------------------------------------------------------------------------------------------ the goldens
@pytest.mark.parametrize("case", ["a", "b", "e"])
def test_the_reference_loop_reproduces_transformers_goldens(case):
    """tests/golden/bias_*.npz - transformers' generate(sequence_bias=...) - against bias_util.soft_generate on the oracle's
    logits under text.bias_automaton's compilation: ids and lengths exactly, token scores within bias_util.SCORE_TOL."""
    import torch
    from gpu_util import oracle
    from oracle.mocr_oracle import Oracle
    g = np.load(os.path.join(GOLDEN, f"bias_{case}.npz"))
    sb = {tuple(int(t) for t in g["seq_tok"][i, :g["seq_len"][i]]): float(g["seq_bias"][i]) for i in range(len(g["seq_len"]))}
    a = bu.from_sequence_bias(sb)
    o = Oracle(synthetic_weights(int(g["weights_seed"]), eos_bias=float(g["eos_bias"])), DEFAULT_SPEC)
    gray = np.stack([np.random.RandomState(int(s)).randint(0, 256, size=(224, 224), dtype=np.uint8) for s in g["crop_seeds"]])
    ML, B = int(g["max_length"]), len(gray)
    with torch.no_grad():
        enc = o.encode(o.preprocess_gray(gray))
    ids, wl, pl, masks, state, _ = bu.soft_generate(o, enc, [a] * B, np.ones((B, V), bool), [0] * B, ML)
    lens = bu.lengths(ids, EOS)
    np.testing.assert_array_equal(lens, g["lens"])
    np.testing.assert_array_equal(state, g["state"])
    worst = 0.0
    for b in range(B):
        np.testing.assert_array_equal(ids[b, :lens[b]], g["ids"][b, :lens[b]])
        lp = su.log_softmax64(wl[b, :lens[b] - 1])[np.arange(lens[b] - 1), ids[b, 1:lens[b]]]
        worst = max(worst, float(np.abs(lp - g["logp"][b, 1:lens[b]]).max()))
    assert worst <= bu.SCORE_TOL, worst
    assert int(g["changed"]) * 2 >= B and (case != "e" or (lens < ML).all()), "the sequences fire, and case e ends early"
    assert any(len(k) == 1 for k in sb) == (case != "b") and (case == "b" or min(sb.values()) < 0)


# ------------------------------------------------------------------------------------------------ Engine on a recording library
def test_engine_automaton_makes_the_call_it_made_unless_asked(rec):
    eng = object.__new__(Engine)
    eng.spec, eng._h, eng.max_batch = DEFAULT_SPEC, C.c_void_p(0), 9

    class CreateLib:
        def mocr_automaton_create(self, h, desc, out):
            d = desc._obj if hasattr(desc, "_obj") else desc.contents
            self.size = d.struct_size
            self.seen = (d.n_states, np.ctypeslib.as_array((C.c_int32 * 3).from_address(d.edge_begin)).tolist(),
                         (C.c_int32 * 1).from_address(d.edge_token)[0], (C.c_int32 * 1).from_address(d.edge_next)[0],
                         list((C.c_uint8 * 2).from_address(d.accepting)))
            self.soft = None
            if d.struct_size >= C.sizeof(_capi.MocrSoftAutomatonDesc):
                sd = C.cast(desc, C.POINTER(_capi.MocrSoftAutomatonDesc)).contents
                self.soft = (None if not sd.edge_weight else (C.c_float * 1).from_address(sd.edge_weight)[0],
                             None if not sd.default_next else list((C.c_int32 * 2).from_address(sd.default_next)))
            out._obj.value = 3
            return _capi.MOCR_OK
    eng.lib = CreateLib()
    assert eng.automaton([0, 1, 1], [5], [1], [False, 7]) == 3
    assert eng.lib.size == C.sizeof(_capi.MocrAutomatonDesc) == 40 and eng.lib.soft is None, "the default call passes the struct as it was"
    assert eng.lib.seen == (2, [0, 1, 1], 5, 1, [0, 1])
    assert eng.automaton([0, 1, 1], [5], [1], [False, 7], edge_weight=[0.5], default_next=[1, -1]) == 3
    assert eng.lib.size == C.sizeof(_capi.MocrSoftAutomatonDesc) == 56 and eng.lib.soft == (0.5, [1, -1]) and eng.lib.seen == (2, [0, 1, 1], 5, 1, [0, 1])
    assert eng.automaton([0, 1, 1], [5], [1], [1, 1], default_next=[0, 0]) == 3 and eng.lib.soft == (None, [0, 0])
    assert eng.automaton_used() == (6, 3), "the states and edges of every create so far"
    assert eng.automaton([0, 1, 1], [5], [1], [1, 1], edge_weight=[2]) == 3 and eng.lib.soft == (2.0, None)
    for bad in (dict(edge_weight=[1.0, 2.0]), dict(default_next=[0])):
        with pytest.raises(ValueError):
            eng.automaton([0, 1, 1], [5], [1], [1, 1], **bad)
    assert _capi.MocrSoftAutomatonDesc.edge_weight.offset == C.sizeof(_capi.MocrAutomatonDesc)
    for name in ("mocr_op_dec_token_soft", "mocr_op_automaton_init_soft", "mocr_op_gemm_argmax_soft"):
        assert name in _capi.SYMBOLS
    assert len(_capi.SYMBOLS["mocr_op_dec_token_soft"][1]) == len(_capi.SYMBOLS["mocr_op_dec_token_automaton"][1]) + 2


# ------------------------------------------------------------------------------------------------ MangaOcr on a fake engine
def _fake_engine(rec):
    class SoftEngine(rec.RecordingEngine):
        """the recorder's engine plus automata, soft ones included: rows read START, 10 + r, 20 + r, EOS"""

        def __init__(self):
            super().__init__()
            self.auts = [None]

        def automaton(self, eb, et, en, acc, edge_weight=None, default_next=None):
            a = au.unpack(*(np.asarray(x) for x in (eb, et, en, acc)))
            if edge_weight is not None or default_next is not None:
                w = {s: {int(et[i]): float(edge_weight[i]) for i in range(eb[s], eb[s + 1])} for s in range(len(acc))} if edge_weight is not None else None
                d = {s: int(x) & (bu.FALLBACK - 1) if x >= 0 else -1 for s, x in enumerate(default_next)} if default_next is not None else None
                fb = default_next is not None and any(int(x) >= bu.FALLBACK for x in default_next)
                a = bu.SoftAutomaton(a.trans, a.accepting, w, d, len(acc), fallback=fb)
            self.auts.append(a)
            self.calls.append(["automaton", len(acc), len(et)] + ([] if edge_weight is None and default_next is None
                                                                   else [edge_weight is not None, default_next is not None]))
            return len(self.auts) - 1

        def _answer(self, method, args, kw, sliver):
            kw = dict(kw)
            handles, states = kw.pop("automata", None), kw.pop("states", False)
            out = super()._answer(method, args, kw, sliver)
            if handles is not None:
                self.calls[-1].append({"automata": list(handles), "states": states})
            if not states:
                return out
            ids, lens = out[0], out[1]
            st = [au.NONE if not h or not lens[r] else self.auts[h].walk(ids[r, 1:lens[r]]) for r, h in enumerate(handles)]
            return out + (np.array(st, np.int32),)
    return SoftEngine()


def test_sequence_bias_glossary_and_find_on_a_fake_engine(rec):
    eng = _fake_engine(rec)
    ocr = rec._ocr(eng)
    try:
        tok = lambda i: ocr.vocab.tokens[i]
        # the raw form: with the defaults the call it made, with weights / default a soft one
        hard = ocr.automaton({0: {10: 1}, 1: {20: 2, 21: 2}}, [2])
        assert eng.calls == [["automaton", 3, 3]] and hard == Lexicon(1, frozenset([2]), {}, ()) and not hard.soft
        soft = ocr.automaton({0: {10: 1}, 1: {20: 0}}, [0, 1], weights={1: {20: 2.5}}, default=0)
        assert eng.calls[-1] == ["automaton", 2, 2, True, True] and soft.soft and soft.handle == 2
        a = eng.auts[2]
        assert a.weights == {0: {10: 0.0}, 1: {20: 2.5}} and a.default == {0: 0, 1: 0}
        # sequence_bias: texts and id tuples, overlapping sequences, every state open and accepting
        lx = ocr.sequence_bias({tok(10) + tok(20): 2.0, (20,): -1.0, (11, 10, 20): 0.5})
        a = eng.auts[lx.handle]
        assert a.fallback and lx.soft and lx.texts == () and all(a.is_open(s) and s in a.accepting for s in range(a.n_states))
        assert a.bias(a.walk([11, 10]))[20] == 1.5 and a.bias(a.walk([10]))[20] == 1.0 and a.bias(0)[20] == -1.0
        imgs = [rec._img(i) for i in range(3)]
        recs = ocr.recognize_batch_scored(imgs, lexicon=lx)
        assert eng.calls[-1][0] == "recognize_images" and eng.calls[-1][2] == {"scores": True} and \
            eng.calls[-1][3] == {"automata": [lx.handle] * 3, "states": True}, "no new keyword: the lexicon= path as it is"
        assert [r.accepted for r in recs] == [None] * 3 and [r.entry for r in recs] == [None] * 3 and all(r.state >= 0 for r in recs)
        assert recs[0].state == a.walk([10, 20]) and recs[0].text == tok(10) + tok(20)
        mixed = ocr.recognize_batch_scored(imgs, lexicon=[hard, lx, None])
        assert mixed[0].accepted is True and mixed[1].accepted is None and mixed[2].state == au.NONE and not mixed[2].accepted
        # the glossary: prefixes of two or more tokens, shared prefixes once, the first token only with start_bonus
        texts = [tok(10) + tok(20) + tok(30), tok(10) + tok(20) + tok(31), tok(12), tok(11) + " " + tok(21)]
        n0 = len(eng.calls)
        gl = ocr.glossary(texts, bonus=1.5)
        a = eng.auts[gl.handle]
        assert gl.soft and gl.texts == tuple(texts) and gl.spellings == ((10, 20, 30), (10, 20, 31), (12,), (11, 21)) and len(eng.calls) == n0 + 1
        assert a.bias(0).sum() == 0, "a name is not suggested out of nothing"
        assert a.bias(a.walk([10]))[20] == 1.5 and np.count_nonzero(a.bias(a.walk([10]))) == 1, "a shared prefix counts once"
        b = a.bias(a.walk([10, 20]))
        assert b[30] == 1.5 and b[31] == 1.5 and np.count_nonzero(b) == 2 and a.bias(a.walk([11]))[21] == 1.5
        assert a.bias(a.walk([5, 10]))[20] == 1.5 and not a.bias(a.walk([10, 20, 30])).any(), "anywhere in the row; nothing behind an entry"
        gs = ocr.glossary(texts, bonus=1.0, start_bonus=0.25)
        a = eng.auts[gs.handle]
        assert a.bias(0)[[10, 11, 12]].tolist() == [0.25] * 3 and a.bias(a.walk([10]))[20] == 1.0 and a.bias(a.walk([10]))[10] == 0.25
        # find: every entry contained in a row, by position then entry
        assert gl.find([START, 10, 20, 30, 12, 11, 21, 10, 20, 31, EOS, 0, 0]) == [(1, 0), (4, 2), (5, 3), (7, 1)]
        assert gl.find([START, 10, 20, EOS]) == [] and hard.find([10, 20]) == [] and gl.find(np.array([12, 12])) == [(0, 2), (1, 2)]
        got = ocr.recognize_scored(imgs[0], lexicon=gl)
        assert got.accepted is None and gl.find(got.ids) == []
        # the refusals
        for bad in ({}, {tok(10) + "#": 1.0}, {(10, EOS): 1.0}, {(START,): 1.0}, {(0, 10): 1.0}, {(10,): float("nan")}, {(10,): float("inf")},
                    {(V,): 1.0}, {(): 1.0}, {"  ": 1.0}, {(10,): True}, [((10,), 1.0)]):
            with pytest.raises(ValueError):
                ocr.sequence_bias(bad)
        for bad in ([], [tok(10), "#"], [tok(10), " "], [tok(12)]):
            with pytest.raises(ValueError):
                ocr.glossary(bad)
        # an automaton beyond what an engine holds is refused here, by name and with the figures, not by the library's code
        import manga_ocr.ocr as ocr_mod
        n2, cap = len(eng.calls), ocr_mod.MAX_AUTOMATON_EDGES
        ocr_mod.MAX_AUTOMATON_EDGES = 5
        try:
            with pytest.raises(ValueError, match="6 edges; an engine holds"):
                ocr.glossary(texts, bonus=1.5)
        finally:
            ocr_mod.MAX_AUTOMATON_EDGES = cap
        assert len(eng.calls) == n2
        # ... and the tables are shared: what the engine's earlier automata have taken counts
        eng.automaton_used = lambda: (0, cap - 5)
        try:
            with pytest.raises(ValueError, match=f"over ALL its automata, and the earlier ones have taken 0 states and {cap - 5} edges"):
                ocr.glossary(texts, bonus=1.5)
        finally:
            del eng.automaton_used
        assert len(eng.calls) == n2
        with pytest.raises(ValueError, match="weight on a token without an edge"):
            ocr.automaton({0: {10: 0}}, [0], weights={0: {11: 1.0}})
        n1 = len(eng.calls)
        for name, args in (("match", (imgs[0],)), ("match_batch", (imgs,))):
            if hasattr(ocr, name):
                with pytest.raises(ValueError, match="soft"):
                    getattr(ocr, name)(*args, lexicon=gl)
        assert len(eng.calls) == n1, "a refused match reached the engine"
    finally:
        ocr._batcher.close()


def test_the_loader_names_a_checkpoints_sequence_bias():
    import json
    import warnings
    from hf_dir import write_hf_dir
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        write_hf_dir(d)
        with open(os.path.join(d, "config.json")) as f:
            cfg = json.load(f)
    cfg["sequence_bias"] = [[[10, 20], 2.0], [[7], -1.5]]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        spec = spec_from_hf_config(cfg)
    ignored = dict(spec.ignored_generation)
    assert ignored["sequence_bias"] == (((10, 20), 2.0), ((7,), -1.5)) and "num_beams" in ignored and any("sequence_bias" in str(x.message) for x in w)
    hash(spec)
    del cfg["sequence_bias"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert "sequence_bias" not in dict(spec_from_hf_config(cfg).ignored_generation)
