"""CPU: token automata (include/mocr.h, "token automata") - the reference helpers of tests/automaton_util.py, the trie builder
and CSR packer of manga_ocr/text.py, the Engine keywords on a recording library and the MangaOcr surface (``lexicon``,
``automaton``, ``lexicon=``, ``Recognition.state`` / ``accepted`` / ``entry``) on a fake engine, in the style of the surface
recorder (tests/golden/make_surface_golden.py), and the refusals."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import automaton_util as au
import constraint_util as cu
from manga_ocr import _capi
from manga_ocr.engine import BeamConfig, Engine
from manga_ocr.ocr import Lexicon
from manga_ocr.text import Vocab, lexicon_trie, pack_automaton
from manga_ocr.weights import DEFAULT_SPEC

V, EOS, START = au.V, au.EOS, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def rec():
    """the surface recorder's fakes"""
    spec = importlib.util.spec_from_file_location("make_surface_golden", os.path.join(GOLDEN, "make_surface_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _words(seed=1, count=120, alphabet=range(100, 110)):
    rs = np.random.RandomState(seed)
    return [[int(t) for t in np.asarray(list(alphabet))[rs.randint(0, 10, size=rs.randint(2, 9))]] for _ in range(count)]


# ------------------------------------------------------------------------------------------------ the reference
def test_the_packer_round_trips():
    words = _words()
    trie, entry = au.trie(words)
    for a in (trie, au.loop([5, 6, 7, 9]), au.universal(), au.Automaton({0: {7: 1}}, [], 3)):
        eb, et, en, acc = au.pack(a)
        assert eb[0] == 0 and (np.diff(eb) >= 0).all() and eb[-1] == len(et) == len(en) and len(acc) == a.n_states == len(eb) - 1
        for s in range(a.n_states):
            assert (np.diff(et[eb[s]:eb[s + 1]]) > 0).all(), "a state's tokens are strictly ascending"
        back = au.unpack(eb, et, en, acc)
        assert back.trans == {s: e for s, e in a.trans.items() if e} and back.accepting == a.accepting and back.n_states == a.n_states
    # several automata behind each other, as the engine's arena holds them
    auts = [trie, au.loop([5, 6]), au.universal()]
    eb, et, en, acc, first = au.pack_many(auts)
    assert first == [0, trie.n_states, trie.n_states + 3] and len(acc) == trie.n_states + 4 and eb[-1] == len(et)
    for a, f in zip(auts, first):
        for s in range(a.n_states):
            got = {int(et[i]): int(en[i]) - f for i in range(eb[f + s], eb[f + s + 1])}
            assert got == a.trans.get(s, {}) and bool(acc[f + s]) == (s in a.accepting)
    # manga_ocr.text.pack_automaton is the same form
    mine = pack_automaton(trie.trans, trie.accepting)
    for got, want in zip(mine, au.pack(trie)):
        assert list(got) == want.tolist()


def test_every_entry_walks_to_an_accepting_state_and_non_entries_die():
    words = _words()
    trie, entry = au.trie(words)
    assert 300 <= trie.n_states <= 700 and set(entry) == trie.accepting
    for k, w in enumerate(words):
        s = trie.walk(w)
        assert s in trie.accepting and words[entry[s]] == w and entry[s] <= k
        assert trie.walk(w + [EOS]) == s, "EOS moves nothing"
    known = {tuple(w) for w in words}
    prefixes = {tuple(w[:i]) for w in words for i in range(len(w) + 1)}
    rs = np.random.RandomState(9)
    died = inner = 0
    for _ in range(400):
        w = tuple(int(t) for t in rs.randint(100, 110, size=rs.randint(1, 10)))
        s = trie.walk(w)
        if w in known:
            assert s in trie.accepting
        elif w in prefixes:
            assert s >= 0 and s not in trie.accepting
            inner += 1
        else:
            assert s == au.DEAD and trie.walk(w + (100,)) == au.DEAD, "a dead row stays dead"
            died += 1
    assert died > 50 and inner > 5
    assert trie.walk([4000]) == au.DEAD and not trie.allowed(au.DEAD).any()
    a0 = trie.allowed(0)
    assert a0.sum() == len(trie.trans[0]) and not a0[EOS]
    leaf = next(s for s in trie.accepting if not trie.trans.get(s))
    assert trie.allowed(leaf).sum() == 1 and trie.allowed(leaf)[EOS]
    u = au.universal()
    assert u.allowed(0).all() and u.walk(range(4, 200)) == 0


def test_the_dead_end_and_forced_token_rules_of_the_reference():
    loop = au.loop([5, 6, 7, 8])
    full = np.ones(V, bool)
    # a base set disjoint from the state's edges: {EOS}, although the state does not accept
    base = cu.mask_of([100, 101])
    m = au.step_mask(loop, 0, [START], 0, base)
    assert m.sum() == 1 and m[EOS]
    # the automaton takes EOS away where the state does not accept, and only it can
    m = au.step_mask(loop, 1, [START, 5], 0, full)
    assert sorted(np.nonzero(m)[0]) == [5, 6, 7, 8]
    m = au.step_mask(loop, 2, [START, 5, 6], 0, full)
    assert sorted(np.nonzero(m)[0]) == [EOS, 5, 6, 7, 8]
    # bans: behind "5 6 5" the bigram rule bans 6; with every edge banned and no EOS the dead-end rule gives {EOS}
    m = au.step_mask(loop, 2, [START, 5, 6, 5], 2, full)
    assert sorted(np.nonzero(m)[0]) == [EOS, 5, 7, 8]
    one = au.Automaton({0: {5: 0}}, [], 1)
    m = au.step_mask(one, 0, [START, 5], 1, full)
    assert m.sum() == 1 and m[EOS], "the only edge is banned: the row ends"
    # a dead state allows nothing: {EOS}; a row without an automaton keeps the n-gram rule and no dead-end rule
    m = au.step_mask(loop, au.DEAD, [START, 4000], 0, full)
    assert m.sum() == 1 and m[EOS]
    assert au.step_mask(None, au.NONE, [START, 5], 0, base).sum() == base.sum()
    # a forced token walks like an emitted one; one without an edge leaves the row dead
    assert loop.walk([5, 4000]) == au.DEAD and loop.walk([5, 6, 7]) == 2 and loop.next(au.DEAD, 5) == au.DEAD
    ok, end = au.is_path(loop, [START, 5, 6, EOS], 4)
    assert ok and end == 2
    assert not au.is_path(loop, [START, 5, EOS], 3)[0], "EOS from a state that does not accept"
    assert not au.is_path(loop, [START, 5, 9, 6], 4)[0], "a token without an edge"
    assert au.is_path(loop, [START, EOS], 2, base=base, eos_by_dead_end=True)[0]


# ------------------------------------------------------------------------------------------------ manga_ocr.text
def test_lexicon_trie_of_the_vocabulary():
    vocab = Vocab.synthetic(64)
    ch = [chr(0x4E00 + i) for i in range(8)]                # the tokens 5 .. 12
    texts = [ch[0] + ch[1], ch[0], ch[0] + ch[1] + ch[2], ch[3] + " " + ch[1], ch[0] + ch[1]]
    trans, entry = lexicon_trie(vocab, texts)
    a = au.unpack(*(np.asarray(x) for x in pack_automaton(trans, entry)))
    for k, t in enumerate(texts):
        s = a.walk(vocab.encode_chars(t))
        assert s in a.accepting and texts[entry[s]].replace(" ", "") == t.replace(" ", "")
    assert entry[a.walk(vocab.encode_chars(texts[4]))] == 0, "an entry given twice keeps its first index"
    assert a.walk([5]) in a.accepting and a.trans[a.walk([5])], "an accepting inner node"
    assert a.n_states == 6 and a.walk([6]) == au.DEAD
    with pytest.raises(ValueError):
        lexicon_trie(vocab, [])
    with pytest.raises(ValueError):
        lexicon_trie(vocab, [ch[0], "#"])
    with pytest.raises(ValueError):
        lexicon_trie(vocab, [ch[0], "  "])
    with pytest.raises(ValueError):
        pack_automaton({0: {5: 3}}, [1], n_states=2)
    assert pack_automaton({0: {9: 1, 5: 1}}, [1]) == ([0, 2, 2], [5, 9], [1, 1], [0, 1])


# ------------------------------------------------------------------------------------------------ Engine on a recording library
def test_engine_keywords_reach_the_automaton_symbols_only_when_asked(rec):
    eng = object.__new__(Engine)
    eng.lib, eng.spec, eng._h, eng.max_batch = rec.RecordingLib(), DEFAULT_SPEC, C.c_void_p(0), 9
    gray = np.zeros((3, 224, 224), np.uint8)
    eng.recognize_gray(gray, 16, scores=True)
    eng.recognize_gray(gray, 16, sources=[0, 1, 2, 2])
    assert [c["symbol"] for c in eng.lib.calls] == ["mocr_recognize_gray_host_positions", "mocr_recognize_gray_host_shared"]
    eng.lib.calls.clear()
    out = eng.recognize_gray(gray, 16, scores=True, automata=[4, None, 5], states=True)
    assert len(out) == 4 and out[3].dtype == np.int32 and out[3].tolist() == [-1, -1, -1]
    call, = eng.lib.calls
    assert call["symbol"] == "mocr_recognize_gray_host_automaton" and len(call["args"]) == 19
    assert call["args"][2:4] == [3, 3] and call["args"][4] == "null" and call["args"][5] == 16, "n_planes, n_rows, no source, max_len"
    assert call["args"][-2:] == ["ptr", "ptr"] and call["args"][-5:-2] == ["null", "null", 0], "no prefix; automata and out_state given"
    eng.lib.calls.clear()
    out = eng.recognize_images([np.zeros((8, 8), np.uint8)] * 2, sources=[1, 0, 1], automata=7)
    assert len(out) == 2 and out[0].shape[0] == 3
    call, = eng.lib.calls
    assert call["symbol"] == "mocr_recognize_images_automaton" and call["args"][2:4] == [2, 3] and call["args"][-2:] == ["ptr", "null"]
    eng.lib.calls.clear()
    eng.recognize_regions([np.zeros((32, 48, 3), np.uint8)], [(0, 1, 2, 8, 8)], states=True)
    eng.recognize_device(0x1000, 2, 0x2000, 0x3000, automata=[1, 2], d_out_state=0x9000)
    assert [c["symbol"] for c in eng.lib.calls] == ["mocr_recognize_regions_automaton", "mocr_recognize_device_automaton"]
    assert eng.lib.calls[0]["args"][-2:] == ["null", "ptr"] and eng.lib.calls[1]["args"][-2:] == ["ptr", "0x9000"]
    eng.lib.calls.clear()
    for bad, exc in ((dict(automata=[1, 2]), ValueError), (dict(automata="x"), TypeError), (dict(automata=[1.5, 2, 3]), TypeError),
                     (dict(automata=True), TypeError), (dict(automata=[1, 2, 3], beam=BeamConfig(2)), ValueError),
                     (dict(states=True, beam=BeamConfig(2)), ValueError)):
        with pytest.raises(exc):
            eng.recognize_gray(gray, 16, **bad)
    assert not eng.lib.calls, "a refused call reached the library"
    with pytest.raises(ValueError):
        eng.automaton([0, 1], [5, 6], [0, 0], [1])

    class CreateLib:
        def mocr_automaton_create(self, h, desc, out):
            d = desc._obj
            self.seen = (d.struct_size, d.n_states, np.ctypeslib.as_array((C.c_int32 * 3).from_address(d.edge_begin)).tolist(),
                         (C.c_int32 * 1).from_address(d.edge_token)[0], (C.c_int32 * 1).from_address(d.edge_next)[0],
                         list((C.c_uint8 * 2).from_address(d.accepting)))
            out._obj.value = 3
            return _capi.MOCR_OK
    eng.lib = CreateLib()
    assert eng.automaton([0, 1, 1], [5], [1], [False, 7]) == 3
    assert eng.lib.seen == (C.sizeof(_capi.MocrAutomatonDesc), 2, [0, 1, 1], 5, 1, [0, 1]) and eng.lib.seen[0] == 40


# ------------------------------------------------------------------------------------------------ MangaOcr on a fake engine
def _fake_engine(rec):
    class AutomatonEngine(rec.RecordingEngine):
        """the recorder's engine plus automata: ``automaton`` keeps the reference form of what it is given, and a call with
        ``automata`` / ``states`` walks every row's fixed ids (START, 10 + r, 20 + r, EOS) for the final state"""

        def __init__(self):
            super().__init__()
            self.auts = [None]

        def automaton(self, eb, et, en, acc):
            self.auts.append(au.unpack(*(np.asarray(x) for x in (eb, et, en, acc))))
            self.calls.append(["automaton", len(acc), len(et)])
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
    return AutomatonEngine()


def test_lexicon_on_a_fake_engine(rec):
    eng = _fake_engine(rec)
    ocr = rec._ocr(eng)
    try:
        tok = lambda i: ocr.vocab.tokens[i]
        # rows read START, 10 + r, 20 + r, EOS: entry 1 is row 0's text, entry 3 is row 2's, row 1's text is no entry
        texts = [tok(10) + tok(11), tok(10) + tok(20), tok(10), tok(12) + tok(22), tok(10) + tok(20)]
        lx = ocr.lexicon(texts)
        assert isinstance(lx, Lexicon) and lx.handle == 1 and lx.texts == tuple(texts) and sorted(lx.entries.values()) == [0, 1, 2, 3]
        assert eng.calls == [["automaton", 6, 5]]
        imgs = [rec._img(i) for i in range(3)]
        recs = ocr.recognize_batch_scored(imgs, lexicon=lx)
        assert eng.calls[-1][0] == "recognize_images" and eng.calls[-1][2] == {"scores": True} and \
            eng.calls[-1][3] == {"automata": [1, 1, 1], "states": True}
        assert [r.accepted for r in recs] == [True, False, True] and [r.entry for r in recs] == [1, None, 3]
        assert recs[0].text == texts[1] and recs[1].state == au.DEAD and recs[0].state in lx.accepting
        per = ocr.recognize_batch_alternatives(imgs, lexicon=[None, lx, None], prefix=[None, None, [12]])
        assert eng.calls[-1][3] == {"automata": [0, 1, 0], "states": True} and [r.state for r in per] == [au.NONE, au.DEAD, au.NONE]
        assert per[2].n_forced == 1 and not per[0].accepted and per[0].entry is None and per[0].alt_ids is not None
        # the plain text methods pass the same keywords and return strings; one crop goes through the batcher
        assert ocr.recognize_batch(imgs, lexicon=lx) == [r.text for r in recs]
        one = ocr.recognize_scored(imgs[0], lexicon=lx)
        assert one.accepted and one.entry == 1 and eng.calls[-1][3] == {"automata": [1], "states": True}
        assert ocr.recognize(imgs[0], lexicon=lx) == texts[1]
        page = np.zeros((32, 48, 3), np.uint8)
        regs = ocr.recognize_regions_scored([page], [(0, 1, 2, 8, 8), (0, 3, 4, 0, 8)], lexicon=lx)
        assert regs[0].accepted and regs[1].text == "" and regs[1].state == au.NONE and not regs[1].accepted
        pos = ocr.recognize_batch_positions(imgs, lexicon=lx)
        assert [r.entry for r in pos] == [1, None, 3] and pos[0].positions is not None
        # a call without a lexicon makes the call it always made, and its rows carry no state
        eng.calls = []
        free = ocr.recognize_batch_scored(imgs)
        assert eng.calls == [["recognize_images", eng.calls[0][1], {"scores": True}]] and free[0].state is None and free[0].entry is None
        ocr.recognize_batch_scored(imgs, lexicon=[None, None, None])
        assert len(eng.calls[-1]) == 3, "a list of None alone is no lexicon"
        # the raw form
        two = ocr.automaton({0: {10: 1}, 1: {20: 2, 21: 2}}, [2])
        r = ocr.recognize_batch_scored(imgs[:2], lexicon=two)
        assert r[0].accepted and r[0].entry is None and r[0].state == 2 and not r[1].accepted
        # the refusals
        for bad, exc in ((dict(lexicon=[lx]), ValueError), (dict(lexicon=3), TypeError), (dict(lexicon=[lx, 5, None]), TypeError),
                         (dict(lexicon="abc"), TypeError)):
            with pytest.raises(exc):
                ocr.recognize_batch_scored(imgs, **bad)
        with pytest.raises(ValueError):
            ocr.lexicon([])
        with pytest.raises(ValueError):
            ocr.lexicon([texts[0], "#"])
        for name, args in (("recognize_beam", (imgs[0],)), ("recognize_batch_beam", (imgs,)), ("recognize_bgr_beam", ([np.zeros((8, 8, 3), np.uint8)],)),
                           ("recognize_regions_beam", ([page], [(0, 1, 2, 8, 8)]))):
            with pytest.raises(ValueError, match="lexicon"):
                getattr(ocr, name)(*args, lexicon=lx)
    finally:
        ocr._batcher.close()
    # on a MangaOcr that decodes with beams, lexicon= makes the call greedy
    eng = _fake_engine(rec)
    ocr = rec._ocr(eng, beam=BeamConfig(2))
    try:
        lx = ocr.lexicon([ocr.vocab.tokens[10] + ocr.vocab.tokens[20]])
        assert ocr.recognize_batch([rec._img(0)] * 2, lexicon=lx)[0] == lx.texts[0]
        assert "beam" not in eng.calls[-1][2] and eng.calls[-1][3]["automata"] == [1, 1]
        ocr.recognize_batch([rec._img(0)] * 2)
        assert "beam" in eng.calls[-1][2]
    finally:
        ocr._batcher.close()
    # several devices: refused by name
    class Multi(type(eng)):
        NO_LEXICON = "token automata are not implemented for several devices"
    ocr = rec._ocr(Multi())
    try:
        with pytest.raises(NotImplementedError):
            ocr.lexicon(["x"])
    finally:
        ocr._batcher.close()
