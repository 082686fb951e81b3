"""-m gpu: beam search under token automata through the engine (include/mocr.h, "beam search under a token automaton").

* fp32 engine against transformers' beam search under a history-dependent prefix_allowed_tokens_fn
  (tests/golden/beam_aut_*.npz): ids, lengths and states identical, token scores within 2e-6, sequence scores within 2e-6 or
  two fp32 steps of the score where that is more (beam_automaton_util.score_tol: the golden scores are fp32 numbers, and
  under length_penalty 0 they lie near -100).
* bf16 engine on the crops whose candidates are at least 2e-2 apart: the reference's hypotheses and states exactly, the
  length-normalised score difference measured and bounded.
* Invariants per kernel regime at 6 crops x 4 beams: graph replay = eager steps, no dependence on the batch position, a crop
  without an automaton inside a mixed batch = the crop of a token-form batch, token positions move nothing, the fp32 sum of
  the token scores is the sequence score; compacted = uncompacted at 160 rows; a long search across the 96 context bucket.
* MangaOcr.match through a real MangaOcr, and the memory hooks.

The -1e9 hypotheses (beam_automaton_util: descendants of the padding beams) are compared engine against engine like
everything else, and masked (real_only) where the other side is transformers."""
import os

import numpy as np
import pytest

import automaton_util as au
import beam_automaton_util as bau
import beam_token_util as tu
from gpu_util import crops, engine, report
from manga_ocr.engine import BeamConfig
from manga_ocr.weights import DEFAULT_SPEC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")      # before the engine's library: one HIP runtime per process, torch's

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ES = {0: False, 1: True, 2: "never"}
NO_GRAPH, NO_COMPACTION, FP8, LATENT_ALWAYS = 2, 2048, 128, 64
PAD, EOS, V = DEFAULT_SPEC.pad_id, DEFAULT_SPEC.eos_id, DEFAULT_SPEC.vocab
NONE = au.NONE
SEQ_SCORE_TOL = TOKEN_SCORE_TOL = 2e-6
BF16_MEASURED = 3.129e-4                 # measured on the MI355X: 1.775e-4 (h2), 3.129e-4 (h3), 2.418e-4 (h4)
BF16_SCORE_TOL = 2 * BF16_MEASURED
INV_EOS_BIAS = 1.7                       # tests/test_gpu_beam.py: crops end at different steps below 16 tokens
REGIMES = [("classic, fp32", "fp32", 0), ("latent, bf16", "bf16", LATENT_ALWAYS), ("fp8 attention, bf16", "bf16", LATENT_ALWAYS | FP8)]
POOL = np.setdiff1d(np.arange(5, V), [EOS, DEFAULT_SPEC.start_id, PAD])


def golden(name):
    g = np.load(os.path.join(GOLD, f"beam_aut_{name}.npz"))
    return {k: g[k] for k in g.files}


def golden_crops(g):
    return np.stack([np.random.RandomState(int(s)).randint(0, 256, size=(224, 224), dtype=np.uint8) for s in g["crop_seeds"]])


def golden_automata(g):
    """the file's automata, unpacked from global to their own state numbers -> one Automaton or None per crop"""
    auts = []
    for i in g["aut_of_crop"]:
        if i < 0:
            auts.append(None)
            continue
        s0, ns = int(g["aut_first"][i]), int(g["aut_states"][i])
        eb = g["edge_begin"][s0:s0 + ns + 1]
        auts.append(au.unpack(eb - eb[0], g["edge_token"][eb[0]:eb[-1]], g["edge_next"][eb[0]:eb[-1]] - s0, g["accepting"][s0:s0 + ns]))
    return auts


def handles_of(eng, auts):
    return [0 if a is None else eng.automaton(*au.pack(a)) for a in auts]


def golden_call(eng, g, **kw):
    ML, K, lp = int(g["max_length"]), int(g["num_beams"]), float(g["length_penalty"])
    cfg = BeamConfig(K, lp, ES[int(g["early_stopping"])], int(g["no_repeat_ngram_size"]))
    sets = [0 if (row < 0).all() else eng.token_set(row[row >= 0].tolist()) for row in g["sets"]]
    if any(sets):
        kw["beam_sets"] = sets
    out = eng.recognize_gray(golden_crops(g), max_len=ML, beam=cfg, beam_scores=True, beam_automata=handles_of(eng, golden_automata(g)),
                             beam_states=True, **kw)
    return out, ML, K, lp


def real(out, lp, ML):
    """(ids, lens, scores, logp, state) [n, K, ...] with every crop's -1e9 hypotheses as empty slots"""
    rows = [bau.real_only(*(x[c] for x in out), lp, ML, PAD) for c in range(out[1].shape[0])]
    return tuple(np.stack([r[i] for r in rows]) for i in range(5))


def check_logp(ids, lens, scores, logp, lp, ML):
    """tests/test_gpu_beam_tokens.py's check on the real hypotheses: the sequential fp32 sum of the token scores / (len - 1) ^
    length_penalty is the sequence score -> the largest relative error"""
    worst = 0.0
    assert logp.dtype == np.float32 and logp.shape == ids.shape and np.isfinite(logp).all() and (logp <= 0).all()
    for c in range(ids.shape[0]):
        for j in range(ids.shape[1]):
            L = int(lens[c, j])
            assert logp[c, j, 0] == 0 and (logp[c, j, L:] == 0).all()
            if L and scores[c, j] > bau.junk_below(lp, ML):
                mine = tu.sequential_score(logp[c, j], L, lp)
                rel = abs(float(mine) - float(scores[c, j])) / abs(float(scores[c, j]))
                worst = max(worst, rel)
                assert rel <= 1e-6, f"crop {c} hypothesis {j}: sequential sum {mine!r} against score {scores[c, j]!r}"
    return worst


def check_paths(ids, lens, scores, state, auts, lp, ML, sets=None):
    """the precision-free properties: every real hypothesis is a path of its crop's automaton, EOS only from an accepting
    state, its state the walk's end and never DEAD; NONE without an automaton and in empty slots"""
    for c, a in enumerate(auts):
        for j in range(lens.shape[1]):
            L = int(lens[c, j])
            if a is None or L == 0:
                assert state[c, j] == NONE
                continue
            if scores[c, j] <= bau.junk_below(lp, ML):
                continue
            ok, end = au.is_path(a, ids[c, j], L, None if sets is None else sets[c])
            assert ok and state[c, j] == end and end >= 0, f"crop {c} hypothesis {j}: {ids[c, j, :L]} state {state[c, j]}"


@pytest.mark.parametrize("name", ["a2", "a3", "a4", "b", "c", "d", "e0", "e2"])
def test_fp32_engine_against_transformers(name):
    g = golden(name)
    eng = engine("fp32", seed=int(g["weights_seed"]), eos_bias=float(g["eos_bias"]), max_batch=24)
    out, ML, K, lp = golden_call(eng, g)
    ids, lens, scores, logp, state = real(out, lp, ML)
    same = np.array_equal(lens, g["lens"]) and np.array_equal(ids[:, :, :ML], g["ids"])
    e_seq = float((np.abs(scores.astype(np.float64) - g["scores"]) / bau.score_tol(g["scores"], SEQ_SCORE_TOL)).max()) * SEQ_SCORE_TOL
    e_tok = float(np.abs(logp[:, :, :ML].astype(np.float64) - g["logp"]).max()) if same else float("nan")
    report(f"beam automaton fp32 case ({name}): {ids.shape[0]} crops x {K} hypotheses, real hypotheses {int((g['lens'] > 0).sum())}; sequence "
           f"scores {e_seq:.2e} in units of the bound ({SEQ_SCORE_TOL:.0e}), token scores within {e_tok:.2e} (bound {TOKEN_SCORE_TOL:.0e})")
    np.testing.assert_array_equal(lens, g["lens"])
    np.testing.assert_array_equal(ids[:, :, :ML], g["ids"])
    np.testing.assert_array_equal(state, g["state"])
    assert (out[0][:, :, ML:] == PAD).all() and (out[3][:, :, ML:] == 0).all()
    assert e_seq <= SEQ_SCORE_TOL
    assert e_tok <= TOKEN_SCORE_TOL
    check_logp(*out[:4], lp, ML)
    check_paths(out[0], out[1], out[2], out[4], golden_automata(g), lp, ML)


@pytest.mark.parametrize("name", ["h2", "h3", "h4"])
def test_bf16_engine_returns_the_reference_hypotheses(name):
    """Every crop of the bf16 set (candidates at least 2e-2 apart, above the 1.5e-2 first-divergence margin of the bf16
    engine): ids, lengths and states exactly; the sequence scores against the golden ones within twice the measured maximum."""
    g = golden(name)
    assert g["gaps"].min() >= 2e-2 and g["lens"].shape[0] >= 6
    eng = engine("bf16", seed=int(g["weights_seed"]), eos_bias=float(g["eos_bias"]), max_batch=24, auto_path=True)
    out, ML, K, lp = golden_call(eng, g)
    ids, lens, scores, logp, state = real(out, lp, ML)
    same = np.array_equal(lens, g["lens"])
    e_seq = float(np.abs(scores.astype(np.float64) - g["scores"])[g["lens"] > 0].max()) if same else float("nan")
    report(f"beam automaton bf16 case ({name}): {ids.shape[0]} crops x {K}; length-normalised scores within {e_seq:.3e} of the reference "
           f"(bound {BF16_SCORE_TOL:.1e})")
    np.testing.assert_array_equal(lens, g["lens"])
    np.testing.assert_array_equal(ids[:, :, :ML], g["ids"])
    np.testing.assert_array_equal(state, g["state"])
    assert e_seq <= BF16_SCORE_TOL


def random_trie(seed, n_words=8, lo=3, hi=9):
    """a small lexicon over random tokens: words that share prefixes of random depth"""
    rs = np.random.RandomState(seed)
    toks = iter(int(x) for x in rs.choice(POOL, 200, replace=False))
    words = [[next(toks) for _ in range(int(rs.randint(lo, hi + 1)))]]
    while len(words) < n_words:
        w = words[int(rs.randint(len(words)))]
        d = int(rs.randint(0, len(w)))
        words.append(w[:d] + [next(toks) for _ in range(int(rs.randint(max(lo, d + 1), hi + 1)) - d)])
    return au.trie(words)[0]


def same_blocks(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x.view(np.int32), y.view(np.int32), err_msg=f"{what}: block {i}")


@pytest.mark.parametrize("name,dtype,flags", REGIMES)
def test_invariants(name, dtype, flags):
    ML, K, n = 24, 4, 6
    cfg = BeamConfig(K, 1.0, False, 0)
    gray = crops(4321, n)
    auts = [random_trie(10), None, random_trie(11, 2), au.universal(), random_trie(12, 12, 2, 6), None]
    kw = dict(seed=1, eos_bias=INV_EOS_BIAS, max_batch=24)
    eng = engine(dtype, flags=flags, **kw)
    hs = handles_of(eng, auts)
    call = lambda e, h, g=gray, **k: e.recognize_gray(g, max_len=ML, beam=cfg, beam_scores=True, beam_automata=h, beam_states=True, **k)
    out = call(eng, hs)
    ids, lens, scores, logp, state = out
    check_paths(ids, lens, scores, state, auts, 1.0, ML)
    worst = check_logp(ids, lens, scores, logp, 1.0, ML)
    assert (lens[:, 0] >= 2).all() and (scores[:, 0] > -1e3).all(), "every crop has a real best hypothesis"
    assert (lens[2, 2:] == 0).all() or (scores[2, 2:] <= bau.junk_below(1.0, ML)).all(), "a 2-entry lexicon has two real hypotheses"
    # graph replay = eager steps
    eager = engine(dtype, flags=flags | NO_GRAPH, **kw)
    same_blocks(call(eager, handles_of(eager, auts)), out, f"{name}: eager steps against graph replay")
    # the batch position
    moved = call(eng, hs[-1:] + hs[:-1], np.roll(gray, 1, axis=0))
    same_blocks(moved, tuple(np.roll(x, 1, axis=0) for x in out), f"{name}: the batch position")
    # a crop without an automaton = the crop of a token-form batch of the same size; the universal automaton = none
    tok = eng.recognize_gray(gray, max_len=ML, beam=cfg, beam_scores=True)
    for c in (1, 5, 3):
        for blk, x, y in zip(("ids", "lens", "scores", "logp"), out, tok):
            np.testing.assert_array_equal(x[c].view(np.int32), y[c].view(np.int32), err_msg=f"{name}: {blk} of crop {c} against the token form")
    assert (state[[1, 5]] == NONE).all() and (state[3][lens[3] > 0] == 0).all()
    # token positions move nothing
    with_pos = call(eng, hs, beam_positions=True)
    assert len(with_pos) == 6 and with_pos[4].shape == ids.shape + (5,) and np.isfinite(with_pos[4]).all()
    same_blocks(with_pos[:4] + with_pos[5:], out, f"{name}: beam_positions=True")
    # both outputs null: the *_beam_positions call
    graphs = eng.graph_count()
    same_blocks(call(eng, hs), out, "a repeated call")
    assert eng.graph_count() == graphs, "repeating the call adds no graph"
    report(f"beam automaton {name}: {n} crops x {K} under a trie / none / 2 entries / universal / a trie / none: eager = graphs, rolled "
           f"batch, NONE and universal crops = token form, positions move nothing; sequential sum = score within {worst:.1e} relative")


def test_compacted_equals_uncompacted_at_160_rows():
    ML, K, n = 24, 4, 40
    cfg = BeamConfig(K, 1.0, False, 0)
    gray = crops(777, n)
    auts = [None if c % 7 == 3 else random_trie(100 + c, 3 + c % 6, 2, 4 + c % 9) for c in range(n)]
    out = []
    for f in (0, NO_COMPACTION):
        eng = engine("bf16", seed=1, eos_bias=INV_EOS_BIAS, max_batch=n * K, flags=LATENT_ALWAYS | f)
        before = eng.compaction_count()
        out.append(eng.recognize_gray(gray, max_len=ML, beam=cfg, beam_scores=True, beam_automata=handles_of(eng, auts), beam_states=True))
        moved = eng.compaction_count() - before
        assert (moved > 0) == (f == 0), "the default engine compacts, the other does not"
    same_blocks(out[0], out[1], "compacted against uncompacted")
    check_paths(out[0][0], out[0][1], out[0][2], out[0][4], auts, 1.0, ML)
    ends = {int(x) for x in out[0][1][:, 0]}
    assert len(ends) >= 3, "crops end at different steps"
    report(f"beam automaton: {n} crops x {K} = 160 rows, compacted = uncompacted; best hypotheses of lengths {sorted(ends)}")


@pytest.mark.parametrize("name,dtype,flags", [("classic, fp32", "fp32", 0), ("latent, bf16", "bf16", LATENT_ALWAYS)])
def test_a_long_search_replays_graphs_as_it_runs_eagerly(name, dtype, flags):
    """104 tokens under a loop that cannot accept before the length stop: the batch crosses the context bucket at 96"""
    ML, K, n = 104, 4, 3
    gray = crops(808, n)
    cfg = BeamConfig(K, 1.0, False, 0)
    rs = np.random.RandomState(3)
    auts = [au.loop([int(x) for x in rs.choice(POOL, m, replace=False)], at_least=ML) for m in (3, 40, 400)]
    out = []
    for f in (0, NO_GRAPH):
        eng = engine(dtype, seed=0, max_batch=n * K, flags=flags | f)
        out.append(eng.recognize_gray(gray, max_len=ML, beam=cfg, beam_scores=True, beam_automata=handles_of(eng, auts), beam_states=True))
    ids, lens, scores, logp, state = out[0]
    assert (lens == ML).all() and (state == ML - 1).all(), "every hypothesis ends on the length rule, its last token walked"
    check_paths(ids, lens, scores, state, auts, 1.0, ML)
    check_logp(ids, lens, scores, logp, 1.0, ML)
    same_blocks(out[0], out[1], f"{name}: graph replay against eager steps")
    report(f"beam automaton {name}: {n} crops x {K}, {ML} tokens each under loops over 3 / 40 / 400 tokens, graph replay identical to eager steps")


def test_memory_refusals_and_the_null_twin():
    ML, K, n = 12, 3, 4
    cfg = BeamConfig(K, 1.0, False, 0)
    gray = crops(55, n)
    from manga_ocr.engine import Engine
    from gpu_util import weights
    eng = Engine(weights(1, 1.7), DEFAULT_SPEC, dtype="bf16", device=0, max_batch=16)
    try:
        h = eng.automaton(*au.pack(random_trie(5)))
        arena = eng.automaton_state_bytes()
        plain = eng.recognize_gray(gray, max_len=ML, beam=cfg, beam_scores=True, beam_positions=True)
        hooks = (eng.beam_state_bytes(), eng.beam_token_state_bytes(), eng.beam_position_state_bytes())
        assert eng.automaton_state_bytes() == arena, "beam batches without an automaton allocate no automaton state"
        # every crop NONE and states asked for: the batch launches what it launched, the states are NONE
        out = eng.recognize_gray(gray, max_len=ML, beam=cfg, beam_scores=True, beam_positions=True, beam_automata=[0] * n, beam_states=True)
        assert eng.automaton_state_bytes() == arena and (out[5] == NONE).all()
        same_blocks(out[:5], plain, "automata all NONE against the *_beam_positions call")
        got = eng.recognize_gray(gray, max_len=ML, beam=cfg, beam_automata=[h, 0, h, 0], beam_states=True)
        grown = eng.automaton_state_bytes() - arena
        assert 0 < grown <= 1 << 16, "the first beam batch under an automaton allocates the rows' states"
        assert (eng.beam_state_bytes(), eng.beam_token_state_bytes(), eng.beam_position_state_bytes()) == hooks
        assert len(got) == 4 and (got[3][[1, 3]] == NONE).all() and (got[3][[0, 2], 0] >= 0).all()
        eng.recognize_gray(gray, max_len=ML, beam=cfg, beam_automata=h)
        assert eng.automaton_state_bytes() - arena == grown
        with pytest.raises(Exception, match="automaton"):
            eng.recognize_gray(gray, max_len=ML, beam=cfg, beam_automata=[h, 0, 99, 0])
        with pytest.raises(ValueError):
            eng.recognize_gray(gray, max_len=ML, beam=cfg, automata=[h] * n)
    finally:
        eng.close()


def test_the_best_beam_entry_can_differ_from_the_greedy_lexicon_answer():
    """the golden crops whose float64 references disagree (make_beam_automaton_goldens.py: greedy_entry / beam_entry): the engine's
    greedy automata= decode reads the one entry, its beam search ranks the other first"""
    g = golden("a4")
    differ = np.nonzero((g["greedy_entry"] >= 0) & (g["beam_entry"] >= 0) & (g["greedy_entry"] != g["beam_entry"]))[0]
    assert differ.size >= 1, "the goldens hold a crop whose best beam entry is not the greedy entry"
    eng = engine("fp32", seed=int(g["weights_seed"]), eos_bias=float(g["eos_bias"]), max_batch=24)
    auts = golden_automata(g)
    hs = handles_of(eng, auts)
    out, ML, K, lp = golden_call(eng, g)
    _, glens, gstate = eng.recognize_gray(golden_crops(g), max_len=ML, automata=hs, states=True)
    for c in differ:
        words = {s: k for k, s in enumerate(sorted(auts[c].accepting))}        # (au.trie numbers its leaves in word order of creation)
        assert int(gstate[c]) in auts[c].accepting and int(out[4][c, 0]) in auts[c].accepting
        assert int(gstate[c]) != int(out[4][c, 0]), f"crop {c}: greedy and beam search read the same entry"
    report(f"beam automaton: on {differ.size} of {len(auts)} golden crops (a4) the best beam entry is not the greedy lexicon answer")


def test_match_through_a_real_mangaocr():
    """MangaOcr.match: the entries come in score order, distinct and accepted, at most k; raw=True gives all K hypotheses marked;
    the greedy lexicon= answer is among the entries whenever its length-normalised score is within the beam's; per-crop lexicons"""
    from PIL import Image
    from manga_ocr import MangaOcr
    imgs = [Image.fromarray(x) for x in crops(77, 4)]
    m = MangaOcr(synthetic_seed=0, dtype="fp32", max_batch=16, lanes=1)
    try:
        free = m.recognize_batch_scored(imgs)
        chars = [m.vocab.tokens[int(t)] for r in free for t in r.ids[1:-1]]
        chars = sorted({c for c in chars if len(c) == 1 and m.vocab.encode_chars(c) is not None})[:6]
        assert len(chars) >= 3
        rs = np.random.RandomState(5)
        names = sorted({"".join(rs.choice(chars, size=rs.randint(2, 6))) for _ in range(40)})
        lx = m.lexicon(names)
        two = m.lexicon(names[:2])
        found = 0
        for im in imgs:
            ents = m.match(im, lx, k=4, token_scores=True)
            assert 1 <= len(ents) <= 4
            assert all(e.accepted and e.entry is not None and names[e.entry] == e.text and e.state >= 0 for e in ents)
            assert len({e.entry for e in ents}) == len(ents), "distinct entries"
            sc = [e.sequence_score for e in ents]
            assert sc == sorted(sc, reverse=True) and sc[-1] > -1e3, "in score order, no padding beam's duplicate"
            greedy = m.recognize_scored(im, lexicon=lx)
            assert greedy.accepted
            g_score = float(np.sum(greedy.logprobs.astype(np.float64))) / len(greedy.logprobs)      # (greedy renormalises: >= the beam's)
            if greedy.entry in [e.entry for e in ents]:
                found += 1
            else:
                mine = {e.entry: e for e in m.match(im, lx, k=4, raw=True, token_scores=True)}
                assert greedy.entry not in mine or not mine[greedy.entry].accepted
        assert found >= 1
        raw = m.match(imgs[0], two, k=4, raw=True)
        kept = m.match(imgs[0], two, k=4)
        assert len(kept) == 2 and {e.text for e in kept} == set(names[:2]), "fewer entries than beams: both, and nothing else"
        assert len(raw) >= 2 and [e.text for e in raw if e.accepted and e.sequence_score > -1e3][:2] == [e.text for e in kept]
        per = m.match_batch(imgs, [lx, None, two, None], k=3)
        assert per[1] == [] and per[3] == [] and len(per[2]) == 2 and per[0][0].text == m.match(imgs[0], lx, k=3)[0].text
        raw1 = m.match_batch(imgs, [lx, None, two, None], k=3, raw=True)[1]
        assert raw1 and all(r.state == NONE and not r.accepted and r.entry is None for r in raw1)
        assert [e.text for e in m.match_bgr([np.asarray(imgs[0].convert("RGB"))[:, :, ::-1]], lx, k=3)[0]] == [e.text for e in m.match(imgs[0], lx, k=3)]
        with pytest.raises(ValueError, match="lexicon"):
            m.recognize_beam(imgs[0], lexicon=lx)
    finally:
        m.close()
