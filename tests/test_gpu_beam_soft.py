"""-m gpu: beam search under SOFT token automata through the engine (include/mocr.h, "beam search under soft token
automata"; transformers' generate(num_beams=K, sequence_bias=...)).

* fp32 engine against transformers' own beam search under sequence_bias (tests/golden/beam_soft_*.npz), every case in the FLAT
  and in the COMPACT (fallback) compilation of its sequences: ids, lengths and states identical, token scores within 2e-6,
  sequence scores within 2e-6 or two fp32 steps of the score where that is more (beam_automaton_util.score_tol) - the bounds of
  tests/test_gpu_beam_automaton.py; the sequential fp32 sum of a hypothesis' token scores over (len - 1) ^ length_penalty is its
  score to 1e-6 relative.
* bf16 engine: every hypothesis it returns is scored by the float64 reference teacher-forced on the hypothesis' ids (the sum of
  lp64 + w, length-normalised).  MEASURED on the MI355X: the largest difference is 2.864e-3 (p2 2.637e-4, p3 2.864e-3, p4
  2.062e-3, g 2.864e-3, n 2.521e-3, e 7.649e-4 - the large ones on hypotheses of one or two tokens, whose score is one bf16
  log-probability and not a mean of many); the bound is twice that.  Wherever the reference's min_gap is at least that bound the hypotheses
  and states are exactly the reference's; the test says how many such crops a case had (at K = 4 there may be none).
* The bit identities inside one mixed batch (soft, zero-weight hard, hard, universal-open, none) per kernel regime; compacted =
  uncompacted; two lanes and merged requests; graphs; the four *_beam_soft twins; MangaOcr.search.

The -1e9 hypotheses (beam_automaton_util: descendants of the padding beams) are compared engine against engine like
everything else, and masked (real_only) where the other side is transformers."""
import ctypes as C
import os

import numpy as np
import pytest

import automaton_util as au
import beam_automaton_util as bau
import beam_soft_util as bsu
import beam_token_util as tu
import bias_util
from gpu_util import crops, engine, oracle, report, weights
from manga_ocr import _capi
from manga_ocr.engine import BeamConfig, _ptr
from manga_ocr.weights import DEFAULT_SPEC
from test_gpu_beam_automaton import ES, INV_EOS_BIAS, LATENT_ALWAYS, NO_COMPACTION, NO_GRAPH, REGIMES, random_trie, same_blocks

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")      # before the engine's library: one HIP runtime per process, torch's

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAD, EOS, V = DEFAULT_SPEC.pad_id, DEFAULT_SPEC.eos_id, DEFAULT_SPEC.vocab
NONE = au.NONE
SEQ_SCORE_TOL = TOKEN_SCORE_TOL = 2e-6      # tests/test_gpu_beam_automaton.py
BF16_MEASURED = 2.864e-3                    # measured on the MI355X (the module's docstring)
BF16_SCORE_TOL = 2 * BF16_MEASURED
CASES = ["p2", "p3", "p4", "g", "n", "e"]
CLASSIC = 8


def golden(name):
    g = np.load(os.path.join(GOLD, f"beam_soft_{name}.npz"))
    return {k: g[k] for k in g.files}


def golden_crops(g):
    return np.stack([np.random.RandomState(int(s)).randint(0, 256, size=(224, 224), dtype=np.uint8) for s in g["crop_seeds"]])


def golden_bias(g):
    return {tuple(int(t) for t in row[:n]): float(b) for row, n, b in zip(g["seq_tok"], g["seq_len"], g["seq_bias"])}


def golden_masks(g):
    return np.unpackbits(g["set_bits"], axis=1)[:, :V].astype(bool)


def create(eng, aut):
    return eng.automaton(*bias_util.pack(aut)) if isinstance(aut, bias_util.SoftAutomaton) else eng.automaton(*au.pack(aut))


def golden_call(eng, g, compact, **kw):
    ML, K, lp = int(g["max_length"]), int(g["num_beams"]), float(g["length_penalty"])
    cfg = BeamConfig(K, lp, ES[int(g["early_stopping"])], int(g["no_repeat_ngram_size"]))
    aut = bias_util.from_sequence_bias(golden_bias(g), compact=compact)
    if int(g["with_set"]):
        kw["beam_sets"] = [eng.token_set(np.nonzero(m)[0].tolist()) for m in golden_masks(g)]
    out = eng.recognize_gray(golden_crops(g), max_len=ML, beam=cfg, beam_scores=True, beam_automata=create(eng, aut), beam_states=True,
                             beam_soft=True, **kw)
    return out, aut, ML, K, lp


def real(out, lp, ML):
    rows = [bau.real_only(*(x[c] for x in out), lp, ML, PAD) for c in range(out[1].shape[0])]
    return tuple(np.stack([r[i] for r in rows]) for i in range(5))


def check_sums(ids, lens, scores, logp, lp, ML):
    """the sequential fp32 sum of the token scores / (len - 1) ^ length_penalty is the sequence score -> the largest relative
    error.  (A token score holds its weight: it may be positive.)"""
    worst = 0.0
    assert logp.dtype == np.float32 and logp.shape == ids.shape and np.isfinite(logp).all()
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


def walks(aut, ids, lens, scores, lp, ML):
    """the state every real hypothesis must report: the walk of its tokens (EOS, its last token, moves nothing)"""
    out = np.full(lens.shape, NONE, np.int32)
    for c in range(lens.shape[0]):
        for j in range(lens.shape[1]):
            if lens[c, j] > 0 and scores[c, j] > bau.junk_below(lp, ML):
                out[c, j] = aut.walk(ids[c, j, 1:lens[c, j]])
    return out


# ------------------------------------------------------------------------------------------------ 1. fp32 against transformers
@pytest.mark.parametrize("form", ["flat", "compact"])
@pytest.mark.parametrize("name", CASES)
def test_fp32_engine_against_transformers(name, form):
    g = golden(name)
    eng = engine("fp32", seed=int(g["weights_seed"]), eos_bias=float(g["eos_bias"]), max_batch=24)
    out, aut, ML, K, lp = golden_call(eng, g, form == "compact")
    ids, lens, scores, logp, state = real(out, lp, ML)
    same = np.array_equal(lens, g["lens"]) and np.array_equal(ids[:, :, :ML], g["ids"])
    e_seq = float((np.abs(scores.astype(np.float64) - g["scores"]) / bau.score_tol(g["scores"], SEQ_SCORE_TOL)).max()) * SEQ_SCORE_TOL
    e_tok = float(np.abs(logp[:, :, :ML].astype(np.float64) - g["logp"]).max()) if same else float("nan")
    report(f"beam soft fp32 case ({name}, {form}): {ids.shape[0]} crops x {K} hypotheses, real hypotheses {int((g['lens'] > 0).sum())}; sequence "
           f"scores {e_seq:.2e} in units of the bound ({SEQ_SCORE_TOL:.0e}), token scores within {e_tok:.2e} (bound {TOKEN_SCORE_TOL:.0e})")
    np.testing.assert_array_equal(lens, g["lens"])
    np.testing.assert_array_equal(ids[:, :, :ML], g["ids"])
    want_state = walks(aut, g["ids"], g["lens"], g["scores"], lp, ML)
    if form == "flat":
        np.testing.assert_array_equal(want_state, g["state"])
    elif int(g["compact"]):
        np.testing.assert_array_equal(want_state, g["state_compact"])
    np.testing.assert_array_equal(state, want_state)
    assert (out[0][:, :, ML:] == PAD).all() and (out[3][:, :, ML:] == 0).all()
    assert e_seq <= SEQ_SCORE_TOL
    assert e_tok <= TOKEN_SCORE_TOL
    check_sums(*out[:4], lp, ML)


# ------------------------------------------------------------------------------------------------ 2. bf16 against float64
@pytest.mark.parametrize("name", CASES)
def test_bf16_engine_scores_its_hypotheses_as_the_reference_does(name):
    """Every hypothesis the bf16 engine returns, teacher-forced through the float64 oracle under the rule: the length-normalised
    sum of lp64 + w within BF16_SCORE_TOL of the engine's score (twice the largest difference measured on the MI355X, 2.864e-3).
    Where the reference's min_gap is at least that bound, the hypotheses and the states are exactly the golden ones."""
    g = golden(name)
    eng = engine("bf16", seed=int(g["weights_seed"]), eos_bias=float(g["eos_bias"]), max_batch=24, auto_path=True)
    out, aut, ML, K, lp = golden_call(eng, g, False)
    ids, lens, scores, logp, state = real(out, lp, ML)
    o = oracle(int(g["weights_seed"]), float(g["eos_bias"]))
    with torch.no_grad():
        enc = o.encode(o.preprocess_gray(golden_crops(g)))
    masks = golden_masks(g)
    worst, n_hyp = 0.0, 0
    for c in range(lens.shape[0]):
        for j in range(K):
            L = int(lens[c, j])
            if not L:
                continue
            assert masks[c][ids[c, j, 1:L]].all(), "a hypothesis stays inside its crop's set"
            want, _ = bsu.forced_score(o, enc[c:c + 1], ids[c, j], L, aut, lp)
            worst = max(worst, abs(want - float(scores[c, j])))
            n_hyp += 1
            assert state[c, j] == aut.walk(ids[c, j, 1:L])
    wide = np.nonzero(g["gaps"] >= BF16_SCORE_TOL)[0]
    report(f"beam soft bf16 case ({name}): {n_hyp} hypotheses of {lens.shape[0]} crops x {K}; length-normalised scores within {worst:.3e} of the "
           f"float64 reference teacher-forced on them (bound {BF16_SCORE_TOL:.2e}); {wide.size} crops with min_gap >= the bound")
    assert n_hyp >= lens.shape[0]
    assert worst <= BF16_SCORE_TOL
    for c in wide:
        np.testing.assert_array_equal(lens[c], g["lens"][c])
        np.testing.assert_array_equal(ids[c, :, :ML], g["ids"][c])
        np.testing.assert_array_equal(state[c], g["state"][c])


# ------------------------------------------------------------------------------------------------ 3. the bit identities
def _mixed(eng, gray):
    """six crops: soft, zero-weight hard, the same hard, universal-open, none, another hard.  Crops 1 / 2 and 3 / 4 are the same
    image -> (the handles of the soft batch, those of its *_beam_automaton twin, the soft automaton)"""
    rs = np.random.RandomState(9)
    free = eng.recognize_gray(gray, max_len=16)[0]
    f = [int(t) for t in free[0, 1:6] if int(t) not in (EOS, PAD)]
    other = [int(x) for x in rs.choice(np.arange(100, 6000), 3, replace=False)]
    soft = bias_util.from_sequence_bias({(f[0],): -2.5, (f[0], other[0]): 4.0, (other[0], other[1]): 3.5, (other[2],): 0.375}, compact=True)
    hard, hard2 = random_trie(10), random_trie(12, 12, 2, 6)
    zero = bias_util.SoftAutomaton(hard.trans, hard.accepting, {s: {t: 0.0 for t in e} for s, e in hard.trans.items()}, None, hard.n_states)
    eb, et, en, acc, w, d = bias_util.pack(zero)
    h_zero = eng.automaton(eb, et, en, acc, w, None)         # (all-zero weights, no default edges: soft by its arrays)
    h_soft, h_hard, h_hard2, h_uni = create(eng, soft), create(eng, hard), create(eng, hard2), create(eng, bias_util.universal_open())
    return [h_soft, h_zero, h_hard, h_uni, 0, h_hard2], [0, h_hard, h_hard, 0, 0, h_hard2], soft


@pytest.mark.parametrize("name,dtype,flags", REGIMES)
def test_bit_identities_in_one_mixed_batch(name, dtype, flags):
    ML, K = 16, 4
    cfg = BeamConfig(K, 2.0, True, 3)
    gray = crops(4321, 6)
    gray[2], gray[4] = gray[1], gray[3]
    eng = engine(dtype, flags=flags, seed=1, eos_bias=INV_EOS_BIAS, max_batch=24)
    hs, twin, soft = _mixed(eng, gray)
    call = lambda h, **k: eng.recognize_gray(gray, max_len=ML, beam=cfg, beam_scores=True, beam_positions=True, beam_automata=h, beam_states=True, **k)
    out = call(hs, beam_soft=True)
    ids, lens, scores, logp, pos, state = out
    for blk in out:         # a hard automaton with all-zero weights = the same automaton without; universal-open = none
        np.testing.assert_array_equal(blk[1].view(np.int32), blk[2].view(np.int32), err_msg=f"{name}: zero weights against none")
    for blk in out[:5]:
        np.testing.assert_array_equal(blk[3].view(np.int32), blk[4].view(np.int32), err_msg=f"{name}: universal-open against NONE")
    assert (state[4] == NONE).all() and (state[3][lens[3] > 0] == 0).all()
    # hard and plain crops of a soft batch = the same crops in a *_beam_automaton batch of the same size
    ref = call(twin)
    for c in (1, 2, 4, 5):
        for x, y in zip(out, ref):
            np.testing.assert_array_equal(x[c].view(np.int32), y[c].view(np.int32), err_msg=f"{name}: crop {c} against the *_beam_automaton batch")
    for x, y in zip(out[:5], ref[:5]):
        np.testing.assert_array_equal(x[3].view(np.int32), y[3].view(np.int32))
    # no soft handle: the *_beam_soft call IS the *_beam_automaton call - the same bits on the graphs it has
    graphs = eng.graph_count()
    same_blocks(call(twin, beam_soft=True), ref, f"{name}: *_beam_soft without a soft handle")
    assert eng.graph_count() == graphs
    # the soft crop: its states are the walks, its sums its scores; eager steps = graph replay
    assert lens[0, 0] >= 2 and state[0, 0] == soft.walk(ids[0, 0, 1:lens[0, 0]])
    check_sums(ids[:1], lens[:1], scores[:1], logp[:1], 2.0, ML)
    eager = engine(dtype, flags=flags | NO_GRAPH, seed=1, eos_bias=INV_EOS_BIAS, max_batch=24)
    hs_e, _, _ = _mixed(eager, gray)
    same_blocks(eager.recognize_gray(gray, max_len=ML, beam=cfg, beam_scores=True, beam_positions=True, beam_automata=hs_e, beam_states=True,
                                     beam_soft=True), out, f"{name}: eager steps against graph replay")
    report(f"beam soft {name}: soft / zero-weight hard / hard / universal-open / none / hard in one batch of 6 x {K}: the identities hold bit for "
           f"bit, eager = graphs")


@pytest.mark.parametrize("name,dtype,flags", [("classic, bf16", "bf16", CLASSIC), ("latent, bf16", "bf16", LATENT_ALWAYS)])
def test_compacted_equals_uncompacted(name, dtype, flags):
    ML, K, n = 16, 4, 40
    cfg = BeamConfig(K, 1.0, False, 0)
    gray = crops(777, n)
    out, moved = [], []
    for f in (0, NO_COMPACTION):
        eng = engine(dtype, seed=1, eos_bias=INV_EOS_BIAS, max_batch=n * K, flags=flags | f)
        free = eng.recognize_gray(gray[:1], max_len=ML)[0]
        t0 = int(free[0, 1])
        soft = create(eng, bias_util.from_sequence_bias({(t0,): -2.5, (t0, 700): 4.0, (701,): 0.5}, compact=True))
        hard = create(eng, random_trie(100, 6, 2, 8))
        hs = [soft if c % 3 == 0 else hard if c % 3 == 1 else 0 for c in range(n)]
        before = eng.compaction_count()
        out.append(eng.recognize_gray(gray, max_len=ML, beam=cfg, beam_scores=True, beam_automata=hs, beam_states=True, beam_soft=True))
        moved.append(eng.compaction_count() - before)
    assert moved[1] == 0 and (moved[0] > 0 or flags == CLASSIC), "the default latent engine compacts, NO_COMPACTION never does"
    same_blocks(out[0], out[1], f"{name}: compacted against uncompacted")
    report(f"beam soft {name}: {n} crops x {K} = {n * K} rows, {moved[0]} compactions = none; best hypotheses of lengths "
           f"{sorted({int(x) for x in out[0][1][:, 0]})}")


def test_two_lanes_and_merged_requests():
    """A two-lane bf16 engine, three beam requests of one configuration submitted together from three threads - a soft one, a hard
    one and a plain one: whatever the scheduler merges and wherever it runs them, every request equals the same request alone."""
    import threading
    from manga_ocr.engine import Engine
    ML, K, n = 16, 3, 4
    cfg = BeamConfig(K, 2.0, True, 3)
    eng = Engine(weights(1, INV_EOS_BIAS), DEFAULT_SPEC, dtype="bf16", device=0, max_batch=48, lanes=2)
    try:
        gray = crops(31, n)
        t0 = int(eng.recognize_gray(gray[:1], max_len=ML)[0][0, 1])
        soft = create(eng, bias_util.from_sequence_bias({(t0,): -2.5, (t0, 700): 4.0}, compact=True))
        hard = create(eng, random_trie(10))
        reqs = [dict(beam_automata=[soft, 0, soft, hard], beam_states=True, beam_soft=True), dict(beam_automata=hard, beam_states=True), dict()]
        alone = [eng.recognize_gray(gray, ML, beam=cfg, beam_scores=True, **kw) for kw in reqs]
        for attempt in range(2):
            got = [None] * 3

            def run(i):
                got[i] = eng.recognize_gray(gray, ML, beam=cfg, beam_scores=True, **reqs[i])
            ts = [threading.Thread(target=run, args=(i,)) for i in range(3)]
            [t.start() for t in ts]
            [t.join() for t in ts]
            for i in range(3):
                same_blocks(got[i], alone[i], f"request {i} among merged requests")
    finally:
        eng.close()


def test_graphs_and_the_refusal_that_stays():
    """a soft beam batch captures graphs of its own; a repeat none; a later hard or plain beam batch reuses its old ones; the
    *_beam_automaton call keeps refusing a soft handle, and no automaton state is added for the soft form"""
    from manga_ocr._capi import MocrError
    from manga_ocr.engine import Engine
    ML, K, n = 16, 4, 4
    cfg = BeamConfig(K, 2.0, True, 3)
    gray = crops(55, n)
    eng = Engine(weights(1, INV_EOS_BIAS), DEFAULT_SPEC, dtype="bf16", device=0, max_batch=16)
    try:
        hard = create(eng, random_trie(5))
        plain = eng.recognize_gray(gray, ML, beam=cfg, beam_scores=True)
        h_out = eng.recognize_gray(gray, ML, beam=cfg, beam_scores=True, beam_automata=hard, beam_states=True)
        g_hard = eng.graph_count()
        soft = create(eng, bias_util.from_sequence_bias({(int(plain[0][0, 0, 1]),): -2.5, (700, 701): 2.0}, compact=True))
        bytes_before = eng.automaton_state_bytes()
        s_out = eng.recognize_gray(gray, ML, beam=cfg, beam_scores=True, beam_automata=[soft, hard, 0, soft], beam_states=True, beam_soft=True)
        g_soft = eng.graph_count()
        assert g_soft > g_hard, "a soft beam batch captures graphs of its own"
        assert eng.automaton_state_bytes() == bytes_before, "the soft form brings no state of its own"
        same_blocks(eng.recognize_gray(gray, ML, beam=cfg, beam_scores=True, beam_automata=[soft, hard, 0, soft], beam_states=True, beam_soft=True),
                    s_out, "a repeated soft batch")
        same_blocks(eng.recognize_gray(gray, ML, beam=cfg, beam_scores=True, beam_automata=hard, beam_states=True), h_out, "a later hard batch")
        same_blocks(eng.recognize_gray(gray, ML, beam=cfg, beam_scores=True), plain, "a later plain batch")
        assert eng.graph_count() == g_soft, "repeats and later hard or plain beam batches reuse their graphs"
        assert int(s_out[0][0, 0, 1]) != int(plain[0][0, 0, 1]) or s_out[2][0, 0] != plain[2][0, 0], "-2.5 on the best first token moves the search"
        with pytest.raises(MocrError):
            eng.recognize_gray(gray, ML, beam=cfg, beam_automata=[soft, hard, 0, soft], beam_states=True)
        with pytest.raises(ValueError):
            eng.recognize_gray(gray, ML, beam_soft=True)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 4. the ABI twins
def test_the_four_beam_soft_twins():
    """mocr_recognize_<kind>_beam_soft on the four source kinds, a soft handle on crops 0 and 2: the same hypotheses, token scores
    and states as Engine.recognize_gray(beam_soft=True) on the same planes"""
    import test_gpu_abi_twins_beam as tw
    eng = tw._engine()
    N, T, K, L = tw.N, tw.T, tw.K, tw.L
    gray = crops(515, N)
    cfg = BeamConfig(K, 2.0, True, 3)
    t0 = int(eng.recognize_gray(gray[:1], T)[0][0, 1])
    soft = create(eng, bias_util.from_sequence_bias({(t0,): -2.5, (t0, 700): 4.0}, compact=True))
    aut = np.array([soft, 0, soft], np.int32)
    want = eng.recognize_gray(gray, T, beam=cfg, beam_scores=True, beam_automata=aut, beam_states=True, beam_soft=True)
    cs = cfg.as_struct()
    for kind in tw.KINDS:
        dev = kind == "device"

        def block(shape, dtype, fill):
            return torch.full(shape, fill, dtype=getattr(torch, dtype), device="cuda") if dev else np.full(shape, fill, dtype=dtype)
        outs = [block((N, K, L), "int32", -7), block((N, K), "int32", -7), block((N, K), "float32", 5.0), block((N, K, L), "float32", 5.0),
                block((N, K), "int32", -7)]
        tail = [C.byref(cs), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), None, None, _ptr(aut), _ptr(outs[4])]
        fn = getattr(eng.lib, f"mocr_recognize_{kind}_beam_soft")
        if dev:
            d_gray = torch.from_numpy(gray).cuda()
            rc = fn(eng._h, _ptr(d_gray), N, *tail)
            eng.synchronize()
        elif kind == "gray_host":
            rc = fn(eng._h, _ptr(gray), N, T, *tail)
        elif kind == "images":
            descs, keep = eng._image_descs(list(gray))
            rc = fn(eng._h, descs, N, *tail)
        else:
            pages = [np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2)) for g in gray]
            descs, keep = eng._image_descs(pages, True)
            arr = (_capi.MocrRegion * N)()
            for i in range(N):
                arr[i].page, arr[i].x, arr[i].y, arr[i].width, arr[i].height = i, 0, 0, 224, 224
            rc = fn(eng._h, descs, N, arr, N, *tail)
        assert rc == _capi.MOCR_OK, (kind, eng.lib.mocr_last_error(eng._h))
        got = [o.cpu().numpy() if dev else o for o in outs]
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes(), f"{kind} differs from Engine.recognize_gray"
        # ... and the *_beam_automaton twin of the same kind keeps refusing the soft handle (gray_host stands for the four)
        if kind == "gray_host":
            rc = eng.lib.mocr_recognize_gray_host_beam_automaton(eng._h, _ptr(gray), N, T, *tail)
            assert rc == -1 and b"soft" in eng.lib.mocr_last_error(eng._h)
    assert (want[4][[0, 2], 0] >= 0).all() and (want[4][1] == NONE).all()


# ------------------------------------------------------------------------------------------------ 5. the product surface
def test_search_through_a_real_mangaocr():
    """MangaOcr.search on a glossary whose entry the free beam search does not read: the best hypothesis holds the entry,
    Lexicon.find locates it, accepted / entry stay None, the state is delivered, and the sequence score - biases included - is
    above what the same ids score unbiased; match keeps refusing the glossary, a hard lexicon is allowed"""
    from PIL import Image
    from manga_ocr import MangaOcr
    imgs = [Image.fromarray(x) for x in crops(77, 3)]
    m = MangaOcr(synthetic_seed=0, dtype="fp32", max_batch=16, lanes=1)
    try:
        free = m.recognize_beam(imgs[0], 4, token_scores=True)
        f0 = [int(t) for t in free[0].ids[1:] if int(t) != EOS]
        assert len(f0) >= 2 and f0[0] not in m.vocab.special_ids
        other = next(t for t in range(5, 64) if t not in f0 and len(m.vocab.tokens[t]) == 1 and all(t not in h.ids for h in free))
        name = m.vocab.tokens[f0[0]] + m.vocab.tokens[other]
        gl = m.glossary([name], bonus=40.0)
        assert all(gl.find(h.ids) == [] for h in free), "the free beam search does not read the entry"
        hyps = m.search(imgs[0], gl, 4, token_scores=True)
        best = hyps[0]
        assert gl.find(best.ids) and gl.find(best.ids)[0] == (1, 0) and name in best.text, best.text
        assert all(h.accepted is None and h.entry is None and h.state >= 0 for h in hyps)
        sc = [h.sequence_score for h in hyps]
        assert sc == sorted(sc, reverse=True)
        # the same ids unbiased: a greedy row forced on them scores every token with the plain log_softmax
        n_tok = len(best.ids) - 1
        forced = m.recognize_scored(imgs[0], prefix=[int(t) for t in best.ids[1:]])
        assert [int(t) for t in forced.ids[:n_tok + 1]] == [int(t) for t in best.ids]
        unbiased = float(np.sum(forced.logprobs[:n_tok].astype(np.float64))) / n_tok
        assert best.sequence_score > unbiased + 0.5 * 40.0 / n_tok, (best.sequence_score, unbiased, n_tok)
        assert abs(float(np.sum(best.logprobs.astype(np.float64))) / (len(best.ids) - 1) - best.sequence_score) <= 1e-5 * abs(best.sequence_score) + 1e-5
        per = m.search_batch(imgs, [gl, None, m.lexicon([name])], 3)
        assert gl.find(per[0][0].ids) and all(h.state == NONE and h.accepted is False for h in per[1])
        assert any(h.accepted and h.entry == 0 for h in per[2]), "a hard Lexicon is allowed, and confines"
        assert [h.text for h in m.search_bgr([np.asarray(imgs[0].convert("RGB"))[:, :, ::-1]], gl, k=4)[0]] == [h.text for h in hyps]
        with pytest.raises(ValueError, match="search"):
            m.match(imgs[0], gl)
        assert m.recognize(imgs[0], lexicon=gl) == m.recognize_scored(imgs[0], lexicon=gl).text, "lexicon= stays greedy"
    finally:
        m.close()
