"""-m gpu: greedy decoding under soft token automata, end to end (include/mocr.h, "soft token automata").

The goldens of tests/golden/make_bias_goldens.py - transformers' generate(sequence_bias=...) - on the fp32 engine; per-row
weights chosen from the oracle's logits so that they change the pick by a margin no precision can undo, on the fp32 engine
and on every bf16 decode path (BF16_CASES of tests/test_gpu_ngram.py), with soft, hard and no automaton mixed in one batch; the
universal-open automaton and the zero-weight hard automaton against their plain twins, bit for bit; compaction; shared
encodings; two lanes and merged requests; graphs, memory and the argument errors; the ABI twins with a soft handle; the
product surface.  Tolerances are those of tests/test_gpu_ngram.py and tests/test_gpu_automaton.py, imported or named where used."""
import ctypes as C
import os

import numpy as np
import pytest

from gpu_util import crops, report

import automaton_util as au
import bias_util as bu
import constraint_util as cu
import ngram_util as nu
import score_util as su
from manga_ocr import _capi
from manga_ocr.text import pack_automaton
from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights
from test_gpu_bf16_parity import BF16_GAP_TOL
from test_gpu_constraints import FP32_LOGIT_TOL, _bits
from test_gpu_ngram import BF16_CASES

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V, K4, EOS, START = 6144, 4, 3, 2
NONE, DEAD = au.NONE, au.DEAD
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_E2E, LEN_E2E = 8, 32
SENT = -777


def _create(eng, a):
    """the automaton on this engine: the soft call for a SoftAutomaton, the call it always was for a hard one"""
    if isinstance(a, bu.SoftAutomaton):
        return eng.automaton(*bu.pack(a))
    return eng.automaton(*au.pack(a))


# ------------------------------------------------------------------------------------------------ 1. transformers' goldens
@pytest.mark.parametrize("compact", [False, True], ids=["flat", "compact"])
@pytest.mark.parametrize("case", ["a", "b", "e"])
def test_fp32_engine_reproduces_transformers_sequence_bias(case, compact):
    """tests/golden/bias_<case>.npz on an fp32 engine under text.bias_automaton's compilation of the golden's sequences - the
    flat one, and the compact one that MangaOcr.sequence_bias creates, whose states leave the root's edges to the fallback walk
    (MOCR_DEFAULT_FALLBACK) and keep their numbers: ids,
    lengths and final states identical to transformers' and to the reference loop; scores within 2 x FP32_LOGIT_TOL of the
    float64 log-softmax of the reference's weighted logits (the bound of tests/test_gpu_ngram.py); the four alternatives are the
    reference's top four of logit + weight.  Without the feature the ids are the free run's, which every golden row leaves."""
    from manga_ocr.engine import Engine
    from oracle.mocr_oracle import Oracle
    g = np.load(os.path.join(GOLDEN, f"bias_{case}.npz"))
    sb = {tuple(int(t) for t in g["seq_tok"][i, :g["seq_len"][i]]): float(g["seq_bias"][i]) for i in range(len(g["seq_len"]))}
    a = bu.from_sequence_bias(sb, compact=compact)
    w = synthetic_weights(int(g["weights_seed"]), eos_bias=float(g["eos_bias"]))
    gray = np.stack([np.random.RandomState(int(s)).randint(0, 256, size=(224, 224), dtype=np.uint8) for s in g["crop_seeds"]])
    ML, B = int(g["max_length"]), len(gray)
    o = Oracle(w, DEFAULT_SPEC)
    with torch.no_grad():
        enc = o.encode(o.preprocess_gray(gray))
    ids_o, wl, pl, masks, state_o, _ = bu.soft_generate(o, enc, [a] * B, np.ones((B, V), bool), [0] * B, ML)
    lens_o = bu.lengths(ids_o, EOS)
    eng = Engine(w, DEFAULT_SPEC, dtype="fp32", device=0, max_batch=8, lanes=1)
    try:
        h = _create(eng, a)
        ids, lens, logp, alt_ids, alt_logp, state = eng.recognize_gray(gray, ML, alternatives=True, automata=h, states=True)
        free_ids, free_lens = eng.recognize_gray(gray, ML)
    finally:
        eng.close()
    np.testing.assert_array_equal(lens, g["lens"]); np.testing.assert_array_equal(lens, lens_o)
    np.testing.assert_array_equal(state, g["state"]); np.testing.assert_array_equal(state, state_o)
    worst, first = 0.0, None
    for b in range(B):
        np.testing.assert_array_equal(ids[b, :lens[b]], g["ids"][b, :lens[b]], err_msg=f"row {b}: not transformers' ids")
        np.testing.assert_array_equal(ids[b, :lens[b]], ids_o[b, :lens[b]])
        assert (ids[b, lens[b]:] == 0).all()
        for t in range(1, lens[b]):
            ref = cu.masked_log_softmax64(wl[b, t - 1], masks[b, t - 1])
            want4, lp4 = cu.masked_top(wl[b, t - 1], masks[b, t - 1])
            np.testing.assert_array_equal(alt_ids[b, t], want4)
            worst = max(worst, abs(float(logp[b, t]) - ref[ids[b, t]]), float(np.abs(alt_logp[b, t].astype(np.float64) - lp4).max()),
                        abs(float(logp[b, t]) - float(g["logp"][b, t])) - bu.SCORE_TOL)
    print(f"fp32 sequence_bias case {case}: max |logp - float64 log-softmax of logit + weight| {worst:.3e} (bound {2 * FP32_LOGIT_TOL:.0e})", flush=True)
    assert worst <= 2 * FP32_LOGIT_TOL, worst
    changed = sum(1 for b in range(B) if free_lens[b] != lens[b] or (free_ids[b, :lens[b]] != ids[b, :lens[b]]).any())
    assert changed == int(g["changed"]) and changed * 2 >= B, "the sequences changed nothing: the weights did not reach the step"
    report(f"soft automata fp32 vs transformers generate(sequence_bias) case {case}: {B} rows, ids, lengths {lens.tolist()} and states identical, "
           f"{changed} rows leave their free run, logp / alt_logp within {worst:.2e}")


# ------------------------------------------------------------------------------------------------ 2. weights from the oracle's logits
KINDS8 = ["w1", "w2", "w3", "w1", "w2", "uopen", "zero", None]


def _chain(step: int, tok: int, weight: float):
    """open states 0 .. step: a token moves along the chain by default; the state of step `step` (1 = the first generated
    token) has one edge, on `tok`, with the weight; everything ends in the last, open, edgeless state.  Every state accepts."""
    n = step + 1
    trans = {step - 1: {tok: step}}
    return bu.SoftAutomaton(trans, range(n), {step - 1: {tok: weight}}, {s: min(s + 1, step) for s in range(n)}, n)


def _case8():
    """the 8 rows of the end-to-end tests on the widened-margin weights, crops(31, 8), max_len 32, computed once on the CPU:
    rows 0 .. 4 under a chain that adds, at generated token 1 + row % 3, a weight to the free run's runner-up of that step -
    the free margin plus 8 x BF16_GAP_TOL, rounded up to 1/8, so that the weighted pick leads by at least 4 x BF16_GAP_TOL; row 5
    under the universal-open automaton; row 6 under a hard loop over the free run's alphabet, created with an all-zero
    edge_weight; row 7 under none.  -> dict(auts, ids, wl, pl, masks, states, lens, flip)"""
    if _case8.cache:
        return _case8.cache
    o = su.score_oracle("wide")
    free_ids, free_logits = su.oracle_run("wide", 31, N_E2E, LEN_E2E)
    alphabet = np.unique(free_ids[:, 1:])
    auts, flip = [], {}
    for b, k in enumerate(KINDS8):
        if k is None:
            auts.append(None)
        elif k == "uopen":
            auts.append(bu.universal_open())
        elif k == "zero":
            lp = au.loop(alphabet[:4])
            auts.append(bu.SoftAutomaton(lp.trans, lp.accepting, {s: {t: 0.0 for t in e} for s, e in lp.trans.items()}, None, lp.n_states))
        else:
            step = int(k[1])
            lg = free_logits[b, step - 1].astype(np.float64)
            order = np.argsort(-lg, kind="stable")
            f, r = int(order[0]), int(next(t for t in order[1:] if int(t) not in (EOS, 0)))
            assert f == free_ids[b, step]
            wgt = float(np.ceil((lg[f] - lg[r] + 8 * BF16_GAP_TOL) * 8) / 8)
            auts.append(_chain(step, r, wgt))
            flip[b] = (step, f, r, wgt)
    with torch.no_grad():
        enc = o.encode(o.preprocess_gray(crops(31, N_E2E)))
    ids, wl, pl, masks, states, _ = bu.soft_generate(o, enc, auts, np.ones((N_E2E, V), bool), np.zeros(N_E2E, np.int32), LEN_E2E)
    lens = bu.lengths(ids, EOS)
    gaps = nu.step_gaps(wl, masks)
    # the condition, on the reference alone: at every step where a weight changes the pick, the weighted top-2 margin is at
    # least 4 x BF16_GAP_TOL; those steps are the rows' chain steps and nothing else
    for b in range(N_E2E):
        changed = [t for t in range(1, lens[b]) if int(np.argmax(cu.masked(wl[b, t - 1], masks[b, t - 1]))) != int(np.argmax(cu.masked(pl[b, t - 1], masks[b, t - 1])))]
        assert changed == ([flip[b][0]] if b in flip else []), (b, changed)
        for t in changed:
            assert gaps[b, t - 1] >= 4 * BF16_GAP_TOL and ids[b, t] == flip[b][2] != flip[b][1], (b, t, gaps[b, t - 1])
    assert len(flip) == 5 and (ids[5, :lens[5]] == free_ids[5, :lens[5]]).all() and (ids[7, :lens[7]] == free_ids[7, :lens[7]]).all()
    _case8.cache.update(auts=auts, ids=ids, wl=wl, pl=pl, masks=masks, states=states, lens=lens, flip=flip, gaps=gaps, alphabet=alphabet)
    return _case8.cache


_case8.cache = {}


def _handles8(eng):
    if id(eng) not in _handles8.cache:
        c = _case8()
        _handles8.cache[id(eng)] = [0 if a is None else _create(eng, a) for a in c["auts"]]
    return _handles8.cache[id(eng)]


_handles8.cache = {}


def test_fp32_weights_change_the_pick_and_the_twins_do_not():
    """fp32 engine, the 8 rows of _case8 in one batch (soft chains, universal-open, zero-weight hard loop, none).  ids, lengths
    and states identical to the reference loop; at every chain step the engine's token is the weighted pick, not the
    unweighted one (what fails without the feature); scores and alternatives within 2 x FP32_LOGIT_TOL of the float64 masked
    log-softmax of logit + weight.  Bit for bit in every output: the universal-open row == the same row under no automaton;
    the zero-weight hard row == the same automaton created without weights (in a batch of the same mode: one soft row keeps
    it soft); the `none` row == a plain batch's row.  The ids-only, scored and alternatives calls agree."""
    c = _case8()
    eng = su.score_engine("wide", "fp32")
    gray = crops(31, N_E2E)
    hs = _handles8(eng)
    ids, lens, logp, alt_ids, alt_logp, state = eng.recognize_gray(gray, LEN_E2E, alternatives=True, automata=hs, states=True)
    L = c["ids"].shape[1]
    live = np.arange(L)[None, :] < c["lens"][:, None]
    np.testing.assert_array_equal(np.where(live, ids[:, :L], 0), np.where(live, c["ids"], 0), err_msg="fp32 ids differ from the reference loop's")
    np.testing.assert_array_equal(lens, c["lens"]); np.testing.assert_array_equal(state, c["states"])
    for b, (step, f, r, wgt) in c["flip"].items():
        assert ids[b, step] == r != f, f"row {b}: token {step} is {ids[b, step]}, the weighted pick is {r}, the unweighted one {f}"
    worst = 0.0
    for b in range(N_E2E):
        for t in range(1, lens[b]):
            ref = cu.masked_log_softmax64(c["wl"][b, t - 1], c["masks"][b, t - 1])
            want4, lp4 = cu.masked_top(c["wl"][b, t - 1], c["masks"][b, t - 1])
            np.testing.assert_array_equal(alt_ids[b, t], want4)
            ok = want4 >= 0
            worst = max(worst, abs(float(logp[b, t]) - ref[ids[b, t]]), float(np.abs(alt_logp[b, t][ok].astype(np.float64) - lp4[ok]).max()))
    assert worst <= 2 * FP32_LOGIT_TOL, worst
    i0, l0, s0 = eng.recognize_gray(gray, LEN_E2E, automata=hs, states=True)
    i1, l1, p1 = eng.recognize_gray(gray, LEN_E2E, scores=True, automata=hs)
    np.testing.assert_array_equal(i0, ids); np.testing.assert_array_equal(i1, ids); np.testing.assert_array_equal(s0, state)
    np.testing.assert_array_equal(_bits(p1), _bits(logp))
    # the twins: row 5 under none, row 6 under the same loop created without weights, both still inside a soft batch
    plain_loop = eng.automaton(*au.pack(au.loop(c["alphabet"][:4])))
    twin = list(hs)
    twin[5], twin[6] = 0, plain_loop
    t_ids, t_lens, t_logp, t_ai, t_al, t_state = eng.recognize_gray(gray, LEN_E2E, alternatives=True, automata=twin, states=True)
    for z in (5, 6, 7):
        np.testing.assert_array_equal(t_ids[z], ids[z]); assert t_lens[z] == lens[z]
        np.testing.assert_array_equal(_bits(t_logp[z]), _bits(logp[z])); np.testing.assert_array_equal(t_ai[z], alt_ids[z])
        np.testing.assert_array_equal(_bits(t_al[z]), _bits(alt_logp[z]))
    assert state[5] == 0 and t_state[5] == NONE and t_state[6] == state[6] and state[7] == NONE
    # ... and against batches that are not soft at all: a hard batch (the loop alone) and a plain one
    h_ids, h_lens, h_logp, h_ai, h_al, h_state = eng.recognize_gray(gray, LEN_E2E, alternatives=True, automata=[0] * 6 + [plain_loop, 0], states=True)
    for z in (5, 6, 7):
        np.testing.assert_array_equal(h_ids[z], ids[z]); np.testing.assert_array_equal(_bits(h_logp[z]), _bits(logp[z]))
        np.testing.assert_array_equal(h_ai[z], alt_ids[z]); np.testing.assert_array_equal(_bits(h_al[z]), _bits(alt_logp[z]))
    f_ids, f_lens, f_logp, f_ai, f_al = eng.recognize_gray(gray, LEN_E2E, alternatives=True)
    for z in (5, 7):
        np.testing.assert_array_equal(f_ids[z], ids[z]); np.testing.assert_array_equal(_bits(f_logp[z]), _bits(logp[z]))
        np.testing.assert_array_equal(_bits(f_al[z]), _bits(alt_logp[z]))
    report(f"soft automata fp32, 8 rows mixed (5 weighted chains, universal-open, zero-weight loop, none): ids, lengths {lens.tolist()}, states identical to "
           f"the reference loop, every chain step takes the weighted pick, logp within {worst:.2e}; the twins bit-identical in every output")


@pytest.mark.parametrize("name,rows,flags", BF16_CASES)
def test_bf16_soft_automaton_paths(name, rows, flags):
    """bf16, the 8-row pattern repeated over the batch, on every decode path (<= 32 rows, fused head on 64 and 128 tiles, the
    slab path of MOCR_FLAG_NO_FUSED_ARGMAX).  The first 8 rows against the fp32 reference loop under the first-divergence rule
    with BF16_GAP_TOL on the WEIGHTED reference logits.  The condition, met by the reference alone (_case8): the weighted margin
    of every chain step is at least 4 x BF16_GAP_TOL; asserted here: at least 3/4 of the chain rows reach their chain step
    undiverged, and on those the engine's token is the weighted pick, not the unweighted one.  Every repeat of the pattern gives
    the first 8 rows' ids; the three kinds of call agree; the universal-open and none rows equal the free run's."""
    c = _case8()
    eng = su.score_engine("wide", "bf16", max_batch=max(64, rows), flags=flags)
    reps = rows // N_E2E
    gray = np.concatenate([crops(31, N_E2E)] * reps)
    hs = _handles8(eng) * reps
    ids, lens, logp, alt_ids, alt_logp, state = eng.recognize_gray(gray, LEN_E2E, alternatives=True, automata=hs, states=True)
    L = c["ids"].shape[1]
    div = {b: (t, g) for b, t, g in cu.first_divergences(ids[:N_E2E, :L], c["ids"], c["gaps"])}
    for b, (t, g) in div.items():
        report(f"[bf16 soft automata {name}] row {b}: first divergence at token {t} (weighted reference margin {g:.3e})")
    assert all(g < BF16_GAP_TOL for t, g in div.values()), div
    reached = [b for b, (step, f, r, wgt) in c["flip"].items() if b not in div or div[b][0] > step]
    assert len(reached) * 4 >= 3 * len(c["flip"]), f"only rows {reached} reach their weighted step undiverged"
    for b in reached:
        step, f, r, wgt = c["flip"][b]
        assert ids[b, step] == r != f, f"row {b}: token {step} is {ids[b, step]}, the weighted pick is {r}, the unweighted one {f}"
    for k in range(1, reps):
        np.testing.assert_array_equal(ids[k * N_E2E:(k + 1) * N_E2E], ids[:N_E2E], err_msg=f"repeat {k} of the pattern differs")
        np.testing.assert_array_equal(state[k * N_E2E:(k + 1) * N_E2E], state[:N_E2E])
    for b in range(rows):
        np.testing.assert_array_equal(alt_ids[b, 1:lens[b], 0], ids[b, 1:lens[b]])
        a = c["auts"][b % N_E2E]
        assert state[b] == (NONE if a is None else a.walk(ids[b, 1:lens[b]])), f"row {b}: out_state is not the walk's end"
    assert np.isfinite(logp).all() and (logp <= 0).all()
    i0, l0 = eng.recognize_gray(gray, LEN_E2E, automata=hs)
    i1, l1, p1, s1 = eng.recognize_gray(gray, LEN_E2E, scores=True, automata=hs, states=True)
    np.testing.assert_array_equal(i0, ids); np.testing.assert_array_equal(i1, ids); np.testing.assert_array_equal(s1, state)
    np.testing.assert_array_equal(_bits(p1), _bits(logp))
    f_ids, f_lens, f_logp = eng.recognize_gray(gray, LEN_E2E, scores=True)
    for z in (5, 7):
        np.testing.assert_array_equal(f_ids[z], ids[z]); np.testing.assert_array_equal(_bits(f_logp[z]), _bits(logp[z]))
    report(f"soft automata bf16 {name} ({rows} rows, flags {flags}): {len(reached)} of {len(c['flip'])} weighted rows reach their step undiverged and take the "
           f"weighted pick; {len(div)} first divergences of 8, all below {BF16_GAP_TOL}; universal-open / none rows == the free run")


# ------------------------------------------------------------------------------------------------ 3. compaction, sharing, lanes
def test_soft_compacted_equals_uncompacted():
    """early-EOS weights, bf16, 96 rows, max_len 32, automata cycling through (a negative one-token bias on the free run's most
    frequent token, the universal-open automaton, a hard loop, none): rows finish at different steps, the batch is compacted,
    and ids, lengths and states equal those of an engine that never compacts (MOCR_FLAG_NO_COMPACTION)."""
    n, max_len = 96, 32
    gray = np.concatenate([crops(4321, 6), crops(4322, n)])[:n]
    eng = su.score_engine("eos", "bf16", max_batch=96)
    nc = su.score_engine("eos", "bf16", max_batch=96, flags=2048)
    f_ids, f_lens = eng.recognize_gray(gray, max_len)
    toks, counts = np.unique(f_ids[:, 1:], return_counts=True)
    alphabet = [int(t) for t in toks[np.argsort(-counts)] if t not in (0, EOS)][:10]
    assert len(alphabet) >= 4
    auts = [bu.from_sequence_bias({(alphabet[0],): -4.0, (alphabet[1], alphabet[2]): 3.0}), bu.universal_open(), au.loop(alphabet[:4]), None]
    kinds = [k % 4 for k in range(n)]
    out = []
    for e in (eng, nc):
        hs = [_create(e, a) for a in auts[:3]] + [0]
        base = e.compaction_count()
        out.append(e.recognize_gray(gray, max_len, automata=[hs[k] for k in kinds], states=True))
        out.append(e.compaction_count() - base)
    (ids, lens, state), compactions, (u_ids, u_lens, u_state), none = out
    assert compactions > 0 and none == 0
    np.testing.assert_array_equal(ids, u_ids); np.testing.assert_array_equal(lens, u_lens); np.testing.assert_array_equal(state, u_state)
    assert lens.min() < lens.max(), "rows were meant to finish at different steps"
    for b in range(n):
        a = auts[kinds[b]]
        assert state[b] == (NONE if a is None else a.walk(ids[b, 1:lens[b]])), f"row {b}"
    z = np.array([k in (1, 3) for k in kinds])
    np.testing.assert_array_equal(ids[z], f_ids[z]); np.testing.assert_array_equal(lens[z], f_lens[z])
    soft_rows = np.array(kinds) == 0
    assert (ids[soft_rows] != f_ids[soft_rows]).any(), "the bias changed no row"
    report(f"soft automata bf16 early-EOS 96 rows, lengths {int(lens.min())}..{int(lens.max())}: compacted == uncompacted (states too), "
           f"universal-open / none rows == the free run")


def test_four_soft_automata_over_one_encoding():
    """One crop decoded in four rows under four soft automata (chain w1 of row 0, universal-open, the zero-weight loop, and a
    compact sequence_bias automaton with fallback default edges that takes 30 off the free run's first token) through
    sources = [0, 0, 0, 0]: every row equals its row of a call in which all four rows bring that automaton, bit for bit; the
    crop is encoded once."""
    c = _case8()
    eng = su.score_engine("wide", "fp32")
    gray = crops(31, 1)
    h8 = _handles8(eng)
    free_ids, _ = eng.recognize_gray(gray, LEN_E2E)
    f1, f2 = int(free_ids[0, 1]), int(free_ids[0, 2])
    assert EOS not in (f1, f2)
    hs = [h8[0], h8[5], h8[6], _create(eng, bu.from_sequence_bias({(f1,): -30.0, (f1, f2): 1.0}, compact=True))]
    before = eng.encoded_crops()
    ids, lens, logp, state = eng.recognize_gray(gray, LEN_E2E, scores=True, sources=[0] * 4, automata=hs, states=True)
    assert eng.encoded_crops() - before == 1
    for k in range(4):
        i1, l1, p1, s1 = eng.recognize_gray(gray, LEN_E2E, scores=True, sources=[0] * 4, automata=[int(hs[k])] * 4, states=True)
        np.testing.assert_array_equal(i1[k], ids[k]); assert l1[k] == lens[k] and s1[k] == state[k]
        np.testing.assert_array_equal(_bits(p1[k]), _bits(logp[k]))
    np.testing.assert_array_equal(ids[0, :lens[0]], c["ids"][0, :lens[0]])
    np.testing.assert_array_equal(ids[1], free_ids[0])
    assert state[1] == 0 and state[3] >= 0 and ids[3, 1] != f1 and (ids[0] != ids[1]).any()


def test_soft_hard_and_none_across_merged_requests_and_two_lanes():
    """A two-lane bf16 engine, three requests submitted together from three threads - a soft one (the 8-row pattern), a hard
    one (the loop on every row) and a plain one: whatever the scheduler merges and wherever it runs them, every request's rows
    equal the rows of the same request made alone."""
    import threading
    from manga_ocr.engine import Engine
    c = _case8()
    eng = Engine(su.score_weights("wide"), DEFAULT_SPEC, dtype="bf16", device=0, max_batch=64, lanes=2)
    try:
        gray = crops(31, N_E2E)
        hs = [0 if a is None else _create(eng, a) for a in c["auts"]]
        loop = eng.automaton(*au.pack(au.loop(c["alphabet"][:4])))
        reqs = [dict(automata=hs, states=True), dict(automata=loop, states=True), dict()]
        alone = [eng.recognize_gray(gray, LEN_E2E, scores=True, **kw) for kw in reqs]
        for attempt in range(3):
            got = [None] * 3
            def run(i):
                got[i] = eng.recognize_gray(gray, LEN_E2E, scores=True, **reqs[i])
            ts = [threading.Thread(target=run, args=(i,)) for i in range(3)]
            [t.start() for t in ts]; [t.join() for t in ts]
            for i in range(3):
                np.testing.assert_array_equal(got[i][0], alone[i][0], err_msg=f"request {i}: ids"); np.testing.assert_array_equal(got[i][1], alone[i][1])
                if i < 2:
                    np.testing.assert_array_equal(got[i][3], alone[i][3], err_msg=f"request {i}: states")
        for b, (step, f, r, wgt) in c["flip"].items():
            assert alone[0][0][b, step] in (r, f)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 4. graphs, memory, errors
def _desc(eb, et, en, acc, ew=None, dn=None, struct_size=None):
    arrs = [np.ascontiguousarray(eb, np.int32), np.ascontiguousarray(et, np.int32), np.ascontiguousarray(en, np.int32),
            np.ascontiguousarray(acc, np.uint8), None if ew is None else np.ascontiguousarray(ew, np.float32),
            None if dn is None else np.ascontiguousarray(dn, np.int32)]
    d = _capi.MocrSoftAutomatonDesc(C.sizeof(_capi.MocrSoftAutomatonDesc) if struct_size is None else struct_size, len(arrs[3]),
                                    *(None if a is None else a.ctypes.data for a in arrs))
    return d, arrs


def test_soft_graphs_memory_and_errors():
    """A hard automaton allocates the 37 MiB arena and nothing soft; the first soft create adds the 20 MiB of edge_weight and
    default_next (mocr_automaton_state_bytes before and after); a soft batch captures graphs of its own, a repeat none, and a
    later hard or plain batch reuses the graphs it had; every MOCR_ERR_ARG of the two new arrays; the beam entry points refuse
    a soft handle."""
    from manga_ocr._capi import MocrError
    from manga_ocr.engine import BeamConfig
    eng = su.score_engine.__wrapped__("wide", "bf16", max_batch=64)
    try:
        gray = crops(5, 40)
        want, want_l = eng.recognize_gray(gray, 16)
        digits = np.unique(want[:, 1:])
        digits = [int(t) for t in digits if t not in (EOS, 0)][:6]
        h1 = eng.automaton(*au.pack(au.loop(digits[:4])))
        hard = eng.recognize_gray(gray, 16, automata=h1, states=True)
        arena, g_hard = eng.automaton_state_bytes(), eng.graph_count()
        assert (36 << 20) <= arena <= (38 << 20)
        soft_a = bu.from_sequence_bias({(digits[0],): -3.0, (digits[1], digits[2]): 2.0})
        h2 = _create(eng, soft_a)
        grown = eng.automaton_state_bytes() - arena
        assert grown == (1 << 22) * 4 + (1 << 20) * 4, f"the soft arena is {grown} bytes"
        assert eng.graph_count() == g_hard
        again = eng.recognize_gray(gray, 16, automata=h1, states=True)              # the hard batch on its old graphs, same results
        assert eng.graph_count() == g_hard
        for a, b in zip(hard, again):
            np.testing.assert_array_equal(a, b)
        ids, lens, st = eng.recognize_gray(gray, 16, automata=[h2, h1] * 20, states=True)
        g_soft = eng.graph_count()
        assert g_soft > g_hard, "a soft batch captures graphs of its own"
        eng.recognize_gray(gray, 16, automata=h2); eng.recognize_gray(gray, 16, automata=[h2, 0] * 20)
        assert eng.graph_count() == g_soft and eng.automaton_state_bytes() == arena + grown
        np.testing.assert_array_equal(ids[1::2], hard[0][1::2]); np.testing.assert_array_equal(st[1::2], hard[2][1::2])
        for b in range(0, 40, 2):
            assert st[b] == soft_a.walk(ids[b, 1:lens[b]])
        b_ids, b_lens = eng.recognize_gray(gray, 16)
        h_again = eng.recognize_gray(gray, 16, automata=h1, states=True)
        assert eng.graph_count() == g_soft, "a later plain or hard batch reuses its old graphs"
        np.testing.assert_array_equal(b_ids, want); np.testing.assert_array_equal(h_again[0], hard[0])
        h3 = _create(eng, bu.universal_open())                                       # created after the soft graphs were captured
        u_ids, u_lens, u_st = eng.recognize_gray(gray, 16, automata=[h3, h2] * 20, states=True)
        assert eng.graph_count() == g_soft
        np.testing.assert_array_equal(u_ids[0::2], want[0::2]); np.testing.assert_array_equal(u_ids[1::2], eng.recognize_gray(gray, 16, automata=h2)[0][1::2])
        # the refusals
        out = C.c_int32(SENT)
        good = ([0, 2, 2], [10, 11], [1, 1], [0, 1])
        cases = {
            "NaN weight": _desc(*good, ew=[0.5, np.nan]), "+inf weight": _desc(*good, ew=[np.inf, 0.0]), "-inf weight": _desc(*good, ew=[0.0, -np.inf]),
            "default_next = n_states": _desc(*good, dn=[0, 2]), "default_next < -1": _desc(*good, dn=[-2, 0]),
            "EOS as a token of a soft automaton": _desc([0, 2, 2], [EOS, 11], [1, 1], [0, 1], ew=[1.0, 1.0]),
        }
        count = eng.automaton_count()
        for what, (d, keep) in cases.items():
            ref = C.cast(C.pointer(d), C.POINTER(_capi.MocrAutomatonDesc))
            assert eng.lib.mocr_automaton_create(eng._h, ref, C.byref(out)) == -1 and out.value == SENT, what
        d, keep = _desc(*good, ew=[np.nan, np.nan], dn=[7, 7], struct_size=C.sizeof(_capi.MocrAutomatonDesc))
        ref = C.cast(C.pointer(d), C.POINTER(_capi.MocrAutomatonDesc))
        assert eng.lib.mocr_automaton_create(eng._h, ref, C.byref(out)) == 0 and out.value == count + 1, "the short struct: the new fields are not read"
        d, keep = _desc(*good, ew=[0.0, 0.0], dn=[-1, -1])
        ref = C.cast(C.pointer(d), C.POINTER(_capi.MocrAutomatonDesc))
        assert eng.lib.mocr_automaton_create(eng._h, ref, C.byref(out)) == 0 and out.value == count + 2
        for kw in (dict(beam_automata=h2), dict(beam_automata=[h1] * 7 + [h2], beam_states=True)):
            with pytest.raises(MocrError):
                eng.recognize_gray(gray[:8], 16, beam=BeamConfig(2), **kw)
        eng.recognize_gray(gray[:4], 16, beam=BeamConfig(2), beam_automata=h1)        # ... and a hard handle still passes
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 5. ABI twins with a soft handle
@pytest.mark.parametrize("kind", ["device", "gray_host", "images", "regions"])
def test_automaton_twins_take_a_soft_handle(kind):
    """mocr_recognize_<kind>_automaton on the four source kinds with a soft handle on rows 0 and 2 (the middle region of the
    regions call is a sliver), 3 rows, max_len 8: the rows' ids are the same on all four kinds as through Engine.recognize_gray
    on the same planes, out_state is the walk's end, and the weighted first token differs from the unweighted one."""
    import test_gpu_abi_twins as tw
    from manga_ocr.engine import _ptr
    eng = tw._engine()
    gray, page = tw._inputs()
    N, L, T = tw.N, tw.L, tw.T
    dev = kind == "device"
    free_ids, free_lens = eng.recognize_gray(gray, T)
    key = ("soft", id(eng))
    if key not in test_automaton_twins_take_a_soft_handle.cache:
        first = [int(free_ids[r, 1]) for r in (0, 2)]
        a = bu.from_sequence_bias({(t,): -24.0 for t in set(first)})
        test_automaton_twins_take_a_soft_handle.cache[key] = (a, _create(eng, a))
    a, h = test_automaton_twins_take_a_soft_handle.cache[key]
    aut = np.array([h, 0, h], np.int32)
    src = np.array([0, 1, 2], np.int32)

    def block(shape, dtype, fill=0):
        return torch.full(shape, fill, dtype=getattr(torch, dtype), device="cuda") if dev else np.full(shape, fill, dtype=dtype)
    outs = [block((N, L), "int32", -7), block((N,), "int32", -7), block((N,), "int32", -7)]
    tail = [_ptr(outs[0]), _ptr(outs[1]), None, None, None, None, None, None, None, None, 0, _ptr(aut), _ptr(outs[2])]
    fn = getattr(eng.lib, f"mocr_recognize_{kind}_automaton")
    if kind == "device":
        d_gray = torch.from_numpy(gray).cuda()
        rc = fn(eng._h, _ptr(d_gray), N, N, _ptr(src), *tail)
        eng.synchronize()
    elif kind == "gray_host":
        rc = fn(eng._h, _ptr(gray), N, N, _ptr(src), T, *tail)
    elif kind == "images":
        descs, keep = eng._image_descs(list(gray))
        rc = fn(eng._h, descs, N, N, _ptr(src), *tail)
    else:
        descs, keep = eng._image_descs([page], True)
        arr = (_capi.MocrRegion * N)()
        for i, (pg, x, y, w, h_) in enumerate(tw.REGIONS):
            arr[i].page, arr[i].x, arr[i].y, arr[i].width, arr[i].height = pg, x, y, w, h_
        rc = fn(eng._h, descs, 1, arr, N, N, _ptr(src), *tail)
    assert rc == _capi.MOCR_OK, eng.last_error() if hasattr(eng, "last_error") else rc
    ids, lens, state = [o.cpu().numpy() if dev else o for o in outs]
    for r in (0, 2):
        assert lens[r] >= 2 and state[r] == a.walk(ids[r, 1:lens[r]]) >= 0
        if kind != "regions":           # (the regions call reads other pixels: its free run is not recognize_gray's)
            assert ids[r, 1] != free_ids[r, 1], f"row {r}: -24 on the free run's first token changed nothing"
    if kind == "regions":
        assert lens[1] == 0 and state[1] == NONE
    else:
        w_ids, w_lens, w_state = eng.recognize_gray(gray, T, automata=aut, states=True)
        np.testing.assert_array_equal(ids[:, :T], w_ids[:, :T]); np.testing.assert_array_equal(lens, w_lens); np.testing.assert_array_equal(state, w_state)
        np.testing.assert_array_equal(ids[1, :lens[1]], free_ids[1, :lens[1]]); assert state[1] == NONE


test_automaton_twins_take_a_soft_handle.cache = {}


# ------------------------------------------------------------------------------------------------ 6. product surface
def test_product_surface_glossary_and_sequence_bias():
    """MangaOcr.sequence_bias / glossary through recognize_scored(lexicon=...): a strong negative bias on a crop's first
    character changes it; a glossary whose entry starts with what the model reads and continues with a character it would not
    read makes the recognition contain the entry, which Lexicon.find locates; accepted / entry stay None, the state is
    delivered, a crop without a lexicon in the same call decodes freely, and match refuses the soft lexicon."""
    from PIL import Image
    from manga_ocr import MangaOcr
    imgs = [Image.fromarray(g) for g in crops(77, 4)]
    m = MangaOcr(synthetic_seed=0, dtype="fp32", max_batch=8, lanes=1)
    try:
        free = m.recognize_batch_scored(imgs)
        f0 = [int(t) for t in free[0].ids[1:-1]] if int(free[0].ids[-1]) == EOS else [int(t) for t in free[0].ids[1:]]
        assert len(f0) >= 2 and f0[0] not in m.vocab.special_ids
        sb = m.sequence_bias({(f0[0],): -30.0})
        r = m.recognize_scored(imgs[0], lexicon=sb)
        assert int(r.ids[1]) != f0[0] and r.accepted is None and r.entry is None and r.state >= 0 and np.isfinite(r.logprobs).all()
        other = next(t for t in range(5, 64) if t not in f0 and len(m.vocab.tokens[t]) == 1)
        name = m.vocab.tokens[f0[0]] + m.vocab.tokens[other]
        gl = m.glossary([name, m.vocab.tokens[other] + m.vocab.tokens[other]], bonus=40.0)
        recs = m.recognize_batch_scored(imgs, lexicon=[gl, None, gl, None])
        assert gl.find(recs[0].ids) and gl.find(recs[0].ids)[0] == (1, 0) and name in recs[0].text, recs[0].text
        assert recs[0].accepted is None and recs[0].entry is None and recs[0].state >= 0
        assert recs[1].text == free[1].text and recs[1].state == NONE and recs[3].text == free[3].text
        assert m.recognize(imgs[0], lexicon=gl) == recs[0].text
        assert gl.find(free[0].ids) == []
        if hasattr(m, "match"):
            with pytest.raises(ValueError):
                m.match(imgs[0], lexicon=gl)
    finally:
        m.close() if hasattr(m, "close") else None
