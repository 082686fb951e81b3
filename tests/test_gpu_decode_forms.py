"""-m gpu: which named form of the three kernels that end a decode step - the token kernel, the beam selection, the fused LM
head - every decode mode runs.  An instrumented (eager) pass names its launches: each mode must run exactly the expected
`dec_token*` / `beam_select*` / `gemm_dec_vocab*` names and give the ids of the uninstrumented call.  The names are literals
here, not read from the engine: they pin the mode -> form mapping of csrc/engine.hip's form tables."""
import functools

import numpy as np
import pytest

from gpu_util import crops, engine
from manga_ocr.engine import BeamConfig

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")      # before the engine's library: one HIP runtime per process, torch's

MAX_LEN = 6
MAX_BATCH = 96
EPI_ARGMAX = 6                            # the plan's vocabulary epilogue of the fused LM head (csrc/kernels_gemm.h)
WATCHED = ("dec_token", "beam_select", "gemm_dec_vocab")


def _engine():
    """one bf16 engine for every case: the product's automatic path choice, so that 8 rows take the small-batch path"""
    return engine("bf16", max_batch=MAX_BATCH, auto_path=True)


@functools.lru_cache(maxsize=None)
def _fused_rows():
    """the smallest row count whose decode plan has the fused LM head on the 64 / 128 tile"""
    eng = _engine()
    for rows in range(9, MAX_BATCH + 1):
        pl = eng.decode_plan(rows)
        if pl["vocab_epi"] == EPI_ARGMAX and pl["launch_tile"] in (64, 128) and pl["vocab_split"] == 1:
            return rows
    raise AssertionError(f"no batch of up to {MAX_BATCH} rows has the fused LM head in its plan")


@functools.lru_cache(maxsize=None)
def _handles():
    """a token set, a hard automaton (one accepting state, a loop on every token from 4 on) and its soft twin (weight 0.5 on
    every edge, open), created once on the shared engine"""
    eng = _engine()
    tok = np.arange(4, 6144, dtype=np.int32)
    loop = ([0, tok.size], tok, np.zeros(tok.size, np.int32), [1])
    return dict(set=eng.token_set(range(100, 3000)), hard=eng.automaton(*loop),
                soft=eng.automaton(*loop, edge_weight=np.full(tok.size, 0.5, np.float32), default_next=[0]))


def _run_named(call):
    """(the outputs of call(), the watched profile names that ran) of an instrumented pass"""
    eng = _engine()
    eng.profile_enable(True)
    try:
        eng.profile_reset()
        out = call()
        ran = {s["name"] for s in eng.profile_get() if s["launches"] > 0}
    finally:
        eng.profile_enable(False)
    return out, {n for n in ran if n.startswith(WATCHED)}


def _check(call, expected):
    plain = call()
    out, ran = _run_named(call)
    assert ran == set(expected), sorted(ran)
    for a, b in zip(plain, out):
        np.testing.assert_array_equal(a, b)


# kind -> (keywords, token-name suffix, head-name suffix); "prefix" scores by itself (level >= 1) and runs the MASK forms
KINDS = {
    "plain": (lambda h: {}, "", None),
    "set": (lambda h: dict(token_sets=h["set"]), "_m", "_m"),
    "ngram": (lambda h: dict(no_repeat_ngram=2), "_ng", "_m"),
    "prefix": (lambda h: dict(prefixes="PER_ROW"), "_m", "_m"),
    "automaton": (lambda h: dict(automata=h["hard"]), "_am", "_m"),
    "soft": (lambda h: dict(automata=h["soft"]), "_sw", "_sw"),
    "penalty": (lambda h: dict(penalty=1.3), "_rp", "_rp"),
}
LEVELS = [({}, ""), (dict(scores=True), "_lse"), (dict(alternatives=True), "_topk")]
GREEDY = [(kind, level) for kind in KINDS for level in range(3) if not (kind == "prefix" and level == 0)]
# the names the cases below expect, written out: 18 step names and 6 head names
STEP_NAMES = {"dec_token", "dec_token_m", "dec_token_ng", "dec_token_am", "dec_token_sw", "dec_token_rp",
              "dec_token_lse", "dec_token_lse_m", "dec_token_lse_ng", "dec_token_lse_am", "dec_token_lse_sw", "dec_token_lse_rp",
              "dec_token_topk", "dec_token_topk_m", "dec_token_topk_ng", "dec_token_topk_am", "dec_token_topk_sw", "dec_token_topk_rp"}
HEAD_NAMES = {"gemm_dec_vocab", "gemm_dec_vocab_lse", "gemm_dec_vocab_topk", "gemm_dec_vocab_m", "gemm_dec_vocab_sw", "gemm_dec_vocab_rp"}


def _greedy_names(kind, level, fused):
    _, tok, head = KINDS[kind]
    step = "dec_token" + LEVELS[level][1] + tok
    names = {"dec_token_first", step}
    if fused:
        names.add("gemm_dec_vocab" + (head if head is not None else LEVELS[level][1]))
    return step, names


def test_the_greedy_cases_name_every_step_and_head_form():
    steps, heads = set(), set()
    for kind, level in GREEDY:
        step, names = _greedy_names(kind, level, True)
        steps.add(step)
        heads |= {n for n in names if n.startswith("gemm_dec_vocab")}
    assert steps == STEP_NAMES and heads == HEAD_NAMES


@pytest.mark.parametrize("fused", [False, True], ids=["small-batch", "fused-head"])
@pytest.mark.parametrize("kind,level", GREEDY)
def test_greedy_mode_runs_its_named_forms(kind, level, fused):
    """8 rows on the small-batch path (its LM head is sm_vocab: no gemm_dec_vocab* name at all) and the smallest batch with the
    fused LM head on a 64 / 128 tile: the start token's kernel, the mode's token kernel and, fused, the mode's LM head - no other"""
    eng = _engine()
    rows = _fused_rows() if fused else 8
    assert (eng.decode_plan(rows)["path"] == "small-batch") == (not fused)
    kw = dict(LEVELS[level][0])
    kw.update(KINDS[kind][0](_handles()))
    if kw.get("prefixes") == "PER_ROW":
        kw["prefixes"] = [[10, 11]] * rows
    gray = np.concatenate([crops(31, 8)] * ((rows + 7) // 8))[:rows]
    step, names = _greedy_names(kind, level, fused)
    assert step in STEP_NAMES and names - {"dec_token_first", step} <= HEAD_NAMES
    _check(lambda: eng.recognize_gray(gray, MAX_LEN, **kw), names)


# beam mode -> (keywords, selection name without / with positions)
BEAM = {
    "plain": (lambda h: {}, "beam_select", "beam_select"),
    "scores": (lambda h: dict(beam_scores=True), "beam_select_tok", "beam_select_tok"),
    "automaton": (lambda h: dict(beam_automata=h["hard"]), "beam_select_am", "beam_select_am_tr"),
    "soft": (lambda h: dict(beam_automata=h["soft"], beam_soft=True), "beam_select_sw", "beam_select_sw_tr"),
}


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("positions", [False, True], ids=["", "positions"])
@pytest.mark.parametrize("mode", list(BEAM))
def test_beam_mode_runs_its_named_selection(mode, positions, K):
    """2 crops x K beams: the start token's kernel, the slab LM head and the mode's selection - no token kernel, no other head"""
    eng = _engine()
    make, name, name_tr = BEAM[mode]
    kw = make(_handles())
    if positions:
        kw["beam_positions"] = True
    gray = crops(31, 2)
    _check(lambda: eng.recognize_gray(gray, MAX_LEN, beam=BeamConfig(K), **kw),
           {"dec_token_first", "gemm_dec_vocab", name_tr if positions else name})
