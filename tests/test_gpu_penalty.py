"""-m gpu: greedy decoding with a repetition penalty, end to end (include/mocr.h, "repetition penalty").

The goldens of tests/golden/make_penalty_goldens.py - transformers' generate(repetition_penalty=p), alone, with
no_repeat_ngram_size=2 and with a sequence_bias - on the fp32 engine; the reference loop of tests/penalty_util.py on the fp32
engine and on every bf16 decode path (BF16_CASES of tests/test_gpu_ngram.py) with rows of different p in one batch, and on an
engine whose batch is compacted; a penalty beside a token set, a no-repeat size, a glossary and a forced prefix;
rows with p = 1 against a batch without the keyword, bit for bit; a plain batch before and after a penalty batch; the ABI
twins.  Tolerances are those of tests/test_gpu_scores.py and tests/test_gpu_bf16_parity.py times max(p, 1 / p): the penalty
scales a logit's error by at most that factor."""
import os

import numpy as np
import pytest

from gpu_util import crops, report

import bias_util as bu
import constraint_util as cu
import penalty_util as pu
import score_util as su
from manga_ocr import _capi
from manga_ocr.weights import DEFAULT_SPEC, synthetic_weights
from test_gpu_bf16_parity import BF16_GAP_TOL
from test_gpu_constraints import FP32_LOGIT_TOL, _bits
from test_gpu_ngram import BF16_CASES

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V, EOS, START = 6144, 3, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_E2E, LEN_E2E = 8, 32
ERR_ARG = -1                 # MOCR_ERR_ARG (include/mocr.h)
P8 = [2.0, 1.3, 0.8, 2.0, 1.0, 1.3, 0.8, 1.0]


def _scale(p) -> float:
    return max(float(p), 1.0 / float(p))


# ------------------------------------------------------------------------------------------------ 1. transformers' goldens
@pytest.mark.parametrize("kind", ["alone", "ngram", "bias"])
def test_fp32_engine_reproduces_transformers_repetition_penalty(kind):
    """tests/golden/penalty_<kind>.npz on an fp32 engine, p = 1.3, 2.0 and 0.8: ids and lengths identical to transformers'; the
    token scores within 2 x FP32_LOGIT_TOL x max(p, 1 / p) (the fp32 bound of tests/test_gpu_scores.py, scaled) of the float64
    log-softmax of transformers' processed scores; as many rows leave the p = 1 decode as the golden says - at least half."""
    from manga_ocr.engine import Engine
    g = np.load(os.path.join(GOLDEN, f"penalty_{kind}.npz"))
    w = synthetic_weights(int(g["weights_seed"]), eos_bias=float(g["eos_bias"]))
    gray = np.stack([np.random.RandomState(int(s)).randint(0, 256, size=(224, 224), dtype=np.uint8) for s in g["crop_seeds"]])
    ML, B = int(g["max_length"]), len(gray)
    eng = Engine(w, DEFAULT_SPEC, dtype="fp32", device=0, max_batch=8, lanes=1)
    try:
        kw = {}
        if kind == "ngram":
            kw["no_repeat_ngram"] = int(g["ngram"])
        if kind == "bias":
            sb = {tuple(int(t) for t in g["seq_tok"][i, :g["seq_len"][i]]): float(g["seq_bias"][i]) for i in range(len(g["seq_len"]))}
            kw["automata"] = eng.automaton(*bu.pack(bu.from_sequence_bias(sb)))
        free_ids, free_lens = eng.recognize_gray(gray, ML, **kw)
        for k, p in enumerate(g["penalties"]):
            ids, lens, logp = eng.recognize_gray(gray, ML, scores=True, penalty=float(p), **kw)
            np.testing.assert_array_equal(lens, g["lens"][k], err_msg=f"p = {p}: lengths")
            worst = 0.0
            for b in range(B):
                np.testing.assert_array_equal(ids[b, :lens[b]], g["ids"][k, b, :lens[b]], err_msg=f"p = {p} row {b}: not transformers' ids")
                assert (ids[b, lens[b]:] == 0).all()
                worst = max(worst, float(np.abs(logp[b, 1:lens[b]].astype(np.float64) - g["logp"][k, b, 1:lens[b]]).max()))
            bound = 2 * FP32_LOGIT_TOL * _scale(p) + bu.SCORE_TOL
            print(f"fp32 repetition_penalty {kind} p = {p}: max |logp - transformers| {worst:.3e} (bound {bound:.1e})", flush=True)
            assert worst <= bound, worst
            changed = sum(1 for b in range(B) if free_lens[b] != lens[b] or (free_ids[b, :lens[b]] != ids[b, :lens[b]]).any())
            assert changed == int(g["changed"][k]) and changed * 2 >= B, "the penalty changed too few rows: it did not reach the step"
            report(f"repetition penalty fp32 vs transformers generate(repetition_penalty={p}) {kind}: {B} rows, ids and lengths {lens.tolist()} "
                   f"identical, {changed} rows leave the p = 1 decode, logp within {worst:.2e}")
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 2. the reference loop, mixed p
def _case8():
    """the 8 rows of the mixed tests on the widened-margin weights, crops(31, 8), max_len 32, p = P8, computed once on the CPU
    -> dict(ids, pl, masks, lens, gaps, free_ids)"""
    if _case8.cache:
        return _case8.cache
    import ngram_util as nu
    o = su.score_oracle("wide")
    free_ids, _ = su.oracle_run("wide", 31, N_E2E, LEN_E2E)
    with torch.no_grad():
        enc = o.encode(o.preprocess_gray(crops(31, N_E2E)))
    ids, pl, raw, masks = pu.penalty_generate(o, enc, P8, LEN_E2E)
    lens = pu.lengths(ids, EOS)
    _case8.cache.update(ids=ids, pl=pl, masks=masks, lens=lens, gaps=nu.step_gaps(pl, masks), free_ids=free_ids)
    L = min(ids.shape[1], free_ids.shape[1])
    changed = [b for b in range(N_E2E) if (ids[b, :L] != free_ids[b, :L]).any()]
    assert all(P8[b] != 1.0 for b in changed) and len(changed) >= 3, f"the penalties change rows {changed} only"
    _case8.cache["changed"] = changed
    return _case8.cache


_case8.cache = {}


def test_fp32_mixed_penalties_against_the_reference_loop():
    """fp32 engine, 8 rows with p = P8 in one batch.  ids and lengths identical to the reference loop; scores and alternatives
    within 2 x FP32_LOGIT_TOL x max(p, 1 / p) of the float64 log-softmax of the penalised logits; the rows with p = 1 are
    bit-identical, in every output, to their rows of a batch without the keyword; the three kinds of call agree; a plain batch
    returns after the penalty batches what it returned before them (graph reuse)."""
    c = _case8()
    eng = su.score_engine("wide", "fp32")
    gray = crops(31, N_E2E)
    f_ids, f_lens, f_logp, f_ai, f_al = eng.recognize_gray(gray, LEN_E2E, alternatives=True)
    ids, lens, logp, alt_ids, alt_logp = eng.recognize_gray(gray, LEN_E2E, alternatives=True, penalty=P8)
    L = c["ids"].shape[1]
    live = np.arange(L)[None, :] < c["lens"][:, None]
    np.testing.assert_array_equal(np.where(live, ids[:, :L], 0), np.where(live, c["ids"], 0), err_msg="fp32 ids differ from the reference loop's")
    np.testing.assert_array_equal(lens, c["lens"])
    worst = 0.0
    for b in range(N_E2E):
        for t in range(1, lens[b]):
            ref = cu.masked_log_softmax64(c["pl"][b, t - 1], c["masks"][b, t - 1])
            want4, lp4 = cu.masked_top(c["pl"][b, t - 1], c["masks"][b, t - 1])
            np.testing.assert_array_equal(alt_ids[b, t], want4)
            err = max(abs(float(logp[b, t]) - ref[ids[b, t]]), float(np.abs(alt_logp[b, t].astype(np.float64) - lp4).max()))
            assert err <= 2 * FP32_LOGIT_TOL * _scale(P8[b]), (b, t, err)
            worst = max(worst, err)
    assert any((ids[b] != f_ids[b]).any() for b in c["changed"])
    for z in (4, 7):            # p = 1 beside penalised rows
        np.testing.assert_array_equal(ids[z], f_ids[z]); assert lens[z] == f_lens[z]
        np.testing.assert_array_equal(_bits(logp[z]), _bits(f_logp[z])); np.testing.assert_array_equal(alt_ids[z], f_ai[z])
        np.testing.assert_array_equal(_bits(alt_logp[z]), _bits(f_al[z]))
    i0, l0 = eng.recognize_gray(gray, LEN_E2E, penalty=P8)
    i1, l1, p1 = eng.recognize_gray(gray, LEN_E2E, scores=True, penalty=P8)
    np.testing.assert_array_equal(i0, ids); np.testing.assert_array_equal(i1, ids); np.testing.assert_array_equal(_bits(p1), _bits(logp))
    g_ids, g_lens, g_logp, g_ai, g_al = eng.recognize_gray(gray, LEN_E2E, alternatives=True)
    for a, b in ((g_ids, f_ids), (g_lens, f_lens), (g_ai, f_ai)):
        np.testing.assert_array_equal(a, b, err_msg="a plain batch changed after a penalty batch")
    np.testing.assert_array_equal(_bits(g_logp), _bits(f_logp)); np.testing.assert_array_equal(_bits(g_al), _bits(f_al))
    ones = eng.recognize_gray(gray, LEN_E2E, alternatives=True, penalty=1.0)
    for a, b in zip(ones, (f_ids, f_lens, f_logp, f_ai, f_al)):
        np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    report(f"repetition penalty fp32, 8 rows p = {P8}: ids and lengths {lens.tolist()} identical to the reference loop, rows {c['changed']} leave "
           f"their free run, logp / alt_logp within {worst:.2e}; p = 1 rows bit-identical to a batch without the keyword; plain batch unchanged")


def test_fp32_penalty_with_a_set_a_ban_a_glossary_and_a_prefix():
    """fp32 engine, 8 rows, every row p = 1.3 or 2.0: rows 0-1 also under a token set (the free run's tokens banned), rows 2-3
    with no_repeat_ngram = 2, rows 4-5 under a sequence_bias automaton on the free run's first two tokens, rows 6-7 with a
    forced prefix that repeats one token three times (causal: the second and third copy score penalised).  ids and lengths
    identical to the reference loop, the scores within the scaled fp32 bound."""
    o = su.score_oracle("wide")
    free_ids, _ = su.oracle_run("wide", 31, N_E2E, LEN_E2E)
    eng = su.score_engine("wide", "fp32")
    gray = crops(31, N_E2E)
    pens = [1.3, 2.0] * 4
    base = np.ones((N_E2E, V), bool)
    for b in (0, 1):
        base[b, np.unique(free_ids[b, 1:])] = False
        base[b, EOS] = True
    ngr = [0, 0, 2, 2, 0, 0, 0, 0]
    f1, f2 = int(free_ids[4, 1]), int(free_ids[4, 2])
    aut = bu.from_sequence_bias({(f1,): -2.5, (f1, f2): 4.0, (int(free_ids[5, 1]),): 1.5})
    auts = [None] * 4 + [aut, aut] + [None] * 2
    tok = int(free_ids[6, 1])
    prefixes = [None] * 6 + [[tok, tok, tok], [tok, int(free_ids[7, 1]), tok]]
    with torch.no_grad():
        enc = o.encode(o.preprocess_gray(gray))
    ids_o, pl, raw, masks = pu.penalty_generate(o, enc, pens, LEN_E2E, automata=auts, base_masks=base, ngrams=ngr,
                                                prefixes=[p or [] for p in prefixes])
    lens_o = pu.lengths(ids_o, EOS)
    sets = [eng.token_set(np.nonzero(base[b])[0]) if b < 2 else 0 for b in range(N_E2E)]
    h = eng.automaton(*bu.pack(aut))
    ids, lens, logp = eng.recognize_gray(gray, LEN_E2E, scores=True, penalty=pens, token_sets=sets, no_repeat_ngram=ngr,
                                         automata=[0] * 4 + [h, h, 0, 0], prefixes=prefixes)
    np.testing.assert_array_equal(lens, lens_o)
    worst = 0.0
    for b in range(N_E2E):
        np.testing.assert_array_equal(ids[b, :lens[b]], ids_o[b, :lens[b]], err_msg=f"row {b}")
        for t in range(1, lens[b]):
            ref = cu.masked_log_softmax64(pl[b, t - 1], masks[b, t - 1])[ids[b, t]]
            if np.isfinite(ref):
                worst = max(worst, abs(float(logp[b, t]) - ref) / _scale(pens[b]))
    assert worst <= 2 * FP32_LOGIT_TOL, worst
    assert ids[6, 1:4].tolist() == [tok] * 3 and logp[6, 2] != logp[6, 1]
    report(f"repetition penalty fp32 with a token set, no_repeat_ngram 2, a sequence_bias and a forced prefix in one batch: ids and lengths "
           f"{lens.tolist()} identical to the reference loop, logp / max(p, 1/p) within {worst:.2e}")


@pytest.mark.parametrize("name,rows,flags", BF16_CASES)
def test_bf16_penalty_paths(name, rows, flags):
    """bf16, the 8-row pattern repeated over the batch, on every decode path (<= 32 rows, fused head on 64 and 128 tiles, the
    slab path of MOCR_FLAG_NO_FUSED_ARGMAX).  The first 8 rows against the fp32 reference loop under the project's bf16 rule: a
    row equals the reference up to its first divergence, which sits at a reference top-2 margin of the PENALISED logits below
    BF16_GAP_TOL x max(p, 1 / p).  Every repeat of the pattern gives the first 8 rows' ids; the three kinds of call agree; the
    p = 1 rows are bit-identical to a batch without the keyword."""
    c = _case8()
    eng = su.score_engine("wide", "bf16", max_batch=max(64, rows), flags=flags)
    reps = rows // N_E2E
    gray = np.concatenate([crops(31, N_E2E)] * reps)
    pens = P8 * reps
    ids, lens, logp, alt_ids, alt_logp = eng.recognize_gray(gray, LEN_E2E, alternatives=True, penalty=pens)
    L = c["ids"].shape[1]
    div = cu.first_divergences(ids[:N_E2E, :L], c["ids"], c["gaps"])
    for b, t, g in div:
        report(f"[bf16 repetition penalty {name}] row {b}: first divergence at token {t} (penalised reference margin {g:.3e}, p = {P8[b]})")
    assert all(g < BF16_GAP_TOL * _scale(P8[b]) for b, t, g in div), div
    for k in range(1, reps):
        np.testing.assert_array_equal(ids[k * N_E2E:(k + 1) * N_E2E], ids[:N_E2E], err_msg=f"repeat {k} of the pattern differs")
    for b in range(rows):
        np.testing.assert_array_equal(alt_ids[b, 1:lens[b], 0], ids[b, 1:lens[b]])
    assert np.isfinite(logp).all() and (logp <= 0).all()
    i0, l0 = eng.recognize_gray(gray, LEN_E2E, penalty=pens)
    i1, l1, p1 = eng.recognize_gray(gray, LEN_E2E, scores=True, penalty=pens)
    np.testing.assert_array_equal(i0, ids); np.testing.assert_array_equal(i1, ids); np.testing.assert_array_equal(_bits(p1), _bits(logp))
    f_ids, f_lens, f_logp = eng.recognize_gray(gray, LEN_E2E, scores=True)
    for z in (4, 7):
        np.testing.assert_array_equal(f_ids[z], ids[z]); np.testing.assert_array_equal(_bits(f_logp[z]), _bits(logp[z]))
    und = [b for b in c["changed"] if b not in [d[0] for d in div]]
    assert any((ids[b] != f_ids[b]).any() for b in und) or not und, "no undiverged penalised row left its free run"
    report(f"repetition penalty bf16 {name} ({rows} rows, flags {flags}): {len(div)} first divergences of 8, all below {BF16_GAP_TOL} x max(p, 1/p); "
           f"p = 1 rows == the free run bit for bit")


def test_bf16_penalty_compacted_equals_uncompacted():
    """early-EOS weights, bf16, 96 rows (the latent path), every other row under p = 1.3, max_len 64: a compaction needs an
    eighth of the rows finished a chunk or two before the batch ends, and of these crops' plain decodes only some ten end
    before token 24 and the rest near token 32 - too late under max_len 32, early enough under 64.  Rows finish at different
    steps, the batch is compacted - `seen` and p are by ROW, so nothing moves - and ids and lengths equal those of an engine
    that never compacts (MOCR_FLAG_NO_COMPACTION); the p = 1 rows equal the free run."""
    n, max_len = 96, 64
    gray = np.concatenate([crops(4321, 6), crops(4322, n)])[:n]
    pens = [[1.3, 1.0][k % 2] for k in range(n)]
    eng = su.score_engine("eos", "bf16", max_batch=96)
    nc = su.score_engine("eos", "bf16", max_batch=96, flags=2048)
    f_ids, f_lens = eng.recognize_gray(gray, max_len)
    base = eng.compaction_count()
    ids, lens = eng.recognize_gray(gray, max_len, penalty=pens)
    compactions = eng.compaction_count() - base
    u_ids, u_lens = nc.recognize_gray(gray, max_len, penalty=pens)
    assert compactions > 0
    np.testing.assert_array_equal(ids, u_ids); np.testing.assert_array_equal(lens, u_lens)
    z = np.array([p == 1.0 for p in pens])
    np.testing.assert_array_equal(ids[z], f_ids[z]); np.testing.assert_array_equal(lens[z], f_lens[z])
    assert (ids[~z] != f_ids[~z]).any(), "the penalty changed no row"
    report(f"repetition penalty bf16 early-EOS 96 rows, lengths {int(lens.min())}..{int(lens.max())}: compacted == uncompacted, p = 1 rows == the free run")


def test_bf16_penalty_latent_compacted_on_two_lanes():
    """early-EOS weights, bf16, the latent path (MOCR_FLAG_LATENT), two lanes with a batch of 40 rows in flight on each (the
    same 40 crops and penalties on both), max_len 48, p cycling through P8: rows finish at different steps and both lanes
    compact - `seen` and p are by ROW and every lane has its own buffers and staging, so nothing moves and nothing is shared.
    Every row against the fp32 reference loop under the bf16 rule: equal up to its first divergence, which sits at a reference
    top-2 margin of the PENALISED logits below BF16_GAP_TOL x max(p, 1 / p); the two lanes agree row for row; the p = 1 rows
    are the free run's."""
    import ngram_util as nu
    from manga_ocr.engine import Engine
    n, max_len = 40, 48
    g = np.concatenate([crops(4321, 6), crops(4322, n)])[:n]
    pens = [P8[k % 8] for k in range(n)]
    o = su.score_oracle("eos")
    with torch.no_grad():
        enc = o.encode(o.preprocess_gray(g))
    ids_o, pl, raw, masks = pu.penalty_generate(o, enc, pens, max_len)
    gaps = nu.step_gaps(pl, masks)
    eng = Engine(su.score_weights("eos"), DEFAULT_SPEC, dtype="bf16", device=0, max_batch=n, flags=64, lanes=2)
    try:
        gray = np.tile(g, (2, 1, 1))
        f_ids, f_lens = eng.recognize_gray(gray, max_len)
        base = eng.compaction_count()
        ids, lens = eng.recognize_gray(gray, max_len, penalty=pens * 2)
        compactions = eng.compaction_count() - base
    finally:
        eng.close()
    assert compactions > 0 and lens.min() < lens.max(), (compactions, lens)
    np.testing.assert_array_equal(ids[:n], ids[n:], err_msg="the two lanes decode the same rows differently")
    np.testing.assert_array_equal(lens[:n], lens[n:])
    L = ids_o.shape[1]
    div = cu.first_divergences(ids[:n, :L], ids_o, gaps)
    for b, t, gp in div:
        report(f"[bf16 repetition penalty two lanes] row {b}: first divergence at token {t} (penalised reference margin {gp:.3e}, p = {pens[b]})")
    assert all(gp < BF16_GAP_TOL * _scale(pens[b]) for b, t, gp in div), div
    assert len(div) * 2 <= n, f"{len(div)} of {n} rows diverge"
    z = np.array([p == 1.0 for p in pens * 2])
    np.testing.assert_array_equal(ids[z], f_ids[z]); np.testing.assert_array_equal(lens[z], f_lens[z])
    assert (ids[~z] != f_ids[~z]).any(), "the penalty changed no row"
    report(f"repetition penalty bf16 latent, 2 lanes x {n} rows, max_len {max_len}: {compactions} compactions, lengths {int(lens.min())}..{int(lens.max())}, "
           f"{len(div)} first divergences of {n}, all below {BF16_GAP_TOL} x max(p, 1/p); lanes agree; p = 1 rows == the free run")


# ------------------------------------------------------------------------------------------------ 3. errors and the ABI twins
def test_penalty_argument_errors_and_memory(request):
    """p = 0, negative, inf and NaN are MOCR_ERR_ARG through the C ABI before any work - a refused call allocates nothing; a
    beam request with a penalty is a ValueError.  Memory, on a fresh engine that has no automaton: the first penalty batch
    allocates the automaton arena with its soft part and the lane's row states (mocr_automaton_state_bytes: 0 before, the
    arena's 57 MiB + 12 B a row after), the second penalty batch and a batch with p = 1 everywhere allocate nothing more."""
    from manga_ocr.engine import BeamConfig, Engine, _ptr
    eng = Engine(su.score_weights("wide"), DEFAULT_SPEC, dtype="fp32", device=0, max_batch=8, lanes=1)
    request.addfinalizer(eng.close)
    gray = crops(31, 2)
    state_bytes = lambda: int(eng.lib.mocr_automaton_state_bytes(eng._h))
    assert state_bytes() == 0
    ids = np.zeros((2, DEFAULT_SPEC.max_len), np.int32); lens = np.zeros(2, np.int32)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        pen = np.array([1.0, bad], np.float32)
        rc = eng.lib.mocr_recognize_gray_host_penalty(eng._h, _ptr(gray), 2, 2, None, 8, _ptr(ids), _ptr(lens), None, None, None, None, None, None,
                                                      None, None, 0, None, None, _ptr(pen))
        assert rc == ERR_ARG, (bad, rc)
        with pytest.raises(ValueError):
            eng.recognize_gray(gray, 8, penalty=[1.0, bad])
    with pytest.raises(ValueError):
        eng.recognize_gray(gray, 8, beam=BeamConfig(2), penalty=1.3)
    a, b = eng.recognize_gray(gray, 8)
    assert (b >= 2).all() and state_bytes() == 0, "a refused or a plain call allocated penalty state"
    eng.recognize_gray(gray, 8, penalty=1.0)
    assert state_bytes() == 0, "p = 1 on every row is a plain batch"
    eng.recognize_gray(gray, 8, penalty=[1.3, 1.0])
    arena = ((1 << 20) + 1) * 4 + 2 * (1 << 22) * 4 + (1 << 20) + (1 << 22) * 4 + (1 << 20) * 4      # AUT_ARENA_BYTES + AUT_SOFT_ARENA_BYTES
    first = state_bytes()
    assert first > arena and (first - arena) % 12 == 0 and first - arena <= 12 * 1024, (first, arena)
    eng.recognize_gray(gray, 8, penalty=[2.0, 0.8])
    eng.recognize_gray(gray, 8, scores=True, penalty=[1.0, 1.0])
    assert state_bytes() == first, "a later penalty batch allocated again"


@pytest.mark.parametrize("kind", ["device", "gray_host", "images", "regions"])
def test_penalty_twin_with_null_is_the_automaton_call(kind):
    """mocr_recognize_<kind>_penalty with penalty = NULL against mocr_recognize_<kind>_automaton on the same inputs, 3 rows,
    max_len 8: ids, lengths and scores bit for bit; with p = 2 on row 0 the call runs and rows 1 and 2 keep their ids."""
    import test_gpu_abi_twins as tw
    from manga_ocr.engine import _ptr
    eng = tw._engine()
    gray, page = tw._inputs()
    N, L, T = tw.N, tw.L, tw.T
    dev = kind == "device"
    src = np.array([0, 1, 2], np.int32)

    def call(variant, pen):
        def block(shape, dtype, fill=0):
            return torch.full(shape, fill, dtype=getattr(torch, dtype), device="cuda") if dev else np.full(shape, fill, dtype=dtype)
        outs = [block((N, L), "int32", -7), block((N,), "int32", -7), block((N, L), "float32", -7)]
        tail = [_ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), None, None, None, None, None, None, None, 0, None, None]
        if variant == "penalty":
            tail.append(_ptr(pen))
        fn = getattr(eng.lib, f"mocr_recognize_{kind}_{variant}")
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
        assert rc == _capi.MOCR_OK, rc
        return [o.cpu().numpy() if dev else o for o in outs]

    want = call("automaton", None)
    got = call("penalty", None)
    for g, w_ in zip(got, want):
        np.testing.assert_array_equal(g.view(np.uint32), w_.view(np.uint32), err_msg=f"{kind}: penalty = NULL is not the _automaton call")
    pen = call("penalty", np.array([2.0, 1.0, 1.0], np.float32))
    for r in (1, 2):
        np.testing.assert_array_equal(pen[0][r], want[0][r]); np.testing.assert_array_equal(pen[2][r].view(np.uint32), want[2][r].view(np.uint32))
    if kind == "regions":           # (the regions call reads other pixels: its rows are not recognize_gray's; row 1 is a sliver)
        assert 2 <= pen[1][0] <= T and pen[0][0, 0] == START and (pen[0][0, pen[1][0]:] == 0).all()
    else:
        w_ids, w_lens, w_logp = eng.recognize_gray(gray, T, scores=True, penalty=[2.0, 1.0, 1.0])
        np.testing.assert_array_equal(pen[0][:, :T], w_ids[:, :T], err_msg=f"{kind}: not Engine.recognize_gray(penalty=[2, 1, 1])")
        np.testing.assert_array_equal(pen[1], w_lens); np.testing.assert_array_equal(pen[2][:, :T].view(np.uint32), w_logp[:, :T].view(np.uint32))
