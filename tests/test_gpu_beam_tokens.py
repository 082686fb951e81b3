"""-m gpu: beam search with token sets and token scores through the engine (include/mocr.h, "beam search with token sets and
token scores").

* fp32 engine against transformers' constrained beam search and its transition scores (tests/golden/beam_tok_*.npz): ids and
  lengths identical, sequence scores within 1e-3 (the bound of tests/test_gpu_beam.py; every crop's min_gap is >= 1e-3,
  tests/test_beam_tokens_cpu.py), token scores within 2e-3 - the bound tests/test_gpu_scores.py puts on the fp32 engine's
  greedy token scores (twice the teacher-forced logit tolerance), the same log-softmax of the same head.
* Identity, per kernel regime: asking for token scores, or passing sets that are all ALL, moves no id, length or score; the
  sequential fp32 sum of a hypothesis' token scores / (len - 1) ^ length_penalty IS its sequence score (1e-6 relative: one
  division and one powf against numpy's); logp[0] and the tail are 0, everything else finite and <= 0.
* Sets: every token is EOS or a member; rolling crops and sets together rolls the results; a crop under ALL among constrained
  crops is the crop of an all-ALL batch.
* bf16 token scores against the same engine's teacher-forced scored decode of the same hypotheses (unconstrained only: the
  greedy sets renormalise their softmax over the set, the beam sets do not, so the two are different numbers under a set).
* Graph replay equals eager steps across a context bucket; token batches leave greedy and plain beam results as they were;
  the token state is allocated by the first token batch; no new graph on a repeated call; the device twin; MangaOcr."""
import os

import numpy as np
import pytest

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
PUBLISHED = BeamConfig(4, 2.0, True, 3)
INV_EOS_BIAS = 1.7                       # tests/test_gpu_beam.py: crops end at different steps below 16 tokens
SEQ_SCORE_TOL = 1e-3                     # tests/test_gpu_beam.py::test_fp32_engine_returns_the_transformers_hypotheses
TOKEN_SCORE_TOL = 2e-3                   # tests/test_gpu_scores.py: 2 x FP32_LOGIT_TOL, fp32 greedy token scores end to end
BF16_SCORE_TOL = 2 * 1.466e-3            # tests/test_gpu_beam.py::test_bf16_scores_against_the_reference
REGIMES = [("classic, fp32", "fp32", 0, False), ("auto (classic), bf16", "bf16", 0, True), ("latent, bf16", "bf16", LATENT_ALWAYS, False),
           ("fp8 attention, bf16", "bf16", LATENT_ALWAYS | FP8, False)]


def golden(name):
    g = np.load(os.path.join(GOLD, f"beam_tok_{name}.npz"))
    return {k: g[k] for k in g.files}


def golden_crops(g):
    return np.stack([np.random.RandomState(int(s)).randint(0, 256, size=(224, 224), dtype=np.uint8) for s in g["crop_seeds"]])


def random_set(seed, size):
    return sorted(int(x) for x in np.random.RandomState(seed).choice(np.arange(5, V), size, replace=False))


def check_logp(ids, lens, scores, logp, lp):
    """what every token-score block must satisfy, and the identity with the sequence scores -> its largest relative error"""
    worst = 0.0
    assert logp.dtype == np.float32 and logp.shape == ids.shape and np.isfinite(logp).all() and (logp <= 0).all()
    for c in range(ids.shape[0]):
        for j in range(ids.shape[1]):
            L = int(lens[c, j])
            assert logp[c, j, 0] == 0 and (logp[c, j, L:] == 0).all(), f"crop {c} hypothesis {j}: the start token and the tail score 0"
            if L:
                assert (logp[c, j, 1:L] < 0).all()
                mine = tu.sequential_score(logp[c, j], L, lp)
                rel = abs(float(mine) - float(scores[c, j])) / abs(float(scores[c, j]))
                worst = max(worst, rel)
                assert rel <= 1e-6, f"crop {c} hypothesis {j}: sequential sum {mine!r} against score {scores[c, j]!r}"
    return worst


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_fp32_engine_against_transformers(name):
    """Measured on the MI355X, engine against golden, the largest over each case's crops: sequence scores 4.8e-7 (a) and
    9.5e-7 (b)-(e); token scores 1.9e-6 (a), 9.5e-7 (b), 1.4e-6 (c), 1.9e-6 (d), 1.4e-6 (e).  The bounds of the
    module's docstring (1e-3 and 2e-3, those of the plain beam test and of the greedy token scores) hold with room."""
    g = golden(name)
    ML, K, lp = int(g["max_length"]), int(g["num_beams"]), float(g["length_penalty"])
    cfg = BeamConfig(K, lp, ES[int(g["early_stopping"])], int(g["no_repeat_ngram_size"]))
    eng = engine("fp32", seed=int(g["weights_seed"]), eos_bias=float(g["eos_bias"]), max_batch=24)
    handles = [0 if (row < 0).all() else eng.token_set(row[row >= 0].tolist()) for row in g["sets"]]
    kw = dict(beam_sets=handles) if any(handles) else {}
    ids, lens, scores, logp = eng.recognize_gray(golden_crops(g), max_len=ML, beam=cfg, beam_scores=True, **kw)
    e_seq = float(np.abs(scores.astype(np.float64) - g["scores"]).max())
    same = np.array_equal(lens, g["lens"]) and np.array_equal(ids[:, :, :ML], g["ids"])
    e_tok = float(np.abs(logp[:, :, :ML].astype(np.float64) - g["logp"]).max()) if same else float("nan")
    report(f"beam tokens fp32 case ({name}): {ids.shape[0]} crops x {K} hypotheses, sets {[int((r >= 0).sum()) for r in g['sets']]}; "
           f"sequence scores within {e_seq:.2e} (bound {SEQ_SCORE_TOL:.0e}), token scores within {e_tok:.2e} (bound {TOKEN_SCORE_TOL:.0e})")
    np.testing.assert_array_equal(lens, g["lens"])
    np.testing.assert_array_equal(ids[:, :, :ML], g["ids"])
    assert (ids[:, :, ML:] == PAD).all() and (logp[:, :, ML:] == 0).all()
    assert e_seq <= SEQ_SCORE_TOL
    assert e_tok <= TOKEN_SCORE_TOL
    check_logp(ids, lens, scores, logp, lp)


@pytest.mark.parametrize("name,dtype,flags,auto", REGIMES)
def test_identity_and_sets(name, dtype, flags, auto):
    ML, K, n = 16, 4, 6
    gray = crops(4321, n)
    eng = engine(dtype, seed=1, eos_bias=INV_EOS_BIAS, max_batch=24, flags=flags, auto_path=auto)
    plain = eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED)
    scored = eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED, beam_scores=True)
    all_sets = eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED, beam_sets=[0] * n)
    both = eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED, beam_scores=True, beam_sets=0)
    assert len(scored) == 4 and len(all_sets) == 3 and len(both) == 4
    for blk, p, a, b, c in zip(("ids", "lens", "scores"), plain, scored, all_sets, both):
        for other, what in ((a, "beam_scores=True"), (b, "sets all ALL"), (c, "both")):
            np.testing.assert_array_equal(other.view(np.int32), p.view(np.int32), err_msg=f"{name}: {blk} move with {what}")
    np.testing.assert_array_equal(both[3], scored[3])
    worst = check_logp(*scored, PUBLISHED.length_penalty)
    assert (scored[1][:, 0] >= 2).all(), "every crop has a best hypothesis"
    graphs = eng.graph_count()
    again = eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED, beam_scores=True)
    assert eng.graph_count() == graphs, "repeating the call adds no graph"
    for a, b in zip(again, scored):
        np.testing.assert_array_equal(a, b)
    # ---- sets: three of them and two crops under ALL, in one call
    lists = [random_set(40, 40), None, random_set(12, 12), random_set(41, 40), None, random_set(40, 40)]
    handles = [0 if s is None else eng.token_set(s) for s in lists]
    ids, lens, scores, logp = eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED, beam_scores=True, beam_sets=handles)
    check_logp(ids, lens, scores, logp, PUBLISHED.length_penalty)
    changed = 0
    for c, s in enumerate(lists):
        for j in range(K):
            toks = ids[c, j, 1:lens[c, j]]
            if s is not None:
                assert np.isin(toks, s + [EOS]).all(), f"{name}: crop {c} hypothesis {j} leaves its set: {toks}"
        if s is None:       # a crop under ALL among constrained crops = the crop of the all-ALL batch of the same size
            for blk, got, want in zip(("ids", "lens", "scores", "logp"), (ids, lens, scores, logp), scored):
                np.testing.assert_array_equal(got[c], want[c], err_msg=f"{name}: {blk} of the unconstrained crop {c}")
        else:
            changed += not np.array_equal(ids[c], plain[0][c])
    assert changed >= 3, "the sets change the search"
    # the same crops and sets at other batch positions
    moved = eng.recognize_gray(np.roll(gray, 1, axis=0), max_len=ML, beam=PUBLISHED, beam_scores=True, beam_sets=handles[-1:] + handles[:-1])
    for a, b, blk in zip(moved, (ids, lens, scores, logp), ("ids", "lens", "scores", "logp")):
        np.testing.assert_array_equal(a, np.roll(b, 1, axis=0), err_msg=f"{name}: {blk} depend on the batch position")
    report(f"beam tokens {name}: {n} crops x {K}: token scores and ALL sets move nothing; sequential sum / (len - 1)^lp = score within "
           f"{worst:.1e} relative; 4 constrained crops stay in their sets, ALL crops and rolled batches identical")


def test_bf16_token_scores_against_the_teacher_forced_scores():
    """The pattern of tests/test_gpu_beam.py::test_bf16_scores_against_the_reference, on the engine's own hypotheses: their
    token scores from the selection against the scored, prefix-forced greedy decode of the same tokens, as length-normalised
    sums with that test's bound.  Unconstrained only: under a set the greedy path renormalises its softmax over the set and
    the beam path does not, so the two score different things."""
    g = golden("a")
    ML, K, lp = int(g["max_length"]), int(g["num_beams"]), float(g["length_penalty"])
    gray = golden_crops(g)
    n = gray.shape[0]
    eng = engine("bf16", seed=int(g["weights_seed"]), eos_bias=float(g["eos_bias"]), max_batch=24, auto_path=True)
    ids, lens, scores, logp = eng.recognize_gray(gray, max_len=ML, beam=BeamConfig(K, lp, True, 3), beam_scores=True)
    check_logp(ids, lens, scores, logp, lp)
    prefixes = [ids[c, j, 1:lens[c, j]].tolist() or None for c in range(n) for j in range(K)]
    _, flens, forced = eng.recognize_gray(gray, max_len=ML, scores=True, prefixes=prefixes, sources=[c for c in range(n) for _ in range(K)])
    worst_seq, worst_tok, cnt = 0.0, 0.0, 0
    for r, (c, j) in enumerate((c, j) for c in range(n) for j in range(K)):
        L = int(lens[c, j])
        if L == 0:
            continue
        assert flens[r] == L
        cnt += 1
        worst_tok = max(worst_tok, float(np.abs(forced[r, 1:L].astype(np.float64) - logp[c, j, 1:L]).max()))
        worst_seq = max(worst_seq, abs(float(forced[r, 1:L].astype(np.float64).sum()) / float(L - 1) ** lp - float(scores[c, j])))
    report(f"beam tokens bf16 vs the engine's teacher-forced scores, {cnt} hypotheses: length-normalised scores within {worst_seq:.3e} "
           f"(bound {BF16_SCORE_TOL:.1e}), single tokens within {worst_tok:.3e}")
    assert cnt >= n and worst_seq <= BF16_SCORE_TOL


@pytest.mark.parametrize("name,dtype,flags", [("classic, fp32", "fp32", 0), ("latent, bf16", "bf16", LATENT_ALWAYS)])
def test_a_long_token_batch_replays_graphs_as_it_runs_eagerly(name, dtype, flags):
    """104 tokens on weights that never emit EOS (tests/test_gpu_beam.py): the token batch crosses the context bucket at 96"""
    ML, K, n = 104, 4, 3
    gray = crops(808, n)
    cfg = BeamConfig(K, 1.0, False, 3)
    kw = dict(seed=0, max_batch=n * K)
    sets = [random_set(7, 3000), None, random_set(8, 200)]
    out = []
    for f in (0, NO_GRAPH):
        eng = engine(dtype, flags=flags | f, **kw)
        out.append(eng.recognize_gray(gray, max_len=ML, beam=cfg, beam_scores=True, beam_sets=[0 if s is None else eng.token_set(s) for s in sets]))
    ids, lens, scores, logp = out[0]
    assert (lens[1] == ML).all(), "the unconstrained crop ends on the length rule, behind the bucket boundary at 96"
    check_logp(ids, lens, scores, logp, 1.0)
    for c, s in enumerate(sets):
        assert s is None or all(np.isin(ids[c, j, 1:lens[c, j]], s + [EOS]).all() for j in range(K))
    for a, b, blk in zip(out[0], out[1], ("ids", "lens", "scores", "logp")):
        np.testing.assert_array_equal(a, b, err_msg=f"{name}: {blk} of the graph replay differ from the eager steps")
    report(f"beam tokens {name}: {n} crops x {K}, {ML} tokens each under sets of 3000 / ALL / 200, graph replay identical to eager steps")


def test_token_batches_leave_greedy_and_plain_beam_results_alone():
    ML = 12
    gray = crops(99, 6)

    some = random_set(5, 60)

    def calls(e):
        h = e.token_set(some)
        out = [e.recognize_gray(gray, max_len=ML), e.recognize_gray(gray, max_len=ML, scores=True, token_sets=[h, 0, h, 0, h, 0]),
               e.recognize_gray(gray[:3], max_len=ML, no_repeat_ngram=2), e.recognize_gray(gray, max_len=ML, beam=PUBLISHED),
               e.recognize_gray(gray[:3], max_len=ML, beam=BeamConfig(2, 1.0, False, 0))]
        return [a for o in out for a in o]

    kw = dict(seed=1, eos_bias=1.2, max_batch=24, auto_path=True)
    clean, mixed = engine("bf16", lanes=1, **kw), engine("bf16", lanes=2, **kw)      # (another cache key: its own engine)
    want = calls(clean)
    assert clean.beam_token_state_bytes() == 0, "plain beam and greedy calls allocate no token state"
    got = calls(mixed)
    plain_bytes = mixed.beam_state_bytes()
    assert mixed.beam_token_state_bytes() == 0
    mixed.recognize_gray(gray, max_len=ML, beam=PUBLISHED, beam_scores=True)
    one = mixed.beam_token_state_bytes()
    assert one > 0 and one % (2 * 4 * DEFAULT_SPEC.max_len) == 0
    got2 = calls(mixed)
    mixed.recognize_gray(gray[:3], max_len=ML, beam=BeamConfig(2, 1.0, False, 0), beam_sets=[mixed.token_set(some), 0, mixed.token_set(some)])
    got3 = calls(mixed)
    assert mixed.beam_token_state_bytes() in (one, 2 * one), "at most once per lane"
    assert mixed.beam_state_bytes() in (plain_bytes, 2 * plain_bytes) and mixed.beam_state_bytes() % (5 + DEFAULT_SPEC.max_len) == 0
    for a, b, c, w in zip(got, got2, got3, want):
        np.testing.assert_array_equal(a, w)
        np.testing.assert_array_equal(b, w)
        np.testing.assert_array_equal(c, w)


def test_the_device_twin_equals_the_host_call():
    ML, K, n = 16, 3, 5
    gray = crops(77, n)
    cfg = BeamConfig(K, 1.0, False, 2)
    eng = engine("bf16", seed=1, eos_bias=INV_EOS_BIAS, max_batch=24, auto_path=True)
    handles = [eng.token_set(random_set(40, 40)), 0, 0, eng.token_set(random_set(12, 12)), 0]
    want = eng.recognize_gray(gray, max_len=ML, beam=cfg, beam_scores=True, beam_sets=handles)
    L = DEFAULT_SPEC.max_len
    d_gray = torch.from_numpy(gray).cuda()
    d_ids = torch.full((n, K, L), -5, dtype=torch.int32, device="cuda")
    d_len = torch.full((n, K), -5, dtype=torch.int32, device="cuda")
    d_score = torch.full((n, K), 5.0, dtype=torch.float32, device="cuda")
    d_logp = torch.full((n, K, L), 5.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.set_generate_max_length(ML)
    try:
        eng.recognize_device(d_gray, n, d_ids, d_len, beam=cfg, d_out_score=d_score, d_out_beam_logp=d_logp, beam_sets=handles)
        eng.synchronize()
    finally:
        eng.set_generate_max_length(L)
    for got, w, blk in zip((d_ids, d_len, d_score, d_logp), want, ("ids", "lens", "scores", "logp")):
        np.testing.assert_array_equal(got.cpu().numpy(), w, err_msg=f"device twin: {blk}")


def test_manga_ocr_hypotheses_with_token_scores_under_a_set(tmp_path):
    from dataclasses import replace
    from PIL import Image
    from hf_dir import write_hf_dir
    from manga_ocr import MangaOcr
    ML = 16
    d = str(tmp_path / "manga-ocr-base")
    write_hf_dir(d, seed=1, spec=replace(DEFAULT_SPEC, max_len=ML), eos_bias=INV_EOS_BIAS)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = MangaOcr(d, dtype="fp32", max_batch=8, lanes=1)
    try:
        chars = "".join(chr(0x4E00 + i) for i in range(100, 160))
        ts = m.token_set(chars=chars)
        imgs = [Image.fromarray(g, mode="L") for g in crops(55, 3)]
        hyps = m.recognize_batch_beam(imgs, 4, 2.0, True, 3, token_scores=True, allowed=ts)
        assert len(hyps) == 3 and all(len(h) >= 1 for h in hyps)
        for h in (x for per in hyps for x in per):
            assert set(h.text) <= set(chars), h.text
            assert len(h.token_logp) == len(h.ids) >= 2 and h.token_logp[0] == 0 and np.array_equal(h.token_logp[1:], h.logprobs)
            assert h.confidence == pytest.approx(float(np.exp(h.token_logp[1:].astype(np.float64).mean())), rel=1e-12)
            mine = tu.sequential_score(h.token_logp, len(h.ids), 2.0)
            assert mine == pytest.approx(h.sequence_score, rel=1e-6)
        one = m.recognize_beam(imgs[0], 4, 2.0, True, 3, token_scores=True, allowed=ts)
        assert [h.ids.tolist() for h in one] == [h.ids.tolist() for h in hyps[0]]
        plain = m.recognize_batch_beam(imgs, 4, 2.0, True, 3)
        assert all(len(h.logprobs) == 0 and h.confidence == 0.0 for per in plain for h in per)
    finally:
        m.close()
