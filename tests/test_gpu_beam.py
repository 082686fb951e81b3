"""-m gpu: beam search through the engine.

* fp32 engine against transformers' own beam search (tests/golden/beam_*.npz, configs (a)-(d), 6 crops each, and (la)-(lc), one crop with searches of 16 .. 19 steps): all K id rows and
  lengths identical, scores within 1e-3 - for every crop, since every crop's min_gap is >= 1e-3 (tests/test_beam_cpu.py) and
  the fp32 logits are within 2.4e-6 of the reference's.  Config (a) also through a model directory and ``MangaOcr(...,
  num_beams="checkpoint")``.
* Engine invariants in bf16, one test per kernel regime: graph / no graph and compaction / no compaction give the same
  outputs, the same crop at two batch positions the same hypotheses, a repeated call no new graph, no hypothesis a repeated
  3-gram, scores in non-increasing order.
* bf16 against the reference: the engine's teacher-forced log-probability of every golden hypothesis against the golden's
  own score.
* No regression of greedy: calls interleaved with beam calls return what an engine that never saw a beam request returns."""
import os

import numpy as np
import pytest

import beam_util as bu
from gpu_util import crops, engine, report
from manga_ocr.engine import BeamConfig
from manga_ocr.weights import DEFAULT_SPEC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")      # before the engine's library: one HIP runtime per process, torch's

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ES = {0: False, 1: True, 2: "never"}
NO_GRAPH, NO_COMPACTION, FP8, LATENT_ALWAYS = 2, 2048, 128, 64
PAD = DEFAULT_SPEC.pad_id
# bf16: the largest |engine - golden| of a hypothesis' length-normalised score measured on the MI355X;
# the bound is twice that, the allowance the project uses for BF16_GAP_TOL
BF16_SCORE_DIFF_MEASURED = 1.466e-3
BF16_SCORE_TOL = 2 * BF16_SCORE_DIFF_MEASURED
PUBLISHED = BeamConfig(4, 2.0, True, 3)
INV_EOS_BIAS = 1.7                       # the invariants' early-EOS weights: config (a) ends crops at different steps below 16 tokens


def golden(name):
    g = np.load(os.path.join(GOLD, f"beam_{name}.npz"))
    return {k: g[k] for k in g.files}


def golden_crops(g):
    return np.stack([np.random.RandomState(int(s)).randint(0, 256, size=(224, 224), dtype=np.uint8) for s in g["crop_seeds"]])


def golden_config(g):
    return BeamConfig(int(g["num_beams"]), float(g["length_penalty"]), ES[int(g["early_stopping"])], int(g["no_repeat_ngram_size"]))


def check_block(ids, lens, scores, ML):
    """what every beam result must satisfy: pad behind a length, empty slots (0, -1e9), scores in non-increasing order"""
    n, K, _ = ids.shape
    for c in range(n):
        for j in range(K):
            assert (ids[c, j, lens[c, j]:] == PAD).all()
            assert (lens[c, j] == 0) == (scores[c, j] == np.float32(-1e9))
            assert lens[c, j] <= ML
        assert (np.diff(scores[c]) <= 0).all(), f"crop {c}: hypotheses out of score order {scores[c]}"


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "la", "lb", "lc"])
def test_fp32_engine_returns_the_transformers_hypotheses(name):
    """THE test that fails without the feature."""
    g = golden(name)
    ML, K = int(g["max_length"]), int(g["num_beams"])
    eng = engine("fp32", seed=int(g["weights_seed"]), eos_bias=float(g["eos_bias"]), max_batch=24)
    ids, lens, scores = eng.recognize_gray(golden_crops(g), max_len=ML, beam=golden_config(g))
    check_block(ids, lens, scores, ML)
    np.testing.assert_array_equal(lens, g["lens"])
    np.testing.assert_array_equal(ids[:, :, :ML], g["ids"])
    assert (ids[:, :, ML:] == PAD).all()
    err = float(np.abs(scores.astype(np.float64) - g["scores"]).max())
    report(f"beam fp32 config ({name}): {ids.shape[0]} crops x {K} hypotheses identical to transformers, scores within {err:.2e}")
    assert err <= 1e-3


def test_checkpoint_settings_through_a_model_directory(tmp_path):
    from dataclasses import replace
    from PIL import Image
    from hf_dir import write_hf_dir
    from manga_ocr import MangaOcr
    from manga_ocr.text import ids_to_text
    g = golden("a")
    ML = int(g["max_length"])
    d = str(tmp_path / "manga-ocr-base")
    write_hf_dir(d, seed=int(g["weights_seed"]), spec=replace(DEFAULT_SPEC, max_len=ML), eos_bias=float(g["eos_bias"]))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)      # every setting the loader would call ignored is honoured: it has nothing to warn about
        m = MangaOcr(d, dtype="fp32", num_beams="checkpoint", max_batch=8, lanes=1)
    try:
        assert m.beam == PUBLISHED
        assert not {"num_beams", "length_penalty", "early_stopping", "no_repeat_ngram_size"} & set(m.ignored_generation_config)
        gray = golden_crops(g)
        for c in (0, 3):
            want = ids_to_text(m.vocab, g["ids"][c, 0, :g["lens"][c, 0]])
            assert m(Image.fromarray(gray[c], mode="L")) == want
        hyps = m.recognize_beam(Image.fromarray(gray[1], mode="L"), 4, 2.0, True, 3)
        assert [h.ids.tolist() for h in hyps] == [g["ids"][1, j, :g["lens"][1, j]].tolist() for j in range(4)]
        assert np.abs(np.array([h.sequence_score for h in hyps]) - g["scores"][1]).max() <= 1e-3
        assert m.recognize_batch([Image.fromarray(gray[c], mode="L") for c in (2, 4)]) == \
            [ids_to_text(m.vocab, g["ids"][c, 0, :g["lens"][c, 0]]) for c in (2, 4)]
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ invariants, per regime
def _no_repeated_3gram(ids, lens):
    for c in range(ids.shape[0]):
        for j in range(ids.shape[1]):
            assert not bu.has_repeat(ids[c, j, :lens[c, j]], 3), f"crop {c} hypothesis {j} repeats a 3-gram"


@pytest.mark.parametrize("name,n_crops,flags,auto", [
    ("generic, 8 rows", 2, 0, True),
    ("classic, 96 rows", 24, 0, True),
    ("latent, 400 rows", 100, LATENT_ALWAYS, False),
    ("fp8 attention, 400 rows", 100, LATENT_ALWAYS | FP8, False),
])
def test_bf16_engine_invariants(name, n_crops, flags, auto):
    ML, K = 16, 4
    rows = n_crops * K
    gray = crops(4321, n_crops)
    kw = dict(seed=1, eos_bias=INV_EOS_BIAS, max_batch=max(rows, 8), auto_path=auto)
    eng = engine("bf16", flags=flags, **kw)
    comp0 = eng.compaction_count()
    ids, lens, scores = eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED)
    n_comp = eng.compaction_count() - comp0
    check_block(ids, lens, scores, ML)
    _no_repeated_3gram(ids, lens)
    assert (lens[:, 0] >= 2).all(), "every crop has a best hypothesis"
    if n_comp:
        # the invariant both kernels rely on: behind a compaction the K rows of a crop still sit in K neighbouring slots, in beam
        # order, from a slot that is a multiple of K (the padding rows are the last slots, so the first `rows` slots hold the rows)
        rm = eng.lane_rowmap(rows).reshape(n_crops, K)
        assert sorted(rm.ravel().tolist()) == list(range(rows))
        assert (rm[:, 0] % K == 0).all() and (rm == rm[:, :1] + np.arange(K)).all(), rm
    graphs = eng.graph_count()
    again = eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED)
    assert eng.graph_count() == graphs, "repeating the call adds no graph"
    for a, b in zip(again, (ids, lens, scores)):
        np.testing.assert_array_equal(a, b)
    # the same crops at other batch positions (every crop moves by one): the same K hypotheses
    moved = eng.recognize_gray(np.roll(gray, 1, axis=0), max_len=ML, beam=PUBLISHED)
    for a, b, blk in zip(moved, (ids, lens, scores), ("ids", "lens", "scores")):
        np.testing.assert_array_equal(a, np.roll(b, 1, axis=0), err_msg=f"{name}: {blk} depend on the batch position")
    assert eng.graph_count() == graphs
    for what, f in (("no graph", NO_GRAPH), ("no compaction", NO_COMPACTION)):
        other = engine("bf16", flags=flags | f, **kw)
        for a, b, blk in zip(other.recognize_gray(gray, max_len=ML, beam=PUBLISHED), (ids, lens, scores), ("ids", "lens", "scores")):
            np.testing.assert_array_equal(a, b, err_msg=f"{name}: {blk} differ with {what}")
        if f == NO_COMPACTION:
            assert other.compaction_count() == 0
    report(f"beam bf16 {name}: {n_crops} crops x {K}, best lengths {int(lens[:, 0].min())}..{int(lens[:, 0].max())}, {n_comp} compactions; "
           "identical with / without graphs and compaction")
    if rows > 32:
        assert n_comp > 0, "the compacting run compacts"


@pytest.mark.parametrize("name,dtype,flags", [
    ("classic, fp32", "fp32", 0),
    ("latent, bf16", "bf16", LATENT_ALWAYS),
    ("fp8 attention, bf16", "bf16", LATENT_ALWAYS | FP8),
])
def test_long_searches_replay_graphs_as_they_run_eagerly(name, dtype, flags):
    """Searches of 104 tokens on weights that never emit EOS: the captured decode graphs cover their context buckets to the
    last position (the buckets end behind steps 95, 159, 255 - the cache reorder of exactly those steps has to move one
    position more than the steps before it), so the outputs equal those of the eager steps, which pass every launch its own
    step."""
    ML, K, n_crops = 104, 4, 3
    gray = crops(808, n_crops)
    cfg = BeamConfig(K, 1.0, False, 3)
    kw = dict(seed=0, max_batch=n_crops * K)
    got = engine(dtype, flags=flags, **kw).recognize_gray(gray, max_len=ML, beam=cfg)
    want = engine(dtype, flags=flags | NO_GRAPH, **kw).recognize_gray(gray, max_len=ML, beam=cfg)
    ids, lens, scores = got
    check_block(ids, lens, scores, ML)
    _no_repeated_3gram(ids, lens)
    assert (lens == ML).all(), "nothing ends early: every hypothesis ends on the length rule, behind the bucket boundary at 96"
    for a, b, blk in zip(got, want, ("ids", "lens", "scores")):
        np.testing.assert_array_equal(a, b, err_msg=f"{name}: {blk} of the graph replay differ from the eager steps")
    report(f"beam {name}: {n_crops} crops x {K}, {ML} tokens each, graph replay identical to eager steps")


def test_beam_state_is_allocated_by_the_first_beam_batch():
    """creating an engine and greedy calls of every kind allocate no beam state; the first beam batch of a lane does, once"""
    ML = 10
    gray = crops(31, 4)
    eng = engine("bf16", seed=1, eos_bias=1.1, max_batch=16, auto_path=True, lanes=2, flags=NO_COMPACTION)
    assert eng.beam_state_bytes() == 0
    eng.recognize_gray(gray, max_len=ML)
    eng.recognize_gray(gray, max_len=ML, scores=True, no_repeat_ngram=2)
    eng.recognize_gray(gray[:2], max_len=ML, scores=True, sources=[0, 0, 1], prefixes=[[10], None, [12]])
    assert eng.beam_state_bytes() == 0
    eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED)
    one = eng.beam_state_bytes()
    assert one > 0 and one % (5 + DEFAULT_SPEC.max_len) == 0
    eng.recognize_gray(gray, max_len=ML, beam=BeamConfig(2, 1.0, False, 0))
    eng.recognize_gray(gray, max_len=ML)
    assert eng.beam_state_bytes() in (one, 2 * one), "at most once per lane"


def test_bf16_scores_against_the_reference():
    """The bf16 engine's teacher-forced log-probability of every golden hypothesis (the score_texts path: forced prefixes,
    scored) against the golden's own score, length-normalised as the golden is; then every crop whose reference margin
    (min_gap, tests/beam_util.py) is at least the bound returns the reference's hypotheses exactly."""
    from test_beam_cpu import reference
    g = golden("a")
    ML, K, lp = int(g["max_length"]), int(g["num_beams"]), float(g["length_penalty"])
    gray = golden_crops(g)
    n = gray.shape[0]
    eng = engine("bf16", seed=int(g["weights_seed"]), eos_bias=float(g["eos_bias"]), max_batch=24, auto_path=True)
    prefixes = [g["ids"][c, j, 1:g["lens"][c, j]].tolist() for c in range(n) for j in range(K)]
    _, flens, logp = eng.recognize_gray(gray, max_len=ML, scores=True, prefixes=prefixes, sources=[c for c in range(n) for _ in range(K)])
    worst = 0.0
    for r, (c, j) in enumerate((c, j) for c in range(n) for j in range(K)):
        L = int(g["lens"][c, j])
        assert flens[r] == L
        mine = float(logp[r, 1:L].astype(np.float64).sum()) / float(L - 1) ** lp
        worst = max(worst, abs(mine - float(g["scores"][c, j])))
    report(f"beam bf16 vs transformers, config (a): largest difference of the length-normalised sequence scores {worst:.3e} "
           f"(recorded {BF16_SCORE_DIFF_MEASURED:.1e}, bound {BF16_SCORE_TOL:.1e})")
    assert worst <= BF16_SCORE_TOL
    ids, lens, scores = eng.recognize_gray(gray, max_len=ML, beam=golden_config(g))
    min_gap = reference("a")[3]["min_gap"]
    skipped = 0
    for c in range(n):
        if min_gap[c] < BF16_SCORE_TOL:
            skipped += 1
            report(f"beam bf16 config (a) crop {c}: reference margin {min_gap[c]:.2e} below the bound, not compared")
            continue
        np.testing.assert_array_equal(lens[c], g["lens"][c], err_msg=f"crop {c} (margin {min_gap[c]:.2e})")
        np.testing.assert_array_equal(ids[c, :, :ML], g["ids"][c], err_msg=f"crop {c} (margin {min_gap[c]:.2e})")
    assert skipped * 2 <= n, f"{skipped} of {n} crops below the bound"


def test_greedy_calls_are_unchanged_by_beam_calls():
    """greedy / scored / shared / n-gram calls interleaved with beam calls of two configurations, on a two-lane engine,
    against the same calls on an engine that never saw a beam request"""
    ML = 12
    gray = crops(99, 6)

    def greedy_calls(e):
        out = [e.recognize_gray(gray, max_len=ML), e.recognize_gray(gray, max_len=ML, scores=True),
               e.recognize_gray(gray[:2], max_len=ML, scores=True, sources=[0, 0, 1, 1, 1], prefixes=[[10], [11], None, [12], [13]]),
               e.recognize_gray(gray[:3], max_len=ML, no_repeat_ngram=2)]
        return [a for o in out for a in o]

    want = greedy_calls(engine("bf16", seed=1, eos_bias=1.1, max_batch=24, auto_path=True, lanes=1))
    mixed = engine("bf16", seed=1, eos_bias=1.1, max_batch=24, auto_path=True, lanes=2)      # (another cache key: its own engine)
    got = greedy_calls(mixed)
    mixed.recognize_gray(gray, max_len=ML, beam=PUBLISHED)
    got2 = greedy_calls(mixed)
    mixed.recognize_gray(gray[:3], max_len=ML, beam=BeamConfig(2, 1.0, False, 0))
    got3 = greedy_calls(mixed)
    for a, b, c, w in zip(got, got2, got3, want):
        np.testing.assert_array_equal(a, w)
        np.testing.assert_array_equal(b, w)
        np.testing.assert_array_equal(c, w)
