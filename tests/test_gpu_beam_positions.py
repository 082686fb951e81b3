"""-m gpu: token positions of beam-search hypotheses through the engine (include/mocr.h, "beam search with token positions").
6 crops x K = 4 at max_len 24 on the position tests' weights and crops, max_batch 24, the published configuration.

* fp32: the five fields of every hypothesis against position_util.reference_for_ids teacher-forced on the engine's own
  hypothesis ids, within FP32_TOL of the greedy positions test (the computation is that test's, the route is not).
* bf16, classic and latent: cx / cy within BF16_CXY_TOL of the same float64 reference; and against the same engine's greedy
  positions of the same ids as forced prefixes over shared sources, within 2 x BF16_CXY_TOL (each side is within one).
  tests/test_beam_positions_cpu.py shows these inputs put a dropped trail more than 10 x BF16_CXY_TOL away.
* Identity: ids, lengths, scores and token scores do not move with positions; plain beam and greedy positions calls are what
  they were before a beam-positions batch.
* Compaction (160 rows on a bf16 latent engine, early-EOS weights), the lazily allocated trails, the graph count, a sliver
  region, the device twin, MangaOcr(num_beams=4).recognize_positions."""
import functools

import numpy as np
import pytest

import beam_position_util as bp
import position_util as pu
from gpu_util import crops, report
from manga_ocr.engine import BeamConfig
from manga_ocr.weights import DEFAULT_SPEC
from test_gpu_positions import BF16_CXY_TOL, FP32_TOL, _enc, _gray

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")      # before the engine's library: one HIP runtime per process, torch's

ML, K, N = bp.MAX_LEN, 4, 6
PUBLISHED = BeamConfig(*bp.PUBLISHED)
EARLY_EOS = 1.7                          # tests/test_gpu_beam.py: the crops end at different steps (hypotheses of 2 .. 13 tokens here)
LATENT, NO_COMPACTION = 64, 2048
PAD = DEFAULT_SPEC.pad_id
assert (bp.G, bp.EOS_BIAS, bp.WEIGHT_SEED, bp.CROP_SEED) == (pu.G, pu.EOS_BIAS, pu.WEIGHT_SEED, pu.CROP_SEED), "test_gpu_positions' crops and encodings"


@functools.lru_cache(maxsize=None)
def _engine(dtype, eos_bias=bp.EOS_BIAS, max_batch=24, flags=0, lanes=1):
    from manga_ocr.engine import Engine
    return Engine(pu.pos_weights(bp.G, eos_bias, bp.WEIGHT_SEED), DEFAULT_SPEC, dtype=dtype, device=0, max_batch=max_batch, flags=flags, lanes=lanes)


@functools.lru_cache(maxsize=None)
def _oracle(eos_bias=bp.EOS_BIAS):
    from oracle.mocr_oracle import Oracle
    return Oracle(pu.pos_weights(bp.G, eos_bias, bp.WEIGHT_SEED), DEFAULT_SPEC)


def check_block(name, ids, lens, pos):
    """what every positions block must satisfy beside its hypotheses"""
    n = ids.shape[0]
    assert pos.dtype == np.float32 and pos.shape == ids.shape + (5,) and np.isfinite(pos).all(), name
    for c in range(n):
        for j in range(ids.shape[1]):
            L = int(lens[c, j])
            assert (pos[c, j, 0] == 0).all() and (pos[c, j, L:] == 0).all(), f"{name}: crop {c} hypothesis {j}: zeros at the start token and behind the length"
            if L > 1:
                assert (pos[c, j, 1:L, 4] > 0).all(), f"{name}: crop {c} hypothesis {j}: every token, EOS included, has patch mass"


def field_errors(name, eos_bias, ids, lens, pos, enc, bound):
    """max |engine - float64| per field over all tokens of all hypotheses, the reference teacher-forced on the engine's ids"""
    check_block(name, ids, lens, pos)
    ref = bp.reference_fields(_oracle(eos_bias), enc, ids[:, :, :ML], lens)
    err, cnt = np.zeros(5), 0
    for c in range(ids.shape[0]):
        for j in range(ids.shape[1]):
            L = int(lens[c, j])
            if L > 1:
                err = np.maximum(err, np.abs(pos[c, j, 1:L].astype(np.float64) - ref[c, j, 1:L]).max(axis=0))
                cnt += L - 1
    live = lens[lens > 0]
    report(f"beam positions {name}: {ids.shape[0]} crops x {ids.shape[1]}, {cnt} tokens, lengths {int(live.min())}..{int(live.max())}: max err cx {err[0]:.2e} "
           f"cy {err[1]:.2e} sx {err[2]:.2e} sy {err[3]:.2e} mass {err[4]:.2e} against the teacher-forced float64 reference (bound {bound:.2e})")
    return err


@pytest.mark.parametrize("eos_bias", [bp.EOS_BIAS, EARLY_EOS], ids=["long hypotheses", "early EOS"])
def test_fp32_engine_positions_of_every_hypothesis(eos_bias):
    """Measured on the MI355X, the worst of the five fields: 2.07e-6 over 552 tokens (24 hypotheses of 24 tokens), 2.44e-6 over
    116 tokens (hypotheses of 2 .. 13 tokens that end on EOS); the bound is FP32_TOL of tests/test_gpu_positions.py, 1.5e-5."""
    eng = _engine("fp32", eos_bias)
    ids, lens, scores, pos = eng.recognize_gray(_gray(N), max_len=ML, beam=PUBLISHED, beam_positions=True)
    assert (lens[:, 0] >= 2).all() and (ids[:, :, ML:] == PAD).all()
    if eos_bias == EARLY_EOS:
        assert len(set(lens[lens > 0].tolist())) >= 3 and (ids[np.arange(N), 0, lens[:, 0] - 1] == DEFAULT_SPEC.eos_id).any()
    err = field_errors(f"fp32 eos_bias {eos_bias}", eos_bias, ids, lens, pos, _enc(N), FP32_TOL)
    assert err.max() <= FP32_TOL


@pytest.mark.parametrize("name,flags", [("classic", 0), ("latent", LATENT)])
def test_bf16_positions_against_float64_and_the_greedy_route(name, flags):
    """Measured on the MI355X: cx / cy within 7.17e-3 (classic) and 7.71e-3 (latent) of float64, bound BF16_CXY_TOL = 2.2e-2;
    against the greedy route 1.76e-3 (classic: the greedy side takes the small-batch path) and 0 (latent: the same kernels on
    the same numbers), bound twice that."""
    eng = _engine("bf16", flags=flags)
    gray = _gray(N)
    ids, lens, scores, pos = eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED, beam_positions=True)
    err = field_errors(f"bf16 {name}", bp.EOS_BIAS, ids, lens, pos, _enc(N), BF16_CXY_TOL)
    # the same ids as forced prefixes over shared sources, through the greedy positions path of the same engine
    prefixes = [ids[c, j, 1:lens[c, j]].tolist() or None for c in range(N) for j in range(K)]
    fids, flens, fpos = eng.recognize_gray(gray, max_len=ML, positions=True, prefixes=prefixes, sources=[c for c in range(N) for _ in range(K)])
    worst, cnt = 0.0, 0
    for r, (c, j) in enumerate((c, j) for c in range(N) for j in range(K)):
        L = int(lens[c, j])
        if L < 2:
            continue
        assert flens[r] >= L and np.array_equal(fids[r, :L], ids[c, j, :L])
        cnt += 1
        worst = max(worst, float(np.abs(fpos[r, 1:L, :2].astype(np.float64) - pos[c, j, 1:L, :2]).max()))
    report(f"beam positions bf16 {name} vs the engine's greedy positions of the same ids as prefixes, {cnt} hypotheses: cx / cy within {worst:.3e} "
           f"(bound {2 * BF16_CXY_TOL:.1e})")
    assert max(err[0], err[1]) <= BF16_CXY_TOL
    assert cnt >= N and worst <= 2 * BF16_CXY_TOL


@pytest.mark.parametrize("dtype,flags", [("fp32", 0), ("bf16", LATENT)])
def test_positions_move_nothing_else(dtype, flags):
    eng = _engine(dtype, EARLY_EOS, flags=flags)
    gray = _gray(N)
    greedy0 = eng.recognize_gray(gray, ML, scores=True, positions=True)
    plain0 = eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED)
    tok0 = eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED, beam_scores=True)
    with_pos = eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED, beam_positions=True)
    both = eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED, beam_scores=True, beam_positions=True)
    assert len(with_pos) == 4 and len(both) == 5
    for blk, p, a, b in zip(("ids", "lens", "scores"), plain0, with_pos, both):
        np.testing.assert_array_equal(a.view(np.int32), p.view(np.int32), err_msg=f"{blk} move with positions")
        np.testing.assert_array_equal(b.view(np.int32), p.view(np.int32), err_msg=f"{blk} move with positions and token scores")
    np.testing.assert_array_equal(both[3].view(np.int32), tok0[3].view(np.int32), err_msg="token scores move with positions")
    np.testing.assert_array_equal(both[4], with_pos[3], err_msg="positions depend on the token form")
    check_block(dtype, with_pos[0], with_pos[1], with_pos[3])
    # behind the beam-positions batches: the earlier calls again
    for a, b in zip(eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED), plain0):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(eng.recognize_gray(gray, ML, scores=True, positions=True), greedy0):
        np.testing.assert_array_equal(a, b)
    # the same crops at other batch positions: the same positions
    moved = eng.recognize_gray(np.roll(gray, 1, axis=0), max_len=ML, beam=PUBLISHED, beam_positions=True)
    np.testing.assert_array_equal(moved[3], np.roll(with_pos[3], 1, axis=0))


def test_positions_survive_compaction():
    """40 crops x 4 = 160 rows in one batch of a bf16 latent engine on early-EOS weights: crops end at different steps, the
    batch is compacted, and the rows the steps recorded are found through rowmap all the same.  Measured on the MI355X: one
    compaction, 668 tokens, cx / cy within 8.78e-3 of float64 (bound 2.2e-2), identical to the uncompacted engine's."""
    n = 40
    eng = _engine("bf16", EARLY_EOS, max_batch=160, flags=LATENT, lanes=2)
    gray = _gray(n)
    base = eng.compaction_count()
    ids, lens, scores, pos = eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED, beam_positions=True)
    n_comp = eng.compaction_count() - base
    err = field_errors(f"bf16 latent, 160 rows, {n_comp} compactions", EARLY_EOS, ids, lens, pos, _enc(40), BF16_CXY_TOL)
    assert n_comp > 0, "the batch compacts"
    assert max(err[0], err[1]) <= BF16_CXY_TOL
    other = _engine("bf16", EARLY_EOS, max_batch=160, flags=LATENT | NO_COMPACTION, lanes=2)
    for a, b, blk in zip(other.recognize_gray(gray, max_len=ML, beam=PUBLISHED, beam_positions=True), (ids, lens, scores, pos), ("ids", "lens", "scores", "pos")):
        np.testing.assert_array_equal(a, b, err_msg=f"{blk} differ without compaction")
    assert other.compaction_count() == 0
    with pytest.raises(Exception, match="max_batch"):
        eng.recognize_gray(np.tile(gray, (2, 1, 1)), max_len=ML, beam=PUBLISHED, beam_positions=True)      # 80 x 4 rows: one request fits one batch


def test_the_trails_are_allocated_by_the_first_batch_that_asks():
    eng = _engine("bf16", EARLY_EOS, flags=LATENT | NO_COMPACTION)
    gray = _gray(N)
    eng.recognize_gray(gray, ML, positions=True)
    eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED)
    eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED, beam_scores=True)
    assert eng.beam_position_state_bytes() == 0, "greedy, plain beam and beam-token batches allocate no trail"
    plain_bytes, token_bytes = eng.beam_state_bytes(), eng.beam_token_state_bytes()
    assert plain_bytes > 0 and token_bytes > 0
    eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED, beam_positions=True)
    one = eng.beam_position_state_bytes()
    assert one > 0 and one % (2 * DEFAULT_SPEC.max_len) == 0
    # alternating batches: the graphs of each kind are captured once
    g0 = eng.graph_count()
    for _ in range(3):
        eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED)
        eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED, beam_positions=True)
        eng.recognize_gray(gray, ML, positions=True)
    g1 = eng.graph_count()
    for _ in range(3):
        eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED, beam_positions=True)
        eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED)
    assert eng.graph_count() == g1 and g1 - g0 <= 12, (g0, g1)
    assert eng.beam_position_state_bytes() in (one, 2 * one), "at most once per lane"
    assert eng.beam_state_bytes() in (plain_bytes, 2 * plain_bytes) and eng.beam_token_state_bytes() in (token_bytes, 2 * token_bytes)
    assert eng.beam_state_bytes() % (5 + DEFAULT_SPEC.max_len) == 0 and eng.beam_token_state_bytes() % (8 * DEFAULT_SPEC.max_len) == 0


def test_a_sliver_region_reads_zeros():
    from manga_ocr.regions import padded_rect
    eng = _engine("bf16", EARLY_EOS, flags=LATENT)
    page = np.random.RandomState(5).randint(0, 256, size=(300, 400, 3), dtype=np.uint8)
    regs = [(0, 20, 30, 100, 60), (0, 403, 10, 50, 50), (0, 10, 10, 0, 0), (0, 396, 0, 50, 40), (0, 100, 303, 40, 40)]
    eng.set_generate_max_length(ML)
    try:
        ids, lens, scores, pos = eng.recognize_regions([page], regs, beam=PUBLISHED, beam_positions=True)
    finally:
        eng.set_generate_max_length(DEFAULT_SPEC.max_len)
    rects = [padded_rect(r[1:], 300, 400) for r in regs]
    assert [r is None for r in rects] == [False, True, True, False, True]
    check_block("regions", ids, lens, pos)
    for i, r in enumerate(rects):
        if r is None:
            assert (lens[i] == 0).all() and (pos[i] == 0).all() and (scores[i] == np.float32(-1e9)).all()
        else:
            assert lens[i, 0] >= 2 and np.abs(pos[i, 0, 1:lens[i, 0]]).max() > 0


def test_the_device_twin_equals_the_host_call():
    n = 5
    gray = _gray(n)
    eng = _engine("bf16", EARLY_EOS, flags=LATENT)
    want = eng.recognize_gray(gray, max_len=ML, beam=PUBLISHED, beam_scores=True, beam_positions=True)
    L = DEFAULT_SPEC.max_len
    d_gray = torch.from_numpy(gray).cuda()
    d_ids = torch.full((n, K, L), -5, dtype=torch.int32, device="cuda")
    d_len = torch.full((n, K), -5, dtype=torch.int32, device="cuda")
    d_score = torch.full((n, K), 5.0, dtype=torch.float32, device="cuda")
    d_logp = torch.full((n, K, L), 5.0, dtype=torch.float32, device="cuda")
    d_pos = torch.full((n, K, L, 5), 5.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.set_generate_max_length(ML)
    try:
        eng.recognize_device(d_gray, n, d_ids, d_len, beam=PUBLISHED, d_out_score=d_score, d_out_beam_logp=d_logp, d_out_beam_pos=d_pos)
        eng.synchronize()
        for got, w, blk in zip((d_ids, d_len, d_score, d_logp, d_pos), want, ("ids", "lens", "scores", "logp", "pos")):
            np.testing.assert_array_equal(got.cpu().numpy(), w, err_msg=f"device twin: {blk}")
        d_pos.fill_(5.0)
        torch.cuda.synchronize()
        eng.recognize_device(d_gray, n, d_ids, d_len, beam=PUBLISHED, d_out_score=d_score, d_out_beam_pos=d_pos)       # without the token scores
        eng.synchronize()
        np.testing.assert_array_equal(d_pos.cpu().numpy(), want[4])
    finally:
        eng.set_generate_max_length(L)


def test_manga_ocr_positions_methods_return_the_best_hypothesis(tmp_path):
    from dataclasses import replace
    from PIL import Image
    from hf_dir import write_hf_dir
    from manga_ocr import MangaOcr
    d = str(tmp_path / "manga-ocr-base")
    write_hf_dir(d, seed=1, spec=replace(DEFAULT_SPEC, max_len=16), eos_bias=EARLY_EOS)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = MangaOcr(d, dtype="fp32", max_batch=8, lanes=1, num_beams=4)
    try:
        assert m.beam == PUBLISHED and m.beam_positions is True
        grays = crops(55, 3)
        imgs = [Image.fromarray(g, mode="L") for g in grays]
        rec = m.recognize_positions(imgs[0])
        assert rec.text == m(imgs[0]) and len(rec.ids) >= 2, "the text __call__ returns"
        assert rec.positions.shape == (len(rec.ids), 5) and (rec.positions[0] == 0).all() and (rec.positions[1:, 4] > 0).all()
        assert len(rec.logprobs) == len(rec.ids) - 1 and rec.sequence_score is not None
        boxes = rec.boxes(224, 224)
        assert boxes.shape == (len(rec.ids), 4) and (boxes[0] == 0).all() and (boxes[1:, 2] > boxes[1:, 0]).all() and (boxes[1:, 3] > boxes[1:, 1]).all()
        best = m.recognize_beam(imgs[0], 4, 2.0, True, 3, token_scores=True, positions=True)[0]
        np.testing.assert_array_equal(best.ids, rec.ids)
        np.testing.assert_array_equal(best.positions, rec.positions)
        batch = m.recognize_batch_positions(imgs)
        assert [r.text for r in batch] == m.recognize_batch(imgs) and batch[0].ids.tolist() == rec.ids.tolist()
        assert all(r.positions.shape == (len(r.ids), 5) for r in batch)
        hyps = m.recognize_batch_beam(imgs, 4, 2.0, True, 3, positions=True)
        assert all(h.positions.shape == (len(h.ids), 5) and len(h.logprobs) == 0 for per in hyps for h in per)
        page = np.repeat(np.pad(grays[0], ((10, 10), (10, 10)))[:, :, None], 3, axis=2)
        regs = m.recognize_regions_positions([page], [(0, 10, 10, 224, 224), (0, 0, 0, 0, 0)])
        assert regs[0].rect is not None and regs[0].page_boxes().shape == (len(regs[0].ids), 4)
        assert regs[1].text == "" and regs[1].rect is None and regs[1].positions.shape == (0, 5)
        with pytest.raises(ValueError, match="do not combine"):
            m.recognize_positions(imgs[0], no_repeat_ngram=2)
        with pytest.raises(ValueError, match="do not combine"):
            m.recognize_batch_positions(imgs, prefix=[5])
    finally:
        m.close()
