"""-m gpu: the one-launch-per-projection decode path of small bf16 batches (<= 32 rows, csrc/kernels_smallm.h) against
the generic path (split-K projections + add/LayerNorm launches, MOCR_FLAG_NO_SMALL_BATCH_PATH) and against the oracle.

The two paths compute the same function with the same rounding points (bf16 operands, fp32 accumulation, bf16 normalised
rows and GELU output); only the order of the fp32 sums differs (no split-K slabs), so their teacher-forced logits must
agree to well within the bf16 noise each of them shows against the fp32 oracle."""
import numpy as np
import pytest

from gpu_util import crops, engine, oracle, report

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NO_SMALL = 256          # MOCR_FLAG_NO_SMALL_BATCH_PATH
CLASSIC = 8             # MOCR_FLAG_CLASSIC_ATTENTION: the attention kernels small batches use anyway


@pytest.mark.parametrize("rows", [1, 5, 16, 17, 32])
def test_small_batch_path_logits_agree_with_the_generic_path_and_the_oracle(rows):
    """One and two sixteen-row tiles, ragged last tiles included; 24 teacher-forced steps (both decoder layers, the layer-1
    LayerNorm-in-the-prologue chain and the LM head)."""
    small = engine("bf16", max_batch=64, flags=CLASSIC)
    generic = engine("bf16", max_batch=64, flags=CLASSIC | NO_SMALL)
    gray = crops(4242, 64)[:rows]
    o = oracle()
    nref = min(rows, 4)
    enc = o.encode(o.preprocess_gray(gray[:nref]))
    ids_ref, ref = o.generate(enc, return_logits=True, max_len=25)
    forced = np.tile(ids_ref[:1, :24], (rows, 1)).astype(np.int32)
    forced[:nref] = ids_ref[:, :24]
    dg = torch.from_numpy(gray).cuda()
    torch.cuda.synchronize()
    a = small.decode_logits(dg, rows, forced)
    b = generic.decode_logits(dg, rows, forced)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    d_paths = np.abs(a - b).max()
    d_a = np.abs(a[:nref] - ref[:, :24]).max()
    d_b = np.abs(b[:nref] - ref[:, :24]).max()
    report(f"small-batch path, {rows} rows x 24 steps: max |logit - generic path| {d_paths:.3e}; vs oracle: small {d_a:.3e}, generic {d_b:.3e}")
    assert d_paths <= 2e-2
    assert d_a <= 3e-2 and d_b <= 3e-2
    assert (a.argmax(-1) == b.argmax(-1)).mean() >= 0.97


def test_small_batch_rows_do_not_depend_on_the_batch():
    """A crop decodes to the same ids whatever else is in its batch, as long as the batch stays in one kernel regime.  On this
    engine (max_batch 32: a slab buffer of 128 rows' worth) the encoder splits its O-proj / FC2 GEMMs over K up to 5 crops -
    (3, 8) ways for one crop, (3, 4) for two, (3, 2) for three, (1, 2) for four and five (mocr_encoder_plan; other summation
    orders, which these ids survive) - and from 6 to 32 rows it does not: six crops are still eligible for the split (228
    blocks of 64 x 64 on 256 CUs), but their slabs do not fit this engine's buffer; from max_batch 129 they do, (3, 2)."""
    eng = engine("bf16", max_batch=32, flags=CLASSIC)
    gray = crops(4343, 32)
    full, _ = eng.recognize_gray(gray, max_len=40)
    for n in (6, 16, 19):
        ids, lens = eng.recognize_gray(gray[:n], max_len=40)
        np.testing.assert_array_equal(ids, full[:n])
        assert (lens == 40).all()
    five, _ = eng.recognize_gray(gray[:5], max_len=40)
    for n in (1, 2, 4):
        ids, _ = eng.recognize_gray(gray[:n], max_len=40)
        np.testing.assert_array_equal(ids, five[:n])


def test_small_batch_early_eos_lengths_and_padding_match_the_generic_path():
    """EOS-biased weights: rows end at different lengths; finished rows emit pad_id and the batch stops early.  The two
    paths may differ where a decision is a numerical tie (with these weights ~2 % of all decisions are closer than the bf16
    noise, so long rows usually meet one - tests/test_gpu_bf16_parity.py pins both paths against the reference with the
    margins at hand); here: the stopping / padding rules hold on both, and the short rows agree."""
    small = engine("bf16", seed=1, eos_bias=1.1, max_batch=32, flags=CLASSIC)
    generic = engine("bf16", seed=1, eos_bias=1.1, max_batch=32, flags=CLASSIC | NO_SMALL)
    gray = crops(4444, 32)
    a, la = small.recognize_gray(gray)
    b, lb = generic.recognize_gray(gray)
    same = int((a == b).all(axis=1).sum())
    report(f"small-batch path, EOS-biased weights, 32 rows: {same} rows identical to the generic path; lengths {la.min()}..{la.max()}")
    assert same >= 8
    short = la <= 40
    assert short.any() and ((a == b).all(axis=1)[short]).mean() >= 0.7
    for i in range(32):
        assert (a[i, la[i]:] == 0).all() and (b[i, lb[i]:] == 0).all()         # pad_id behind the end
        if (a[i] == b[i]).all():
            assert la[i] == lb[i]
