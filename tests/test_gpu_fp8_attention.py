"""-m gpu: the opt-in fp8 attention mode (MOCR_FLAG_FP8_ATTENTION, BASELINE configs[4]): OCP e4m3 key/value rows,
fp8 MFMA for both products of the latent decode attention, fp32 softmax.  NOT the parity configuration: these tests pin
the kernels against references that model the quantisation, and REPORT the mode's accuracy against the fp32 oracle
(teacher-forced logits, id-match rate) next to the bf16 engine's."""
import os

import numpy as np
import pytest

from gpu_util import bf16_round, crops, e4m3_quant, e4m3_table, engine, oracle, report

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FP8 = 128          # MOCR_FLAG_FP8_ATTENTION
LATENT_ALWAYS = 64


def _bf16_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda().to(torch.bfloat16)


def test_e4m3_quantiser_is_round_to_nearest_even_and_bit_exact():
    eng = engine("bf16")
    rs = np.random.RandomState(0)
    x = bf16_round(np.concatenate([rs.standard_normal(4096) * 3, rs.standard_normal(4096) * 0.01, [448.0, -448.0, 0.0, 1.0, 0.0625, 2 ** -9, 3 * 2 ** -10, 0.0]
                                   + [0.0] * 8]).astype(np.float32))
    inv = 7.25
    dx = _bf16_dev(x)
    d8 = torch.zeros(x.size, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    xin = np.clip(x.astype(np.float64) * np.float32(inv), -448, 448)
    keep = np.abs(x.astype(np.float64) * inv) <= 448
    eng.op_quant_fp8(dx, d8, x.size, inv)
    got = e4m3_table()[d8.cpu().numpy()]
    want = e4m3_quant((x.astype(np.float32) * np.float32(inv)).astype(np.float64))
    np.testing.assert_array_equal(got[keep], want[keep])
    assert np.isfinite(got[keep]).all() and xin.size == x.size


@pytest.mark.parametrize("form", ["T", "r02"])
@pytest.mark.parametrize("L,n", [(1, 5), (5, 5), (16, 5), (17, 5), (32, 5), (33, 5), (64, 5), (160, 5), (197, 5), (300, 5), (20, 300), (197, 520),
                                 (290, 300), (40, 1300), (197, 1100)])
def test_latent_attention_fp8_kernel(L, n, form):
    """The fp8 latent attention - latent_attnT8_kernel (the default: transposed score tile, two blocks per CU) and r02's
    latent_attn_fp8_kernel (MOCR_FLAG_LATENT_TILE32) - against float64 attention on the SAME quantised operands (e4m3 keys,
    per-head e4m3 query; exact probabilities): what is left is the e4m3 rounding of the probabilities (<= 6.25 % each,
    averaging out over the keys) and the bf16 output.  Also reported: the error against the unquantised attention.
    n > 512: persistent blocks take several sequences each."""
    eng = engine("bf16", flags=1024 if form == "r02" else 0)
    rs = np.random.RandomState(L + n)
    H, D = 12, 768
    stride = (L + 7) * D
    qt = np.zeros((n, 16, D), np.float32)
    qt[:, :H] = bf16_round((rs.standard_normal((n, H, D)) * 0.08).astype(np.float32))
    x = bf16_round(rs.standard_normal((n * (L + 7) + 64, D)).astype(np.float32))
    sx = 6.5 / 448.0                                         # |x| < 6.5 for 1e6 standard normals
    assert np.abs(x).max() < 6.5
    dx = _bf16_dev(x)
    d8 = torch.zeros(x.size, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.op_quant_fp8(dx, d8, x.size, 1.0 / sx)
    xq = (e4m3_table()[d8.cpu().numpy()] * np.float64(np.float32(sx))).reshape(x.shape)
    xs = np.stack([xq[b * (L + 7): b * (L + 7) + L] for b in range(n)])                 # dequantised keys [n,L,D]
    xe = np.stack([x[b * (L + 7): b * (L + 7) + L] for b in range(n)]).astype(np.float64)
    q = qt[:, :H].astype(np.float64)
    qs = np.maximum(np.abs(q).max(-1, keepdims=True), 1e-30) / 448.0
    qq = e4m3_quant(q / qs) * qs                                                          # per-head e4m3 query

    def attn(qm, km):
        sc = np.einsum("bhd,bkd->bhk", qm, km)
        sc -= sc.max(-1, keepdims=True)
        pr = np.exp(sc)
        pr /= pr.sum(-1, keepdims=True)
        return np.einsum("bhk,bkd->bhd", pr, km)

    ref_q, ref_e = attn(qq, xs), attn(q, xe)
    dq = _bf16_dev(qt)
    do = torch.full((n, 16, D), float("nan"), device="cuda", dtype=torch.bfloat16)
    torch.cuda.synchronize()
    eng.op_latent_attention_fp8(dq, d8, do, n, L, stride, sx)
    got = do[:, :H].float().cpu().numpy().astype(np.float64)
    scale = np.abs(ref_e).max()
    err_q, err_e = np.abs(got - ref_q).max(), np.abs(got - ref_e).max()
    report(f"latent attention fp8 ({form}) L={L} n={n}: max abs err vs quantisation-aware reference {err_q:.3e}, vs exact attention {err_e:.3e} "
           f"(|ref| max {scale:.2f})")
    assert np.isfinite(got).all()
    # vs the exact attention the bound is the e4m3 rounding of the keys themselves: half a unit in the 3-bit mantissa
    # = up to 6.25 % of an element (a sharp softmax copies single key rows, so nothing averages out)
    assert err_q <= 0.04 * scale + 2e-2 and err_e <= 0.0625 * np.abs(xe).max() + 0.04 * scale + 2e-2


FP8_LOGIT_TOL = 6e-2      # teacher-forced |logit - oracle| (measured 3.2e-2; the bf16 engine: 1.3e-2 under a 3e-2 bound)
FP8_GAP_TOL = 2.5e-2      # a free-running row may leave the reference only where the reference's own top-2 margin is below this


def test_fp8_attention_engine_against_the_reference(golden_dir):
    """The whole engine with fp8 attention against the fp32 oracle and the transformers goldens, next to the bf16 engine:
    teacher-forced logits over 47 steps (max error, argmax agreement, disagreements only at small reference margins) and
    free-running ids of the first 64 golden rows held to the SAME first-divergence rule as the bf16 engine."""
    g = np.load(os.path.join(golden_dir, "bf16_parity.npz"))
    gray = crops(777, 256)[:64]
    forced = g["ids_seed0"][:64, :47].astype(np.int32)
    o = oracle()
    enc = o.encode(o.preprocess_gray(gray[:8]))
    _, ref = o.generate(enc, return_logits=True, forced_ids=g["ids_seed0"][:8, :48].astype(np.int64))
    ref = ref[:, :47]
    srt = np.sort(ref, axis=-1)
    margin = srt[..., -1] - srt[..., -2]
    dg = torch.from_numpy(gray).cuda()
    torch.cuda.synchronize()
    for name, flags, ltol, gtol in (("bf16 latent", LATENT_ALWAYS, 3e-2, FP8_GAP_TOL), ("fp8 attention", LATENT_ALWAYS | FP8, FP8_LOGIT_TOL, FP8_GAP_TOL)):
        eng = engine("bf16", max_batch=64, flags=flags)
        lg = eng.decode_logits(dg, 64, forced)[:8]
        d = np.abs(lg - ref)
        agree = lg.argmax(-1) == ref.argmax(-1)
        ids, lens = eng.recognize(gray)
        want = g["ids_seed0"][:64].astype(np.int32)
        first = [int(np.nonzero(ids[b] != want[b])[0][0]) if (ids[b] != want[b]).any() else 300 for b in range(64)]
        gaps = [float(g["gaps_seed0"][b, t - 1]) for b, t in enumerate(first) if t < 300]
        report(f"[{name}] teacher-forced logits vs oracle: max abs err {d.max():.3e}, mean {d.mean():.3e}, argmax agreement {agree.mean():.4f}, "
               f"disagreements at reference margins < {margin[~agree].max() if (~agree).any() else 0:.3e}; free-running 64 rows x 300: first "
               f"divergence at token {np.mean(first):.0f} on average, reference margin there max {max(gaps) if gaps else 0:.3e}, median "
               f"{np.median(gaps) if gaps else 0:.3e}")
        assert np.isfinite(lg).all() and (lens == 300).all()
        assert d.max() <= ltol, f"{name}: teacher-forced logits {d.max():.3e} from the oracle"
        assert agree.mean() >= 0.97, f"{name}: argmax agreement {agree.mean():.4f}"
        assert (margin[~agree] < ltol).all(), f"{name}: argmax differs where the reference's margin exceeds the logit tolerance"
        assert not gaps or max(gaps) < gtol, f"{name}: a row leaves the reference at a margin of {max(gaps):.3e}"


def test_config4_variable_resolution_crops_through_the_fp8_engine():
    """BASELINE configs[4], both halves together: variable-resolution RGB crops (h, w = round(exp(U(ln 32, ln 512))),
    SURVEY.md 8(d)) from host memory -> luminance + Pillow-exact resize on the device -> bf16 encoder -> fp8-attention
    greedy decode, against the CPU oracle fed the same crops through its Pillow restatement (oracle/pil_ops.py): every
    row identical to the oracle up to its first divergence, which must sit at an oracle margin below FP8_GAP_TOL."""
    from oracle import pil_ops
    rs = np.random.RandomState(4321)
    n, L = 24, 40
    hw = np.rint(np.exp(rs.uniform(np.log(32), np.log(512), size=(n, 2)))).astype(int)
    imgs = [rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in hw]
    eng = engine("bf16", max_batch=64, flags=LATENT_ALWAYS | FP8)
    ids, lens = eng.recognize_images(imgs)
    planes = np.stack([pil_ops.preprocess_rgb_to_gray224(im) for im in imgs])
    np.testing.assert_array_equal(eng.preprocess(imgs), planes)           # the planes the encoder saw
    o = oracle()
    want, logits = o.generate(o.encode(o.preprocess_gray(planes)), max_len=L, return_logits=True)
    srt = np.sort(logits, axis=-1)
    margin = srt[..., -1] - srt[..., -2]
    worst, ndiv = 0.0, 0
    for b in range(n):
        neq = np.nonzero(ids[b, :L] != want[b, :L])[0]
        if neq.size:
            t = int(neq[0])
            ndiv += 1
            worst = max(worst, float(margin[b, t - 1]))
            assert margin[b, t - 1] < FP8_GAP_TOL, f"crop {b} ({hw[b][0]}x{hw[b][1]}) leaves the oracle at token {t}, margin {margin[b, t - 1]:.3e}"
    report(f"configs[4] on one GPU: {n} variable-resolution RGB crops -> device resize -> fp8-attention engine vs oracle over {L} tokens: "
           f"{n - ndiv} rows identical, {ndiv} diverge at oracle margins <= {worst:.3e}")
