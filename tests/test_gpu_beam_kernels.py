"""-m gpu: the two beam-search kernels through their operator hooks (mocr_op_beam_select / mocr_op_beam_permute), which
launch through the helpers the decode step uses.

beam_select_kernel against tests/beam_util.py in float64: hand-built logits rows (multiples of 1/64, so the slab sums are exact
in fp32) for eight situations - each crop group of a launch is one of them, the launches of a test walk through all eight:
tokens, parents, histories, the finished set's ids / lengths and every flag exact, scores within 1e-5, n_unfinished down by
exactly K per crop that ended, and on the reference no two candidates closer than 1e-3.  K = 3 runs on 8 slots: two live
groups and a trailing partial group of padding slots.

beam_permute_kernel against numpy.take, bit for bit, on a buffer of random bytes with a guard region behind it."""
import numpy as np
import pytest

import beam_util as bu
from gpu_util import bf16_round, engine, report, weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

D, V = 768, 6144
MAX_LEN = 300                       # the engines' max_len: the latent cache's position stride
START, EOS, PAD = 2, 3, 0
SENT = -777
GUARD = 2
ML, LD = 16, 20                     # generate(max_length) of the launches and the ids rows' stride (> ML: the tail stays)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _emb_ref(w, tok, pos, eps=1e-12):
    d = "decoder.bert.embeddings."
    x = (w[d + "word_embeddings.weight"][tok].astype(np.float64) + w[d + "token_type_embeddings.weight"][0]
         + w[d + "position_embeddings.weight"][pos])
    m = x.mean()
    return (x - m) / np.sqrt(((x - m) ** 2).mean() + eps) * w[d + "LayerNorm.weight"].astype(np.float64) + w[d + "LayerNorm.bias"].astype(np.float64)


# ------------------------------------------------------------------------------------------------ the eight situations
def _base(rs, K, t):
    """a live crop at step t: distinct history tokens (no n-gram can repeat), noise logits in [-8, -4)"""
    hist = [[START] + [int(x) for x in rs.choice(np.arange(1000, 6000), t, replace=False)] for _ in range(K)]
    lg = rs.randint(-512, -256, (K, V)).astype(np.float64) / 64.0
    return dict(t=t, hist=hist, run=[-1.0 - 0.3125 * k for k in range(K)], hyp=[], open=True, finished=False, logits=lg)


def _plant(sc, k, first_tok, vals):
    for j, v in enumerate(vals):
        sc["logits"][k, first_tok + j] = v


def _sc_eos_best(rs, K):
    sc = _base(rs, K, 3)
    for k in range(K):
        _plant(sc, k, 200 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
    sc["logits"][0, EOS] = 4.0
    sc["check"] = lambda c: c["ctok"][0] == EOS
    return sc


def _sc_eos_low(rs, K):
    """EOS ranks in K .. 2K - 1: it neither enters the finished set nor continues.  The last beam holds nothing but its EOS
    among the candidates, so its value can be set between ranks K - 1 and K of the others."""
    sc = _base(rs, K, 4)
    _plant(sc, 0, 300, [4.0 - 0.375 * j for j in range(2 * K + 2)])
    st = _state_of(sc, K)
    acc = bu.accumulate(sc["logits"], st, bu.Config(K))
    top = np.sort(acc.reshape(-1))[::-1]
    target = 0.5 * (top[K - 1] + top[K])
    lo, hi = -4.0, 12.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        sc["logits"][K - 1, EOS] = mid
        a = bu.accumulate(sc["logits"], st, bu.Config(K))[K - 1, EOS]
        lo, hi = (mid, hi) if a < target else (lo, mid)
    sc["logits"][K - 1, EOS] = np.round(lo * 64.0) / 64.0
    sc["check"] = lambda c: EOS in list(c["ctok"][K:]) and EOS not in list(c["ctok"][:K])
    return sc


def _sc_all_eos(rs, K):
    """the top K candidates are all EOS - the reason for keeping 2 K"""
    sc = _base(rs, K, 2)
    for k in range(K):
        sc["logits"][k, EOS] = 6.0
        _plant(sc, k, 400 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
    sc["check"] = lambda c: all(int(x) == EOS for x in c["ctok"][:K]) and all(int(x) != EOS for x in c["ctok"][K:])
    return sc


def _sc_one_beam(rs, K):
    """the first step: running scores [0, -1e9, ...], all K winners come from beam 0"""
    sc = _base(rs, K, 0)
    sc["run"] = [0.0] + [-bu.NEG] * (K - 1)
    for k in range(K):
        _plant(sc, k, 500, [3.0 - 0.5 * j for j in range(2 * K + 2)])
    sc["check"] = lambda c: all(int(p) == 0 for p in c["cpar"])
    return sc


def _sc_ban(rs, K):
    """no_repeat_ngram_size 2: beam 1 holds (50, 60) and ends in 50, so 60 - the best token of both beams - is banned for it only"""
    sc = _base(rs, K, 3)
    sc["hist"][0] = [START, 50, 61, 51]
    sc["hist"][1] = [START, 50, 60, 50]
    for k in range(K):
        sc["logits"][k, 60] = 5.0
        _plant(sc, k, 600 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
    sc["check"] = lambda c: (0, 60) in list(zip(c["cpar"], c["ctok"])) and (1, 60) not in list(zip(c["cpar"], c["ctok"]))
    return sc


def _sc_length(rs, K):
    sc = _base(rs, K, ML - 2)
    for k in range(K):
        _plant(sc, k, 700 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
    sc["check"] = lambda c: bool(np.all(c["stop"]))
    return sc


def _sc_full(rs, K):
    """the finished set is already full and early_stopping is true: the best candidate, an EOS that would score above the
    set's worst, is not taken"""
    sc = _base(rs, K, 3)
    sc["run"] = [-0.125 - 0.3125 * k for k in range(K)]
    sc["hyp"] = [(-0.25 - 0.125 * j, [START] + [int(x) for x in rs.choice(np.arange(1000, 6000), 2 + j, replace=False)] + [EOS]) for j in range(K)]
    sc["logits"][0, EOS] = 9.0
    for k in range(K):
        _plant(sc, k, 800 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
    sc["check"] = lambda c: c["ctok"][0] == EOS and c["cv"][0] / 4.0 > -0.25 - 0.125 * (K - 1)
    return sc


def _sc_done(rs, K):
    sc = _base(rs, K, 5)
    sc["finished"] = True
    sc["hyp"] = [(-0.5, [START, 1234, EOS])]
    return sc


SITUATIONS = [_sc_eos_best, _sc_eos_low, _sc_all_eos, _sc_one_beam, _sc_ban, _sc_length, _sc_full, _sc_done]


def _state_of(sc, K):
    st = bu.State(K, START)
    st.seqs = [list(h) for h in sc["hist"]]
    st.run = np.array(sc["run"], np.float64)
    for j, (s, seq) in enumerate(sc["hyp"]):
        st.hyp_score[j] = s
        st.hyp_seq[j] = list(seq)
    st.open = sc["open"]
    return st


def _launch_and_check(eng, w, rs, K, nslab, dtype, cfg, bcfg, scs, n):
    """One launch over the crop groups `scs` on n slots (beside two crops nobody decodes) against beam_util in float64
    -> (the worst score error, the worst embedding error, the closest two candidates of the reference)."""
    G = n // K
    worst_score, worst_emb, min_gap = 0.0, 0.0, np.inf
    crops_n = G + 2                             # two crops nobody decodes: their rows must stay as they are
    R = crops_n * K
    crop_of = rs.permutation(crops_n)[:G]
    rowmap = np.full(n, R - 1, np.int32)        # (the padding slots of a partial group name a row of the last crop)
    ids = np.full((R + 1, LD), SENT, np.int32)
    step = np.zeros(n, np.int32)
    finished = np.zeros(R, np.int32)
    lens = np.full(R, ML, np.int32)
    bscore = np.full(R, -5.5, np.float32)
    parent = np.full(R, SENT, np.int32)
    hyp_ids = np.full((R + 1, LD), PAD, np.int32)
    hyp_len = np.zeros(R, np.int32)
    hyp_score = np.full(R, -bu.NEG, np.float32)
    hopen = np.full(crops_n, 1, np.int32)
    logits = rs.randint(-512, -256, (n, V)).astype(np.float64) / 64.0
    for g, sc in enumerate(scs):
        c = int(crop_of[g])
        for k in range(K):
            r, s = c * K + k, g * K + k
            rowmap[s] = r
            step[s] = sc["t"]
            ids[r, :sc["t"] + 1] = sc["hist"][k]
            bscore[r] = sc["run"][k]
            finished[r] = 1 if sc["finished"] else 0
            logits[s] = sc["logits"][k]
        for j, (s_, seq) in enumerate(sc["hyp"]):
            hyp_ids[c * K + j, :len(seq)] = seq
            hyp_len[c * K + j] = len(seq)
            hyp_score[c * K + j] = s_
        hopen[c] = 1 if sc["open"] else 0
    step[G * K:] = 7                            # the padding slots' steps advance like everybody's
    bias = rs.randint(-128, 128, V).astype(np.float64) / 64.0
    parts = rs.randint(-128, 128, (nslab, n, V)).astype(np.float64) / 64.0
    parts[-1] = logits - bias - parts[:-1].sum(0)
    n_unf0 = 1000
    d = dict(ids=_i32(ids), step=_i32(step), fin=_i32(finished), len=_i32(lens), unf=_i32([n_unf0, SENT]), map=_i32(rowmap),
             bscore=_f32(bscore), parent=_i32(parent), hyp_ids=_i32(hyp_ids), hyp_len=_i32(hyp_len), hyp_score=_f32(hyp_score),
             hopen=_i32(hopen))
    x32 = torch.full((n + GUARD, D), float("nan"), device="cuda")
    xt = torch.full((n + GUARD, D), float("nan"), device="cuda", dtype=torch.bfloat16 if dtype == "bf16" else torch.float32)
    cache = torch.full((R, MAX_LEN, D), float("nan"), device="cuda", dtype=xt.dtype)
    torch.cuda.synchronize()
    eng.op_beam_select(bcfg, d["bscore"], d["parent"], d["hyp_ids"], d["hyp_len"], d["hyp_score"], d["hopen"],
                       first=0, n=n, slabs=_f32(parts), nslab=nslab, vbias=_f32(bias), ids=d["ids"], step=d["step"], finished=d["fin"],
                       len=d["len"], n_unfinished=d["unf"], rowmap=d["map"], ids_ld=LD, max_len=ML, n_real=G * K, x_f32=x32, x_t=xt,
                       cache=cache)
    got = {k: v.cpu().numpy() for k, v in d.items()}
    # ---- the reference, group by group
    want_ids, want_fin, want_len = ids.copy(), finished.copy(), lens.copy()
    want_parent, want_hyp_ids, want_hyp_len = parent.copy(), hyp_ids.copy(), hyp_len.copy()
    want_hyp_score = hyp_score.astype(np.float64)
    want_bscore = bscore.astype(np.float64)
    want_open = hopen.copy()
    n_unf = n_unf0
    emb = {}                                    # slot -> (row, token, position)
    for g, sc in enumerate(scs):
        c = int(crop_of[g])
        if sc["finished"]:
            continue
        st = _state_of(sc, K)
        cv, cpar, ctok, stop = bu.step(bu.accumulate(sc["logits"], st, cfg), st, cfg, ML, EOS)
        assert sc["check"](dict(cv=cv, cpar=cpar, ctok=ctok, stop=stop)), f"situation {sc} is not what it says"
        assert st.min_gap >= 1e-3, f"a constructed case has candidates {st.min_gap} apart"
        min_gap = min(min_gap, st.min_gap)
        L = sc["t"] + 1
        for j in range(K):
            r = c * K + j
            want_hyp_len[r] = len(st.hyp_seq[j])
            want_hyp_score[r] = st.hyp_score[j]
            want_hyp_ids[r] = PAD
            want_hyp_ids[r, :len(st.hyp_seq[j])] = st.hyp_seq[j]
        want_open[c] = 1 if st.open else 0
        for k in range(K):
            r = c * K + k
            if st.done:
                want_fin[r], want_len[r], want_parent[r] = 1, sc["t"] + 2, k
                want_bscore[r] = np.nan        # (written, but nobody reads a crop's running scores once it ended)
            else:
                want_parent[r] = st.parents[k]
                want_bscore[r] = st.run[k]
                want_ids[r, :L + 1] = st.seqs[k]
                emb[g * K + k] = (r, st.seqs[k][-1], L)
        n_unf -= K if st.done else 0
    np.testing.assert_array_equal(got["ids"], want_ids, err_msg="ids: the new beams' histories (a crop that ended keeps its rows)")
    np.testing.assert_array_equal(got["parent"], want_parent, err_msg="parent")
    np.testing.assert_array_equal(got["fin"], want_fin, err_msg="finished")
    np.testing.assert_array_equal(got["len"], want_len, err_msg="len")
    np.testing.assert_array_equal(got["unf"], [n_unf, SENT], err_msg="n_unfinished drops by K per crop that ended")
    np.testing.assert_array_equal(got["step"], step + 1, err_msg="step advances in every slot, padding and ended crops included")
    np.testing.assert_array_equal(got["map"], rowmap)
    np.testing.assert_array_equal(got["hopen"], want_open, err_msg="heuristic_open")
    np.testing.assert_array_equal(got["hyp_len"], want_hyp_len, err_msg="finished set: lengths")
    np.testing.assert_array_equal(got["hyp_ids"], want_hyp_ids, err_msg="finished set: ids")
    live = ~np.isnan(want_bscore)
    for name, g_, w_ in (("hyp_score", got["hyp_score"], want_hyp_score), ("beam_score", got["bscore"][live], want_bscore[live])):
        err = float(np.abs(g_.astype(np.float64) - w_).max())
        worst_score = max(worst_score, err)
        assert err <= 1e-5, f"{name}: {err} from float64"
    # ---- the next inputs: x by slot, the layer-0 cache by row at position t + 1; nothing else
    g32, gt, gc = x32.cpu().numpy().astype(np.float64), xt.float().cpu().numpy().astype(np.float64), cache.float().cpu().numpy()
    written = np.zeros((R, MAX_LEN), bool)
    for s in range(n + GUARD):
        if s not in emb:
            assert np.isnan(g32[s]).all() and np.isnan(gt[s]).all(), f"x of slot {s} written (ended crop, padding or guard)"
            continue
        r, tok, p = emb[s]
        ref = _emb_ref(w, tok, p)
        err = float((np.abs(g32[s] - ref) / np.abs(ref).max()).max())
        worst_emb = max(worst_emb, err)
        assert err <= 1e-5, f"embedding of slot {s}: {err} of the row scale"
        stored = bf16_round(g32[s].astype(np.float32)).astype(np.float64) if dtype == "bf16" else g32[s].astype(np.float32).astype(np.float64)
        np.testing.assert_array_equal(gt[s], stored, err_msg="x_t != storage rounding of x_f32")
        np.testing.assert_array_equal(gc[r, p].astype(np.float64), gt[s], err_msg="cache row != x_t")
        written[r, p] = True
    assert np.isnan(gc[~written]).all(), "cache written outside the new beams' rows at position t + 1"
    return worst_score, worst_emb, min_gap


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("nslab", [1, 3])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_beam_select_against_float64(K, nslab, dtype):
    from manga_ocr.engine import BeamConfig
    eng = engine(dtype)
    w = weights(0)
    rs = np.random.RandomState(1000 * K + 10 * nslab + (dtype == "bf16"))
    cfg = bu.Config(K, 1.0, True, 2)
    bcfg = BeamConfig(K, 1.0, True, 2)
    n = 8 if K == 3 else 3 * K                      # K = 3: two live groups and a partial group of two padding slots
    G = n // K
    seen = set()
    worst_score, worst_emb, min_gap = 0.0, 0.0, np.inf
    for first in range(0, len(SITUATIONS), G):
        scs = [SITUATIONS[(first + g) % len(SITUATIONS)](rs, K) for g in range(G)]
        seen.update((first + g) % len(SITUATIONS) for g in range(G))
        ws, we, mg = _launch_and_check(eng, w, rs, K, nslab, dtype, cfg, bcfg, scs, n)
        worst_score, worst_emb, min_gap = max(worst_score, ws), max(worst_emb, we), min(min_gap, mg)
    assert seen == set(range(len(SITUATIONS)))
    report(f"beam_select {dtype} K={K} nslab={nslab}: 8 situations exact; scores {worst_score:.2e} from float64, embedding {worst_emb:.2e} "
           f"of the row scale; closest candidates {min_gap:.2e}")


def _sc_windows(rs, K, n):
    """no_repeat_ngram_size n on histories of five tokens: token 60 - the best of both beams - is banned for beam 1 only.
    n = 1: every token of a row is banned, and beam 1 alone holds 60.  n = 3: beam 1 ends in (50, 51), which it holds
    followed by 60; beam 0 ends in (50, 51) too, but holds it nowhere else - it holds 51 followed by 60, the ban of n = 2."""
    sc = _base(rs, K, 4)
    sc["hist"][0] = {1: [START, 50, 61, 52, 53], 3: [START, 51, 60, 50, 51]}[n]
    sc["hist"][1] = {1: [START, 50, 60, 52, 53], 3: [50, 51, 60, 50, 51]}[n]
    for k in range(K):
        sc["logits"][k, 60] = 5.0
        _plant(sc, k, 600 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
    sc["check"] = lambda c: (0, 60) in list(zip(c["cpar"], c["ctok"])) and (1, 60) not in list(zip(c["cpar"], c["ctok"]))
    return sc


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 3])
def test_beam_ngram_windows_exact(n, dtype):
    """The selection's n-gram scan at the window lengths the launches above (n = 2) do not run: an empty key and a key of two
    tokens.  K = 2, one live group beside the two untouched crops, one slab; everything test_beam_select_against_float64 asserts."""
    from manga_ocr.engine import BeamConfig
    K = 2
    rs = np.random.RandomState(77 + 10 * n + (dtype == "bf16"))
    ws, we, mg = _launch_and_check(engine(dtype), weights(0), rs, K, 1, dtype, bu.Config(K, 1.0, True, n), BeamConfig(K, 1.0, True, n),
                                   [_sc_windows(rs, K, n)], K)
    report(f"beam_select {dtype} K={K} no_repeat_ngram_size={n}: exact; scores {ws:.2e} from float64, embedding {we:.2e} of the row scale; "
           f"closest candidates {mg:.2e}")


# ------------------------------------------------------------------------------------------------ the cache reorder
def _parents(kind, K):
    if kind == "identity":
        return list(range(K))
    if kind == "cycle":
        return [(k + 1) % K for k in range(K)]
    if kind == "from0":
        return [0] * K
    p = list(range(K))          # one swap
    p[0], p[K - 1] = p[K - 1], p[0]
    return p


LAYOUTS = {            # name -> (segments, bytes per position)
    "latent_bf16": (1, D * 2), "latent_fp32": (1, D * 4), "latent_e4m3": (1, D), "classic_bf16": (12, 64 * 2),
}


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_beam_permute_against_numpy_take(layout, K):
    eng = engine("fp32")
    segs, pb = LAYOUTS[layout]
    layers, P = 2, 24                               # positions per segment (a cache of max_len 24)
    kinds = ["cycle", "done", "from0", "identity", "swap"]      # a crop that ended between two live ones
    G = len(kinds)
    n = G * K + (2 if K == 3 else 0)                # K = 3: a trailing partial group
    crops_n = G + 1
    R = crops_n * K
    rs = np.random.RandomState(7 * K + len(layout))
    seg_stride, row_stride = P * pb, segs * P * pb
    layer_stride = R * row_stride
    total = layers * layer_stride
    guard = 4096
    # (t, max_pos): the selection has left step = t + 1; max_pos sizes the grid and bounds what moves.  The engine's eager steps
    # pass t + 2, a captured graph its bucket's bound (>= step); a bound below step moves max_pos positions only
    for t, max_pos in ((0, 1), (1, 3), (17, 18), (17, 19), (17, P - 1), (17, 12), (P - 2, P - 1)):
        moved = min(t + 1, max_pos)
        buf = rs.randint(0, 256, total + guard).astype(np.uint8)
        crop_of = rs.permutation(crops_n)[:G]
        rowmap = np.full(n, R - 1, np.int32)
        parent = np.full(R, SENT, np.int32)
        finished = np.zeros(R, np.int32)
        step = np.full(n, t + 1, np.int32)          # behind the selection: positions 0 .. t move
        view = buf[:total].reshape(layers, R, segs, P, pb)
        want = buf.copy()
        wv = want[:total].reshape(layers, R, segs, P, pb)
        for g, kind in enumerate(kinds):
            c = int(crop_of[g])
            rows = np.arange(c * K, c * K + K)
            rowmap[g * K:(g + 1) * K] = rows
            par = _parents("identity" if kind == "done" else kind, K)
            if kind == "done":
                par = _parents("cycle", K)          # whatever its parents say, a crop that ended keeps its caches
                finished[rows] = 1
            parent[rows] = par
            if kind != "done":
                wv[:, rows, :, :moved] = np.take(view, rows[np.asarray(par)], axis=1)[:, :, :, :moved]
        d_buf = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        eng.op_beam_permute(d_buf, layers, layer_stride, row_stride, segs, seg_stride, pb, K, _i32(parent), _i32(rowmap), _i32(finished),
                            _i32(step), n, max_pos)
        got = d_buf.cpu().numpy()
        np.testing.assert_array_equal(got[total:], buf[total:], err_msg="guard region behind the buffer")
        np.testing.assert_array_equal(got, want, err_msg=f"{layout} K={K} t={t} max_pos={max_pos}: positions 0 .. {moved - 1} permuted, everything else as it was")
        assert not np.array_equal(want, buf), "the case moves something"
