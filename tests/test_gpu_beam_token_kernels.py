"""-m gpu: the token form of beam_select_kernel through its operator hook (mocr_op_beam_select_tokens) against
tests/beam_token_util.py in float64, on hand-built logits rows (multiples of 1/64: the slab sums are exact in fp32), as
tests/test_gpu_beam_kernels.py tests the plain form.

* The eight situations of the plain test with the four new arrays set and every row under set 0 (ALL): every old output is
  bit-identical to mocr_op_beam_select's, and the two log-probability histories equal the reference.
* Seven new situations under token sets: tokens, parents, both histories of ids and of log-probabilities, the finished set
  and every flag exact; guard rows and the tails behind ids_ld / generate(max_length) untouched.

BOUNDS.  A token log-probability is (v - max) - log S with |v - max| <= ~20 and log S <= log 6144 = 8.7: three fp32 roundings
of values below 32 (ulp 1.9e-6 each) and the error of the fp32 sum of 6144 __expf terms and of logf, ~1e-6 relative to S -
1e-5 absolute is generous, and it is the bound the plain test puts on the scores.  A running score of a candidate that
stopped carries the reference's -1e9: fp32 holds it to half an ulp of 1e9 (32), so such scores are compared to 1e-7 relative.
The measured maxima go to the parity report."""
import numpy as np
import pytest

import beam_token_util as tu
import beam_util as bu
import constraint_util as cu
from gpu_util import engine, report
from test_gpu_beam_kernels import D, EOS, GUARD, LD, MAX_LEN, ML, PAD, SENT, SITUATIONS, START, V, _base, _f32, _i32, _plant

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LSENT = -777.0                      # what the log-probability rows hold where nothing may write


def _with_histories(rs, sc, K):
    """a situation of either test plus what the token form reads: random log-probability histories (multiples of 1/64, so a
    swap is visible and the copies are exact), those of its finished entries, and no set"""
    sc.setdefault("mask", None)
    sc["logp"] = [[0.0] + [float(x) for x in -rs.randint(1, 256, sc["t"]) / 64.0] for _ in range(K)]
    sc["hyp_logp"] = [[0.0] + [float(x) for x in -rs.randint(1, 256, len(seq) - 1) / 64.0] for _, seq in sc["hyp"]]
    return sc


def _planted(first, K, per=3):
    return [first + 10 * k + j for k in range(K) for j in range(per)]


# ------------------------------------------------------------------------------------------------ the seven new situations
def _sc_best_outside(rs, K):
    """beam 0's best token (60) lies outside the set; the others' best token (61) is a member and wins for them"""
    sc = _base(rs, K, 3)
    for k in range(K):
        _plant(sc, k, 200 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
        sc["logits"][k, 61 if k else 60] = 5.0
    sc["mask"] = cu.mask_of(_planted(200, K) + [61] + [int(x) for x in rs.choice(np.arange(1000, 6000), 20, replace=False)])
    sc["check"] = lambda c: (0, 60) not in list(zip(c["cpar"], c["ctok"])) and all((k, 61) in list(zip(c["cpar"], c["ctok"])) for k in range(1, K))
    return sc


def _sc_ban_and_set(rs, K):
    """no_repeat_ngram_size 2: beam 1 holds (50, 60) and (50, 62) and ends in 50 - 60 is banned AND outside the set, 62 is banned
    inside it; both are the best tokens of every beam"""
    sc = _base(rs, K, 5)
    sc["hist"][0] = [START, 50, 63, 51, 64, 52]
    sc["hist"][1] = [START, 50, 60, 50, 62, 50]
    for k in range(K):
        sc["logits"][k, 60] = 6.0
        sc["logits"][k, 62] = 5.0 - 0.125 * k
        _plant(sc, k, 300 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
    sc["mask"] = cu.mask_of(_planted(300, K) + [62, 50, 51, 52])
    pairs = lambda c: list(zip(c["cpar"], c["ctok"]))
    sc["check"] = lambda c: all(t != 60 for t in c["ctok"]) and (0, 62) in pairs(c) and (1, 62) not in pairs(c)
    return sc


def _sc_eos_unlisted(rs, K):
    """the caller's list does not name EOS (every set holds it all the same) and EOS is the best candidate"""
    sc = _base(rs, K, 3)
    for k in range(K):
        _plant(sc, k, 400 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
    sc["logits"][0, EOS] = 4.0
    listed = _planted(400, K)
    assert EOS not in listed
    sc["mask"] = cu.mask_of(listed)
    sc["check"] = lambda c: c["ctok"][0] == EOS
    return sc


def _sc_swap(rs, K):
    """beam 1 leads: the next beams' parents start [1, 0, ...], so the two histories change places - ids and log-probabilities"""
    sc = _base(rs, K, 6)
    sc["run"] = [-2.0, -1.0] + [-3.0 - 0.3125 * k for k in range(2, K)]
    for k in range(K):
        _plant(sc, k, 500 + 10 * k, [3.0 - 1.5 * j for j in range(3)])
    sc["mask"] = cu.mask_of(_planted(500, K) + [int(x) for x in rs.choice(np.arange(1000, 6000), 30, replace=False)])
    sc["check"] = lambda c: list(c["cpar"][:2]) == [1, 0]
    return sc


def _sc_push_down(rs, K):
    """the finished set holds one entry; the best candidate is an EOS that scores above it, so the old entry moves to slot 1 -
    its ids and its log-probabilities"""
    sc = _base(rs, K, 3)
    sc["run"] = [-0.125 - 0.3125 * k for k in range(K)]
    sc["hyp"] = [(-2.5, [START] + [int(x) for x in rs.choice(np.arange(1000, 6000), 4, replace=False)] + [EOS])]
    sc["logits"][0, EOS] = 9.0
    for k in range(K):
        _plant(sc, k, 600 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
    sc["mask"] = cu.mask_of(_planted(600, K))
    sc["check"] = lambda c: c["ctok"][0] == EOS and c["cv"][0] / 4.0 > -2.5
    return sc


def _sc_dead(rs, K):
    """a set of two tokens (a and EOS) with no_repeat_ngram_size 2, and every beam but the first holds (50, a) and ends in 50:
    K + 1 of the K V scores are finite, the other winners are dead"""
    a = 700
    sc = _base(rs, K, 3)
    sc["hist"][0] = [START, 51, 52, 53]
    for k in range(1, K):
        sc["hist"][k] = [START, 50, a, 50]
    for k in range(K):
        sc["logits"][k, a] = 3.0
        sc["logits"][k, EOS] = 2.0 - 0.25 * k
    sc["mask"] = cu.mask_of([a])
    sc["check"] = lambda c: int(np.isfinite(c["cv"]).sum()) == K + 1 and (0, a) == (c["cpar"][0], c["ctok"][0])
    return sc


def _sc_done_under_a_set(rs, K):
    """a crop that has ended writes nothing, whatever its set"""
    sc = _base(rs, K, 5)
    sc["finished"] = True
    sc["hyp"] = [(-0.5, [START, 1234, EOS])]
    sc["mask"] = cu.mask_of([1234])
    return sc


NEW_SITUATIONS = [_sc_best_outside, _sc_ban_and_set, _sc_eos_unlisted, _sc_swap, _sc_push_down, _sc_dead, _sc_done_under_a_set]


# ------------------------------------------------------------------------------------------------ one launch
def _build(rs, scs, K, nslab):
    """the arrays of one launch, as tests/test_gpu_beam_kernels.py lays them out: G groups of K slots (K = 3: a trailing partial
    group of two padding slots), two crops nobody decodes, a guard row behind ids / hyp_ids and behind the two histories"""
    G = len(scs)
    n = 8 if K == 3 else G * K
    crops_n = G + 2
    R = crops_n * K
    crop_of = rs.permutation(crops_n)[:G]
    a = dict(n=n, G=G, R=R, crop_of=crop_of)
    a["rowmap"] = np.full(n, R - 1, np.int32)
    a["ids"] = np.full((R + 1, LD), SENT, np.int32)
    a["step"] = np.zeros(n, np.int32)
    a["fin"] = np.zeros(R, np.int32)
    a["len"] = np.full(R, ML, np.int32)
    a["bscore"] = np.full(R, -5.5, np.float32)
    a["parent"] = np.full(R, SENT, np.int32)
    a["hyp_ids"] = np.full((R + 1, LD), PAD, np.int32)
    a["hyp_len"] = np.zeros(R, np.int32)
    a["hyp_score"] = np.full(R, -bu.NEG, np.float32)
    a["hopen"] = np.full(crops_n, 1, np.int32)
    a["blogp"] = np.full((R + 1, LD), LSENT, np.float32)
    a["hlogp"] = np.zeros((R + 1, LD), np.float32)
    a["hlogp"][R] = LSENT
    masks = [np.ones(V, bool)]                      # set 0: the whole vocabulary
    a["set_of_row"] = np.zeros(R, np.int32)
    logits = rs.randint(-512, -256, (n, V)).astype(np.float64) / 64.0
    for g, sc in enumerate(scs):
        c = int(crop_of[g])
        if sc["mask"] is not None:
            masks.append(sc["mask"])
            a["set_of_row"][c * K:(c + 1) * K] = len(masks) - 1
        for k in range(K):
            r, s = c * K + k, g * K + k
            a["rowmap"][s] = r
            a["step"][s] = sc["t"]
            a["ids"][r, :sc["t"] + 1] = sc["hist"][k]
            a["blogp"][r, :sc["t"] + 1] = sc["logp"][k]
            a["bscore"][r] = sc["run"][k]
            a["fin"][r] = 1 if sc["finished"] else 0
            logits[s] = sc["logits"][k]
        for j, (s_, seq) in enumerate(sc["hyp"]):
            a["hyp_ids"][c * K + j, :len(seq)] = seq
            a["hyp_len"][c * K + j] = len(seq)
            a["hyp_score"][c * K + j] = s_
            a["hlogp"][c * K + j, :len(seq)] = sc["hyp_logp"][j]
        a["hopen"][c] = 1 if sc["open"] else 0
    a["step"][G * K:] = 7
    a["bias"] = rs.randint(-128, 128, V).astype(np.float64) / 64.0
    parts = rs.randint(-128, 128, (nslab, n, V)).astype(np.float64) / 64.0
    parts[-1] = logits - a["bias"] - parts[:-1].sum(0)
    a["parts"] = parts
    a["table"] = cu.pack_sets(np.stack(masks))
    a["unf"] = np.array([1000, SENT], np.int32)
    return a


def _run(eng, dtype, a, bcfg, nslab, tokens):
    n, R = a["n"], a["R"]
    d = {k: _i32(a[k]) for k in ("ids", "step", "fin", "len", "unf", "rowmap", "parent", "hyp_ids", "hyp_len", "hopen")}
    d.update({k: _f32(a[k]) for k in ("bscore", "hyp_score", "blogp", "hlogp")})
    x32 = torch.full((n + GUARD, D), float("nan"), device="cuda")
    xt = torch.full((n + GUARD, D), float("nan"), device="cuda", dtype=torch.bfloat16 if dtype == "bf16" else torch.float32)
    cache = torch.full((R, MAX_LEN, D), float("nan"), device="cuda", dtype=xt.dtype)
    table = torch.from_numpy(a["table"].view(np.int32).copy()).cuda()
    sets = _i32(a["set_of_row"])
    torch.cuda.synchronize()
    kw = dict(first=0, n=n, slabs=_f32(a["parts"]), nslab=nslab, vbias=_f32(a["bias"]), ids=d["ids"], step=d["step"], finished=d["fin"],
              len=d["len"], n_unfinished=d["unf"], rowmap=d["rowmap"], ids_ld=LD, max_len=ML, n_real=a["G"] * bcfg.num_beams,
              x_f32=x32, x_t=xt, cache=cache)
    state = (d["bscore"], d["parent"], d["hyp_ids"], d["hyp_len"], d["hyp_score"], d["hopen"])
    if tokens:
        eng.op_beam_select_tokens(bcfg, *state, d["blogp"], d["hlogp"], table, sets, **kw)
    else:
        eng.op_beam_select(bcfg, *state, **kw)
    got = {k: v.cpu().numpy() for k, v in d.items()}
    got["x32"], got["cache"] = x32.cpu().numpy().view(np.int32), cache.view(torch.int16 if dtype == "bf16" else torch.int32).cpu().numpy()
    got["xt"] = xt.view(torch.int16 if dtype == "bf16" else torch.int32).cpu().numpy()
    return got


def _state_of(sc, K):
    st = tu.State(K, START)
    st.seqs = [list(h) for h in sc["hist"]]
    st.logp = [list(h) for h in sc["logp"]]
    st.run = np.array(sc["run"], np.float64)
    for j, (s, seq) in enumerate(sc["hyp"]):
        st.hyp_score[j], st.hyp_seq[j], st.hyp_logp[j] = s, list(seq), list(sc["hyp_logp"][j])
    st.open = sc["open"]
    return st


def _close(got, want, what):
    """|got - want| of two score arrays: 1e-5 absolute, 1e-7 relative on the -1e9 ones, -inf exactly; returns the largest
    absolute error among the ordinary ones"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    dead = np.isinf(want)
    np.testing.assert_array_equal(got[dead], want[dead], err_msg=f"{what}: a dead score is -inf")
    big = ~dead & (np.abs(want) > 1e8)
    assert (np.abs(got[big] - want[big]) <= 1e-7 * np.abs(want[big])).all(), f"{what}: the -1e9 scores"
    err = float(np.abs(got[~dead & ~big] - want[~dead & ~big]).max()) if (~dead & ~big).any() else 0.0
    assert err <= 1e-5, f"{what}: {err} from float64"
    return err


def _check(a, got, scs, cfg, K):
    """a token-form launch against the float64 reference, group by group -> (largest score error, largest log-probability
    error, smallest candidate gap)"""
    R = a["R"]
    want = {k: a[k].copy() for k in ("ids", "fin", "len", "parent", "hyp_ids", "hyp_len", "hopen", "blogp", "hlogp")}
    want_hs, want_bs = a["hyp_score"].astype(np.float64), a["bscore"].astype(np.float64)
    free = np.zeros((R + 1, LD), bool)              # cells of a dead running beam: a token in [0, vocab), any log-probability
    n_unf, min_gap = 1000, np.inf
    for g, sc in enumerate(scs):
        c = int(a["crop_of"][g])
        if sc["finished"]:
            continue
        st = _state_of(sc, K)
        cv, cpar, ctok, stop, clp = tu.step(tu.processed(sc["logits"], st, cfg, sc["mask"]), st, cfg, ML, EOS)
        assert sc["check"](dict(cv=cv, cpar=cpar, ctok=ctok, stop=stop)), f"situation {g} is not what it says"
        assert st.min_gap >= 1e-3, f"a constructed case has candidates {st.min_gap} apart"
        min_gap = min(min_gap, st.min_gap)
        L = sc["t"] + 1
        for j in range(K):
            r = c * K + j
            n_h = len(st.hyp_seq[j])
            want["hyp_len"][r], want_hs[r] = n_h, st.hyp_score[j]
            want["hyp_ids"][r], want["hlogp"][r] = PAD, 0.0
            want["hyp_ids"][r, :n_h], want["hlogp"][r, :n_h] = st.hyp_seq[j], st.hyp_logp[j]
        want["hopen"][c] = 1 if st.open else 0
        for k in range(K):
            r = c * K + k
            if st.done:
                want["fin"][r], want["len"][r], want["parent"][r] = 1, sc["t"] + 2, k
                want_bs[r] = np.nan
            else:
                want_bs[r] = st.run[k]
                if np.isinf(st.run[k]):
                    free[r, :L + 1] = True
                    assert 0 <= got["parent"][r] < K and ((got["ids"][r, :L + 1] >= 0) & (got["ids"][r, :L + 1] < V)).all()
                    want["parent"][r] = got["parent"][r]
                else:
                    want["parent"][r] = st.parents[k]
                    want["ids"][r, :L + 1] = st.seqs[k]
                    want["blogp"][r, :L + 1] = st.logp[k]
        n_unf -= K if st.done else 0
    for k in ("ids", "parent", "fin", "len", "hopen", "hyp_len", "hyp_ids"):
        np.testing.assert_array_equal(np.where(free, 0, got[k]) if k == "ids" else got[k], np.where(free, 0, want[k]) if k == "ids" else want[k],
                                      err_msg=k)
    np.testing.assert_array_equal(got["unf"], [n_unf, SENT])
    np.testing.assert_array_equal(got["step"], a["step"] + 1)
    np.testing.assert_array_equal(got["rowmap"], a["rowmap"])
    live = ~np.isnan(want_bs)
    e_score = max(_close(got["hyp_score"], want_hs, "hyp_score"), _close(got["bscore"][live], want_bs[live], "beam_score"))
    # the histories: what the step appended within the bound, everything else - the copied histories, the zeros behind a
    # hypothesis, the guard row, the tails, the rows of crops that ended or that nobody decodes - exactly
    e_logp = 0.0
    for name in ("blogp", "hlogp"):
        g_, w_ = got[name].astype(np.float64), want[name].astype(np.float64)
        cmp = ~free
        assert np.isfinite(g_[cmp]).all() and (g_[cmp][g_[cmp] != LSENT] <= 0).all(), f"{name}: finite and <= 0"
        err = np.abs(g_ - w_)
        e_logp = max(e_logp, float(err[cmp].max()))
        assert err[cmp].max() <= 1e-5, f"{name}: {err[cmp].max()} from float64"
        exact = cmp & (w_ * 64.0 == np.round(w_ * 64.0))          # cells the step only copied or left alone: multiples of 1/64
        np.testing.assert_array_equal(got[name][exact], w_[exact].astype(np.float32), err_msg=f"{name}: copied or untouched cells")
    return e_score, e_logp, min_gap


def _walk(rs, situations, K):
    G = 2 if K == 3 else 3
    for first in range(0, len(situations), G):
        yield [(first + g) % len(situations) for g in range(G)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("nslab", [1, 3])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_set_all_is_the_plain_selection_bit_for_bit(K, nslab, dtype):
    from manga_ocr.engine import BeamConfig
    eng = engine(dtype)
    rs = np.random.RandomState(2000 * K + 10 * nslab + (dtype == "bf16"))
    cfg, bcfg = bu.Config(K, 1.0, True, 2), BeamConfig(K, 1.0, True, 2)
    seen, worst = set(), [0.0, 0.0]
    for idx in _walk(rs, SITUATIONS, K):
        scs = [_with_histories(rs, SITUATIONS[i](rs, K), K) for i in idx]
        seen.update(idx)
        a = _build(rs, scs, K, nslab)
        plain, tok = _run(eng, dtype, a, bcfg, nslab, False), _run(eng, dtype, a, bcfg, nslab, True)
        for k in ("ids", "step", "fin", "len", "unf", "rowmap", "parent", "hyp_ids", "hyp_len", "hopen", "x32", "xt", "cache"):
            np.testing.assert_array_equal(tok[k], plain[k], err_msg=f"{k}: the token form under set 0 against the plain form")
        for k in ("bscore", "hyp_score"):
            np.testing.assert_array_equal(tok[k].view(np.int32), plain[k].view(np.int32), err_msg=f"{k}: bit for bit")
        for k in ("blogp", "hlogp"):
            np.testing.assert_array_equal(plain[k], a[k], err_msg=f"{k}: the plain form writes no history")
        e_score, e_logp, _ = _check(a, tok, scs, cfg, K)
        worst = [max(worst[0], e_score), max(worst[1], e_logp)]
    assert seen == set(range(len(SITUATIONS)))
    report(f"beam_select_tokens {dtype} K={K} nslab={nslab}: 8 plain situations under set 0 bit-identical to beam_select; "
           f"log-probability histories {worst[1]:.2e} from float64 (bound 1e-5), scores {worst[0]:.2e}")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("nslab", [1, 3])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_token_sets_against_float64(K, nslab, dtype):
    from manga_ocr.engine import BeamConfig
    eng = engine(dtype)
    rs = np.random.RandomState(3000 * K + 10 * nslab + (dtype == "bf16"))
    cfg, bcfg = bu.Config(K, 1.0, False, 2), BeamConfig(K, 1.0, False, 2)
    seen, worst, min_gap = set(), [0.0, 0.0], np.inf
    for idx in _walk(rs, NEW_SITUATIONS, K):
        scs = [_with_histories(rs, NEW_SITUATIONS[i](rs, K), K) for i in idx]
        seen.update(idx)
        a = _build(rs, scs, K, nslab)
        got = _run(eng, dtype, a, bcfg, nslab, True)
        e_score, e_logp, gap = _check(a, got, scs, cfg, K)
        worst, min_gap = [max(worst[0], e_score), max(worst[1], e_logp)], min(min_gap, gap)
    assert seen == set(range(len(NEW_SITUATIONS)))
    report(f"beam_select_tokens {dtype} K={K} nslab={nslab}: 7 situations under token sets exact; log-probability histories "
           f"{worst[1]:.2e} from float64 (bound 1e-5), scores {worst[0]:.2e}; closest candidates {min_gap:.2e}")
