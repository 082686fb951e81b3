"""-m gpu: the automaton form of beam_select_kernel through its operator hook (mocr_op_beam_select_automaton) against
tests/beam_automaton_util.py in float64, on hand-built logits rows (multiples of 1/64: the slab sums are exact in fp32), as
tests/test_gpu_beam_token_kernels.py tests the token form.

* Seven situations under automata - a state with one edge whose row maximum is a banned EOS, the universal state (6,143
  edges) with an n-gram ban, an accepting leaf (EOS only), a set that meets no edge (a dead beam) beside a beam that is DEAD
  already, several new beams from one parent into different states, a hypothesis inserted above an old one (the states
  shift), the stop by length (the last token walks): tokens, parents, both histories, the beams' and the hypotheses' states,
  the finished set and every flag exact; rows of crops nobody decodes and the guard rows untouched.  Every launch has three
  crop groups and a trailing partial group of K - 1 padding slots.
* With the seven automaton pointers null the hook IS mocr_op_beam_select_positions; under the universal automaton and under
  the one-state automaton of a token set it is bit-identical to the token form under that set.

BOUNDS: those of tests/test_gpu_beam_token_kernels.py (1e-5 absolute on a log-probability and a score, 1e-7 relative on the
-1e9 ones), for its reasons; the reference's candidates are at least 1e-3 apart by construction."""
import numpy as np
import pytest

import automaton_util as au
import beam_automaton_util as bau
import beam_util as bu
import constraint_util as cu
from gpu_util import engine, report
from test_gpu_beam_kernels import D, EOS, GUARD, LD, MAX_LEN, ML, PAD, SENT, START, V, _base, _f32, _i32, _plant
from test_gpu_beam_token_kernels import LSENT, NEW_SITUATIONS, _close, _with_histories

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NONE, DEAD = au.NONE, au.DEAD


def _abase(rs, K, t, trans, accepting, states):
    sc = _base(rs, K, t)
    sc.update(aut=au.Automaton(trans, accepting), ast=list(states), hyp_state=[], mask=None)
    return sc


# ------------------------------------------------------------------------------------------------ the seven situations
def _sc_one_edge(rs, K):
    """every beam in a state of its own with ONE edge and no acceptance; EOS is the maximum of every row and banned all the same"""
    trans = {1 + k: {300 + k: 20 + k} for k in range(K)}
    sc = _abase(rs, K, 1, trans, [], [1 + k for k in range(K)])
    for k in range(K):
        sc["logits"][k, EOS] = 9.0
        sc["logits"][k, 300 + k] = 3.0 - 0.25 * k
    sc["check"] = lambda c: EOS not in list(c["ctok"][:K]) and int(np.isfinite(c["cv"]).sum()) == K and \
        [(int(p), int(x)) for p, x in zip(c["cpar"][:K], c["ctok"][:K])] == [(k, 300 + k) for k in range(K)]
    return sc


def _sc_universal(rs, K):
    """the universal state, 6,143 edges, with no_repeat_ngram_size 2: tests/test_gpu_beam_kernels.py's ban situation"""
    sc = _abase(rs, K, 3, au.universal().trans, [0], [0] * K)
    sc["hist"][0] = [START, 50, 61, 51]
    sc["hist"][1] = [START, 50, 60, 50]
    for k in range(K):
        sc["logits"][k, 60] = 5.0
        _plant(sc, k, 600 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
    sc["check"] = lambda c: (0, 60) in list(zip(c["cpar"], c["ctok"])) and (1, 60) not in list(zip(c["cpar"], c["ctok"])) and \
        bool(np.isfinite(c["cv"]).all())
    return sc


def _sc_leaf(rs, K):
    """beam 0 sits in an accepting leaf: EOS is all it may emit, although token 410 is its maximum; the others choose among three
    edges.  The EOS enters the finished set with the leaf's state"""
    trans = {6: {400: 7, 401: 8, 402: 9}}
    sc = _abase(rs, K, 2, trans, [5], [5] + [6] * (K - 1))
    sc["logits"][0, 410] = 8.0
    sc["logits"][0, EOS] = 7.0
    for k in range(1, K):
        _plant(sc, k, 400, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
        sc["logits"][k, EOS] = 9.0
    sc["check"] = lambda c: (c["cpar"][0], c["ctok"][0]) == (0, EOS) and int(np.isfinite(c["cv"]).sum()) == min(2 * K, 1 + 3 * (K - 1)) and \
        list(c["ctok"]).count(EOS) == 1
    return sc


def _sc_dead(rs, K):
    """the crop's set holds none of beam 1's edges: a dead beam.  Beam 2 (K >= 3) is DEAD already, with score -inf; beams 0 and 3
    choose between two edges inside the set"""
    trans = {1: {501: 4, 502: 5}, 2: {500: 3}}
    states = [1, 2] + [DEAD, 1][:K - 2]
    sc = _abase(rs, K, 4, trans, [], states)
    if K >= 3:
        sc["run"][2] = -np.inf
    for k in range(K):
        sc["logits"][k, 500] = 6.0
        _plant(sc, k, 501, [3.0 - 0.5 * j - 0.125 * k for j in range(2)])
    sc["mask"] = cu.mask_of([501, 502] + [int(x) for x in rs.choice(np.arange(1000, 6000), 20, replace=False)])
    n_fin = 2 * sum(1 for s in states if s == 1)
    sc["check"] = lambda c: int(np.isfinite(c["cv"]).sum()) == n_fin and all(int(x) != 500 for x in c["ctok"][:n_fin])
    return sc


def _sc_siblings(rs, K):
    """beam 0 leads by far and has three edges into three states: the first new beams all descend from it and must not share a
    state"""
    trans = {1: {600: 2, 601: 3, 602: 4}, 5: {610: 6}}
    sc = _abase(rs, K, 5, trans, [], [1] + [5] * (K - 1))
    sc["run"] = [-0.5] + [-6.0 - 0.3125 * k for k in range(1, K)]
    _plant(sc, 0, 600, [3.0, 2.5, 2.0])
    for k in range(1, K):
        sc["logits"][k, 610] = 3.0
    m = min(3, K)
    sc["check"] = lambda c: all(int(p) == 0 for p in c["cpar"][:m]) and [int(x) for x in c["ctok"][:3]] == [600, 601, 602]
    return sc


def _sc_insert(rs, K):
    """the finished set holds one entry in state 31; beam 0 is in the accepting state 32 and its EOS scores above the entry: the
    new hypothesis takes slot 0 with state 32, the old one moves to slot 1 with its ids, its log-probabilities and its state"""
    trans = {0: {700: 30}, 30: {701: 31}, 32: {710: 33}, 34: {720: 35, 721: 36}}
    sc = _abase(rs, K, 3, trans, [31, 32], [32] + [34] * (K - 1))
    sc["run"] = [-0.125 - 0.3125 * k for k in range(K)]
    sc["hyp"] = [(-2.5, [START, 700, 701, EOS])]
    sc["hyp_state"] = [31]
    sc["logits"][0, EOS] = 9.0
    sc["logits"][0, 710] = 3.0
    for k in range(1, K):
        _plant(sc, k, 720, [3.0 - 0.5 * j - 0.125 * k for j in range(2)])
    sc["check"] = lambda c: c["ctok"][0] == EOS and c["cv"][0] / 4.0 > -2.5
    return sc


def _sc_length(rs, K):
    """the step completes generate(max_length): every candidate stops, and the hypotheses keep next(state of the parent, token) -
    the last token walks"""
    trans = {10 + k: {800 + 10 * k + j: 50 + 10 * k + j for j in range(3)} for k in range(K)}
    sc = _abase(rs, K, ML - 2, trans, [], [10 + k for k in range(K)])
    for k in range(K):
        _plant(sc, k, 800 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
    sc["check"] = lambda c: bool(np.all(c["stop"]))
    return sc


AUT_SITUATIONS = [_sc_one_edge, _sc_universal, _sc_leaf, _sc_dead, _sc_siblings, _sc_insert, _sc_length]


# ------------------------------------------------------------------------------------------------ one launch
def _build(rs, scs, K, nslab):
    """the arrays of one launch: G groups of K slots and a trailing partial group of K - 1 padding slots, two crops nobody
    decodes, a guard row behind ids / hyp_ids and the two histories; the crops' automata behind each other over global state
    numbers, a universal automaton nobody uses in front (so that no crop's base is 0)"""
    G = len(scs)
    n = G * K + (K - 1)
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
    a["abase"] = np.full(R, -1, np.int32)
    a["ast"] = np.full(R + 1, SENT, np.int32)
    a["hst"] = np.full(R + 1, SENT, np.int32)
    masks = [np.ones(V, bool)]
    a["set_of_row"] = np.zeros(R, np.int32)
    auts = [au.Automaton({0: {7: 0}}, [0])] + [sc["aut"] for sc in scs if sc.get("aut") is not None]
    eb, et, en, acc, first = au.pack_many(auts)
    a.update(eb=eb, et=et, en=en, acc=acc)
    logits = rs.randint(-512, -256, (n, V)).astype(np.float64) / 64.0
    ai = 1
    glob = lambda base, s: base + s if s >= 0 else s
    for g, sc in enumerate(scs):
        c = int(crop_of[g])
        base = -1
        if sc.get("aut") is not None:
            base = first[ai]
            ai += 1
        sc["base"] = base
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
            a["abase"][r] = base
            a["ast"][r] = glob(base, sc["ast"][k]) if base >= 0 else NONE
            a["hst"][r] = NONE
            logits[s] = sc["logits"][k]
        for j, (s_, seq) in enumerate(sc["hyp"]):
            a["hyp_ids"][c * K + j, :len(seq)] = seq
            a["hyp_len"][c * K + j] = len(seq)
            a["hyp_score"][c * K + j] = s_
            a["hlogp"][c * K + j, :len(seq)] = sc["hyp_logp"][j]
            if base >= 0:
                a["hst"][c * K + j] = glob(base, sc["hyp_state"][j])
        a["hopen"][c] = 1 if sc["open"] else 0
    a["step"][G * K:] = 7
    a["bias"] = rs.randint(-128, 128, V).astype(np.float64) / 64.0
    parts = rs.randint(-128, 128, (nslab, n, V)).astype(np.float64) / 64.0
    parts[-1] = logits - a["bias"] - parts[:-1].sum(0)
    a["parts"] = parts
    a["table"] = cu.pack_sets(np.stack(masks))
    a["unf"] = np.array([1000, SENT], np.int32)
    return a


def _run(eng, dtype, a, bcfg, nslab, form):
    """form: "aut" (the seven automaton pointers set), "null" (the hook with them null), "tok" (mocr_op_beam_select_tokens)"""
    n, R = a["n"], a["R"]
    d = {k: _i32(a[k]) for k in ("ids", "step", "fin", "len", "unf", "rowmap", "parent", "hyp_ids", "hyp_len", "hopen", "ast", "hst")}
    d.update({k: _f32(a[k]) for k in ("bscore", "hyp_score", "blogp", "hlogp")})
    x32 = torch.full((n + GUARD, D), float("nan"), device="cuda")
    xt = torch.full((n + GUARD, D), float("nan"), device="cuda", dtype=torch.bfloat16 if dtype == "bf16" else torch.float32)
    cache = torch.full((R, MAX_LEN, D), float("nan"), device="cuda", dtype=xt.dtype)
    table = torch.from_numpy(a["table"].view(np.int32).copy()).cuda()
    sets = _i32(a["set_of_row"])
    tabs = [_i32(a["eb"]), _i32(a["et"]), _i32(a["en"]), torch.from_numpy(a["acc"].copy()).cuda(), _i32(a["abase"])]
    torch.cuda.synchronize()
    kw = dict(first=0, n=n, slabs=_f32(a["parts"]), nslab=nslab, vbias=_f32(a["bias"]), ids=d["ids"], step=d["step"], finished=d["fin"],
              len=d["len"], n_unfinished=d["unf"], rowmap=d["rowmap"], ids_ld=LD, max_len=ML, n_real=a["G"] * bcfg.num_beams,
              x_f32=x32, x_t=xt, cache=cache)
    state = (d["bscore"], d["parent"], d["hyp_ids"], d["hyp_len"], d["hyp_score"], d["hopen"], d["blogp"], d["hlogp"], table, sets)
    if form == "tok":
        eng.op_beam_select_tokens(bcfg, *state, **kw)
    elif form == "null":
        eng.op_beam_select_automaton(bcfg, *state, **kw)
    else:
        eng.op_beam_select_automaton(bcfg, *state, None, None, *tabs, d["ast"], d["hst"], **kw)
    got = {k: v.cpu().numpy() for k, v in d.items()}
    got["x32"], got["cache"] = x32.cpu().numpy().view(np.int32), cache.view(torch.int16 if dtype == "bf16" else torch.int32).cpu().numpy()
    got["xt"] = xt.view(torch.int16 if dtype == "bf16" else torch.int32).cpu().numpy()
    return got


def _state_of(sc, K):
    st = bau.State(K, START, sc["aut"])
    st.seqs = [list(h) for h in sc["hist"]]
    st.logp = [list(h) for h in sc["logp"]]
    st.run = np.array(sc["run"], np.float64)
    st.ast = list(sc["ast"])
    for j, (s, seq) in enumerate(sc["hyp"]):
        st.hyp_score[j], st.hyp_seq[j], st.hyp_logp[j], st.hyp_state[j] = s, list(seq), list(sc["hyp_logp"][j]), sc["hyp_state"][j]
    st.open = sc["open"]
    return st


def _check(a, got, scs, cfg, K):
    """an automaton-form launch against the float64 reference, group by group -> (largest score error, largest log-probability
    error, smallest candidate gap)"""
    R = a["R"]
    want = {k: a[k].copy() for k in ("ids", "fin", "len", "parent", "hyp_ids", "hyp_len", "hopen", "blogp", "hlogp", "ast", "hst")}
    want_hs, want_bs = a["hyp_score"].astype(np.float64), a["bscore"].astype(np.float64)
    free = np.zeros((R + 1, LD), bool)              # cells of a dead running beam: a token in [0, vocab), any log-probability
    n_unf, min_gap = 1000, np.inf
    glob = lambda base, s: base + s if s >= 0 else s
    for g, sc in enumerate(scs):
        c = int(a["crop_of"][g])
        base = sc["base"]
        st = _state_of(sc, K)
        old_ast = list(st.ast)
        cv, cpar, ctok, stop, clp, cst = bau.step(bau.processed(sc["logits"], st, cfg, sc["mask"]), st, cfg, ML, EOS)
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
            want["hst"][r] = glob(base, st.hyp_state[j]) if n_h else NONE
            assert not n_h or st.hyp_state[j] >= 0, "a finished hypothesis is never DEAD"
        want["hopen"][c] = 1 if st.open else 0
        for k in range(K):
            r = c * K + k
            if st.done:
                want["fin"][r], want["len"][r], want["parent"][r] = 1, sc["t"] + 2, k
                want_bs[r] = np.nan
            else:
                want_bs[r] = st.run[k]
                if np.isinf(st.run[k]):
                    # a dead candidate: its token is any token of the vocabulary, its parent any beam - and its state what the rule
                    # makes of the two
                    free[r, :L + 1] = True
                    assert 0 <= got["parent"][r] < K and ((got["ids"][r, :L + 1] >= 0) & (got["ids"][r, :L + 1] < V)).all()
                    want["parent"][r] = got["parent"][r]
                    want["ast"][r] = glob(base, sc["aut"].next(old_ast[int(got["parent"][r])], int(got["ids"][r, L])))
                else:
                    want["parent"][r] = st.parents[k]
                    want["ids"][r, :L + 1] = st.seqs[k]
                    want["blogp"][r, :L + 1] = st.logp[k]
                    want["ast"][r] = glob(base, st.ast[k])
        n_unf -= K if st.done else 0
    for k in ("ids", "parent", "fin", "len", "hopen", "hyp_len", "hyp_ids", "ast", "hst"):
        np.testing.assert_array_equal(np.where(free, 0, got[k]) if k == "ids" else got[k], np.where(free, 0, want[k]) if k == "ids" else want[k],
                                      err_msg=k)
    np.testing.assert_array_equal(got["unf"], [n_unf, SENT])
    np.testing.assert_array_equal(got["step"], a["step"] + 1)
    np.testing.assert_array_equal(got["rowmap"], a["rowmap"])
    live = ~np.isnan(want_bs)
    e_score = max(_close(got["hyp_score"], want_hs, "hyp_score"), _close(got["bscore"][live], want_bs[live], "beam_score"))
    e_logp = 0.0
    for name in ("blogp", "hlogp"):
        g_, w_ = got[name].astype(np.float64), want[name].astype(np.float64)
        cmp = ~free
        assert np.isfinite(g_[cmp]).all() and (g_[cmp][g_[cmp] != LSENT] <= 0).all(), f"{name}: finite and <= 0"
        err = np.abs(g_ - w_)
        e_logp = max(e_logp, float(err[cmp].max()))
        assert err[cmp].max() <= 1e-5, f"{name}: {err[cmp].max()} from float64"
        exact = cmp & (w_ * 64.0 == np.round(w_ * 64.0))
        np.testing.assert_array_equal(got[name][exact], w_[exact].astype(np.float32), err_msg=f"{name}: copied or untouched cells")
    return e_score, e_logp, min_gap


def _histories(rs, sc, K):
    sc = _with_histories(rs, sc, K)
    if np.isinf(sc["run"]).any():                   # a beam that is dead already carries a dead last token
        for k in range(K):
            if np.isinf(sc["run"][k]):
                sc["logp"][k][-1] = -np.inf
    return sc


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("nslab", [1, 3])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_automata_against_float64(K, nslab, dtype):
    from manga_ocr.engine import BeamConfig
    eng = engine(dtype)
    rs = np.random.RandomState(5000 * K + 10 * nslab + (dtype == "bf16"))
    cfg, bcfg = bu.Config(K, 1.0, False, 2), BeamConfig(K, 1.0, False, 2)
    seen, worst, min_gap = set(), [0.0, 0.0], np.inf
    for first in range(0, len(AUT_SITUATIONS), 3):
        idx = [(first + g) % len(AUT_SITUATIONS) for g in range(3)]
        scs = [_histories(rs, AUT_SITUATIONS[i](rs, K), K) for i in idx]
        seen.update(idx)
        a = _build(rs, scs, K, nslab)
        got = _run(eng, dtype, a, bcfg, nslab, "aut")
        e_score, e_logp, gap = _check(a, got, scs, cfg, K)
        worst, min_gap = [max(worst[0], e_score), max(worst[1], e_logp)], min(min_gap, gap)
    assert seen == set(range(len(AUT_SITUATIONS)))
    report(f"beam_select_automaton {dtype} K={K} nslab={nslab}: 7 situations under automata exact, states included; log-probability "
           f"histories {worst[1]:.2e} from float64 (bound 1e-5), scores {worst[0]:.2e}; closest candidates {min_gap:.2e}")


BITS = ("ids", "step", "fin", "len", "unf", "rowmap", "parent", "hyp_ids", "hyp_len", "hopen", "x32", "xt", "cache")


def _same(x, y, what, keys=BITS):
    for k in keys:
        np.testing.assert_array_equal(x[k], y[k], err_msg=f"{k}: {what}")
    for k in ("bscore", "hyp_score", "blogp", "hlogp"):
        np.testing.assert_array_equal(x[k].view(np.int32), y[k].view(np.int32), err_msg=f"{k}, bit for bit: {what}")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_the_reductions_are_bit_identical_to_the_token_form(K, dtype):
    """the token test's seven situations under token sets: with null automaton pointers the hook is the token form; with every
    crop under the universal automaton it is too, down to the states it leaves (the one universal state, NONE in empty slots);
    and with the set given as a one-state automaton instead of through ``sets`` as well"""
    from manga_ocr.engine import BeamConfig
    eng = engine(dtype)
    nslab = 3
    rs = np.random.RandomState(7000 * K + (dtype == "bf16"))
    bcfg = BeamConfig(K, 1.0, False, 2)
    for first in range(0, len(NEW_SITUATIONS), 3):
        scs = [_with_histories(rs, NEW_SITUATIONS[(first + g) % len(NEW_SITUATIONS)](rs, K), K) for g in range(3)]
        a = _build(rs, scs, K, nslab)
        tok = _run(eng, dtype, a, bcfg, nslab, "tok")
        _same(_run(eng, dtype, a, bcfg, nslab, "null"), tok, "null automaton pointers against the token form", BITS + ("ast", "hst"))
        # every crop under the universal automaton, its set still through `sets`
        u = dict(a)
        eb, et, en, acc, first_state = au.pack_many([au.Automaton({0: {7: 0}}, [0]), au.universal()])
        u.update(eb=eb, et=et, en=en, acc=acc, abase=a["abase"].copy(), ast=a["ast"].copy(), hst=a["hst"].copy())
        live = np.concatenate([np.arange(int(c) * K, int(c) * K + K) for c in a["crop_of"]])
        u["abase"][live], u["ast"][live], u["hst"][live] = first_state[1], first_state[1], NONE
        for g, sc in enumerate(scs):
            c = int(a["crop_of"][g])
            u["hst"][c * K:c * K + len(sc["hyp"])] = first_state[1]
        got = _run(eng, dtype, u, bcfg, nslab, "aut")
        _same(got, tok, "the universal automaton against the token form")
        for g, sc in enumerate(scs):
            c = int(a["crop_of"][g])
            rows = np.arange(c * K, c * K + K)
            np.testing.assert_array_equal(got["hst"][rows], np.where(got["hyp_len"][rows] > 0, first_state[1], NONE))
            if not sc["finished"] and not got["fin"][rows[0]]:
                alive = np.isfinite(got["bscore"][rows]) & (got["ids"][rows, sc["t"] + 1] != EOS)
                np.testing.assert_array_equal(got["ast"][rows][alive], first_state[1])
        # every crop's set as a one-state automaton of its own, and set 0 through `sets`
        auts = [au.Automaton({0: {7: 0}}, [0])] + [bau.set_automaton(sc["mask"] if sc["mask"] is not None else np.ones(V, bool)) for sc in scs]
        eb, et, en, acc, first_state = au.pack_many(auts)
        s = dict(a)
        s.update(eb=eb, et=et, en=en, acc=acc, abase=a["abase"].copy(), ast=a["ast"].copy(), hst=a["hst"].copy(),
                 set_of_row=np.zeros_like(a["set_of_row"]))
        for g, sc in enumerate(scs):
            c = int(a["crop_of"][g])
            rows = np.arange(c * K, c * K + K)
            s["abase"][rows], s["ast"][rows], s["hst"][rows] = first_state[1 + g], first_state[1 + g], NONE
        _same(_run(eng, dtype, s, bcfg, nslab, "aut"), tok, "a token set as a one-state automaton against the set through `sets`")
    report(f"beam_select_automaton {dtype} K={K}: null pointers, the universal automaton and one-state set automata bit-identical "
           f"to beam_select_tokens on its 7 situations")
