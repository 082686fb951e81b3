"""-m gpu: the SOFT form of beam_select_kernel through its operator hook (mocr_op_beam_select_soft) against
tests/beam_soft_util.py in float64, on hand-built logits rows (multiples of 1/64: the slab sums are exact in fp32; weights
multiples of 1/8), as tests/test_gpu_beam_automaton_kernels.py tests the automaton form, whose launch layout (three crop groups,
a trailing partial group, crops nobody decodes, guard rows) it uses.

* Ten situations under soft automata - a weight that lifts a non-maximal token into the 2 K, a negative weight that drops a
  beam's maximum out of them, a weight on a token the crop's set masks (it stays -inf), an open state that does not accept
  (EOS, the row's maximum, is masked) beside one that does, a miss that takes the default edge, a miss under
  MOCR_DEFAULT_FALLBACK that lands on the default state's edge target, a closed state beside open ones in one group, a state
  with 6,143 weighted edges (every float4 of every thread adds), the stop by length, a hypothesis inserted above an old one
  (the states shift): tokens, parents, both histories, the beams' and the hypotheses' states, the finished set and every flag
  exact; K = 2, 3, 4, fp32 and bf16 storage, 1 and 3 slabs.
* With the two soft arrays null the hook IS mocr_op_beam_select_automaton, and with all-zero weights and no default edge it
  is bit-identical to it, on that test's seven situations.

* The next step's inputs of the SOFT instantiations: x of every new beam's slot and the layer-0 cache row at position t + 1 are
  the embedding of the reference's new token (tests/test_gpu_beam_kernels.py's check), and nothing else is written.

BOUNDS.  Integers exact.  Token scores: "exact" against a float64 reference is not attainable for an fp32 value that holds a
logf; what is exact is every copied cell (histories are multiples of 1/64 and compared bit for bit), and a NEW token score
s = ((v - gmax) - logS) + w is held to TOKEN_TOL = 4e-6 with |s| < 16 asserted: v - gmax is exact here, logS <= log 6144 < 9
carries the exp sum's relative error (about 2e-7, 1.4e-6 at most with logf's ulp of 9.5e-7), and the subtraction and the add of
w each round once at a magnitude below 16, 9.5e-7 each - 3.3e-6 in all.  (1e-5 is the automaton kernel test's bound; this one is
tighter because the weight add is what is new.)  Sequence scores and running scores: 1e-5 absolute as there (a score is a sum or
a quotient of several such values), 1e-7 relative on the -1e9 ones.  Embeddings: 1e-5 of the row scale, the storage rounding
and the cache row bit for bit.  The reference's candidates are at least 1e-3 apart by construction.  A token score may be
positive here: it holds the weight."""
import numpy as np
import pytest

import automaton_util as au
import beam_soft_util as bsu
import beam_util as bu
import bias_util
import constraint_util as cu
from gpu_util import bf16_round, engine, report, weights
from test_gpu_beam_automaton_kernels import AUT_SITUATIONS, BITS, _build, _histories, _same, _state_of
from test_gpu_beam_kernels import D, EOS, GUARD, LD, MAX_LEN, ML, PAD, SENT, START, V, _base, _emb_ref, _f32, _i32, _plant
from test_gpu_beam_token_kernels import LSENT, _close, _planted

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NONE = au.NONE
TOKEN_TOL = 4e-6                    # a new token score against float64 (the module's docstring)


def _sbase(rs, K, t, trans, accepting, states, weights=None, default=None, fallback=False, n_states=None):
    sc = _base(rs, K, t)
    sc.update(aut=bias_util.SoftAutomaton(trans, accepting, weights, default, n_states, fallback), ast=list(states), hyp_state=[], mask=None)
    return sc


def _pairs(c):
    return [(int(p), int(x)) for p, x in zip(c["cpar"], c["ctok"])]


# ------------------------------------------------------------------------------------------------ the ten situations
def _sc_lift(rs, K):
    """beam 0 is in a state with an edge on token 5350 (the last of a thread's six float4s), weight + 6: its logit, - 1, is below
    the three planted ones, and the weight makes it the crop's best candidate; the other beams, in a state without that edge, do
    not see it"""
    sc = _sbase(rs, K, 3, {1: {5350: 2}}, [0, 1, 2], [1] + [0] * (K - 1), {1: {5350: 6.0}}, 0)
    for k in range(K):
        _plant(sc, k, 200 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
        sc["logits"][k, 5350] = -1.0
    sc["check"] = lambda c: _pairs(c)[0] == (0, 5350) and all((k, 5350) not in _pairs(c) for k in range(1, K)) and c["cst"][0] == 2
    return sc


def _sc_drop(rs, K):
    """a weight of - 4.5 on beam 0's maximum: it leaves the 2 K, the beam's second token leads it"""
    sc = _sbase(rs, K, 2, {1: {200: 2, 201: 3}}, [0, 1], [1] + [0] * (K - 1), {1: {200: -4.5}}, 0)
    for k in range(K):
        _plant(sc, k, 200 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
    sc["check"] = lambda c: (0, 200) not in _pairs(c) and (0, 201) in _pairs(c) and bool(np.isfinite(c["cv"]).all())
    return sc


def _sc_masked_weight(rs, K):
    """a weight of + 8 on a token the crop's set does not hold: it stays -inf, for every beam"""
    sc = _sbase(rs, K, 4, {0: {360: 1, 200: 1}}, [0, 1], [0] * K, {0: {360: 8.0, 200: 0.25}}, 0)
    for k in range(K):
        _plant(sc, k, 200 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
        sc["logits"][k, 360] = 2.0
    sc["mask"] = cu.mask_of(_planted(200, K) + [int(x) for x in rs.choice(np.arange(1000, 6000), 20, replace=False)])
    sc["check"] = lambda c: 360 not in [int(x) for x in c["ctok"]] and bool(np.isfinite(c["cv"]).all()) and (0, 200) in _pairs(c)
    return sc


def _sc_open_eos(rs, K):
    """EOS is every row's maximum.  The beams are in an OPEN state that does not accept - EOS is masked - but the last one, whose
    open state accepts: its EOS is the best candidate and the only EOS"""
    sc = _sbase(rs, K, 3, {}, [2], [1] * (K - 1) + [2], None, {1: 1, 2: 1}, n_states=3)
    for k in range(K):
        sc["logits"][k, EOS] = 9.0
        _plant(sc, k, 400 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
    sc["check"] = lambda c: _pairs(c)[0] == (K - 1, EOS) and [int(x) for x in c["ctok"]].count(EOS) == 1
    return sc


def _sc_default(rs, K):
    """state 1 has one edge (3370 -> 2, weighted, in the fourth float4) and a default edge to 3: beam 0's best token takes the edge, every other candidate is a
    miss and goes to 3"""
    sc = _sbase(rs, K, 5, {1: {3370: 2}}, [1, 2, 3], [1] * K, {1: {3370: 0.5}}, {1: 3, 2: 3, 3: 3})
    for k in range(K):
        _plant(sc, k, 500 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
    sc["logits"][0, 3370] = 4.0
    sc["check"] = lambda c: _pairs(c)[0] == (0, 3370) and c["cst"][0] == 2 and all(s == 3 for s in c["cst"][1:])
    return sc


def _sc_fallback(rs, K):
    """MOCR_DEFAULT_FALLBACK: state 1 has an edge on 601 only; 600 is a miss that the default state 0 has an edge on (-> 5), 602 a
    miss everywhere (-> 0)"""
    sc = _sbase(rs, K, 2, {0: {600: 5, 610: 6}, 1: {601: 7}}, [0, 1, 5, 6, 7], [1] * K, {1: {601: 0.25}}, 0, fallback=True, n_states=8)
    for k in range(K):
        _plant(sc, k, 600 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
    sc["run"] = [-0.5] + [-6.0 - 0.3125 * k for k in range(1, K)]
    sc["check"] = lambda c: _pairs(c)[:3] == [(0, 600), (0, 601), (0, 602)] and list(c["cst"][:3]) == [5, 7, 0]
    return sc


def _sc_closed_and_open(rs, K):
    """beam 0 is in a CLOSED state with two edges, one weighted (its row's maximum, token 60, has no edge and is masked); the
    others are in an open state and may emit 60"""
    sc = _sbase(rs, K, 4, {4: {1700: 5, 1701: 6}}, [1], [4] + [1] * (K - 1), {4: {1701: 1.0}}, {1: 1}, n_states=7)
    for k in range(K):
        sc["logits"][k, 60] = 5.0 - 0.125 * k
        if k:
            _plant(sc, k, 740 + 10 * k, [2.0 - 0.5 * j - 0.0625 * k for j in range(3)])
    _plant(sc, 0, 1700, [3.0, 2.5])
    sc["check"] = lambda c: (0, 60) not in _pairs(c) and all((k, 60) in _pairs(c) for k in range(1, K)) and \
        (0, 1701) in _pairs(c) and (0, 1700) in _pairs(c) and _pairs(c).index((0, 1701)) < _pairs(c).index((0, 1700))
    return sc


def _sc_many(rs, K):
    """the universal state with a weight on every one of its 6,143 edges (multiples of 1/8 in [-1, 1], some of them 0); beam k's
    candidates lie in float4 k + 2 of the threads that hold them (columns 2800 + 1024 k ...)"""
    trans = au.universal().trans
    weights = {0: {t: ((t * 37) % 17 - 8) / 8.0 for t in trans[0]}}
    sc = _sbase(rs, K, 3, trans, [0], [0] * K, weights, None)
    for k in range(K):
        _plant(sc, k, 2800 + 1024 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
    sc["check"] = lambda c: bool(np.isfinite(c["cv"]).all()) and {int(x) // 1024 for x in c["ctok"]} == {k + 2 for k in range(K)}
    return sc


def _sc_length(rs, K):
    """the step completes generate(max_length): every candidate stops, and the hypotheses keep next(state of the parent, token) -
    an edge's target or the default state"""
    trans = {10 + k: {900 + 10 * k: 50 + k} for k in range(K)}
    sc = _sbase(rs, K, ML - 2, trans, list(range(60)), [10 + k for k in range(K)], {10 + k: {900 + 10 * k: 0.75} for k in range(K)}, 40,
                n_states=60)
    for k in range(K):
        _plant(sc, k, 900 + 10 * k, [3.0 - 0.5 * j - 0.125 * k for j in range(3)])
    sc["check"] = lambda c: bool(np.all(c["stop"])) and 40 in c["cst"] and 50 in c["cst"]
    return sc


def _sc_insert(rs, K):
    """the finished set holds one entry in state 31; beam 0 is in the accepting open state 32 and its EOS scores above the entry:
    the new hypothesis takes slot 0 with state 32, the old one moves to slot 1 with its ids, its token scores and its state"""
    trans = {0: {700: 30}, 30: {701: 31}, 32: {710: 33}}
    sc = _sbase(rs, K, 3, trans, [31, 32], [32] + [34] * (K - 1), {32: {710: 0.5}}, {32: 0, 34: 0, 0: 0}, n_states=35)
    sc["run"] = [-0.125 - 0.3125 * k for k in range(K)]
    sc["hyp"] = [(-2.5, [START, 700, 701, EOS])]
    sc["hyp_state"] = [31]
    sc["logits"][0, EOS] = 9.0
    sc["logits"][0, 710] = 3.0
    for k in range(1, K):
        _plant(sc, k, 720, [3.0 - 0.5 * j - 0.125 * k for j in range(2)])
    sc["check"] = lambda c: c["ctok"][0] == EOS and c["cv"][0] / 4.0 > -2.5
    return sc


SOFT_SITUATIONS = [_sc_lift, _sc_drop, _sc_masked_weight, _sc_open_eos, _sc_default, _sc_fallback, _sc_closed_and_open, _sc_many,
                   _sc_length, _sc_insert]


# ------------------------------------------------------------------------------------------------ one launch
def _soft_tables(a, scs):
    """the two soft arrays of a launch that tests/test_gpu_beam_automaton_kernels.py ``_build`` laid out: the same automata in the
    same order, so the same global numbers"""
    auts = [au.Automaton({0: {7: 0}}, [0])] + [sc["aut"] for sc in scs if sc.get("aut") is not None]
    eb, et, en, acc, w, d, _ = bias_util.pack_many(auts)
    for k, v in (("eb", eb), ("et", et), ("en", en)):
        np.testing.assert_array_equal(a[k], v)
    a["ew"], a["dn"] = w, d
    return a


def _run(eng, dtype, a, bcfg, nslab, form):
    """form: "soft" (all nine pointers), "zero" (all-zero weights, no default edges), "null" (the soft hook with the two soft
    arrays null), "half" (the weights without the default edges: refused), "aut" (mocr_op_beam_select_automaton)"""
    n, R = a["n"], a["R"]
    d = {k: _i32(a[k]) for k in ("ids", "step", "fin", "len", "unf", "rowmap", "parent", "hyp_ids", "hyp_len", "hopen", "ast", "hst")}
    d.update({k: _f32(a[k]) for k in ("bscore", "hyp_score", "blogp", "hlogp")})
    x32 = torch.full((n + GUARD, D), float("nan"), device="cuda")
    xt = torch.full((n + GUARD, D), float("nan"), device="cuda", dtype=torch.bfloat16 if dtype == "bf16" else torch.float32)
    cache = torch.full((R, MAX_LEN, D), float("nan"), device="cuda", dtype=xt.dtype)
    table = torch.from_numpy(a["table"].view(np.int32).copy()).cuda()
    sets = _i32(a["set_of_row"])
    tabs = [_i32(a["eb"]), _i32(a["et"]), _i32(a["en"]), torch.from_numpy(a["acc"].copy()).cuda(), _i32(a["abase"])]
    if form == "soft":
        soft = (_f32(a["ew"]), _i32(a["dn"]))
    elif form == "zero":
        soft = (_f32(np.zeros(len(a["et"]), np.float32)), _i32(np.full(len(a["acc"]), -1, np.int32)))
    elif form == "half":
        soft = (_f32(a["ew"]), None)
    else:
        soft = (None, None)
    torch.cuda.synchronize()
    kw = dict(first=0, n=n, slabs=_f32(a["parts"]), nslab=nslab, vbias=_f32(a["bias"]), ids=d["ids"], step=d["step"], finished=d["fin"],
              len=d["len"], n_unfinished=d["unf"], rowmap=d["rowmap"], ids_ld=LD, max_len=ML, n_real=a["G"] * bcfg.num_beams,
              x_f32=x32, x_t=xt, cache=cache)
    state = (d["bscore"], d["parent"], d["hyp_ids"], d["hyp_len"], d["hyp_score"], d["hopen"], d["blogp"], d["hlogp"], table, sets)
    if form == "aut":
        eng.op_beam_select_automaton(bcfg, *state, None, None, *tabs, d["ast"], d["hst"], **kw)
    else:
        eng.op_beam_select_soft(bcfg, *state, None, None, *tabs, d["ast"], d["hst"], *soft, **kw)
    got = {k: v.cpu().numpy() for k, v in d.items()}
    got["x32"], got["cache"] = x32.cpu().numpy().view(np.int32), cache.view(torch.int16 if dtype == "bf16" else torch.int32).cpu().numpy()
    got["xt"] = xt.view(torch.int16 if dtype == "bf16" else torch.int32).cpu().numpy()
    got["x32f"], got["xtf"], got["cachef"] = x32.cpu().numpy().astype(np.float64), xt.float().cpu().numpy().astype(np.float64), cache.float().cpu().numpy()
    return got


def reference(scs, cfg, K):
    """the float64 step of every situation -> per situation (its State after the step, its states before, cv, cpar, ctok, stop,
    clp, cst); asserts that the situation is what it says and that its candidates are 1e-3 apart"""
    out = []
    for g, sc in enumerate(scs):
        st = _state_of(sc, K)
        old_ast = list(st.ast)
        cv, cpar, ctok, stop, clp, cst = bsu.step(bsu.processed(sc["logits"], st, cfg, sc["mask"]), st, cfg, ML, EOS)
        assert sc["check"](dict(cv=cv, cpar=cpar, ctok=ctok, stop=stop, cst=list(cst))), f"situation {g} is not what it says"
        assert st.min_gap >= 1e-3, f"a constructed case has candidates {st.min_gap} apart"
        out.append((st, old_ast))
    return out


def _check(a, got, scs, cfg, K, dtype):
    """a soft-form launch against the float64 reference, group by group -> (largest score error, largest token-score error,
    smallest candidate gap, largest embedding error)"""
    R = a["R"]
    emb = {}                                        # slot -> (row, token, position) of every new running beam
    want = {k: a[k].copy() for k in ("ids", "fin", "len", "parent", "hyp_ids", "hyp_len", "hopen", "blogp", "hlogp", "ast", "hst")}
    want_hs, want_bs = a["hyp_score"].astype(np.float64), a["bscore"].astype(np.float64)
    free = np.zeros((R + 1, LD), bool)              # cells of a dead running beam: a token in [0, vocab), any token score
    n_unf, min_gap = 1000, np.inf
    glob = lambda base, s: base + s if s >= 0 else s
    for g, (sc, (st, old_ast)) in enumerate(zip(scs, reference(scs, cfg, K))):
        c = int(a["crop_of"][g])
        base = sc["base"]
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
                    free[r, :L + 1] = True
                    assert 0 <= got["parent"][r] < K and ((got["ids"][r, :L + 1] >= 0) & (got["ids"][r, :L + 1] < V)).all()
                    want["parent"][r] = got["parent"][r]
                    want["ast"][r] = glob(base, sc["aut"].next(old_ast[int(got["parent"][r])], int(got["ids"][r, L])))
                    emb[g * K + k] = (r, int(got["ids"][r, L]), L)
                else:
                    emb[g * K + k] = (r, st.seqs[k][-1], L)
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
        assert np.isfinite(g_[cmp]).all(), f"{name}: finite"
        err = np.abs(g_ - w_)
        e_logp = max(e_logp, float(err[cmp].max()))
        assert err[cmp].max() <= TOKEN_TOL and np.abs(w_[cmp & (w_ != LSENT)]).max() < 16.0, f"{name}: {err[cmp].max()} from float64"
        exact = cmp & (w_ * 64.0 == np.round(w_ * 64.0))
        np.testing.assert_array_equal(got[name][exact], w_[exact].astype(np.float32), err_msg=f"{name}: copied or untouched cells")
    # the next inputs: x by slot, the layer-0 cache by row at position t + 1; nothing else
    w, e_emb = weights(), 0.0
    g32, gt, gc = got["x32f"], got["xtf"], got["cachef"]
    written = np.zeros(gc.shape[:2], bool)
    for s in range(g32.shape[0]):
        if s not in emb:
            assert np.isnan(g32[s]).all() and np.isnan(gt[s]).all(), f"x of slot {s} written (ended crop, padding or guard)"
            continue
        r, tok, p = emb[s]
        ref = _emb_ref(w, tok, p)
        err = float((np.abs(g32[s] - ref) / np.abs(ref).max()).max())
        e_emb = max(e_emb, err)
        assert err <= 1e-5, f"embedding of slot {s}: {err} of the row scale"
        stored = bf16_round(g32[s].astype(np.float32)).astype(np.float64) if dtype == "bf16" else g32[s].astype(np.float32).astype(np.float64)
        np.testing.assert_array_equal(gt[s], stored, err_msg="x_t != storage rounding of x_f32")
        np.testing.assert_array_equal(gc[r, p].astype(np.float64), gt[s], err_msg="cache row != x_t")
        written[r, p] = True
    assert np.isnan(gc[~written]).all(), "cache written outside the new beams' rows at position t + 1"
    return e_score, e_logp, min_gap, e_emb


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("nslab", [1, 3])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_soft_automata_against_float64(K, nslab, dtype):
    from manga_ocr.engine import BeamConfig
    eng = engine(dtype)
    rs = np.random.RandomState(9000 * K + 10 * nslab + (dtype == "bf16"))
    cfg, bcfg = bu.Config(K, 1.0, False, 2), BeamConfig(K, 1.0, False, 2)
    seen, worst, min_gap = set(), [0.0, 0.0, 0.0], np.inf
    for first in range(0, len(SOFT_SITUATIONS), 3):
        idx = [(first + g) % len(SOFT_SITUATIONS) for g in range(3)]
        scs = [_histories(rs, SOFT_SITUATIONS[i](rs, K), K) for i in idx]
        seen.update(idx)
        a = _soft_tables(_build(rs, scs, K, nslab), scs)
        got = _run(eng, dtype, a, bcfg, nslab, "soft")
        e_score, e_logp, gap, e_emb = _check(a, got, scs, cfg, K, dtype)
        worst, min_gap = [max(worst[0], e_score), max(worst[1], e_logp), max(worst[2], e_emb)], min(min_gap, gap)
    assert seen == set(range(len(SOFT_SITUATIONS)))
    report(f"beam_select_soft {dtype} K={K} nslab={nslab}: {len(SOFT_SITUATIONS)} situations under soft automata exact, states included; "
           f"token scores {worst[1]:.2e} from float64 (bound {TOKEN_TOL:.0e}), scores {worst[0]:.2e}, embedding {worst[2]:.2e} of the row scale; "
           f"closest candidates {min_gap:.2e}")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_null_arrays_and_zero_weights_are_the_automaton_form(K, dtype):
    """the automaton test's seven situations: with the two soft arrays null the hook is mocr_op_beam_select_automaton, and the
    SOFT kernel on all-zero weights and no default edge leaves the same bits, the states included"""
    from manga_ocr.engine import BeamConfig
    eng = engine(dtype)
    nslab = 3
    rs = np.random.RandomState(11000 * K + (dtype == "bf16"))
    bcfg = BeamConfig(K, 1.0, False, 2)
    for first in range(0, len(AUT_SITUATIONS), 3):
        scs = [_histories(rs, AUT_SITUATIONS[(first + g) % len(AUT_SITUATIONS)](rs, K), K) for g in range(3)]
        a = _build(rs, scs, K, nslab)
        aut = _run(eng, dtype, a, bcfg, nslab, "aut")
        _same(_run(eng, dtype, a, bcfg, nslab, "null"), aut, "null soft arrays against the automaton form", BITS + ("ast", "hst"))
        _same(_run(eng, dtype, a, bcfg, nslab, "zero"), aut, "zero weights on hard automata against the automaton form", BITS + ("ast", "hst"))
    report(f"beam_select_soft {dtype} K={K}: null soft arrays and all-zero weights bit-identical to beam_select_automaton on its 7 situations")


def test_the_soft_arrays_come_as_a_pair():
    from manga_ocr._capi import MocrError
    from manga_ocr.engine import BeamConfig
    eng = engine("fp32")
    K, nslab = 2, 1
    rs = np.random.RandomState(77)
    scs = [_histories(rs, _sc_lift(rs, K), K) for _ in range(3)]
    a = _soft_tables(_build(rs, scs, K, nslab), scs)
    with pytest.raises(MocrError):
        _run(eng, "fp32", a, BeamConfig(K, 1.0, False, 2), nslab, "half")
