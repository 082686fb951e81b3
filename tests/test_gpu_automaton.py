"""-m gpu: greedy decoding under token automata - lexicons (tries) and patterns whose allowed set depends on what the row has
emitted (include/mocr.h, "token automata").

Bottom up: the start-of-batch kernel (mocr_op_automaton_init) and the AUTOMATON token kernel (mocr_op_dec_token_automaton)
against numpy, exactly (ids, states and mask words); whole recognitions against the reference loop on the fp32 oracle
(automaton_util.automaton_generate: the masked greedy loop with every row's state walked through a dictionary of
dictionaries); the bf16 decode paths under an exact path property and the first-divergence rule; a loop with bans and a token
set; compaction; shared encodings; graphs, memory and the argument errors; the ABI twins; the Python surface.

Tolerances are those of tests/test_gpu_ngram.py (named where used); the bf16 gap bound is imported."""
import ctypes as C

import numpy as np
import pytest

from gpu_util import crops, report

import automaton_util as au
import constraint_util as cu
import ngram_util as nu
import score_util as su
from manga_ocr import _capi
from test_gpu_bf16_parity import BF16_GAP_TOL
from test_gpu_constraints import FP32_LOGIT_TOL, _bits, _f32, _i32, _u32, lex_top
from test_gpu_ngram import BF16_CASES, _unpack

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

D, V, K4, EOS, START = 768, 6144, 4, 3, 2
MW = V // 32
NO_IDX = cu.NO_IDX
GUARD = 2
FILL = 4000                  # the unwritten tail of an ids row in the kernel test (see tests/test_gpu_ngram.py)
SENT = -777
NONE, DEAD = au.NONE, au.DEAD


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _words(alphabet, seed: int, count: int = 120):
    """`count` random words of 2 to 8 tokens of the alphabet"""
    rs = np.random.RandomState(seed)
    return [[int(t) for t in np.asarray(alphabet)[rs.randint(0, len(alphabet), size=rs.randint(2, 9))]] for _ in range(count)]


# ------------------------------------------------------------------------------------------------ 1. the kernels, exact
K_ALPHA = list(range(1000, 1010))
K_LOOP = [100, 101, 102, 103]


def _kernel_automata():
    """the automata of the kernel tests behind each other, as the engine's arena holds them: a trie of ~400 states, the digit
    loop (two or more of four tokens), the universal automaton, and a chain 200 -> 201 whose second token base set 1 lacks"""
    words = _words(K_ALPHA, 7)
    trie, _ = au.trie(words)
    chain = au.Automaton({0: {200: 1}, 1: {201: 2}}, [2], 3)
    auts = [trie, au.loop(K_LOOP), au.universal(), chain]
    assert 300 <= trie.n_states <= 600 and len(auts[2].trans[0]) == V - 1
    return auts, words, au.pack_many(auts)


def test_automaton_init_kernel_exact():
    """mocr_op_automaton_init, 8 rows and a junk-filled guard row behind them (masks and states), which must not be written:
    rows under the trie, the loop and the universal automaton, with both base sets; a row without an automaton (n = 0 and
    n = 1: what mocr_op_ngram_init gives); a row with n = 1 under the universal automaton (the start token banned); a row
    whose base set is disjoint from the start state's edges ({EOS} by the dead-end rule).  Masks and states exact."""
    eng = su.score_engine("wide", "fp32")
    auts, words, (eb, et, en, acc, first) = _kernel_automata()
    R = 8
    base2 = np.ones((2, V), bool)
    base2[1] = np.random.RandomState(3).rand(V) < 0.5
    base2[1, [START, EOS]] = True
    base2[1, K_LOOP] = False                                # disjoint from the loop's start state
    base2[1, 200] = True
    which = [0, 1, 2, None, 1, 2, None, 3]                  # the automaton of every row
    sor = np.array([0, 0, 1, 1, 1, 0, 0, 1], np.int32)
    ngr = np.array([0, 2, 0, 0, 0, 1, 1, 3], np.int32)
    abase = np.array([-1 if k is None else first[k] for k in which] + [first[0]], np.int32)
    junk = np.random.RandomState(4).randint(0, 2 ** 32, size=(R + 1, MW), dtype=np.uint64).astype(np.uint32)
    d_rm, d_state = _u32(junk), _i32(np.full(R + 1, SENT))
    torch.cuda.synchronize()
    eng.op_automaton_init(d_rm, _u32(cu.pack_sets(base2)), _i32(sor), _i32(ngr), R, _i32(eb), _i32(et), _u8(acc), _i32(abase), d_state)
    got, state = d_rm.cpu().numpy().view(np.uint32), d_state.cpu().numpy()
    want = np.stack([au.step_mask(None if k is None else auts[k], 0, [START], int(ngr[r]), base2[sor[r]]) for r, k in enumerate(which)])
    np.testing.assert_array_equal(got[:R], cu.pack_sets(want))
    np.testing.assert_array_equal(got[R], junk[R], err_msg="the mask row behind the batch was written")
    np.testing.assert_array_equal(state, [NONE if k is None else first[k] for k in which] + [SENT])
    # what the table proves, so that it cannot rot
    assert want[4].sum() == 1 and want[4, EOS], "row 4: the loop under a set without its tokens -> {EOS}"
    assert want[5].sum() == V - 1 and not want[5, START], "row 5: universal, n = 1 -> everything but the start token"
    assert want[2].sum() == base2[1].sum() and want[3].sum() == base2[1].sum() and want[6].sum() == V - 1
    assert want[7].sum() == 1 and want[7, 200] and want[0].sum() == len(auts[0].trans[0]) and not want[0, EOS]


def _kernel_case():
    auts, words, packed = _kernel_automata()
    trie = auts[0]
    long_word = max(words, key=len)
    assert len(long_word) >= 7
    other = next(w for w in words if w[0] != long_word[0])
    inner, longer = next((w, v) for w in words for v in words if len(v) > len(w) and v[:len(w)] == w)     # an entry that is a prefix of another
    # slot -> (row, automaton, n, base set, the row's tokens so far, finished, prefix)
    slots = [
        (5, 0, 0, 0, [START] + long_word[:2], False, None),          # the trie, two tokens in
        (2, 1, 0, 0, [START, 100], False, None),                     # the digit loop: EOS only from the third state on
        (7, 2, 0, 0, [START, 50], False, None),                      # universal
        (0, None, 0, 1, [START, 20], False, None),                   # no automaton, n = 0: the mask is left alone
        (9, 3, 0, 1, [START], False, None),                          # 200, then base set 1 lacks 201: a dead end by token set
        (1, 1, 2, 0, [START, 100, 101, 100], False, None),           # the loop with n = 2: 101 is banned behind the second 100
        (3, 0, 0, 0, [START], False, [other[0], 4000]),              # forced: a token with an edge, then one without -> DEAD, {EOS}
        (8, 1, 0, 0, [START, 100, EOS, 0], True, None),              # finished: mask and state are left alone
        (6, 0, 0, 0, [START] + inner, False, None),                  # the trie at an accepting inner node: EOS and the edges are allowed
    ]
    # the tokens with the four largest logits of every slot, largest first, for the three consecutive steps
    w = long_word
    top = [
        ([4001, w[2], 4002, 4003], [4004, w[3], 4001, 4002], [4001, 4002, w[4], 4003]),
        ([4001, 101, EOS, 102], [4001, 103, EOS, 100], [EOS, 100, 101, 102]),
        ([60, 61, 62, 63], [EOS + 1, 61, 62, 63], [70, 71, 72, 73]),
        ([21, 22, 23, 24], [22, 23, 24, 25], [99, 22, 23, 24]),
        ([4001, 201, 200, 5], [200, 201, 5, 6], [200, 201, 5, 6]),
        ([101, 102, 100, 103], [4001, 100, 101, 102], [101, 102, 103, EOS]),
        ([other[0], 4001, 4002, 4003], [4001, 4002, 4003, 4004], [4001, 4002, 4003, 4004]),
        ([100, 101, 102, 103], [100, 101, 102, 103], [100, 101, 102, 103]),
        ([longer[len(inner)], EOS, 4001, 4002], [EOS, 4001, 4002, 4003], [EOS, 4001, 4002, 4003]),   # passes the entry, then stops where it may
    ]
    return auts, packed, slots, top


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("path", ["cand64", "cand128", "slabs1", "slabs3"])
def test_automaton_token_step_exact(dtype, path):
    """mocr_op_dec_token_automaton, three consecutive steps (each on the one before's outputs), alternatives form (with the
    forced prefixes) and ids form (without: the prefix belongs to the scored kernels), candidate and slab path.  9 slots over
    10 rows through a permuted rowmap, ids_ld 16, a different step per slot: the rows of _kernel_case.  Expected, exactly,
    from numpy (automaton_util): the emitted id = the argmax over the row's effective set (or the forced token); the row's
    state walked by every stored non-EOS token, DEAD where it has no edge; row_mask[row] = the automaton's set of the new state
    AND the base set minus the bans, {EOS} if empty, for every row still unfinished; a row without an automaton and n = 0, a
    finished row, the rows no slot decodes and the guard row: mask words and state untouched."""
    eng = su.score_engine("wide", dtype)
    auts, (eb, et, en, acc, first), slots, top = _kernel_case()
    n, R, ids_ld, max_len = len(slots), 10, 16, 16
    rowmap = np.array([s[0] for s in slots], np.int32)
    base2 = np.ones((2, V), bool)
    base2[1, [21, 99, 201, 3000]] = False
    aut_of_row, ngr, bsor = [None] * (R + 1), np.zeros(R + 1, np.int32), np.zeros(R + 1, np.int32)
    ids = np.full((R + 1, ids_ld), FILL, np.int32)
    step, finished, lens = np.zeros(n, np.int32), np.zeros(R + 1, np.int32), np.full(R + 1, max_len, np.int32)
    ld = 4
    prefix, plen = np.zeros((R + 1, ld), np.int32), np.zeros(R + 1, np.int32)
    rel = np.full(R + 1, SENT, np.int64)                     # every row's state in its automaton's numbering
    for s, (row, k, g, bs, hist, fin, pre) in enumerate(slots):
        aut_of_row[row], ngr[row], bsor[row] = k, g, bs
        ids[row, :len(hist)] = hist
        step[s] = len(hist) - 1
        rel[row] = NONE if k is None else auts[k].walk(hist[1:hist.index(EOS)] if EOS in hist else hist[1:])
        if fin:
            finished[row] = 1; lens[row] = hist.index(EOS) + 1
        if pre:
            prefix[row, :len(pre)] = pre; plen[row] = len(pre)
    aut_of_row[4], ngr[4] = 1, 2                            # a row no slot decodes: whatever it holds stays
    abase = np.array([-1 if k is None else first[k] for k in aut_of_row], np.int32)
    rs = np.random.RandomState({"slabs1": 31, "slabs3": 33, "cand64": 364, "cand128": 428}[path])
    junk = rs.randint(0, 2 ** 32, size=(R + 1, MW), dtype=np.uint64).astype(np.uint32)

    def glob(rel_):
        return np.array([r + first[aut_of_row[i]] if r >= 0 else r for i, r in enumerate(rel_)], np.int32)

    def logits(k):
        lg = (np.round(rs.standard_normal((n, V)) * 3 * 256) / 256)
        for s in range(n):
            lg[s, top[s][k]] = [30.0, 29.0, 28.0, 27.0]
        return lg.astype(np.float32).astype(np.float64)

    def forced_of(state, with_prefix):
        _, step_, fin_, _, _, _ = state
        return {s: int(prefix[rowmap[s], step_[s]]) for s in range(n)
                if with_prefix and step_[s] < plen[rowmap[s]] and not fin_[rowmap[s]]}

    def inputs(lg, mk, forced):
        tgt = np.full(n + GUARD, np.nan, np.float32)
        if path.startswith("slabs"):
            nslab = int(path[5:])
            r2 = np.random.RandomState(5)
            bias = (r2.randint(-100, 100, V) / 64.0).astype(np.float64)
            parts = (r2.randint(-300, 300, (nslab, n, V)) / 64.0).astype(np.float64)
            parts[-1] = lg - bias - parts[:-1].sum(0)
            assert (parts.astype(np.float32).astype(np.float64) == parts).all()
            return dict(slabs=_f32(parts), nslab=nslab, vbias=_f32(bias)), None, None, None, _f32(tgt)
        tile = int(path[4:])
        nt = V // tile
        m, idx, s_ = cu.masked_tile_stats(lg, mk, tile)                  # what the masked LM head leaves for these sets
        t3 = cu.masked(lg, mk).reshape(n, nt, tile)
        ti = lex_top(t3)
        tv = np.take_along_axis(t3, ti, -1)
        ti = np.where(np.isneginf(tv), NO_IDX, ti + (np.arange(nt) * tile)[None, :, None])
        for s, tok in forced.items():                                    # ... and the target epilogue, for the forced slots
            tgt[s] = lg[s, tok] if mk[s, tok] else -np.inf
        return dict(cand_val=_f32(m), cand_idx=_i32(idx), ncand=nt), _f32(s_), _f32(tv), _i32(ti), _f32(tgt)

    def run(variant, lg, state):
        """one step on `state` (ids, step, finished, len, row_mask words, relative states) -> the state after it, alt_ids, scores"""
        ids_, step_, fin_, len_, rm_, rel_ = state
        kw, cand_sum, top_val, top_idx, tgt = inputs(lg, _unpack(rm_[rowmap]), forced_of(state, variant == 2))
        d = dict(ids=_i32(ids_), step=_i32(step_), finished=_i32(fin_), len=_i32(len_), n_unfinished=_i32([8, SENT]),
                 rowmap=_i32(rowmap), x_f32=torch.full((n + GUARD, D), float("nan"), device="cuda"),
                 x_t=torch.full((n + GUARD, D), float("nan"), device="cuda", dtype=torch.bfloat16 if dtype == "bf16" else torch.float32))
        sc = torch.full((R + 1, ids_ld), float("nan"), device="cuda") if variant == 2 else None
        ai = torch.full((R + 1, ids_ld, K4), SENT, dtype=torch.int32, device="cuda") if variant == 2 else None
        al = torch.full((R + 1, ids_ld, K4), float("nan"), device="cuda") if variant == 2 else None
        d_rm, d_state = _u32(rm_), _i32(glob(rel_))
        pre = (_i32(prefix), _i32(plen), ld, tgt) if variant == 2 else (None, None, 0, None)
        torch.cuda.synchronize()
        eng.op_dec_token_automaton(cand_sum if variant == 2 else None, sc, top_val if variant == 2 else None,
                                   top_idx if variant == 2 else None, ai, al, d_rm, _i32(np.arange(R + 1)), d_rm,
                                   _u32(cu.pack_sets(base2)), _i32(bsor), _i32(ngr), *pre, _i32(eb), _i32(et), _i32(en), _u8(acc),
                                   _i32(abase), d_state, first=0, n=n, ids_ld=ids_ld, max_len=max_len, n_real=n, **d, **kw)
        o = {k: v.cpu().numpy() for k, v in d.items() if k in ("ids", "step", "finished", "len")}
        g = d_state.cpu().numpy()
        back = np.array([int(x) - first[aut_of_row[i]] if x >= 0 and aut_of_row[i] is not None else int(x) for i, x in enumerate(g)], np.int64)
        return ((o["ids"], o["step"], o["finished"], o["len"], d_rm.cpu().numpy().view(np.uint32), back),
                None if ai is None else ai.cpu().numpy(), None if sc is None else sc.cpu().numpy())

    def reference(state, lg, with_prefix):
        """numpy: the state after one step on `state`, and the four best allowed tokens of every slot"""
        ids_, step_, fin_, len_, rm_, rel_ = (a.copy() for a in state)
        forced = forced_of(state, with_prefix)
        want4 = np.full((n, K4), -1)
        for s in range(n):
            row, t = rowmap[s], step_[s]
            eff = _unpack(rm_[row])
            was = bool(fin_[row])
            tok = 0 if was else int(np.argmax(np.where(eff, lg[s], -np.inf)))
            if not was:
                want4[s] = cu.masked_top(lg[s], eff)[0]
            tok = forced.get(s, tok)
            ids_[row, t + 1] = tok
            step_[s] = t + 1
            if not was and (tok == EOS or t + 2 >= max_len):
                fin_[row] = 1; len_[row] = t + 2
            a = None if aut_of_row[row] is None else auts[aut_of_row[row]]
            if was:
                continue
            if a is not None and tok != EOS:
                rel_[row] = a.next(int(rel_[row]), tok)
            if not fin_[row] and (a is not None or ngr[row] > 0):
                rm_[row] = cu.pack_sets(au.step_mask(a, int(rel_[row]), ids_[row, :t + 2], int(ngr[row]), base2[bsor[row]])[None])[0]
        return (ids_, step_, fin_, len_, rm_, rel_), want4

    LG = [logits(0), logits(1), logits(2)]
    rm0 = junk.copy()
    for s, (row, k, g, bs, hist, fin, pre) in enumerate(slots):
        if not fin:
            rm0[row] = cu.pack_sets(au.step_mask(None if k is None else auts[k], int(rel[row]), hist, g, base2[bs])[None])[0]
    names = ("ids", "step", "finished", "len", "row_mask", "state")
    state2 = state0 = (ids, step, finished, lens, rm0, rel)
    for k in range(3):
        want2, want4 = reference(state2, LG[k], True)
        want0, _ = reference(state0, LG[k], False)
        got2, ai, sc = run(2, LG[k], state2)
        got0, _, _ = run(0, LG[k], state0)
        for name, g2, w2, g0, w0 in zip(names, got2, want2, got0, want0):
            np.testing.assert_array_equal(g2, w2, err_msg=f"step {k + 1}, alternatives form: {name}")
            np.testing.assert_array_equal(g0, w0, err_msg=f"step {k + 1}, ids form: {name}")
        a4 = ai[rowmap, state2[1] + 1]
        live = state2[2][rowmap] == 0
        np.testing.assert_array_equal(a4[live], want4[live], err_msg="alt_ids is not the top four of the effective set")
        assert (a4[~live] == -1).all()
        for s in np.nonzero(live)[0]:
            a = a4[s][a4[s] >= 0]
            assert _unpack(state2[4][rowmap[s]])[a].all(), f"slot {s}: a token outside the effective set among the four"
            if s not in forced_of(state2, True):
                assert a4[s, 0] == got2[0][rowmap[s], state2[1][s] + 1]
        if k == 1:
            assert np.isneginf(sc[3, state2[1][6] + 1]), "the forced token without an edge is outside the effective set: -inf"
        state2, state0 = got2, got0
    # what the three steps proved (so that the table above cannot rot)
    ids3, _, fin3, len3, rm3, rel3 = state2
    w = slots[0][4][1:] + [top[0][0][1], top[0][1][1], top[0][2][2]]
    assert ids3[5, 1:6].tolist() == w and rel3[5] == auts[0].walk(w) >= 0, "slot 0 follows its word through the trie"
    assert ids3[2, 2:5].tolist() == [101, 103, EOS] and fin3[2] == 1 and rel3[2] == 2, "slot 1: EOS only once the loop accepts"
    assert ids3[7, 2:5].tolist() == [60, EOS + 1, 70] and _unpack(rm3[7]).all() and rel3[7] == 0, "slot 2: universal = unconstrained"
    assert ids3[0, 2:5].tolist() == [22, 22, 22] and (rm3[0] == rm0[0]).all() and rel3[0] == NONE, "slot 3: no automaton"
    assert ids3[9, 1:4].tolist() == [200, EOS, 0] and len3[9] == 3 and rel3[9] == 1, "slot 4: the dead end by token set ends the row"
    assert ids3[1, 4:7].tolist() == [102, 100, 103], "slot 5: the loop's bigram bans"
    assert ids3[3, 1:4].tolist() == [slots[6][6][0], 4000, EOS] and rel3[3] == DEAD and fin3[3] == 1, "slot 6: forced off the trie"
    assert state0[5][3] >= 0 and state0[0][3, 2] != 4000, "... and free in the ids form"
    k6 = len(slots[8][4])
    assert _unpack(rm0[6])[EOS] and ids3[6, k6] == top[8][0][0] != EOS, "slot 8 passes an accepting inner node of the trie without stopping"
    for untouched in (4, 8, 10):
        np.testing.assert_array_equal(rm3[untouched], junk[untouched], err_msg=f"row {untouched}: mask rewritten")
    assert rel3[8] == 1 and rel3[4] == SENT and rel3[10] == SENT
    report(f"dec_token AUTOMATON {dtype} {path}: three consecutive steps, ids, states and the 192 mask words of 10 rows exact against numpy "
           f"(trie of {auts[0].n_states} states, loop, universal, none, dead end by set, loop with n = 2, forced off the trie, finished, an accepting inner node)")


# ------------------------------------------------------------------------------------------------ 3 .. 5. end to end
N_E2E, LEN_E2E = 8, 32
KINDS8 = ["lexA", "lexA", "lexB", "loop", "loop", "universal", None, None]


def _automata8():
    """name -> Automaton of the end-to-end tests, and the lexicons' entry maps; the alphabet is what the free run emits"""
    if not _automata8.cache:
        free_ids, _ = su.oracle_run("wide", 31, N_E2E, LEN_E2E)
        alphabet = np.unique(free_ids[:, 1:])
        assert len(alphabet) == 10 and EOS not in alphabet and 0 not in alphabet
        la, ea = au.trie(_words(alphabet, 1))
        lb, eb_ = au.trie(_words(alphabet, 2))
        _automata8.cache.update(lexA=la, lexB=lb, loop=au.loop(alphabet[:4]), universal=au.universal(), alphabet=alphabet)
    return _automata8.cache


_automata8.cache = {}


def _handles(eng):
    """name -> handle of the end-to-end automata on this engine, created once"""
    if id(eng) not in _handles.cache:
        a8 = _automata8()
        _handles.cache[id(eng)] = {k: eng.automaton(*au.pack(a8[k])) for k in ("lexA", "lexB", "loop", "universal")}
    return _handles.cache[id(eng)]


_handles.cache = {}


def _rows(eng, kinds):
    h = _handles(eng)
    return np.array([0 if k is None else h[k] for k in kinds], np.int32)


def _reference():
    """(ids, logits, per-step masks, final states) of the reference loop on the fp32 oracle, widened-margin weights, crops(31, 8),
    max_len 32, rows under KINDS8; computed once"""
    if not _reference.cache:
        o = su.score_oracle("wide")
        a8 = _automata8()
        with torch.no_grad():
            enc = o.encode(o.preprocess_gray(crops(31, N_E2E)))
        _reference.cache.append(au.automaton_generate(o, enc, [None if k is None else a8[k] for k in KINDS8], np.ones((N_E2E, V), bool),
                                                      np.zeros(N_E2E, np.int32), LEN_E2E))
    return _reference.cache[0]


_reference.cache = []


def _oracle_preconditions():
    """On the oracle alone: every lexicon row ends by EOS in an accepting state before position 32 and differs from the free
    run; some step chooses among three or more edges; some row passes an accepting inner node without stopping.  -> the
    smallest allowed-token margin of every row"""
    a8 = _automata8()
    free_ids, _ = su.oracle_run("wide", 31, N_E2E, LEN_E2E)
    ids_o, logits, masks, states = _reference()
    lens_o = nu.lengths(ids_o)
    wide = passed = False
    for b in range(3):
        a = a8[KINDS8[b]]
        assert lens_o[b] < LEN_E2E and ids_o[b, lens_o[b] - 1] == EOS and states[b] in a.accepting, f"lexicon row {b} does not end in an entry"
        assert (free_ids[b, :lens_o[b]] != ids_o[b, :lens_o[b]]).any(), f"row {b}: the lexicon changed nothing"
    for b in range(6):                                      # every row under an automaton
        for t in range(1, lens_o[b]):
            wide = wide or masks[b, t - 1].sum() - masks[b, t - 1, EOS] >= 3
            passed = passed or (masks[b, t - 1, EOS] and ids_o[b, t] != EOS and masks[b, t - 1].sum() < V)
    assert wide, "no step chooses among three or more edges"
    assert passed, "no row passes an accepting inner node without stopping"
    assert (lens_o[3:] == LEN_E2E).all()
    gaps = nu.step_gaps(logits, masks)
    return np.array([gaps[b, :lens_o[b] - 1].min() for b in range(N_E2E)])


def test_fp32_automata_against_the_reference_loop():
    """fp32 engine, crops(31, 8), max_len 32, rows under [lexA, lexA, lexB, loop, loop, universal, none, none]: the lexicons are
    tries of 120 random words of 2 .. 8 of the ten tokens the free run emits, the loop runs over the first four of them.  After
    the oracle's own preconditions: ids, lengths and out_state identical to the reference loop; scores and alternatives within
    2 x FP32_LOGIT_TOL of the float64 masked log-softmax under the per-step masks (the bound of tests/test_gpu_ngram.py);
    alt_ids entry 0 = the id and no alternative outside its step's mask; the ids-only, scored and alternatives calls agree;
    the `none` rows and the universal row bit-identical to the unconstrained run."""
    margins = _oracle_preconditions()
    ids_o, logits, masks, states_o = _reference()
    lens_o = nu.lengths(ids_o)
    L = ids_o.shape[1]
    print(f"fp32 automata: reference lengths {lens_o.tolist()}, smallest allowed-token margins {[f'{m:.1e}' for m in margins]}", flush=True)
    eng = su.score_engine("wide", "fp32")
    gray = crops(31, N_E2E)
    rows = _rows(eng, KINDS8)
    ids, lens, logp, alt_ids, alt_logp, state = eng.recognize_gray(gray, LEN_E2E, alternatives=True, automata=rows, states=True)
    live = np.arange(L)[None, :] < lens_o[:, None]
    np.testing.assert_array_equal(np.where(live, ids[:, :L], 0), np.where(live, ids_o, 0), err_msg="fp32 ids differ from the reference loop's")
    np.testing.assert_array_equal(lens, lens_o)
    np.testing.assert_array_equal(state, states_o)
    assert (ids[:, L:] == 0).all()
    tol = 2 * FP32_LOGIT_TOL
    worst = 0.0
    for b in range(N_E2E):
        for t in range(1, lens[b]):
            ref = cu.masked_log_softmax64(logits[b, t - 1], masks[b, t - 1])
            a = alt_ids[b, t]
            ok = a >= 0
            assert a[0] == ids[b, t] and masks[b, t - 1][a[ok]].all() and ok.sum() == min(K4, masks[b, t - 1].sum()), \
                f"row {b} token {t}: alternatives {a.tolist()}"
            want4, lp4 = cu.masked_top(logits[b, t - 1], masks[b, t - 1])
            np.testing.assert_array_equal(a, want4)
            worst = max(worst, abs(float(logp[b, t]) - ref[ids[b, t]]), float(np.abs(alt_logp[b, t][ok] - ref[a[ok]]).max()),
                        float(np.abs(alt_logp[b, t][ok].astype(np.float64) - lp4[ok]).max()))
            assert np.isneginf(alt_logp[b, t][~ok]).all()
            np.testing.assert_array_equal(_bits(alt_logp[b, t, :1]), _bits(logp[b, t:t + 1]))
    print(f"fp32 automata: max |logp - float64 masked log-softmax| {worst:.3e} (bound {tol:.0e})", flush=True)
    assert worst <= tol, worst
    i0, l0, s0 = eng.recognize_gray(gray, LEN_E2E, automata=rows, states=True)
    i1, l1, p1 = eng.recognize_gray(gray, LEN_E2E, scores=True, automata=rows)
    np.testing.assert_array_equal(i0, ids); np.testing.assert_array_equal(i1, ids); np.testing.assert_array_equal(l0, lens)
    np.testing.assert_array_equal(l1, lens); np.testing.assert_array_equal(s0, state)
    np.testing.assert_array_equal(_bits(p1), _bits(logp))
    z = [5, 6, 7]
    fi, fl, fp, fa, fal = eng.recognize_gray(gray, LEN_E2E, alternatives=True)
    np.testing.assert_array_equal(fi[z], ids[z], err_msg="a row without an automaton, or the universal row, differs from the unconstrained run")
    np.testing.assert_array_equal(fl[z], lens[z]); np.testing.assert_array_equal(_bits(fp[z]), _bits(logp[z]))
    np.testing.assert_array_equal(fa[z], alt_ids[z]); np.testing.assert_array_equal(_bits(fal[z]), _bits(alt_logp[z]))
    assert state[5] == 0 and (state[6:] == NONE).all()
    report(f"token automata fp32 vs the reference loop, 8 crops, max_len 32: ids, lengths {lens.tolist()} and states identical (smallest "
           f"allowed margin {margins.min():.1e}), logp / alt_logp within {worst:.2e} (bound {tol:.0e}); none / universal rows == the free run")


def test_loop_ngram_and_token_set_together():
    """The situation of tests/test_gpu_ngram.py's test_token_set_and_ngram_together, under the loop as well: a set of 4 tokens,
    the loop over the same 4 and n = 2, fp32, 8 crops, max_len 32.  4 symbols have 16 bigrams, so a row holds at most 17 of
    them before every one is banned; the loop accepts from two tokens on, so EOS is allowed then: every row ends by EOS with at
    most 19 tokens, identical to the reference loop, states included."""
    o = su.score_oracle("wide")
    a8 = _automata8()
    digits = a8["alphabet"][:4]
    base = np.repeat(cu.mask_of(digits)[None], N_E2E, 0)
    ngr = np.full(N_E2E, 2, np.int32)
    with torch.no_grad():
        enc = o.encode(o.preprocess_gray(crops(31, N_E2E)))
    ids_o, logits, masks, states_o = au.automaton_generate(o, enc, [a8["loop"]] * N_E2E, base, ngr, LEN_E2E)
    eng = su.score_engine("wide", "fp32")
    ids, lens, logp, alt_ids, alt_logp, state = eng.recognize_gray(crops(31, N_E2E), LEN_E2E, alternatives=True, token_sets=eng.token_set(digits),
                                                                   no_repeat_ngram=2, automata=_handles(eng)["loop"], states=True)
    L = ids_o.shape[1]
    lens_o = nu.lengths(ids_o)
    live = np.arange(L)[None, :] < lens_o[:, None]
    np.testing.assert_array_equal(np.where(live, ids[:, :L], 0), np.where(live, ids_o, 0))
    np.testing.assert_array_equal(lens, lens_o); np.testing.assert_array_equal(state, states_o)
    for b in range(N_E2E):
        assert ids[b, lens[b] - 1] == EOS and 4 <= lens[b] <= 19, f"row {b}: {ids[b, :lens[b]].tolist()}"
        assert nu.first_repeat(ids[b, :lens[b]], 2) is None and state[b] == 2
        for t in range(1, lens[b]):
            a = alt_ids[b, t]
            assert masks[b, t - 1][a[a >= 0]].all() and a[0] == ids[b, t] and (a >= 0).sum() == min(K4, int(masks[b, t - 1].sum()))
    report(f"loop + n = 2 + a set of 4, fp32: ids and states identical to the reference loop, lengths {lens.tolist()}, every row ends by EOS")


@pytest.mark.parametrize("name,rows,flags", BF16_CASES)
def test_bf16_automaton_paths(name, rows, flags):
    """bf16, the 8-row pattern of the fp32 test repeated over the batch.  Every row, exactly and whatever the precision: its
    ids are a path of its automaton, EOS appears only from an accepting state (or by the dead-end rule), out_state is the
    walk's end; the rows without an automaton have state NONE.  The first 8 rows against the fp32 reference loop under the
    first-divergence rule with BF16_GAP_TOL - and the lexicon rows admit no divergence: their reference margins are at least
    3 x BF16_GAP_TOL, asserted on the oracle."""
    margins = _oracle_preconditions()
    assert (margins[:3] >= 3 * BF16_GAP_TOL).all(), f"the lexicon rows' margins {margins[:3]} do not exclude a bf16 divergence"
    ids_o, logits, masks, states_o = _reference()
    a8 = _automata8()
    eng = su.score_engine("wide", "bf16", max_batch=max(64, rows), flags=flags)
    gray = np.concatenate([crops(31, N_E2E)] * (rows // N_E2E))
    kinds = KINDS8 * (rows // N_E2E)
    aut = _rows(eng, kinds)
    ids, lens, logp, alt_ids, alt_logp, state = eng.recognize_gray(gray, LEN_E2E, alternatives=True, automata=aut, states=True)
    for b in range(rows):
        np.testing.assert_array_equal(alt_ids[b, 1:lens[b], 0], ids[b, 1:lens[b]])
        if kinds[b] is None:
            assert state[b] == NONE
            continue
        ok, end = au.is_path(a8[kinds[b]], ids[b], lens[b], eos_by_dead_end=True)
        assert ok, f"row {b} ({kinds[b]}) left its automaton: {ids[b, :lens[b]].tolist()}"
        assert state[b] == end, f"row {b}: out_state {state[b]}, the walk ends in {end}"
    assert np.isfinite(logp).all() and (logp <= 0).all()
    i0, l0 = eng.recognize_gray(gray, LEN_E2E, automata=aut)
    i1, l1, p1, s1 = eng.recognize_gray(gray, LEN_E2E, scores=True, automata=aut, states=True)
    np.testing.assert_array_equal(i0, ids); np.testing.assert_array_equal(i1, ids); np.testing.assert_array_equal(l1, lens)
    np.testing.assert_array_equal(_bits(p1), _bits(logp)); np.testing.assert_array_equal(s1, state)
    L = ids_o.shape[1]
    lens_o = nu.lengths(ids_o)
    div = cu.first_divergences(ids[:N_E2E, :L], ids_o, nu.step_gaps(logits, masks))
    for b, t, g in div:
        report(f"[bf16 automata {name}] row {b}: first divergence at token {t} (reference margin among the allowed tokens {g:.3e})")
    assert all(g < BF16_GAP_TOL for _, _, g in div), div
    assert not [b for b, _, _ in div if b < 3], "a lexicon row left the reference"
    np.testing.assert_array_equal(lens[:3], lens_o[:3]); np.testing.assert_array_equal(state[:3], states_o[:3])
    report(f"token automata bf16 {name} ({rows} rows, flags {flags}): every row a path of its automaton with out_state the walk's end, "
           f"{len(div)} first divergences of 8 (none on a lexicon row), all below the allowed margin {BF16_GAP_TOL}")


# ------------------------------------------------------------------------------------------------ 6. compaction
def test_automaton_compacted_equals_uncompacted():
    """The shape of tests/test_gpu_ngram.py's compaction test: early-EOS weights, 96 rows, max_len 120, automata cycling through
    (lexicon, loop, universal, none) over the tokens the free run emits.  Rows finish at different steps, the batch is
    compacted, and ids, lengths and states equal those of an engine that never compacts: states and masks are indexed by row,
    so a compaction moves none.  The rows without an automaton equal the free run."""
    n, max_len = 96, 120
    gray = np.concatenate([crops(4321, 6), crops(4322, n)])[:n]
    eng = su.score_engine("eos", "bf16", max_batch=96)
    nc = su.score_engine("eos", "bf16", max_batch=96, flags=2048)          # MOCR_FLAG_NO_COMPACTION
    f_ids, f_lens = eng.recognize_gray(gray, max_len)
    toks, counts = np.unique(f_ids[:, 1:], return_counts=True)
    alphabet = [int(t) for t in toks[np.argsort(-counts)] if t not in (0, EOS)][:10]
    assert len(alphabet) >= 4
    auts = [au.trie(_words(alphabet, 3))[0], au.loop(alphabet[:4]), au.universal(), None]
    kinds = [k % 4 for k in range(n)]
    out = []
    for e in (eng, nc):
        hs = [e.automaton(*au.pack(a)) for a in auts[:3]] + [0]
        base = e.compaction_count()
        out.append(e.recognize_gray(gray, max_len, automata=[hs[k] for k in kinds], states=True))
        out.append(e.compaction_count() - base)
    (ids, lens, state), compactions, (u_ids, u_lens, u_state), none = out
    assert compactions > 0 and none == 0
    np.testing.assert_array_equal(ids, u_ids); np.testing.assert_array_equal(lens, u_lens); np.testing.assert_array_equal(state, u_state)
    assert lens.min() < lens.max(), "rows were meant to finish at different steps"
    for b in range(n):
        if auts[kinds[b]] is None:
            assert state[b] == NONE
            continue
        ok, end = au.is_path(auts[kinds[b]], ids[b], lens[b], eos_by_dead_end=True)
        assert ok and state[b] == end, f"row {b}: {ids[b, :lens[b]].tolist()} state {state[b]}"
    z = np.array(kinds) >= 2
    np.testing.assert_array_equal(ids[z], f_ids[z]); np.testing.assert_array_equal(lens[z], f_lens[z])
    assert (ids[~z] != f_ids[~z]).any()
    report(f"token automata bf16 early-EOS 96 rows, lengths {int(lens.min())}..{int(lens.max())}: compacted == uncompacted (states too), "
           f"none / universal rows == the free run")


# ------------------------------------------------------------------------------------------------ 7. shared encodings
def test_four_automata_over_one_encoding():
    """One crop decoded in four rows under (lexA, loop, universal, none) through sources = [0, 0, 0, 0]: every row equals its
    row of a call of the same batch size - four rows over the one crop - in which all four rows bring that automaton, bit
    for bit; the crop is encoded once."""
    eng = su.score_engine("wide", "fp32")
    gray = crops(31, 1)
    kinds = ["lexA", "loop", "universal", None]
    hs = _rows(eng, kinds)
    before = eng.encoded_crops()
    ids, lens, logp, state = eng.recognize_gray(gray, LEN_E2E, scores=True, sources=[0] * 4, automata=hs, states=True)
    assert eng.encoded_crops() - before == 1
    for k in range(4):
        i1, l1, p1, s1 = eng.recognize_gray(gray, LEN_E2E, scores=True, sources=[0] * 4, automata=[int(hs[k])] * 4, states=True)
        np.testing.assert_array_equal(i1[k], ids[k]); assert l1[k] == lens[k] and s1[k] == state[k]
        np.testing.assert_array_equal(_bits(p1[k]), _bits(logp[k]))
    ref = _reference()
    np.testing.assert_array_equal(ids[0, :lens[0]], ref[0][0, :lens[0]])
    assert state[3] == NONE and state[2] == 0 and (ids[0] != ids[3]).any()


# ------------------------------------------------------------------------------------------------ 8. graphs, memory, errors
def _desc(eb, et, en, acc, struct_size=None, n_states=None):
    arrs = (np.ascontiguousarray(eb, np.int32), np.ascontiguousarray(et, np.int32), np.ascontiguousarray(en, np.int32),
            np.ascontiguousarray(acc, np.uint8))
    d = _capi.MocrAutomatonDesc(C.sizeof(_capi.MocrAutomatonDesc) if struct_size is None else struct_size,
                                len(arrs[3]) if n_states is None else n_states, *(a.ctypes.data for a in arrs))
    return d, arrs


def test_graphs_memory_and_errors():
    """An engine nobody asked allocates nothing for the feature (mocr_automaton_state_bytes 0, free device memory unchanged, also
    by calls whose automata are all MOCR_AUTOMATON_NONE); the first create allocates the arena, the first automaton batch the
    rows' states and captures graphs of its own; a repeat captures no graph and allocates nothing; an automaton created after
    the graphs were captured works on replay; every MOCR_ERR_ARG case of mocr_automaton_create and an unknown handle are refused."""
    from manga_ocr._capi import MocrError
    from manga_ocr.engine import device_memory
    eng = su.score_engine.__wrapped__("wide", "bf16", max_batch=64)
    try:
        gray = crops(5, 40)
        want, want_l = eng.recognize_gray(gray, 16)
        eng.recognize_gray(gray, 16, scores=True)
        g1 = eng.graph_count()
        torch.cuda.synchronize()
        free0 = device_memory(0)[0]
        eng.recognize_gray(gray, 16); eng.recognize_gray(gray, 16, scores=True)
        i_, l_, s_ = eng.recognize_gray(gray, 16, automata=0, states=True)
        eng.recognize_gray(gray, 16, automata=[None] * 40)
        assert eng.graph_count() == g1 and device_memory(0)[0] == free0 and eng.automaton_state_bytes() == 0, "an engine nobody asked grew"
        np.testing.assert_array_equal(i_, want); assert (s_ == NONE).all() and eng.automaton_count() == 0
        digits = np.unique(want[:, 1:])
        digits = digits[(digits != EOS) & (digits != 0)][:6]
        assert len(digits) == 6
        a1, a2 = au.loop(digits[:4]), au.loop(digits[2:6], at_least=1)
        h1 = eng.automaton(*au.pack(a1))
        arena = eng.automaton_state_bytes()
        assert h1 == 1 and eng.automaton_count() == 1 and (36 << 20) <= arena <= (38 << 20)
        ids, lens, st = eng.recognize_gray(gray, 16, automata=h1, states=True)
        g2 = eng.graph_count()
        free1 = device_memory(0)[0]
        assert g2 > g1, "the first automaton batch captures graphs of its own"
        assert 0 < eng.automaton_state_bytes() - arena <= 1 << 16 and free0 - free1 <= 64 << 20
        for b in range(40):
            ok, end = au.is_path(a1, ids[b], lens[b], eos_by_dead_end=True)
            assert ok and st[b] == end
        eng.recognize_gray(gray, 16, automata=h1); eng.recognize_gray(gray, 16, automata=[h1, 0] * 20)
        assert eng.graph_count() == g2 and device_memory(0)[0] == free1, "a repeated call captured a graph or allocated"
        assert g2 - g1 <= g1, "the automaton graphs are the ids-mode ones only"
        h2 = eng.automaton(*au.pack(a2))                      # created after the graphs were captured: works on replay
        ids2, lens2, st2 = eng.recognize_gray(gray, 16, automata=[h2, h1] * 20, states=True)
        assert h2 == 2 and eng.graph_count() == g2 and device_memory(0)[0] == free1
        for b in range(40):
            ok, end = au.is_path((a2, a1)[b % 2], ids2[b], lens2[b], eos_by_dead_end=True)
            assert ok and st2[b] == end, f"row {b}"
        np.testing.assert_array_equal(ids2[1::2], ids[1::2])
        b_ids, b_lens = eng.recognize_gray(gray, 16)
        np.testing.assert_array_equal(b_ids, want); np.testing.assert_array_equal(b_lens, want_l)
        # the refusals
        for bad in ([99] * 40, [-1] * 40, [h1] * 39 + [3]):
            with pytest.raises(MocrError):
                eng.recognize_gray(gray, 16, automata=bad)
        with pytest.raises(ValueError):
            eng.recognize_gray(gray, 16, automata=[h1] * 39)
        out = C.c_int32(SENT)
        good = ([0, 2, 2], [10, 11], [1, 1], [0, 1])
        cases = {
            "a short struct": _desc(*good, struct_size=8),
            "n_states < 1": _desc([0], [], [], [], n_states=0),
            "edge_begin[0] != 0": _desc([1, 2, 2], [10, 11], [1, 1], [0, 1]),
            "edge_begin not monotone": _desc([0, 2, 1], [10, 11], [1, 1], [0, 1]),
            "a negative token": _desc([0, 2, 2], [-1, 11], [1, 1], [0, 1]),
            "a token = vocab": _desc([0, 2, 2], [10, V], [1, 1], [0, 1]),
            "EOS as a token": _desc([0, 2, 2], [EOS, 11], [1, 1], [0, 1]),
            "equal tokens": _desc([0, 2, 2], [10, 10], [1, 1], [0, 1]),
            "descending tokens": _desc([0, 2, 2], [11, 10], [1, 1], [0, 1]),
            "edge_next = n_states": _desc([0, 2, 2], [10, 11], [1, 2], [0, 1]),
            "edge_next < 0": _desc([0, 2, 2], [10, 11], [-1, 1], [0, 1]),
            "more states than the table holds": _desc(np.zeros(_capi.MAX_AUTOMATON_STATES + 2, np.int32), [], [],
                                                      np.zeros(_capi.MAX_AUTOMATON_STATES + 1, np.uint8)),
        }
        for what, (d, keep) in cases.items():
            assert eng.lib.mocr_automaton_create(eng._h, C.byref(d), C.byref(out)) == -1 and out.value == SENT, what
        assert eng.lib.mocr_automaton_create(eng._h, None, C.byref(out)) == -1, "a null struct"
        d, keep = _desc(*good)
        assert eng.lib.mocr_automaton_create(eng._h, C.byref(d), C.byref(out)) == 0 and out.value == 3 and eng.automaton_count() == 3
        for k in range(4, _capi.MAX_AUTOMATA + 1):
            assert eng.lib.mocr_automaton_create(eng._h, C.byref(d), C.byref(out)) == 0 and out.value == k
        assert eng.lib.mocr_automaton_create(eng._h, C.byref(d), C.byref(out)) == -1, "the handle list is full"
        assert eng.automaton_count() == _capi.MAX_AUTOMATA and device_memory(0)[0] == free1
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 9. ABI twins
@pytest.mark.parametrize("kind", ["device", "gray_host", "images", "regions"])
def test_automaton_twin_with_nulls_is_the_shared_call(kind):
    """mocr_recognize_<kind>_automaton with `automata` and out_state null against mocr_recognize_<kind>_shared, every other
    argument given, 3 rows over 3 sources (the middle region a sliver), max_len 8: every output bit for bit."""
    import test_gpu_abi_twins as tw
    from manga_ocr.engine import _ptr
    eng = tw._engine()
    gray, page = tw._inputs()
    N, L, T = tw.N, tw.L, tw.T
    dev = kind == "device"
    sets, ngram = tw._per_crop()
    src = np.array([0, 1, 2], np.int32)
    prefix, plen = np.zeros((N, 1), np.int32), np.zeros(N, np.int32)

    def call(variant):
        def block(shape, dtype, fill=0):
            return torch.full(shape, fill, dtype=getattr(torch, dtype), device="cuda") if dev else np.full(shape, fill, dtype=dtype)
        outs = [block((N, L), "int32", -7), block((N,), "int32", -7), block((N, L), "float32"), block((N, L, 4), "int32", -1),
                block((N, L, 4), "float32"), block((N, L, 5), "float32")]
        tail = [_ptr(o) for o in outs[:5]] + [_ptr(sets), _ptr(ngram), _ptr(outs[5]), _ptr(prefix), _ptr(plen), 1]
        tail += [None, None] if variant == "automaton" else []
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
            for i, (pg, x, y, w, h) in enumerate(tw.REGIONS):
                arr[i].page, arr[i].x, arr[i].y, arr[i].width, arr[i].height = pg, x, y, w, h
            rc = fn(eng._h, descs, 1, arr, N, N, _ptr(src), *tail)
        assert rc == _capi.MOCR_OK
        return [o.cpu().numpy() if dev else o for o in outs]

    got, want = call("automaton"), call("shared")
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    assert (got[1][[0, 2]] >= 2).all() and (got[2][[0, 2], 1] < 0).all()
    assert eng.automaton_state_bytes() == 0


# ------------------------------------------------------------------------------------------------ 10. product surface
def test_product_surface_lexicon():
    """MangaOcr.lexicon and lexicon=: the recognition is an entry of the list, `accepted` is true and `entry` points at it; a
    crop without a lexicon in the same call decodes freely; the raw form (MangaOcr.automaton) gives a pattern."""
    from PIL import Image
    from manga_ocr import MangaOcr
    imgs = [Image.fromarray(g) for g in crops(77, 4)]
    m = MangaOcr(synthetic_seed=0, dtype="fp32", max_batch=8, lanes=1)
    try:
        free = m.recognize_batch_scored(imgs)
        chars = [m.vocab.tokens[int(t)] for r in free for t in r.ids[1:-1]]
        chars = sorted({c for c in chars if len(c) == 1 and m.vocab.encode_chars(c) is not None})[:6]
        assert len(chars) >= 3
        rs = np.random.RandomState(5)
        names = sorted({"".join(rs.choice(chars, size=rs.randint(2, 6))) for _ in range(40)})
        lx = m.lexicon(names)
        rec = m.recognize_scored(imgs[0], lexicon=lx)
        assert rec.accepted and rec.entry is not None and names[rec.entry] == rec.text and rec.text in names
        assert rec.state >= 0 and np.isfinite(rec.logprobs).all()
        recs = m.recognize_batch_scored(imgs, lexicon=[lx, None, lx, None])
        assert recs[0].text == rec.text and recs[0].entry == rec.entry
        assert recs[1].text == free[1].text and recs[1].entry is None and recs[1].state == NONE and not recs[1].accepted
        assert recs[2].accepted and names[recs[2].entry] == recs[2].text
        assert m.recognize(imgs[0], lexicon=lx) == rec.text and m.recognize_batch(imgs, lexicon=lx)[2] == recs[2].text
        ids = [m.vocab.encode_chars(c)[0] for c in chars[:3]]
        two = m.automaton({0: {t: 1 for t in ids}, 1: {t: 2 for t in ids}}, [2])
        r2 = m.recognize_scored(imgs[3], lexicon=two)
        assert len(r2.text) == 2 and set(r2.text) <= set(chars[:3]) and r2.accepted and r2.entry is None and r2.state == 2
        with pytest.raises(ValueError):
            m.recognize_beam(imgs[0], lexicon=lx)
    finally:
        m.close()
