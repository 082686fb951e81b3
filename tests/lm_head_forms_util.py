"""The fused LM head's tile forms (tests/test_lm_head_forms_cpu.py, tests/test_gpu_lm_head_forms.py): the list of forms, the
operands that make every one of them exact, and the numpy mirror.

TileFamily (csrc/engine.hip, tile_forms()) builds gemm_kernel with a vocabulary epilogue in 72 forms per storage type:
(level ids / scored / alternatives) x (masked) x (target column) x (plain / SOFT / PEN) x (64 / 128 tile) x (2 / 4 ring slots),
a target column only on the masked scored and alternatives forms and SOFT / PEN only on the masked ones.  `forms()` states
that list again without the device, `hook_of` names the operator hook and the arguments that make launch_gemm_tile ask for a
form, and `rows_for` gives the smallest row count at which tile_launch hands out a ring.

The operands are the dyadic ones of tests/test_gpu_penalty_kernels.py and tests/test_gpu_soft_automaton_kernels.py (A in
{-1, 0, 1}, W in {-2 .. 2} / 4, bias on a 1/8 grid: every fp32 sum and every bf16 store exact), but live in every 32-element
K-tile of every row of A and W, so a K-tile that is dropped, staged into the wrong ring slot or multiplied twice changes a sum.
Everything the kernel reads by ROW (set, automaton state, seen words, penalty, prefix) is indexed by row behind a permuted
rowmap; `step` and `tgt_val` are by slot.  `build` asserts on the reference, before any launch, what the shapes are for."""
import collections
import functools
import types

import numpy as np

import automaton_util as au
import bias_util as bu
import constraint_util as cu
import penalty_util as pu
import score_util as su

D, V, K4, EOS = 768, 6144, 4, 3
KT = 32                               # elements of the shortest K-tile (fp32: 128 bytes of a row; bf16 walks 64)
NONE, DEAD = au.NONE, au.DEAD
NO_IDX = cu.NO_IDX

# ------------------------------------------------------------------------------------------------ the forms
LEVELS = ("ids", "scored", "alternatives")
RICHES = ("plain", "soft", "pen")
TILES, RINGS = (64, 128), (2, 4)
EPI_NAME = {("ids", False): "EPI_ARGMAX", ("scored", False): "EPI_ARGMAX_LSE", ("alternatives", False): "EPI_TOPK",
            ("ids", True): "EPI_ARGMAX_M", ("scored", True): "EPI_ARGMAX_LSE_M", ("alternatives", True): "EPI_TOPK_M"}
Variant = collections.namedtuple("Variant", "level masked tgt rich")
Form = collections.namedtuple("Form", "level masked tgt rich tile ring")


def variants():
    """the 18 forms of one (tile, ring), by tile_forms()'s rule: a target column only on the masked scored / alternatives
    epilogues, SOFT / PEN only on the masked ones"""
    return [Variant(level, masked, tgt, rich)
            for level in LEVELS for masked in (False, True) for tgt in (False, True) for rich in RICHES
            if (not tgt or (masked and level != "ids")) and (rich == "plain" or masked)]


def forms():
    return [Form(*v, tile, ring) for tile in TILES for ring in RINGS for v in variants()]


def form_name(f) -> str:
    return EPI_NAME[(f.level, f.masked)] + (" TGT" if f.tgt else "") + {"plain": "", "soft": " SOFT", "pen": " PEN"}[f.rich]


def hook_of(v):
    """-> (the Engine method that launches the form, what it is given): cs / top = d_cand_sum / d_top_val + d_top_idx given,
    target = the five target arrays given, tables = the soft tables given, pen = seen words and penalties given.  A PEN form
    is reached with and without tables (launch_gemm_tile: "a penalty's form is a SOFT one whether or not `soft` is given")."""
    given = dict(cs=v.level != "ids", top=v.level == "alternatives", target=v.tgt, tables=v.rich != "plain", pen=v.rich == "pen")
    if not v.masked:
        return {"ids": "op_gemm_argmax", "scored": "op_gemm_argmax_lse", "alternatives": "op_gemm_topk"}[v.level], given
    if v.rich == "pen":
        return "op_gemm_argmax_penalty", given
    if v.rich == "soft":
        return "op_gemm_argmax_soft", given
    return ("op_gemm_argmax_target" if v.tgt else "op_gemm_argmax_masked"), given


def key_of(hook: str, given) -> tuple:
    """launch_gemm_tile's key from what a hook is given: (epilogue by the richest output and the mask, tgt_val != nullptr,
    soft || pen, pen != nullptr)"""
    masked = hook not in ("op_gemm_argmax", "op_gemm_argmax_lse", "op_gemm_topk")
    level = "alternatives" if given["top"] else "scored" if given["cs"] else "ids"
    return EPI_NAME[(level, masked)], bool(given["target"]), bool(given["tables"] or given["pen"]), bool(given["pen"])


def untested_before():
    """the 24 forms per type that no kernel-level test reached before these: on (128, ring 2) everything but the plain
    EPI_ARGMAX of tests/test_gpu_decode_regimes.py, on (64, ring 2) the five PEN forms and the two plain target forms"""
    out = [f for f in forms() if (f.tile, f.ring) == (128, 2) and not (f.level == "ids" and not f.masked)]
    out += [f for f in forms() if (f.tile, f.ring) == (64, 2) and (f.rich == "pen" or (f.tgt and f.rich == "plain"))]
    return out


def case_id(dtype: str, tile: int, ring: int) -> str:
    return f"{dtype}-tile{tile}-ring{ring}"


def ring_rule(dtype: str, rows: int, tile: int, cus: int) -> int:
    """tile_launch: four slots iff rows < 1280, at least 4 K-tiles and at most one block per compute unit (N 6144, K 768, no split)"""
    ktiles = D // (64 if dtype == "bf16" else 32)
    return 4 if rows < 1280 and ktiles >= 4 and -(-rows // tile) * (V // tile) <= cus else 2


def rows_for(tile: int, ring: int, cus: int) -> int:
    """the smallest row count with a ragged last M-tile of one row that gets the ring on `cus` compute units: ring 2 one M-tile
    more than fits one block per unit (or 1280 rows, where the rule turns by itself), ring 4 two M-tiles"""
    return min((cus // (V // tile)) * tile + 1, 1280) if ring == 2 else tile + 1


# ------------------------------------------------------------------------------------------------ the operands
# the constructed columns of test_penalty_lm_head_exact: every row's logit there is the value, whatever A's random part holds
CONS = {100: 50.0, 200: 40.0, 37: 25.0, 150: 0.0, 210: -30.0}
# first / last column of a 64 and a 128 tile, both sides of a word boundary, the first column of the last tile, the last column
CORNERS = [0, 31, 32, 63, 64, 127, 128, 255, V - 64, V - 1]
BANNED_CORNERS = [31, 32, 64, 127, V - 1]            # ... of which sets 1 and 2 ban these (both sides of a word boundary among them)
NK = 10
# row kinds r % 10: 0 .. 7 are test_penalty_lm_head_exact's, 8 .. 9 and the NONE rows test_soft_lm_head_exact's
#   0 p = 2, 100 and 200 seen: 25.0 ties with the unseen 37, 200 falls to 20 - the lower column wins
#   1 p = 1.3, 100 seen: the unpenalised winner falls below 200
#   2 p = 0.8, 200 seen: 40 / 0.8 = 50.0 ties with 100 - a tie made by a reward, the lower column wins
#   3 p = 2, 100 and 37 seen: 200 wins
#   4 p = 1: nothing changes
#   5 p = 1.3, 100 seen and outside the row's set (set 1): it stays -inf
#   6 p = 2, 100 seen under an edge weight of +32: (50 + 32) / 2 = 41 wins - the order sequence_bias -> penalty; the automaton
#     also has edges on the group / tile corners
#   7 p = 1.3, a random half seen (as every row has)
#   8 state DEAD, p = 1.3
#   9 p = 2, an edge of -64 on the winner: 200, in another tile, wins
# (kinds 0 .. 5 and 7 are in state NONE)
P_OF_KIND = np.array([2.0, 1.3, 0.8, 2.0, 1.0, 1.3, 2.0, 1.3, 1.3, 2.0], np.float32)
RAGGED_ROW = 16                       # kind 6, set 2, a target at step 0 (column 100): the row of the ragged M-tile's one slot


def _round_up(n, q):
    return -(-n // q) * q


def _sprinkle(rs, rows, per_tile, values, first):
    """[rows, D]: `per_tile` entries drawn from `values` at random places >= `first` of every KT-element K-tile, 0 elsewhere"""
    nkt = D // KT
    x = np.zeros((rows, nkt, KT), np.float32)
    where = np.argsort(rs.rand(rows, nkt, KT - first), axis=-1)[..., :per_tile] + first
    np.put_along_axis(x, where, rs.choice(values, size=where.shape).astype(np.float32), axis=-1)
    return x.reshape(rows, D)


@functools.lru_cache(maxsize=1)
def weights():
    """(W [V, D], bias [V]) of every case: four entries of {-2, -1, 1, 2} / 4 in every K-tile of every row, bias on a 1/8 grid;
    a constructed column has 1/4 or 1/2 at the first element of every K-tile - where every row of A holds 1 - and nothing else,
    so its logit is 9 + bias in every row and still loses or gains 1/4 or 1/2 with a K-tile"""
    rs = np.random.RandomState(72)
    W = _sprinkle(rs, V, 4, np.array([-2, -1, 1, 2]) / 4.0, 0)
    bias = (rs.randint(-16, 17, size=V) / 8.0).astype(np.float32)
    pilot = (1 + np.arange(D // KT) % 2) / 4.0
    for c, val in CONS.items():
        W[c] = 0
        W[c, ::KT] = pilot
        bias[c] = val - pilot.sum()
    for a in (W, bias):
        a.setflags(write=False)
    return W, bias


def automata():
    """kind 6's and kind 9's one-state automata and their packed tables (tests/bias_util.py)"""
    corners = {0: 1.5, 15: -2.0, 16: 0.5, 63: 3.0, 64: -1.0, 127: 2.5, 128: 1.0, 255: -4.0, V - 1: 4.0}
    edges = [{100: 32.0, **corners}, {100: -64.0}]
    auts = [bu.SoftAutomaton({0: {t: 0 for t in e}}, [0], {0: e}, 0, 1) for e in edges]
    return auts, bu.pack_many(auts)


@functools.lru_cache(maxsize=4)
def build(tile: int, M: int):
    """the operands of one (tile, rows) - shared by both storage types, whose values they all are - with everything asserted
    that the shapes are meant to hold.  GEMM row m is slot m of rowmap over R = M + 3 rows."""
    assert M > tile and M % tile == 1, "at least one full M-tile and a ragged one of a single row"
    rs = np.random.RandomState(1000 + 7 * tile + M)
    R, Mp, nt = M + 3, _round_up(M, tile), V // tile
    perm = rs.permutation(R)
    j = int(np.nonzero(perm == RAGGED_ROW)[0][0])
    perm[[j, M - 1]] = perm[[M - 1, j]]
    rowmap = perm[:M].astype(np.int32)
    rows = rowmap
    r_ = np.arange(R)
    kind = r_ % NK
    W, bias = weights()
    A = np.full((Mp, D), np.nan, np.float32)                 # the rows behind M are staged and may reach no output
    A[:M] = _sprinkle(rs, M, 6, np.array([-1, 1]), 1)
    A[:M, ::KT] = 1
    for x in (A[:M], W):
        assert (x.reshape(x.shape[0], D // KT, KT) != 0).any(-1).all(), "a K-tile of a row without a nonzero"
    logits64 = A[:M].astype(np.float64) @ W.astype(np.float64).T + bias
    logits = logits64.astype(np.float32)
    assert (logits == logits64).all(), "a logit is not exact in fp32"
    assert np.abs(logits64).max() < 64
    for c, val in CONS.items():
        assert (logits[:, c] == val).all()
    assert np.delete(logits, list(CONS), axis=1).max() < 20, "a random column above the constructed ones' penalised values"

    masks = np.ones((3, V), bool)
    masks[1:] = rs.rand(2, V) < 0.5
    masks[1:, [EOS, 0, 63, 128, 255, V - 64] + list(CONS)] = True
    masks[1:, BANNED_CORNERS] = False
    masks[1, 100] = False
    set_of_row = np.where(kind == 5, 1, np.where((r_ // NK) % 2 == 1, 2, 0)).astype(np.int32)
    auts, (eb, et, en, acc, ew, dn, first) = automata()
    aut_of_row = np.where(kind == 6, 0, np.where(kind == 9, 1, -1))
    state = np.where(aut_of_row >= 0, np.asarray(first)[np.maximum(aut_of_row, 0)], np.where(kind == 8, DEAD, NONE)).astype(np.int32)
    weight = np.stack([a.bias(0) for a in auts] + [np.zeros(V, np.float32)])          # [-1]: no automaton / dead
    seen = rs.rand(R, V) < 0.5
    seen[:, CORNERS + [150, 210]] = True
    seen[:, [100, 200, 37]] = False
    seen[np.isin(kind, [0, 1, 3, 5, 6]), 100] = True
    seen[np.isin(kind, [0, 2]), 200] = True
    seen[kind == 3, 37] = True
    p = P_OF_KIND[kind]
    ld = 2
    prefix = np.stack([np.array([100, V - 1, 255, 150])[r_ % 4], np.array([37, 31, 200, 64])[(r_ // 4) % 4]], 1).astype(np.int32)
    plen = (r_ % 3).astype(np.int32)
    step = (np.arange(M) % 2).astype(np.int32)
    has_tgt = step < plen[rows]
    target = np.where(has_tgt, prefix[rows, step], -1)

    c = types.SimpleNamespace(tile=tile, M=M, R=R, Mp=Mp, nt=nt, rowmap=rowmap, kind=kind, A=A, W=W, bias=bias, logits=logits, masks=masks,
                              set_of_row=set_of_row, state=state, aut_of_row=aut_of_row, weight=weight, tables=(eb, et, ew), seen=seen, p=p,
                              ld=ld, prefix=prefix, plen=plen, step=step, has_tgt=has_tgt, target=target, refs={})

    # ---- what the case proves, on the reference
    k_of, mask = kind[rows], masks[set_of_row[rows]]
    for t0 in range(0, M, tile):
        sl = np.arange(t0, min(t0 + tile, M))
        assert (k_of[sl] != kind[sl]).any(), "a kernel reading a by-ROW array by slot must fail in every M-tile"
        assert (k_of[sl] != kind[sl - t0]).any(), "... and one reading it by the slot within the tile"
        if sl.size == tile:
            assert (step[sl] != rows[sl] % 2).any(), "a kernel reading the step by row must fail"
            assert set(k_of[sl].tolist()) == set(range(NK)), "every kind in every full M-tile"
            assert {0, 1, 2} == set(set_of_row[rows[sl]].tolist()) and has_tgt[sl].any() and not has_tgt[sl].all()
    pl = mirror_values(c, "pen", True).astype(np.float64)
    win, free = np.argmax(cu.masked(pl, mask), -1), np.argmax(cu.masked(logits64, mask), -1)
    assert (free[k_of != 5] == 100).all()
    assert (win[k_of == 0] == 37).all() and (pl[k_of == 0][:, 100] == 25.0).all(), "kind 0: a tie made by the penalty, the lower column"
    assert (win[k_of == 1] == 200).all() and (win[k_of == 3] == 200).all()
    assert (win[k_of == 2] == 100).all() and (pl[k_of == 2][:, 200] == 50.0).all(), "kind 2: p < 1 lifts 200 to a tie, the lower column"
    assert (win[k_of == 4] == 100).all() and (win[k_of == 5] == 200).all() and not mask[k_of == 5][:, 100].any()
    assert (win[k_of == 6] == 100).all() and (pl[k_of == 6][:, 100] == 41.0).all(), "kind 6: (50 + 32) / 2, not 50 / 2 + 32"
    assert (win[np.isin(k_of, [7, 8])] == 100).all() and (win[k_of == 9] == 200).all() and 100 // tile != 200 // tile
    assert (pl[:, 150] == 0.0).all() and (pl[k_of == 0][:, 210] == -60.0).all() and (pl[k_of == 2][:, 210] == -24.0).all()
    wl = mirror_values(c, "soft", True).astype(np.float64)
    wwin = np.argmax(cu.masked(wl, mask), -1)
    assert (wwin[k_of == 9] == 200).all() and (wwin[k_of == 6] == 100).all() and (wl[k_of == 6][:, 100] == 82.0).all()
    assert (state[rows][k_of == 8] == DEAD).all() and (state[rows][k_of < 6] == NONE).all() and (state[rows][np.isin(k_of, [6, 9])] >= 0).all()
    assert seen[:, CORNERS].all() and not masks[1:, BANNED_CORNERS].any() and (set_of_row[rows] != 0).any()
    # the targets: seen with p != 1, outside the row's set, none at all, weighted
    tm = np.nonzero(has_tgt)[0]
    assert any(seen[rows[m], target[m]] and p[rows[m]] != 1 for m in tm), "a seen target column"
    assert any(not mask[m, target[m]] for m in tm) and any(mask[m, target[m]] for m in tm) and not has_tgt.all()
    assert any(weight[aut_of_row[rows[m]], target[m]] != 0 for m in tm), "a target column that carries a weight"
    # the ragged tile's one row: mask, weight, penalty and target all act - each of them changes what the row's tiles hold
    m = M - 1
    assert rows[m] == RAGGED_ROW and kind[rows[m]] == 6 and set_of_row[rows[m]] == 2 and target[m] == 100 and mask[m, 100]
    full = cu.masked_tile_stats(pl[m], mask[m], tile)[0]
    for what, other in (("mask", cu.masked_tile_stats(pl[m], True, tile)[0]),
                        ("weight", cu.masked_tile_stats(mirror_values(c, "pen", False)[m].astype(np.float64), mask[m], tile)[0]),
                        ("penalty", cu.masked_tile_stats(wl[m], mask[m], tile)[0])):
        assert (full != other).any(), f"the {what} does not act on the ragged tile's row"
    return c


def mirror_values(c, rich: str, tables: bool) -> np.ndarray:
    """float32 [M, V]: what the epilogue compares - logit (+ the row's edge weights) (then penalised where seen), unmasked"""
    rows = c.rowmap
    val = c.logits
    if rich != "plain" and tables:
        v64 = val.astype(np.float64) + c.weight[c.aut_of_row[rows]]
        val = v64.astype(np.float32)
        assert (val == v64).all(), "logit + weight is not exact in fp32"
    if rich == "pen":
        val = pu.pen32(val, c.seen[rows], c.p[rows][:, None])
        assert np.isfinite(val).all()
    return val


def reference(c, masked: bool, rich: str, tables: bool = True):
    """the mirror of one (masked, rich, tables) at the case's tile, computed once: tile maxima, their (lowest) columns, the four
    best with NO_IDX where -inf, tgt_val (NaN = not written), the float64 logsumexp over the allowed columns and its tolerance,
    8 x max(the fp32 logsumexp's own error, the spacing of the reference) - tests/test_gpu_constraints.py's exact-input rule"""
    from test_gpu_constraints import lex_top
    key = (masked, rich, tables)
    if key in c.refs:
        return c.refs[key]
    M, nt, tile = c.M, c.nt, c.tile
    val = mirror_values(c, rich, tables)
    mask = c.masks[c.set_of_row[c.rowmap]] if masked else np.ones((M, V), bool)
    v64 = val.astype(np.float64)
    m64, idx64, _ = cu.masked_tile_stats(v64, mask, tile)
    t3 = cu.masked(v64, mask).reshape(M, nt, tile)
    tile_lo = (np.arange(nt) * tile)[None, :, None]
    top_i = lex_top(t3) + tile_lo
    top_v = np.take_along_axis(t3, top_i - tile_lo, -1)
    top_i = np.where(np.isneginf(top_v), NO_IDX, top_i)
    tgt = np.full(M, np.nan)
    for m in np.nonzero(c.has_tgt)[0]:
        tgt[m] = v64[m, c.target[m]] if mask[m, c.target[m]] else -np.inf
    lse = su.lse64(t3.reshape(M, V))
    e32 = su.f32_lse_error(np.where(mask, val, -1e30).astype(np.float32))
    tol = 8 * np.maximum(e32, np.spacing(np.abs(lse).astype(np.float32)).astype(np.float64))
    ref = types.SimpleNamespace(cand_val=m64, cand_idx=idx64, top_val=top_v, top_idx=top_i, tgt=tgt, lse=lse, tol=tol)
    c.refs[key] = ref
    return ref
