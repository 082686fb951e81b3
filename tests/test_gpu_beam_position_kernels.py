"""-m gpu: the two kernels behind the token positions of beam hypotheses, through their operator hooks.

* beam_select_kernel in its trail form (mocr_op_beam_select_positions): six consecutive steps of two crops (plus a trailing
  partial group of padding slots) on hand-made logits that move the lead from row to row and finish a hypothesis ahead of an
  existing one.  After every step beam_trail / hyp_trail equal the numpy restatement (tests/beam_position_util.py) exactly,
  and every other output is bit-identical to mocr_op_beam_select_tokens run beside it on the same inputs; with null trails
  the hook IS mocr_op_beam_select_tokens, and the trails beside the plain form leave mocr_op_beam_select's outputs alone.
* attn_positions_kernel in its gathered-query form (mocr_op_attn_positions_gathered): random trails and lengths, 0 and 1
  among them, against position_util.ref_positions on the gathered queries within the kernel tolerance of
  tests/test_gpu_positions.py (the arithmetic is that kernel's, only the query's address is new); a null trail gives
  mocr_op_attn_positions bit for bit."""
import numpy as np
import pytest

import beam_position_util as bp
import beam_token_util as tu
import beam_util as bu
import position_util as pu
from gpu_util import bf16_round, engine, report
from test_gpu_beam_kernels import D, EOS, GUARD, LD, MAX_LEN, ML, PAD, SENT, START, V, _f32, _i32
from test_gpu_positions import KERNEL_TOL

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STEPS = 6
TSENT = 0xEE                        # what the trails' guard row holds
LSENT = -777.0


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).cuda()


# ------------------------------------------------------------------------------------------------ the selection
def step_logits(rs, K, s, crop):
    """logits [K, V] of one crop at step s (multiples of 1/64; noise in [-8, -4)).  Every beam gets 2 K + 2 tokens of its own
    (the 2 K + 1 best candidates are planted ones, never two equal noise values); the beam (s + 1 + crop) % K gets the
    strongest, so the lead changes rows from step to step.  EOS on the leading beam: at step 2 just below its best token (a
    first hypothesis), at step 4 well above everything (a hypothesis that scores above the first and is inserted ahead of
    it)."""
    lg = rs.randint(-512, -256, (K, V)).astype(np.float64) / 64.0
    lead = (s + 1 + crop) % K
    for k in range(K):
        first = 200 + 100 * s + 12 * k
        for j in range(2 * K + 2):
            lg[k, first + j] = 3.0 - 0.5 * j - 0.125 * k + (2.5 if k == lead and j == 0 else 0.0)
    if s == 2:
        lg[lead, EOS] = 5.0
    if s == 4:
        lg[lead, EOS] = 9.0
    return lg


def reference_walk(K, seed):
    """the float64 search of two crops over STEPS steps with the trails: per step the logits [2, K, V] and a snapshot of
    (state, trails) behind it"""
    rs = np.random.RandomState(seed)
    cfg = bu.Config(K, 1.0, False, 0)
    sts = [tu.State(K, START) for _ in range(2)]
    trs = [bp.Trails(K) for _ in range(2)]
    walk = []
    for s in range(STEPS):
        lg = np.stack([step_logits(rs, K, s, c) for c in range(2)])
        for c in range(2):
            if not sts[c].done:
                bp.step(tu.processed(lg[c], sts[c], cfg), sts[c], trs[c], cfg, ML, EOS, base=tu.step)
        walk.append((lg, [st.copy() for st in sts], [(list(map(list, tr.trail)), list(map(list, tr.hyp_trail))) for tr in trs]))
    return cfg, walk


class Device:
    """the arrays of the launches, as tests/test_gpu_beam_kernels.py lays them out: two groups of K slots and one padding
    slot; rows: the two crops in permuted places, one crop nobody decodes, a guard row behind every [rows][LD] array"""

    def __init__(self, K, dtype, crop_of):
        self.K, self.n, self.R = K, 2 * K + 1, 3 * K
        n, R = self.n, self.R
        rowmap = np.zeros(n, np.int32)
        ids = np.full((R + 1, LD), SENT, np.int32)
        bscore = np.full(R, -5.5, np.float32)
        for g, c in enumerate(crop_of):
            for k in range(K):
                rowmap[g * K + k] = c * K + k
                ids[c * K + k, 0] = START
                bscore[c * K + k] = 0.0 if k == 0 else -bu.NEG
        self.spare = [r for r in range(R) if r // K not in crop_of]
        rowmap[2 * K:] = self.spare[-1]
        step = np.zeros(n, np.int32)
        step[2 * K:] = 7
        hl = np.zeros((R + 1, LD), np.float32)
        hl[R] = LSENT
        bl = np.full((R + 1, LD), LSENT, np.float32)
        bl[:R, 0] = 0.0
        tr = np.zeros((R + 1, LD), np.uint8)
        tr[R] = TSENT
        tr[self.spare] = TSENT                          # rows of the crop nobody decodes: never written
        self.trail0 = tr
        self.d = dict(ids=_i32(ids), step=_i32(step), fin=_i32(np.zeros(R)), len=_i32(np.full(R, ML)), unf=_i32([1000, SENT]),
                      rowmap=_i32(rowmap), parent=_i32(np.full(R, SENT)), hyp_ids=_i32(np.full((R + 1, LD), PAD)), hyp_len=_i32(np.zeros(R)),
                      hopen=_i32(np.ones(3)), bscore=_f32(bscore), hyp_score=_f32(np.full(R, -bu.NEG)), blogp=_f32(bl), hlogp=_f32(hl),
                      btrail=_u8(tr), htrail=_u8(tr))
        tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        self.x32 = torch.full((n + GUARD, D), float("nan"), device="cuda")
        self.xt = torch.full((n + GUARD, D), float("nan"), device="cuda", dtype=tdt)
        self.cache = torch.full((R, MAX_LEN, D), float("nan"), device="cuda", dtype=tdt)
        self.bits = torch.int16 if dtype == "bf16" else torch.int32

    def launch(self, eng, bcfg, parts, bias, form):
        d = self.d
        kw = dict(first=0, n=self.n, slabs=parts, nslab=parts.shape[0], vbias=bias, ids=d["ids"], step=d["step"], finished=d["fin"], len=d["len"],
                  n_unfinished=d["unf"], rowmap=d["rowmap"], ids_ld=LD, max_len=ML, n_real=2 * self.K, x_f32=self.x32, x_t=self.xt, cache=self.cache)
        state = (d["bscore"], d["parent"], d["hyp_ids"], d["hyp_len"], d["hyp_score"], d["hopen"])
        if form == "plain":
            eng.op_beam_select(bcfg, *state, **kw)
        elif form == "tokens":
            eng.op_beam_select_tokens(bcfg, *state, d["blogp"], d["hlogp"], **kw)
        elif form == "positions, null trails":
            eng.op_beam_select_positions(bcfg, *state, d["blogp"], d["hlogp"], **kw)
        elif form == "plain + trails":
            eng.op_beam_select_positions(bcfg, *state, d_beam_trail=d["btrail"], d_hyp_trail=d["htrail"], **kw)
        else:
            eng.op_beam_select_positions(bcfg, *state, d["blogp"], d["hlogp"], d_beam_trail=d["btrail"], d_hyp_trail=d["htrail"], **kw)

    def read(self):
        got = {k: v.cpu().numpy() for k, v in self.d.items()}
        for k in ("bscore", "hyp_score", "blogp", "hlogp"):
            got[k] = got[k].view(np.int32)
        got["x32"], got["xt"], got["cache"] = self.x32.cpu().numpy().view(np.int32), self.xt.view(self.bits).cpu().numpy(), self.cache.view(self.bits).cpu().numpy()
        return got


FORMS = ["positions", "tokens", "positions, null trails", "plain + trails", "plain"]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_the_trails_follow_six_steps(K, dtype):
    from manga_ocr.engine import BeamConfig
    eng = engine(dtype)
    cfg, walk = reference_walk(K, 4000 + K)
    bcfg = BeamConfig(K, 1.0, False, 0)
    rs = np.random.RandomState(5000 + K)
    crop_of = [2, 0]                                    # group 0 holds crop 2's rows, group 1 crop 0's; crop 1 is nobody's
    devs = {f: Device(K, dtype, crop_of) for f in FORMS}
    swaps = ahead = 0
    want_b, want_h = devs["positions"].trail0.copy(), devs["positions"].trail0.copy()
    for s, (lg, sts, trs) in enumerate(walk):
        n = 2 * K + 1
        logits = rs.randint(-512, -256, (n, V)).astype(np.float64) / 64.0
        logits[:2 * K] = lg.reshape(2 * K, V)
        bias = rs.randint(-128, 128, V).astype(np.float64) / 64.0
        parts = rs.randint(-128, 128, (2, n, V)).astype(np.float64) / 64.0
        parts[-1] = logits - bias - parts[0]
        d_parts, d_bias = _f32(parts), _f32(bias)
        torch.cuda.synchronize()
        for f in FORMS:
            devs[f].launch(eng, bcfg, d_parts, d_bias, f)
        got = {f: devs[f].read() for f in FORMS}
        # every other output: bit-identical to the token form (the plain form beside its own trails: to the plain form)
        for a, b in (("positions", "tokens"), ("positions, null trails", "tokens"), ("plain + trails", "plain")):
            for k in got[a]:
                if k not in ("btrail", "htrail"):
                    np.testing.assert_array_equal(got[a][k], got[b][k], err_msg=f"step {s}: {k} of '{a}' against '{b}'")
        for f in ("tokens", "positions, null trails", "plain"):
            assert np.array_equal(got[f]["btrail"], devs[f].trail0) and np.array_equal(got[f]["htrail"], devs[f].trail0), f"'{f}' writes no trail"
        np.testing.assert_array_equal(got["plain + trails"]["btrail"], got["positions"]["btrail"])
        np.testing.assert_array_equal(got["plain + trails"]["htrail"], got["positions"]["htrail"])
        # the trails, and the histories they belong to, against the numpy restatement
        g = got["positions"]
        for c_ref, c in enumerate(crop_of):
            st, (trail, hyp_trail) = sts[c_ref], trs[c_ref]
            assert st.min_gap >= 1e-3, f"a constructed step has candidates {st.min_gap} apart"
            for k in range(K):
                r = c * K + k
                if not st.done:         # (a crop that ends keeps its rows - ids and trails - as they were: only the finished set moves)
                    np.testing.assert_array_equal(g["ids"][r, :s + 2], st.seqs[k], err_msg=f"step {s} crop {c} beam {k}")
                    want_b[r, :s + 2] = trail[k]
                n_h = len(st.hyp_seq[k])
                assert g["hyp_len"][r] == n_h
                np.testing.assert_array_equal(g["hyp_ids"][r, :n_h], st.hyp_seq[k])
                want_h[r] = 0
                want_h[r, :n_h] = hyp_trail[k]
            swaps += st.parents != list(range(K))
            lens = [len(h) for h in st.hyp_seq if h]
            ahead += any(a > b for a, b in zip(lens, lens[1:]))
        np.testing.assert_array_equal(g["btrail"], want_b, err_msg=f"step {s}: beam_trail")
        np.testing.assert_array_equal(g["htrail"], want_h, err_msg=f"step {s}: hyp_trail")
    assert swaps >= 6 and ahead >= 1, "the walk swaps parents and inserts a hypothesis ahead of an existing one"
    final = [t for trail, _ in walk[-1][2] for t in trail]
    assert any(len(set(t[1:])) > 1 for t in final), "a running beam changed rows"
    report(f"beam_select trails {dtype} K={K}: {STEPS} steps x 2 crops + a partial group, {swaps} parent swaps, hypotheses inserted ahead: "
           f"beam_trail / hyp_trail exact; every other output bit-identical to the token / plain form; null trails are the token form")


def test_one_trail_without_the_other_is_refused():
    from manga_ocr._capi import MocrError
    from manga_ocr.engine import BeamConfig
    eng = engine("fp32")
    dev = Device(2, "fp32", [2, 0])
    parts, bias = _f32(np.zeros((1, 5, V))), _f32(np.zeros(V))
    d = dev.d
    kw = dict(first=0, n=dev.n, slabs=parts, nslab=1, vbias=bias, ids=d["ids"], step=d["step"], finished=d["fin"], len=d["len"],
              n_unfinished=d["unf"], rowmap=d["rowmap"], ids_ld=LD, max_len=ML, n_real=4, x_f32=dev.x32, x_t=dev.xt, cache=dev.cache)
    before = dev.read()
    with pytest.raises(MocrError):
        eng.op_beam_select_positions(BeamConfig(2), d["bscore"], d["parent"], d["hyp_ids"], d["hyp_len"], d["hyp_score"], d["hopen"],
                                     d_beam_trail=d["btrail"], **kw)
    after = dev.read()
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)


# ------------------------------------------------------------------------------------------------ the gathered positions
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_gathered_positions_against_float64(dtype):
    """K = 4, two groups, T = 20 (two tiles of positions, the second partial), lengths 0 and 1 among them.  Row r's position p
    reads the query of row (r / 4) * 4 + trail[r][p + 1]; the float64 reference is given the gathered queries.  Trail entries
    behind a row's length hold 255: nothing may read them as a row."""
    K, G, T = 4, 2, 20
    rows = K * G
    eng = engine(dtype)
    rng = np.random.RandomState(77)
    q = rng.standard_normal((rows, T, 768)).astype(np.float32)
    Km = rng.standard_normal((rows, 197, 768)).astype(np.float32)
    if dtype == "bf16":
        q, Km = bf16_round(q), bf16_round(Km)
    lens = np.array([20, 0, 1, 7, 16, 17, 20, 3], np.int32)
    trail = rng.randint(0, K, size=(rows, T + 1)).astype(np.uint8)
    for r in range(rows):
        trail[r, lens[r] + 1:] = 255
    gathered = np.zeros_like(q)
    for r in range(rows):
        for p in range(lens[r]):
            gathered[r, p] = q[r // K * K + trail[r, p + 1], p]
    assert any((trail[r, 1:lens[r] + 1] != r % K).any() for r in range(rows))
    ref_map, ref_f = pu.ref_positions(gathered, Km, lens)
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    d_q, d_k = torch.from_numpy(q).cuda().to(tdt), torch.from_numpy(Km).cuda().to(tdt)
    d_len, d_trail = torch.from_numpy(lens).cuda(), _u8(trail)
    d_pos = torch.full((rows, T, 5), float("nan"), device="cuda")
    d_map = torch.full((rows, T, 197), float("nan"), device="cuda")
    eng.op_attn_positions_gathered(d_q, d_k, d_len, rows, T, d_pos, d_map, d_trail, T + 1, K)
    got_f, got_map = d_pos.cpu().numpy().astype(np.float64), d_map.cpu().numpy().astype(np.float64)
    assert np.isfinite(got_f).all() and np.isfinite(got_map).all()
    for r in range(rows):
        assert (got_f[r, lens[r]:] == 0).all() and (got_map[r, lens[r]:] == 0).all(), f"row {r}: behind d_len"
    e_map, e_f = float(np.abs(got_map - ref_map).max()), float(np.abs(got_f - ref_f).max())
    own_map, own_f = pu.ref_positions(q, Km, lens)
    report(f"attn_positions gathered {dtype}: {rows} rows of {G} groups, T {T}: max |map - f64| {e_map:.2e}, max |fields - f64| {e_f:.2e} "
           f"(tol {KERNEL_TOL:.1e}); the rows' own queries would be {np.abs(own_f - ref_f).max():.2e} away")
    assert e_map <= KERNEL_TOL and e_f <= KERNEL_TOL
    assert np.abs(own_f - ref_f).max() > 1e3 * KERNEL_TOL, "the inputs tell a gathered query from the row's own"
    # a null trail: mocr_op_attn_positions, bit for bit
    a_pos, b_pos = torch.full((rows, T, 5), float("nan"), device="cuda"), torch.full((rows, T, 5), float("nan"), device="cuda")
    a_map, b_map = torch.full((rows, T, 197), float("nan"), device="cuda"), torch.full((rows, T, 197), float("nan"), device="cuda")
    eng.op_attn_positions(d_q, d_k, d_len, rows, T, a_pos, a_map)
    eng.op_attn_positions_gathered(d_q, d_k, d_len, rows, T, b_pos, b_map)
    np.testing.assert_array_equal(a_pos.cpu().numpy().view(np.int32), b_pos.cpu().numpy().view(np.int32))
    np.testing.assert_array_equal(a_map.cpu().numpy().view(np.int32), b_map.cpu().numpy().view(np.int32))
    # an identity trail: the same again
    ident = np.tile((np.arange(rows) % K).astype(np.uint8)[:, None], (1, T + 1))
    eng.op_attn_positions_gathered(d_q, d_k, d_len, rows, T, b_pos, b_map, _u8(ident), T + 1, K)
    np.testing.assert_array_equal(a_pos.cpu().numpy().view(np.int32), b_pos.cpu().numpy().view(np.int32))


def test_gathered_positions_refuse_partial_groups_and_short_trails():
    from manga_ocr._capi import MocrError
    eng = engine("fp32")
    q, k = torch.zeros((6, 4, 768), device="cuda"), torch.zeros((6, 197, 768), device="cuda")
    ln, out = torch.ones(6, dtype=torch.int32, device="cuda"), torch.zeros((6, 4, 5), device="cuda")
    tr = torch.zeros((6, 5), dtype=torch.uint8, device="cuda")
    for rows, ld, K in ((6, 5, 4), (6, 4, 3), (6, 5, 5), (6, 5, 0)):
        with pytest.raises(MocrError):
            eng.op_attn_positions_gathered(q, k, ln, rows, 4, out, None, tr, ld, K)
    eng.op_attn_positions_gathered(q, k, ln, 6, 4, out, None, tr, 5, 3)
