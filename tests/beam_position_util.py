"""Numpy restatement of the beam-index trail and the float64 reference of the hypotheses' token positions
(tests/test_beam_positions_cpu.py, tests/test_gpu_beam_position*.py; include/mocr.h, "beam search with token positions").

The trail.  ``trail[k][t]``, t >= 1, of a running beam is the beam 0 .. K - 1 whose ROW ran the step that appended token t
of its history (entry 0, the start token's, is 0): transformers' ``beam_indices``, relative to the crop's group.  It travels
with the history - the new beam k inherits its parent's trail and appends the parent - and ``hyp_trail[j]`` travels with the
finished hypothesis j.  The step is tests/beam_util.py's (or tests/beam_token_util.py's) own, wrapped: the wrapper looks at
the state before and behind it, so nothing of the selection is restated here.

What a row recorded.  ``Recorder`` keeps, per step s, the history every row held when it ran that step.  The row that ran
step t - 1 for hypothesis h is ``trail[t]``, and what that row recorded there is a function of the history it held - so the
trail is right exactly when ``hist[t - 1][trail[t]] == h[:t]`` for every 1 <= t < len(h) (``replay``)."""
import numpy as np

import beam_util as bu
import position_util as pu

# The published configuration at max_len 24 on the position tests' weights (position_util.G, EOS_BIAS, WEIGHT_SEED) and
# crops (CROP_SEED): chosen values, checked by tests/test_beam_positions_cpu.py::test_the_inputs_tell_a_dropped_trail - with
# them the float64 search returns hypotheses whose trail is not constant and whose fields, taken from their own row's
# recordings instead, are off by more than 10 x BF16_CXY_TOL.  (The defaults of position_util satisfy it: nothing overridden.)
G, EOS_BIAS, WEIGHT_SEED, CROP_SEED = pu.G, pu.EOS_BIAS, pu.WEIGHT_SEED, pu.CROP_SEED
MAX_LEN = 24
PUBLISHED = (4, 2.0, True, 3)


class Trails:
    """the trails of one crop's running beams and finished set, beside a beam_util / beam_token_util State"""

    def __init__(self, K):
        self.trail = [[0] for _ in range(K)]
        self.hyp_trail = [[] for _ in range(K)]


class Recorder:
    """per step, the history every row held when it ran it"""

    def __init__(self):
        self.hist = []

    def record(self, st):
        self.hist.append([list(s) for s in st.seqs])


def step(acc, st, tr, cfg, max_len, eos=bu.EOS, base=bu.step):
    """``base`` (beam_util.step, or beam_token_util.step on its own input) with the trails moved beside it.  The old finished
    hypotheses are recognised as the very list objects the step keeps; the new ones are the stopped candidates among the first
    K in candidate order (equal scores: the old entry first, the candidates in order - a stable sort), of which the step can
    only have dropped the last."""
    K = cfg.K
    old_seqs, old_hyp = st.seqs, list(st.hyp_seq)
    old_of = {id(h): tr.hyp_trail[j] for j, h in enumerate(old_hyp)}
    out = base(acc, st, cfg, max_len, eos)
    cpar, ctok, stop = out[1], out[2], out[3]
    new_trail = [tr.trail[p] + [int(p)] for p in st.parents]
    for k, p in enumerate(st.parents):
        assert st.seqs[k][:-1] == old_seqs[p], "a new beam continues its parent's history"
    stopped = [i for i in range(K) if stop[i]]
    hyp_trail, used = [], 0
    for h in st.hyp_seq:
        if id(h) in old_of:
            hyp_trail.append(old_of[id(h)])
        else:
            i = stopped[used]
            used += 1
            assert h == old_seqs[cpar[i]] + [int(ctok[i])]
            hyp_trail.append(tr.trail[cpar[i]] + [int(cpar[i])])
    tr.trail, tr.hyp_trail = new_trail, hyp_trail
    return out


def replay(hyp, trail, hist):
    """does walking ``trail`` through the recorded histories give back the hypothesis?"""
    if len(hyp) != len(trail):
        return False
    return all(hist[t - 1][trail[t]] == list(hyp[:t]) for t in range(1, len(hyp)))


def beam_generate(o, enc, cfg, max_len):
    """beam_util.beam_generate with the trails: -> (ids, lens, scores float64, trails int [n, K, max_len] (0 behind a length),
    info) with info["hist"][c] the crop's Recorder.hist"""
    import torch
    sp = o.spec
    K = cfg.K
    states, all_tr, hists = [], [], []
    with torch.no_grad():
        for c in range(enc.shape[0]):
            ckv = o.cross_kv(enc[c:c + 1].repeat(K, 1, 1))
            self_kv = [None] * sp.dec_layers
            st, tr, rec = bu.State(K, sp.start_id), Trails(K), Recorder()
            t = 0
            while not st.done:
                rec.record(st)
                tok = torch.tensor([s[-1] for s in st.seqs], dtype=torch.int64)
                logits = o.decode_step(tok, t, self_kv, ckv).numpy()
                step(bu.accumulate(logits, st, cfg), st, tr, cfg, max_len, sp.eos_id)
                idx = torch.tensor(st.parents, dtype=torch.int64)
                self_kv = [(k.index_select(0, idx), v.index_select(0, idx)) for k, v in self_kv]
                t += 1
            states.append(st)
            all_tr.append(tr)
            hists.append(rec.hist)
    ids, lens, scores = bu.result_block(states, K, max_len, sp.pad_id)
    trails = np.zeros((len(states), K, max_len), np.int64)
    for c, tr in enumerate(all_tr):
        for j in range(K):
            trails[c, j, :len(tr.hyp_trail[j])] = tr.hyp_trail[j]
    return ids, lens, scores, trails, {"states": states, "hist": hists, "min_gap": np.array([s.min_gap for s in states])}


def reference_fields(o, enc, ids, lens):
    """float64 [n, K, L, 5]: position_util.reference_for_ids of every hypothesis, teacher-forced on its own ids over its crop's
    encoding (one oracle pass over the n K rows); 0 for empty slots"""
    n, K, L = ids.shape
    rows_enc = enc.repeat_interleave(K, dim=0)
    flat_lens = np.asarray(lens).reshape(-1)
    ref = pu.reference_for_ids(o, None, np.asarray(ids).reshape(n * K, L), np.maximum(flat_lens, 1), enc=rows_enc)
    ref[flat_lens == 0] = 0.0
    return ref.reshape(n, K, L, pu.FIELDS)


def own_row_fields(o, enc_c, j, length, hist):
    """float64 [length, 5]: the fields hypothesis slot j of one crop would get with the trail DROPPED - token t from what row j
    itself recorded at step t - 1, i.e. from the history hist[t - 1][j] that row held (enc_c: the crop's encoding [1, S, D])"""
    out = np.zeros((length, pu.FIELDS), np.float64)
    if length < 2:
        return out
    # one teacher-forced row per token t: the t tokens row j held at step t - 1, padded (the decoder is causal: the fields of
    # token t, from the step that consumed position t - 1, see nothing behind it)
    block = np.zeros((length - 1, length), np.int64)
    for t in range(1, length):
        assert len(hist[t - 1][j]) == t
        block[t - 1, :t] = hist[t - 1][j]
    ref = pu.reference_for_ids(o, None, block, [t + 1 for t in range(1, length)], enc=enc_c.repeat(length - 1, 1, 1))
    for t in range(1, length):
        out[t] = ref[t - 1, t]
    return out
