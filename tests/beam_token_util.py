"""Float64 / numpy reference of beam search under token sets, with per-token log-probabilities (tests/test_beam_tokens_cpu.py,
tests/test_gpu_beam_token*.py): tests/beam_util.py's step restated with the two additions of include/mocr.h, "beam search with
token sets and token scores".

  log_softmax over the FULL row -> -inf for every token outside the crop's set and for the beam's own n-gram bans (the order
  does not matter, nothing renormalises: transformers' PrefixConstrainedLogitsProcessor and NoRepeatNGramLogitsProcessor) ->
  + the beam's running score -> beam_util's selection.

The processed log-probability of the token a candidate appends travels with its history: ``logp[k]`` of a running beam and
``hyp_logp[j]`` of a finished hypothesis hold one value per token, 0 for the start token - transformers'
``compute_transition_scores(sequences, scores, beam_indices, normalize_logits=False)``.

DEAD CANDIDATES.  With a small set fewer than 2 K of the K V accumulated scores can be finite.  A -inf candidate is dead: it
sorts behind every finite one, among -inf candidates the LOWER FLAT INDEX beam * V + token goes first (the stable sort below;
torch.topk promises no order among equals, so tests compare nothing of a dead candidate but the range of its token), it never
enters the finished set (-inf < the empty slots' -1e9), and a running beam that is dead keeps score -inf."""
import numpy as np

import beam_util as bu
import ngram_util as ngu

V, EOS, NEG = bu.V, bu.EOS, bu.NEG


class State(bu.State):
    """beam_util's state of one crop plus the token log-probabilities of the running beams and of the finished set"""

    def __init__(self, K, start_id):
        super().__init__(K, start_id)
        self.logp = [[0.0] for _ in range(K)]
        self.hyp_logp = [[] for _ in range(K)]


def processed(logits, st, cfg, mask=None):
    """logits [K, V] of the running beams -> the processed log-probabilities [K, V] float64: log_softmax over the full row,
    then -inf outside ``mask`` (bool [V], None: everything allowed) and on each beam's own n-gram bans"""
    lp = bu.log_softmax64(logits)
    if mask is not None:
        lp[:, ~np.asarray(mask, bool)] = -np.inf
    for k in range(cfg.K):
        ban = ngu.banned_tokens(st.seqs[k], cfg.ngram)
        if ban:
            lp[k, np.asarray(ban, np.int64)] = -np.inf
            st.n_banned += len(ban)
    return lp


def step(lp, st, cfg, max_len, eos=EOS):
    """One selection on the processed log-probabilities [K, V] of a live crop: beam_util.step on lp + running score, with the
    log-probability histories moved as the id histories are.  Returns (scores [2K], parents, tokens, stopped, lps [2K])."""
    K = cfg.K
    assert not st.done
    with np.errstate(invalid="ignore"):
        acc = np.asarray(lp, np.float64) + st.run[:, None]
    acc[np.isnan(acc)] = -np.inf
    cur = len(st.seqs[0])
    flat = acc.reshape(-1)
    order = np.argsort(-flat, kind="stable")[:2 * K + 1]       # (-inf last, the lower flat index first among them)
    gap = bu._gap(flat[order])
    order = order[:2 * K]
    cv, cpar, ctok = flat[order], order // acc.shape[1], order % acc.shape[1]
    clp = np.asarray(lp, np.float64)[cpar, ctok]
    clp = np.where(np.isfinite(cv), clp, -np.inf)               # the child of a dead beam is dead whatever its token
    stop = (ctok == eos) | (cur + 1 >= max_len)
    adj = cv - NEG * stop
    pick = np.argsort(-adj, kind="stable")[:K]                  # by value: a dead candidate ranks behind a stopped one's - 1e9
    new_seqs = [st.seqs[cpar[i]] + [int(ctok[i])] for i in pick]
    new_logp = [st.logp[cpar[i]] + [float(clp[i])] for i in pick]
    new_run = adj[pick]
    parents = [int(cpar[i]) for i in pick]
    filled = [len(s) > 0 for s in st.hyp_seq]
    full_guard = all(filled) and cfg.es == 1
    entries = [(st.hyp_score[j], st.hyp_seq[j], st.hyp_logp[j]) for j in range(K)]
    for i in range(K):
        if stop[i]:
            s = cv[i] / (float(cur) ** cfg.lp)
            if full_guard or not st.open:
                s -= NEG
            entries.append((s, st.seqs[cpar[i]] + [int(ctok[i])], st.logp[cpar[i]] + [float(clp[i])]))
    keep = np.argsort(-np.array([e[0] for e in entries]), kind="stable")[:K]
    merged_real = sorted([e[0] for e in entries if len(e[1]) > 0 and np.isfinite(e[0])], reverse=True)
    gap = min(gap, bu._gap(merged_real))
    st.hyp_score = np.array([entries[j][0] for j in keep], np.float64)
    st.hyp_seq = [entries[j][1] for j in keep]
    st.hyp_logp = [entries[j][2] for j in keep]
    assert all(np.isfinite(s) for s in st.hyp_score), "a dead candidate never enters the finished set"
    st.seqs, st.logp, st.run, st.parents = new_seqs, new_logp, new_run, parents
    st.min_gap = min(st.min_gap, gap)
    cur2 = cur + 1
    hyp_len = (max_len - 1) if (cfg.es == 2 and cfg.lp > 0.0) else (cur2 - 1)
    best_possible = st.run[0] / (float(hyp_len) ** cfg.lp)
    filled = [len(s) > 0 for s in st.hyp_seq]
    worst = [st.hyp_score.min() if f else -NEG for f in filled]
    st.open = st.open and any(best_possible > w for w in worst)
    st.done = (not st.open) or (all(filled) and cfg.es == 1) or bool(np.all(stop))
    return cv, cpar, ctok, stop, clp


def result_block(states, K, ld, pad_id=0):
    """the engine's output layout: beam_util.result_block plus logp float64 [n, K, ld], 0 behind a length and in empty slots"""
    ids, lens, scores = bu.result_block(states, K, ld, pad_id)
    logp = np.zeros((len(states), K, ld), np.float64)
    for c, st in enumerate(states):
        for j in range(K):
            logp[c, j, :len(st.hyp_logp[j])] = st.hyp_logp[j]
    return ids, lens, scores, logp


def beam_generate(o, enc, cfg, max_len, masks=None):
    """beam_util.beam_generate under per-crop token sets ``masks`` (bool [n, V], EOS a member of every row; None: no sets):
    -> (ids, lens, scores, logp float64 [n, K, max_len], info)"""
    import torch
    sp = o.spec
    K = cfg.K
    states, steps = [], []
    with torch.no_grad():
        for c in range(enc.shape[0]):
            ckv = o.cross_kv(enc[c:c + 1].repeat(K, 1, 1))
            self_kv = [None] * sp.dec_layers
            st = State(K, sp.start_id)
            t = 0
            while not st.done:
                tok = torch.tensor([s[-1] for s in st.seqs], dtype=torch.int64)
                logits = o.decode_step(tok, t, self_kv, ckv).numpy()
                step(processed(logits, st, cfg, None if masks is None else masks[c]), st, cfg, max_len, sp.eos_id)
                idx = torch.tensor(st.parents, dtype=torch.int64)
                self_kv = [(k.index_select(0, idx), v.index_select(0, idx)) for k, v in self_kv]
                t += 1
            states.append(st)
            steps.append(t)
    ids, lens, scores, logp = result_block(states, K, max_len, sp.pad_id)
    return ids, lens, scores, logp, {"min_gap": np.array([s.min_gap for s in states]), "steps": np.array(steps), "states": states}


def sequential_score(logp_row, length, length_penalty):
    """the identity of include/mocr.h: the fp32 sum of logp[1 .. len - 1] taken in order, / (len - 1) ^ length_penalty"""
    acc = np.float32(0.0)
    for v in np.asarray(logp_row, np.float32)[1:int(length)]:
        acc = np.float32(v + acc)
    return np.float32(acc / np.float32(np.float32(length - 1) ** np.float32(length_penalty)))
