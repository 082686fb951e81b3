"""Float64 / numpy reference of beam search (tests/test_beam_cpu.py, tests/test_gpu_beam*.py).

A plain restatement of ``GenerationMixin._beam_search`` of transformers 5.x (do_sample = False, one EOS id, a prompt of one
token; include/mocr.h, "beam search") for ONE crop at a time, on top of the Oracle's step logits:

  log_softmax over the full row -> the beam's own n-gram bans as -inf (no renormalising) -> + the beam's running score ->
  the top 2 K of the K x V accumulated scores -> a candidate stops on EOS or when it completes max_len tokens -> the next
  running beams are the best K after -1e9 on the stopped ones -> the finished set (K entries, scores from -1e9) is merged
  with the stopped candidates among the first K, score / (tokens generated) ^ length_penalty, and keeps its best K -> the
  early-stop heuristic and the three-way end condition.

Equal scores go to the lower index (a stable sort), as the engine states for itself.  Every step also reports its gap: the
smallest difference between adjacent entries of the sorted top-(2 K + 1) accumulated scores and between adjacent REAL
entries of the merged finished set (the unfilled -1e9 slots are equal by construction and are not compared) - an engine
whose scores are closer to the reference's than half that gap makes the same choices."""
import numpy as np

import ngram_util as ngu

V, EOS = ngu.V, ngu.EOS
NEG = 1.0e9
EARLY = {False: 0, True: 1, "never": 2, 0: 0, 1: 1, 2: 2}


class Config:
    def __init__(self, K, length_penalty=1.0, early_stopping=False, ngram=0):
        self.K, self.lp, self.es, self.ngram = int(K), float(length_penalty), EARLY[early_stopping], int(ngram)


class State:
    """one crop: K running beams and the finished set"""

    def __init__(self, K, start_id):
        self.seqs = [[int(start_id)] for _ in range(K)]
        self.run = np.array([0.0] + [-NEG] * (K - 1), np.float64)
        self.hyp_seq = [[] for _ in range(K)]           # [] = the slot never received a finished sequence
        self.hyp_score = np.full(K, -NEG, np.float64)
        self.open = True                                # is_early_stop_heuristic_unsatisfied
        self.done = False
        self.parents = list(range(K))
        self.min_gap = np.inf
        self.n_banned = 0                               # tokens the n-gram rule has banned so far, over steps and beams

    def copy(self):
        import copy
        return copy.deepcopy(self)


def log_softmax64(logits):
    x = np.asarray(logits, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def accumulate(logits, st, cfg):
    """logits [K, V] of the running beams -> the accumulated scores [K, V] float64: log_softmax, bans, + running score"""
    acc = log_softmax64(logits)
    for k in range(cfg.K):
        ban = ngu.banned_tokens(st.seqs[k], cfg.ngram)
        if ban:
            acc[k, np.asarray(ban, np.int64)] = -np.inf
            st.n_banned += len(ban)
    return acc + st.run[:, None]


def _gap(sorted_desc):
    v = np.asarray(sorted_desc, np.float64)
    v = v[np.isfinite(v)]
    return float(np.min(v[:-1] - v[1:])) if v.size >= 2 else np.inf


def step(acc, st, cfg, max_len, eos=EOS):
    """One selection on the accumulated scores [K, V] (float64) of a live crop; updates `st` in place and returns the
    candidates it considered: (scores [2K], parents [2K], tokens [2K], stopped [2K])."""
    K = cfg.K
    assert not st.done
    cur = len(st.seqs[0])                               # cur_len: tokens every running beam holds
    flat = np.asarray(acc, np.float64).reshape(-1)
    order = np.argsort(-flat, kind="stable")[:2 * K + 1]
    gap = _gap(flat[order])
    order = order[:2 * K]
    cv, cpar, ctok = flat[order], order // acc.shape[1], order % acc.shape[1]
    stop = (ctok == eos) | (cur + 1 >= max_len)
    # the running beams of the next step
    pick = np.argsort(-(cv - NEG * stop), kind="stable")[:K]
    new_seqs = [st.seqs[cpar[i]] + [int(ctok[i])] for i in pick]
    new_run = (cv - NEG * stop)[pick]
    parents = [int(cpar[i]) for i in pick]
    # the finished set: only the stopped candidates among the first K may enter (the others carry -1e9 in the reference
    # and never displace anything real); the two -1e9 guards hold exactly when the crop has already ended
    filled = [len(s) > 0 for s in st.hyp_seq]
    full_guard = all(filled) and cfg.es == 1
    entries = [(st.hyp_score[j], st.hyp_seq[j]) for j in range(K)]
    for i in range(K):
        if stop[i]:
            s = cv[i] / (float(cur) ** cfg.lp)
            if full_guard or not st.open:
                s -= NEG
            entries.append((s, st.seqs[cpar[i]] + [int(ctok[i])]))
    keep = np.argsort(-np.array([e[0] for e in entries]), kind="stable")[:K]
    merged_real = sorted([e[0] for e in entries if len(e[1]) > 0], reverse=True)
    gap = min(gap, _gap(merged_real))
    st.hyp_score = np.array([entries[j][0] for j in keep], np.float64)
    st.hyp_seq = [entries[j][1] for j in keep]
    st.seqs, st.run, st.parents = new_seqs, new_run, parents
    st.min_gap = min(st.min_gap, gap)
    # the heuristic of the next iteration (cur_len + 1) and the end condition
    cur2 = cur + 1
    hyp_len = (max_len - 1) if (cfg.es == 2 and cfg.lp > 0.0) else (cur2 - 1)
    best_possible = st.run[0] / (float(hyp_len) ** cfg.lp)
    filled = [len(s) > 0 for s in st.hyp_seq]
    worst = [st.hyp_score.min() if f else -NEG for f in filled]
    st.open = st.open and any(best_possible > w for w in worst)
    st.done = (not st.open) or (all(filled) and cfg.es == 1) or bool(np.all(stop))
    return cv, cpar, ctok, stop


def result_block(states, K, max_len_ld, pad_id=0):
    """the engine's output layout: ids [n, K, ld] (pad behind a length), lens [n, K] (0: empty slot), scores [n, K]"""
    n = len(states)
    ids = np.full((n, K, max_len_ld), pad_id, np.int32)
    lens = np.zeros((n, K), np.int32)
    scores = np.full((n, K), -NEG, np.float64)
    for c, st in enumerate(states):
        for j in range(K):
            if st.hyp_seq[j]:
                lens[c, j] = len(st.hyp_seq[j])
                ids[c, j, :lens[c, j]] = st.hyp_seq[j]
                scores[c, j] = st.hyp_score[j]
    return ids, lens, scores


def beam_generate(o, enc, cfg, max_len):
    """Beam search of every crop of enc [n, S, D] (the Oracle's encodings) on the Oracle's KV-cached decoder.
    -> (ids int32 [n, K, max_len], lens [n, K], scores float64 [n, K], info) with info["min_gap"] [n], info["steps"] [n] (the
    steps each crop ran) and info["states"]."""
    import torch
    sp = o.spec
    K = cfg.K
    states = []
    steps = []
    with torch.no_grad():
        for c in range(enc.shape[0]):
            ckv = o.cross_kv(enc[c:c + 1].repeat(K, 1, 1))
            self_kv = [None] * sp.dec_layers
            st = State(K, sp.start_id)
            t = 0
            while not st.done:
                tok = torch.tensor([s[-1] for s in st.seqs], dtype=torch.int64)
                logits = o.decode_step(tok, t, self_kv, ckv).numpy()
                step(accumulate(logits, st, cfg), st, cfg, max_len, sp.eos_id)
                idx = torch.tensor(st.parents, dtype=torch.int64)
                self_kv = [(k.index_select(0, idx), v.index_select(0, idx)) for k, v in self_kv]
                t += 1
            states.append(st)
            steps.append(t)
    ids, lens, scores = result_block(states, K, max_len, sp.pad_id)
    return ids, lens, scores, {"min_gap": np.array([s.min_gap for s in states]), "steps": np.array(steps), "states": states}


def has_repeat(row, n):
    return n > 0 and ngu.first_repeat(row, n) is not None
