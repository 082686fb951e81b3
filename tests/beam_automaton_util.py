"""Float64 / numpy reference of beam search under token automata (tests/test_beam_automaton_cpu.py,
tests/test_gpu_beam_automaton*.py): tests/beam_token_util.py's step restated with the rule of include/mocr.h, "beam search
under a token automaton", on the automata of tests/automaton_util.py (dictionaries, not the kernel's CSR arithmetic).

  Every running beam k of a crop is in a state s_k of the crop's automaton (the start state at first).  log_softmax over the
  FULL row -> -inf for every token outside A(s_k) AND the crop's set (A(s): the edge tokens, plus EOS iff s accepts; A(DEAD) is
  empty) and for the beam's own n-gram bans -> + the beam's running score -> beam_token_util's selection, dead candidates
  included.  There is no dead-end rule: a beam with an empty effective set is a dead beam.
  A new running beam made from (parent p, token x) is in next(s_p, x), DEAD where s_p has no such edge (EOS is never an edge).
  A finished hypothesis keeps the state behind its last token other than EOS: s_p if it stopped on EOS, next(s_p, x) if it
  stopped by length - which is the walk of its tokens, EOS moving nothing.

THE -1e9 BEAMS.  Under a lexicon a beam has two or three finite candidates, so the 2 K winners regularly include children of
the padding beams that start at -1e9.  In fp32 - the engine's and transformers' arithmetic alike - such a score is -1e9 + lp
with |lp| far below the 64 that one ulp of 1e9 is: every one of them IS -1e9f, and they rank by the tie rule (the lower flat
index beam * V + token) and not by lp.  ``step`` therefore rounds the accumulated scores at or below -1e8 to float32 before
it ranks; float64 would order them by lp and follow other, equally meaningless paths.  Differences between such scores are no
decisions and do not enter ``min_gap``.  Hypotheses that descend from them score about -1e9: tests compare them with the
engine like everything else (the rounding makes them deterministic), and with transformers not at all (torch.topk promises no
order among equals)."""
import numpy as np

import automaton_util as au
import beam_token_util as btu
import beam_util as bu
import ngram_util as ngu

V, EOS, NEG = bu.V, bu.EOS, bu.NEG
NONE, DEAD = au.NONE, au.DEAD
JUNK = -1.0e8                   # scores at or below: descendants of the padding beams


class State(btu.State):
    """beam_token_util's state of one crop plus the automaton state of every running beam and of every finished hypothesis"""

    def __init__(self, K, start_id, aut=None):
        super().__init__(K, start_id)
        self.aut = aut
        self.ast = [NONE if aut is None else 0 for _ in range(K)]
        self.hyp_state = [NONE for _ in range(K)]


def beam_masks(st, cfg, base=None):
    """the effective set of every running beam, bool [K, V], before the n-gram bans: A(state) AND the crop's set; without an
    automaton the crop's set for every beam"""
    base = np.ones(V, bool) if base is None else np.asarray(base, bool)
    if st.aut is None:
        return np.repeat(base[None], cfg.K, 0)
    return np.stack([st.aut.allowed(s) & base for s in st.ast])


def processed(logits, st, cfg, base=None):
    """logits [K, V] of the running beams -> the processed log-probabilities [K, V] float64: log_softmax over the full row, then
    -inf outside each beam's own effective set and on each beam's own n-gram bans"""
    lp = bu.log_softmax64(logits)
    lp[~beam_masks(st, cfg, base)] = -np.inf
    for k in range(cfg.K):
        ban = ngu.banned_tokens(st.seqs[k], cfg.ngram)
        if ban:
            lp[k, np.asarray(ban, np.int64)] = -np.inf
            st.n_banned += len(ban)
    return lp


def _gap(sorted_desc):
    """beam_util._gap over the real scores only: the -1e9 ones are equal by construction"""
    v = np.asarray(sorted_desc, np.float64)
    return bu._gap(v[v > JUNK])


def step(lp, st, cfg, max_len, eos=EOS):
    """One selection on the processed log-probabilities [K, V] of a live crop: beam_token_util.step with the -1e9 scores in
    fp32 (above), and the states walked.  Returns (scores [2K], parents, tokens, stopped, lps [2K], next states [2K])."""
    K = cfg.K
    assert not st.done
    with np.errstate(invalid="ignore"):
        acc = np.asarray(lp, np.float64) + st.run[:, None]
    acc[np.isnan(acc)] = -np.inf
    low = acc <= JUNK
    acc[low] = acc[low].astype(np.float32).astype(np.float64)
    cur = len(st.seqs[0])
    flat = acc.reshape(-1)
    order = np.argsort(-flat, kind="stable")[:2 * K + 1]
    gap = _gap(flat[order])
    order = order[:2 * K]
    cv, cpar, ctok = flat[order], order // acc.shape[1], order % acc.shape[1]
    clp = np.asarray(lp, np.float64)[cpar, ctok]
    clp = np.where(np.isfinite(cv), clp, -np.inf)
    cst = [NONE if st.aut is None else st.aut.next(st.ast[p], int(x)) for p, x in zip(cpar, ctok)]      # (EOS: no edge, DEAD)
    stop = (ctok == eos) | (cur + 1 >= max_len)
    adj = cv - NEG * stop
    adj[adj <= JUNK] = adj[adj <= JUNK].astype(np.float32).astype(np.float64)     # (a stopped candidate's score - 1e9 is -1e9f too)
    pick = np.argsort(-adj, kind="stable")[:K]
    new_seqs = [st.seqs[cpar[i]] + [int(ctok[i])] for i in pick]
    new_logp = [st.logp[cpar[i]] + [float(clp[i])] for i in pick]
    new_ast = [cst[i] for i in pick]
    new_run = adj[pick]
    parents = [int(cpar[i]) for i in pick]
    filled = [len(s) > 0 for s in st.hyp_seq]
    full_guard = all(filled) and cfg.es == 1
    entries = [(st.hyp_score[j], st.hyp_seq[j], st.hyp_logp[j], st.hyp_state[j]) for j in range(K)]
    for i in range(K):
        if stop[i]:
            s = cv[i] / (float(cur) ** cfg.lp)
            if full_guard or not st.open:
                s -= NEG
            kept = NONE if st.aut is None else (st.ast[cpar[i]] if ctok[i] == eos else cst[i])
            entries.append((s, st.seqs[cpar[i]] + [int(ctok[i])], st.logp[cpar[i]] + [float(clp[i])], kept))
    keep = np.argsort(-np.array([e[0] for e in entries]), kind="stable")[:K]
    merged_real = sorted([e[0] for e in entries if len(e[1]) > 0 and np.isfinite(e[0])], reverse=True)
    gap = min(gap, _gap(merged_real))
    st.hyp_score = np.array([entries[j][0] for j in keep], np.float64)
    st.hyp_seq = [entries[j][1] for j in keep]
    st.hyp_logp = [entries[j][2] for j in keep]
    st.hyp_state = [entries[j][3] for j in keep]
    assert all(np.isfinite(s) for s in st.hyp_score), "a dead candidate never enters the finished set"
    st.seqs, st.logp, st.run, st.parents, st.ast = new_seqs, new_logp, new_run, parents, new_ast
    st.min_gap = min(st.min_gap, gap)
    cur2 = cur + 1
    hyp_len = (max_len - 1) if (cfg.es == 2 and cfg.lp > 0.0) else (cur2 - 1)
    best_possible = st.run[0] / (float(hyp_len) ** cfg.lp)
    filled = [len(s) > 0 for s in st.hyp_seq]
    worst = [st.hyp_score.min() if f else -NEG for f in filled]
    st.open = st.open and any(best_possible > w for w in worst)
    st.done = (not st.open) or (all(filled) and cfg.es == 1) or bool(np.all(stop))
    return cv, cpar, ctok, stop, clp, cst


def result_block(states, K, ld, pad_id=0):
    """the engine's output layout: beam_token_util.result_block plus state int32 [n, K], NONE for a crop without an automaton
    and for an empty slot"""
    ids, lens, scores, logp = btu.result_block(states, K, ld, pad_id)
    state = np.full((len(states), K), NONE, np.int32)
    for c, st in enumerate(states):
        for j in range(K):
            if st.hyp_seq[j]:
                state[c, j] = st.hyp_state[j]
    return ids, lens, scores, logp, state


def search(step_logits, K, cfg, max_len, aut=None, base=None, start_id=2, eos=EOS):
    """one crop's search on a callable ``step_logits(seqs, parents, t) -> logits [K, V]`` -> its final State"""
    st = State(K, start_id, aut)
    t = 0
    while not st.done:
        step(processed(step_logits(st.seqs, st.parents, t), st, cfg, base), st, cfg, max_len, eos)
        t += 1
        if aut is not None:     # the moved state IS the walk of the hypothesis' tokens, and a finished hypothesis is never DEAD
            for seq, s in zip(st.hyp_seq, st.hyp_state):
                assert (s == NONE) if not seq else (s == aut.walk(seq[1:]) and s >= 0), (seq, s)
    st.steps = t
    return st


def beam_generate(o, enc, cfg, max_len, automata=None, masks=None):
    """beam_token_util.beam_generate with one Automaton or None per crop (``automata``) and per-crop token sets ``masks`` (bool
    [n, V], EOS a member of every row; None: no sets) -> (ids, lens, scores, logp float64 [n, K, max_len], state int32 [n, K],
    info)"""
    import torch
    sp = o.spec
    K = cfg.K
    states, steps = [], []
    with torch.no_grad():
        for c in range(enc.shape[0]):
            ckv = o.cross_kv(enc[c:c + 1].repeat(K, 1, 1))
            kv = [[None] * sp.dec_layers]

            def logits_of(seqs, parents, t):
                if t > 0:
                    idx = torch.tensor(parents, dtype=torch.int64)
                    kv[0] = [(k.index_select(0, idx), v.index_select(0, idx)) for k, v in kv[0]]
                tok = torch.tensor([s[-1] for s in seqs], dtype=torch.int64)
                return o.decode_step(tok, t, kv[0], ckv).numpy()
            st = search(logits_of, K, cfg, max_len, None if automata is None else automata[c], None if masks is None else masks[c],
                        sp.start_id, sp.eos_id)
            states.append(st)
            steps.append(st.steps)
    ids, lens, scores, logp, state = result_block(states, K, max_len, sp.pad_id)
    return ids, lens, scores, logp, state, {"min_gap": np.array([s.min_gap for s in states]), "steps": np.array(steps), "states": states}


def junk_below(length_penalty, max_len):
    """the score at or below which a hypothesis descends from a padding beam: -1e9f / len ^ length_penalty with len <= max_len
    (real scores are sums of a few dozen log-probabilities above -20)"""
    return -NEG / float(max_len) ** max(float(length_penalty), 0.0)


def score_tol(want, tol):
    """the bound on a sequence score that is compared with an fp32 number: ``tol``, or two fp32 steps at the score's magnitude
    where that is more (under length_penalty 0 a score is a sum near -100, where fp32 numbers lie 7.6e-6 apart)"""
    w = np.abs(np.asarray(want, np.float64))
    return np.maximum(tol, 2.0 * np.spacing(w.astype(np.float32)).astype(np.float64))


def real_only(ids, lens, scores, logp, state, length_penalty, max_len, pad_id=0):
    """one crop's [K, ...] blocks with the -1e9 hypotheses as empty slots and the real ones moved up: what tests compare with
    transformers, whose order among equal scores is torch.topk's business"""
    K = lens.shape[0]
    out = (np.full_like(ids, pad_id), np.zeros_like(lens), np.full(K, -NEG, np.asarray(scores).dtype), np.zeros_like(logp),
           np.full_like(state, NONE))
    j2 = 0
    for j in range(K):
        if lens[j] > 0 and scores[j] > junk_below(length_penalty, max_len):
            for o, v in zip(out, (ids, lens, scores, logp, state)):
                o[j2] = v[j]
            j2 += 1
    return out


def set_automaton(mask):
    """one accepting state whose self-loops are the members of a token set (EOS is never an edge): the set as an automaton"""
    return au.Automaton({0: {int(t): 0 for t in np.nonzero(np.asarray(mask, bool))[0] if int(t) != EOS}}, [0], 1)
