"""Float64 / numpy reference of beam search under SOFT token automata (tests/test_beam_soft_cpu.py,
tests/test_gpu_beam_soft*.py): tests/beam_automaton_util.py's search with the rule of include/mocr.h, "beam search under soft
token automata", on the automata of tests/bias_util.py.  It is transformers' generate(num_beams=K, sequence_bias=...).

  At the step that chooses token L of beam k, in state s_k: lp = log_softmax over the FULL row of the raw logits; s = lp +
  edge_weight(s_k, t) where s_k has an edge on t (``bias_util.bias_of``); -inf outside A(s_k) AND the crop's set and on the
  beam's n-gram bans; acc = s + running.  Nothing renormalises - NOT the greedy soft rule, which adds the weight before its
  softmax - and a weight never revives a masked token.  A(s) of an open state is every non-EOS token plus EOS iff s accepts
  (``SoftAutomaton.allowed``).
  The states walk with ``SoftAutomaton.next``: the edge, else the default edge (with the fallback form, the default state's
  edge on the token), else DEAD.  EOS is never an edge, so a candidate that stopped on EOS and is carried on at score - 1e9
  follows the default edge of an open state and is DEAD in a closed one.
  The token scores are s = lp + w, the value that was ranked.

Everything else - the selection, the -1e9 beams in fp32, the finished set, the hypotheses' states - is
``beam_automaton_util.step`` itself, which reads the processed values and calls the automaton's ``next``."""
import numpy as np

import beam_automaton_util as bau
import beam_util as bu
import bias_util
import ngram_util as ngu

V, EOS, NEG = bau.V, bau.EOS, bau.NEG
NONE, DEAD = bau.NONE, bau.DEAD
State = bau.State
step = bau.step
result_block = bau.result_block
score_tol = bau.score_tol
real_only = bau.real_only
junk_below = bau.junk_below


def processed(logits, st, cfg, base=None):
    """beam_automaton_util.processed with the state's edge weights added behind the log_softmax and before the masks:
    logits [K, V] -> the processed scores [K, V] float64"""
    lp = bu.log_softmax64(logits)
    if st.aut is not None:
        for k in range(cfg.K):
            lp[k] += bias_util.bias_of(st.aut, st.ast[k]).astype(np.float64)
    lp[~bau.beam_masks(st, cfg, base)] = -np.inf
    for k in range(cfg.K):
        ban = ngu.banned_tokens(st.seqs[k], cfg.ngram)
        if ban:
            lp[k, np.asarray(ban, np.int64)] = -np.inf
            st.n_banned += len(ban)
    return lp


def search(step_logits, K, cfg, max_len, aut=None, base=None, start_id=2, eos=EOS):
    """one crop's search on a callable ``step_logits(seqs, parents, t) -> logits [K, V]`` -> its final State"""
    st = State(K, start_id, aut)
    t = 0
    while not st.done:
        step(processed(step_logits(st.seqs, st.parents, t), st, cfg, base), st, cfg, max_len, eos)
        t += 1
        if aut is not None:     # a real hypothesis holds one EOS at most, its last token: its state IS the walk of its tokens
            for seq, s, sc in zip(st.hyp_seq, st.hyp_state, st.hyp_score):
                if seq and sc > bau.JUNK and eos not in seq[1:-1]:
                    assert s == aut.walk(seq[1:]) and s >= 0, (seq, s)
    st.steps = t
    return st


def beam_generate(o, enc, cfg, max_len, automata=None, masks=None):
    """beam_automaton_util.beam_generate under the soft rule: one (Soft)Automaton or None per crop, per-crop token sets ``masks``
    -> (ids, lens, scores, logp float64 [n, K, max_len], state int32 [n, K], info)"""
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


def forced_score(o, enc_row, ids, length, aut, length_penalty):
    """The float64 score of ONE hypothesis under the rule, teacher-forced on its ids (``enc_row`` [1, S, D], ``ids`` with the
    start token, ``length`` tokens): (sum over its tokens of log_softmax64(logits)[tok] + weight(state, tok)) /
    (length - 1) ** length_penalty, and the per-token terms float64 [length - 1]"""
    import torch
    sp = o.spec
    terms = []
    with torch.no_grad():
        ckv = o.cross_kv(enc_row)
        kv = [None] * sp.dec_layers
        s = NONE if aut is None else 0
        for t in range(int(length) - 1):
            logits = o.decode_step(torch.tensor([int(ids[t])], dtype=torch.int64), t, kv, ckv).numpy()
            lp = bu.log_softmax64(logits)[0]
            tok = int(ids[t + 1])
            w = float(bias_util.bias_of(aut, s)[tok]) if aut is not None else 0.0
            terms.append(float(lp[tok]) + w)
            if aut is not None:
                s = aut.next(s, tok)
    terms = np.asarray(terms, np.float64)
    return float(terms.sum() / float(int(length) - 1) ** float(length_penalty)), terms
