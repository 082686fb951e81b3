"""Numpy reference helpers of the soft-automaton tests (tests/test_soft_automaton_cpu.py, tests/test_gpu_soft_automaton*.py).

The rule is include/mocr.h, "soft token automata", on top of tests/automaton_util.py's: an edge may carry a weight, which is
added in fp32 to its token's logit at the step taken in that state, and a state may be OPEN - it has a default edge, allows
every token but EOS (EOS iff it accepts) and sends a token without an edge along the default.  As there, an automaton is a
dictionary of dictionaries and not the CSR arithmetic of the kernels."""
import numpy as np

import automaton_util as au

V, EOS = au.V, au.EOS
NONE, DEAD = au.NONE, au.DEAD
FALLBACK = 1 << 30             # MOCR_DEFAULT_FALLBACK
SCORE_TOL = 3e-6               # transformers' fp32 token scores against the float64 reference (tests/golden/make_beam_automaton_goldens.py)


class SoftAutomaton(au.Automaton):
    """transitions / accepting as au.Automaton; weights: {state: {token: bias}} on existing edges; default: {state: next
    state} (a state without one is closed), or one int for every state; fallback: every default edge carries
    MOCR_DEFAULT_FALLBACK - a token without an edge is walked from the default state, to that state's edge's target if it has one"""

    def __init__(self, transitions, accepting, weights=None, default=None, n_states=None, fallback=False):
        super().__init__(transitions, accepting, n_states)
        self.fallback = bool(fallback)
        self.weights = {int(s): {int(t): float(w) for t, w in e.items()} for s, e in (weights or {}).items()}
        for s, e in self.weights.items():
            assert set(e) <= set(self.trans.get(s, {})), "a weight without an edge"
        if default is None:
            self.default = {}
        elif isinstance(default, dict):
            self.default = {int(s): int(d) for s, d in default.items() if int(d) >= 0}
        else:
            self.default = {s: int(default) for s in range(self.n_states)}
        self.n_states = max([self.n_states] + [d + 1 for d in self.default.values()] + [s + 1 for s in self.default])

    def is_open(self, state: int) -> bool:
        return state >= 0 and state in self.default

    def next(self, state: int, tok: int) -> int:
        if state < 0:
            return DEAD
        e = self.trans.get(state, {})
        if int(tok) in e:
            return e[int(tok)]
        d = self.default.get(state, DEAD)
        if d >= 0 and self.fallback:
            return self.trans.get(d, {}).get(int(tok), d)
        return d

    def allowed(self, state: int) -> np.ndarray:
        if not self.is_open(state):
            return super().allowed(state)
        m = np.ones(V, bool)
        m[EOS] = state in self.accepting
        return m

    def bias(self, state: int) -> np.ndarray:
        """float32 [V]: what the state's edges add to the logits (zeros for NONE / DEAD)"""
        b = np.zeros(V, np.float32)
        if state >= 0:
            for t, w in self.weights.get(state, {}).items():
                b[t] = np.float32(w)
        return b


def bias_of(aut, state: int) -> np.ndarray:
    return aut.bias(state) if isinstance(aut, SoftAutomaton) else np.zeros(V, np.float32)


def step_logits(aut, state: int, logits) -> np.ndarray:
    """the step's logits as the rule sees them: fp32 logit + fp32 weight where the state has an edge"""
    return (np.asarray(logits, np.float32) + bias_of(aut, state)).astype(np.float32)


def universal_open():
    """one accepting open state, default edge to itself, no edges: the soft twin of au.universal()"""
    return SoftAutomaton({}, [0], None, 0, 1)


def from_sequence_bias(sequence_bias, compact=False):
    """{tuple of ids: bias} -> the SoftAutomaton manga_ocr.text.bias_automaton compiles: every state open and accepting;
    compact: its compact form, walked with the fallback rule (what MangaOcr.sequence_bias creates)"""
    from manga_ocr.text import bias_automaton
    trans, weights = bias_automaton(sequence_bias, compact=compact)
    return SoftAutomaton(trans, set(trans), weights, 0, len(trans), fallback=compact)


def pack(aut):
    """au.pack plus (edge_weight float32 [edges], default_next int32 [n_states], -1: closed, | FALLBACK for a fallback automaton)"""
    eb, et, en, acc = au.pack(aut)
    w = np.zeros(len(et), np.float32)
    d = np.full(aut.n_states, -1, np.int32)
    if isinstance(aut, SoftAutomaton):
        for s in range(aut.n_states):
            for i in range(eb[s], eb[s + 1]):
                w[i] = np.float32(aut.weights.get(s, {}).get(int(et[i]), 0.0))
            d[s] = aut.default.get(s, -1)
            if d[s] >= 0 and aut.fallback:
                d[s] |= FALLBACK
    return eb, et, en, acc, w, d


def pack_many(auts):
    """au.pack_many plus the two soft arrays over GLOBAL state numbers, as the engine's arena holds them"""
    eb, et, en, acc, first = au.pack_many(auts)
    ws, ds = [], []
    for a, s0 in zip(auts, first):
        _, _, _, _, w, d = pack(a)
        ws.append(w)
        ds.append(np.where(d >= 0, ((d & (FALLBACK - 1)) + s0) | (d & FALLBACK), -1).astype(np.int32))
    return eb, et, en, acc, np.concatenate(ws).astype(np.float32), np.concatenate(ds).astype(np.int32), first


def hf_bias_vector(sequence_bias, history, vocab: int = V) -> np.ndarray:
    """transformers' SequenceBiasLogitsProcessor applied to zero scores after `history` (token ids, without a start token):
    the float32 bias vector of the next step.  transformers refuses an empty history row, so a start token that occurs in no
    sequence is put in front."""
    import torch
    from transformers import SequenceBiasLogitsProcessor
    proc = SequenceBiasLogitsProcessor(sequence_bias={tuple(int(t) for t in k): float(b) for k, b in sequence_bias.items()})
    ids = torch.tensor([[vocab - 1] + [int(t) for t in history]], dtype=torch.long)
    return proc(ids, torch.zeros(1, vocab, dtype=torch.float32))[0].numpy()


def soft_generate(o, enc, automata, base_masks, ngrams, max_len: int, prefixes=None):
    """au.automaton_generate with the edge weights added to the step's logits before everything else.  automata: one
    (Soft)Automaton or None per row; prefixes: None or one list of forced tokens per row.
    -> (ids int64 [B, L], the fp32 logits of every step [B, L - 1, V] WITH the weights added, unmasked, the same without them,
    the masks bool [B, L - 1, V], the final states [B], the states every step was taken in [B, L - 1])"""
    import torch
    sp = o.spec
    B = enc.shape[0]
    base = np.asarray(base_masks, bool)
    state = [NONE if a is None else 0 for a in automata]
    with torch.no_grad():
        ckv = o.cross_kv(enc)
        self_kv = [None] * sp.dec_layers
        ids = torch.full((B, 1), sp.start_id, dtype=torch.int64)
        unfinished = torch.ones(B, dtype=torch.int64)
        weighted_all, plain_all, masks_all, states_all = [], [], [], []
        t = 0
        while True:
            logits = o.decode_step(ids[:, -1], t, self_kv, ckv)
            plain_all.append(logits)
            states_all.append(list(state))
            wl = torch.from_numpy(np.stack([step_logits(automata[b], state[b], logits[b].numpy()) for b in range(B)]))
            weighted_all.append(wl)
            hist = ids.numpy()
            mk = np.stack([au.step_mask(automata[b], state[b], hist[b], int(ngrams[b]), base[b]) if int(unfinished[b]) else base[b]
                           for b in range(B)])
            masks_all.append(mk)
            nxt = torch.argmax(torch.where(torch.from_numpy(mk), wl, torch.full_like(wl, float("-inf"))), dim=-1)
            if prefixes is not None:
                for b in range(B):
                    if t < len(prefixes[b]):
                        nxt[b] = int(prefixes[b][t])
            nxt = nxt * unfinished + sp.pad_id * (1 - unfinished)
            for b in range(B):
                if int(unfinished[b]) and automata[b] is not None and int(nxt[b]) != sp.eos_id:
                    state[b] = automata[b].next(state[b], int(nxt[b]))
            ids = torch.cat((ids, nxt[:, None]), dim=1)
            done = (nxt == sp.eos_id) | (ids.shape[1] >= max_len)
            unfinished = unfinished & (~done).long()
            t += 1
            if int(unfinished.max()) == 0:
                break
    return (ids.numpy(), torch.stack(weighted_all, dim=1).numpy(), torch.stack(plain_all, dim=1).numpy(), np.stack(masks_all, axis=1),
            np.array(state, np.int64), np.array(states_all, np.int64).T)


def lengths(ids, eos: int = EOS) -> np.ndarray:
    """tokens of every row incl. the start token and EOS (the whole row when it never emits EOS)"""
    ids = np.asarray(ids)
    out = np.full(ids.shape[0], ids.shape[1], np.int64)
    for b in range(ids.shape[0]):
        hit = np.nonzero(ids[b, 1:] == eos)[0]
        if hit.size:
            out[b] = int(hit[0]) + 2
    return out
