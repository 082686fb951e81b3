"""Numpy reference helpers of the token-automaton tests (tests/test_automaton_cpu.py, tests/test_gpu_automaton.py).

The rule is include/mocr.h, "token automata": a row under an automaton is in a state; the step's effective set is the
automaton's set of that state (its edge tokens, plus EOS iff it accepts) AND the row's token set, minus the n-gram bans, and
{EOS} if that is empty; every stored non-EOS token walks the state.  Written here the way a reader would write it - an
automaton is a dictionary of dictionaries, state -> token -> next state, and a set of accepting states - and not with the CSR
arithmetic of the kernel."""
import numpy as np

import constraint_util as cu
import ngram_util as nu

V, EOS = cu.V, cu.EOS
NONE, DEAD = -1, -2            # MOCR_STATE_NONE, MOCR_STATE_DEAD


class Automaton:
    """transitions: {state: {token: next state}} (a state without edges may be left out), accepting: the accepting states;
    state 0 is the start"""

    def __init__(self, transitions, accepting, n_states=None):
        self.trans = {int(s): {int(t): int(n) for t, n in e.items()} for s, e in transitions.items()}
        self.accepting = {int(s) for s in accepting}
        seen = set(self.trans) | self.accepting | {n for e in self.trans.values() for n in e.values()} | {0}
        self.n_states = int(n_states) if n_states is not None else max(seen) + 1

    def next(self, state: int, tok: int) -> int:
        if state < 0:
            return DEAD
        return self.trans.get(state, {}).get(int(tok), DEAD)

    def allowed(self, state: int) -> np.ndarray:
        """A(state) as bool [V]: the edge tokens, plus EOS iff the state accepts; A(DEAD) is empty"""
        m = np.zeros(V, bool)
        if state >= 0:
            m[list(self.trans.get(state, {}))] = True
            m[EOS] = state in self.accepting
        return m

    def walk(self, tokens, state: int = 0) -> int:
        """the state after these tokens (EOS moves nothing)"""
        for t in tokens:
            if int(t) != EOS:
                state = self.next(state, int(t))
        return state


def step_mask(aut, state, row, n: int, base) -> np.ndarray:
    """the effective set of the step that follows `row` (the tokens the row holds) in `state`: the automaton's set AND the
    base set, minus the n-gram bans, {EOS} if nothing is left.  aut None: ngram_util.step_mask"""
    if aut is None:
        return nu.step_mask(row, n, base)
    m = aut.allowed(state) & np.asarray(base, bool)
    ban = nu.banned_tokens(row, n)
    if ban:
        m[np.asarray(ban, np.int64)] = False
    if not m.any():
        m[EOS] = True
    return m


def trie(words):
    """words: sequences of token ids -> (Automaton whose accepted sequences are exactly the words, {accepting state: index
    of its word}); a word given twice keeps its first index"""
    trans, entry, n = {0: {}}, {}, 1
    for k, w in enumerate(words):
        s = 0
        for t in w:
            t = int(t)
            if t not in trans.setdefault(s, {}):
                trans[s][t] = n
                n += 1
            s = trans[s][t]
        entry.setdefault(s, k)
    return Automaton(trans, entry.keys(), n), entry


def loop(tokens, at_least: int = 2):
    """`at_least` or more tokens of the set: states 0 .. at_least, the last one accepting with a self-loop"""
    trans = {s: {int(t): min(s + 1, at_least) for t in tokens} for s in range(at_least + 1)}
    return Automaton(trans, [at_least], at_least + 1)


def universal():
    """one accepting state with a self-loop on every token except EOS"""
    return Automaton({0: {t: 0 for t in range(V) if t != EOS}}, [0], 1)


def pack(aut):
    """-> (edge_begin int32 [n_states + 1], edge_token, edge_next int32 [edges], accepting uint8 [n_states]): the CSR form of
    mocr_automaton_desc, every state's edges sorted by token"""
    begin, tok, nxt = [0], [], []
    for s in range(aut.n_states):
        for t, n in sorted(aut.trans.get(s, {}).items()):
            tok.append(t); nxt.append(n)
        begin.append(len(tok))
    acc = np.array([s in aut.accepting for s in range(aut.n_states)], np.uint8)
    return np.array(begin, np.int32), np.array(tok, np.int32), np.array(nxt, np.int32), acc


def unpack(edge_begin, edge_token, edge_next, accepting):
    """the inverse of pack"""
    trans = {s: {int(edge_token[i]): int(edge_next[i]) for i in range(edge_begin[s], edge_begin[s + 1])} for s in range(len(accepting))}
    return Automaton({s: e for s, e in trans.items() if e}, np.nonzero(accepting)[0], len(accepting))


def pack_many(auts):
    """several automata behind each other over GLOBAL state numbers, as the engine's arena holds them -> (edge_begin,
    edge_token, edge_next, accepting, the first global state of every automaton)"""
    begin, tok, nxt, acc, first = [np.zeros(1, np.int32)], [], [], [], []
    s0 = e0 = 0
    for a in auts:
        b, t, n, c = pack(a)
        first.append(s0)
        begin.append(b[1:] + e0); tok.append(t); nxt.append(n + s0); acc.append(c)
        s0 += a.n_states; e0 += len(t)
    return (np.concatenate(begin).astype(np.int32), np.concatenate(tok).astype(np.int32), np.concatenate(nxt).astype(np.int32),
            np.concatenate(acc).astype(np.uint8), first)


def automaton_generate(o, enc, automata, base_masks, ngrams, max_len: int):
    """ngram_util.ngram_generate with every row's state walked and its mask recomputed at every step from the rule above:
    automata: one Automaton or None per row, base_masks bool [B, V], ngrams int [B].  -> (ids int64 [B, L], the fp32 logits of
    every step [B, L - 1, V] unmasked, the masks of every step bool [B, L - 1, V], the final states [B]: NONE without an
    automaton)"""
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
        logits_all, masks_all = [], []
        t = 0
        while True:
            logits = o.decode_step(ids[:, -1], t, self_kv, ckv)
            logits_all.append(logits)
            hist = ids.numpy()
            mk = np.stack([step_mask(automata[b], state[b], hist[b], int(ngrams[b]), base[b]) if int(unfinished[b]) else base[b]
                           for b in range(B)])
            masks_all.append(mk)
            nxt = torch.argmax(torch.where(torch.from_numpy(mk), logits, torch.full_like(logits, float("-inf"))), dim=-1)
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
    return ids.numpy(), torch.stack(logits_all, dim=1).numpy(), np.stack(masks_all, axis=1), np.array(state, np.int64)


def is_path(aut, row, length: int, base=None, eos_by_dead_end=False):
    """the exact, precision-free property of an emitted row (ids incl. the start token, `length` tokens): its tokens are a
    path of the automaton, EOS appears only from an accepting state (or, eos_by_dead_end, from a state whose set AND base is
    empty) -> (ok, the walk's end state)"""
    state = 0
    for t in range(1, int(length)):
        tok = int(row[t])
        if tok == EOS:
            if t != length - 1:
                return False, state
            dead = state < 0 or not (aut.allowed(state) & (np.ones(V, bool) if base is None else np.asarray(base, bool))).any()
            return (state in aut.accepting) or (eos_by_dead_end and dead), state
        if aut.next(state, tok) == DEAD:
            return False, state
        state = aut.next(state, tok)
    return True, state
