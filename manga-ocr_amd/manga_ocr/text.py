"""Token ids -> the string the application consumes.

Host-side, pure Python (microseconds per crop).  Two steps of the reference's recogniser:

* ``tokenizer.decode(ids, skip_special_tokens=True)`` of the character-level BERT-Japanese
  tokenizer: id -> token through ``vocab.txt``, special tokens dropped,
  ``" ".join(tokens).replace(" ##", "")`` (TF/models/bert_japanese/tokenization_bert_japanese.py:250-262);
* ``post_process`` of the ``manga-ocr`` package [RECALL - the package is not available offline]:
  strip ALL whitespace; ``…`` -> ``...``; every run of two or more of ``・`` / ``.`` -> the same
  number of ``.``; then ``jaconv.h2z(text, ascii=True, digit=True)`` (half-width -> full-width for
  ASCII, digits and katakana).  ``jaconv`` is not installed here; ``h2z`` below restates its tables.
"""
from __future__ import annotations

import os
import re
from typing import Iterable, List, Optional, Sequence

SPECIAL_TOKENS = ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")

# jaconv's conv_table [RECALL, two independent recollections agree; the package is not installed here]: the
# full-width partners of " ' \ ` are the typographic ” ’ ￥ ‘, not the code-point-shifted ＂ ＇ ＼ ｀.
_HALF_ASCII = "abcdefghijklmnopqrstuvwxyz" + "ABCDEFGHIJKLMNOPQRSTUVWXYZ" + "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~ "
_FULL_ASCII = "ａｂｃｄｅｆｇｈｉｊｋｌｍｎｏｐｑｒｓｔｕｖｗｘｙｚ" + "ＡＢＣＤＥＦＧＨＩＪＫＬＭＮＯＰＱＲＳＴＵＶＷＸＹＺ" + \
              "！”＃＄％＆’（）＊＋，－．／：；＜＝＞？＠［￥］＾＿‘｛｜｝～　"
_HALF_DIGIT = "0123456789"
_FULL_DIGIT = "０１２３４５６７８９"
_HALF_KANA = "ｧｱｨｲｩｳｪｴｫｵｶｷｸｹｺｻｼｽｾｿﾀﾁｯﾂﾃﾄﾅﾆﾇﾈﾉﾊﾋﾌﾍﾎﾏﾐﾑﾒﾓｬﾔｭﾕｮﾖﾗﾘﾙﾚﾛﾜｦﾝｰ｡｢｣､･ﾞﾟ"
_FULL_KANA = "ァアィイゥウェエォオカキクケコサシスセソタチッツテトナニヌネノハヒフヘホマミムメモャヤュユョヨラリルレロワヲンー。「」、・゛゜"
_VOICED_HALF = "ｶｷｸｹｺｻｼｽｾｿﾀﾁﾂﾃﾄﾊﾋﾌﾍﾎｳ"
_VOICED_FULL = "ガギグゲゴザジズゼゾダヂヅデドバビブベボヴ"
_SEMI_HALF = "ﾊﾋﾌﾍﾎ"
_SEMI_FULL = "パピプペポ"

_H2Z_A = dict(zip(_HALF_ASCII, _FULL_ASCII))
_H2Z_D = dict(zip(_HALF_DIGIT, _FULL_DIGIT))
_H2Z_K = dict(zip(_HALF_KANA, _FULL_KANA))
_H2Z_V = {h + "ﾞ": f for h, f in zip(_VOICED_HALF, _VOICED_FULL)}
_H2Z_S = {h + "ﾟ": f for h, f in zip(_SEMI_HALF, _SEMI_FULL)}


_H2Z_TR = {(True, False, False): str.maketrans(_H2Z_K),
           (True, True, False): str.maketrans({**_H2Z_K, **_H2Z_A}),
           (True, False, True): str.maketrans({**_H2Z_K, **_H2Z_D}),
           (True, True, True): str.maketrans({**_H2Z_K, **_H2Z_A, **_H2Z_D}),
           (False, True, False): str.maketrans(_H2Z_A),
           (False, False, True): str.maketrans(_H2Z_D),
           (False, True, True): str.maketrans({**_H2Z_A, **_H2Z_D}),
           (False, False, False): {}}


def _h2z_tables(text: str, kana: bool = True, ascii: bool = False, digit: bool = False) -> str:
    """The restated tables: voiced / semi-voiced pairs first (longest match), then one character-wise translate."""
    if kana and ("ﾞ" in text or "ﾟ" in text):
        for pair, full in _H2Z_V.items():
            if pair in text:
                text = text.replace(pair, full)
        for pair, full in _H2Z_S.items():
            if pair in text:
                text = text.replace(pair, full)
    return text.translate(_H2Z_TR[(bool(kana), bool(ascii), bool(digit))])


try:        # the reference's recogniser calls jaconv itself: when the package is installed, so do we
    import jaconv as _jaconv
except ImportError:
    _jaconv = None


def h2z(text: str, kana: bool = True, ascii: bool = False, digit: bool = False) -> str:
    """Half-width -> full-width (jaconv.h2z semantics: voiced / semi-voiced marks combine with
    the preceding half-width katakana).  Uses ``jaconv`` when it is importable, else the restated tables."""
    if _jaconv is not None:
        return _jaconv.h2z(text, kana=kana, ascii=ascii, digit=digit)
    return _h2z_tables(text, kana=kana, ascii=ascii, digit=digit)


def post_process(text: str) -> str:
    text = "".join(text.split())
    text = text.replace("…", "...")
    text = re.sub("[・.]{2,}", lambda m: (m.end() - m.start()) * ".", text)
    return h2z(text, ascii=True, digit=True)


class Vocab:
    """id <-> token table of the decoder (one token per line of ``vocab.txt``)."""

    def __init__(self, tokens: Sequence[str]):
        self.tokens = list(tokens)
        self.special_ids = {i for i, t in enumerate(self.tokens) if t in SPECIAL_TOKENS}
        import numpy as np
        self._arr = np.array(self.tokens + ["[UNK]"], dtype=object)       # last slot: ids outside the table
        self._special = np.zeros(len(self.tokens) + 1, dtype=bool)
        self._special[list(self.special_ids)] = True
        # fast path of ids_to_text: post_process removes ALL whitespace, so the decode's `" ".join(...).replace(" ##", "")`
        # reduces to concatenating the tokens with the "##" of every non-first word piece dropped and the whitespace inside
        # tokens removed; both per-token forms are precomputed (checked against the plain composition in the CPU tests)
        nows = ["".join(t.split()) for t in self.tokens] + ["[UNK]"]
        self._first = np.array(nows, dtype=object)
        self._rest = np.array(["".join(t[2:].split()) if t.startswith("##") else n for t, n in zip(self.tokens + ["[UNK]"], nows)], dtype=object)
        self._plain = not any((" ##" in t) or (t != "##" and t.endswith(" ") ) for t in self.tokens)
        # ... and with post_process's character-wise steps applied per token where they commute with concatenation:
        # "…" -> "..." and the half -> full-width translation of everything except '.' and '･' (the dot-run rule must
        # still see the ASCII dot and must not see a '・' that comes from a half-width '･'); tokens with a (semi-)voiced
        # mark combine with their neighbour and send the row down the plain path
        def pre(t):
            t = t.replace("…", "...")
            return "".join(ch if ch in ".･" else _h2z_tables(ch, ascii=True, digit=True) for ch in t)
        self._first_pre = np.array([pre(t) for t in self._first.tolist()], dtype=object)
        self._rest_pre = np.array([pre(t) for t in self._rest.tolist()], dtype=object)
        self._mark = np.array([("ﾞ" in t) or ("ﾟ" in t) for t in self.tokens] + [False], dtype=bool)

    @classmethod
    def from_file(cls, path: str) -> "Vocab":
        with open(path, "r", encoding="utf-8") as f:
            return cls([line.rstrip("\n") for line in f])

    @classmethod
    def synthetic(cls, size: int = 6144) -> "Vocab":
        """Stand-in vocabulary for the synthetic-weight model: the five special tokens, then one
        CJK ideograph per id (so decoded strings are well-defined and whitespace-free)."""
        toks = list(SPECIAL_TOKENS) + [chr(0x4E00 + i) for i in range(size - len(SPECIAL_TOKENS))]
        return cls(toks)

    def __len__(self) -> int:
        return len(self.tokens)

    def ids_for_chars(self, chars: Iterable[str]) -> List[int]:
        """The ids of the tokens spelt with ``chars`` only - what a token set for "digits" or "kana" is built from
        (``MangaOcr.token_set``).  A token counts when its text, taken with a leading ``##`` and all whitespace stripped,
        is non-empty and every character of it is in ``chars``; special tokens never count.  The match is on the RAW token
        text of ``vocab.txt``, before ``post_process``: a set for full-width digits must name the half-width digits too if
        the vocabulary spells them so, because the half -> full-width step runs on the decoded string, after the decoder."""
        allowed = set("".join(chars))
        out = []
        for i, t in enumerate(self.tokens):
            if i in self.special_ids:
                continue
            body = "".join((t[2:] if t.startswith("##") else t).split())
            if body and all(ch in allowed for ch in body):
                out.append(i)
        return out

    def encode_chars(self, text: str) -> List[int]:
        """``text`` as one token per character - what a forced prefix (``MangaOcr.recognize(prefix=...)``, ``score_text``) is
        built from.  Matched on the RAW token text of ``vocab.txt`` as ``ids_for_chars`` does (a leading ``##`` and whitespace
        stripped, special tokens never count, the lowest id wins); whitespace in ``text`` is skipped.  A character without a
        single-token spelling raises ``ValueError`` naming it."""
        table = getattr(self, "_char_ids", None)
        if table is None:
            table = {}
            for i, t in enumerate(self.tokens):
                if i in self.special_ids:
                    continue
                body = "".join((t[2:] if t.startswith("##") else t).split())
                if len(body) == 1:
                    table.setdefault(body, i)
            self._char_ids = table
        out = []
        for ch in str(text):
            if ch.isspace():
                continue
            if ch not in table:
                raise ValueError(f"encode_chars: the vocabulary has no single token for the character {ch!r} (U+{ord(ch):04X})")
            out.append(table[ch])
        return out

    def decode(self, ids: Iterable[int], skip_special_tokens: bool = True) -> str:
        import numpy as np
        a = np.asarray(list(ids) if not hasattr(ids, "__len__") else ids, dtype=np.int64).ravel()
        a = np.where((a >= 0) & (a < len(self.tokens)), a, len(self.tokens))
        if skip_special_tokens:
            a = a[~self._special[a]]
        return " ".join(self._arr[a].tolist()).replace(" ##", "").strip()


def ids_to_text(vocab: Vocab, ids: Iterable[int]) -> str:
    """tokenizer.decode(ids, skip_special_tokens=True) followed by post_process."""
    if not vocab._plain:           # a vocabulary with whitespace-bearing tokens that could fake a " ##" seam: plain composition
        return post_process(vocab.decode(ids, skip_special_tokens=True))
    import numpy as np
    a = np.asarray(list(ids) if not hasattr(ids, "__len__") else ids, dtype=np.int64).ravel()
    a = np.where((a >= 0) & (a < len(vocab.tokens)), a, len(vocab.tokens))
    a = a[~vocab._special[a]]
    if a.size == 0:
        return ""
    if _jaconv is not None or vocab._mark[a].any():
        text = vocab._first[a[0]] + "".join(vocab._rest[a[1:]].tolist())
        text = text.replace("…", "...")
        if "・" in text or ".." in text:
            text = re.sub("[・.]{2,}", lambda m: (m.end() - m.start()) * ".", text)
        return h2z(text, ascii=True, digit=True)
    text = vocab._first_pre[a[0]] + "".join(vocab._rest_pre[a[1:]].tolist())
    if "・" in text or ".." in text:
        text = re.sub("[・.]{2,}", lambda m: (m.end() - m.start()) * ".", text)
    if "." in text:
        text = text.replace(".", _H2Z_A["."])
    if "･" in text:
        text = text.replace("･", _H2Z_K["･"])
    return text


DEFAULT_FALLBACK = 1 << 30      # MOCR_DEFAULT_FALLBACK (include/mocr.h): a bit of a default_next value


def pack_automaton(transitions, accepting, n_states: Optional[int] = None, weights=None, default=None, fallback: bool = False):
    """A token automaton ``{state: {token id: next state}}`` with its accepting states -> the CSR form the engine takes
    (include/mocr.h, "token automata"): (edge_begin [states + 1], edge_token, edge_next [edges], accepting [states]), every
    state's edges sorted by token.  State 0 is the start; states are 0 .. the largest one named (or ``n_states`` - 1).
    Soft automata: ``weights`` = ``{state: {token id: bias}}`` (an edge without one: 0; a weight without an edge: ValueError) and
    ``default`` = ``{state: next state}``, or one int for every state (a state without one: -1, closed); ``fallback`` = True
    marks every default edge with ``DEFAULT_FALLBACK``: a token without an edge is walked from the default state, to the target
    of that state's edge on it if it has one.  With either of ``weights`` / ``default`` given the result has two more elements,
    edge_weight [edges] and default_next [states]; with both None it is what it always was."""
    trans = {int(s): {int(t): int(n) for t, n in e.items()} for s, e in dict(transitions).items()}
    acc = {int(s) for s in accepting}
    named = set(trans) | acc | {n for e in trans.values() for n in e.values()} | {0}
    soft = weights is not None or default is not None
    dflt = {}
    if default is not None and not isinstance(default, dict):
        if isinstance(default, bool) or int(default) != default:
            raise ValueError("automaton: default is {state: next state} or one state number")
        named |= {int(default)}
    elif default is not None:
        dflt = {int(s): int(d) for s, d in default.items()}
        named |= set(dflt) | {d for d in dflt.values() if d >= 0}
    wts = {int(s): {int(t): float(w) for t, w in e.items()} for s, e in dict(weights or {}).items()}
    for s, e in wts.items():
        if set(e) - set(trans.get(s, {})):
            raise ValueError(f"automaton: state {s} has a weight on a token without an edge")
    if min(named) < 0:
        raise ValueError("automaton: states are numbered from 0")
    n = max(named) + 1 if n_states is None else int(n_states)
    if max(named) >= n:
        raise ValueError(f"automaton: a state beyond n_states ({n})")
    begin, tok, nxt = [0], [], []
    for s in range(n):
        for t, to in sorted(trans.get(s, {}).items()):
            tok.append(t)
            nxt.append(to)
        begin.append(len(tok))
    if soft:
        if any(d < -1 or d >= n for d in dflt.values()):
            raise ValueError(f"automaton: a default edge beyond n_states ({n})")
        wt = [wts.get(s, {}).get(t, 0.0) for s in range(n) for t in sorted(trans.get(s, {}))]
        dn = [int(default)] * n if default is not None and not isinstance(default, dict) else [dflt.get(s, -1) for s in range(n)]
        if fallback:
            dn = [d | DEFAULT_FALLBACK if d >= 0 else d for d in dn]
        return begin, tok, nxt, [1 if s in acc else 0 for s in range(n)], wt, dn
    return begin, tok, nxt, [1 if s in acc else 0 for s in range(n)]


def bias_automaton(sequence_bias, compact: bool = False):
    """transformers' ``generate(sequence_bias=...)`` (SequenceBiasLogitsProcessor) as a soft token automaton:
    ``{tuple of token ids: bias}`` -> (transitions, weights) for :func:`pack_automaton` with ``default=0`` and every state
    accepting.  The bias of a sequence goes to its last token when its earlier tokens are the row's most recent ones; a
    one-token sequence applies at every step; overlapping sequences add.
    The Aho-Corasick automaton of the sequences WITHOUT their last tokens: a state is the longest suffix of the history that
    is a proper prefix of a sequence; its edges are the union of the trie children along its fail chain (the child of the
    deepest node wins the target - that is the goto function), and an edge's weight is the sum, formed in float64 and rounded
    once by the engine, of the biases of every sequence that completes there - the ones ending at any node of the chain.  A
    token without an edge falls to the root.
    ``compact`` = True, for :func:`pack_automaton` with ``default=0, fallback=True``: a state other than the root leaves out
    every edge that weighs nothing and leads where the root's edge on that token leads (or to the root, where it has none) -
    the fallback walk finds those in the root.  The flat form repeats the root's edges in every state, states x first tokens
    edges in all; the compact one keeps a state's own children and completions, those of its fail chain below the root, and
    the root's weighted edges.  Both walk through the same states and weigh the same tokens."""
    seqs = {}
    for ids, b in dict(sequence_bias).items():
        ids = tuple(int(t) for t in ids)
        if not ids:
            raise ValueError("sequence_bias: an empty sequence")
        seqs[ids] = seqs.get(ids, 0.0) + float(b)
    # the trie over every proper prefix of a sequence (node 0: the empty history)
    child = [{}]
    ends = [{}]                                 # node -> {last token: summed bias of the sequences prefix(node) + token}
    for ids, b in sorted(seqs.items()):            # (sorted: the state numbers do not depend on the dict's order)
        s = 0
        for t in ids[:-1]:
            if t not in child[s]:
                child[s][t] = len(child)
                child.append({})
                ends.append({})
            s = child[s][t]
        ends[s][ids[-1]] = ends[s].get(ids[-1], 0.0) + b
    # breadth-first, so that a node's fail target (shallower) is done first: the full goto row and the weights of a node are
    # those of its fail target, overridden / increased by its own children and completions
    fail = [0] * len(child)
    trans, weights = {}, {}
    queue, at = [0], 0
    while at < len(queue):
        s = queue[at]
        at += 1
        if compact and s and not fail[s]:       # below the root: only what the fallback walk does not find there
            go = {t: trans[0][t] for t, w in weights[0].items() if w != 0.0}
            wt = {t: w for t, w in weights[0].items() if w != 0.0}
        else:
            go = dict(trans[fail[s]]) if s else {}
            wt = dict(weights[fail[s]]) if s else {}
        for t, c in child[s].items():
            # goto(fail[s], t), before this node's own child replaces it
            fail[c] = (go[t] if t in go else trans[0].get(t, 0) if compact else 0) if s else 0
            queue.append(c)
        for t, c in child[s].items():
            go[t] = c
        for t, b in ends[s].items():
            wt[t] = wt.get(t, 0.0) + b
            # a completing token that continues nothing: an edge for its weight, to where the token leads anyway
            go.setdefault(t, trans[0].get(t, 0) if compact and s else 0)
        trans[s], weights[s] = go, wt
    return trans, weights


def lexicon_trie(vocab: Vocab, texts: Sequence[str]):
    """The trie of ``texts`` over token ids, one token per character (``Vocab.encode_chars``): (transitions, {accepting state:
    index of its entry}) for :func:`pack_automaton` - a word's last node accepts, and an entry given twice keeps its first
    index.  An empty list, an entry without a character, or a character without a single-token spelling raises ``ValueError``."""
    texts = list(texts)
    if not texts:
        raise ValueError("lexicon: no entries")
    trans, entry, n = {0: {}}, {}, 1
    for k, text in enumerate(texts):
        ids = vocab.encode_chars(text)
        if not ids:
            raise ValueError(f"lexicon: entry {k} ({text!r}) has no characters")
        s = 0
        for t in ids:
            nxt = trans.setdefault(s, {})
            if t not in nxt:
                nxt[t] = n
                n += 1
            s = nxt[t]
        entry.setdefault(s, k)
    return trans, entry


def find_vocab(model_dir: Optional[str]) -> Optional[str]:
    if model_dir:
        p = os.path.join(model_dir, "vocab.txt")
        if os.path.exists(p):
            return p
    return None
