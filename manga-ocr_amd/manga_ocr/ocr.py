"""``MangaOcr`` - the drop-in for the recogniser the reference application constructs once
(``src/ui/main_window.py:3394``: ``MangaOcr()``) and calls per crop from many threads
(``src/ui/main_window.py:9801``: ``self.manga_ocr_reader(pil_img) -> str``).

Same call surface as the ``manga-ocr`` package [RECALL]: ``MangaOcr(pretrained_model_name_or_path=
'kha-white/manga-ocr-base', force_cpu=False)``, ``__call__(PIL.Image | str | Path) -> str`` and
``ValueError`` for anything else.  Behind it: the HIP engine (libmocr_hip.so) on this
process's MI355X.  Concurrent callers (the reference runs up to 15 QueueProcessorWorker threads
on one shared instance, ``src/core/workers.py:209-247``) are coalesced into one batch per decode
instead of being serialised.  There is no CPU path: without the library or a GPU the constructor
raises, which the application already handles (``main_window.py:3396-3398``).
"""
from __future__ import annotations

import glob
import os
import threading
import time
from concurrent.futures import Future
from dataclasses import dataclass, field, replace
from pathlib import Path
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from ._capi import MAX_AUTOMATON_EDGES, MAX_AUTOMATON_STATES, MAX_BEAMS
from .engine import BeamConfig, Engine, result_layout
from .text import Vocab, find_vocab, ids_to_text
from .weights import DEFAULT_SPEC, load_checkpoint, synthetic_weights

DEFAULT_MODEL = "kha-white/manga-ocr-base"


def _resolve_model_dir(name_or_path: str) -> Optional[str]:
    """A local directory, $MANGA_OCR_MODEL_DIR, or an already-downloaded HF cache snapshot.
    Never touches the network."""
    cands = [name_or_path, os.environ.get("MANGA_OCR_MODEL_DIR", "")]
    hub = os.environ.get("HF_HOME", os.path.join(os.path.expanduser("~"), ".cache", "huggingface"))
    cands += sorted(glob.glob(os.path.join(hub, "hub", "models--" + name_or_path.replace("/", "--"), "snapshots", "*")))
    for c in cands:
        if c and os.path.isdir(c) and os.path.exists(os.path.join(c, "config.json")):
            return c
    return None


def to_gray224(img, size: int = 224) -> np.ndarray:
    """PIL image -> uint8 [224,224] ON THE HOST: ``convert('L')`` then the HF image processor's
    ``resize((224,224), BILINEAR)``.  Kept for callers that want the plane itself; the recogniser's own
    path (:func:`to_pixels`) leaves both steps to the device, which is bit-exact with this."""
    from PIL import Image
    g = img.convert("L")
    if g.size != (size, size):
        g = g.resize((size, size), Image.BILINEAR)
    return np.asarray(g, dtype=np.uint8)


def to_pixels(img) -> np.ndarray:
    """PIL image -> the uint8 array handed to the engine: [h,w,3] for RGB crops (what the reference builds at
    ``src/ui/main_window.py:9796-9800``), [h,w] for L; any other mode goes through Pillow's own convert('L')
    first (palettes, alpha, 16-bit ...: rare, and not worth restating).  ``convert('L')`` of RGB and the
    BILINEAR resize to 224x224 then run on the device (csrc/preprocess.h)."""
    if img.mode not in ("RGB", "L"):
        img = img.convert("L")
    return np.asarray(img, dtype=np.uint8)


_ALTERNATIVES = 4      # include/mocr.h MOCR_ALTERNATIVES
_POSITION_FIELDS = 5   # include/mocr.h MOCR_POSITION_FIELDS: cx, cy, sx, sy, mass


@dataclass(frozen=True)
class TokenSet:
    """What ``MangaOcr.token_set`` returns and ``allowed=`` takes: the engine's handle of an allowed-token set and the
    number of tokens in it as the caller named it (the engine adds EOS).  Handle 0 is the whole vocabulary."""
    handle: int
    size: int


def _set_handles(allowed, n: int) -> Optional[List[int]]:
    """``allowed=``: None, one set (TokenSet or engine handle) for all ``n`` crops, or one per crop -> None / n handles"""
    if allowed is None:
        return None
    one = lambda a: int(a.handle) if isinstance(a, TokenSet) else int(a)
    if isinstance(allowed, (TokenSet, int, np.integer)):
        return [one(allowed)] * n
    hs = [one(a) for a in allowed]
    if len(hs) != n:
        raise ValueError(f"allowed: {n} crops but {len(hs)} token sets")
    return hs


class Lexicon(NamedTuple):
    """A token automaton of a MangaOcr (:meth:`MangaOcr.lexicon`, :meth:`MangaOcr.automaton`) for ``lexicon=``: its engine
    handle, its accepting states, and for a lexicon the entry index of every accepting state and the entries themselves."""
    handle: int
    accepting: frozenset
    entries: dict
    texts: tuple
    # a soft automaton (:meth:`MangaOcr.sequence_bias`, :meth:`MangaOcr.glossary`, :meth:`MangaOcr.automaton` with weights or
    # default edges): it biases, it does not confine - ``accepted`` / ``entry`` stay None and ``match`` refuses it (``search``
    # takes it: beam search with the biases inside the hypotheses' scores)
    soft: bool = False
    spellings: tuple = ()       # glossary: the token ids of every entry, for :meth:`find`

    def find(self, ids) -> list:
        """Host code: (start position, entry index) of every glossary entry contained in the row ``ids`` (token ids, with or
        without the start token, EOS and padding), in order of position, then of entry."""
        row = [int(t) for t in ids]
        out = []
        for at in range(len(row)):
            for k, sp in enumerate(self.spellings):
                if sp and tuple(row[at:at + len(sp)]) == sp:
                    out.append((at, k))
        return out


def _lexicons(lexicon, n: int) -> Optional[List[Optional[Lexicon]]]:
    """``lexicon=`` (None: not used; one Lexicon for all crops; or one Lexicon / None per crop) -> a list of n, or None"""
    if lexicon is None:
        return None
    if isinstance(lexicon, Lexicon):
        return [lexicon] * n
    if isinstance(lexicon, (str, bytes, int, np.integer)):
        raise TypeError(f"lexicon: a Lexicon of MangaOcr.lexicon() / automaton() or a sequence of them, instead got {lexicon!r}")
    ls = list(lexicon)
    if len(ls) != n:
        raise ValueError(f"lexicon: {n} crops but {len(ls)} lexicons")
    if any(x is not None and not isinstance(x, Lexicon) for x in ls):
        raise TypeError("lexicon: every entry is a Lexicon of MangaOcr.lexicon() / automaton(), or None")
    return ls if any(x is not None for x in ls) else None


def resolve_no_repeat_ngram(value, ignored: dict, max_len: int):
    """``MangaOcr(no_repeat_ngram_size=...)`` -> (the size every call uses by default, or None for today's behaviour; what is
    left of the checkpoint's ignored generation settings).  ``None``: nothing changes.  An int in 0 .. max_len: that size (0 =
    off), whatever the checkpoint says - the checkpoint's own value then stays listed as ignored.  ``"checkpoint"``: the
    checkpoint's ``no_repeat_ngram_size`` (0 when its config has none), which is then honoured and leaves the ignored
    settings; the beam settings stay there."""
    ignored = dict(ignored)
    if value is None:
        return None, ignored
    if isinstance(value, str):
        if value != "checkpoint":
            raise ValueError(f"no_repeat_ngram_size: None, an int or 'checkpoint', instead got {value!r}")
        value = ignored.pop("no_repeat_ngram_size", 0)
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise TypeError(f"no_repeat_ngram_size: None, an int or 'checkpoint', instead got {value!r}")
    if not 0 <= int(value) <= max_len:
        raise ValueError(f"no_repeat_ngram_size must be in 0 .. max_len ({max_len}), 0 = off; got {value}")
    return int(value), ignored


def resolve_repetition_penalty(value, ignored: dict):
    """``MangaOcr(repetition_penalty=...)`` -> (the penalty every call uses by default; what is then still ignored of the
    checkpoint's generation config).  1.0 = off, as always; a float, finite and > 0; ``"checkpoint"`` = the checkpoint's
    ``repetition_penalty`` (1.0 when its config has none), which is then honoured and leaves the ignored settings."""
    ignored = dict(ignored)
    if isinstance(value, str):
        if value != "checkpoint":
            raise ValueError(f"repetition_penalty: a float or 'checkpoint', instead got {value!r}")
        value = ignored.pop("repetition_penalty", 1.0)
    return _penalty_value(value, "repetition_penalty"), ignored


def _penalty_value(value, name: str) -> float:
    """one repetition penalty: a real number, finite and > 0"""
    import math
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise TypeError(f"{name}: a float (finite, > 0; 1 = off), instead got {value!r}")
    if not math.isfinite(float(value)) or not float(value) > 0:
        raise ValueError(f"{name} must be finite and > 0 (1 = off; below 1 rewards repeats); got {value!r}")
    return float(value)


def _penalties(repetition_penalty, default: float, n: int) -> Optional[List[float]]:
    """``repetition_penalty=`` of a call (None: the constructor's ``default``), one float for all crops or one per crop ->
    one per crop, or None when every crop is at 1 (the call the method always made)"""
    if repetition_penalty is None:
        repetition_penalty = default
    if isinstance(repetition_penalty, (str, bytes)):
        raise TypeError(f"repetition_penalty: a float or a sequence of floats, instead got {repetition_penalty!r}")
    if isinstance(repetition_penalty, (bool, np.bool_, int, float, np.integer, np.floating)):
        ps = [_penalty_value(repetition_penalty, "repetition_penalty")] * n
    else:
        ps = [_penalty_value(p, "repetition_penalty") for p in repetition_penalty]
        if len(ps) != n:
            raise ValueError(f"repetition_penalty: {n} crops but {len(ps)} values")
    return ps if any(p != 1.0 for p in ps) else None


def resolve_num_beams(value, ignored: dict, ngram_default=None):
    """``MangaOcr(num_beams=...)`` -> (the :class:`BeamConfig` every plain call decodes with, or None for today's greedy
    behaviour; what is left of the checkpoint's ignored generation settings).  ``None``: nothing changes.  ``"checkpoint"``:
    ``num_beams``, ``length_penalty``, ``early_stopping`` and ``no_repeat_ngram_size`` of the checkpoint's config, which are
    then honoured and leave the ignored settings (a checkpoint that asks for no beams: None, nothing leaves).  An int in
    2 .. 4: the same with the caller's number of beams.  ``ngram_default``: the size ``no_repeat_ngram_size=`` already
    resolved to (it may have taken the checkpoint's value out of ``ignored`` before)."""
    ignored = dict(ignored)
    if value is None:
        return None, ignored
    if isinstance(value, str):
        if value != "checkpoint":
            raise ValueError(f"num_beams: None, an int or 'checkpoint', instead got {value!r}")
        if int(ignored.get("num_beams", 1)) < 2:
            return None, ignored
        value = int(ignored["num_beams"])
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise TypeError(f"num_beams: None, an int or 'checkpoint', instead got {value!r}")
    if not 2 <= int(value) <= MAX_BEAMS:
        raise ValueError(f"num_beams must be in 2 .. {MAX_BEAMS} (the engine's limit; None = greedy), instead got {value}")
    ignored.pop("num_beams", None)
    ngram = ignored.pop("no_repeat_ngram_size", ngram_default or 0)
    cfg = BeamConfig(int(value), float(ignored.pop("length_penalty", 1.0)), ignored.pop("early_stopping", False), int(ngram))
    return cfg, ignored


def _ngram_sizes(no_repeat_ngram, default, n: int) -> Optional[List[int]]:
    """``no_repeat_ngram=`` of a call (None: the constructor's ``default``, itself None for "not used"), one size for all
    ``n`` crops or one per crop -> None / n sizes"""
    if no_repeat_ngram is None:
        no_repeat_ngram = default
    if no_repeat_ngram is None:
        return None
    if isinstance(no_repeat_ngram, (bool, np.bool_, str)):
        raise TypeError(f"no_repeat_ngram: an int or a sequence of ints, instead got {no_repeat_ngram!r}")
    if isinstance(no_repeat_ngram, (int, np.integer)):
        gs = [int(no_repeat_ngram)] * n
    else:
        gs = [int(g) for g in no_repeat_ngram]
        if len(gs) != n:
            raise ValueError(f"no_repeat_ngram: {n} crops but {len(gs)} sizes")
    if any(g < 0 for g in gs):
        raise ValueError("no_repeat_ngram: sizes must be >= 0 (0 = off)")
    return gs


def _prefix_rows(prefix, n: int, vocab) -> Optional[List[Optional[List[int]]]]:
    """``prefix=`` of a call -> None (no crop has one) or, per crop, its token ids / None.  A ``str`` (encoded with
    ``Vocab.encode_chars``) or a flat int sequence applies to all ``n`` crops; a sequence of ``str``, int sequences or ``None``
    holds one entry per crop."""
    scalars = (bytes, bool, np.bool_, int, np.integer, float)

    def one(p):
        if p is None:
            return None
        if isinstance(p, str):
            return vocab.encode_chars(p) or None
        if isinstance(p, scalars) or not hasattr(p, "__iter__"):
            raise TypeError(f"prefix: a str, a sequence of token ids or None per crop, instead got {p!r}")
        ids = list(p)
        if any(isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)) for t in ids):
            raise TypeError(f"prefix: token ids must be ints, instead got {p!r}")
        return [int(t) for t in ids] or None

    if prefix is None:
        return None
    if isinstance(prefix, str):
        rows = [one(prefix)] * n
    elif isinstance(prefix, scalars) or not hasattr(prefix, "__iter__"):
        raise TypeError(f"prefix: a str, a sequence of token ids, or one of those (or None) per crop, instead got {prefix!r}")
    else:
        items = list(prefix)
        if not items:                       # an empty flat sequence: no prefix
            return None
        if all(isinstance(t, (int, np.integer)) and not isinstance(t, (bool, np.bool_)) for t in items):
            rows = [one(items)] * n         # a flat int sequence: every crop
        else:
            if len(items) != n:
                raise ValueError(f"prefix: {n} crops but {len(items)} prefixes")
            rows = [one(p) for p in items]
    return rows if any(r is not None for r in rows) else None


@dataclass(frozen=True)
class Recognition:
    """One recognised crop with the recogniser's own confidence (the ``*_scored`` methods of :class:`MangaOcr`).

    ``logprobs[k]`` is the natural-log probability the decoder gave ``ids[k + 1]`` - the generated tokens, EOS included;
    the start token is given, not predicted, and carries no score.  ``confidence`` is the geometric-mean token
    probability ``exp(mean(logprobs))``, ``min_prob`` the least certain token's ``exp(min(logprobs))``; both are 0.0 for a
    region that was never decoded (reduced to a sliver: ``text == ''``, no ids).

    The ``*_alternatives`` methods also fill ``alt_ids`` int32 ``[len - 1, 4]`` and ``alt_logprobs`` float32 ``[len - 1, 4]``
    (``None`` otherwise): row ``k`` belongs to ``ids[k + 1]`` like ``logprobs[k]`` and holds the four most probable tokens
    of that position, most probable first, so ``alt_ids[k, 0] == ids[k + 1]`` and ``alt_logprobs[k, 0] == logprobs[k]``
    (include/mocr.h, "token alternatives").  ``candidates(k)`` gives them as (token string, probability) pairs.

    The ``*_positions`` methods also fill ``positions`` float32 ``[len, 5]`` (``None`` otherwise): row ``t`` belongs to
    ``ids[t]`` and holds (cx, cy, sx, sy, mass) - centre, spread and patch mass of the last decoder layer's cross-attention
    when it emitted that token, in fractions of the 224 x 224 plane the encoder saw (include/mocr.h, "token positions"); row 0
    (the start token) is zeros.  ``boxes(width, height)`` turns them into pixel rectangles on the crop; for a region,
    ``rect`` is its padded, clipped rectangle on the page and ``page_boxes()`` gives page pixels."""
    text: str
    ids: np.ndarray
    logprobs: np.ndarray
    confidence: float
    min_prob: float
    alt_ids: Optional[np.ndarray] = None
    alt_logprobs: Optional[np.ndarray] = None
    positions: Optional[np.ndarray] = None
    rect: Optional[Tuple[int, int, int, int]] = None     # regions: (x, y, w, h) of the padded, clipped crop in page pixels
    n_forced: int = 0       # ``prefix=``: how many of ids[1:] the caller gave (their logprobs score the caller's tokens)
    # the ``*_beam`` methods: the hypothesis' beam-search score, sum of its token log-probabilities / (tokens generated) **
    # length_penalty (transformers' ``sequences_scores``); such a Recognition carries no per-token logprobs (confidence 0.0)
    # unless the call asked with ``token_scores=True``
    sequence_score: Optional[float] = None
    # ``lexicon=``: the automaton state the row ended in (-1: the crop had no lexicon, -2: it left its automaton), whether it
    # ended by EOS in an accepting state, and for a lexicon the index of the entry it read (None otherwise)
    state: Optional[int] = None
    accepted: bool = False
    entry: Optional[int] = None
    _vocab: object = field(default=None, repr=False, compare=False)      # what candidates() names the tokens with

    @classmethod
    def from_row(cls, vocab, ids_row: np.ndarray, logp_row: np.ndarray, length: int, alt_ids_row: Optional[np.ndarray] = None,
                 alt_logp_row: Optional[np.ndarray] = None, pos_row: Optional[np.ndarray] = None, rect=None) -> "Recognition":
        """A row of the engine's (ids, logp[, alt_ids, alt_logp]) blocks and its length (0: a sliver region) -> Recognition."""
        n = int(length)
        ids = np.array(ids_row[:n], dtype=np.int32)
        lp = np.array(logp_row[1:n], dtype=np.float32) if n > 1 else np.zeros(0, dtype=np.float32)
        alts = {}
        if alt_ids_row is not None:
            k = _ALTERNATIVES
            alts = dict(alt_ids=np.array(alt_ids_row[1:n], dtype=np.int32).reshape(-1, k) if n > 1 else np.zeros((0, k), np.int32),
                        alt_logprobs=np.array(alt_logp_row[1:n], dtype=np.float32).reshape(-1, k) if n > 1 else np.zeros((0, k), np.float32),
                        _vocab=vocab)
        if pos_row is not None:
            alts["positions"] = np.array(pos_row[:n], dtype=np.float32).reshape(-1, _POSITION_FIELDS)
            alts["rect"] = tuple(int(v) for v in rect) if rect is not None else None
        if lp.size == 0:
            return cls("" if n == 0 else ids_to_text(vocab, ids), ids, lp, 0.0, 0.0, **alts)
        lp64 = lp.astype(np.float64)
        return cls(ids_to_text(vocab, ids), ids, lp, float(np.exp(lp64.mean())), float(np.exp(lp64.min())), **alts)

    def boxes(self, width: float, height: float, rotate: int = 0, k: float = 2.0) -> np.ndarray:
        """Per token (x0, y0, x1, y1) in pixels of a ``width`` x ``height`` crop AS IT LAY IN MEMORY: centre -+ ``k`` spreads,
        clipped to the crop; float64 ``[len, 4]``, row 0 (the start token) and tokens without patch mass all 0.  ``rotate``: the
        crop's device rotation (0; 1 = 90 degrees clockwise; 2 = counter-clockwise) - the encoder saw the rotated crop, so the
        position is mapped back: clockwise x = cy', y = 1 - cx'; counter-clockwise x = 1 - cy', y = cx'; the spreads swap."""
        if self.positions is None:
            raise ValueError("this Recognition carries no positions: use MangaOcr.recognize_positions and friends")
        if rotate not in (0, 1, 2):
            raise ValueError(f"rotate must be 0, 1 or 2, instead got {rotate!r}")
        p = self.positions.astype(np.float64)
        cx, cy, sx, sy, mass = (p[:, i] for i in range(_POSITION_FIELDS))
        if rotate == 1:
            cx, cy, sx, sy = cy, 1.0 - cx, sy, sx
        elif rotate == 2:
            cx, cy, sx, sy = 1.0 - cy, cx, sy, sx
        W, H = float(width), float(height)
        out = np.stack([np.clip((cx - k * sx) * W, 0.0, W), np.clip((cy - k * sy) * H, 0.0, H),
                        np.clip((cx + k * sx) * W, 0.0, W), np.clip((cy + k * sy) * H, 0.0, H)], axis=1)
        out[mass <= 0.0] = 0.0
        return out

    def page_boxes(self, k: float = 2.0) -> np.ndarray:
        """``boxes`` of a region's Recognition in PAGE pixels, through ``rect`` (regions are never rotated)."""
        if self.rect is None:
            raise ValueError("this Recognition is not a region's (no rect): use boxes(width, height)")
        x, y, w, h = self.rect
        b = self.boxes(w, h, 0, k)
        live = (b != 0.0).any(axis=1)
        b[live] += np.array([x, y, x, y], dtype=np.float64)
        return b

    @property
    def token_logp(self) -> np.ndarray:
        """``logprobs`` in the engine's row form: float32 ``[len]``, one value per id, 0 for the start token."""
        return np.concatenate([np.zeros(min(1, len(self.ids)), dtype=np.float32), np.asarray(self.logprobs, dtype=np.float32)])

    @property
    def logprob(self) -> float:
        """The natural-log probability of the whole row, ``sum(logprobs)`` in float64: for a ``score_text`` result
        ``log p(text | crop)``."""
        return float(self.logprobs.astype(np.float64).sum())

    def branch(self, k: int, j: int) -> List[int]:
        """The prefix that acts on an alternative: the row as decoded up to generated position ``k``, then candidate ``j`` of
        that position - ``ids[1:k+1] + [alt_ids[k, j]]``, ready to pass as ``prefix=`` to decode the rest under the
        correction.  Needs a result of one of the ``*_alternatives`` methods."""
        if self.alt_ids is None:
            raise ValueError("this Recognition carries no alternatives: use MangaOcr.recognize_alternatives and friends")
        if not 0 <= k < len(self.alt_ids) or not 0 <= j < self.alt_ids.shape[1]:
            raise IndexError(f"branch: position {k} / candidate {j} outside the {len(self.alt_ids)} x {self.alt_ids.shape[1]} alternatives")
        tok = int(self.alt_ids[k, j])
        if tok < 0:
            raise ValueError(f"branch: position {k} has no candidate {j} (the crop's token set left fewer)")
        return [int(t) for t in self.ids[1:k + 1]] + [tok]

    def candidates(self, k: int) -> List[Tuple[str, float]]:
        """The four most probable tokens of generated position ``k`` (the one that emitted ``ids[k + 1]``), most probable
        first: (token as the vocabulary spells it, probability).  Entry 0 is the emitted token - except at a forced position (``k < n_forced``), where the entries
        are the step's own four best: entry 0 is what the model would have chosen, not necessarily the forced ``ids[k + 1]``.
        Fewer than four when the crop
        was decoded under a token set of fewer than four tokens (``allowed=``): the missing entries, id -1, are skipped.
        Needs a result of one of the ``*_alternatives`` methods."""
        if self.alt_ids is None or self.alt_logprobs is None:
            raise ValueError("this Recognition carries no alternatives: use MangaOcr.recognize_alternatives and friends")
        toks = self._vocab.tokens if self._vocab is not None else None
        out = []
        for i, lp in zip(self.alt_ids[k].tolist(), self.alt_logprobs[k].astype(np.float64).tolist()):
            if i < 0:
                continue
            name = toks[i] if toks is not None and 0 <= i < len(toks) else f"[{i}]"
            out.append((name, float(np.exp(lp))))
        return out


class _Request(NamedTuple):
    """one queued single-crop request of the batcher"""
    gray: np.ndarray
    future: Future
    scored: bool            # wants its logp (alternatives imply it)
    alternatives: bool
    positions: bool
    token_set: int          # 0: unconstrained
    ngram: int              # no-repeat n-gram size, 0: off
    prefix: Optional[tuple] = None      # forced prefix (token ids), None: none
    beam: Optional[BeamConfig] = None   # beam search with this configuration, None: greedy
    beam_scores: bool = False           # a beam request: wants its hypotheses' token log-probabilities
    beam_set: int = 0                   # a beam request: the token set its beams search under, 0: unconstrained
    beam_positions: bool = False        # a beam request: wants its hypotheses' token positions
    automaton: int = 0                  # token automaton handle (``lexicon=``), 0: none; such a caller gets its final state, last
    beam_automaton: int = 0             # a beam request (``match``): the automaton its beams walk, 0: none; such a caller gets its
                                        # hypotheses' states [K], last
    beam_soft: bool = False             # ... and that automaton may be soft (``search``): the batch makes the *_beam_soft call
    penalty: float = 1.0                # repetition penalty, 1: off


class _Batcher:
    """Coalesces concurrent single-crop requests into engine batches (FIFO, per-request error
    isolation like the reference's worker loop, ``src/core/workers.py:241-244``).  A request may ask for token scores;
    a batch with such a request makes the engine's scored call (the ids do not depend on it), and every caller gets
    what it asked for: ids, or (ids, logp).  The same one kind further for token alternatives: the batch makes the richest
    call any of its requests asked for, and such a caller gets (ids, logp, alt_ids, alt_logp).  A request may also carry a
    token set (``allowed=``); only a batch with such a request passes ``token_sets=`` - one handle per crop, 0 for the others -
    to the engine, so batches nobody constrains make exactly the calls they always made.  The same for a no-repeat n-gram size
    (``no_repeat_ngram=``): only a batch with a request of size > 0 passes ``no_repeat_ngram=``, one size per crop.  And for
    token positions (``positions=True``): only a batch with such a request passes ``positions=True``, and such a caller gets
    its positions as one more, last element of its result.  And for forced prefixes (``prefix=``): only a batch with such a
    request passes ``prefixes=``, one per crop, None for the others.  Beam search (``beam=``) is a call of its own: a batch
    is the run of queued requests that share the head's beam configuration (None for the greedy ones), so beam and greedy
    submissions are never merged, and a beam batch holds at most ``max_batch // num_beams`` crops; such a caller gets
    (ids [K, max_len], lengths [K], scores [K]).  A beam request may ask for its token scores (``beam_scores``) and carry a
    token set (``beam_set``): only a beam batch with such a request passes ``beam_scores=True`` / ``beam_sets=`` (one handle per
    crop, 0 for the others), and only a caller that asked gets logp [K, max_len] as a fourth element.  The same for the
    hypotheses' token positions (``beam_positions``): only a beam batch with such a request passes ``beam_positions=True``, and
    only a caller that asked gets pos [K, max_len, 5] as its last element.  And for a beam request's token automaton
    (``beam_automaton``, the ``match`` methods): only a beam batch with such a request passes ``beam_automata=`` (one handle per
    crop, 0 for the others) and ``beam_states=True``, and only such a caller gets state [K], behind everything else.  A
    ``search`` request marks its automaton ``beam_soft``: only a beam batch with such a request passes ``beam_soft=True``.  A
    greedy request may carry a repetition penalty (``repetition_penalty=``): only a batch with a request of p != 1 passes
    ``penalty=``, one value per crop, 1 for the others."""

    def __init__(self, engine: Engine, max_batch: int, timeout_ms: float):
        self.engine, self.max_batch, self.timeout = engine, max_batch, timeout_ms / 1000.0
        self._q: List = []
        self._cv = threading.Condition()
        self._stop = False
        self._thread = threading.Thread(target=self._run, name="mocr-batcher", daemon=True)
        self._thread.start()

    def submit(self, gray: np.ndarray, scored: bool = False, alternatives: bool = False, token_set: int = 0,
               no_repeat_ngram: int = 0, positions: bool = False, prefix=None, beam: Optional[BeamConfig] = None,
               beam_scores: bool = False, beam_set: int = 0, beam_positions: bool = False, automaton: int = 0,
               beam_automaton: int = 0, beam_soft: bool = False, penalty: float = 1.0) -> Future:
        f: Future = Future()
        with self._cv:
            if self._stop:
                raise RuntimeError("MangaOcr is closed")
            self._q.append(_Request(gray, f, bool(scored or alternatives), bool(alternatives), bool(positions), int(token_set), int(no_repeat_ngram),
                                    tuple(prefix) if prefix else None, beam, bool(beam_scores), int(beam_set), bool(beam_positions), int(automaton),
                                    int(beam_automaton), bool(beam_soft), float(penalty)))
            self._cv.notify()
        return f

    def _run(self):
        while True:
            with self._cv:
                while not self._q and not self._stop:
                    self._cv.wait()
                if self._stop and not self._q:
                    return
                deadline = time.monotonic() + self.timeout
                while len(self._q) < self.max_batch and not self._stop:
                    left = deadline - time.monotonic()
                    if left <= 0:
                        break
                    self._cv.wait(left)
                head = self._q[0].beam
                cap = self.max_batch if head is None else max(1, self.max_batch // head.num_beams)
                take = 1
                while take < min(cap, len(self._q)) and self._q[take].beam == head:
                    take += 1
                batch, self._q = self._q[:take], self._q[take:]
            try:
                if head is not None:
                    bkw = {}        # only what somebody asked for: a batch of plain beam requests makes the plain beam call
                    if any(r.beam_scores for r in batch):
                        bkw["beam_scores"] = True
                    if any(r.beam_set for r in batch):
                        bkw["beam_sets"] = [r.beam_set for r in batch]
                    if any(r.beam_positions for r in batch):
                        bkw["beam_positions"] = True
                    if any(r.beam_automaton for r in batch):
                        bkw["beam_automata"] = [r.beam_automaton for r in batch]
                        bkw["beam_states"] = True
                    if any(r.beam_soft for r in batch):
                        bkw["beam_soft"] = True
                    ids, lens, sc, *rest = self.engine.recognize_images([r.gray for r in batch], beam=head, **bkw)
                    logp = rest.pop(0) if bkw.get("beam_scores") else None
                    pos = rest.pop(0) if bkw.get("beam_positions") else None
                    state = rest.pop(0) if bkw.get("beam_states") else None
                    for i, r in enumerate(batch):
                        r.future.set_result((ids[i].copy(), lens[i].copy(), sc[i].copy()) + ((logp[i].copy(),) if r.beam_scores else ()) +
                                            ((pos[i].copy(),) if r.beam_positions else ()) + ((state[i].copy(),) if r.beam_automaton else ()))
                    continue
                kw = {}         # only what somebody asked for: a batch of plain requests makes the plain call
                if any(r.scored for r in batch):        # the richest call any request asked for
                    kw["alternatives" if any(r.alternatives for r in batch) else "scores"] = True
                if any(r.token_set for r in batch):
                    kw["token_sets"] = [r.token_set for r in batch]
                if any(r.ngram for r in batch):
                    kw["no_repeat_ngram"] = [r.ngram for r in batch]
                if any(r.positions for r in batch):
                    kw["positions"] = True
                if any(r.prefix for r in batch):
                    kw["prefixes"] = [list(r.prefix) if r.prefix else None for r in batch]
                if any(r.automaton for r in batch):         # (the same again for a token automaton, ``lexicon=``)
                    kw["automata"] = [r.automaton for r in batch]
                    kw["states"] = True
                if any(r.penalty != 1.0 for r in batch):    # (and for a repetition penalty)
                    kw["penalty"] = [r.penalty for r in batch]
                res = self.engine.recognize_images([r.gray for r in batch], **kw)
                state = res[-1] if kw.get("states") else None
                got = dict(zip(result_layout(kw.get("scores", False), kw.get("alternatives", False), kw.get("positions", False)), res))
                for i, r in enumerate(batch):
                    # what this caller asked for, cut to its length: bare ids, or a tuple with its logp / alternatives / positions
                    names = ["ids"] + ["logp"] * r.scored + ["alt_ids", "alt_logp"] * r.alternatives + ["pos"] * r.positions
                    out = tuple(got[name][i, :got["lens"][i]].copy() for name in names) + ((state[i:i + 1].copy(),) if r.automaton else ())
                    r.future.set_result(out if len(out) > 1 else out[0])
            except BaseException as exc:  # every waiting caller gets the error; the loop lives on
                for r in batch:
                    if not r.future.done():
                        r.future.set_exception(exc)

    def close(self):
        with self._cv:
            self._stop = True
            self._cv.notify_all()
        self._thread.join(timeout=5)


# HBM one row of a lane's workspace takes (bf16): 197 encoder rows x (fp32 residual + LN out + QKV + context + FFN
# intermediate + encoder output = 18,432 B) + latent key/value rows + input planes
_BYTES_PER_ROW_PER_LANE = 197 * 18432 + 2 * 300 * 768 * 2 + 4 * 224 * 224


def default_max_batch(device: int, lanes: int) -> int:
    """Rows per internal batch when the caller does not say: as fat as a fifth of the free HBM allows, capped at
    2048 (decode throughput is bought with fat batches - DESIGN.md §5 - and flattens beyond that), at least 64."""
    from .engine import device_memory
    free, _total = device_memory(device)
    rows = int(free * 0.2 / (max(1, lanes) * _BYTES_PER_ROW_PER_LANE))
    return max(64, min(2048, rows // 64 * 64))


class _Kind(NamedTuple):
    """A result kind of the recognise surface: the engine flags that ask for it, what :meth:`MangaOcr._require` refuses it by on
    several devices, and ``rows(ocr, source, *the engine's blocks)``: one result per row."""
    flags: dict
    refusal: Optional[str]
    rows: object


_TEXT = _Kind({}, None, lambda ocr, src, ids, lens: [ids[i, :lens[i]].copy() for i in range(len(lens))])      # token ids: the methods make the strings
_SCORED = _Kind(dict(scores=True), "SCORES", lambda ocr, src, *blocks: ocr._recognitions(*blocks))
_ALTS = _Kind(dict(alternatives=True), "ALTERNATIVES", lambda ocr, src, *blocks: ocr._recognitions_alt(*blocks))
_POS = _Kind(dict(scores=True, positions=True), "POSITIONS", lambda ocr, src, *blocks: ocr._recognitions_pos(*blocks, rects=src.rects))


class _Images(NamedTuple):
    """A source of the recognise surface: crops for ``recognize_images``, 3-channel ones in OpenCV order with ``bgr``, each
    with its rotation code in ``rotate``.  ``call(ocr, a, b, **kw)``: the engine call for crops a .. b (all of them by default)."""
    crops: list
    bgr: bool = False
    rotate: Optional[Sequence[int]] = None
    rects = None

    @property
    def n(self) -> int:
        return len(self.crops)

    def call(self, ocr, a: int = 0, b: Optional[int] = None, **kw):
        return ocr.engine.recognize_images(self.crops[a:b], self.bgr, None if self.rotate is None else list(self.rotate)[a:b], **kw)


class _Regions(NamedTuple):
    """A source: (page_index, x, y, w, h) regions on BGR pages for ``recognize_regions``; ``rects`` (the positions kind): every
    region's padded, clipped rectangle on its page."""
    pages: list
    regions: list
    rects: Optional[list] = None

    @property
    def n(self) -> int:
        return len(self.regions)

    def with_rects(self) -> "_Regions":
        from .regions import padded_rect
        return self._replace(rects=[padded_rect(r[1:5], self.pages[int(r[0])].shape[0], self.pages[int(r[0])].shape[1]) for r in self.regions])

    def call(self, ocr, a: int = 0, b: Optional[int] = None, **kw):
        return ocr.engine.recognize_regions(self.pages, self.regions[a:b], True, **kw)


class _Single(NamedTuple):
    """A source: one crop that goes through the batcher and comes back as the one-row blocks the engine would have returned."""
    pixels: np.ndarray
    n = 1
    rects = None

    @staticmethod
    def batcher_kw(kw: dict) -> dict:
        """one row's engine keywords (``MangaOcr._decode_kw``) as ``_Batcher.submit`` names them"""
        names = (("token_sets", "token_set"), ("no_repeat_ngram", "no_repeat_ngram"), ("prefixes", "prefix"), ("automata", "automaton"),
                 ("penalty", "penalty"))
        return {single: kw[many][0] for many, single in names if many in kw}

    def call(self, ocr, scores: bool = False, alternatives: bool = False, positions: bool = False, states: bool = False, **kw):
        out = ocr._batcher.submit(self.pixels, scored=scores, alternatives=alternatives, positions=positions, **self.batcher_kw(kw)).result()
        ids, *rest = out if isinstance(out, tuple) else (out,)
        state = (rest.pop(),) if states else ()           # (the row's final state comes as an array of one already)
        return (ids[None], np.array([len(ids)]), *(a[None] for a in rest), *state)


class MangaOcr:
    def __init__(self, pretrained_model_name_or_path: str = DEFAULT_MODEL, force_cpu: bool = False, *,
                 dtype: Optional[str] = None, device: Optional[int] = None, devices: Optional[Sequence[int]] = None,
                 max_batch: Optional[int] = None, lanes: Optional[int] = None, batch_timeout_ms: Optional[float] = None,
                 synthetic_seed: Optional[int] = None, no_repeat_ngram_size=None, num_beams=None, repetition_penalty=1.0):
        """``MangaOcr()`` as the application calls it (``src/ui/main_window.py:3394``) builds the engine on this
        process's GPU with two lanes and an internal batch sized from the free HBM.  ``devices=[0, 1, ...]`` (or
        ``MANGA_OCR_DEVICES=0,1,...``) instead starts one child process per GPU and shards every batch call over
        them (``manga_ocr/multi.py``); the parent then never touches a GPU.
        ``no_repeat_ngram_size``: transformers' setting of that name under this engine's greedy decoding (include/mocr.h,
        "no-repeat n-grams") for every call that does not say otherwise (``no_repeat_ngram=``): None = not used, as always; an
        int; or ``"checkpoint"`` = the value in the checkpoint's generation config, which then leaves
        ``ignored_generation_config`` (the beam settings stay ignored).
        ``num_beams``: beam search (include/mocr.h, "beam search") for ``__call__`` and every plain ``recognize*`` method,
        which then return the best hypothesis: None = greedy, as always; ``"checkpoint"`` = ``num_beams``,
        ``length_penalty``, ``early_stopping`` and ``no_repeat_ngram_size`` of the checkpoint's generation config, which then
        leave ``ignored_generation_config``; an int in 2 .. 4 = the same with that many beams.  The loader's warning about
        ignored generation settings is then given only for what is still ignored.  The ``*_positions`` methods
        (``recognize_positions`` and its batch, BGR and regions forms) then decode with the beams too: they return the best
        hypothesis - the text ``__call__`` returns - with its token scores, ``sequence_score`` and ``positions`` (include/mocr.h,
        "beam search with token positions"), so ``boxes`` / ``page_boxes`` belong to the text returned; like the plain methods
        they then refuse ``allowed=`` / ``no_repeat_ngram=`` / ``prefix=`` (the instance's ``beam_positions``, set here whenever
        ``beam`` is, says so).  The scored, alternatives and n-best methods
        (``recognize_scored``, ``recognize_alternatives``, ``recognize_nbest`` and their batch forms, ``score_text``) keep decoding
        greedily: they return one greedy row per crop, with its alternatives or prefix; use ``recognize_beam`` for all
        hypotheses with their sequence scores - and, with ``token_scores=True`` / ``allowed=`` / ``positions=True``, their token
        log-probabilities, a search under a token set and their token positions.
        ``repetition_penalty``: transformers' setting of that name under this engine's greedy decoding (include/mocr.h,
        "repetition penalty") for every greedy call that does not say otherwise (``repetition_penalty=``): 1.0 = off, as always;
        a float, finite and > 0 (below 1 rewards repeats); or ``"checkpoint"`` = the value in the checkpoint's generation
        config, which then leaves ``ignored_generation_config``.  It does not combine with ``num_beams`` (under beams
        transformers penalises log-probabilities, which this engine does not do yet): ``ValueError``."""
        if force_cpu:
            raise RuntimeError("this MangaOcr is the MI355X engine: there is no CPU path (force_cpu=True is not supported)")
        dtype = dtype or os.environ.get("MANGA_OCR_DTYPE", "bf16")
        if devices is None and os.environ.get("MANGA_OCR_DEVICES"):
            devices = [int(x) for x in os.environ["MANGA_OCR_DEVICES"].split(",") if x.strip() != ""]
        device = int(os.environ.get("LOCAL_RANK", "0")) if device is None else device
        lanes = int(lanes or os.environ.get("MANGA_OCR_LANES", "2"))
        if max_batch is None and os.environ.get("MANGA_OCR_MAX_BATCH"):
            max_batch = int(os.environ["MANGA_OCR_MAX_BATCH"])
        if synthetic_seed is None and os.environ.get("MANGA_OCR_SYNTHETIC"):
            synthetic_seed = int(os.environ["MANGA_OCR_SYNTHETIC"])
        model_dir = None
        if synthetic_seed is not None:
            spec, weights, vocab = DEFAULT_SPEC, None, Vocab.synthetic(DEFAULT_SPEC.vocab)
        else:
            model_dir = _resolve_model_dir(str(pretrained_model_name_or_path))
            if model_dir is None:
                raise FileNotFoundError(
                    f"no local copy of '{pretrained_model_name_or_path}' (looked at the path, $MANGA_OCR_MODEL_DIR and the "
                    "HF cache; this build never downloads). Set MANGA_OCR_SYNTHETIC=<seed> for synthetic weights.")
            import warnings
            with warnings.catch_warnings(record=num_beams is not None) as caught:
                # (with num_beams= the loader's "ignores it" may not be true: what is still ignored is said below)
                if num_beams is not None:
                    warnings.simplefilter("always")         # recorded whatever the caller's filters; the others are given again
                spec, weights = load_checkpoint(model_dir)
            for w_ in caught or ():
                if not (issubclass(w_.category, RuntimeWarning) and "non-greedy generation" in str(w_.message)):
                    warnings.warn_explicit(w_.message, w_.category, w_.filename, w_.lineno)
            vp = find_vocab(model_dir)
            if vp is None:
                raise FileNotFoundError(f"vocab.txt not found in {model_dir}")
            vocab = Vocab.from_file(vp)
            if len(vocab) != spec.vocab:
                raise ValueError(f"vocab.txt has {len(vocab)} entries, config says {spec.vocab}")
        self.spec, self.vocab = spec, vocab
        # what the checkpoint's config.json asked of generate() and this engine ignores (greedy decode only): the reference
        # application's recogniser would honour e.g. num_beams=4 / no_repeat_ngram_size=3, so on such a checkpoint the
        # strings can differ from the pip package's; {} when there is nothing to report
        self.no_repeat_ngram_size, self.ignored_generation_config = resolve_no_repeat_ngram(
            no_repeat_ngram_size, dict(getattr(spec, "ignored_generation", ())), spec.max_len)
        self.beam, self.ignored_generation_config = resolve_num_beams(num_beams, self.ignored_generation_config, self.no_repeat_ngram_size)
        # do the *_positions methods decode with those beams too (the best hypothesis with its positions)?  Every MangaOcr this
        # constructor builds with beams says yes; an instance that holds ``beam`` alone keeps the greedy positions rows it had
        self.beam_positions = self.beam is not None
        self.repetition_penalty, self.ignored_generation_config = resolve_repetition_penalty(repetition_penalty, self.ignored_generation_config)
        if self.beam is not None and self.repetition_penalty != 1.0:
            raise ValueError("repetition_penalty does not combine with num_beams: beam search takes no repetition penalty")
        if num_beams is not None and self.ignored_generation_config:
            import warnings
            warnings.warn("checkpoint config asks for generation settings this engine still ignores: " + repr(self.ignored_generation_config) +
                          (" (num_beams=: the checkpoint asks for no beams; greedy decode)" if self.beam is None else ""),
                          RuntimeWarning, stacklevel=2)
        if self.no_repeat_ngram_size and devices is not None and len(devices) > 1:
            from .multi import MultiGpuEngine
            raise NotImplementedError(MultiGpuEngine.NO_NGRAM)
        if self.beam is not None and devices is not None and len(devices) > 1:
            from .multi import MultiGpuEngine
            raise NotImplementedError(MultiGpuEngine.NO_BEAM)
        if self.repetition_penalty != 1.0 and devices is not None and len(devices) > 1:
            from .multi import MultiGpuEngine
            raise NotImplementedError(MultiGpuEngine.NO_PENALTY)
        if devices is not None and len(devices) > 1:
            from .multi import MultiGpuEngine
            max_batch = int(max_batch or 2048)
            self.engine = MultiGpuEngine(devices, factory_args=dict(synthetic_seed=synthetic_seed, model_dir=model_dir, dtype=dtype,
                                                                    max_batch=max_batch, lanes=lanes))
        else:
            if devices:
                device = int(devices[0])
            if weights is None:
                weights = synthetic_weights(synthetic_seed)
            max_batch = int(max_batch or default_max_batch(device, lanes))
            self.engine = Engine(weights, spec, dtype=dtype, device=device, max_batch=max_batch, lanes=lanes)
        self.max_batch = max_batch
        # How long the first single-crop caller waits for company before its batch is sent off.  Callers that arrive while a
        # batch is being decoded queue up behind it and form the next batch anyway, so the window only has to catch a burst
        # of workers that start together.  MI355X, 24-token texts (tools/call_latency.py): 2.0 / 0.3 / 0 ms -> one caller
        # 5.3 / 3.6 / 3.2 ms per call, 15 worker threads 2100 / 2350 / 1880 crops/s
        if batch_timeout_ms is None:
            batch_timeout_ms = float(os.environ.get("MANGA_OCR_BATCH_WINDOW_MS", "0.3"))
        self._batcher = _Batcher(self.engine, max_batch, batch_timeout_ms)
        self._token_sets = {}
        self._token_sets_lock = threading.Lock()
        # same warm-up the reference's recogniser does in its constructor (one inference)
        self.recognize_ids([np.zeros((spec.image_size, spec.image_size), dtype=np.uint8)])

    # ------------------------------------------------------------------ reference call surface
    def __call__(self, img_or_path) -> str:
        return self.recognize(img_or_path)

    def _require(self, what: str) -> None:
        """refuse ``what`` (SCORES, CONSTRAINTS, NGRAM, PREFIX, POSITIONS, ALTERNATIVES, BEAM, BEAM_POSITIONS, PENALTY) on an engine that says it cannot:
        MultiGpuEngine, whose workers make the plain greedy call and ship ids and lengths only, has a NO_* message for each"""
        no = getattr(self.engine, "NO_" + what, None)
        if no:
            raise NotImplementedError(no)

    # ------------------------------------------------------------------ token constraints
    def token_set(self, chars=None, ids=None, exclude_chars=None) -> TokenSet:
        """An allowed-token set for ``allowed=``: what the caller knows about a crop (a page-number box holds digits, a
        sound-effect bubble kana) or never wants to see.  ``chars``: the tokens spelt with these characters only
        (``Vocab.ids_for_chars``: matched on the raw token text of vocab.txt, before ``post_process`` - name half- and
        full-width forms as the vocabulary spells them); ``ids``: these token ids; both: their union; neither: the whole
        vocabulary.  ``exclude_chars`` then removes every token whose text contains one of these characters.  EOS is always
        a member (the engine adds it).  The same content gives the same handle; sets live as long as this MangaOcr, at most
        255 of them (include/mocr.h, "token constraints")."""
        self._require("CONSTRAINTS")
        if chars is None and ids is None:
            members = set(range(len(self.vocab)))
        else:
            members = set(self.vocab.ids_for_chars(chars)) if chars is not None else set()
            if ids is not None:
                members |= {int(i) for i in ids}
        if exclude_chars:
            banned = set("".join(exclude_chars))
            members = {i for i in members if not (0 <= i < len(self.vocab)) or not (banned & set(self.vocab.tokens[i]))}
        if not members:
            raise ValueError("token_set: no token of the vocabulary is left in the set")
        key = frozenset(members)
        with self._token_sets_lock:
            ts = self._token_sets.get(key)
            if ts is None:
                ts = self._token_sets[key] = TokenSet(self.engine.token_set(sorted(members)), len(members))
            return ts

    # ------------------------------------------------------------------ token automata
    def lexicon(self, texts) -> Lexicon:
        """A closed list of texts for ``lexicon=``: the crop is read as one of them (include/mocr.h, "token automata") at one
        decode row, whatever the size of the list.  The entries are spelt one token per character (``Vocab.encode_chars``, on
        the raw token text of vocab.txt); an empty list or a character without a single-token spelling raises ``ValueError``.
        ``Recognition.entry`` then indexes ``texts``.  Lexicons live as long as this MangaOcr, at most 256 of them."""
        from .text import lexicon_trie, pack_automaton
        self._require("LEXICON")
        texts = tuple(str(t) for t in texts)
        trans, entry = lexicon_trie(self.vocab, texts)
        return Lexicon(self.engine.automaton(*pack_automaton(trans, entry)), frozenset(entry), dict(entry), texts)

    def automaton(self, transitions, accepting, weights=None, default=None) -> Lexicon:
        """The raw form, for patterns such as "one or two digits": ``transitions`` = {state: {token id: next state}} with state 0
        the start, ``accepting`` = the states a row may end in.  For ``lexicon=``; ``Recognition.entry`` stays None.
        ``weights`` (the nesting of ``transitions``: {state: {token id: bias}}) and ``default`` ({state: next state}, or one int
        for every state) make it a soft automaton (include/mocr.h, "soft token automata"): an edge's bias is added to its
        token's logit, and a state with a default edge allows every token."""
        from .text import pack_automaton
        self._require("LEXICON")
        acc = frozenset(int(s) for s in accepting)
        if weights is None and default is None:
            return Lexicon(self.engine.automaton(*pack_automaton(transitions, acc)), acc, {}, ())
        return Lexicon(self.engine.automaton(*pack_automaton(transitions, acc, weights=weights, default=default)), acc, {}, (), True)

    def sequence_bias(self, sequence_bias) -> Lexicon:
        """transformers' ``generate(sequence_bias=...)`` for ``lexicon=``: ``{text or tuple of token ids: bias}``.  A text is
        spelt one token per character (``Vocab.encode_chars``).  The bias goes to the last token of a sequence whose earlier
        tokens are the row's most recent ones; a one-token sequence applies at every step; overlapping sequences add (in
        float64, rounded once).  Nothing is forbidden: the row may say anything and ends wherever EOS wins.  ``ValueError``:
        an empty dict, EOS or a special token in a sequence, a bias that is not finite."""
        import math
        from .text import bias_automaton, pack_automaton
        self._require("LEXICON")
        if not isinstance(sequence_bias, dict) or not sequence_bias:
            raise ValueError("sequence_bias: a non-empty dict {text or tuple of token ids: bias}")
        seqs = {}
        for key, b in sequence_bias.items():
            ids = tuple(self.vocab.encode_chars(key)) if isinstance(key, str) else tuple(int(t) for t in key)
            if not ids:
                raise ValueError(f"sequence_bias: {key!r} has no tokens")
            if any(t < 0 or t >= self.spec.vocab or t == self.spec.eos_id or t in self.vocab.special_ids for t in ids):
                raise ValueError(f"sequence_bias: {key!r} holds EOS, a special token or an id outside the vocabulary")
            if isinstance(b, bool) or not math.isfinite(float(b)):
                raise ValueError(f"sequence_bias: the bias of {key!r} is not a finite number")
            seqs[ids] = seqs.get(ids, 0.0) + float(b)
        # (the compact form: a state does not repeat the root's edges, the fallback walk finds them there)
        trans, weights = bias_automaton(seqs, compact=True)
        edges = sum(len(e) for e in trans.values())
        # (the tables are shared by every automaton of the engine: what counts is what the earlier ones have left)
        used = self.engine.automaton_used() if hasattr(self.engine, "automaton_used") else (0, 0)
        if len(trans) > MAX_AUTOMATON_STATES - used[0] or edges > MAX_AUTOMATON_EDGES - used[1]:
            raise ValueError(f"sequence_bias: the automaton of these sequences has {len(trans)} states and {edges} edges; an engine holds "
                             f"{MAX_AUTOMATON_STATES} states and {MAX_AUTOMATON_EDGES} edges over ALL its automata, and the earlier ones "
                             f"have taken {used[0]} states and {used[1]} edges")
        return Lexicon(self.engine.automaton(*pack_automaton(trans, set(trans), weights=weights, default=0, fallback=True)), frozenset(trans),
                       {}, (), True)

    def glossary(self, texts, bonus: float = 2.0, start_bonus: float = 0.0) -> Lexicon:
        """A cast list or series glossary for ``lexicon=``, as a preference instead of a confinement: once the model has started
        an entry, its continuation is preferred by ``bonus`` (natural-log units on the logit) per token; ``start_bonus``
        (default 0: a name is not suggested out of nothing) goes to every entry's first token at every step.  Every prefix of
        two or more tokens of an entry is a :meth:`sequence_bias` sequence with ``bonus`` - a prefix shared by several entries
        counts once.  The returned Lexicon carries the entries: ``Lexicon.find(recognition.ids)`` lists which were read where."""
        texts = tuple(str(t) for t in texts)
        if not texts:
            raise ValueError("glossary: no entries")
        spellings = tuple(tuple(self.vocab.encode_chars(t)) for t in texts)
        seqs = {}
        for k, sp in enumerate(spellings):
            if not sp:
                raise ValueError(f"glossary: entry {k} ({texts[k]!r}) has no characters")
            for n in range(2, len(sp) + 1):
                seqs[sp[:n]] = float(bonus)
            if start_bonus:
                seqs[sp[:1]] = float(start_bonus)
        if not seqs:
            raise ValueError("glossary: every entry is a single token and start_bonus is 0: nothing to prefer")
        lex = self.sequence_bias(seqs)
        return lex._replace(texts=texts, spellings=spellings)

    def _allowed(self, allowed, n: int) -> dict:
        """the engine keyword of ``allowed=`` ({} for None: the call the method always made)"""
        hs = _set_handles(allowed, n)
        if hs is None:
            return {}
        self._require("CONSTRAINTS")
        return dict(token_sets=hs)

    # ------------------------------------------------------------------ the request path: a source x a result kind
    def _decode_kw(self, allowed, no_repeat_ngram, n: int, prefix=None, repetition_penalty=1.0) -> dict:
        """the engine keywords of ``allowed=``, ``no_repeat_ngram=``, ``prefix=`` and ``repetition_penalty=`` ({} when none is in
        use: the call the method always made); a call's ``no_repeat_ngram`` overrides the constructor's ``no_repeat_ngram_size``
        (0 = off for this call); ``repetition_penalty`` is the call's own (``_run`` resolves the constructor's default; the
        n-best and text-scoring methods, which take no penalty, leave it at 1)"""
        kw = self._allowed(allowed, n)
        gs = _ngram_sizes(no_repeat_ngram, getattr(self, "no_repeat_ngram_size", None), n)
        if gs is not None and any(gs):
            self._require("NGRAM")
            kw["no_repeat_ngram"] = gs
        rows = _prefix_rows(prefix, n, self.vocab) if prefix is not None else None
        if rows is not None:
            self._require("PREFIX")
            kw["prefixes"] = rows
        ps = _penalties(repetition_penalty, 1.0, n)
        if ps is not None:
            self._require("PENALTY")
            kw["penalty"] = ps
        return kw

    def _single(self, allowed, no_repeat_ngram, prefix=None) -> dict:
        """the batcher keywords of one crop's ``allowed=`` / ``no_repeat_ngram=`` / ``prefix=``"""
        return _Single.batcher_kw(self._decode_kw(allowed, no_repeat_ngram, 1, prefix))

    def _run(self, source, kind: _Kind, allowed=None, no_repeat_ngram=None, prefix=None, sources=None, lexicon=None,
             repetition_penalty=None) -> list:
        """Every greedy recognise method: one row of ``kind`` per crop or region of the source - or per entry of ``sources``
        (shared encodings).  In this order: the kind's refusal (several devices), before the image is opened or any argument
        is looked at; for plain text and positions, whether the constructor's beams decode it instead (``_beam_default``: text
        gets the best hypothesis' ids, positions the best hypothesis with its token scores and positions); ``source()``, which
        opens, converts and checks the inputs; ``_decode_kw``; the ONE engine call, with the kind's flags and only the keywords
        somebody asked for; the kind's rows; ``n_forced`` of the rows that were given a prefix.  ``lexicon=`` (a token automaton per
        crop) makes the call greedy and adds ``automata=`` / ``states=True``; the rows then carry ``state``, ``accepted``, ``entry``."""
        if kind.refusal:
            self._require(kind.refusal)
        if repetition_penalty is not None and getattr(self, "beam", None) is not None:
            raise ValueError("this MangaOcr decodes with beam search (num_beams=): beam search takes no repetition_penalty=")
        beams = (kind is _TEXT or (kind is _POS and getattr(self, "beam_positions", False))) and lexicon is None and \
            self._beam_default(allowed, no_repeat_ngram, prefix, repetition_penalty)
        if beams and kind is _POS:
            self._require("BEAM_POSITIONS")
        src = source()
        if beams and kind is _POS:
            ids, lens, sc, logp, pos = self._beam(src, self.beam, True, positions=True)
            return [self._best_hypothesis(ids[i], lens[i], sc[i], logp[i], pos[i], src.rects[i] if src.rects is not None else None)
                    for i in range(len(lens))]
        if beams:
            ids, lens, _ = self._beam(src, self.beam)
            return [ids[i, 0, :lens[i, 0]].copy() for i in range(len(lens))]
        if repetition_penalty is None:
            repetition_penalty = getattr(self, "repetition_penalty", 1.0)
        kw = self._decode_kw(allowed, no_repeat_ngram, src.n if sources is None else len(sources), prefix, repetition_penalty)
        if sources is not None:
            kw["sources"] = sources
        lex = _lexicons(lexicon, src.n if sources is None else len(sources))
        if lex is None:
            rows = kind.rows(self, src, *src.call(self, **kind.flags, **kw))
            return rows if kind is _TEXT else self._mark_forced(rows, kw.get("prefixes"))
        self._require("LEXICON")
        *blocks, state = src.call(self, **kind.flags, **kw, automata=[0 if x is None else x.handle for x in lex], states=True)
        rows = kind.rows(self, src, *blocks)
        return rows if kind is _TEXT else self._mark_lexicon(self._mark_forced(rows, kw.get("prefixes")), lex, state)

    @staticmethod
    def _open(img_or_path):
        from PIL import Image
        if isinstance(img_or_path, (str, Path)):
            return Image.open(img_or_path)
        if isinstance(img_or_path, Image.Image):
            return img_or_path
        raise ValueError(f"img_or_path must be a path or PIL.Image, instead got: {img_or_path}")

    def _one(self, img_or_path):
        """source of the single-crop methods: the image, opened, through the batcher"""
        return lambda: _Single(to_pixels(self._open(img_or_path)))

    @staticmethod
    def _pil(images):
        """source of the ``recognize_batch*`` methods: PIL images"""
        return lambda: _Images([to_pixels(im) for im in images])

    @staticmethod
    def _bgr(method: str, crops_bgr, orientations) -> _Images:
        """source of the ``recognize_bgr*`` methods: BGR crops, each with the rotation code of its orientation setting"""
        from .queue_worker import rotation_code
        crops = list(crops_bgr)
        rot = None
        if orientations is not None:
            if len(orientations) != len(crops):        # zip() would truncate silently: a short list must not cost a decode
                raise ValueError(f"{method}: {len(crops)} crops but {len(orientations)} orientations")
            rot = [rotation_code(c.shape[0], c.shape[1], o) for c, o in zip(crops, orientations)]
        return _Images(crops, True, rot)

    def _texts(self, rows) -> List[str]:
        return [ids_to_text(self.vocab, r) for r in rows]

    @staticmethod
    def _mark_forced(recs: List[Recognition], prefixes) -> List[Recognition]:
        """``Recognition.n_forced`` of the rows that were given a prefix (a row that finished inside it counts what it took)"""
        if prefixes is None:
            return recs
        return [replace(r, n_forced=min(len(p), max(len(r.ids) - 1, 0))) if p else r for r, p in zip(recs, prefixes)]

    def _mark_lexicon(self, recs: List[Recognition], lex, state) -> List[Recognition]:
        """``Recognition.state`` / ``accepted`` / ``entry`` of a call with ``lexicon=``: accepted = the row ended by EOS in an
        accepting state of its automaton; entry = the lexicon entry that state stands for"""
        out = []
        for r, x, s in zip(recs, lex, state):
            s = int(s)
            if x is not None and x.soft:        # a soft automaton confines nothing: there is nothing to accept
                out.append(replace(r, state=s, accepted=None, entry=None))
                continue
            ok = x is not None and len(r.ids) > 1 and int(r.ids[-1]) == self.spec.eos_id and s in x.accepting
            out.append(replace(r, state=s, accepted=bool(ok), entry=x.entries.get(s) if ok else None))
        return out

    def _recognitions(self, ids, lens, logp) -> List[Recognition]:
        return [Recognition.from_row(self.vocab, ids[i], logp[i], lens[i]) for i in range(len(lens))]

    def _recognitions_alt(self, ids, lens, logp, alt_ids, alt_logp) -> List[Recognition]:
        return [Recognition.from_row(self.vocab, ids[i], logp[i], lens[i], alt_ids[i], alt_logp[i]) for i in range(len(lens))]

    def _recognitions_pos(self, ids, lens, logp, pos, rects=None) -> List[Recognition]:
        return [Recognition.from_row(self.vocab, ids[i], logp[i], lens[i], pos_row=pos[i], rect=rects[i] if rects is not None else None)
                for i in range(len(lens))]

    # ------------------------------------------------------------------ batch surface (callers that hold many crops)
    def recognize_ids(self, crops: Sequence[np.ndarray], bgr: bool = False, rotate: Optional[Sequence[int]] = None, *,
                      allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> List[np.ndarray]:
        """uint8 crops of any sizes ([h,w] luminance or [h,w,3] RGB; BGR with ``bgr=True``; ``rotate``: per crop 0 / 1 (90
        degrees clockwise) / 2 (counter-clockwise), done by the device) -> token ids (without padding).  ``allowed``: a
        token set of :meth:`token_set` for all crops, or one per crop.  ``no_repeat_ngram``: the no-repeat n-gram size of this
        call, an int for all crops or one per crop, 0 = off (None: the constructor's ``no_repeat_ngram_size``).  ``prefix``:
        tokens the rows start with, behind the start token - a ``str`` (one token per character, ``Vocab.encode_chars``) or a
        flat sequence of token ids for all crops, or a sequence of those (or None) per crop; the engine scores them and decodes
        on from there (include/mocr.h, "forced prefixes").  ``lexicon``: a :class:`Lexicon` of :meth:`lexicon` / :meth:`automaton`
        for all crops, or one (or None) per crop - the row is decoded under that token automaton (include/mocr.h, "token
        automata"); the scored kinds then fill ``Recognition.state`` / ``accepted`` / ``entry``.  Every greedy ``recognize*``
        method takes all four, and ``repetition_penalty``: transformers' setting of that name under greedy decoding, a float for
        all crops or one per crop, finite and > 0, 1 = off (None: the constructor's ``repetition_penalty``; include/mocr.h,
        "repetition penalty") - a reader built with ``num_beams=`` refuses it.  A call with ``lexicon=`` decodes GREEDILY even when this MangaOcr was built with ``num_beams=``:
        :meth:`match` searches a lexicon with beams, :meth:`search` a glossary or ``sequence_bias`` (the biases then count inside
        the hypotheses' scores)."""
        return self._run(lambda: _Images(list(crops), bgr, rotate), _TEXT, allowed, no_repeat_ngram, prefix, lexicon=lexicon, repetition_penalty=repetition_penalty)

    def recognize(self, img_or_path, *, allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> str:
        """``__call__`` (which keeps the reference's signature) with ``allowed=``: one crop decoded under a token set, and
        ``no_repeat_ngram=``: this call's no-repeat n-gram size (None: the constructor's ``no_repeat_ngram_size``)."""
        return self._texts(self._run(self._one(img_or_path), _TEXT, allowed, no_repeat_ngram, prefix, lexicon=lexicon, repetition_penalty=repetition_penalty))[0]

    def recognize_batch(self, images: Sequence, *, allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> List[str]:
        """All crops of a page (or chapter) at once - what ``_collect_manga_detections``
        (``src/ui/main_window.py:9462-9476``) does one region at a time."""
        return self._texts(self.recognize_ids([to_pixels(im) for im in images], allowed=allowed, no_repeat_ngram=no_repeat_ngram, prefix=prefix, lexicon=lexicon, repetition_penalty=repetition_penalty))

    def recognize_batch_arrays(self, crops: Sequence[np.ndarray], *, allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> List[str]:
        """uint8 arrays ([h,w] luminance or [h,w,3] RGB, any sizes) -> strings: what a caller that already holds numpy
        crops (the crop-job queue) uses instead of wrapping each one in a PIL image."""
        return self._texts(self.recognize_ids(crops, allowed=allowed, no_repeat_ngram=no_repeat_ngram, prefix=prefix, lexicon=lexicon, repetition_penalty=repetition_penalty))

    def recognize_bgr(self, crops_bgr: Sequence[np.ndarray], orientations: Optional[Sequence[str]] = None, *, allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> List[str]:
        """BGR crops exactly as the crop tools and the worker hold them (``cropped_cv_img``, ``src/core/workers.py:300``):
        the BGR -> RGB swap of ``src/ui/main_window.py:9800`` is folded into the device's luminance conversion, and with
        ``orientations`` (the jobs' "Auto-Detect" / "Vertical" / "Horizontal" settings) the orientation-only rotation of
        ``src/core/workers.py:320-326`` / ``src/ui/main_window.py:9787-9795`` into the device's resize addressing."""
        src = self._bgr("recognize_bgr", crops_bgr, orientations)
        return self._texts(self._run(lambda: src, _TEXT, allowed, no_repeat_ngram, prefix, lexicon=lexicon, repetition_penalty=repetition_penalty))

    def recognize_regions(self, pages_bgr: Sequence[np.ndarray], regions, *, allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> List[str]:
        """``regions``: (page_index, x, y, w, h) bounding rectangles on BGR pages; every page is uploaded once and
        the padded crops (``src/ui/main_window.py:9530-9540``) are cut on the device.  One string per region
        ('' for a region reduced to a sliver, like the reference)."""
        return self._texts(self._run(lambda: _Regions(list(pages_bgr), list(regions)), _TEXT, allowed, no_repeat_ngram, prefix, lexicon=lexicon, repetition_penalty=repetition_penalty))

    # ------------------------------------------------------------------ scored surface: the same recognitions + confidence
    def recognize_scored(self, img_or_path, *, allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> Recognition:
        """``__call__`` with the recogniser's confidence: same text, plus the token log-probabilities computed on the
        device (include/mocr.h, "token scores").  Goes through the same batcher as ``__call__``; scored and unscored
        callers may share a batch."""
        return self._run(self._one(img_or_path), _SCORED, allowed, no_repeat_ngram, prefix, lexicon=lexicon, repetition_penalty=repetition_penalty)[0]

    def recognize_batch_scored(self, images: Sequence, *, allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> List[Recognition]:
        """``recognize_batch`` with confidences."""
        return self._run(self._pil(images), _SCORED, allowed, no_repeat_ngram, prefix, lexicon=lexicon, repetition_penalty=repetition_penalty)

    def recognize_bgr_scored(self, crops_bgr: Sequence[np.ndarray], orientations: Optional[Sequence[str]] = None, *,
                             allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> List[Recognition]:
        """``recognize_bgr`` with confidences."""
        return self._run(lambda: self._bgr("recognize_bgr_scored", crops_bgr, orientations), _SCORED, allowed, no_repeat_ngram, prefix, lexicon=lexicon, repetition_penalty=repetition_penalty)

    def recognize_regions_scored(self, pages_bgr: Sequence[np.ndarray], regions, *, allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> List[Recognition]:
        """``recognize_regions`` with confidences; a region reduced to a sliver gives text '' and confidence 0.0."""
        return self._run(lambda: _Regions(list(pages_bgr), list(regions)), _SCORED, allowed, no_repeat_ngram, prefix, lexicon=lexicon, repetition_penalty=repetition_penalty)

    # ------------------------------------------------------------------ alternatives surface: + the runners-up of every position
    def recognize_alternatives(self, img_or_path, *, allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> Recognition:
        """``recognize_scored`` plus, for every generated position, the four most probable tokens and their log-probabilities
        (``Recognition.alt_ids`` / ``alt_logprobs`` / ``candidates``; include/mocr.h, "token alternatives").  Same text; goes
        through the same batcher as ``__call__``, and callers of all three kinds may share a batch."""
        return self._run(self._one(img_or_path), _ALTS, allowed, no_repeat_ngram, prefix, lexicon=lexicon, repetition_penalty=repetition_penalty)[0]

    def recognize_batch_alternatives(self, images: Sequence, *, allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> List[Recognition]:
        """``recognize_batch`` with confidences and alternatives."""
        return self._run(self._pil(images), _ALTS, allowed, no_repeat_ngram, prefix, lexicon=lexicon, repetition_penalty=repetition_penalty)

    def recognize_bgr_alternatives(self, crops_bgr: Sequence[np.ndarray], orientations: Optional[Sequence[str]] = None, *,
                                   allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> List[Recognition]:
        """``recognize_bgr`` with confidences and alternatives."""
        return self._run(lambda: self._bgr("recognize_bgr_alternatives", crops_bgr, orientations), _ALTS, allowed, no_repeat_ngram, prefix, lexicon=lexicon, repetition_penalty=repetition_penalty)

    def recognize_regions_alternatives(self, pages_bgr: Sequence[np.ndarray], regions, *, allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> List[Recognition]:
        """``recognize_regions`` with confidences and alternatives; a region reduced to a sliver gives text '', confidence
        0.0 and empty alternatives."""
        return self._run(lambda: _Regions(list(pages_bgr), list(regions)), _ALTS, allowed, no_repeat_ngram, prefix, lexicon=lexicon, repetition_penalty=repetition_penalty)

    # ------------------------------------------------------------------ positions surface: + where each token was read
    def recognize_positions(self, img_or_path, *, allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> Recognition:
        """``recognize_scored`` plus ``Recognition.positions``: per token where in the crop the decoder looked when it emitted
        it (include/mocr.h, "token positions"); ``Recognition.boxes(width, height)`` gives pixel rectangles.  Same text and
        scores; goes through the same batcher as ``__call__``, and callers of all kinds may share a batch."""
        return self._run(self._one(img_or_path), _POS, allowed, no_repeat_ngram, prefix, lexicon=lexicon, repetition_penalty=repetition_penalty)[0]

    def recognize_batch_positions(self, images: Sequence, *, allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> List[Recognition]:
        """``recognize_batch_scored`` with positions."""
        return self._run(self._pil(images), _POS, allowed, no_repeat_ngram, prefix, lexicon=lexicon, repetition_penalty=repetition_penalty)

    def recognize_bgr_positions(self, crops_bgr: Sequence[np.ndarray], orientations: Optional[Sequence[str]] = None, *,
                                allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> List[Recognition]:
        """``recognize_bgr_scored`` with positions.  The positions are those of the crop the encoder saw, i.e. after the
        orientation's rotation: pass the crop's rotation code (``queue_worker.rotation_code``) to ``Recognition.boxes`` to get
        rectangles on the crop as it was handed in."""
        return self._run(lambda: self._bgr("recognize_bgr_positions", crops_bgr, orientations), _POS, allowed, no_repeat_ngram, prefix, lexicon=lexicon, repetition_penalty=repetition_penalty)

    def recognize_regions_positions(self, pages_bgr: Sequence[np.ndarray], regions, *, allowed=None, no_repeat_ngram=None, prefix=None, lexicon=None, repetition_penalty=None) -> List[Recognition]:
        """``recognize_regions_scored`` with positions: every Recognition carries ``rect``, the region's padded, clipped
        rectangle on its page (``regions.padded_rect``), so ``Recognition.page_boxes()`` gives the tokens' rectangles in page
        pixels.  A region reduced to a sliver gives text '', no positions rows and ``rect`` None."""
        return self._run(lambda: _Regions(list(pages_bgr), list(regions)).with_rects(), _POS, allowed, no_repeat_ngram, prefix, lexicon=lexicon, repetition_penalty=repetition_penalty)

    # ------------------------------------------------------------------ forced prefixes: score a given text
    def _text_prefix(self, text) -> List[int]:
        ids = self.vocab.encode_chars(text) if isinstance(text, str) else [int(t) for t in text]
        if len(ids) + 2 > self.spec.max_len:
            raise ValueError(f"score_text: {len(ids)} tokens do not fit max_len {self.spec.max_len} with the start token and EOS")
        return ids + [int(self.spec.eos_id)]

    def score_text(self, img_or_path, text) -> Recognition:
        """How likely is ``text`` (a ``str``, one token per character, or token ids) for this crop: the row is forced to the
        text plus EOS and scored, so ``Recognition.logprob`` is ``log p(text | crop)`` and ``logprobs`` its per-token terms."""
        return self.recognize_scored(img_or_path, prefix=self._text_prefix(text))

    def score_texts(self, images: Sequence, texts: Sequence) -> List[Recognition]:
        """``score_text`` for many crops at once: one text per crop."""
        images, texts = list(images), list(texts)
        if len(images) != len(texts):
            raise ValueError(f"score_texts: {len(images)} crops but {len(texts)} texts")
        return self.recognize_batch_scored(images, prefix=[self._text_prefix(t) for t in texts])

    # ------------------------------------------------------------------ shared encodings: many rows of one crop
    def score_candidates(self, img_or_path, texts) -> List[Recognition]:
        """``score_text`` for many texts of ONE crop, in the order given: every text (a ``str`` or token ids) is forced through
        EOS and scored, so ``Recognition.logprob`` is ``log p(text | crop)``.  One engine call; the crop is encoded once for
        all of its rows (include/mocr.h, "shared encodings")."""
        self._require("SCORES")
        self._require("PREFIX")      # MultiGpuEngine: the workers make the plain greedy call
        prefixes = [self._text_prefix(t) for t in texts]
        if not prefixes:
            return []
        return self._run(lambda: _Images([to_pixels(self._open(img_or_path))]), _SCORED, prefix=prefixes, sources=[0] * len(prefixes))

    @staticmethod
    def _nbest_branches(rec: Recognition, count: int) -> List[Tuple[int, int]]:
        """The ``count`` cheapest single-token deviations (t, j) of an alternatives row: generated position ``t`` before the
        row's last one, candidate ``j >= 1`` with a token and a finite log-probability; cost ``alt_logprobs[t, 0] -
        alt_logprobs[t, j]``, ties to the lower ``t``, then the lower ``j``."""
        found = []
        for t in range(len(rec.alt_ids) - 1):
            top = float(rec.alt_logprobs[t, 0])
            for j in range(1, rec.alt_ids.shape[1]):
                lp = float(rec.alt_logprobs[t, j])
                if rec.alt_ids[t, j] >= 0 and np.isfinite(lp):
                    found.append((top - lp, t, j))
        found.sort()
        return [(t, j) for _, t, j in found[:max(count, 0)]]

    def recognize_batch_nbest(self, images: Sequence, k: int = 4, *, allowed=None, no_repeat_ngram=None) -> List[List[Recognition]]:
        """Up to ``k`` readings per crop, most probable first, in two engine calls for the whole batch.  Call 1 decodes every
        crop greedily with alternatives.  Call 2 takes, per crop, the ``k - 1`` cheapest single-token deviations from that
        reading - position ``t`` before the row's last, candidate ``j >= 1``, cost ``alt_logprobs[t, 0] - alt_logprobs[t, j]`` -
        and continues each greedily from ``Recognition.branch(t, j)``, scored, all crops' branches in one call that encodes
        every crop once (include/mocr.h, "shared encodings").  A crop's result is its greedy row plus the continuations,
        rows with equal ids dropped (the first kept), sorted by ``logprob`` descending (ties in that order of construction):
        at most ``k`` entries, fewer when fewer deviations exist; ``k = 1`` is the greedy row and makes no second call.
        ``allowed`` / ``no_repeat_ngram`` apply to both calls, per crop.

        This is NOT beam search and is not guaranteed to hold the ``k`` most probable sequences: it holds the greedy reading
        and the ``k - 1`` cheapest one-token departures from it, each continued greedily.  Beam search proper is
        :meth:`recognize_beam` / :meth:`recognize_batch_beam`."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"recognize_nbest: k must be an int >= 1, instead got {k!r}")
        self._require("ALTERNATIVES")
        if k > 1:
            self._require("PREFIX")
        src = self._pil(images)()
        if not src.n:
            return []
        kw = self._decode_kw(allowed, no_repeat_ngram, src.n)
        first = self._recognitions_alt(*src.call(self, alternatives=True, **kw))
        results = [[r] for r in first]
        prefixes, owner = [], []
        if k > 1:
            for c, rec in enumerate(first):
                for t, j in self._nbest_branches(rec, k - 1):
                    prefixes.append(rec.branch(t, j))
                    owner.append(c)
        if prefixes:
            used = sorted(set(owner))       # a crop without a deviation (a one-token row) is not sent again
            place = {c: i for i, c in enumerate(used)}
            kw2 = {name: [vals[c] for c in owner] for name, vals in kw.items()}
            out = _Images([src.crops[c] for c in used]).call(self, scores=True, prefixes=prefixes, sources=[place[c] for c in owner], **kw2)
            for c, rec in zip(owner, self._mark_forced(self._recognitions(*out), prefixes)):
                results[c].append(rec)
        ranked = []
        for rows in results:
            kept = []
            for r in rows:
                if not any(np.array_equal(r.ids, q.ids) for q in kept):
                    kept.append(r)
            kept.sort(key=lambda r: -r.logprob)     # (stable: ties keep the order of construction)
            ranked.append(kept[:k])
        return ranked

    def recognize_nbest(self, img_or_path, k: int = 4, *, allowed=None, no_repeat_ngram=None) -> List[Recognition]:
        """``recognize_batch_nbest`` for one crop."""
        return self.recognize_batch_nbest([self._open(img_or_path)], k, allowed=allowed, no_repeat_ngram=no_repeat_ngram)[0]

    # ------------------------------------------------------------------ beam search
    def _beam_default(self, allowed, no_repeat_ngram, prefix, repetition_penalty=None) -> bool:
        """does a plain call decode with the constructor's beams?  (They do not combine with the per-call keywords.)"""
        if getattr(self, "beam", None) is None:
            return False
        if allowed is not None or no_repeat_ngram is not None or prefix is not None:
            raise ValueError("this MangaOcr decodes with beam search (num_beams=): allowed= / no_repeat_ngram= / prefix= do not combine with it")
        if repetition_penalty is not None:
            raise ValueError("this MangaOcr decodes with beam search (num_beams=): beam search takes no repetition_penalty=")
        return True

    def _beam(self, src, beam: BeamConfig, token_scores: bool = False, allowed=None, positions: bool = False, lexicons=None,
              soft: bool = False):
        """(ids [n, K, max_len], lengths [n, K], scores [n, K]) of a source: one crop through the batcher, any number of crops
        or regions max_batch // K of them per engine call (a beam request fits one batch: n * K <= max_batch).  With
        ``token_scores`` also logp [n, K, max_len]; ``allowed``: the crops' token sets; with ``positions`` also, last, pos
        [n, K, max_len, 5].  ``lexicons`` (the ``match`` methods): one Lexicon or None per crop - the beams walk the crops'
        automata, and the hypotheses' states [n, K] come behind everything else; ``soft`` (the ``search`` methods): those automata
        may be soft, the call is the engine's ``beam_soft=True`` one.  The engine is passed only what was asked."""
        self._require("BEAM")
        if positions:
            self._require("BEAM_POSITIONS")
        hs = _set_handles(allowed, src.n)
        if hs is not None:
            self._require("CONSTRAINTS")
        flags = dict(**(dict(beam_scores=True) if token_scores else {}), **(dict(beam_positions=True) if positions else {}))
        if isinstance(src, _Single):
            kw = dict(flags)
            if hs is not None:
                kw["beam_set"] = hs[0]
            if lexicons is not None and lexicons[0] is not None:
                kw["beam_automaton"] = lexicons[0].handle
                if soft:
                    kw["beam_soft"] = True
            out = tuple(a[None] for a in self._batcher.submit(src.pixels, beam=beam, **kw).result())
            if lexicons is not None and lexicons[0] is None:        # (no automaton: the batcher made the call it always made)
                out += (np.full(out[1].shape, -1, dtype=np.int32),)
            return out
        if not src.n and isinstance(src, _Images):
            src = _Images([])       # no crops: the bare call, which only shapes the empty result
        step = max(1, int(self.max_batch) // beam.num_beams)
        aut = None if lexicons is None else [0 if x is None else x.handle for x in lexicons]
        kw = lambda a: dict(**flags, **(dict(beam_sets=hs[a:a + step]) if hs is not None else {}),
                            **(dict(beam_automata=aut[a:a + step], beam_states=True) if aut is not None else {}),
                            **(dict(beam_soft=True) if soft and aut is not None else {}))
        parts = [src.call(self, a, a + step, beam=beam, **kw(a)) for a in range(0, src.n, step)] or [src.call(self, beam=beam, **kw(0))]
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(3 + bool(token_scores) + bool(positions) + (aut is not None)))

    def _hypotheses(self, ids, lens, scores, logp=None, pos=None, rect=None) -> List[Recognition]:
        """one crop's [K, max_len] / [K] / [K] (/ [K, max_len] / [K, max_len, 5]) -> its finished hypotheses, best first (empty
        slots dropped); with ``logp`` they carry their token log-probabilities and the confidence of a greedy row
        (Recognition.from_row), with ``pos`` their ``positions`` [len, 5] - and ``rect``, a region's rectangle on its page"""
        none = np.zeros(0, dtype=np.float32)
        if logp is not None:
            return [replace(Recognition.from_row(self.vocab, ids[j], logp[j], lens[j], pos_row=None if pos is None else pos[j], rect=rect),
                            sequence_score=float(scores[j])) for j in range(len(lens)) if lens[j] > 0]
        where = lambda j: {} if pos is None else dict(positions=np.array(pos[j, :lens[j]], dtype=np.float32).reshape(-1, pos.shape[-1]),
                                                      rect=tuple(int(v) for v in rect) if rect is not None else None)
        return [Recognition(ids_to_text(self.vocab, ids[j, :lens[j]]), np.array(ids[j, :lens[j]], dtype=np.int32), none, 0.0, 0.0,
                            sequence_score=float(scores[j]), **where(j)) for j in range(len(lens)) if lens[j] > 0]

    def _best_hypothesis(self, ids, lens, scores, logp, pos, rect=None) -> Recognition:
        """the ``*_positions`` methods of a MangaOcr that decodes with beams: one crop's best hypothesis with its token scores and
        positions; a region reduced to a sliver (no hypothesis) gives what the greedy methods give - text '', no rows, no rect"""
        hyps = self._hypotheses(ids[:1], lens[:1], scores[:1], logp[:1], pos[:1], rect)
        return hyps[0] if hyps else Recognition.from_row(self.vocab, ids[0], logp[0], 0, pos_row=pos[0])

    def _run_beam(self, source, *config, token_scores: bool = False, allowed=None, positions: bool = False, lexicon=None) -> List[List[Recognition]]:
        """the ``*_beam`` methods: the configuration is checked, then the inputs; one list of hypotheses per crop or region.
        ``lexicon=`` is refused: beam search takes no token automaton (include/mocr.h, "token automata")"""
        if lexicon is not None:
            raise ValueError("the *_beam methods do not combine with lexicon= (token automata are for greedy decoding here): "
                             "match() / match_batch() / match_bgr() / match_regions() search a lexicon with beams")
        beam = BeamConfig(*config)
        src = source()
        if positions and isinstance(src, _Regions):
            src = src.with_rects()
        ids, lens, sc, *rest = self._beam(src, beam, bool(token_scores), allowed, bool(positions))
        logp = rest.pop(0) if token_scores else None
        pos = rest.pop(0) if positions else None
        rects = src.rects if positions else None
        return [self._hypotheses(ids[i], lens[i], sc[i], None if logp is None else logp[i], None if pos is None else pos[i],
                                 rects[i] if rects is not None else None) for i in range(len(lens))]

    def recognize_beam(self, img_or_path, num_beams: int = 4, length_penalty: float = 1.0, early_stopping=False,
                       no_repeat_ngram: int = 0, *, token_scores: bool = False, allowed=None, positions: bool = False, lexicon=None) -> List[Recognition]:
        """Beam search for one crop (include/mocr.h, "beam search"): what transformers' ``generate(num_beams=...,
        length_penalty=..., early_stopping=..., no_repeat_ngram_size=...)`` returns with ``num_return_sequences=num_beams`` -
        the finished hypotheses, best first, each with its ``sequence_score``.  ``num_beams`` 2 .. 4; ``early_stopping``
        False, True or "never".  Goes through the batcher; beam and greedy callers never share a batch.
        ``token_scores=True``: every hypothesis also carries ``logprobs`` (one per token behind the start token: the
        log-probability the search gave it, EOS included), ``confidence`` and ``min_prob`` as a greedy scored row does.
        ``allowed``: a :class:`TokenSet` - the search runs under it: a token outside scores -inf at every step, WITHOUT the
        renormalising of the greedy ``allowed=`` (transformers' ``prefix_allowed_tokens_fn``; include/mocr.h).
        ``positions=True``: every hypothesis also carries ``positions`` float32 ``[len, 5]`` - where the decoder looked when the
        search appended each of ITS tokens, what a greedy row teacher-forced on the hypothesis would give (include/mocr.h, "beam
        search with token positions") - so ``Recognition.boxes`` works on it.  Nothing else of the result moves."""
        self._require("BEAM")
        return self._run_beam(self._one(img_or_path), num_beams, length_penalty, early_stopping, no_repeat_ngram, token_scores=token_scores,
                              allowed=allowed, positions=positions, lexicon=lexicon)[0]

    def recognize_batch_beam(self, images: Sequence, num_beams: int = 4, length_penalty: float = 1.0, early_stopping=False,
                             no_repeat_ngram: int = 0, *, token_scores: bool = False, allowed=None,
                             positions: bool = False, lexicon=None) -> List[List[Recognition]]:
        """``recognize_beam`` for many crops: one list of hypotheses per crop (``allowed``: one set for all, or one per crop)."""
        return self._run_beam(self._pil(images), num_beams, length_penalty, early_stopping, no_repeat_ngram, token_scores=token_scores, allowed=allowed,
                              positions=positions, lexicon=lexicon)

    def recognize_bgr_beam(self, crops_bgr: Sequence[np.ndarray], orientations: Optional[Sequence[str]] = None, num_beams: int = 4,
                           length_penalty: float = 1.0, early_stopping=False, no_repeat_ngram: int = 0, *, token_scores: bool = False,
                           allowed=None, positions: bool = False, lexicon=None) -> List[List[Recognition]]:
        """``recognize_bgr`` with beam search: one list of hypotheses per crop (``token_scores`` / ``allowed`` / ``positions``: see
        recognize_beam; the positions are those of the rotated crop, as for ``recognize_bgr_positions``)."""
        return self._run_beam(lambda: self._bgr("recognize_bgr_beam", crops_bgr, orientations), num_beams, length_penalty, early_stopping, no_repeat_ngram,
                              token_scores=token_scores, allowed=allowed, positions=positions, lexicon=lexicon)

    def recognize_regions_beam(self, pages_bgr: Sequence[np.ndarray], regions, num_beams: int = 4, length_penalty: float = 1.0,
                               early_stopping=False, no_repeat_ngram: int = 0, *, token_scores: bool = False,
                               allowed=None, positions: bool = False, lexicon=None) -> List[List[Recognition]]:
        """``recognize_regions`` with beam search: one list of hypotheses per region ([] for a sliver; ``token_scores`` /
        ``allowed``: see recognize_beam, one set per region; ``positions``: every hypothesis also carries ``rect``, so
        ``page_boxes()`` works)."""
        return self._run_beam(lambda: _Regions(list(pages_bgr), list(regions)), num_beams, length_penalty, early_stopping, no_repeat_ngram,
                              token_scores=token_scores, allowed=allowed, positions=positions, lexicon=lexicon)

    # ------------------------------------------------------------------ beam search under a lexicon
    def _run_match(self, source, lexicon, k, length_penalty, early_stopping, no_repeat_ngram, token_scores, allowed, positions,
                   raw, soft: bool = False) -> List[List[Recognition]]:
        """the ``match*`` methods: the refusals (several devices), the configuration, the inputs, the lexicons; ONE beam search per
        crop whose K beams walk the crop's automaton; per crop the hypotheses marked with ``state`` / ``accepted`` / ``entry``,
        and unless ``raw`` only the distinct accepted ones that are no padding beam's duplicate.  ``soft`` (the ``search*``
        methods, always ``raw``): the lexicons may be soft, and a soft one leaves ``accepted`` / ``entry`` None"""
        self._require("BEAM")
        self._require("LEXICON")
        if lexicon is None:
            raise ValueError("match: lexicon= is required (a Lexicon of MangaOcr.lexicon() / automaton(), or one or None per crop)")
        beam = BeamConfig(k, length_penalty, early_stopping, no_repeat_ngram)
        src = source()
        if positions and isinstance(src, _Regions):
            src = src.with_rects()
        lex = _lexicons(lexicon, src.n) or [None] * src.n
        if not soft and any(x is not None and x.soft for x in lex):
            raise ValueError("match: it ranks what a lexicon ALLOWS and takes no soft automaton (sequence_bias / glossary / weights): "
                             "search() / search_batch() / search_bgr() / search_regions() run beam search under one")
        ids, lens, sc, *rest = self._beam(src, beam, bool(token_scores), allowed, bool(positions), lex, soft)
        logp = rest.pop(0) if token_scores else None
        pos = rest.pop(0) if positions else None
        state = rest.pop(0)
        rects = src.rects if positions else None
        eos = self.spec.eos_id
        # a padding beam's descendant scores -1e9 / (tokens generated) ** length_penalty: at or below this, whatever its length
        junk = -1.0e9 / float(self.spec.max_len) ** max(float(beam.length_penalty), 0.0)
        out = []
        for i, x in enumerate(lex):
            live = [j for j in range(lens.shape[1]) if lens[i, j] > 0]
            hyps = self._hypotheses(ids[i], lens[i], sc[i], None if logp is None else logp[i], None if pos is None else pos[i],
                                    rects[i] if rects is not None else None)
            marked = []
            for j, h in zip(live, hyps):
                st = int(state[i, j])
                if x is not None and x.soft:        # a soft automaton confines nothing: there is nothing to accept
                    marked.append(replace(h, state=st, accepted=None, entry=None))
                    continue
                ok = x is not None and len(h.ids) > 1 and int(h.ids[-1]) == eos and st in x.accepting
                marked.append(replace(h, state=st, accepted=bool(ok), entry=x.entries.get(st) if ok else None))
            if not raw:
                seen, kept = set(), []
                for h in marked:
                    key = h.entry if h.entry is not None else ("state", h.state, tuple(int(t) for t in h.ids))
                    if h.accepted and h.sequence_score > junk and key not in seen:
                        seen.add(key)
                        kept.append(h)
                marked = kept
            out.append(marked)
        return out

    def match(self, img_or_path, lexicon, k: int = 4, *, length_penalty: float = 1.0, early_stopping=False, no_repeat_ngram: int = 0,
              token_scores: bool = False, allowed=None, positions: bool = False, raw: bool = False) -> List[Recognition]:
        """The entries of ``lexicon`` (:meth:`lexicon` / :meth:`automaton`) that fit one crop best: a beam search of ``k`` beams
        (2 .. 4) whose every beam walks the automaton (include/mocr.h, "beam search under a token automaton") - transformers'
        ``generate(num_beams=k, prefix_allowed_tokens_fn=...)``.  Where the greedy ``lexicon=`` commits to one branch of the trie at
        the first character, this ranks whole entries.  Returns the distinct accepted entries in score order, at most ``k``: each
        a :class:`Recognition` with ``text``, ``sequence_score``, ``state``, ``accepted=True`` and ``entry``.  A hypothesis is
        dropped if it did not end by EOS in an accepting state, if it is a padding beam's duplicate (the lexicon has fewer
        reachable entries than beams; such a hypothesis scores -1e9 / tokens ** length_penalty, so the line is drawn at
        -1e9 / max_len ** length_penalty), or if it repeats an earlier one.  ``raw=True``: all hypotheses as
        the engine delivered them, with ``state`` / ``accepted`` / ``entry`` filled.  ``length_penalty`` / ``early_stopping`` /
        ``no_repeat_ngram`` / ``token_scores`` / ``allowed`` / ``positions``: as for :meth:`recognize_beam`.  Goes through the
        batcher; only requests of one beam configuration share a batch."""
        return self._run_match(self._one(img_or_path), lexicon, k, length_penalty, early_stopping, no_repeat_ngram, token_scores, allowed,
                               positions, raw)[0]

    def match_batch(self, images: Sequence, lexicon, k: int = 4, *, length_penalty: float = 1.0, early_stopping=False,
                    no_repeat_ngram: int = 0, token_scores: bool = False, allowed=None, positions: bool = False,
                    raw: bool = False) -> List[List[Recognition]]:
        """:meth:`match` for many crops: one list per crop (``lexicon``: one for all, or one Lexicon or None per crop - a crop
        without one is searched freely and, accepting nothing, keeps its hypotheses only with ``raw=True``)."""
        return self._run_match(self._pil(images), lexicon, k, length_penalty, early_stopping, no_repeat_ngram, token_scores, allowed, positions, raw)

    def match_bgr(self, crops_bgr: Sequence[np.ndarray], lexicon, orientations: Optional[Sequence[str]] = None, k: int = 4, *,
                  length_penalty: float = 1.0, early_stopping=False, no_repeat_ngram: int = 0, token_scores: bool = False, allowed=None,
                  positions: bool = False, raw: bool = False) -> List[List[Recognition]]:
        """:meth:`match_batch` on BGR crops with their orientation settings, as ``recognize_bgr`` takes them."""
        return self._run_match(lambda: self._bgr("match_bgr", crops_bgr, orientations), lexicon, k, length_penalty, early_stopping,
                               no_repeat_ngram, token_scores, allowed, positions, raw)

    def match_regions(self, pages_bgr: Sequence[np.ndarray], regions, lexicon, k: int = 4, *, length_penalty: float = 1.0,
                      early_stopping=False, no_repeat_ngram: int = 0, token_scores: bool = False, allowed=None,
                      positions: bool = False, raw: bool = False) -> List[List[Recognition]]:
        """:meth:`match_batch` on regions of BGR pages, as ``recognize_regions`` takes them: [] for a sliver."""
        return self._run_match(lambda: _Regions(list(pages_bgr), list(regions)), lexicon, k, length_penalty, early_stopping,
                               no_repeat_ngram, token_scores, allowed, positions, raw)

    # ------------------------------------------------------------------ beam search under a glossary
    def search(self, img_or_path, bias, k: int = 4, *, length_penalty: float = 1.0, early_stopping=False, no_repeat_ngram: int = 0,
               token_scores: bool = False, allowed=None, positions: bool = False) -> List[Recognition]:
        """Beam search for one crop with a glossary's preferences INSIDE the hypotheses' scores (include/mocr.h, "beam search
        under soft token automata"): transformers' ``generate(num_beams=k, sequence_bias=...)``.  ``bias``: a Lexicon of
        :meth:`glossary` / :meth:`sequence_bias` / :meth:`automaton` with ``weights=`` or ``default=`` (a hard Lexicon is
        allowed, and then confines as in :meth:`match`).  An edge's weight is added to its token's log-probability behind the
        log_softmax - nothing renormalises, unlike the greedy ``lexicon=`` - so a cast list re-ranks whole hypotheses instead of
        one token at a time.  Returns the finished hypotheses as the engine delivered them, best first, each with
        ``sequence_score`` (the biases included) and ``state``; ``accepted`` / ``entry`` are None under a soft Lexicon and
        :meth:`match`'s under a hard one.  ``Lexicon.find(hypothesis.ids)`` lists the glossary entries a hypothesis holds.
        ``k`` 2 .. 4; ``length_penalty`` / ``early_stopping`` / ``no_repeat_ngram`` / ``token_scores`` (the biased values, whose
        sum over ``(len - 1) ** length_penalty`` is the score) / ``allowed`` / ``positions``: as for :meth:`recognize_beam`.
        A MangaOcr built with ``num_beams=`` still decodes a plain ``recognize(..., lexicon=)`` greedily: this is the call that
        searches with beams under a glossary.  Goes through the batcher; only requests of one beam configuration share a batch."""
        return self._run_match(self._one(img_or_path), bias, k, length_penalty, early_stopping, no_repeat_ngram, token_scores, allowed,
                               positions, True, True)[0]

    def search_batch(self, images: Sequence, bias, k: int = 4, *, length_penalty: float = 1.0, early_stopping=False,
                     no_repeat_ngram: int = 0, token_scores: bool = False, allowed=None, positions: bool = False) -> List[List[Recognition]]:
        """:meth:`search` for many crops: one list per crop (``bias``: one Lexicon for all, or one Lexicon or None per crop - a crop
        without one is searched freely)."""
        return self._run_match(self._pil(images), bias, k, length_penalty, early_stopping, no_repeat_ngram, token_scores, allowed, positions,
                               True, True)

    def search_bgr(self, crops_bgr: Sequence[np.ndarray], bias, orientations: Optional[Sequence[str]] = None, k: int = 4, *,
                   length_penalty: float = 1.0, early_stopping=False, no_repeat_ngram: int = 0, token_scores: bool = False, allowed=None,
                   positions: bool = False) -> List[List[Recognition]]:
        """:meth:`search_batch` on BGR crops with their orientation settings, as ``recognize_bgr`` takes them."""
        return self._run_match(lambda: self._bgr("search_bgr", crops_bgr, orientations), bias, k, length_penalty, early_stopping,
                               no_repeat_ngram, token_scores, allowed, positions, True, True)

    def search_regions(self, pages_bgr: Sequence[np.ndarray], regions, bias, k: int = 4, *, length_penalty: float = 1.0,
                       early_stopping=False, no_repeat_ngram: int = 0, token_scores: bool = False, allowed=None,
                       positions: bool = False) -> List[List[Recognition]]:
        """:meth:`search_batch` on regions of BGR pages, as ``recognize_regions`` takes them: [] for a sliver."""
        return self._run_match(lambda: _Regions(list(pages_bgr), list(regions)), bias, k, length_penalty, early_stopping,
                               no_repeat_ngram, token_scores, allowed, positions, True, True)

    def recognize_page(self, page_bgr: np.ndarray, regions):
        """``_collect_manga_detections`` for one page: ``regions`` = the detector's (text, polygon) pairs."""
        from .regions import recognize_page
        return recognize_page(self, page_bgr, regions)

    def recognize_pages(self, pages_bgr, regions_per_page, on_error=None):
        """``AutoDetectorWorker.run`` (Text mode) over several pages: one job queue for all regions of all pages."""
        from .regions import recognize_pages
        return recognize_pages(self, pages_bgr, regions_per_page, on_error)

    def close(self) -> None:
        self._batcher.close()
        self.engine.close()
