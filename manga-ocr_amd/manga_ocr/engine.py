"""Python handle on the native engine (libmocr_hip.so) - thin, typed wrappers over the C ABI."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _capi
from .weights import DEFAULT_SPEC, ModelSpec, check_weights

DTYPES = {"fp32": _capi.MOCR_F32, "f32": _capi.MOCR_F32, "float32": _capi.MOCR_F32,
          "bf16": _capi.MOCR_BF16, "bfloat16": _capi.MOCR_BF16}


EARLY_STOPPING = {False: 0, True: 1, "never": 2}


class BeamConfig:
    """generate(num_beams, length_penalty, early_stopping, no_repeat_ngram_size) of a beam request (include/mocr.h, "beam
    search"): ``num_beams`` 2 .. 4, ``early_stopping`` False / True / "never", ``no_repeat_ngram`` 0 = off."""
    __slots__ = ("num_beams", "length_penalty", "early_stopping", "no_repeat_ngram")

    def __init__(self, num_beams: int = 4, length_penalty: float = 1.0, early_stopping=False, no_repeat_ngram: int = 0):
        if isinstance(num_beams, (bool, np.bool_)) or not isinstance(num_beams, (int, np.integer)):
            raise TypeError(f"num_beams: an int, instead got {num_beams!r}")
        if not 2 <= int(num_beams) <= _capi.MAX_BEAMS:
            raise ValueError(f"num_beams must be in 2 .. {_capi.MAX_BEAMS} (the engine's limit), instead got {num_beams}")
        if isinstance(early_stopping, (bool, np.bool_)):
            early_stopping = bool(early_stopping)
        elif early_stopping != "never":
            raise ValueError(f"early_stopping must be False, True or 'never', instead got {early_stopping!r}")
        if isinstance(no_repeat_ngram, (bool, np.bool_)) or not isinstance(no_repeat_ngram, (int, np.integer)) or no_repeat_ngram < 0:
            raise ValueError(f"no_repeat_ngram: an int >= 0, instead got {no_repeat_ngram!r}")
        self.num_beams, self.length_penalty = int(num_beams), float(length_penalty)
        self.early_stopping, self.no_repeat_ngram = early_stopping, int(no_repeat_ngram)

    def key(self):
        return (self.num_beams, self.length_penalty, self.early_stopping, self.no_repeat_ngram)

    def __eq__(self, other):
        return isinstance(other, BeamConfig) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return "BeamConfig(num_beams=%d, length_penalty=%r, early_stopping=%r, no_repeat_ngram=%d)" % self.key()

    def as_struct(self) -> "_capi.MocrBeamConfig":
        return _capi.MocrBeamConfig(self.num_beams, self.length_penalty, EARLY_STOPPING[self.early_stopping], self.no_repeat_ngram)


BLOCKS = ("ids", "lens", "logp", "alt_ids", "alt_logp", "pos")       # the output blocks of a greedy recognise call, in C order


def result_layout(scores: bool = False, alternatives: bool = False, positions: bool = False) -> Tuple[str, ...]:
    """The names of what a greedy recognise call returns, in order: (ids, lens[, logp[, alt_ids, alt_logp]][, pos]) - logp with
    ``scores``, logp and the pair with ``alternatives``, pos last with ``positions``.  The one place that writes the layout
    down: ``Engine._result`` packs by it, the batcher of ``manga_ocr/ocr.py`` unpacks by it."""
    names = BLOCKS[:5] if alternatives else BLOCKS[:3] if scores else BLOCKS[:2]
    return names + BLOCKS[5:] if positions else names


def _ptr(a) -> C.c_void_p:
    """numpy array (host) / torch tensor (host or device) / int address -> void*"""
    if a is None:
        return C.c_void_p(0)
    if isinstance(a, int):
        return C.c_void_p(a)
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data)
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    raise TypeError(f"cannot take the address of {type(a)}")


def device_memory(device: int = 0) -> Tuple[int, int]:
    """(free, total) bytes of HBM on a device."""
    lib = _capi.load_library()
    f, t = C.c_int64(0), C.c_int64(0)
    rc = lib.mocr_device_memory(device, C.byref(f), C.byref(t))
    if rc != _capi.MOCR_OK:
        raise _capi.MocrError(f"mocr_device_memory({device}) failed with code {rc} (is a MI355X visible to this process?)")
    return int(f.value), int(t.value)


class Engine:
    """One engine = one GPU = one HIP stream.  Thread-safe (calls are serialised natively)."""

    def __init__(self, weights: Dict[str, np.ndarray], spec: ModelSpec = DEFAULT_SPEC, *, dtype: str = "bf16",
                 device: int = 0, max_batch: int = 64, flags: int = 0, lanes: int = 1,
                 lib_path: Optional[str] = None):
        self.lib = _capi.load_library(lib_path)
        self.spec = spec
        self.dtype = dtype
        self.max_batch = int(max_batch)
        self.device = int(device)
        check_weights(weights, spec)
        cfg = _capi.MocrConfig(
            struct_size=C.sizeof(_capi.MocrConfig), device=device, dtype=DTYPES[dtype], max_batch=max_batch,
            max_len=spec.max_len, image_size=spec.image_size, patch_size=spec.patch_size, hidden=spec.hidden,
            enc_layers=spec.enc_layers, dec_layers=spec.dec_layers, heads=spec.heads, ffn=spec.ffn, vocab=spec.vocab,
            max_pos=spec.max_pos, start_id=spec.start_id, eos_id=spec.eos_id, pad_id=spec.pad_id,
            ln_eps=spec.ln_eps, flags=flags, lanes=lanes)
        h = C.c_void_p()
        rc = self.lib.mocr_create(C.byref(cfg), C.byref(h))
        if rc != _capi.MOCR_OK or not h.value:
            raise _capi.MocrError(f"mocr_create failed with code {rc} (is a MI355X visible to this process?)")
        self._h = h
        for name, arr in weights.items():
            a = np.ascontiguousarray(arr, dtype=np.float32)
            shape = (C.c_int64 * a.ndim)(*a.shape)
            self._check(self.lib.mocr_set_tensor(self._h, name.encode(), _ptr(a), shape, a.ndim))
        self._check(self.lib.mocr_commit_weights(self._h))

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc: int) -> None:
        if rc != _capi.MOCR_OK:
            msg = self.lib.mocr_last_error(self._h)
            raise _capi.MocrError(f"libmocr_hip error {rc}: {msg.decode(errors='replace') if msg else ''}")

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.mocr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return int(self.lib.mocr_stream(self._h) or 0)

    def synchronize(self) -> None:
        self._check(self.lib.mocr_synchronize(self._h))

    # ------------------------------------------------------------------ the hot path
    def recognize(self, images: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """images uint8 [n,224,224] (luminance) or [n,224,224,3] (RGB), host memory.
        Returns (ids int32 [n,max_len], lengths int32 [n])."""
        a = np.ascontiguousarray(images, dtype=np.uint8)
        if a.ndim == 3:
            n, h, w = a.shape
            ch = 1
        elif a.ndim == 4 and a.shape[3] == 3:
            n, h, w, ch = a.shape
        else:
            raise ValueError("images must be uint8 [n,h,w] or [n,h,w,3]")
        ids = np.zeros((n, self.spec.max_len), dtype=np.int32)
        lens = np.zeros(n, dtype=np.int32)
        self._check(self.lib.mocr_recognize(self._h, _ptr(a), n, h, w, w * ch, h * w * ch, ch, _ptr(ids), _ptr(lens)))
        return ids, lens

    def _image_descs(self, images, bgr: bool = False, rotate=None):
        """numpy uint8 [h,w] (L) or [h,w,3] (RGB; B,G,R order when `bgr`) arrays of any sizes -> (ctypes array of
        mocr_image, keep-alive list).  Arrays with contiguous pixels and any row stride are passed as they are
        (a crop that is a view into a page is not copied here).  ``rotate``: per image 0 / ROTATE_90_CW / ROTATE_90_CCW -
        the reference's orientation-only rotation, done by the device's resize addressing."""
        keep = []
        descs = (_capi.MocrImage * len(images))()
        for i, im in enumerate(images):
            a = im if isinstance(im, np.ndarray) and im.dtype == np.uint8 else np.ascontiguousarray(im, dtype=np.uint8)
            if a.ndim == 2:
                ch = 1
            elif a.ndim == 3 and a.shape[2] == 3:
                ch = 3
            else:
                raise ValueError("each image must be uint8 [h,w] or [h,w,3]")
            pix_ok = a.strides[1] == ch and (ch == 1 or a.strides[2] == 1) and a.strides[0] >= a.shape[1] * ch
            if not pix_ok:
                a = np.ascontiguousarray(a)
            keep.append(a)
            d = descs[i]
            d.data = a.__array_interface__["data"][0]        # (a.ctypes.data builds a ctypes object per call: 10x slower)
            d.height, d.width = a.shape[0], a.shape[1]
            d.row_stride = a.strides[0]
            d.channels = _capi.CHANNELS_BGR if (bgr and ch == 3) else ch
            d.rotate = int(rotate[i]) if rotate is not None else 0
        return descs, keep

    # ------------------------------------------------------------------ token constraints
    def token_set(self, ids) -> int:
        """A token set of this engine (include/mocr.h, "token constraints"): the handle of the set holding ``ids`` (token ids
        in [0, vocab), duplicates allowed) and EOS, which the engine adds.  Sets are immutable and live as long as the engine;
        the same content gives the same handle.  Handle 0 is the whole vocabulary."""
        a = np.ascontiguousarray(np.asarray(list(ids) if not isinstance(ids, np.ndarray) else ids).ravel(), dtype=np.int32)
        out = C.c_int32(0)
        self._check(self.lib.mocr_token_set_create(self._h, _ptr(a), int(a.size), C.byref(out)))
        return int(out.value)

    def token_set_count(self) -> int:
        """Handles in use, set 0 included."""
        return int(self.lib.mocr_token_set_count(self._h))

    @staticmethod
    def _sets(token_sets, n: int) -> np.ndarray:
        """``token_sets=``: one handle for every crop, or one handle per crop -> int32 [n]"""
        if isinstance(token_sets, (int, np.integer)):
            return np.full(n, int(token_sets), dtype=np.int32)
        a = np.ascontiguousarray(np.asarray(list(token_sets)).ravel(), dtype=np.int32)
        if a.size != n:
            raise ValueError(f"token_sets: {n} crops but {a.size} set handles")
        return a

    # ------------------------------------------------------------------ token automata
    def automaton(self, edge_begin, edge_token, edge_next, accepting, edge_weight=None, default_next=None) -> int:
        """A token automaton of this engine (include/mocr.h, "token automata") in CSR form: state s has the edges
        ``edge_begin[s] .. edge_begin[s + 1]`` of ``edge_token`` / ``edge_next``, tokens strictly ascending, state 0 the start;
        ``accepting``: one flag per state.  Returns its handle (>= 1) for ``automata=``; automata are immutable and live as
        long as the engine.  ``edge_weight`` (float32 per edge, finite) and ``default_next`` (per state: where a token without
        an edge goes, -1 = nowhere) make it a SOFT automaton ("soft token automata"); with both None the call is the one it
        always was."""
        eb = np.ascontiguousarray(np.asarray(edge_begin).ravel(), dtype=np.int32)
        et = np.ascontiguousarray(np.asarray(edge_token).ravel(), dtype=np.int32)
        en = np.ascontiguousarray(np.asarray(edge_next).ravel(), dtype=np.int32)
        acc = np.ascontiguousarray(np.asarray(accepting).ravel() != 0, dtype=np.uint8)
        if eb.size < 2 or acc.size != eb.size - 1 or et.size != en.size or (eb.size and int(eb[-1]) != et.size):
            raise ValueError("automaton: edge_begin [states + 1], accepting [states] and edge_token / edge_next [edge_begin[-1]]")
        # (without the two arrays: the struct as it was before it grew, which the library reads as a hard automaton)
        desc = _capi.MocrAutomatonDesc(C.sizeof(_capi.MocrAutomatonDesc), int(acc.size), _ptr(eb), _ptr(et), _ptr(en), _ptr(acc))
        ref = C.byref(desc)
        if edge_weight is not None or default_next is not None:
            ew = None if edge_weight is None else np.ascontiguousarray(np.asarray(edge_weight).ravel(), dtype=np.float32)
            dn = None if default_next is None else np.ascontiguousarray(np.asarray(default_next).ravel(), dtype=np.int32)
            if (ew is not None and ew.size != et.size) or (dn is not None and dn.size != acc.size):
                raise ValueError("automaton: edge_weight [edges] and default_next [states]")
            desc = _capi.MocrSoftAutomatonDesc(C.sizeof(_capi.MocrSoftAutomatonDesc), int(acc.size), _ptr(eb), _ptr(et), _ptr(en),
                                               _ptr(acc), _ptr(ew), _ptr(dn))
            ref = C.cast(C.pointer(desc), C.POINTER(_capi.MocrAutomatonDesc))
        out = C.c_int32(0)
        self._check(self.lib.mocr_automaton_create(self._h, ref, C.byref(out)))
        used = self.automaton_used()
        self._automaton_used = (used[0] + int(acc.size), used[1] + int(et.size))
        return int(out.value)

    def automaton_used(self) -> tuple:
        """(states, edges) of the automata this object has created: what is taken of the engine's tables, which all its
        automata share (``_capi.MAX_AUTOMATON_STATES`` / ``MAX_AUTOMATON_EDGES``)."""
        return getattr(self, "_automaton_used", (0, 0))

    def automaton_count(self) -> int:
        """Automata created so far."""
        return int(self.lib.mocr_automaton_count(self._h))

    def automaton_state_bytes(self) -> int:
        """Device bytes the automata hold: 0 until the first :meth:`automaton` / the first batch that brings one."""
        return int(self.lib.mocr_automaton_state_bytes(self._h))

    @staticmethod
    def _automata(automata, n: int) -> np.ndarray:
        """``automata=``: one handle for every row, or one per row (None = no automaton) -> int32 [n]"""
        if isinstance(automata, (bool, np.bool_, str)):
            raise TypeError(f"automata: a handle or a sequence of handles, instead got {automata!r}")
        if isinstance(automata, (int, np.integer)):
            return np.full(n, int(automata), dtype=np.int32)
        hs = [_capi.AUTOMATON_NONE if h is None else h for h in automata]
        if len(hs) != n:
            raise ValueError(f"automata: {n} rows but {len(hs)} handles")
        if any(isinstance(h, (bool, np.bool_)) or not isinstance(h, (int, np.integer)) for h in hs):
            raise TypeError("automata: the handles must be ints (or None)")
        return np.ascontiguousarray(np.asarray(hs, dtype=np.int64).ravel(), dtype=np.int32)

    # ------------------------------------------------------------------ no-repeat n-grams
    def _ngram(self, no_repeat_ngram, n: int) -> np.ndarray:
        """``no_repeat_ngram=``: one size for every crop, or one size per crop -> int32 [n], each in 0 .. max_len"""
        if isinstance(no_repeat_ngram, (bool, np.bool_)) or isinstance(no_repeat_ngram, str):
            raise TypeError(f"no_repeat_ngram: an int or a sequence of ints, instead got {no_repeat_ngram!r}")
        if isinstance(no_repeat_ngram, (int, np.integer)):
            a = np.full(n, int(no_repeat_ngram), dtype=np.int64)
        else:
            a = np.asarray(list(no_repeat_ngram)).ravel()
            if a.size != n:
                raise ValueError(f"no_repeat_ngram: {n} crops but {a.size} sizes")
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise TypeError("no_repeat_ngram: the sizes must be ints")
            a = a.astype(np.int64)
        if a.size and (a.min() < 0 or a.max() > self.spec.max_len):
            raise ValueError(f"no_repeat_ngram: sizes must be in 0 .. max_len ({self.spec.max_len}), 0 = off")
        return np.ascontiguousarray(a, dtype=np.int32)

    # ------------------------------------------------------------------ repetition penalty
    @staticmethod
    def _penalty(penalty, n: int) -> np.ndarray:
        """``penalty=``: one p for every row, or one per row -> float32 [n], each finite and > 0 (1 = off)"""
        if isinstance(penalty, (bool, np.bool_, str, bytes)):
            raise TypeError(f"penalty: a float or a sequence of floats, instead got {penalty!r}")
        if isinstance(penalty, (int, float, np.integer, np.floating)):
            a = np.full(n, float(penalty), dtype=np.float64)
        else:
            vals = list(penalty)
            if any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) for v in vals):
                raise TypeError("penalty: the values must be floats")
            a = np.asarray(vals, dtype=np.float64).ravel()
            if a.size != n:
                raise ValueError(f"penalty: {n} rows but {a.size} values")
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.size and not (np.isfinite(a).all() and (a > 0).all()):
            raise ValueError("penalty: a repetition penalty is finite and > 0 (1 = off)")
        return a

    # ------------------------------------------------------------------ forced prefixes
    @staticmethod
    def _prefixes(prefixes, n: int):
        """``prefixes=``: one int sequence (or None) per crop -> (tokens int32 [n, ld], lengths int32 [n], ld), one block"""
        rows = list(prefixes)
        if len(rows) != n:
            raise ValueError(f"prefixes: {n} crops but {len(rows)} prefixes")
        rows = [np.zeros(0, dtype=np.int64) if r is None else np.asarray(list(r)) for r in rows]
        for r in rows:
            if r.ndim != 1 or (r.size and not np.issubdtype(r.dtype, np.integer)):
                raise TypeError("prefixes: every prefix is a flat sequence of token ids")
        ld = max([int(r.size) for r in rows] + [1])
        block = np.zeros((n, ld), dtype=np.int32)
        for i, r in enumerate(rows):
            block[i, :r.size] = r
        return block, np.array([r.size for r in rows], dtype=np.int32), ld

    # ------------------------------------------------------------------ shared encodings
    @staticmethod
    def _sources(sources, n_images: int) -> np.ndarray:
        """``sources=``: a flat sequence of ints, one per output row - the image, region or plane the row decodes -> int32
        [rows].  Every index is in [0, n_images) and every image is named (the engine checks the same)."""
        if isinstance(sources, (str, bytes, int, np.integer, bool, np.bool_)):
            raise TypeError(f"sources: a flat sequence of ints, one per output row, instead got {sources!r}")
        a = np.asarray(list(sources))
        if a.ndim != 1 or a.size == 0 or not np.issubdtype(a.dtype, np.integer):
            raise TypeError("sources: a flat, non-empty sequence of ints, one per output row")
        if a.min() < 0 or a.max() >= n_images:
            raise ValueError(f"sources: indices must be in [0, {n_images})")
        if np.unique(a).size != n_images:
            raise ValueError("sources: every image, region or plane must be named by a row")
        return np.ascontiguousarray(a, dtype=np.int32)

    def _prefix_args(self, prefixes, n: int):
        """the (prefix, prefix_len, prefix_ld) tail of a *_prefix / *_shared call; the arrays must outlive the call"""
        if prefixes is None:
            return None, None, 0
        return self._prefixes(prefixes, n)

    def encoded_crops(self) -> int:
        """Crops the recognise calls have put through the encoder so far (include/mocr.h, "shared encodings")."""
        return int(self.lib.mocr_encoded_crops(self._h))

    def _blocks(self, n: int, scores: bool, alternatives: bool, positions: bool):
        """The output blocks of a recognise call: (ids, lens, logp, alt_ids, alt_logp, pos), None where not asked - what
        the engine is then passed as null.  The alternatives come as the engine leaves unwritten positions: -1 / 0."""
        L = self.spec.max_len
        logp = np.zeros((n, L), dtype=np.float32) if (scores or alternatives) else None
        alt_ids = np.full((n, L, _capi.ALTERNATIVES), -1, dtype=np.int32) if alternatives else None
        alt_logp = np.zeros((n, L, _capi.ALTERNATIVES), dtype=np.float32) if alternatives else None
        pos = np.zeros((n, L, _capi.POSITION_FIELDS), dtype=np.float32) if positions else None
        return np.zeros((n, L), dtype=np.int32), np.zeros(n, dtype=np.int32), logp, alt_ids, alt_logp, pos

    @staticmethod
    def _result(blocks, scores: bool, alternatives: bool, positions: bool):
        """what the caller gets back of the six blocks: the ones :func:`result_layout` names"""
        named = dict(zip(BLOCKS, blocks))
        return tuple(named[name] for name in result_layout(scores, alternatives, positions))

    # ------------------------------------------------------------------ beam search
    def _beam_blocks(self, beam, n: int, **others):
        """``beam=``: the config struct and the output blocks (ids [n,K,max_len], lens [n,K], scores [n,K]) of a beam call, which
        takes none of the per-row keywords"""
        if not isinstance(beam, BeamConfig):
            raise TypeError(f"beam: a BeamConfig, instead got {beam!r}")
        used = [k for k, v in others.items() if v is not None and v is not False]
        if used:
            raise ValueError(f"beam search does not combine with {', '.join(used)}")
        K, L = beam.num_beams, self.spec.max_len
        if n * K > self.max_batch:
            raise ValueError(f"beam search: {n} crops x {K} beams exceed max_batch ({self.max_batch})")
        return (beam.as_struct(), np.full((n, K, L), self.spec.pad_id, dtype=np.int32), np.zeros((n, K), dtype=np.int32),
                np.full((n, K), -1e9, dtype=np.float32))

    def _per_crop(self, token_sets, no_repeat_ngram, n: int):
        """(sets, ngram) int32 [n] each, None where not given (the sizes are checked first)"""
        ngram = self._ngram(no_repeat_ngram, n) if no_repeat_ngram is not None else None
        sets = self._sets(token_sets, n) if token_sets is not None else None
        return sets, ngram

    def _recognize(self, kind: str, n: int, lead, tail=(), *, beam, d_out=None, skip_empty: bool = False, beam_scores=False, beam_sets=None,
                   beam_positions=False, beam_automata=None, beam_states=False, beam_soft=False, penalty=None, **req):
        """The one request path under recognize_images / _regions / _gray / _device.  ``kind``: the source kind as the C symbols
        spell it; ``n``: its number of sources; ``lead()``: (the call's leading C arguments, sources counted last; whatever they
        point into, kept until the call returns) - built only once the call is going to be made; ``tail``: what follows the
        sources (recognize_gray's max_len).  ``req``: the method's other keywords IN ITS ORDER (the beam refusal names them so);
        a host kind's ``scores`` / ``alternatives`` / ``positions`` flags make the output blocks here, with one row per entry
        of ``sources`` when given; recognize_device brings buffers: ``d_out`` = (ids, lengths, beam scores) and the rest in
        ``req``.  ``skip_empty``: no sources, no call.
        The arguments are checked in this order: beam with anything else, ``sources``, the n-gram sizes, the sets, the
        prefixes, the automata.  The symbol is mocr_recognize_{kind}_beam, else _automaton with ``automata`` or ``states``
        (recognize_device: ``d_out_state``), else _shared with ``sources``, else _prefix with ``prefixes``, else _positions - each
        the richest of its line, every output nobody asked for passed as null.  ``states``: a host kind returns the rows' final
        automaton states int32 [rows] as the LAST element.
        ``beam_scores`` (a host kind's flag; recognize_device: its ``d_out_beam_logp`` buffer) and ``beam_sets`` belong to a beam
        call: with either in use the symbol is mocr_recognize_{kind}_beam_tokens - the beam call plus (out_logp, sets), null
        where not asked - and a host kind returns logp [n,K,max_len] behind the scores when asked.
        ``beam_positions`` (a host kind's flag; recognize_device: its ``d_out_beam_pos`` buffer) belongs to a beam call too: the
        symbol is then mocr_recognize_{kind}_beam_positions - the _beam_tokens call plus out_pos - and a host kind returns pos
        [n,K,max_len,5] as the LAST element.
        ``beam_automata`` (one automaton handle for every crop, or one per crop, None / 0 = none) and ``beam_states`` (a host kind's
        flag; recognize_device: its ``d_out_beam_state`` buffer) belong to a beam call as well: with either in use the symbol is
        mocr_recognize_{kind}_beam_automaton - the _beam_positions call plus (automata, out_state), null where not asked - and
        a host kind returns state int32 [n,K] as the LAST element, behind pos.  ``beam_soft=True`` (a beam call, too): the symbol
        is mocr_recognize_{kind}_beam_soft, the same argument list with soft handles allowed among ``beam_automata``
        (include/mocr.h, "beam search under soft token automata"); without the flag every call is the one it was.
        ``penalty`` (one repetition penalty for every row, or one per row; include/mocr.h, "repetition penalty"): the symbol is
        mocr_recognize_{kind}_penalty, the _automaton call plus the penalties; a beam call refuses it; None is every call as it
        was."""
        host = d_out is None
        if beam is not None and penalty is not None:
            raise ValueError("beam search does not combine with penalty")
        automata, states = req.pop("automata", None), req.pop("states" if host else "d_out_state", None)
        if beam is not None and (automata is not None or (states is not None and states is not False)):
            raise ValueError("beam search does not combine with automata / states")
        wants_pos = beam_positions is not None and beam_positions is not False
        tokens = (beam_scores is not None and beam_scores is not False) or beam_sets is not None
        if (tokens or wants_pos) and beam is None:
            raise ValueError("beam_scores / beam_sets / beam_positions belong to a beam call: pass beam=")
        wants_aut = beam_automata is not None or (beam_states is not None and beam_states is not False)
        if wants_aut and beam is None:
            raise ValueError("beam_automata / beam_states belong to a beam call: pass beam=")
        if beam_soft and beam is None:
            raise ValueError("beam_soft belongs to a beam call: pass beam=")
        if beam is not None:
            cfg, *out = self._beam_blocks(beam, n if host else 0, **req)
            if wants_aut or beam_soft:
                sets = self._sets(beam_sets, n) if beam_sets is not None else None
                handles = self._automata(beam_automata, n) if beam_automata is not None else None
                if host:
                    logp = np.zeros(out[0].shape, dtype=np.float32) if beam_scores else None
                    pos = np.zeros(out[0].shape + (_capi.POSITION_FIELDS,), dtype=np.float32) if wants_pos else None
                    state = np.full(out[1].shape, _capi.STATE_NONE, dtype=np.int32) if beam_states else None
                else:
                    logp, pos, state = beam_scores, (beam_positions if wants_pos else None), (beam_states if beam_states is not False else None)
                if n > 0 or not skip_empty:
                    args, keep = lead()
                    self._check(getattr(self.lib, f"mocr_recognize_{kind}_beam_{'soft' if beam_soft else 'automaton'}")(
                        self._h, *args, *tail, C.byref(cfg), *map(_ptr, out if host else d_out), _ptr(logp), _ptr(sets), _ptr(pos),
                        _ptr(handles), _ptr(state)))
                return (tuple(out) + tuple(x for x in (logp, pos, state) if x is not None)) if host else None
            if wants_pos:
                sets = self._sets(beam_sets, n) if beam_sets is not None else None
                if host:
                    logp = np.zeros(out[0].shape, dtype=np.float32) if beam_scores else None
                    pos = np.zeros(out[0].shape + (_capi.POSITION_FIELDS,), dtype=np.float32)
                else:
                    logp, pos = beam_scores, beam_positions
                if n > 0 or not skip_empty:
                    args, keep = lead()
                    self._check(getattr(self.lib, f"mocr_recognize_{kind}_beam_positions")(
                        self._h, *args, *tail, C.byref(cfg), *map(_ptr, out if host else d_out), _ptr(logp), _ptr(sets), _ptr(pos)))
                return (tuple(out) + ((logp,) if logp is not None else ()) + (pos,)) if host else None
            if not tokens:
                if n > 0 or not skip_empty:
                    args, keep = lead()
                    self._check(getattr(self.lib, f"mocr_recognize_{kind}_beam")(self._h, *args, *tail, C.byref(cfg), *map(_ptr, out if host else d_out)))
                return tuple(out) if host else None
            sets = self._sets(beam_sets, n) if beam_sets is not None else None
            if host:
                logp = np.zeros(out[0].shape, dtype=np.float32) if beam_scores else None
            else:
                logp = beam_scores
            if n > 0 or not skip_empty:
                args, keep = lead()
                self._check(getattr(self.lib, f"mocr_recognize_{kind}_beam_tokens")(self._h, *args, *tail, C.byref(cfg), *map(_ptr, out if host else d_out),
                                                                                   _ptr(logp), _ptr(sets)))
            return (tuple(out) + ((logp,) if logp is not None else ())) if host else None
        rows, shared = n, ()
        if req["sources"] is not None:
            src = self._sources(req["sources"], n)
            rows = int(src.size)
            shared = (rows, _ptr(src))
        flags = (req["scores"], req["alternatives"], req["positions"]) if host else None
        blocks = self._blocks(rows, *flags) if host else d_out[:2] + (req["d_out_logp"], req["d_out_alt_ids"], req["d_out_alt_logp"], req["d_out_pos"])
        state = (np.full(rows, _capi.STATE_NONE, dtype=np.int32) if states else None) if host else states
        if rows > 0 or not skip_empty:
            args, keep = lead()
            sets, ngram = self._per_crop(req["token_sets"], req["no_repeat_ngram"], rows)
            pre, plen, ld = self._prefix_args(req["prefixes"], rows)
            variant = "shared" if shared else "prefix" if req["prefixes"] is not None else "positions"
            forced = (_ptr(pre), _ptr(plen), ld) if variant != "positions" else ()
            if automata is not None or state is not None:      # the shared call (source null: row r reads number r) plus two
                variant, shared, forced = "automaton", shared or (rows, _ptr(None)), (_ptr(pre), _ptr(plen), ld)
                handles = self._automata(automata, rows) if automata is not None else None      # (kept until the call returns)
                forced += (_ptr(handles), _ptr(state))
            if penalty is not None:         # the automaton call (automata / out_state null where not given) plus one
                pen = self._penalty(penalty, rows)          # (kept until the call returns)
                if variant != "automaton":
                    variant, shared, forced = "automaton", shared or (rows, _ptr(None)), (_ptr(pre), _ptr(plen), ld, _ptr(None), _ptr(None))
                variant, forced = "penalty", forced + (_ptr(pen),)
            self._check(getattr(self.lib, f"mocr_recognize_{kind}_{variant}")(self._h, *args, *shared, *tail, *map(_ptr, blocks[:5]), _ptr(sets), _ptr(ngram),
                                                                            _ptr(blocks[5]), *forced))
        if not host:
            return None
        return self._result(blocks, *flags) + ((state,) if state is not None else ())

    def recognize_images(self, images, bgr: bool = False, rotate=None, *, scores: bool = False, alternatives: bool = False,
                         token_sets=None, no_repeat_ngram=None, positions: bool = False, prefixes=None, sources=None, beam=None,
                         beam_scores: bool = False, beam_sets=None, beam_positions: bool = False, automata=None, states: bool = False,
                         beam_automata=None, beam_states: bool = False, beam_soft: bool = False, penalty=None):
        """Crops of any sizes (list of uint8 [h,w] / [h,w,3] arrays; `bgr`: 3-channel crops are in OpenCV order;
        `rotate`: per crop 0 / 1 (90 degrees clockwise) / 2 (counter-clockwise), applied on the device): luminance
        conversion and the Pillow-exact BILINEAR resize to 224x224 run on the device.
        Returns (ids int32 [n,max_len], lengths int32 [n]); with ``scores=True`` (ids, lengths, logp float32 [n,max_len]):
        the log-probability of every emitted token, computed on the device (include/mocr.h, "token scores"); same ids.
        With ``alternatives=True`` (ids, lengths, logp, alt_ids int32 [n,max_len,4], alt_logp float32 [n,max_len,4]): the four
        most probable tokens of every position and their log-probabilities (include/mocr.h, "token alternatives"); same ids.
        ``token_sets``: a handle of :meth:`token_set` for every crop, or one per crop - each crop is decoded under its set
        (include/mocr.h, "token constraints"); the return value is shaped by ``scores`` / ``alternatives`` as above.
        ``no_repeat_ngram``: transformers' ``no_repeat_ngram_size`` under greedy decoding, an int for every crop or one per
        crop, 0 = off (include/mocr.h, "no-repeat n-grams"); combines with ``token_sets``.
        ``positions=True``: the return value gets one more, LAST element, pos float32 [n,max_len,5] - per token the centre
        (cx, cy), spread (sx, sy) and patch mass of the last decoder layer's cross-attention, in fractions of the 224 x 224
        plane the encoder sees (include/mocr.h, "token positions"); same ids, scores and alternatives.
        ``prefixes``: per crop a sequence of token ids (or None) the row starts with, behind the start token; the engine
        scores them and continues greedily (include/mocr.h, "forced prefixes").
        ``sources``: a flat sequence of ints, one per output ROW - row r decodes ``images[sources[r]]``, which is encoded
        once however many rows name it (include/mocr.h, "shared encodings").  The outputs then have ``len(sources)`` rows,
        and ``token_sets`` / ``no_repeat_ngram`` / ``prefixes`` are per row.
        ``beam``: a :class:`BeamConfig` - beam search instead of greedy decoding (include/mocr.h, "beam search"), with none of
        the other keywords.  Returns (ids int32 [n,K,max_len], lengths int32 [n,K], scores float32 [n,K]): every crop's K
        finished hypotheses, the best first, with their sequence scores; an empty slot has length 0 and score -1e9.
        ``beam_scores=True`` / ``beam_sets`` (only with ``beam``; include/mocr.h, "beam search with token sets and token scores"):
        ``beam_sets`` is a handle of :meth:`token_set` for every crop, or one per crop - all K beams of a crop search under it,
        a token outside scoring -inf without renormalising; ``beam_scores`` adds a LAST element logp float32 [n,K,max_len], the
        log-probability of every token of every hypothesis at the step that appended it (0 at the start token and behind the
        length).  Neither moves an id, a length or a sequence score of an unconstrained search.
        ``beam_positions=True`` (only with ``beam``; include/mocr.h, "beam search with token positions"): one more, LAST element
        pos float32 [n,K,max_len,5] - the token positions of every hypothesis, as ``positions=True`` gives them for a greedy row
        teacher-forced on the hypothesis' ids; zeros at the start token, behind the length and in empty slots.  Same ids,
        lengths, scores and token scores.
        ``automata``: a handle of :meth:`automaton` for every ROW, or one per row, None / 0 = none - the row is decoded under
        that token automaton (include/mocr.h, "token automata"); combines with everything but ``beam``.  ``states=True``: one
        more, LAST element state int32 [rows] - the state every row ended in, in its automaton's numbering; -1 without an
        automaton, -2 for a dead row.
        ``beam_automata`` / ``beam_states=True`` (only with ``beam``; include/mocr.h, "beam search under a token automaton"):
        ``beam_automata`` is a handle of :meth:`automaton` for every crop, or one per crop, None / 0 = none - all K beams of the
        crop walk it, each with its own state, so the hypotheses are the K best paths the automaton allows; ``beam_states`` adds
        a LAST element state int32 [n,K], the state behind every hypothesis' last token other than EOS (-1: no automaton, or an
        empty slot).  They combine with ``beam_scores`` / ``beam_sets`` / ``beam_positions``; ``automata`` / ``states`` stay
        refused with ``beam``.
        ``beam_soft=True`` (only with ``beam``; include/mocr.h, "beam search under soft token automata"): ``beam_automata`` may
        hold SOFT automata - their edge weights are added to the log-probabilities behind the log_softmax and enter the
        hypotheses' scores (transformers' ``generate(num_beams=K, sequence_bias=...)``).  Without it a soft handle is refused.
        ``penalty``: transformers' ``repetition_penalty`` under greedy decoding, one float for every ROW or one per row, finite
        and > 0, 1 = off (include/mocr.h, "repetition penalty"); combines with everything but ``beam``."""
        def lead():
            descs, keep = self._image_descs(images, bgr, rotate)
            return (descs, len(keep)), keep
        return self._recognize("images", len(images), lead, beam=beam, beam_scores=beam_scores, beam_sets=beam_sets, beam_positions=beam_positions, skip_empty=True, scores=scores, alternatives=alternatives, token_sets=token_sets,
                               no_repeat_ngram=no_repeat_ngram, positions=positions, prefixes=prefixes, sources=sources, automata=automata, states=states,
                               beam_automata=beam_automata, beam_states=beam_states, beam_soft=beam_soft, penalty=penalty)

    def recognize_regions(self, pages, regions, bgr: bool = True, *, scores: bool = False, alternatives: bool = False,
                          token_sets=None, no_repeat_ngram=None, positions: bool = False, prefixes=None, sources=None, beam=None,
                          beam_scores: bool = False, beam_sets=None, beam_positions: bool = False, automata=None, states: bool = False,
                         beam_automata=None, beam_states: bool = False, beam_soft: bool = False, penalty=None):
        """pages: list of uint8 [H,W,3] (or [H,W]) arrays; regions: iterable of (page_index, x, y, w, h) bounding
        rectangles.  Each page is uploaded once; the 8 %-padded, page-clipped crop of every region
        (``src/ui/main_window.py:9530-9540``) is cut on the device.  Returns (ids [n,max_len], lengths [n]);
        a region reduced to a sliver has length 0.  ``scores=True``: (ids, lengths, logp float32 [n,max_len]), a sliver's
        row all 0.  ``alternatives=True``: (ids, lengths, logp, alt_ids, alt_logp) as for recognize_images, a sliver's rows
        all -1 / 0.  ``token_sets``: a set handle for every region, or one per region (see recognize_images);
        ``no_repeat_ngram``: a no-repeat n-gram size for every region, or one per region (see recognize_images).
        ``positions=True``: one more, last element pos float32 [n,max_len,5] (see recognize_images), in fractions of the
        region's padded, clipped rectangle (manga_ocr.regions.padded_rect); a sliver's rows all 0.
        ``prefixes``: per region a forced prefix or None (see recognize_images); a sliver ignores its prefix.
        ``sources``: one region index per output ROW (see recognize_images): the outputs have ``len(sources)`` rows, the
        per-region arguments are per row, and every row of a sliver region has length 0.
        ``beam``: a :class:`BeamConfig` (see recognize_images): (ids [n,K,max_len], lengths [n,K], scores [n,K]); a sliver's K
        slots are empty.  ``beam_scores`` / ``beam_sets``: as for recognize_images, one set per region; a sliver's logp rows all 0.
        ``beam_positions``: as for recognize_images, in fractions of the region's padded, clipped rectangle; a sliver's rows all 0.
        ``automata`` / ``states``: as for recognize_images, per row; a sliver's state is -1."""
        regs = list(regions)

        def lead():
            descs, keep = self._image_descs(pages, bgr)
            arr = (_capi.MocrRegion * len(regs))()
            for i, (pg, x, y, w, h) in enumerate(regs):
                arr[i].page, arr[i].x, arr[i].y, arr[i].width, arr[i].height = int(pg), int(x), int(y), int(w), int(h)
            return (descs, len(keep), arr, len(regs)), keep
        return self._recognize("regions", len(regs), lead, beam=beam, beam_scores=beam_scores, beam_sets=beam_sets, beam_positions=beam_positions, skip_empty=True, scores=scores, alternatives=alternatives, token_sets=token_sets,
                               no_repeat_ngram=no_repeat_ngram, positions=positions, prefixes=prefixes, sources=sources, automata=automata, states=states,
                               beam_automata=beam_automata, beam_states=beam_states, beam_soft=beam_soft, penalty=penalty)

    def graph_count(self) -> int:
        return int(self.lib.mocr_graph_count(self._h))

    def ln_fold_state(self) -> Tuple[bool, float]:
        """(folds, noise_ratio): whether fat bf16 batches run with the encoder's LayerNorms folded into the GEMMs, and the
        input-rounding noise ratio commit measured on this checkpoint's residual stream (include/mocr.h)."""
        r = C.c_float(0.0)
        on = self.lib.mocr_ln_fold_state(self._h, C.byref(r))
        return bool(on), float(r.value)

    def decode_slot_steps(self) -> int:
        """Decode slots x steps enqueued so far (what the decode launches were sized for, in row-steps)."""
        return int(self.lib.mocr_decode_slot_steps(self._h))

    def beam_state_bytes(self) -> int:
        """Bytes of beam state the engine holds: 0 until its first beam batch (include/mocr.h, test hook)."""
        return int(self.lib.mocr_beam_state_bytes(self._h))

    def beam_token_state_bytes(self) -> int:
        """Bytes of the token form's beam state, which beam_state_bytes does not count: 0 until the first beam batch with token
        scores or a token set (include/mocr.h, test hook)."""
        return int(self.lib.mocr_beam_token_state_bytes(self._h))

    def beam_position_state_bytes(self) -> int:
        """Bytes of the two beam-index trails, which neither of the two above counts: 0 until the first beam batch that asks for
        token positions (include/mocr.h, test hook)."""
        return int(self.lib.mocr_beam_position_state_bytes(self._h))

    def lane_rowmap(self, n: int, lane: int = 0) -> np.ndarray:
        """The first ``n`` entries of a lane's decode slot -> row map as its last batch left it (include/mocr.h, test hook)."""
        out = np.zeros(n, dtype=np.int32)
        self._check(self.lib.mocr_lane_rowmap(self._h, int(lane), _ptr(out), int(n)))
        return out

    def compaction_count(self) -> int:
        """Row compactions performed so far: unfinished rows moved to the first decode slots between chunks of steps."""
        return int(self.lib.mocr_compaction_count(self._h))

    def preprocess(self, images, bgr: bool = False, rotate=None) -> np.ndarray:
        """Test hook: the uint8 [n,224,224] planes the encoder sees for these crops."""
        descs, keep = self._image_descs(images, bgr, rotate)
        out = np.zeros((len(keep), self.spec.image_size, self.spec.image_size), dtype=np.uint8)
        self._check(self.lib.mocr_preprocess(self._h, descs, len(keep), _ptr(out)))
        return out

    def recognize_device(self, d_gray, n: int, d_out_ids, d_out_len, d_out_logp=None, d_out_alt_ids=None, d_out_alt_logp=None, *,
                         token_sets=None, no_repeat_ngram=None, d_out_pos=None, prefixes=None, sources=None, beam=None,
                         d_out_score=None, d_out_beam_logp=None, beam_sets=None, d_out_beam_pos=None, automata=None,
                         d_out_state=None, beam_automata=None, d_out_beam_state=None, beam_soft: bool = False, penalty=None) -> None:
        """Asynchronous; all are device buffers (torch CUDA tensors or raw addresses).  ``d_out_logp`` (float32
        [n,max_len]): also the token log-probabilities.  ``d_out_alt_ids`` (int32) with ``d_out_alt_logp`` (float32), both
        [n,max_len,4]: also the token alternatives.  ``token_sets``: a set handle for every crop, or one per crop (host values).
        ``no_repeat_ngram``: a no-repeat n-gram size for every crop, or one per crop (host values).
        ``d_out_pos`` (float32 [n,max_len,5]): also the token positions.  ``prefixes``: per crop a forced prefix or None (host
        values, copied by the call).  ``sources``: one plane index per output ROW (host values, see recognize_images) -
        ``n`` then counts the planes of ``d_gray``, the output buffers have ``len(sources)`` rows and the per-crop arguments
        are per row.  ``beam`` (a :class:`BeamConfig`) with ``d_out_score``: beam search - ``d_out_ids`` int32 [n,K,max_len],
        ``d_out_len`` int32 [n,K] and ``d_out_score`` float32 [n,K] receive the hypotheses; none of the other keywords but ``d_out_beam_logp`` (float32
        [n,K,max_len]: also the hypotheses' token scores), ``beam_sets`` (host values) and ``d_out_beam_pos`` (float32 [n,K,max_len,5]: also
        the hypotheses' token positions), as for recognize_images.  ``automata`` (host values): a token automaton for every row, or
        one per row; ``d_out_state`` (int32 [rows]): also the rows' final states.  ``beam_automata`` (host values, only with ``beam``): a
        token automaton for every crop, or one per crop; ``d_out_beam_state`` (int32 [n,K]): also the hypotheses' states;
        ``beam_soft=True``: the automata may be soft (see recognize_images)."""
        self._recognize("device", n, lambda: ((_ptr(d_gray), n), None), beam=beam, beam_scores=d_out_beam_logp, beam_sets=beam_sets, beam_positions=d_out_beam_pos, d_out=(d_out_ids, d_out_len, d_out_score), d_out_logp=d_out_logp,
                        d_out_alt_ids=d_out_alt_ids, d_out_alt_logp=d_out_alt_logp, token_sets=token_sets, no_repeat_ngram=no_repeat_ngram,
                        d_out_pos=d_out_pos, prefixes=prefixes, sources=sources, automata=automata, d_out_state=d_out_state,
                        beam_automata=beam_automata, beam_states=d_out_beam_state if d_out_beam_state is not None else False,
                        beam_soft=beam_soft, penalty=penalty)

    def set_generate_max_length(self, max_len: int) -> None:
        self._check(self.lib.mocr_set_generate_max_length(self._h, int(max_len)))

    def recognize_gray(self, gray: np.ndarray, max_len: Optional[int] = None, *, scores: bool = False, alternatives: bool = False,
                       token_sets=None, no_repeat_ngram=None, positions: bool = False, prefixes=None, sources=None, beam=None,
                       beam_scores: bool = False, beam_sets=None, beam_positions: bool = False, automata=None, states: bool = False,
                         beam_automata=None, beam_states: bool = False, beam_soft: bool = False, penalty=None):
        """Luminance planes uint8 [n,224,224] (host), generate(max_length) ``max_len``; the keywords as for recognize_images
        (``sources``: one plane index per output row; ``beam``: (ids [n,K,max_len], lengths [n,K], scores [n,K]), with ``beam_scores`` also
        logp [n,K,max_len]; ``beam_sets``: one set per plane; ``beam_positions``: also pos [n,K,max_len,5], last)."""
        a = np.ascontiguousarray(gray, dtype=np.uint8)
        return self._recognize("gray_host", a.shape[0], lambda: ((_ptr(a), a.shape[0]), a), (max_len or self.spec.max_len,), beam=beam, beam_scores=beam_scores,
                               beam_sets=beam_sets, beam_positions=beam_positions, scores=scores,
                               alternatives=alternatives, token_sets=token_sets, no_repeat_ngram=no_repeat_ngram, positions=positions, prefixes=prefixes,
                               sources=sources, automata=automata, states=states,
                               beam_automata=beam_automata, beam_states=beam_states, beam_soft=beam_soft, penalty=penalty)

    # ------------------------------------------------------------------ test hooks
    def encode(self, d_gray, n: int) -> np.ndarray:
        out = np.zeros((n, self.spec.enc_tokens, self.spec.hidden), dtype=np.float32)
        self._check(self.lib.mocr_encode(self._h, _ptr(d_gray), n, _ptr(out)))
        return out

    def decode_logits(self, d_gray, n: int, forced_ids: np.ndarray) -> np.ndarray:
        f = np.ascontiguousarray(forced_ids, dtype=np.int32)
        T = f.shape[1]
        out = np.zeros((n, T, self.spec.vocab), dtype=np.float32)
        self._check(self.lib.mocr_decode_logits(self._h, _ptr(d_gray), n, _ptr(f), T, _ptr(out)))
        return out

    def op_gemm(self, dA, dW, d_bias, d_out, d_resid, M, N, K, epilogue, tile=128, split_k=1) -> None:
        self._check(self.lib.mocr_op_gemm(self._h, _ptr(dA), _ptr(dW), _ptr(d_bias), _ptr(d_out), _ptr(d_resid),
                                          M, N, K, epilogue, tile, split_k))

    def op_gemm_ln(self, dA, dW, d_bias, d_out, d_resid, M, N, K, epilogue, tile, d_part, d_csum, d_xb) -> None:
        """The persistent encoder GEMM with the LayerNorm folded in (include/mocr.h, mocr_op_gemm_ln)."""
        self._check(self.lib.mocr_op_gemm_ln(self._h, _ptr(dA), _ptr(dW), _ptr(d_bias), _ptr(d_out), _ptr(d_resid), M, N, K, epilogue, tile,
                                             _ptr(d_part), _ptr(d_csum), _ptr(d_xb)))

    def op_ln_prep(self, d_x, d_xb, d_part, M) -> None:
        self._check(self.lib.mocr_op_ln_prep(self._h, _ptr(d_x), _ptr(d_xb), _ptr(d_part), M))

    def op_layernorm(self, d_x, d_gamma, d_beta, d_out, M) -> None:
        self._check(self.lib.mocr_op_layernorm(self._h, _ptr(d_x), _ptr(d_gamma), _ptr(d_beta), _ptr(d_out), M))

    def op_enc_attention(self, d_qkv, d_ctx, n, impl) -> None:
        self._check(self.lib.mocr_op_enc_attention(self._h, _ptr(d_qkv), _ptr(d_ctx), n, impl))

    def op_embed(self, d_gray, n, tile, d_patches, d_x) -> None:
        """The encoder's front end on the caller's buffers (include/mocr.h, mocr_op_embed); tile 0 = the encoder's choice."""
        self._check(self.lib.mocr_op_embed(self._h, _ptr(d_gray), int(n), int(tile), _ptr(d_patches), _ptr(d_x)))

    def op_layernorm_slab(self, d_x, d_slabs, nslab, slab_stride, d_bias, d_gamma, d_beta, d_out, M) -> None:
        """x += bias + slabs in place, out = LayerNorm(x) (include/mocr.h, mocr_op_layernorm_slab)."""
        self._check(self.lib.mocr_op_layernorm_slab(self._h, _ptr(d_x), _ptr(d_slabs), int(nslab), int(slab_stride), _ptr(d_bias),
                                                    _ptr(d_gamma), _ptr(d_beta), _ptr(d_out), int(M)))

    ENCODER_PLAN_FIELDS = ("embed_tile", "tile_qkv", "tile_o", "tile_fc1", "tile_fc2", "split_o", "split_2", "fold", "ysplit", "attn_impl")

    def encoder_plan(self, n: int) -> dict:
        """What the encoder decides from the number of crops (include/mocr.h, mocr_encoder_plan), by name."""
        out = np.zeros(10, dtype=np.int32)
        self._check(self.lib.mocr_encoder_plan(self._h, int(n), _ptr(out)))
        return dict(zip(self.ENCODER_PLAN_FIELDS, (int(v) for v in out)))

    DECODE_PLAN_GEMMS = ("qkv", "proj", "fc1", "fc2", "vocab")
    DECODE_PLAN_FIELDS = ("path", "regime_tile", "launch_tile") + \
        tuple(f"{g}_{f}" for g in DECODE_PLAN_GEMMS for f in ("split", "ring", "epi")) + \
        ("qkv_tile_gemm", "fused_query", "query_block_rows", "qt_tile", "attn_nt", "chunk_steps", "graph_rows")
    DECODE_PATHS = ("small-batch", "classic", "latent")

    def decode_plan(self, rows: int, regime_rows: int = 0) -> dict:
        """What a greedy decode step of ``rows`` rows decides, ``regime_rows`` being the rows its batch started with (0: the
        same), by name (include/mocr.h, mocr_decode_plan); ``path`` as one of DECODE_PATHS.  Nothing is launched."""
        out = np.zeros(_capi.DECODE_PLAN_FIELDS, dtype=np.int32)
        self._check(self.lib.mocr_decode_plan(self._h, int(rows), int(regime_rows), _ptr(out)))
        pl = dict(zip(self.DECODE_PLAN_FIELDS, (int(v) for v in out)))
        pl["path"] = self.DECODE_PATHS[pl["path"]]
        return pl

    def op_gemm_args(self, **kw) -> None:
        """The 64 / 128 tile GEMM; keyword arguments are the fields of mocr_gemm_args (buffers as device tensors or addresses)."""
        self._check(self.lib.mocr_op_gemm_args(self._h, self._args(_capi.MocrGemmArgs, kw)))

    def last_tile_launch(self) -> dict:
        """The calling thread's last tile-GEMM launch (include/mocr.h, mocr_last_tile_launch)."""
        out = np.zeros(4, dtype=np.int32)
        self._check(self.lib.mocr_last_tile_launch(self._h, _ptr(out)))
        return dict(zip(("tile", "ring", "blocks", "split"), (int(v) for v in out)))

    def encoder_groups(self, n: int) -> dict:
        """N-tiles per column group of the tile order of the encoder's QKV and FC1 for n crops (include/mocr.h, mocr_encoder_groups)."""
        out = np.zeros(2, dtype=np.int32)
        self._check(self.lib.mocr_encoder_groups(self._h, int(n), _ptr(out)))
        return {"qkv": int(out[0]), "fc1": int(out[1])}

    def op_gemm_pers(self, **kw) -> None:
        """The persistent encoder GEMM as the encoder launches it; keyword arguments are the fields of mocr_gemm_pers_args
        (buffers as device tensors or addresses)."""
        self._check(self.lib.mocr_op_gemm_pers(self._h, self._args(_capi.MocrGemmPersArgs, kw)))

    def last_pers_launch(self) -> dict:
        """The calling thread's last launch of the persistent GEMM (include/mocr.h, mocr_last_pers_launch)."""
        out = np.zeros(4, dtype=np.int32)
        self._check(self.lib.mocr_last_pers_launch(self._h, _ptr(out)))
        return dict(zip(("blocks", "strips", "tiles", "group_n"), (int(v) for v in out)))

    def op_latent_attention(self, d_qt, d_x, d_out, n, length, x_batch_stride) -> None:
        self._check(self.lib.mocr_op_latent_attention(self._h, _ptr(d_qt), _ptr(d_x), _ptr(d_out), n, length, x_batch_stride))

    def op_quant_fp8(self, d_x, d_x8, n_elems: int, inv_sx: float) -> None:
        self._check(self.lib.mocr_op_quant_fp8(self._h, _ptr(d_x), _ptr(d_x8), n_elems, inv_sx))

    def op_latent_attention_fp8(self, d_qt, d_x8, d_out, n, length, x_batch_stride_bytes, sx) -> None:
        self._check(self.lib.mocr_op_latent_attention_fp8(self._h, _ptr(d_qt), _ptr(d_x8), _ptr(d_out), n, length, x_batch_stride_bytes, sx))

    def op_dec_attn(self, self_attn: bool, d_slabs, nslab, d_bias, d_k, d_v, d_ctx, n, *, layer=0, d_step=None, d_rowmap=None,
                    approx_len=0, nt=-1) -> None:
        """Classic decode attention (include/mocr.h, mocr_op_dec_attn): self (appends the new K/V to the cache) or cross."""
        self._check(self.lib.mocr_op_dec_attn(self._h, 1 if self_attn else 0, _ptr(d_slabs), nslab, _ptr(d_bias), _ptr(d_k), _ptr(d_v),
                                              layer, _ptr(d_step), _ptr(d_rowmap), _ptr(d_ctx), n, approx_len, nt))

    def op_dec_add_ln(self, d_slabs, nslab, d_bias, d_resid, d_gamma, d_beta, gelu, d_out_f32, d_out_t, rows, *, d_cache=None,
                      cache_fp8=False, inv_sx=0.0, d_step=None, d_rowmap=None) -> None:
        """Slab sum + bias [+ GELU] [+ residual] + LayerNorm, optionally writing the latent cache row."""
        self._check(self.lib.mocr_op_dec_add_ln(self._h, _ptr(d_slabs), nslab, _ptr(d_bias), _ptr(d_resid), _ptr(d_gamma), _ptr(d_beta),
                                                1 if gelu else 0, _ptr(d_out_f32), _ptr(d_out_t), rows, _ptr(d_cache),
                                                1 if cache_fp8 else 0, inv_sx, _ptr(d_step), _ptr(d_rowmap)))

    def op_dec_bias_gelu(self, d_slabs, nslab, d_bias, d_out, rows, N) -> None:
        self._check(self.lib.mocr_op_dec_bias_gelu(self._h, _ptr(d_slabs), nslab, _ptr(d_bias), _ptr(d_out), rows, N))

    @staticmethod
    def _args(struct, kw):
        """a ctypes argument struct of the C ABI (struct_size set) from keywords: buffers as device tensors or addresses"""
        a = struct()
        a.struct_size = C.sizeof(struct)
        ftypes = dict(struct._fields_)
        for name, value in kw.items():
            setattr(a, name, _ptr(value).value if ftypes[name] is C.c_void_p else value)
        return C.byref(a)

    def op_dec_token(self, **kw) -> None:
        """The token step; keyword arguments are the fields of mocr_token_args (buffers as device tensors or addresses)."""
        self._check(self.lib.mocr_op_dec_token(self._h, self._args(_capi.MocrTokenArgs, kw)))

    def op_dec_token_scored(self, d_cand_sum, d_scores, **kw) -> None:
        """The scored token step: op_dec_token plus the tiles' exp sums (candidate path) and the score rows."""
        self._check(self.lib.mocr_op_dec_token_scored(self._h, self._args(_capi.MocrTokenArgs, kw), _ptr(d_cand_sum), _ptr(d_scores)))

    def op_dec_token_topk(self, d_cand_sum, d_scores, d_top_val, d_top_idx, d_alt_ids, d_alt_logp, **kw) -> None:
        """The token step with alternatives: op_dec_token_scored plus the tiles' four best (candidate path) and the
        alternatives rows."""
        self._check(self.lib.mocr_op_dec_token_topk(self._h, self._args(_capi.MocrTokenArgs, kw), _ptr(d_cand_sum), _ptr(d_scores),
                                                    _ptr(d_top_val), _ptr(d_top_idx), _ptr(d_alt_ids), _ptr(d_alt_logp)))

    def op_dec_token_masked(self, d_cand_sum, d_scores, d_top_val, d_top_idx, d_alt_ids, d_alt_logp, d_tok_mask, d_set_of_row, **kw) -> None:
        """The token step under token sets: op_dec_token_topk (outputs nullable from the right) plus the set table and the
        set of every row."""
        self._check(self.lib.mocr_op_dec_token_masked(self._h, self._args(_capi.MocrTokenArgs, kw), _ptr(d_cand_sum), _ptr(d_scores),
                                                      _ptr(d_top_val), _ptr(d_top_idx), _ptr(d_alt_ids), _ptr(d_alt_logp), _ptr(d_tok_mask),
                                                      _ptr(d_set_of_row)))

    def op_dec_token_ngram(self, d_cand_sum, d_scores, d_top_val, d_top_idx, d_alt_ids, d_alt_logp, d_tok_mask, d_set_of_row,
                           d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row, **kw) -> None:
        """The token step with no-repeat n-grams: op_dec_token_masked plus the per-row masks (in / out), the base sets and the
        rows' sizes; the engine passes d_tok_mask = d_row_mask and d_set_of_row = 0, 1, 2, ..."""
        self._check(self.lib.mocr_op_dec_token_ngram(self._h, self._args(_capi.MocrTokenArgs, kw), _ptr(d_cand_sum), _ptr(d_scores),
                                                     _ptr(d_top_val), _ptr(d_top_idx), _ptr(d_alt_ids), _ptr(d_alt_logp), _ptr(d_tok_mask),
                                                     _ptr(d_set_of_row), _ptr(d_row_mask), _ptr(d_base_mask), _ptr(d_base_set_of_row),
                                                     _ptr(d_ngram_of_row)))

    def op_dec_token_prefix(self, d_cand_sum, d_scores, d_top_val, d_top_idx, d_alt_ids, d_alt_logp, d_tok_mask, d_set_of_row,
                            d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row, d_prefix, d_prefix_len, prefix_ld, d_tgt_val,
                            **kw) -> None:
        """The token step with forced prefixes: op_dec_token_ngram plus the rows' prefixes and lengths and, on the candidate
        path, the LM head's target values (op_gemm_argmax_target)."""
        self._check(self.lib.mocr_op_dec_token_prefix(self._h, self._args(_capi.MocrTokenArgs, kw), _ptr(d_cand_sum), _ptr(d_scores),
                                                      _ptr(d_top_val), _ptr(d_top_idx), _ptr(d_alt_ids), _ptr(d_alt_logp), _ptr(d_tok_mask),
                                                      _ptr(d_set_of_row), _ptr(d_row_mask), _ptr(d_base_mask), _ptr(d_base_set_of_row),
                                                      _ptr(d_ngram_of_row), _ptr(d_prefix), _ptr(d_prefix_len), int(prefix_ld),
                                                      _ptr(d_tgt_val)))

    def op_beam_select(self, beam: BeamConfig, d_beam_score, d_parent, d_hyp_ids, d_hyp_len, d_hyp_score, d_heuristic_open, **kw) -> None:
        """The selection that ends a beam step (include/mocr.h mocr_op_beam_select); keywords: the fields of mocr_token_args."""
        cfg = beam.as_struct()
        self._check(self.lib.mocr_op_beam_select(self._h, self._args(_capi.MocrTokenArgs, kw), C.byref(cfg), _ptr(d_beam_score),
                                                 _ptr(d_parent), _ptr(d_hyp_ids), _ptr(d_hyp_len), _ptr(d_hyp_score), _ptr(d_heuristic_open)))

    def op_beam_select_tokens(self, beam: BeamConfig, d_beam_score, d_parent, d_hyp_ids, d_hyp_len, d_hyp_score, d_heuristic_open,
                              d_beam_logp=None, d_hyp_logp=None, d_tok_mask=None, d_set_of_row=None, **kw) -> None:
        """The selection in its token form (include/mocr.h mocr_op_beam_select_tokens); keywords: the fields of mocr_token_args."""
        cfg = beam.as_struct()
        self._check(self.lib.mocr_op_beam_select_tokens(self._h, self._args(_capi.MocrTokenArgs, kw), C.byref(cfg), _ptr(d_beam_score),
                                                        _ptr(d_parent), _ptr(d_hyp_ids), _ptr(d_hyp_len), _ptr(d_hyp_score),
                                                        _ptr(d_heuristic_open), _ptr(d_beam_logp), _ptr(d_hyp_logp), _ptr(d_tok_mask),
                                                        _ptr(d_set_of_row)))

    def op_beam_select_positions(self, beam: BeamConfig, d_beam_score, d_parent, d_hyp_ids, d_hyp_len, d_hyp_score, d_heuristic_open,
                                 d_beam_logp=None, d_hyp_logp=None, d_tok_mask=None, d_set_of_row=None, d_beam_trail=None,
                                 d_hyp_trail=None, **kw) -> None:
        """The selection in its trail form (include/mocr.h mocr_op_beam_select_positions); keywords: the fields of mocr_token_args."""
        cfg = beam.as_struct()
        self._check(self.lib.mocr_op_beam_select_positions(self._h, self._args(_capi.MocrTokenArgs, kw), C.byref(cfg), _ptr(d_beam_score),
                                                           _ptr(d_parent), _ptr(d_hyp_ids), _ptr(d_hyp_len), _ptr(d_hyp_score),
                                                           _ptr(d_heuristic_open), _ptr(d_beam_logp), _ptr(d_hyp_logp), _ptr(d_tok_mask),
                                                           _ptr(d_set_of_row), _ptr(d_beam_trail), _ptr(d_hyp_trail)))

    def op_beam_select_automaton(self, beam: BeamConfig, d_beam_score, d_parent, d_hyp_ids, d_hyp_len, d_hyp_score, d_heuristic_open,
                                 d_beam_logp=None, d_hyp_logp=None, d_tok_mask=None, d_set_of_row=None, d_beam_trail=None,
                                 d_hyp_trail=None, d_edge_begin=None, d_edge_token=None, d_edge_next=None, d_accepting=None,
                                 d_aut_base_of_row=None, d_aut_state=None, d_hyp_state=None, **kw) -> None:
        """The selection in its automaton form (include/mocr.h mocr_op_beam_select_automaton): op_beam_select_positions plus the
        tables (global state numbers), the rows' start states (-1: none), the beams' states and the hypotheses' states, both
        in / out; keywords: the fields of mocr_token_args."""
        cfg = beam.as_struct()
        self._check(self.lib.mocr_op_beam_select_automaton(
            self._h, self._args(_capi.MocrTokenArgs, kw), C.byref(cfg), _ptr(d_beam_score), _ptr(d_parent), _ptr(d_hyp_ids),
            _ptr(d_hyp_len), _ptr(d_hyp_score), _ptr(d_heuristic_open), _ptr(d_beam_logp), _ptr(d_hyp_logp), _ptr(d_tok_mask),
            _ptr(d_set_of_row), _ptr(d_beam_trail), _ptr(d_hyp_trail), _ptr(d_edge_begin), _ptr(d_edge_token), _ptr(d_edge_next),
            _ptr(d_accepting), _ptr(d_aut_base_of_row), _ptr(d_aut_state), _ptr(d_hyp_state)))

    def op_beam_select_soft(self, beam: BeamConfig, d_beam_score, d_parent, d_hyp_ids, d_hyp_len, d_hyp_score, d_heuristic_open,
                            d_beam_logp=None, d_hyp_logp=None, d_tok_mask=None, d_set_of_row=None, d_beam_trail=None,
                            d_hyp_trail=None, d_edge_begin=None, d_edge_token=None, d_edge_next=None, d_accepting=None,
                            d_aut_base_of_row=None, d_aut_state=None, d_hyp_state=None, d_edge_weight=None, d_default_next=None,
                            **kw) -> None:
        """The selection in its SOFT form (include/mocr.h mocr_op_beam_select_soft): op_beam_select_automaton plus the edges'
        weights float32 [edges] and the states' default edges int32 [states] (global numbers, -1: closed), both or neither;
        keywords: the fields of mocr_token_args."""
        cfg = beam.as_struct()
        self._check(self.lib.mocr_op_beam_select_soft(
            self._h, self._args(_capi.MocrTokenArgs, kw), C.byref(cfg), _ptr(d_beam_score), _ptr(d_parent), _ptr(d_hyp_ids),
            _ptr(d_hyp_len), _ptr(d_hyp_score), _ptr(d_heuristic_open), _ptr(d_beam_logp), _ptr(d_hyp_logp), _ptr(d_tok_mask),
            _ptr(d_set_of_row), _ptr(d_beam_trail), _ptr(d_hyp_trail), _ptr(d_edge_begin), _ptr(d_edge_token), _ptr(d_edge_next),
            _ptr(d_accepting), _ptr(d_aut_base_of_row), _ptr(d_aut_state), _ptr(d_hyp_state), _ptr(d_edge_weight), _ptr(d_default_next)))

    def op_beam_permute(self, d_cache, layers: int, layer_stride: int, row_stride: int, segs: int, seg_stride: int, pos_bytes: int,
                        K: int, d_parent, d_rowmap, d_finished, d_step, n_slots: int, max_pos: int) -> None:
        """The cache reorder behind the selection on a device buffer (include/mocr.h mocr_op_beam_permute); strides in bytes."""
        self._check(self.lib.mocr_op_beam_permute(self._h, _ptr(d_cache), int(layers), int(layer_stride), int(row_stride), int(segs),
                                                  int(seg_stride), int(pos_bytes), int(K), _ptr(d_parent), _ptr(d_rowmap),
                                                  _ptr(d_finished), _ptr(d_step), int(n_slots), int(max_pos)))

    def op_attn_positions(self, d_q, d_k, d_len, rows: int, T: int, d_out_pos, d_out_map=None) -> None:
        """The positions kernel on device buffers (include/mocr.h mocr_op_attn_positions)."""
        self._check(self.lib.mocr_op_attn_positions(self._h, _ptr(d_q), _ptr(d_k), _ptr(d_len), int(rows), int(T), _ptr(d_out_pos),
                                                    _ptr(d_out_map)))

    def op_attn_positions_gathered(self, d_q, d_k, d_len, rows: int, T: int, d_out_pos, d_out_map=None, d_trail=None, trail_ld: int = 0,
                                   K: int = 0) -> None:
        """The positions kernel in its gathered-query form (include/mocr.h mocr_op_attn_positions_gathered)."""
        self._check(self.lib.mocr_op_attn_positions_gathered(self._h, _ptr(d_q), _ptr(d_k), _ptr(d_len), int(rows), int(T), _ptr(d_out_pos),
                                                             _ptr(d_out_map), _ptr(d_trail), int(trail_ld), int(K)))

    def op_enc_expand(self, d_enc, d_src_of_row, n_src: int, n_rows: int) -> None:
        """The expansion of shared encodings on a device buffer (include/mocr.h mocr_op_enc_expand)."""
        self._check(self.lib.mocr_op_enc_expand(self._h, _ptr(d_enc), _ptr(d_src_of_row), int(n_src), int(n_rows)))

    def op_dec_token_automaton(self, d_cand_sum, d_scores, d_top_val, d_top_idx, d_alt_ids, d_alt_logp, d_tok_mask, d_set_of_row,
                               d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row, d_prefix, d_prefix_len, prefix_ld, d_tgt_val,
                               d_edge_begin, d_edge_token, d_edge_next, d_accepting, d_aut_base_of_row, d_aut_state, **kw) -> None:
        """The token step with token automata: op_dec_token_prefix plus the tables (global state numbers), the rows' start
        states (-1: none) and the rows' current states, which the step walks (include/mocr.h)."""
        self._check(self.lib.mocr_op_dec_token_automaton(
            self._h, self._args(_capi.MocrTokenArgs, kw), _ptr(d_cand_sum), _ptr(d_scores), _ptr(d_top_val), _ptr(d_top_idx),
            _ptr(d_alt_ids), _ptr(d_alt_logp), _ptr(d_tok_mask), _ptr(d_set_of_row), _ptr(d_row_mask), _ptr(d_base_mask),
            _ptr(d_base_set_of_row), _ptr(d_ngram_of_row), _ptr(d_prefix), _ptr(d_prefix_len), int(prefix_ld), _ptr(d_tgt_val),
            _ptr(d_edge_begin), _ptr(d_edge_token), _ptr(d_edge_next), _ptr(d_accepting), _ptr(d_aut_base_of_row), _ptr(d_aut_state)))

    def op_automaton_init(self, d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row, rows: int, d_edge_begin, d_edge_token,
                          d_accepting, d_aut_base_of_row, d_aut_state) -> None:
        """The start of a batch with token automata on the caller's buffers (include/mocr.h: mocr_op_automaton_init)."""
        self._check(self.lib.mocr_op_automaton_init(self._h, _ptr(d_row_mask), _ptr(d_base_mask), _ptr(d_base_set_of_row),
                                                    _ptr(d_ngram_of_row), int(rows), _ptr(d_edge_begin), _ptr(d_edge_token),
                                                    _ptr(d_accepting), _ptr(d_aut_base_of_row), _ptr(d_aut_state)))

    def op_dec_token_soft(self, d_cand_sum, d_scores, d_top_val, d_top_idx, d_alt_ids, d_alt_logp, d_tok_mask, d_set_of_row,
                          d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row, d_prefix, d_prefix_len, prefix_ld, d_tgt_val,
                          d_edge_begin, d_edge_token, d_edge_next, d_accepting, d_aut_base_of_row, d_aut_state, d_edge_weight,
                          d_default_next, **kw) -> None:
        """The token step with soft token automata: op_dec_token_automaton plus the edges' weights and the states' default
        edges (include/mocr.h mocr_op_dec_token_soft); both None is that call."""
        self._check(self.lib.mocr_op_dec_token_soft(
            self._h, self._args(_capi.MocrTokenArgs, kw), _ptr(d_cand_sum), _ptr(d_scores), _ptr(d_top_val), _ptr(d_top_idx),
            _ptr(d_alt_ids), _ptr(d_alt_logp), _ptr(d_tok_mask), _ptr(d_set_of_row), _ptr(d_row_mask), _ptr(d_base_mask),
            _ptr(d_base_set_of_row), _ptr(d_ngram_of_row), _ptr(d_prefix), _ptr(d_prefix_len), int(prefix_ld), _ptr(d_tgt_val),
            _ptr(d_edge_begin), _ptr(d_edge_token), _ptr(d_edge_next), _ptr(d_accepting), _ptr(d_aut_base_of_row), _ptr(d_aut_state),
            _ptr(d_edge_weight), _ptr(d_default_next)))

    def op_automaton_init_soft(self, d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row, rows: int, d_edge_begin, d_edge_token,
                               d_accepting, d_aut_base_of_row, d_aut_state, d_default_next) -> None:
        """The start of a batch with soft token automata (include/mocr.h: mocr_op_automaton_init_soft); d_default_next None is
        op_automaton_init."""
        self._check(self.lib.mocr_op_automaton_init_soft(self._h, _ptr(d_row_mask), _ptr(d_base_mask), _ptr(d_base_set_of_row),
                                                         _ptr(d_ngram_of_row), int(rows), _ptr(d_edge_begin), _ptr(d_edge_token),
                                                         _ptr(d_accepting), _ptr(d_aut_base_of_row), _ptr(d_aut_state),
                                                         _ptr(d_default_next)))

    def op_gemm_argmax_soft(self, dA, dW, d_bias, d_cand_val, d_cand_idx, d_cand_sum, d_top_val, d_top_idx, M, N, K, tile,
                            d_tok_mask, d_set_of_row, d_rowmap, d_prefix, d_prefix_len, prefix_ld, d_step, d_tgt_val,
                            d_aut_state=None, d_edge_begin=None, d_edge_token=None, d_edge_weight=None) -> None:
        """The masked LM head with the rows' automaton edge weights added (include/mocr.h mocr_op_gemm_argmax_soft); the four
        last arguments all None is op_gemm_argmax_target."""
        soft = None
        if not (d_aut_state is None and d_edge_begin is None and d_edge_token is None and d_edge_weight is None):
            soft = self._args(_capi.MocrSoftTables, dict(d_aut_state=d_aut_state, d_edge_begin=d_edge_begin, d_edge_token=d_edge_token,
                                                          d_edge_weight=d_edge_weight))
        self._check(self.lib.mocr_op_gemm_argmax_soft(self._h, _ptr(dA), _ptr(dW), _ptr(d_bias), _ptr(d_cand_val), _ptr(d_cand_idx),
                                                      _ptr(d_cand_sum), _ptr(d_top_val), _ptr(d_top_idx), M, N, K, tile,
                                                      _ptr(d_tok_mask), _ptr(d_set_of_row), _ptr(d_rowmap), _ptr(d_prefix),
                                                      _ptr(d_prefix_len), int(prefix_ld), _ptr(d_step), _ptr(d_tgt_val), soft))

    def op_dec_token_penalty(self, d_cand_sum, d_scores, d_top_val, d_top_idx, d_alt_ids, d_alt_logp, d_tok_mask, d_set_of_row,
                             d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row, d_prefix, d_prefix_len, prefix_ld, d_tgt_val,
                             d_edge_begin, d_edge_token, d_edge_next, d_accepting, d_aut_base_of_row, d_aut_state, d_edge_weight,
                             d_default_next, d_seen_mask, d_penalty_of_row, **kw) -> None:
        """The token step with a repetition penalty: op_dec_token_soft plus the rows' seen words and penalties (include/mocr.h
        mocr_op_dec_token_penalty); both None is that call, and the automaton arrays may all be None beside them."""
        self._check(self.lib.mocr_op_dec_token_penalty(
            self._h, self._args(_capi.MocrTokenArgs, kw), _ptr(d_cand_sum), _ptr(d_scores), _ptr(d_top_val), _ptr(d_top_idx),
            _ptr(d_alt_ids), _ptr(d_alt_logp), _ptr(d_tok_mask), _ptr(d_set_of_row), _ptr(d_row_mask), _ptr(d_base_mask),
            _ptr(d_base_set_of_row), _ptr(d_ngram_of_row), _ptr(d_prefix), _ptr(d_prefix_len), int(prefix_ld), _ptr(d_tgt_val),
            _ptr(d_edge_begin), _ptr(d_edge_token), _ptr(d_edge_next), _ptr(d_accepting), _ptr(d_aut_base_of_row), _ptr(d_aut_state),
            _ptr(d_edge_weight), _ptr(d_default_next), _ptr(d_seen_mask), _ptr(d_penalty_of_row)))

    def op_penalty_init(self, d_seen_mask, rows: int) -> None:
        """Start of a batch with a repetition penalty: every row's seen words = the start token's bit alone."""
        self._check(self.lib.mocr_op_penalty_init(self._h, _ptr(d_seen_mask), int(rows)))

    def op_gemm_argmax_penalty(self, dA, dW, d_bias, d_cand_val, d_cand_idx, d_cand_sum, d_top_val, d_top_idx, M, N, K, tile,
                               d_tok_mask, d_set_of_row, d_rowmap, d_prefix, d_prefix_len, prefix_ld, d_step, d_tgt_val,
                               d_aut_state=None, d_edge_begin=None, d_edge_token=None, d_edge_weight=None, d_seen_mask=None,
                               d_penalty_of_row=None) -> None:
        """The masked LM head with a repetition penalty (include/mocr.h mocr_op_gemm_argmax_penalty): op_gemm_argmax_soft plus
        the rows' seen words and penalties; the four soft arguments all None is a penalty without any automaton."""
        soft = None
        if not (d_aut_state is None and d_edge_begin is None and d_edge_token is None and d_edge_weight is None):
            soft = self._args(_capi.MocrSoftTables, dict(d_aut_state=d_aut_state, d_edge_begin=d_edge_begin, d_edge_token=d_edge_token,
                                                          d_edge_weight=d_edge_weight))
        self._check(self.lib.mocr_op_gemm_argmax_penalty(self._h, _ptr(dA), _ptr(dW), _ptr(d_bias), _ptr(d_cand_val), _ptr(d_cand_idx),
                                                         _ptr(d_cand_sum), _ptr(d_top_val), _ptr(d_top_idx), M, N, K, tile,
                                                         _ptr(d_tok_mask), _ptr(d_set_of_row), _ptr(d_rowmap), _ptr(d_prefix),
                                                         _ptr(d_prefix_len), int(prefix_ld), _ptr(d_step), _ptr(d_tgt_val), soft,
                                                         _ptr(d_seen_mask), _ptr(d_penalty_of_row)))

    def op_ngram_init(self, d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row, rows: int) -> None:
        """Start of a batch with no-repeat n-grams: every row's mask = its base set (n = 1: minus the start token)."""
        self._check(self.lib.mocr_op_ngram_init(self._h, _ptr(d_row_mask), _ptr(d_base_mask), _ptr(d_base_set_of_row),
                                                _ptr(d_ngram_of_row), int(rows)))

    def op_gemm_argmax_masked(self, dA, dW, d_bias, d_cand_val, d_cand_idx, d_cand_sum, d_top_val, d_top_idx, M, N, K, tile,
                              d_tok_mask, d_set_of_row, d_rowmap=None) -> None:
        self._check(self.lib.mocr_op_gemm_argmax_masked(self._h, _ptr(dA), _ptr(dW), _ptr(d_bias), _ptr(d_cand_val), _ptr(d_cand_idx),
                                                        _ptr(d_cand_sum), _ptr(d_top_val), _ptr(d_top_idx), M, N, K, tile,
                                                        _ptr(d_tok_mask), _ptr(d_set_of_row), _ptr(d_rowmap)))

    def op_gemm_argmax_target(self, dA, dW, d_bias, d_cand_val, d_cand_idx, d_cand_sum, d_top_val, d_top_idx, M, N, K, tile,
                              d_tok_mask, d_set_of_row, d_rowmap, d_prefix, d_prefix_len, prefix_ld, d_step, d_tgt_val) -> None:
        """The masked, scored LM head plus the target column of every row with a forced step (include/mocr.h)."""
        self._check(self.lib.mocr_op_gemm_argmax_target(self._h, _ptr(dA), _ptr(dW), _ptr(d_bias), _ptr(d_cand_val), _ptr(d_cand_idx),
                                                        _ptr(d_cand_sum), _ptr(d_top_val), _ptr(d_top_idx), M, N, K, tile,
                                                        _ptr(d_tok_mask), _ptr(d_set_of_row), _ptr(d_rowmap), _ptr(d_prefix),
                                                        _ptr(d_prefix_len), int(prefix_ld), _ptr(d_step), _ptr(d_tgt_val)))

    def op_gemm_topk(self, dA, dW, d_bias, d_cand_val, d_cand_idx, d_cand_sum, d_top_val, d_top_idx, M, N, K, tile) -> None:
        self._check(self.lib.mocr_op_gemm_topk(self._h, _ptr(dA), _ptr(dW), _ptr(d_bias), _ptr(d_cand_val), _ptr(d_cand_idx),
                                               _ptr(d_cand_sum), _ptr(d_top_val), _ptr(d_top_idx), M, N, K, tile))

    def op_gemm_argmax_lse(self, dA, dW, d_bias, d_cand_val, d_cand_idx, d_cand_sum, M, N, K, tile) -> None:
        self._check(self.lib.mocr_op_gemm_argmax_lse(self._h, _ptr(dA), _ptr(dW), _ptr(d_bias), _ptr(d_cand_val), _ptr(d_cand_idx),
                                                     _ptr(d_cand_sum), M, N, K, tile))

    def op_gemm_argmax(self, dA, dW, d_bias, d_cand_val, d_cand_idx, M, N, K, tile) -> None:
        self._check(self.lib.mocr_op_gemm_argmax(self._h, _ptr(dA), _ptr(dW), _ptr(d_bias), _ptr(d_cand_val), _ptr(d_cand_idx),
                                                 M, N, K, tile))

    def op_smallm_gemm(self, **kw) -> None:
        """The small-batch projection; keyword arguments are the fields of mocr_smallm_args."""
        self._check(self.lib.mocr_op_smallm_gemm(self._h, self._args(_capi.MocrSmallmArgs, kw)))

    def op_latent_block(self, /, **kw) -> None:
        """The latent attention block (q -> Qt -> latent attention -> ctx); keyword arguments are the fields of
        mocr_latent_args (`self` among them: the engine is positional-only)."""
        self._check(self.lib.mocr_op_latent_block(self._h, self._args(_capi.MocrLatentArgs, kw)))

    # ------------------------------------------------------------------ per-kernel timing
    def op_qqt(self, d_x, d_wq, d_bq, d_wkT, d_qt, n: int) -> None:
        self._check(self.lib.mocr_op_qqt(self._h, _ptr(d_x), _ptr(d_wq), _ptr(d_bq), _ptr(d_wkT), _ptr(d_qt), n))

    def profile_enable(self, on: bool = True) -> None:
        self._check(self.lib.mocr_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self) -> None:
        self._check(self.lib.mocr_profile_reset(self._h))

    def profile_get(self) -> List[dict]:
        cap = 64
        arr = (_capi.MocrKernelStat * cap)()
        n = C.c_int32(0)
        self._check(self.lib.mocr_profile_get(self._h, arr, cap, C.byref(n)))
        return [dict(name=arr[i].name.decode(), launches=int(arr[i].launches), total_ms=float(arr[i].total_ms),
                     flops=float(arr[i].flops), bytes=float(arr[i].bytes)) for i in range(n.value)]
