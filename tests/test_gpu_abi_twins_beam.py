"""GPU: the four exported mocr_recognize_*_beam symbols, called through the library directly: the four source kinds give the
same hypotheses for the same crops - planes on the device, planes on the host, 224 x 224 luminance images (the device's
resize is the identity on them) and whole-page regions of grey BGR pages (the padded rectangle is clipped to the page,
equal channels keep their value as luminance) - and keep the argument checks, which come before any work."""
import ctypes as C
import functools

import numpy as np
import pytest

from gpu_util import crops, weights
from manga_ocr import _capi
from manga_ocr.engine import BeamConfig, _ptr
from manga_ocr.weights import DEFAULT_SPEC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")      # before the engine's library: one HIP runtime per process, torch's

N, T, K, L = 3, 8, 3, DEFAULT_SPEC.max_len
KINDS = ["device", "gray_host", "images", "regions"]
ERR_ARG = -1


@functools.lru_cache(maxsize=None)
def _engine():
    from manga_ocr.engine import Engine
    eng = Engine(weights(1, 1.7), DEFAULT_SPEC, dtype="fp32", device=0, max_batch=12, lanes=1)
    eng.set_generate_max_length(T)
    return eng


def _call(kind, cfg, n=N):
    eng = _engine()
    gray = crops(515, N)
    dev = kind == "device"

    def block(shape, dtype, fill):
        return torch.full(shape, fill, dtype=getattr(torch, dtype), device="cuda") if dev else np.full(shape, fill, dtype=dtype)

    outs = [block((N, K, L), "int32", -7), block((N, K), "int32", -7), block((N, K), "float32", 5.0)]
    tail = [C.byref(cfg) if cfg is not None else None] + [_ptr(o) for o in outs]
    fn = getattr(eng.lib, f"mocr_recognize_{kind}_beam")
    if dev:
        d_gray = torch.from_numpy(gray).cuda()
        rc = fn(eng._h, _ptr(d_gray), n, *tail)
        eng.synchronize()
    elif kind == "gray_host":
        rc = fn(eng._h, _ptr(gray), n, T, *tail)
    elif kind == "images":
        descs, keep = eng._image_descs(list(gray))
        rc = fn(eng._h, descs, n, *tail)
    else:
        pages = [np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2)) for g in gray]
        descs, keep = eng._image_descs(pages, True)
        arr = (_capi.MocrRegion * N)()
        for i in range(N):
            arr[i].page, arr[i].x, arr[i].y, arr[i].width, arr[i].height = i, 0, 0, 224, 224
        rc = fn(eng._h, descs, N, arr, n, *tail)
    return rc, [o.cpu().numpy() if dev else o for o in outs]


def test_the_four_source_kinds_give_the_same_hypotheses():
    cfg = BeamConfig(K, 2.0, True, 3).as_struct()
    first = None
    for kind in KINDS:
        rc, out = _call(kind, cfg)
        assert rc == _capi.MOCR_OK, kind
        ids, lens, scores = out
        assert (lens[:, 0] >= 2).all() and (ids != -7).all() and (scores < 0).all(), kind
        if first is None:
            first = out
        for a, b in zip(out, first):
            assert a.tobytes() == b.tobytes(), f"{kind} differs from {KINDS[0]}"


@pytest.mark.parametrize("kind", KINDS)
def test_the_beam_symbols_check_their_arguments_first(kind):
    eng = _engine()
    for bad in tuple(_capi.MocrBeamConfig(k, 1.0, 0, 0) for k in (0, 1, 5)) + \
            (_capi.MocrBeamConfig(2, 1.0, 3, 0), _capi.MocrBeamConfig(2, 1.0, 0, -1), None):
        rc, out = _call(kind, bad)
        assert rc == ERR_ARG
        assert (out[0] == -7).all() and (out[2] == 5.0).all(), "nothing was written"
    rc, _ = _call(kind, _capi.MocrBeamConfig(4, 1.0, 0, 0), n=4)       # 4 crops x 4 beams > max_batch 12
    assert rc == ERR_ARG
    assert b"max_batch" in eng.lib.mocr_last_error(eng._h)
