"""-m gpu: jobs merged into one batch do not depend on where in it they lie.  Every job brings its own per-row arrays - sets,
n-gram sizes, prefixes, penalties, sources, automata - and the scheduler merges them in row order over the batch's rows
(csrc/engine.hip: start_batch) and hands each job its rows back (finish_batch): the same jobs submitted in another order must
get the same answers, and each of them the ids it gets alone.  That the jobs did merge is asserted: the encoder count rises by
the planes of ONE batch and an instrumented pass launches the start token's kernel once.

The float outputs (log-probabilities, alternatives' log-probabilities, positions, beam scores) of a row at another offset of
the batch: measured on the library before the scheduler's merge was rewritten, all of them came out bit-identical across the
orders below (max |difference| 0.0 in every block), so the bound is bit-identity - FLOAT_BOUND = 0 ULP."""
import functools

import numpy as np
import pytest

from gpu_util import crops, engine, report
from manga_ocr.engine import BeamConfig

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")      # before the engine's library: one HIP runtime per process, torch's

MAX_LEN = 8
SEED = 31
FLOAT_BOUND = 0.0                         # max |difference| of a float output across submission orders (see the module's text)


def _engine():
    return engine("fp32", max_batch=8)


@functools.lru_cache(maxsize=None)
def _handles():
    """a token set, a hard automaton (one accepting state, a loop on every token from 4 on) and its soft twin (weight 0.5 on
    every edge, open), as tests/test_gpu_decode_forms.py makes them"""
    eng = _engine()
    tok = np.arange(4, 6144, dtype=np.int32)
    loop = ([0, tok.size], tok, np.zeros(tok.size, np.int32), [1])
    return dict(set=eng.token_set(range(100, 3000)), hard=eng.automaton(*loop),
                soft=eng.automaton(*loop, edge_weight=np.full(tok.size, 0.5, np.float32), default_next=[0]))


def _greedy_jobs():
    """name -> (planes, rows, first plane of crops(SEED, 7), keywords, the outputs it asks for)"""
    h = _handles()
    return {
        "A": (3, 3, 0, dict(token_sets=[h["set"], 0, h["set"]], no_repeat_ngram=[2, 0, 3]), ("logp",)),
        "B": (2, 2, 3, dict(prefixes=[[10, 11], []], penalty=[1.3, 1.0]), ("logp", "alt_ids", "alt_logp")),
        "C": (2, 3, 5, dict(sources=[0, 1, 0], automata=[h["hard"], 0, h["soft"]]), ("state", "pos")),
    }


def _beam_jobs():
    h = _handles()
    return {
        "D": (2, 2, 0, dict(beam_sets=[h["set"], 0]), ("score", "logp")),
        "E": (2, 2, 2, dict(beam_automata=[h["hard"], 0]), ("score", "state")),
    }


def _buffers(rows, L, outs, K=None):
    """device output blocks of one job, filled with values no run leaves"""
    lead = (rows,) if K is None else (rows, K)
    z = lambda shape, dtype, fill: torch.full(shape, fill, dtype=dtype, device="cuda")
    b = dict(ids=z(lead + (L,), torch.int32, -7), len=z(lead, torch.int32, -7))
    shapes = dict(logp=(lead + (L,), torch.float32), alt_ids=(lead + (L, 4), torch.int32), alt_logp=(lead + (L, 4), torch.float32),
                  pos=(lead + (L, 5), torch.float32), state=(lead, torch.int32), score=(lead, torch.float32))
    for name in outs:
        b[name] = z(shapes[name][0], shapes[name][1], -7)
    return b


def _submit(eng, gray, job, beam=None):
    planes, rows, first, kw, outs = job
    L = eng.spec.max_len
    b = _buffers(rows, L, outs, beam.num_beams if beam else None)
    g = gray[first:first + planes]
    if beam is None:
        eng.recognize_device(g, planes, b["ids"], b["len"], b.get("logp"), b.get("alt_ids"), b.get("alt_logp"),
                             d_out_pos=b.get("pos"), d_out_state=b.get("state"), **kw)
    else:
        eng.recognize_device(g, planes, b["ids"], b["len"], beam=beam, d_out_score=b["score"], d_out_beam_logp=b.get("logp"),
                             d_out_beam_state=b.get("state"), **kw)
    return b


def _run(jobs, order, beam=None, planes_total=None):
    """the jobs submitted in `order` and run: name -> {output: numpy array}; with planes_total, asserts that they ran as ONE
    batch (the encoder took exactly that many crops)"""
    eng = _engine()
    gray = torch.from_numpy(crops(SEED, 7)).cuda()
    eng.set_generate_max_length(MAX_LEN)
    try:
        torch.cuda.synchronize()
        before = eng.encoded_crops()
        bufs = {name: _submit(eng, gray, jobs[name], beam) for name in order}
        eng.synchronize()
        torch.cuda.synchronize()
        if planes_total is not None:
            assert eng.encoded_crops() - before == planes_total, (order, eng.encoded_crops() - before)
    finally:
        eng.set_generate_max_length(eng.spec.max_len)
    return {name: {k: v.cpu().numpy() for k, v in b.items()} for name, b in bufs.items()}


def _launches(jobs, order, beam=None):
    """profile name -> launches of an instrumented pass of `order`"""
    eng = _engine()
    eng.profile_enable(True)
    try:
        eng.profile_reset()
        _run(jobs, order, beam)
        return {s["name"]: s["launches"] for s in eng.profile_get() if s["launches"] > 0}
    finally:
        eng.profile_enable(False)


def _compare_orders(runs, orders, what):
    """ids, lengths and states exact, the float blocks within FLOAT_BOUND (0: bit-identical) of the first order's"""
    base = runs[0]
    worst = {}
    for order, run in zip(orders[1:], runs[1:]):
        for name, blocks in run.items():
            for k, v in blocks.items():
                if v.dtype == np.int32:
                    np.testing.assert_array_equal(v, base[name][k], err_msg=f"{what}: job {name} {k}, order {order}")
                else:
                    assert np.isfinite(v).all() and np.isfinite(base[name][k]).all(), (what, name, k)
                    worst[k] = max(worst.get(k, 0.0), float(np.abs(v.astype(np.float64) - base[name][k]).max()))
    for k, d in sorted(worst.items()):
        report(f"[batch-merge] {what}: {k} max |difference| across orders {d:.3e} (bound {FLOAT_BOUND:.1e})")
    for order, run in zip(orders[1:], runs[1:]):
        for name, blocks in run.items():
            for k, v in blocks.items():
                if v.dtype != np.int32:
                    if FLOAT_BOUND == 0.0:
                        np.testing.assert_array_equal(v.view(np.uint32), base[name][k].view(np.uint32),
                                                      err_msg=f"{what}: job {name} {k} bits, order {order}")
                    else:
                        assert float(np.abs(v.astype(np.float64) - base[name][k]).max()) <= FLOAT_BOUND, (what, name, k, order)


def test_merged_greedy_jobs_do_not_depend_on_their_order():
    jobs = _greedy_jobs()
    orders = ["ABC", "CBA", "BCA"]
    runs = [_run(jobs, order, planes_total=7) for order in orders]
    for run in runs:                    # every block was written: no fill value is left in what a job asked for
        for name, blocks in run.items():
            assert (blocks["len"] >= 1).all() and (blocks["ids"] >= 0).all(), name
    _compare_orders(runs, orders, "greedy")
    ran = _launches(jobs, "ABC")
    assert ran.get("dec_token_first") == 1, ran
    assert "dec_token_topk_rp" in ran and not [n for n in ran if n.startswith("dec_token") and n not in ("dec_token_first", "dec_token_topk_rp")], ran
    for name in jobs:                   # ... and alone, each job's ids and lengths are the merged run's
        alone = _run(jobs, name, planes_total=jobs[name][0])[name]
        np.testing.assert_array_equal(alone["ids"], runs[0][name]["ids"], err_msg=f"job {name} alone")
        np.testing.assert_array_equal(alone["len"], runs[0][name]["len"], err_msg=f"job {name} alone")


def test_merged_beam_jobs_do_not_depend_on_their_order():
    jobs = _beam_jobs()
    beam = BeamConfig(2)
    orders = ["DE", "ED"]
    runs = [_run(jobs, order, beam, planes_total=4) for order in orders]
    for run in runs:
        for name, blocks in run.items():
            assert (blocks["len"][:, 0] >= 1).all(), name
    _compare_orders(runs, orders, "beam")
    ran = _launches(jobs, "DE", beam)
    assert ran.get("dec_token_first") == 1, ran
    assert "beam_select_am" in ran and not [n for n in ran if n.startswith("beam_select") and n != "beam_select_am"], ran
