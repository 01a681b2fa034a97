"""Host-side checks of lookup decoding for sampled rows (no GPU): the library exports the three
new symbols, the ctypes bindings match include/llmi.h, the Python signatures are the documented ones (and
Model.batch_generate_lookup's is unchanged), the samplers are marshalled as batch_generate marshals them, and the rule
itself -- ref_accept_sampled below: section 15's ref_accept fed with the span rows' seeded draws -- behaves as stated
on synthetic logits."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from test_batch_lookup_host import declared, ref_accept, simulate  # noqa: E402
from test_sampling import ref_sample  # noqa: E402


# ---------------------------------------------------------------------------
# the rule (include/llmi.h)
# ---------------------------------------------------------------------------
def drawn_ids(logits_rows, sampler, pos):
    """a[j] of a span whose row j ran at position pos + j: the seeded draw from that row's logits with the row's
    sampler at the token row's own position; sampler None (a greedy row): the first-index arg-max."""
    if sampler is None:
        return [int(np.argmax(l)) for l in logits_rows]
    return [ref_sample(l, sampler["temperature"], sampler.get("top_k", 0), sampler.get("top_p", 1.0),
                       sampler.get("seed", 0), pos + j) for j, l in enumerate(logits_rows)]


def ref_accept_sampled(draft, logits_rows, sampler, pos, stop, remaining):
    """The ids a step emits for a sampled row: ref_accept with a = the span rows' drawn ids."""
    assert len(logits_rows) == len(draft) + 1
    return ref_accept(draft, drawn_ids(logits_rows, sampler, pos), stop, remaining)


def test_accept_against_the_seeded_draw():
    rng = np.random.default_rng(3)
    V, pos = 97, 40
    sp = dict(temperature=1.3, top_k=20, top_p=0.9, seed=77)
    rows = (rng.standard_normal((5, V)) * 2).astype(np.float32)
    a = drawn_ids(rows, sp, pos)
    am = drawn_ids(rows, None, pos)
    assert a != am, "the draws are the arg-max: the case shows nothing"
    # the draw depends on the token row's position, not on where in a step the row sits
    assert [drawn_ids(rows[j:j + 1], sp, pos + j)[0] for j in range(5)] == a
    assert drawn_ids(rows[1:2], sp, pos)[0] == ref_sample(rows[1], 1.3, 20, 0.9, 77, pos)
    # a draft of the drawn ids is accepted whole, one of the arg-max ids only as far as the two agree
    assert ref_accept_sampled(a[:4], rows, sp, pos, (), 9) == a
    agree = 0
    while agree < 4 and am[agree] == a[agree]:
        agree += 1
    assert ref_accept_sampled(am[:4], rows, sp, pos, (), 9) == a[:agree + 1]
    wrong = [(a[0] + 1) % V] + a[1:4]
    assert ref_accept_sampled(wrong, rows, sp, pos, (), 9) == a[:1]
    assert ref_accept_sampled(a[:4], rows, sp, pos, (a[2],), 9) == a[:a.index(a[2]) + 1]
    assert ref_accept_sampled(a[:4], rows, sp, pos, (), 3) == a[:3]
    assert ref_accept_sampled([], rows[:1], sp, pos, (), 9) == a[:1]
    # a greedy row is section 15's rule
    assert ref_accept_sampled(am[:4], rows, None, pos, (), 9) == am
    # the whole loop with the model replaced by a table of drawn ids: full acceptance from a planted history
    ids = [int(x) for x in rng.integers(10, 90, 12)]
    hist = [1, 2, 3] + ids + [4] + [1, 2, 3]
    draw = lambda p: ids[len(p) - 1] if list(p[1:]) == ids[:len(p) - 1] else -1  # noqa: E731
    got, steps, drafted, accepted = simulate(hist, draw, 12, 7, 3, 1)
    assert got == ids and (steps, drafted, accepted) == (2, 10, 10)


# ---------------------------------------------------------------------------
# the interface
# ---------------------------------------------------------------------------
NEW = {"llmi_session_batch_generate_lookup_sampled": 14, "llmi_logits_rows_gather": 10, "llmi_sample_logits_rows": 7}


def test_symbols_exported_and_bound_as_declared():
    from llm_inference_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym, n in NEW.items():
        params = declared(sym)
        assert len(params) == n and hasattr(lib, sym), sym
        res, args = _lib._SIGS[sym]
        assert res is ctypes.c_int and len(args) == n
        for p, a in zip(params, args):
            if "*" in p:
                assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), p
            elif p.startswith("float"):
                assert a is ctypes.c_float, p
            else:
                assert a is ctypes.c_int, p
    params = declared("llmi_session_batch_generate_lookup_sampled")
    args = _lib._SIGS["llmi_session_batch_generate_lookup_sampled"][1]
    # llmi_session_batch_generate_lookup's parameters with `samplers` before the outputs
    old = declared("llmi_session_batch_generate_lookup")
    assert params[:10] == old[:10] and params[11:] == old[10:]
    assert "llmi_sampler*" in params[10].replace(" *", "*") and params[10].endswith("samplers")
    assert args[10] is ctypes.POINTER(_lib.Sampler) and args[6] is ctypes.POINTER(_lib.Lookup)
    assert args[13] is ctypes.POINTER(_lib.LookupStats)
    assert [p.split()[-1].lstrip("*") for p in declared("llmi_logits_rows_gather")] == \
        ["x16", "w16", "T", "V", "E", "softcap", "idx", "n_idx", "cap", "logits"]
    assert [p.split()[-1].lstrip("*") for p in declared("llmi_sample_logits_rows")] == \
        ["logits", "R", "V", "samplers", "sampler_of_row", "pos", "ids"]
    assert _lib._SIGS["llmi_sample_logits_rows"][1][3] is ctypes.POINTER(_lib.Sampler)
    # the greedy entry point and llmi_session_info are not touched
    assert len(old) == 13 and len(_lib._SIGS["llmi_session_batch_generate_lookup"][1]) == 13
    assert _lib.SessionInfo._fields_[-1][0] == "score_path" and ctypes.sizeof(_lib.SessionInfo) == 136


def test_python_signatures():
    from llm_inference_amd import ops
    from llm_inference_amd.model import LookupResult, Model
    p = inspect.signature(Model.batch_generate_lookup_sampled).parameters
    assert list(p) == ["self", "histories", "slots", "pos", "max_new", "samplers", "draft_len", "ngram_max", "ngram_min",
                       "stop", "max_steps"]
    assert p["samplers"].default is inspect.Parameter.empty
    assert (p["draft_len"].default, p["ngram_max"].default, p["ngram_min"].default) == (7, 3, 1)
    assert p["stop"].default == () and p["max_steps"].default == 0
    assert inspect.signature(Model.batch_generate_lookup_sampled).return_annotation in (LookupResult, "LookupResult")
    # the greedy method's parameter list is unchanged
    q = inspect.signature(Model.batch_generate_lookup).parameters
    assert list(q) == ["self", "histories", "slots", "pos", "max_new", "draft_len", "ngram_max", "ngram_min", "stop",
                       "max_steps"]
    assert list(inspect.signature(ops.logits_rows_gather).parameters) == ["x16", "w16", "idx", "cap", "softcap", "out"]
    assert inspect.signature(ops.logits_rows_gather).parameters["cap"].default == 64
    assert list(inspect.signature(ops.sample_logits_rows).parameters) == ["logits", "samplers", "sampler_of_row", "pos"]


def test_samplers_marshalling():
    from llm_inference_amd import _lib
    from llm_inference_amd.model import Model, marshal_samplers, normalize_samplers
    sps = normalize_samplers([dict(temperature=0.5, top_k=40, top_p=0.9, seed=(1 << 64) + 5), None,
                              dict(temperature=2.0)], 3)
    arr = marshal_samplers(sps)
    assert len(arr) == 3 and isinstance(arr[0], _lib.Sampler)
    assert (arr[0].temperature, arr[0].top_k, arr[0].seed) == (0.5, 40, 5)
    assert abs(arr[0].top_p - 0.9) < 1e-7
    assert (arr[1].temperature, arr[1].top_k, arr[1].top_p, arr[1].seed) == (0.0, 0, 1.0, 0)  # None: a greedy row
    assert (arr[2].temperature, arr[2].top_k, arr[2].top_p, arr[2].seed) == (2.0, 0, 1.0, 0)
    one = marshal_samplers(normalize_samplers(dict(temperature=1.0, seed=9), 4))  # one dict: every row
    assert [one[b].seed for b in range(4)] == [9] * 4
    assert len(marshal_samplers([])) == 1  # (ctypes needs one entry; B = 0 reaches the library's check)
    # the method refuses before it reaches the library: no samplers, the wrong count, an unknown keyword
    m = object.__new__(Model)
    m.h = None
    with pytest.raises(ValueError, match="samplers"):
        Model.batch_generate_lookup_sampled(m, [[5, 6]], [0], [1], 4, None)
    with pytest.raises(ValueError, match="entries"):
        Model.batch_generate_lookup_sampled(m, [[5, 6]], [0], [1], 4, [dict(temperature=1.0)] * 2)
    with pytest.raises(ValueError, match="unknown"):
        Model.batch_generate_lookup_sampled(m, [[5, 6]], [0], [1], 4, dict(temperature=1.0, topk=3))
    with pytest.raises(ValueError, match="one entry"):
        Model.batch_generate_lookup_sampled(m, [[5, 6]], [0, 1], [1], 4, dict(temperature=1.0))
