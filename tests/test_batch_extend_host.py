"""Host-side checks of the ragged batch step's interface (no GPU): the library exports
llmi_session_batch_extend, llmi_span and the ctypes binding match include/llmi.h, plan_extend_calls plans what
Model.prefill_sequences promises, and Model.batch_extend's arguments are marshalled as documented."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def header():
    src = open(os.path.join(ROOT, "include", "llmi.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_symbol_exported_and_bound_as_declared():
    from llm_inference_amd import _lib
    src = header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    sym = "llmi_session_batch_extend"
    m = re.search(r"\bint\s+" + sym + r"\s*\(([^)]*)\)\s*;", src)
    assert m, sym
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 7 and hasattr(lib, sym)
    res, args = _lib._SIGS[sym]
    assert res is ctypes.c_int and len(args) == 7
    for p, a in zip(params, args):
        if "*" in p:
            assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), p
        else:
            assert a is ctypes.c_int, p
    assert "llmi_span" in params[2] and args[2] is ctypes.POINTER(_lib.Span)
    assert params[3] == "int n_spans"
    # no field was added to llmi_session_info
    assert _lib.SessionInfo._fields_[-1][0] == "score_path" and ctypes.sizeof(_lib.SessionInfo) == 136


def test_span_struct_and_constants_match_the_header():
    from llm_inference_amd import _lib
    src = header()
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*llmi_span\s*;", src)
    assert m
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ty, names = decl.split(None, 1)
            assert ty == "int32_t", decl
            fields += [n.strip() for n in names.split(",")]
    assert fields == ["slot", "pos", "n_tokens", "out"]
    assert [n for n, _t in _lib.Span._fields_] == fields
    assert all(t is ctypes.c_int32 for _n, t in _lib.Span._fields_)
    assert ctypes.sizeof(_lib.Span) == 16
    assert [getattr(_lib.Span, n).offset for n in fields] == [0, 4, 8, 12]
    m = re.search(r"#define\s+LLMI_BATCH_TOKENS_MAX\s+(\d+)", src)
    assert m and int(m.group(1)) == _lib.BATCH_TOKENS_MAX == 512
    m = re.search(r"enum\s*\{([^}]*LLMI_SPAN_LAST[^}]*)\}", src)
    assert m
    enum = {k.strip(): int(v) for k, v in (e.split("=") for e in m.group(1).split(","))}
    assert enum == {"LLMI_SPAN_LAST": _lib.SPAN_LAST, "LLMI_SPAN_ALL": _lib.SPAN_ALL, "LLMI_SPAN_NONE": _lib.SPAN_NONE}
    assert (_lib.SPAN_LAST, _lib.SPAN_ALL, _lib.SPAN_NONE) == (0, 1, 2)


def test_python_signatures():
    from llm_inference_amd.model import Model, plan_extend_calls
    p = inspect.signature(Model.batch_extend).parameters
    assert list(p) == ["self", "seqs", "slots", "pos", "out", "want_logits"]
    assert p["out"].default == "last" and p["want_logits"].default is False
    p = inspect.signature(Model.prefill_sequences).parameters
    assert list(p) == ["self", "prompts", "slots", "pos"] and p["pos"].default == 0
    assert list(inspect.signature(plan_extend_calls).parameters) == ["lengths", "slots", "pos", "max_tokens"]


def check_plan(lengths, slots, pos, max_tokens=512):
    """The properties Model.prefill_sequences relies on; returns the calls."""
    from llm_inference_amd.model import plan_extend_calls
    calls = plan_extend_calls(lengths, slots, pos, max_tokens)
    starts = [pos] * len(lengths) if np.isscalar(pos) else list(pos)
    done = [0] * len(lengths)
    lasts = [0] * len(lengths)
    for call in calls:
        assert 1 <= sum(sp.n_tokens for sp in call) <= max_tokens
        assert len({sp.slot for sp in call}) == len(call), "a slot at most once per call"
        for sp in call:
            assert sp.n_tokens >= 1 and sp.slot == slots[sp.prompt]
            # consecutive: the span starts where the prompt's previous one ended
            assert sp.start == done[sp.prompt] and sp.pos == starts[sp.prompt] + sp.start
            done[sp.prompt] += sp.n_tokens
            final = done[sp.prompt] == lengths[sp.prompt]
            assert sp.out == ("last" if final else "none")
            lasts[sp.prompt] += final
    assert done == list(lengths), "every prompt covered exactly once"
    assert lasts == [1] * len(lengths)
    return calls


def test_plan_extend_calls():
    from llm_inference_amd.model import plan_extend_calls
    lengths = [1, 511, 512, 513, 1300]
    calls = check_plan(lengths, [3, 0, 4, 1, 2], [0, 5, 0, 7, 100])
    # nothing is wasted: every call but the last is full
    assert [sum(sp.n_tokens for sp in c) for c in calls[:-1]] == [512] * (len(calls) - 1)
    assert len(calls) == -(-sum(lengths) // 512)
    # the first call packs the two short prompts; the 1300 tokens are cut 511 + 512 + 277 over the last three calls
    assert [(sp.prompt, sp.n_tokens, sp.out) for sp in calls[0]] == [(0, 1, "last"), (1, 511, "last")]
    assert [(sp.n_tokens, sp.out) for c in calls for sp in c if sp.prompt == 4] == [(511, "none"), (512, "none"), (277, "last")]
    check_plan(lengths, [3, 0, 4, 1, 2], 0)
    check_plan(lengths[::-1], [3, 0, 4, 1, 2], [9, 0, 1, 0, 0])
    # 64 prompts of 9 tokens: 576 rows, two calls, at most 64 spans each
    calls = check_plan([9] * 64, list(range(64)), 0)
    assert len(calls) == 2 and all(len(c) <= 64 for c in calls)
    # a smaller budget
    calls = check_plan([5, 70, 3], [0, 1, 2], [0, 3, 0], max_tokens=32)
    assert len(calls) == 3
    with pytest.raises(ValueError, match="empty"):
        plan_extend_calls([4, 0, 2], [0, 1, 2], 0, 512)
    with pytest.raises(ValueError, match="slot"):
        plan_extend_calls([4, 4], [1, 1], 0, 512)
    with pytest.raises(ValueError, match="one entry"):
        plan_extend_calls([4, 4], [0, 1], [0], 512)
    assert plan_extend_calls([], [], 0, 512) == []


def test_batch_extend_argument_marshalling():
    from llm_inference_amd import _lib
    from llm_inference_amd.model import marshal_extend
    seqs = [[5, 6, 7], np.array([8], np.int64), (9, 10)]
    tok, arr, off = marshal_extend(seqs, [2, 0, 4], [10, 0, 31], ["all", "last", "none"])
    assert tok.dtype == np.int32 and tok.tolist() == [5, 6, 7, 8, 9, 10]
    assert isinstance(arr[0], _lib.Span) and len(arr) == 3
    assert [(s.slot, s.pos, s.n_tokens, s.out) for s in arr] == [(2, 10, 3, 1), (0, 0, 1, 0), (4, 31, 2, 2)]
    assert off.tolist() == [0, 3, 4, 4]
    # one value for every span
    for out, want, code in (("last", [0, 1, 2, 3], 0), ("all", [0, 3, 4, 6], 1), ("none", [0, 0, 0, 0], 2)):
        tok, arr, off = marshal_extend(seqs, [2, 0, 4], [10, 0, 31], out)
        assert off.tolist() == want and [s.out for s in arr] == [code] * 3
    assert marshal_extend(seqs, [2, 0, 4], [10, 0, 31])[2].tolist() == [0, 1, 2, 3]  # the default: "last"
    with pytest.raises(ValueError, match="one entry"):
        marshal_extend(seqs, [2, 0], [10, 0, 31])
    with pytest.raises(ValueError, match="one entry"):
        marshal_extend(seqs, [2, 0, 4], [10, 0, 31], ["all", "last"])
    with pytest.raises(ValueError, match="none of"):
        marshal_extend(seqs, [2, 0, 4], [10, 0, 31], "first")
