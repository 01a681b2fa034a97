"""Host-side checks of the sampled batch loop's interface (no GPU): the library exports the new
entry points, their ctypes signatures match include/llmi.h, and Model.batch_generate's `samplers` argument is
normalised as documented."""
import ctypes
import inspect
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = {"llmi_session_batch_generate_sampled": 10, "llmi_logits_rows": 7, "llmi_logits_rows_rb": 1}


def test_new_symbols_exported_and_bound_as_declared():
    from llm_inference_amd import _lib
    src = open(os.path.join(ROOT, "include", "llmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym, n_args in NEW.items():
        m = re.search(r"\bint\s+" + sym + r"\s*\(([^)]*)\)\s*;", src)
        assert m, sym
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == n_args, sym
        assert hasattr(lib, sym), sym
        res, args = _lib._SIGS[sym]
        assert res is ctypes.c_int and len(args) == n_args, sym
        # pointers are bound as pointers, ints as ints, the soft-cap as a float
        for p, a in zip(params, args):
            if "*" in p:
                assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), (sym, p)
            elif p.startswith("float"):
                assert a is ctypes.c_float, (sym, p)
            else:
                assert a is ctypes.c_int, (sym, p)
    sampled = _lib._SIGS["llmi_session_batch_generate_sampled"][1]
    assert sampled[8] is ctypes.POINTER(_lib.Sampler)
    # the greedy entry's arguments with the samplers before `out`
    assert sampled[:8] == _lib._SIGS["llmi_session_batch_generate"][1][:8]
    # no field was added to llmi_session_info
    assert _lib.SessionInfo._fields_[-1][0] == "score_path" and ctypes.sizeof(_lib.SessionInfo) == 136


def test_logits_rows_rb_needs_no_device():
    from llm_inference_amd import ops
    assert [ops.logits_rows_rb(E) for E in (0, 64, 136, 6272)] == [0, 0, 0, 0]
    got = {E: ops.logits_rows_rb(E) for E in (128, 1152, 2560, 3840, 3968, 5376, 6144)}
    assert all(rb >= 2 for rb in got.values()), got
    # the block's rows wait in at most 64 KB of LDS
    assert all(rb * E * 2 <= 65536 for E, rb in got.items()), got


def test_python_signatures():
    from llm_inference_amd import ops
    from llm_inference_amd.model import Model
    p = inspect.signature(Model.batch_generate).parameters
    assert list(p) == ["self", "first", "slots", "pos", "n_steps", "stop", "samplers"]
    assert p["samplers"].default is None and p["stop"].default == ()
    p = inspect.signature(ops.logits_rows).parameters
    assert list(p) == ["x16", "w16", "softcap"] and p["softcap"].default == 0.0


def test_samplers_argument_normalisation():
    from llm_inference_amd.model import normalize_samplers
    assert normalize_samplers(None, 3) is None
    full = dict(temperature=0.7, top_k=40, top_p=0.9, seed=5)
    # one dict applies to every row
    assert normalize_samplers(full, 3) == [full, full, full]
    # set_sampler's defaults
    assert normalize_samplers(dict(temperature=2), 1) == [dict(temperature=2.0, top_k=0, top_p=1.0, seed=0)]
    # a sequence of dicts or None entries (None: a greedy row), any sequence type
    got = normalize_samplers((full, None, dict(temperature=1.0, seed=9)), 3)
    assert got == [full, None, dict(temperature=1.0, top_k=0, top_p=1.0, seed=9)]
    assert normalize_samplers([None, None], 2) == [None, None]
    assert normalize_samplers([], 0) == []
    for bad, n in (([full], 2), ([full, None, None], 2), ([], 1)):
        with pytest.raises(ValueError, match="entries"):
            normalize_samplers(bad, n)
    with pytest.raises(ValueError, match="unknown"):
        normalize_samplers(dict(temperature=1.0, min_p=0.1), 2)
    with pytest.raises(ValueError, match="temperature"):
        normalize_samplers([dict(top_k=4)], 1)
    with pytest.raises(ValueError, match="dict"):
        normalize_samplers([1.0], 1)
