"""Host-side checks of the scoring interface (no GPU): the C ABI declares it (tests/test_host.py's export test then
covers the built library), the Python signatures, the nll / perplexity arithmetic, and the scorer's launch planning
(llm_inference_amd/csrc/score_plan.h, compiled here with the host compiler)."""
import inspect
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_score_entry_points_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "llmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for sym, n_args in (("llmi_session_score", 8), ("llmi_score_rows", 10)):
        m = re.search(r"\bint\s+" + sym + r"\s*\(([^)]*)\)\s*;", src)
        assert m, sym
        assert len(m.group(1).split(",")) == n_args, sym
    from llm_inference_amd import _lib
    assert len(_lib._SIGS["llmi_session_score"][1]) == 8
    assert len(_lib._SIGS["llmi_score_rows"][1]) == 10
    # score_path is appended at the end of llmi_session_info, in the header and in its ctypes mirror
    body = re.search(r"typedef struct \{([^}]*)\}\s*llmi_session_info;", src).group(1)
    assert re.findall(r"(\w+)\s*;", body)[-1] == "score_path"
    assert _lib.SessionInfo._fields_[-1][0] == "score_path"
    # the struct is the caller's: code built against this header passes its size (the macro), and the unsized symbol
    # keeps the layout binaries built before the field expect (128 bytes, up to `sampling`)
    assert re.search(r"#define\s+llmi_session_get_info\(s,\s*info\)\s+llmi_session_get_info_sized\(\(s\),\s*\(info\),\s*"
                     r"sizeof\(llmi_session_info\)\)", src)
    assert _lib.SessionInfo.score_path.offset == 128 and _lib.SessionInfo.sampling.offset == 124
    assert len(_lib._SIGS["llmi_session_get_info_sized"][1]) == 3


def test_python_signatures():
    from llm_inference_amd import ops
    from llm_inference_amd.model import Model
    p = inspect.signature(Model.score).parameters
    assert list(p) == ["self", "tokens", "pos", "targets"]
    assert p["pos"].default == 0 and p["targets"].default is None
    assert list(inspect.signature(Model.perplexity).parameters) == ["self", "tokens"]
    assert inspect.signature(Model.trace).parameters["score"].default is False
    p = inspect.signature(ops.score_rows).parameters
    assert list(p) == ["x16", "w16", "targets", "softcap"]
    assert p["targets"].default is None and p["softcap"].default == 0.0


def test_nll_and_perplexity_arithmetic():
    from llm_inference_amd.score import ScoreResult, resolve_targets
    lp = np.array([-1.5, -0.25, 0.0, -2.0], np.float32)
    r = ScoreResult(lp, np.zeros(4, np.float32), np.zeros(4, np.int32), [7, 3, -1, 9])
    assert r.count == 3
    assert r.nll == 3.75
    assert r.perplexity == math.exp(3.75 / 3)
    # float64 summation: 2^24 + 1 + 1 is lost in float32, kept here
    big = ScoreResult(np.array([-16777216.0, -1.0, -1.0], np.float32), np.zeros(3), np.zeros(3), [1, 1, 1])
    assert big.nll == 16777218.0
    none = ScoreResult(np.zeros(2, np.float32), np.zeros(2), np.zeros(2), [-1, -1])
    assert none.count == 0 and none.nll == 0.0 and math.isnan(none.perplexity)
    t = np.array([5, 6, 7], np.int32)
    assert resolve_targets(t, None).tolist() == [6, 7, -1]
    assert resolve_targets(t, [1, -1, 2]).tolist() == [1, -1, 2]
    with pytest.raises(ValueError):
        resolve_targets(t, [1, 2])


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_score_plan_over_the_test_shapes(tmp_path):
    """scripts/dev/score_plan_check.cpp walks every tile of the plans for the GPU tests' shapes (and the real
    table's) and checks that no load index leaves the rows or the table and that the partial buffers hold every
    (token, tile) pair."""
    exe = str(tmp_path / "score_plan_check")
    src = os.path.join(ROOT, "scripts", "dev", "score_plan_check.cpp")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "score_plan_check OK" in out.stdout
