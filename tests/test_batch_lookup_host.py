"""Host-side checks of lookup decoding's interface (no GPU): the library exports both symbols,
llmi_lookup and the ctypes bindings match include/llmi.h, Model.batch_generate_lookup's arguments are marshalled as
documented, and the rule itself -- ref_lookup_draft and ref_accept below, the short pure-Python statements the GPU
tests compare the kernel with -- agrees with a brute-force enumeration on small random histories."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


# ---------------------------------------------------------------------------
# the rule (include/llmi.h)
# ---------------------------------------------------------------------------
def ref_lookup_draft(h, ngram_max, ngram_min, n_draft):
    """(draft list, match_end, match_len): candidate ends e in [0, L-2], ml(e) the longest common suffix of h[..e] and
    h, capped by ngram_max, e + 1 and L - 1; the largest (ml, e) with ml >= ngram_min; the continuation from e + 1,
    periodic with period L - (e + 1).  n_draft: how many tokens to draft on a match (min(draft_len, remaining - 1))."""
    h = [int(x) for x in h]
    L = len(h)
    best = None
    for e in range(L - 1):
        ml = 0
        while ml < min(ngram_max, e + 1, L - 1) and h[e - ml] == h[L - 1 - ml]:
            ml += 1
        if ml >= ngram_min and (best is None or (ml, e) > best):
            best = (ml, e)
    if best is None or n_draft <= 0:
        return [], -1, 0
    c = best[1] + 1
    return [h[c + j % (L - c)] for j in range(n_draft)], best[1], best[0]


def ref_accept(draft, a, stop, remaining):
    """The ids a step emits: a[j] = the greedy id of span row j of [cur, draft...]."""
    out = [int(a[0])]
    for j in range(1, len(draft) + 1):
        if int(draft[j - 1]) != int(a[j - 1]):
            break
        out.append(int(a[j]))
    for i, t in enumerate(out):
        if t in stop:
            out = out[:i + 1]
            break
    return out[:remaining]


def simulate(hist, greedy, max_new, draft_len, ngram_max, ngram_min, stop=(), max_steps=0, trace=None):
    """The whole loop for one row on the host.  greedy(prefix list) -> the greedy id after that prefix, where the
    prefix is what the row has run so far *from its last history token on* ([cur], [cur, x1], ...).  Returns
    (ids, steps, drafted, accepted); trace (a list) receives (draft, emitted ids) per step."""
    h = [int(x) for x in hist]
    ran = []  # the tokens run at pos, pos + 1, ...
    ids, steps, drafted, accepted, remaining = [], 0, 0, 0, max_new
    done = False
    while not done and (max_steps == 0 or steps < max_steps):
        d, _e, _ml = ref_lookup_draft(h, ngram_max, ngram_min, min(draft_len, remaining - 1))
        span = [h[-1]] + d
        a = [greedy(ran + span[:j + 1]) for j in range(len(span))]
        out = ref_accept(d, a, stop, remaining)
        ran += span[:len(out)]
        h += out
        ids += out
        remaining -= len(out)
        steps += 1
        drafted += len(d)
        accepted += len(out) - 1
        if trace is not None:
            trace.append((d, out))
        done = remaining == 0 or out[-1] in stop
    return ids, steps, drafted, accepted


def brute_draft(h, N, nmin, n_draft):
    """The rule by enumeration: every (n, start) with h[start:start + n] == the last n tokens, the occurrence not the
    suffix itself; longest n first, then the latest."""
    h = list(h)
    L = len(h)
    for n in range(min(N, L - 1), nmin - 1, -1):
        for start in range(L - 1 - n, -1, -1):  # the occurrence ends at start + n - 1 <= L - 2
            if h[start:start + n] == h[L - n:]:
                c = start + n
                ext = list(h)
                while len(ext) < c + n_draft:  # periodic continuation: the history extended by its own tail
                    ext.append(ext[len(ext) - (L - c)])
                return ext[c:c + n_draft], c - 1, n
    return [], -1, 0


def test_reference_rule_against_enumeration():
    rng = np.random.default_rng(21)
    n_match = n_wrap = 0
    for _ in range(1500):
        L = int(rng.integers(1, 14))
        h = rng.integers(0, 3, L).tolist()
        N = int(rng.integers(1, 5))
        nmin = int(rng.integers(1, N + 1))
        D = int(rng.integers(1, 9))
        got = ref_lookup_draft(h, N, nmin, D)
        assert got == tuple(brute_draft(h, N, nmin, D)), (h, N, nmin, D)
        if got[0]:
            n_match += 1
            n_wrap += got[1] + 1 + D > L
            assert len(got[0]) == D and got[2] >= nmin
    assert n_match > 300 and n_wrap > 100
    # the cases the GPU test names
    assert ref_lookup_draft([7], 3, 1, 4) == ([], -1, 0)
    assert ref_lookup_draft([1, 2, 3, 4], 3, 1, 4) == ([], -1, 0)
    assert ref_lookup_draft([5, 5], 3, 1, 3) == ([5, 5, 5], 0, 1)                       # period 1
    assert ref_lookup_draft([1, 2, 3, 1, 2, 3, 1], 3, 1, 5) == ([2, 3, 1, 2, 3], 3, 3)  # period 3, wraps
    assert ref_lookup_draft([1, 2, 9, 8, 2, 7, 1, 2], 3, 1, 2) == ([9, 8], 1, 2)        # longer and older wins
    assert ref_lookup_draft([1, 2, 9, 8, 2, 7, 1, 2], 1, 1, 2) == ([7, 1], 4, 1)        # ... unless n is capped
    assert ref_lookup_draft([4, 9, 5, 6, 9], 3, 2, 2) == ([], -1, 0)                    # ngram_min rejects n = 1


def test_reference_accept():
    assert ref_accept([], [9], (), 5) == [9]
    assert ref_accept([1, 2, 3], [1, 2, 7, 8], (), 9) == [1, 2, 7]        # 2 of 3 accepted
    assert ref_accept([1, 2, 3], [1, 2, 3, 8], (), 9) == [1, 2, 3, 8]     # all accepted: nd + 1 ids
    assert ref_accept([4, 2, 3], [1, 2, 3, 8], (), 9) == [1]              # the first draft is wrong
    assert ref_accept([1, 2, 3], [1, 2, 3, 8], (2,), 9) == [1, 2]         # cut after the stop id, inclusive
    assert ref_accept([1, 2, 3], [1, 2, 3, 8], (7,), 9) == [1, 2, 3, 8]
    assert ref_accept([1, 2, 3], [1, 2, 3, 8], (), 2) == [1, 2]           # the budget
    # the loop on a model that repeats its input: every draft after the first step is accepted
    ids, steps, drafted, accepted = simulate([3, 4, 5], lambda p: p[-1], 20, 7, 3, 1)
    # (step 1 has no match: 1 id; then 7 drafts + 1, twice; the last step's draft is cut to the 3 ids left: 2 + 1)
    assert ids == [5] * 20 and (steps, drafted, accepted) == (4, 16, 16)
    ids, steps, _d, _a = simulate([3, 4, 5], lambda p: p[-1], 20, 7, 3, 1, max_steps=2)
    assert ids == [5] * 9 and steps == 2


# ---------------------------------------------------------------------------
# the interface
# ---------------------------------------------------------------------------
def header():
    src = open(os.path.join(ROOT, "include", "llmi.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def declared(sym):
    m = re.search(r"\bint\s+" + sym + r"\s*\(([^)]*)\)\s*;", header())
    assert m, sym
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_symbols_exported_and_bound_as_declared():
    from llm_inference_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym, n in (("llmi_session_batch_generate_lookup", 13), ("llmi_lookup_draft", 9)):
        params = declared(sym)
        assert len(params) == n and hasattr(lib, sym), sym
        res, args = _lib._SIGS[sym]
        assert res is ctypes.c_int and len(args) == n
        for p, a in zip(params, args):
            if "*" in p:
                assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), p
            else:
                assert a is ctypes.c_int, p
    params = declared("llmi_session_batch_generate_lookup")
    args = _lib._SIGS["llmi_session_batch_generate_lookup"][1]
    assert "llmi_lookup*" in params[6].replace(" *", "*") and args[6] is ctypes.POINTER(_lib.Lookup)
    assert "llmi_lookup_stats*" in params[12].replace(" *", "*") and args[12] is ctypes.POINTER(_lib.LookupStats)
    assert params[5] == "int B" and params[7] == "int max_steps" and params[9] == "int n_stop"
    assert declared("llmi_lookup_draft")[1:5] == ["int L", "int ngram_max", "int ngram_min", "int draft_len"]
    # llmi_session_info is not touched
    assert _lib.SessionInfo._fields_[-1][0] == "score_path" and ctypes.sizeof(_lib.SessionInfo) == 136


def test_lookup_structs_match_the_header():
    from llm_inference_amd import _lib
    src = header()
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*llmi_lookup\s*;", src)
    assert m
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ty, names = decl.split(None, 1)
            assert ty == "int32_t", decl
            fields += [n.strip() for n in names.split(",")]
    assert fields == ["draft_len", "ngram_max", "ngram_min", "max_new"]
    assert [n for n, _t in _lib.Lookup._fields_] == fields
    assert all(t is ctypes.c_int32 for _n, t in _lib.Lookup._fields_)
    assert ctypes.sizeof(_lib.Lookup) == 16
    assert [getattr(_lib.Lookup, n).offset for n in fields] == [0, 4, 8, 12]
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*llmi_lookup_stats\s*;", src)
    assert m
    decls = [" ".join(d.split()) for d in m.group(1).split(";") if d.strip()]
    assert decls == ["int32_t steps", "int32_t drafted[LLMI_SEQ_MAX]", "int32_t accepted[LLMI_SEQ_MAX]"]
    m = re.search(r"#define\s+LLMI_SEQ_MAX\s+(\d+)", src)
    assert m and int(m.group(1)) == _lib.SEQ_MAX
    assert [n for n, _t in _lib.LookupStats._fields_] == ["steps", "drafted", "accepted"]
    assert ctypes.sizeof(_lib.LookupStats) == 4 + 8 * _lib.SEQ_MAX
    assert _lib.LookupStats.drafted.offset == 4 and _lib.LookupStats.accepted.offset == 4 + 4 * _lib.SEQ_MAX


def test_python_signatures():
    from llm_inference_amd import ops
    from llm_inference_amd.model import LookupResult, Model
    p = inspect.signature(Model.batch_generate_lookup).parameters
    assert list(p) == ["self", "histories", "slots", "pos", "max_new", "draft_len", "ngram_max", "ngram_min", "stop",
                       "max_steps"]
    assert (p["draft_len"].default, p["ngram_max"].default, p["ngram_min"].default) == (7, 3, 1)
    assert p["stop"].default == () and p["max_steps"].default == 0
    assert list(inspect.signature(ops.lookup_draft).parameters) == ["history", "ngram_max", "ngram_min", "draft_len"]
    assert [f for f in LookupResult.__dataclass_fields__] == ["ids", "steps", "drafted", "accepted"]


def test_argument_marshalling():
    from llm_inference_amd.model import marshal_lookup
    tok, hl, sl, p = marshal_lookup([[5, 6, 7], np.array([8], np.int64), (9, 10)], [2, 0, 4], [10, 1, 31])
    assert tok.dtype == hl.dtype == sl.dtype == p.dtype == np.int32
    assert tok.tolist() == [5, 6, 7, 8, 9, 10] and hl.tolist() == [3, 1, 2]
    assert sl.tolist() == [2, 0, 4] and p.tolist() == [10, 1, 31]
    tok, hl, _sl, _p = marshal_lookup([[5], []], [0, 1], [1, 1])  # an empty history reaches the library's check
    assert tok.tolist() == [5] and hl.tolist() == [1, 0]
    with pytest.raises(ValueError, match="one entry"):
        marshal_lookup([[5, 6]], [0, 1], [3, 4])
    with pytest.raises(ValueError, match="one entry"):
        marshal_lookup([[5, 6], [7]], [0, 1], [3])
