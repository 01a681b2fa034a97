"""Teacher-forced scoring on the device (llmi_session_score / llmi_score_rows; llm_inference_amd/csrc/k_score.hip;
DESIGN.md section 11): per-position log-probs, log-sum-exp and greedy ids.

Bounds (derived in DESIGN.md section 11, not measured).  The f64 reference is computed in numpy from the very f16
inputs the kernel reads.  For token t:
  B_t   = max_v E 2^-23 sum_k |w_vk x_tk|   (any f32 summation order of E exact f16 x f16 products, truncating
          accumulation included; the soft-cap and the log-sum-exp are 1-Lipschitz in the logits)
  eps_t = 64 2^-24 (1 + max_v |l_tv|)       (expf / logf at a few ulp, a tree of depth <= 18, the final f32 rounding)
  |lse - ref| <= B_t + eps_t,  |logprob - ref| <= 2 B_t + eps_t,
  argmax = the f64 argmax wherever the f64 top-2 margin exceeds 2 B_t, and the lower id on exact ties.
With a soft-cap `cap` every capped logit carries, besides B_t, the rounding of l / cap, tanhf's 2 ulp of a value
below 1 and the rounding of the product: at most CAP_ULPS = 2 cap 2^-23 per logit, so lse gets + CAP_ULPS, logprob
+ 2 CAP_ULPS and the argmax margin 2 (B_t + CAP_ULPS).
Every test prints its worst measured error over bound.
"""
import contextlib
import functools
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FAST_VS_REF = 6e-2  # tests/test_prefill.py: the fast budget between the batched prefill and the token loop
VT = 128            # vocabulary rows per work-group of the scorer (score_plan.h SCORE_VT)


# ---------------------------------------------------------------------------
# the f64 reference and the bounds
# ---------------------------------------------------------------------------
def ref_scores(x16, w16, targets, softcap=0.0):
    """x16 [T][E], w16 [V][E] float16.  Returns dict(l, lse, logprob, argmax, margin, B, eps, cap_ulps)."""
    x, w = x16.astype(np.float64), w16.astype(np.float64)
    E = x.shape[1]
    l = x @ w.T
    B = E * 2.0 ** -23 * (np.abs(x) @ np.abs(w).T).max(axis=1)
    cap_ulps = 0.0
    if softcap > 0:
        l = softcap * np.tanh(l / softcap)
        cap_ulps = 2.0 * softcap * 2.0 ** -23
    return logits_scores(l, targets, B, cap_ulps)


def logits_scores(l, targets, B=None, cap_ulps=0.0):
    """The same from f64 logits l [T][V] (B: the GEMM bound per token, 0 when the logits are given)."""
    T = l.shape[0]
    m = l.max(axis=1)
    lse = m + np.log(np.exp(l - m[:, None]).sum(axis=1))
    tg = np.asarray(targets)
    lp = np.where(tg >= 0, l[np.arange(T), np.maximum(tg, 0)] - lse, 0.0)
    srt = np.sort(l, axis=1)
    margin = srt[:, -1] - srt[:, -2] if l.shape[1] > 1 else np.full(T, np.inf)
    eps = 64 * 2.0 ** -24 * (1 + np.abs(l).max(axis=1))
    return dict(l=l, lse=lse, logprob=lp, argmax=l.argmax(axis=1), margin=margin,
                B=np.zeros(T) if B is None else B, eps=eps, cap_ulps=cap_ulps)


def check_bounds(got, ref, targets, what):
    """got: a ScoreResult (or anything with .lse / .logprobs / .argmax)."""
    tg = np.asarray(targets)
    b_lse = ref["B"] + ref["eps"] + ref["cap_ulps"]
    b_lp = 2 * ref["B"] + ref["eps"] + 2 * ref["cap_ulps"]
    e_lse = np.abs(got.lse.astype(np.float64) - ref["lse"])
    e_lp = np.abs(got.logprobs.astype(np.float64) - ref["logprob"])
    decided = ref["margin"] > 2 * (ref["B"] + ref["cap_ulps"])
    print(f"{what}: worst |lse - f64| / bound {float((e_lse / b_lse).max()):.3g}, "
          f"|logprob - f64| / bound {float((e_lp / b_lp)[tg >= 0].max()) if (tg >= 0).any() else 0.0:.3g}, "
          f"{int(decided.sum())} of {len(decided)} argmax rows decided by the margin")
    assert np.isfinite(got.lse).all() and np.isfinite(got.logprobs).all(), what
    assert (e_lse <= b_lse).all(), (what, float((e_lse / b_lse).max()))
    assert (e_lp <= b_lp).all(), (what, float((e_lp / b_lp).max()))
    assert (got.logprobs[tg < 0] == 0.0).all(), what
    np.testing.assert_array_equal(got.argmax[decided], ref["argmax"][decided], err_msg=what)


def boundary_targets(V):
    """0, V - 1, both sides of every vocabulary-tile boundary, and -1."""
    ids = [0, V - 1, -1]
    for b in range(VT, V, VT):
        ids += [b - 1, b]
    return ids


def rand16(rng, shape, scale):
    return (rng.standard_normal(shape) * scale).astype(np.float16)


# ---------------------------------------------------------------------------
# 1. op level
# ---------------------------------------------------------------------------
OP_CASES = [(1, 64, 256), (31, 129, 256), (33, 1000, 1152), (130, 4096, 2560), (70, 2113, 5376)]


@functools.lru_cache(maxsize=None)
def op_case(T, V, E):
    rng = np.random.default_rng(1000 * T + V + E)
    x = rand16(rng, (T, E), 1.0)
    w = rand16(rng, (V, E), 4.0 / np.sqrt(E))  # logits of a few units
    x.setflags(write=False)
    w.setflags(write=False)
    return x, w


@pytest.mark.parametrize("T,V,E", OP_CASES)
def test_score_rows_bounds(T, V, E):
    from llm_inference_amd.ops import score_rows
    x, w = op_case(T, V, E)
    ids = boundary_targets(V)
    rng = np.random.default_rng(5)
    for off in range(0, len(ids), T):  # every boundary id is some row's target (several calls when T is small)
        part = ids[off:off + T]
        tg = np.array(part + rng.integers(0, V, T - len(part)).tolist(), np.int32)
        ref = ref_scores(x, w, tg)
        check_bounds(score_rows(x, w, tg), ref, tg, f"score_rows T={T} V={V} E={E} targets[{off}:]")
    none = score_rows(x, w)  # no targets at all
    assert (none.logprobs == 0.0).all()
    np.testing.assert_array_equal(none.lse.view(np.uint32), score_rows(x, w, tg).lse.view(np.uint32))


@pytest.mark.parametrize("T,V,E,cut", [(33, 1000, 1152, 7), (130, 4096, 2560, 100)])
def test_score_rows_split_calls_bit_identical(T, V, E, cut):
    """A row's results read only its own x16 row: the rows in two calls give the same bits."""
    from llm_inference_amd.ops import score_rows
    x, w = op_case(T, V, E)
    tg = np.random.default_rng(6).integers(-1, V, T).astype(np.int32)
    whole = score_rows(x, w, tg)
    a, b = score_rows(x[:cut], w, tg[:cut]), score_rows(x[cut:], w, tg[cut:])
    for name in ("logprobs", "lse", "argmax"):
        got = np.concatenate([getattr(a, name), getattr(b, name)])
        np.testing.assert_array_equal(got.view(np.uint32), getattr(whole, name).view(np.uint32), err_msg=name)


def test_score_rows_ties_lower_id_wins():
    """Two identical table rows hold the maximum, in one 32-row MFMA tile, in two waves of a work-group and in two
    work-groups: the lower id wins each time."""
    from llm_inference_amd.ops import score_rows
    rng = np.random.default_rng(7)
    T, V, E = 6, 300, 256
    x = rand16(rng, (T, E), 1.0)
    for lo, hi in ((3, 17), (5, 70), (40, 200), (129, 299)):
        w = rand16(rng, (V, E), 0.05)
        w[lo] = w[hi] = (np.sign(x[2].astype(np.float32)) * 0.5).astype(np.float16)  # row 2's logit: 0.5 sum |x|
        got = score_rows(x, w, np.full(T, hi, np.int32))
        ref = ref_scores(x, w, np.full(T, hi, np.int32))
        assert ref["l"][2, lo] == ref["l"][2, hi] == ref["l"][2].max()
        assert got.argmax[2] == lo, (lo, hi, got.argmax[2])
        check_bounds(got, ref, np.full(T, hi, np.int32), f"tie {lo}/{hi}")


def test_score_rows_large_logits_and_zero_row():
    """Logits reaching +-80: exp(80) overflows nothing only if the maximum is subtracted -- no inf / NaN, the same
    bounds.  An all-zero x row: every logit 0, lse = log V, argmax = 0."""
    from llm_inference_amd.ops import score_rows
    rng = np.random.default_rng(8)
    T, V, E = 9, 777, 512
    x, w = rand16(rng, (T, E), 1.0), rand16(rng, (V, E), 0.05)
    l = x.astype(np.float64) @ w.astype(np.float64).T
    x = (x.astype(np.float64) * (80.0 / np.abs(l).max(axis=1))[:, None]).astype(np.float16)
    x[4] = 0
    tg = rng.integers(0, V, T).astype(np.int32)
    ref = ref_scores(x, w, tg)
    assert np.abs(ref["l"]).max() > 79
    got = score_rows(x, w, tg)
    check_bounds(got, ref, tg, "logits to +-80")
    assert got.argmax[4] == 0
    assert abs(float(got.lse[4]) - np.log(V)) <= ref["eps"][4]
    assert abs(float(got.logprobs[4]) + np.log(V)) <= ref["eps"][4]


def test_score_rows_softcap():
    """softcap = 30 against f64 30 tanh(l / 30).  eps_t is widened by tanhf's 2 ulp (and the two roundings around
    it): CAP_ULPS = 2 cap 2^-23 per capped logit (module docstring)."""
    from llm_inference_amd.ops import score_rows
    rng = np.random.default_rng(9)
    T, V, E = 12, 1000, 256
    x, w = rand16(rng, (T, E), 1.0), rand16(rng, (V, E), 1.5)  # logits of +-24 rms: well into the cap's bend
    tg = rng.integers(-1, V, T).astype(np.int32)
    ref = ref_scores(x, w, tg, softcap=30.0)
    assert np.abs(ref["l"]).max() > 29
    check_bounds(score_rows(x, w, tg, softcap=30.0), ref, tg, "softcap 30")


def test_score_rows_argument_errors():
    from llm_inference_amd._lib import LLMIError
    from llm_inference_amd.ops import score_rows
    x, w = np.zeros((2, 24), np.float16), np.zeros((5, 24), np.float16)
    with pytest.raises(LLMIError) as ei:  # E % 16 != 0
        score_rows(x, w)
    assert ei.value.status == "E_SIZE"
    x, w = np.zeros((2, 32), np.float16), np.zeros((5, 32), np.float16)
    with pytest.raises(LLMIError) as ei:
        score_rows(x, w, np.array([0, 5], np.int32))
    assert ei.value.status == "E_RANGE" and "targets" in str(ei.value)


# ---------------------------------------------------------------------------
# sessions
# ---------------------------------------------------------------------------
@contextlib.contextmanager
def env(**kv):
    """LLMI_* variables the library reads at the call (chunking, LLMI_NO_PREFILL), restored afterwards."""
    keys = ("LLMI_NO_PREFILL", "LLMI_PREFILL_CHUNK", "LLMI_PREFILL_FULL_LAST")
    old = {k: os.environ.get(k) for k in keys}
    for k in keys:
        os.environ.pop(k, None)
    for k, v in kv.items():
        os.environ[k] = str(v)
    try:
        yield
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def taps(trace, name, dtype):
    return np.concatenate([np.frombuffer(b, dtype) for n, _l, b in trace if n == name])


class Tapped:
    def __init__(self, trace):
        self.lse = taps(trace, "sc_lse", np.float32)
        self.logprobs = taps(trace, "sc_logprob", np.float32)
        self.argmax = taps(trace, "sc_argmax", np.int32)


def table16(g, cfg):
    from llm_inference_amd.gguf import GGUFFile
    f = GGUFFile(g)
    return np.frombuffer(f.get_tensor_data(f.tensor("token_embd.weight")), np.float16).reshape(cfg.vocab, cfg.n_embd)


FUSED = {"mini-1b": dict(n=40, chunk=None, cut=17), "mini-4b": dict(n=300, chunk=128, cut=100)}


@functools.lru_cache(maxsize=None)
def fused_case(cfg_name):
    """The gguf, the prompt, and one traced scoring run (computed once, read-only)."""
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg, c = CONFIGS[cfg_name], FUSED[cfg_name]
    g = build_gemma3_gguf(cfg, seed=21)
    prompt = np.random.default_rng(3).integers(4, cfg.vocab, c["n"]).astype(np.int32)
    kv = {"LLMI_PREFILL_CHUNK": c["chunk"]} if c["chunk"] else {}
    with env(**kv):
        m = Model(g, max_ctx=512)
        assert m.get_info().score_path == 1
        tr = m.trace(prompt, 0, score=True)
        m.close()
    x16 = taps(tr, "sc_x16", np.float16).reshape(c["n"], cfg.n_embd)
    return dict(cfg=cfg, g=g, prompt=prompt, kv=kv, x16=x16, tap=Tapped(tr), names={n for n, _l, _b in tr})


@pytest.mark.parametrize("cfg_name", list(FUSED))
def test_fused_rows_are_forwards_rows(cfg_name):
    """sc_x16 row i = f16(result_norm of trace(prompt[:i + 1])) bit for bit: the scorer reads what forward of the
    prefix hands its logits GEMV.  The rows carry no per-token scales (no sc_xs tap)."""
    from llm_inference_amd.model import Model
    c = fused_case(cfg_name)
    n = len(c["prompt"])
    assert "sc_xs" not in c["names"]
    with env(**c["kv"]):
        m = Model(c["g"], max_ctx=512)
        for i in (0, 1, 31, 32, n - 1):
            tr = m.trace(c["prompt"][:i + 1], 0)
            rn = [np.frombuffer(b, np.float32) for nm, _l, b in tr if nm == "result_norm"][-1]
            np.testing.assert_array_equal(c["x16"][i].view(np.uint16), rn.astype(np.float16).view(np.uint16),
                                          err_msg=f"row {i}")
        m.close()


@pytest.mark.parametrize("cfg_name", list(FUSED))
def test_fused_outputs_meet_bounds(cfg_name):
    c = fused_case(cfg_name)
    tg = np.concatenate([c["prompt"][1:], [-1]]).astype(np.int32)
    ref = ref_scores(c["x16"], table16(c["g"], c["cfg"]), tg)
    check_bounds(c["tap"], ref, tg, f"{cfg_name} fused session, every position")


@pytest.mark.parametrize("cfg_name", list(FUSED))
def test_fused_entry_points_and_rechunking_bit_identical(cfg_name):
    """score() returns the taps' bits; re-chunking (33, the default) and scoring the prompt in two calls (the second
    at a later position, its keys from the first) change no bit."""
    from llm_inference_amd.model import Model
    c = fused_case(cfg_name)
    prompt, cut = c["prompt"], FUSED[cfg_name]["cut"]
    tg = np.concatenate([prompt[1:], [-1]]).astype(np.int32)

    def same(r, what):
        for name in ("logprobs", "lse", "argmax"):
            np.testing.assert_array_equal(getattr(r, name).view(np.uint32), getattr(c["tap"], name).view(np.uint32),
                                          err_msg=f"{what}: {name}")

    for kv in (c["kv"], {"LLMI_PREFILL_CHUNK": 33}, {}):
        with env(**kv):
            m = Model(c["g"], max_ctx=512)
            r = m.score(prompt)
            same(r, f"score() with {kv}")
            assert r.targets.tolist() == tg.tolist()
            same(m.score(prompt, 0, tg), "explicit targets")
            m.close()
    with env():
        m = Model(c["g"], max_ctx=512)
        a = m.score(prompt[:cut], 0, tg[:cut])
        b = m.score(prompt[cut:], cut, tg[cut:])
        m.close()
    from llm_inference_amd.score import ScoreResult
    same(ScoreResult(*[np.concatenate([getattr(a, k), getattr(b, k)]) for k in ("logprobs", "lse", "argmax", "targets")]),
         f"two calls cut at {cut}")


@pytest.mark.parametrize("cfg_name", list(FUSED))
def test_fused_state_after_score_is_forwards(cfg_name):
    """After score(prompt) the session continues as after forward(prompt): the same greedy ids; the last position's
    results are those of forward's logits.  forward itself keeps its trim: its logits equal the full last layer's
    (LLMI_PREFILL_FULL_LAST) bit for bit, as tests/test_prefill.py::test_prefill_last_layer_final_token_only."""
    from llm_inference_amd.model import Model
    c = fused_case(cfg_name)
    prompt, n = c["prompt"], len(c["prompt"])
    with env(**c["kv"]):
        mf = Model(c["g"], max_ctx=512)
        lg = mf.forward(prompt, 0)
        ids_f = mf.generate(int(np.argmax(lg)), n, 8).tolist()
        mf.close()
        ms = Model(c["g"], max_ctx=512)
        r = ms.score(prompt)
        ids_s = ms.generate(int(r.argmax[-1]), n, 8).tolist()
        lg2 = ms.forward(prompt, 0)  # and forward after a score on the same session
        ms.close()
    assert int(r.argmax[-1]) == int(np.argmax(lg))
    assert ids_s == ids_f
    np.testing.assert_array_equal(lg2.view(np.uint32), lg.view(np.uint32))
    last = logits_scores(lg.astype(np.float64)[None, :], [-1])
    # forward's f32 logits against the scorer's own chain of the same products: both within B of the exact ones
    B = ref_scores(c["x16"][-1:], table16(c["g"], c["cfg"]), [-1])["B"][0]
    assert abs(float(r.lse[-1]) - last["lse"][0]) <= 2 * B + last["eps"][0]
    with env(LLMI_PREFILL_FULL_LAST=1, **c["kv"]):
        mfull = Model(c["g"], max_ctx=512)
        lfull = mfull.forward(prompt, 0)
        mfull.close()
    np.testing.assert_array_equal(lfull.view(np.uint32), lg.view(np.uint32))


def test_time_kernel_scorer():
    """time_kernel(9): 0 / 0 before anything was scored, then the scorer's launches over the last chunk with the
    table's and the rows' bytes."""
    from llm_inference_amd.model import Model
    c = fused_case("mini-1b")
    cfg = c["cfg"]
    with env():
        m = Model(c["g"], max_ctx=512)
        assert m.time_kernel(9, 2) == (0.0, 0.0)
        m.score(c["prompt"])
        us, by = m.time_kernel(9, 2)
        m.close()
    assert us > 0 and by == 2.0 * cfg.n_embd * (cfg.vocab + len(c["prompt"]))


def test_get_info_never_writes_past_the_callers_struct():
    """score_path is appended to a struct the CALLER allocates.  A binary built before it (the 128-byte struct, e.g.
    an already built main loop of integration/main_mi355x.cpp with the struct on its stack) calls the unsized symbol:
    it fills the fields up to `sampling` and leaves every byte after them alone.  The sized form stops at the size
    it is given."""
    import ctypes as C
    from llm_inference_amd._lib import SessionInfo, check, lib
    from llm_inference_amd.model import Model
    c = fused_case("mini-1b")
    with env():
        m = Model(c["g"], max_ctx=64)
        full = m.get_info()
        old = SessionInfo.score_path.offset
        assert old == 128 and C.sizeof(SessionInfo) == 136
        buf = (C.c_ubyte * 256)(*([0xA5] * 256))
        check(lib().llmi_session_get_info(m.h, C.addressof(buf)))
        assert bytes(buf[:old]) == bytes(full)[:old]
        assert bytes(buf[old:]) == b"\xa5" * (256 - old)
        for size in (0, 56, old, C.sizeof(SessionInfo), 200):
            buf = (C.c_ubyte * 256)(*([0xA5] * 256))
            check(lib().llmi_session_get_info_sized(m.h, C.cast(buf, C.POINTER(SessionInfo)), size))
            n = min(size, C.sizeof(SessionInfo))
            assert bytes(buf[:n]) == bytes(full)[:n] and bytes(buf[n:]) == b"\xa5" * (256 - n), size
        m.close()


# ---------------------------------------------------------------------------
# 3. row path
# ---------------------------------------------------------------------------
def test_row_path_vs_fused_path():
    """LLMI_NO_PREFILL=1: the token loop with full logits and the f64 row reduce (score_path 2) against the fused
    path: twice the fast budget between exactly these two paths, the same ids wherever the row path's top-2 margin
    exceeds that."""
    from llm_inference_amd.model import Model
    c = fused_case("mini-1b")
    prompt = c["prompt"]
    with env(LLMI_NO_PREFILL=1):
        m = Model(c["g"], max_ctx=512)
        assert m.get_info().score_path == 2
        r = m.score(prompt)
        assert m.time_kernel(9, 2) == (0.0, 0.0)
        margins = []
        for i in range(len(prompt)):  # the row path's own logits: the token loop's
            lg = np.sort(m.forward(prompt[:i + 1], 0))
            margins.append(float(lg[-1] - lg[-2]))
        m.close()
    f = c["tap"]
    d_lp, d_lse = np.abs(r.logprobs - f.logprobs).max(), np.abs(r.lse - f.lse).max()
    print(f"row path vs fused path: max |dlogprob| {d_lp:.3g}, |dlse| {d_lse:.3g} (bound {2 * FAST_VS_REF})")
    assert d_lp <= 2 * FAST_VS_REF and d_lse <= 2 * FAST_VS_REF
    decided = np.array(margins) > 2 * FAST_VS_REF
    np.testing.assert_array_equal(r.argmax[decided], f.argmax[decided])


def test_row_path_q8_0_table():
    """A Q8_0 output table takes the row path with or without the batched prefill; its results are the f64 reduction
    of forward's own logits per prefix (the token loop on both sides) within eps_t."""
    from llm_inference_amd.gguf import TensorType as TT
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg = CONFIGS["mini-1b"]
    g = build_gemma3_gguf(cfg, seed=21, embd_type=TT.Q8_0)
    prompt = np.random.default_rng(3).integers(4, cfg.vocab, 40).astype(np.int32)
    tg = np.concatenate([prompt[1:], [-1]]).astype(np.int32)
    with env():
        m = Model(g, max_ctx=512)
        assert m.get_info().score_path == 2
        m.close()
    with env(LLMI_NO_PREFILL=1):
        m = Model(g, max_ctx=512)
        assert m.get_info().score_path == 2
        r = m.score(prompt)
        worst = 0.0
        for i in (0, 7, len(prompt) - 1):
            ref = logits_scores(m.forward(prompt[:i + 1], 0).astype(np.float64)[None, :], tg[i:i + 1])
            e = max(abs(float(r.lse[i]) - ref["lse"][0]), abs(float(r.logprobs[i]) - ref["logprob"][0]))
            worst = max(worst, e / ref["eps"][0])
            assert e <= ref["eps"][0], (i, e, ref["eps"][0])
            assert r.argmax[i] == ref["argmax"][0]
        m.close()
    print(f"Q8_0 table, row path: worst error / eps_t {worst:.3g}")


# ---------------------------------------------------------------------------
# 4. exact session vs the oracle
# ---------------------------------------------------------------------------
def test_exact_session_vs_oracle(oracle):
    """Model(exact=True) scores on the row path; its logits at every position are the reference's bits, so argmax is
    the reference's greedy id and lse / logprob are within eps_t of f64 from the oracle's logits."""
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg = CONFIGS["tiny"]
    g = build_gemma3_gguf(cfg, seed=7, swa_pattern=[True, False, True])
    prompt = np.random.default_rng(3).integers(4, cfg.vocab, 12).astype(np.int32)
    tg = np.concatenate([prompt[1:], [-1]]).astype(np.int32)
    with env():
        m = Model(g, exact=True, max_ctx=64)
        assert m.get_info().score_path == 2
        r = m.score(prompt)
        m.close()
    worst = 0.0
    om = oracle.model(g, n_threads=4, max_ctx=64)
    for i in range(len(prompt)):
        lo = om.forward(prompt[:i + 1], 0)
        ref = logits_scores(lo.astype(np.float64)[None, :], tg[i:i + 1])
        assert r.argmax[i] == int(np.argmax(lo)), i
        e = max(abs(float(r.lse[i]) - ref["lse"][0]), abs(float(r.logprobs[i]) - ref["logprob"][0]))
        worst = max(worst, e / ref["eps"][0])
        assert e <= ref["eps"][0], (i, e, ref["eps"][0])
    print(f"exact session vs oracle: worst error / eps_t {worst:.3g}")


# ---------------------------------------------------------------------------
# 5. errors
# ---------------------------------------------------------------------------
def test_score_argument_errors():
    from llm_inference_amd._lib import LLMIError
    from llm_inference_amd.model import Model, TPGroup
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg = CONFIGS["mini-1b"]
    g = build_gemma3_gguf(cfg, seed=21)
    with env():
        m = Model(g, max_ctx=64)
        with pytest.raises(LLMIError) as ei:
            m.score([5, 6, 7], 0, [6, cfg.vocab, -1])
        assert ei.value.status == "E_RANGE" and "targets" in str(ei.value)
        with pytest.raises(LLMIError) as ei:
            m.score([5, 6, 7], 0, [6, -2, -1])
        assert ei.value.status == "E_RANGE" and "targets" in str(ei.value)
        with pytest.raises(LLMIError) as ei:
            m.score([5, cfg.vocab], 0)
        assert ei.value.status == "E_RANGE" and "tokens" in str(ei.value)
        with pytest.raises(LLMIError) as ei:
            m.score(np.zeros(0, np.int32), 0)
        assert ei.value.status == "E_ARG" and "n_tokens" in str(ei.value)
        with pytest.raises(LLMIError) as ei:
            m.score([5] * 10, 60)
        assert ei.value.status == "E_RANGE" and "context overflow" in str(ei.value)
        assert m.score([5, 6, 7], 0).count == 2  # and the session still works
        m.close()
        # a tensor-parallel session refuses (every rank, before any exchange)
        grp = TPGroup(2)
        got = [None, None]

        def rank(r):
            try:
                mr = Model(g, max_ctx=64, tp_rank=r, tp_size=2, tp_group=grp)
                assert mr.get_info().score_path == 0
                try:
                    mr.score([5, 6, 7], 0)
                except LLMIError as e:
                    got[r] = (e.status, str(e))
                mr.close()
            except Exception as e:  # noqa: BLE001 -- reported below
                got[r] = ("unexpected", repr(e))

        th = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join(300)
        grp.close()
    for st in got:
        assert st is not None and st[0] == "E_ARG" and "tensor-parallel" in st[1], got
