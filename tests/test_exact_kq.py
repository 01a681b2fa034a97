"""The exact-order engine on K-quant layers, opt-in (LLMI_EXACT_KQ; k_exact.hip: the K-quant streaming layouts,
exact_gemv_kq_kernel, xp_gemm_kq_kernel).  The reference's Q4_K row (ops.cpp:614-700) is one chain of plain fp32 adds
over the sub-blocks' t = fmaf((float)a, d sc, -((dmin m) (float)bs)), its Q6_K row (ops.cpp:702-785) one fma chain over
the 128-element halves' (float)part, on quantize_row_q8_k's activation; the engine computes the t / part in parallel
and keeps the chains, so everything here is compared on the logits' BITS (.view(np.uint32)), without tolerances:
against the oracle (pinned to the reference's bits by tests/test_oracle_golden.py), against the per-op exact kernels
(LLMI_EXACT_XL=0, pinned to the oracle by tests/test_hip_model.py) and against the token loop (LLMI_XP_OFF=1).

Three shapes, one per input-width class of the decode launches (n <= 1536, <= 3072, <= 6144), two layers each so
layer 1's q|k|v launch runs the residual / norm prologue; odd and even super-block counts (kq-small 6 and 12,
mini-4b 10, 8 and 40, kq-wide 21, 16 and 11), so the chunks' tails are exercised.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _cfg(name):
    from llm_inference_amd.synthetic import CONFIGS, Gemma3Config
    if name == "kq-small":
        return Gemma3Config("kq-small", 2, 1536, 3072, 4, 1, 256, 512)
    if name == "kq-wide":
        return Gemma3Config("kq-wide", 2, 5376, 2816, 32, 16, 128, 512)
    return CONFIGS[name]


def _tt():
    from llm_inference_amd.gguf import TensorType
    return TensorType


def _mix(kind):
    """(wtype, wtypes) of a named mix"""
    TT = _tt()
    return {
        "q4_k_m": (TT.Q4_K, {"v": TT.Q6_K, "down": TT.Q6_K}),
        "q4_k": (TT.Q4_K, None),
        "o-down-q6": (TT.Q4_K, {"o": TT.Q6_K, "down": TT.Q6_K}),
        "o-q4_0": (TT.Q4_K, {"v": TT.Q6_K, "down": TT.Q6_K, "o": TT.Q4_0}),
        "up-q6": (TT.Q4_K, {"up": TT.Q6_K}),
        "gate-up-q6": (TT.Q4_K, {"gate": TT.Q6_K, "up": TT.Q6_K}),
        "k-q4_0": (TT.Q4_K, {"k": TT.Q4_0}),
    }[kind]


@functools.lru_cache(maxsize=None)
def _gguf(name, seed, kind="q4_k_m"):
    from llm_inference_amd.synthetic import build_gemma3_gguf
    wtype, wtypes = _mix(kind)
    return build_gemma3_gguf(_cfg(name), seed=seed, wtype=wtype, wtypes=wtypes)


def _same_bits(got, want, msg=""):
    np.testing.assert_array_equal(np.asarray(got).view(np.uint32), np.asarray(want).view(np.uint32), err_msg=msg)


def _session(g, monkeypatch, env, max_ctx, engine=None, batched=None, exact_kq=True):
    from llm_inference_amd.model import Model
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = Model(g, exact=True, max_ctx=max_ctx, exact_kq=exact_kq)
    info = m.get_info()
    if engine is not None:
        assert info.exact_engine == engine
    if batched is not None:
        assert info.exact_batched_prefill == batched
    return m


def _run(g, prompt, forced, n_gen, monkeypatch, env, **want):
    """forward(prompt), teacher-forced single tokens, then n_gen free-running ids; the env removed afterwards"""
    m = _session(g, monkeypatch, env, len(prompt) + len(forced) + n_gen + 8, **want)
    out = [m.forward(prompt, 0)]
    for i, t in enumerate(forced):
        out.append(m.forward(np.array([t], np.int32), len(prompt) + i))
    ids = m.generate(int(np.argmax(out[-1])), len(prompt) + len(forced), n_gen).tolist()
    m.close()
    for k in env:
        monkeypatch.delenv(k)
    return np.stack(out), ids


# ---- 1. engine selection ----------------------------------------------------------------------------------------
def _info(g, monkeypatch, env, exact_kq):
    m = _session(g, monkeypatch, env, 32, exact_kq=exact_kq)
    info = m.get_info()
    m.close()
    for k in env:
        monkeypatch.delenv(k)
    return info.exact_engine, info.exact_batched_prefill


def test_flag_selects_the_engine(monkeypatch):
    assert _info(_gguf("mini-4b", 11), monkeypatch, {}, True) == (1, 1)


def test_environment_selects_the_engine(monkeypatch):
    assert _info(_gguf("mini-4b", 11), monkeypatch, {"LLMI_EXACT_KQ": "1"}, False) == (1, 1)


def test_default_session_stays_per_op(monkeypatch):
    assert _info(_gguf("mini-4b", 11), monkeypatch, {}, False)[0] == 0
    assert _info(_gguf("mini-4b", 11), monkeypatch, {"LLMI_EXACT_KQ": "0"}, False)[0] == 0


def test_exact_xl_0_keeps_the_per_op_kernels(monkeypatch):
    assert _info(_gguf("mini-4b", 11), monkeypatch, {"LLMI_EXACT_XL": "0"}, True)[0] == 0


def test_flag_needs_exact_mode():
    """LLMI_EXACT_KQ is meaningful only with LLMI_EXACT: a fast session is what it was"""
    from llm_inference_amd.model import Model
    m = Model(_gguf("mini-4b", 11), exact=False, max_ctx=32, exact_kq=True)
    info = m.get_info()
    m.close()
    assert info.exact_engine == 0


@pytest.mark.parametrize("kind", ["up-q6", "k-q4_0", "gate-up-q6"])
def test_refused_mixes_stay_per_op(oracle, monkeypatch, kind):
    """gate and up of different types, q|k|v across the two families, and gate and up both Q6_K (the GELU role has
    the Q4_K row body only) are turned away with the flag set; the logits are the oracle's either way."""
    cfg = _cfg("kq-small")
    g = _gguf("kq-small", 13, kind)
    prompt = np.random.default_rng(14).integers(4, cfg.vocab, 7).astype(np.int32)
    om = oracle.model(g, n_threads=8, max_ctx=32)
    ref = [om.forward(prompt, 0), om.forward([5], len(prompt))]
    m = _session(g, monkeypatch, {}, 32, engine=0)
    got = [m.forward(prompt, 0), m.forward(np.array([5], np.int32), len(prompt))]
    m.close()
    _same_bits(np.stack(got), np.stack(ref))


# ---- 2. against the oracle ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_run(oracle, name, kind):
    cfg = _cfg(name)
    rng = np.random.default_rng(21)
    prompt = np.concatenate([[2], rng.integers(4, cfg.vocab, 8)]).astype(np.int32)
    forced = rng.integers(4, cfg.vocab, 3).astype(np.int32)
    om = oracle.model(_gguf(name, 20, kind), n_threads=8, max_ctx=64)
    rows = [om.forward(prompt, 0)]
    for i, t in enumerate(forced):
        rows.append(om.forward([int(t)], len(prompt) + i))
    ids, pos, tok = [], len(prompt) + len(forced), int(np.argmax(rows[-1]))
    for _ in range(8):
        tok = int(np.argmax(om.forward([tok], pos)))
        ids.append(tok)
        pos += 1
    return prompt, forced, np.stack(rows), ids


@pytest.mark.parametrize("batched", [False, True], ids=["decode-kernels", "batched-prompt"])
@pytest.mark.parametrize("name", ["kq-small", "mini-4b"])
def test_engine_matches_oracle(oracle, monkeypatch, name, batched):
    prompt, forced, want, ids_want = _oracle_run(oracle, name, "q4_k_m")
    env = {} if batched else {"LLMI_XP_OFF": "1"}
    got, ids = _run(_gguf(name, 20), prompt, forced, 8, monkeypatch, env, engine=1, batched=int(batched))
    print(f"{name} batched={batched}: max |device - oracle| per row {np.abs(got - want).max(1).tolist()}")
    _same_bits(got, want)
    assert ids == ids_want


# ---- 3. the engine against the per-op exact kernels ----------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("kq-small", "q4_k_m"), ("mini-4b", "q4_k_m"), ("kq-wide", "q4_k_m"),
                                       ("kq-wide", "q4_k"), ("kq-small", "o-down-q6")])
def test_engine_matches_per_op_kernels(monkeypatch, name, kind):
    cfg = _cfg(name)
    rng = np.random.default_rng(31)
    prompt = np.concatenate([[2], rng.integers(4, cfg.vocab, 4)]).astype(np.int32)
    forced = rng.integers(4, cfg.vocab, 2).astype(np.int32)
    g = _gguf(name, 30, kind)
    want, ids_want = _run(g, prompt, forced, 4, monkeypatch, {"LLMI_EXACT_XL": "0"}, engine=0)
    got, ids = _run(g, prompt, forced, 4, monkeypatch, {}, engine=1)
    print(f"{name} {kind}: max |engine - per-op| per row {np.abs(got - want).max(1).tolist()}")
    _same_bits(got, want)
    assert ids == ids_want


# ---- 4. the two families in one layer ---------------------------------------------------------------------------
@pytest.mark.parametrize("batched", [False, True], ids=["decode-kernels", "batched-prompt"])
def test_mixed_families(oracle, monkeypatch, batched):
    """Q4_K_M with a Q4_0 o projection: the attention launch's Q8_0 blocks feed o, every other launch takes Q8_K"""
    prompt, forced, want, ids_want = _oracle_run(oracle, "mini-4b", "o-q4_0")
    env = {} if batched else {"LLMI_XP_OFF": "1"}
    got, ids = _run(_gguf("mini-4b", 20, "o-q4_0"), prompt, forced, 8, monkeypatch, env, engine=1, batched=int(batched))
    _same_bits(got, want)
    assert ids == ids_want


# ---- 5. the batched prompt against the token loop ---------------------------------------------------------------
@pytest.mark.parametrize("name,n,chunk", [("kq-small", 130, "7"), ("mini-4b", 70, None), ("kq-wide", 37, "16")])
def test_batched_prompt_matches_token_loop(monkeypatch, name, n, chunk):
    cfg = _cfg(name)
    rng = np.random.default_rng(n)
    prompt = np.concatenate([[2], rng.integers(4, cfg.vocab, n - 1)]).astype(np.int32)
    forced = rng.integers(4, cfg.vocab, 3).astype(np.int32)
    g = _gguf(name, 40)
    want, ids_want = _run(g, prompt, forced, 4, monkeypatch, {"LLMI_XP_OFF": "1"}, engine=1, batched=0)
    got, ids = _run(g, prompt, forced, 4, monkeypatch, {"LLMI_XP_CHUNK": chunk} if chunk else {}, engine=1, batched=1)
    print(f"{name} n={n} chunk={chunk}: max |batched - token loop| per row {np.abs(got - want).max(1).tolist()}")
    _same_bits(got, want)
    assert ids == ids_want


# ---- 6. state ----------------------------------------------------------------------------------------------------
def test_prompt_again_at_position_0(monkeypatch):
    cfg = _cfg("kq-small")
    prompt = np.concatenate([[2], np.random.default_rng(51).integers(4, cfg.vocab, 10)]).astype(np.int32)
    m = _session(_gguf("kq-small", 50), monkeypatch, {}, 64, engine=1, batched=1)
    first = m.forward(prompt, 0)
    tok = int(np.argmax(first))
    for i in range(4):
        tok = int(np.argmax(m.forward(np.array([tok], np.int32), len(prompt) + i)))
    again = m.forward(prompt, 0)
    m.close()
    _same_bits(again, first)
