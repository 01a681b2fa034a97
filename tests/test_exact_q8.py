"""The exact-order engine on Q8_0 layers (k_exact.hip: the Q8_0 streaming layout, exact_gemv_kernel's Q8_0 rows,
xp_gemm_q8_kernel).  The reference's Q8_0 row (ops.cpp:806-824) is one fp32 chain over the row's blocks in order,
sum = fmaf((float)dot * f16(w.d), f16(x.d), sum); the engine computes the products in parallel and keeps the chain,
so everything here is compared on the logits' BITS (.view(np.uint32)), without tolerances: against the oracle
(pinned to the reference's bits by tests/test_oracle_golden.py), against the per-op exact kernels (LLMI_EXACT_XL=0,
pinned to the oracle by tests/test_hip_model.py) and against the token loop (LLMI_XP_OFF=1).

Three shapes, one per input-width class of the decode launches (n <= 1536, <= 3072, <= 6144), two layers each so
layer 1's q|k|v launch runs the residual / norm prologue.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _cfg(name):
    from llm_inference_amd.synthetic import CONFIGS, Gemma3Config
    if name == "q8-wide":  # the E > 3072 class at head_dim 128, about a quarter of mini-27b's weight bytes
        return Gemma3Config("q8-wide", 2, 5376, 2688, 32, 16, 128, 512)
    return CONFIGS[name]


@functools.lru_cache(maxsize=None)
def _gguf(name, seed):
    from llm_inference_amd.gguf import TensorType
    from llm_inference_amd.synthetic import build_gemma3_gguf
    return build_gemma3_gguf(_cfg(name), seed=seed, wtype=TensorType.Q8_0)


def _same_bits(got, want, msg=""):
    np.testing.assert_array_equal(np.asarray(got).view(np.uint32), np.asarray(want).view(np.uint32), err_msg=msg)


def _session(g, monkeypatch, env, max_ctx, engine=None, batched=None):
    from llm_inference_amd.model import Model
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = Model(g, exact=True, max_ctx=max_ctx)
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
def test_q8_0_session_runs_on_the_engine():
    from llm_inference_amd.model import Model
    m = Model(_gguf("mini-1b", 11), exact=True, max_ctx=32)
    info = m.get_info()
    m.close()
    assert info.exact_engine == 1
    assert info.exact_batched_prefill == 1


def test_k_quant_session_stays_per_op():
    from llm_inference_amd.gguf import TensorType
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import build_gemma3_gguf
    # (mini-4b: Q4_K rows are whole 256-element super-blocks, which mini-1b's 1152 columns are not)
    m = Model(build_gemma3_gguf(_cfg("mini-4b"), seed=12, wtype=TensorType.Q4_K), exact=True, max_ctx=32)
    info = m.get_info()
    m.close()
    assert info.exact_engine == 0


@pytest.mark.parametrize("part,engine", [("v", 0), ("down", 1)])
def test_mixed_types(oracle, part, engine):
    """Q4_0 with one Q8_0 projection: inside the q|k|v concatenation (one XL weight, one type) the engine is
    refused; a whole projection of the other type runs on it.  Either way the logits are the oracle's."""
    from llm_inference_amd.gguf import TensorType
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import build_gemma3_gguf
    cfg = _cfg("mini-1b")
    g = build_gemma3_gguf(cfg, seed=13, wtypes={part: TensorType.Q8_0})
    prompt = np.random.default_rng(14).integers(4, cfg.vocab, 7).astype(np.int32)
    om = oracle.model(g, n_threads=8, max_ctx=32)
    ref = [om.forward(prompt, 0), om.forward([5], len(prompt))]
    m = Model(g, exact=True, max_ctx=32)
    assert m.get_info().exact_engine == engine
    got = [m.forward(prompt, 0), m.forward(np.array([5], np.int32), len(prompt))]
    m.close()
    _same_bits(np.stack(got), np.stack(ref))


def test_tensor_parallel_q8_0_refused():
    from llm_inference_amd._lib import LLMIError
    from llm_inference_amd.model import Model, TPGroup
    grp = TPGroup(2)
    with pytest.raises(LLMIError) as ei:
        Model(_gguf("mini-1b", 11), exact=True, max_ctx=32, tp_rank=0, tp_size=2, tp_group=grp)
    grp.close()
    assert ei.value.status == "E_ARG"


# ---- 2. against the oracle ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_run(oracle, name):
    cfg = _cfg(name)
    rng = np.random.default_rng(21)
    prompt = np.concatenate([[2], rng.integers(4, cfg.vocab, 8)]).astype(np.int32)
    forced = rng.integers(4, cfg.vocab, 3).astype(np.int32)
    om = oracle.model(_gguf(name, 20), n_threads=8, max_ctx=64)
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
@pytest.mark.parametrize("name", ["mini-1b", "mini-4b"])
def test_engine_matches_oracle(oracle, monkeypatch, name, batched):
    prompt, forced, want, ids_want = _oracle_run(oracle, name)
    env = {} if batched else {"LLMI_XP_OFF": "1"}
    got, ids = _run(_gguf(name, 20), prompt, forced, 8, monkeypatch, env, engine=1, batched=int(batched))
    print(f"{name} batched={batched}: max |device - oracle| per row {np.abs(got - want).max(1).tolist()}")
    _same_bits(got, want)
    assert ids == ids_want


# ---- 3. the engine against the per-op exact kernels ----------------------------------------------------------
@pytest.mark.parametrize("name", ["mini-1b", "mini-4b", "q8-wide"])
def test_engine_matches_per_op_kernels(monkeypatch, name):
    cfg = _cfg(name)
    rng = np.random.default_rng(31)
    prompt = np.concatenate([[2], rng.integers(4, cfg.vocab, 4)]).astype(np.int32)
    forced = rng.integers(4, cfg.vocab, 2).astype(np.int32)
    g = _gguf(name, 30)
    want, ids_want = _run(g, prompt, forced, 4, monkeypatch, {"LLMI_EXACT_XL": "0"}, engine=0)
    got, ids = _run(g, prompt, forced, 4, monkeypatch, {}, engine=1)
    print(f"{name}: max |engine - per-op| per row {np.abs(got - want).max(1).tolist()}")
    _same_bits(got, want)
    assert ids == ids_want


# ---- 4. the batched prompt against the token loop ---------------------------------------------------------------
@pytest.mark.parametrize("name,n,chunk", [("mini-1b", 130, "7"), ("mini-4b", 70, None), ("q8-wide", 37, "16")])
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


# ---- 5. state ----------------------------------------------------------------------------------------------------
def test_prompt_again_at_position_0(monkeypatch):
    cfg = _cfg("mini-1b")
    prompt = np.concatenate([[2], np.random.default_rng(51).integers(4, cfg.vocab, 10)]).astype(np.int32)
    m = _session(_gguf("mini-1b", 50), monkeypatch, {}, 64, engine=1, batched=1)
    first = m.forward(prompt, 0)
    tok = int(np.argmax(first))
    for i in range(4):
        tok = int(np.argmax(m.forward(np.array([tok], np.int32), len(prompt) + i)))
    again = m.forward(prompt, 0)
    m.close()
    _same_bits(again, first)
