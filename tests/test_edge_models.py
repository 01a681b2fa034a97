"""The exact-order engine and one batch step on models whose block scales are signed, zero and subnormal
(build_gemma3_gguf(scales=...), llm_inference_amd/synthetic.py SCALE_PROFILES).  The positive-scale versions of these
comparisons are tests/test_exact_q8.py, tests/test_exact_kq.py and tests/test_batch_decode.py; the oracle is pinned to
the reference on such scales by tests/test_edge_scales.py.  Everything is compared on the logits' bits.
"""
import functools

import numpy as np
import pytest

from test_batch_decode import env, load_prefixes, rows_of, u32

pytestmark = pytest.mark.gpu
N_PROMPT, N_DECODE, CTX = 40, 3, 128


def _kinds():
    from llm_inference_amd.gguf import TensorType as TT
    return {"mini-1b-q8_0": ("mini-1b", dict(wtype=TT.Q8_0), False),
            "mini-4b-q4_0": ("mini-4b", dict(wtype=TT.Q4_0), False),
            "mini-4b-q4_k_m": ("mini-4b", dict(wtype=TT.Q4_K, wtypes={"v": TT.Q6_K, "down": TT.Q6_K}), True)}


@functools.lru_cache(maxsize=None)
def _gguf(kind, scales):
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg_name, kw, _kq = _kinds()[kind]
    return build_gemma3_gguf(CONFIGS[cfg_name], seed=61, scales=scales, **kw)


@pytest.mark.parametrize("kind", ["mini-1b-q8_0", "mini-4b-q4_0", "mini-4b-q4_k_m"])
def test_exact_engine_matches_oracle_on_edge_scales(oracle, kind):
    """Model(exact=True) (exact_kq=True for the K-quant mix) on a scales="edge" file: the batched exact prompt's
    logits of a 40-token prompt and three teacher-forced decode steps of the exact-order engine carry the oracle's
    bits."""
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS
    cfg_name, _kw, kq = _kinds()[kind]
    g = _gguf(kind, "edge")
    rng = np.random.default_rng(62)
    V = CONFIGS[cfg_name].vocab
    prompt = np.concatenate([[2], rng.integers(4, V, N_PROMPT - 1)]).astype(np.int32)
    forced = rng.integers(4, V, N_DECODE).astype(np.int32)
    om = oracle.model(g, n_threads=8, max_ctx=CTX)
    want = [om.forward(prompt, 0)] + [om.forward([int(t)], N_PROMPT + i) for i, t in enumerate(forced)]
    with env():
        m = Model(g, exact=True, max_ctx=CTX, exact_kq=kq)
        info = m.get_info()
        got = [m.forward(prompt, 0)] + [m.forward(np.array([t], np.int32), N_PROMPT + i) for i, t in enumerate(forced)]
        m.close()
    assert info.exact_engine == 1 and info.exact_batched_prefill == 1
    want, got = np.stack(want), np.stack(got)
    assert np.isfinite(want).all() and np.ptp(want[0]) > 0
    print(f"{kind}: max |device - oracle| per row {np.abs(got - want).max(1).tolist()}")
    np.testing.assert_array_equal(u32(got), u32(want))


def test_batch_step_rows_equal_single_sequence_bits_on_signed_scales():
    """One batch_forward of 3 slots at positions (0, 31, 33) -- each side of a 32-key tile -- on a scales="signed"
    mini-4b: each row's logits carry the bits of forward() of that sequence alone on a session that never reserved
    a slot."""
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS
    g = _gguf("mini-4b-q4_0", "signed")
    rng = np.random.default_rng(63)
    prompts = [rng.integers(4, CONFIGS["mini-4b"].vocab, p + 1).astype(np.int32) for p in (0, 31, 33)]
    slots = (2, 0, 1)
    with env():
        ref = Model(g, max_ctx=CTX)
        want = np.stack([ref.forward(x, 0) for x in prompts])
        ref.close()
        m = Model(g, max_ctx=CTX)
        m.reserve_sequences(3)
        load_prefixes(m, prompts, slots)
        got = m.batch_forward(*rows_of(prompts, slots, [0, 1, 2]), want_logits=True)
        m.close()
    assert np.isfinite(want).all()
    np.testing.assert_array_equal(got.argmax, want.argmax(1))
    np.testing.assert_array_equal(u32(got.logits), u32(want))
