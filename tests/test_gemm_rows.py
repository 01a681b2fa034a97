"""The skinny f16 x Q4_0 GEMM (k_gemm_rows.hip): against float64, bit for bit against the tiled
kernel v6 whose launches it takes, inside the session's batch step, and its argument errors."""
import functools
import os

import numpy as np
import pytest

from oplevel import PREFILL16_RTOL, dequant_q4_0, rel_err

pytestmark = pytest.mark.gpu
# (rows, K): WK = 2 with one block per K group pair; nb = 36, no multiple of 8; nb = 160, the first WK = 4; a row-tile
# count that is no power of two
SHAPES = [(64, 128), (128, 1152), (64, 5120), (192, 2560)]
TS = [1, 2, 31, 32, 33, 64]
SENTINEL = np.float32(-1234.5)


@functools.lru_cache(maxsize=None)
def case(rows, K, T, scales="positive"):
    """Weights (GGUF blocks), their float64 values, the f16 inputs and power-of-two token scales: read-only."""
    from llm_inference_amd.gguf import TensorType as TT
    from llm_inference_amd.synthetic import random_tensor
    w = random_tensor(TT.Q4_0, rows, K, seed=rows + K, centered=True, scales=scales)
    rng = np.random.default_rng(T * 7919 + K)
    x = rng.standard_normal((T, K)).astype(np.float16)
    ts = (2.0 ** rng.integers(-3, 4, T)).astype(np.float32)
    return w, dequant_q4_0((w, TT.Q4_0, rows, K)), x, ts


def run(rows, K, T, kernel, slab, scaled, scales="positive"):
    """[T + 1][rows + 5] pre-filled with the sentinel; the launch gets the first T rows."""
    from llm_inference_amd import ops
    w, _, x, ts = case(rows, K, T, scales)
    out = np.full((T + 1, rows + 5), SENTINEL, np.float32)
    out[:T] = ops.gemm_rows(w, rows, K, x, ts if scaled else None, kernel=kernel, slab=slab, out=out[:T])
    return out


def variants(K):
    return [(slab, scaled) for slab in ((False, True) if (K // 32) % 8 == 0 else (False,)) for scaled in (False, True)]


def check_f64(rows, K, T, scales="positive"):
    _, W, x, ts = case(rows, K, T, scales)
    for slab, scaled in variants(K):
        ref = (x.astype(np.float64) * (ts[:, None] if scaled else 1.0)) @ W.T
        out = run(rows, K, T, "skinny", slab, scaled, scales)
        for t in range(T):
            err = rel_err(out[t, :rows], ref[t])
            assert err <= PREFILL16_RTOL, f"slab {slab} tscale {scaled} row {t}: relative error {err:.3g}"


def check_bits(rows, K, T, scales="positive"):
    for slab, scaled in variants(K):
        sk, tl = (run(rows, K, T, k, slab, scaled, scales) for k in ("skinny", "tiled"))
        np.testing.assert_array_equal(sk.view(np.uint32), tl.view(np.uint32), err_msg=f"slab {slab} tscale {scaled}")
        assert np.all(sk[:, rows:] == SENTINEL) and np.all(sk[T:] == SENTINEL), "wrote past the outputs"
        assert not np.any(sk[:T, :rows] == SENTINEL)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("rows,K", SHAPES)
def test_skinny_against_f64(rows, K, T):
    check_f64(rows, K, T)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("rows,K", SHAPES)
def test_skinny_bits_equal_tiled(rows, K, T):
    check_bits(rows, K, T)


def test_edge_block_scales():
    """Signed, zero, subnormal and smallest-normal d, blocks of all-0 and all-15 nibbles."""
    check_f64(192, 2560, 33, "edge")
    check_bits(192, 2560, 33, "edge")


def test_session_batch_step():
    """mini-4b, batch_forward of 5 rows: the default (skinny) against LLMI_PG_SKINNY=0 (the tiled launches), the plan
    for the model's projection shapes, time_kernel(15)."""
    from llm_inference_amd import ops
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg = CONFIGS["mini-4b"]
    pos, slots = (0, 31, 32, 127, 129), (3, 0, 4, 1, 2)
    rng = np.random.default_rng(11)
    prompts = [rng.integers(4, cfg.vocab, p + 1).astype(np.int32) for p in pos]
    shapes = [((cfg.n_head + 2 * cfg.n_head_kv) * cfg.head_dim, cfg.n_embd), (cfg.n_embd, cfg.n_head * cfg.head_dim),
              (2 * cfg.n_ff, cfg.n_embd), (cfg.n_embd, cfg.n_ff)]
    old = os.environ.pop("LLMI_PG_SKINNY", None)
    try:
        assert [ops.gemm_rows_plan(r, k, 5) for r, k in shapes] == [1, 1, 1, 1]
        assert all(ops.gemm_rows_plan(r, k, 128) in (6, 7) for r, k in shapes)
        m = Model(build_gemma3_gguf(cfg, seed=21), max_ctx=512)
        m.reserve_sequences(5)
        assert m.time_kernel(15, 2) == (0.0, 0.0)
        for i in sorted(range(5), key=lambda i: slots[i] == 0):
            if pos[i]:
                m.forward(prompts[i][:-1], 0, want_logits=False)
                m.copy_sequence(slots[i], 0, pos[i])
        rows = ([int(p[-1]) for p in prompts], list(slots), list(pos))
        got = m.batch_forward(*rows, want_logits=True)
        us, by = m.time_kernel(15, 2)
        os.environ["LLMI_PG_SKINNY"] = "0"
        assert [ops.gemm_rows_plan(r, k, 5) for r, k in shapes] == [6, 6, 6, 6]
        ref = m.batch_forward(*rows, want_logits=True)
        m.close()
    finally:
        os.environ.pop("LLMI_PG_SKINNY", None)
        if old is not None:
            os.environ["LLMI_PG_SKINNY"] = old
    np.testing.assert_array_equal(got.logits.view(np.uint32), ref.logits.view(np.uint32))
    np.testing.assert_array_equal(got.argmax, ref.argmax)
    np.testing.assert_array_equal(np.asarray(got.lse, np.float32).view(np.uint32), np.asarray(ref.lse, np.float32).view(np.uint32))
    print(f"time_kernel(15): {us:.1f} us per layer for {by:.0f} bytes")
    assert us > 0 and by == sum(r * (k // 32) * 18 for r, k in shapes)


def test_argument_errors():
    from llm_inference_amd import ops
    from llm_inference_amd._lib import LLMIError
    w, _, x, _ = case(64, 128, 2)

    def raises(status, word, *a, **k):
        with pytest.raises(LLMIError) as ei:
            ops.gemm_rows(*a, **k)
        assert ei.value.status == status and word in str(ei.value), (ei.value.status, str(ei.value))

    raises("E_RANGE", "(T)", w, 64, 128, np.zeros((513, 128), np.float16))
    raises("E_RANGE", "(T)", w, 64, 128, np.zeros((65, 128), np.float16), kernel="skinny")
    raises("E_SIZE", "n_rows", w[: 32 * 4 * 18], 32, 128, x)
    raises("E_SIZE", "n_cols", w[: 64 * 3 * 18], 64, 96, x[:, :96])
    raises("E_SIZE", "slab", w, 64, 128, x, slab=True)
    raises("E_SIZE", "ostride", w, 64, 128, x, out=np.zeros((2, 63), np.float32))
    assert ops.gemm_rows_plan(32, 128, 4) == 0 and ops.gemm_rows_plan(64, 96, 4) == 0
