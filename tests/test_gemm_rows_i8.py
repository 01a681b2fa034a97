"""The skinny int8 GEMM (k_gemm_rows.hip): against float64, bit for bit against the tiled kernel
v5 whose launches it takes, on edge block scales, inside a Q8_0 session's batch step, and its argument errors."""
import functools
import os

import numpy as np
import pytest

from oplevel import GEMV_RTOL, rel_err

pytestmark = pytest.mark.gpu
Q8_0, Q4_0 = 8, 2
# (rows, K): nb = 4, WK = 2, one block pair per group; nb = 36, a ragged stage tail, rows no multiple of 64; nb = 160,
# the first WK = 4; nb = 80
SHAPES = [(64, 128), (96, 1152), (32, 5120), (160, 2560)]
TS = [1, 2, 7, 8, 31, 32]
SENTINEL = np.float32(-1234.5)


@functools.lru_cache(maxsize=None)
def case(wtype, rows, K, T, scales="positive"):
    """Weights (GGUF blocks), float32 inputs and the float64 reference sum_b d_w d_x isum_b: read-only.  "edge":
    signed, zero and subnormal weight scales; inputs with a zero row, zero blocks and blocks whose Q8_0 scale
    amax / 127 is an f16 subnormal."""
    from llm_inference_amd.synthetic import random_tensor
    w = random_tensor(wtype, rows, K, seed=rows + K, centered=True, scales=scales)
    rng = np.random.default_rng(T * 7919 + K)
    x = rng.standard_normal((T, K // 32, 32)).astype(np.float32)
    if scales == "edge":
        x *= np.float32(2.0) ** rng.integers(-14, 1, (T, K // 32, 1)).astype(np.float32)
        x[rng.integers(0, 5, (T, K // 32)) == 0] = 0.0
        x[T // 2] = 0.0
    # quantize_row_q8_0: d = amax / 127, id = 1 / d from the unrounded d, q = the nearest integer of the exact x id
    d = np.abs(x).max(-1) / np.float32(127.0)
    inv = np.divide(np.float32(1.0), d, out=np.zeros_like(d), where=d != 0)
    xq = np.rint(x.astype(np.float64) * inv[..., None].astype(np.float64))
    dx = d.astype(np.float16).astype(np.float64)
    blk = w.reshape(rows, K // 32, -1)
    dw = blk[..., :2].copy().view(np.float16)[..., 0].astype(np.float64)
    if wtype == Q8_0:
        wq = blk[..., 2:].view(np.int8).astype(np.float64)
    else:
        wq = np.concatenate([blk[..., 2:] & 15, blk[..., 2:] >> 4], -1).astype(np.float64) - 8.0
    ref = np.einsum("nb,tb,nbk,tbk->tn", dw, dx, wq, xq)
    return w, x.reshape(T, K), ref


def run(wtype, rows, K, T, kernel, slab, scales="positive"):
    """[T + 1][rows + 5] pre-filled with the sentinel; the launch gets the first T rows."""
    from llm_inference_amd import ops
    w, x, _ = case(wtype, rows, K, T, scales)
    out = np.full((T + 1, rows + 5), SENTINEL, np.float32)
    out[:T] = ops.gemm_rows_i8(w, wtype, rows, K, x, kernel=kernel, slab=slab, out=out[:T])
    return out


def slabs(wtype, K):
    return (False, True) if wtype == Q4_0 and (K // 32) % 8 == 0 else (False,)


def check_f64(wtype, rows, K, T, scales="positive"):
    ref = case(wtype, rows, K, T, scales)[2]
    for slab in slabs(wtype, K):
        out = run(wtype, rows, K, T, "skinny", slab, scales)
        errs = [rel_err(out[t, :rows], ref[t]) for t in range(T) if np.any(ref[t])]
        print(f"wtype {wtype} slab {slab}: largest relative error {max(errs):.3g}")
        assert max(errs) <= GEMV_RTOL, f"slab {slab}: relative error {max(errs):.3g}"
        assert all(np.all(out[t, :rows] == 0) for t in range(T) if not np.any(ref[t]))


def check_bits(wtype, rows, K, T, scales="positive"):
    for slab in slabs(wtype, K):
        sk, tl = (run(wtype, rows, K, T, k, slab, scales) for k in ("skinny", "tiled"))
        np.testing.assert_array_equal(sk.view(np.uint32), tl.view(np.uint32), err_msg=f"slab {slab}")
        assert np.all(sk[:, rows:] == SENTINEL) and np.all(sk[T:] == SENTINEL), "wrote past the outputs"
        assert not np.any(sk[:T, :rows] == SENTINEL)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("rows,K", SHAPES)
@pytest.mark.parametrize("wtype", [Q8_0, Q4_0])
def test_skinny_against_f64(wtype, rows, K, T):
    check_f64(wtype, rows, K, T)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("rows,K", SHAPES)
@pytest.mark.parametrize("wtype", [Q8_0, Q4_0])
def test_skinny_bits_equal_tiled(wtype, rows, K, T):
    check_bits(wtype, rows, K, T)


@pytest.mark.parametrize("wtype", [Q8_0, Q4_0])
def test_edge_block_scales(wtype):
    """Signed, zero and subnormal scales on both sides and a row of zeros: the scale products are v5's."""
    check_f64(wtype, 160, 2560, 7, "edge")
    check_bits(wtype, 160, 2560, 7, "edge")


def test_session_batch_step():
    """mini-1b Q8_0, batch_forward of 8 rows and of 1 at positions 0 and 33: a session on the skinny kernel against
    one under LLMI_PG_SKINNY=0 (v5's launches), and the plan for the model's projection shapes.  The committed switch
    GEMM_ROWS_I8_T_SKINNY is 0 (the kernel measured behind v5), so the skinny session moves
    it to 8 rows with LLMI_GR_I8_T."""
    from llm_inference_amd import ops
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg = CONFIGS["mini-1b"]
    pos, slots = [0, 33] * 4, list(range(8))
    rng = np.random.default_rng(11)
    prompts = [rng.integers(4, cfg.vocab, p + 1).astype(np.int32) for p in pos]
    toks = [int(p[-1]) for p in prompts]
    shapes = [((cfg.n_head + 2 * cfg.n_head_kv) * cfg.head_dim, cfg.n_embd), (cfg.n_embd, cfg.n_head * cfg.head_dim),
              (2 * cfg.n_ff, cfg.n_embd), (cfg.n_embd, cfg.n_ff)]

    def session(plans):
        for B in (1, 8):
            assert [ops.gemm_rows_i8_plan(Q8_0, r, k, B) for r, k in shapes] == [plans] * 4
        assert [ops.gemm_rows_i8_plan(Q8_0, r, k, 9) for r, k in shapes] == [5] * 4
        m = Model(build_gemma3_gguf(cfg, seed=21, wtype=Q8_0), max_ctx=64)
        m.reserve_sequences(8)
        for i in range(1, 8, 2):
            m.forward(prompts[i][:-1], 0, want_logits=False)
            m.copy_sequence(slots[i], 0, pos[i])
        res = [m.batch_forward(toks[a:b], slots[a:b], pos[a:b], want_logits=True) for a, b in ((0, 8), (1, 2))]
        m.close()
        return res

    old = {k: os.environ.pop(k, None) for k in ("LLMI_PG_SKINNY", "LLMI_GR_I8_T")}
    try:
        assert [ops.gemm_rows_i8_plan(Q8_0, r, k, 1) for r, k in shapes] == [5] * 4  # (the committed switch)
        os.environ["LLMI_GR_I8_T"] = "8"
        got = session(1)
        os.environ["LLMI_PG_SKINNY"] = "0"
        ref = session(5)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g.logits.view(np.uint32), r.logits.view(np.uint32))
        np.testing.assert_array_equal(g.argmax, r.argmax)
        np.testing.assert_array_equal(np.asarray(g.lse, np.float32).view(np.uint32), np.asarray(r.lse, np.float32).view(np.uint32))


def test_argument_errors():
    from llm_inference_amd import ops
    from llm_inference_amd._lib import LLMIError
    w, x, _ = case(Q8_0, 64, 128, 2)

    def raises(status, word, *a, **k):
        with pytest.raises(LLMIError) as ei:
            ops.gemm_rows_i8(*a, **k)
        assert ei.value.status == status and word in str(ei.value), (ei.value.status, str(ei.value))

    raises("E_TYPE", "(wtype)", w, 12, 64, 128, x)
    raises("E_SIZE", "n_cols", w[: 64 * 3 * 34], Q8_0, 64, 96, x[:, :96])
    raises("E_SIZE", "n_cols", w[: 64 * 3 * 34], Q8_0, 64, 100, np.zeros((2, 100), np.float32))
    raises("E_RANGE", "(T)", w, Q8_0, 64, 128, np.zeros((0, 128), np.float32))
    raises("E_RANGE", "(T)", w, Q8_0, 64, 128, np.zeros((33, 128), np.float32), kernel="skinny")
    raises("E_SIZE", "slab", w, Q8_0, 64, 128, x, slab=True)
    raises("E_SIZE", "ostride", w, Q8_0, 64, 128, x, out=np.zeros((2, 63), np.float32))
    with pytest.raises(ValueError):
        ops.gemm_rows_i8(w[:-34], Q8_0, 64, 128, x)
    assert ops.gemm_rows_i8_plan(12, 64, 128, 4) == 0 and ops.gemm_rows_i8_plan(Q8_0, 48, 128, 4) == 0
    assert ops.gemm_rows_i8_plan(Q8_0, 64, 96, 4) == 0
