"""The multi-row Q8_0 x Q8_0 logits GEMV at the op level (ops.logits_rows_q8; csrc/k_gemv.hip gemv_q8_0_rows_multi;
DESIGN.md section 20).

Bits: row t equals the fast single-row Q8_0 GEMV of x[t] alone through the handle API (ops.DeviceWeight:
llmi_weight_create / llmi_weight_mat_vec_mul, which quantizes x to Q8_0 and calls launch_gemv).
f64 reference: the dequantized table times the dequantized Q8_0 activations (the oracle's quantize_row_q8_0).  The
bound is derived: a block dot is an integer below 2^24, exact in f32; a term (sw * dx) * (float)dot takes two
roundings; a lane adds its terms of a table row in a chain of at most nb additions and wave_sum adds the 64 lane sums
in a tree six additions deep (four DPP steps over 16 lanes, then (a + b) + (c + d)); every partial sum is at most
S = sum_b |term_b|.  So |err| <= (nb + 8) 2^-24 S per output, to first order.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
Q8_0, T_MAX = 8, 64
# (E, V): 4 blocks per row (fewer items than lanes), V no multiple of 4 R | mini-1b's width, 36 blocks: table rows
# straddle lanes in the flat list | 80 blocks
SHAPES = ((128, 257), (1152, 1003), (2560, 515))


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(E, V, scales):
    """x [64][E] (mixed signs, a zero row, zero columns), the table's GGUF blocks, the single-row GEMV of every row,
    the f64 product and its sum of |term_b|.  Computed once per case, read-only."""
    from llm_inference_amd import ops
    from llm_inference_amd.synthetic import random_tensor
    from oracle.bind import Oracle
    orc, nb = Oracle(), E // 32
    x = np.random.default_rng(1000 * E + V).standard_normal((T_MAX, E)).astype(np.float32)
    x[3] = 0
    x[:, [5, E - 1]] = 0
    w = random_tensor(Q8_0, V, E, seed=E + V, scales=scales)
    dw = ops.DeviceWeight(Q8_0, w, V, E)
    ref = np.stack([dw(x[t]) for t in range(T_MAX)])
    wf = np.stack([orc.dequantize_row(Q8_0, w[v * nb * 34:(v + 1) * nb * 34], E) for v in range(V)]).astype(np.float64)
    xf = np.stack([orc.dequantize_row(Q8_0, orc.quantize_q8_0(x[t]), E) for t in range(T_MAX)]).astype(np.float64)
    terms = np.einsum("vbk,tbk->tvb", wf.reshape(V, nb, 32), xf.reshape(T_MAX, nb, 32))
    out = (x, w, ref, terms.sum(axis=2), np.abs(terms).sum(axis=2))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("scales", ["positive", "edge"])
@pytest.mark.parametrize("E,V", SHAPES)
def test_rows_equal_single_row_gemv_bits_and_f64(E, V, scales):
    from llm_inference_amd import ops
    RB = ops.logits_rows_q8_rb(E)
    assert RB >= 2
    x, w, ref, f64, mag = case(E, V, scales)
    assert np.isfinite(ref).all() and (ref[3] == 0).all() and (ref != 0).any()
    bound = (E // 32 + 8) * 2.0 ** -24 * mag
    for T in (1, RB - 1, RB, RB + 1, T_MAX):
        got = ops.logits_rows_q8(x[:T], w)
        assert got.shape == (T, V) and got.dtype == np.float32
        np.testing.assert_array_equal(u32(got), u32(ref[:T]), err_msg=f"E = {E}, V = {V}, T = {T}")
        err = np.abs(got.astype(np.float64) - f64[:T])
        print(f"E {E} V {V} {scales} T {T}: max err / bound = {(err / np.maximum(bound[:T], 1e-300)).max():.3f}")
        assert (err <= bound[:T]).all()


def test_softcap_is_the_existing_softcap_of_the_single_row_result():
    """cap tanhf(l / cap) in f32 with glibc's tanhf (the soft-cap launch's arithmetic) on the single-row logits."""
    from llm_inference_amd import ops
    tanhf = ctypes.CDLL("libm.so.6").tanhf
    tanhf.restype, tanhf.argtypes = ctypes.c_float, [ctypes.c_float]
    (E, V), cap = SHAPES[1], np.float32(2.0)
    x, w, ref, _, _ = case(E, V, "positive")
    T = ops.logits_rows_q8_rb(E) + 1
    q = ref[:T] / cap
    want = cap * np.array([tanhf(float(v)) for v in q.reshape(-1)], np.float32).reshape(q.shape)
    assert np.abs(ref[:T]).max() > 2 and q.dtype == np.float32 and want.dtype == np.float32
    np.testing.assert_array_equal(u32(ops.logits_rows_q8(x[:T], w, softcap=float(cap))), u32(want))
    np.testing.assert_array_equal(u32(ops.logits_rows_q8(x[:T], w)), u32(ref[:T]))  # softcap 0: none


def test_errors():
    from llm_inference_amd import ops
    from llm_inference_amd._lib import LLMIError, lib, ptr
    w = np.zeros(5 * 4 * 34, np.uint8)
    assert ops.logits_rows_q8_rb(136) == 0 and ops.logits_rows_q8_rb(0) == 0
    for x, status in ((np.zeros((2, 136), np.float32), "E_SIZE"), (np.zeros((0, 128), np.float32), "E_ARG")):
        with pytest.raises(LLMIError) as ei:
            ops.logits_rows_q8(x, w)
        assert ei.value.status == status
    x, o = np.zeros((2, 128), np.float32), np.zeros((2, 5), np.float32)
    for args in ((None, ptr(w), ptr(o)), (ptr(x), None, ptr(o)), (ptr(x), ptr(w), None)):
        assert lib().llmi_logits_rows_q8(args[0], args[1], 2, 5, 128, 0.0, args[2]) == 3  # LLMI_E_ARG
