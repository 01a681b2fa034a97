"""The multi-row F16 logits GEMV at the op level (ops.logits_rows; csrc/k_gemv.hip gemv_f16_rows_multi; DESIGN.md
section 13).

Its contract needs no tolerance: row t of the result carries the bits the fast single-row F16 GEMV (launch_gemv's
gemv_f16_rows_pipe, reached here through ops.DeviceWeight on an F16 weight: it rounds x to f16 -- a no-op on the
f16-representable x used here -- and calls launch_gemv) writes for x[t] alone, whatever the other rows are.  RB, the
rows that share one read of the table, comes from the library (ops.logits_rows_rb).
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_libm = ctypes.CDLL("libm.so.6")
_libm.tanhf.restype = ctypes.c_float
_libm.tanhf.argtypes = [ctypes.c_float]

F16 = 1  # TensorType.F16
T_MAX = 64
# E: P full passes of 64 lanes + a partial pass of T lanes -- P = 0 with T = 16, P = 2 with T = 16, T = 0, T = 32, P = 12
WIDTHS = (128, 1152, 2560, 5376, 6144)


def launch_waves(E):
    """The waves launch_gemv (and the multi-row launch) starts for a table of at least that many rows."""
    return 256 * 8 if E >= 2560 else 256 * 16


def vocab_sizes(E):
    """37: fewer table rows than the waves of its 10 work-groups.  waves + 517: every wave takes a first row, 517
    of them a second one (517 is no multiple of anything the launch uses), so the grid-stride loop, the clamped
    prefetch (the waves without a second row prefetch row V - 1) and a ragged last iteration all run."""
    return 37, launch_waves(E) + 517


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(E, V):
    """x [64][E] and w [V][E] as f16, mixed signs, some rows and columns all zero; and the single-row GEMV's result
    for every row of x.  Computed once per shape, read-only."""
    from llm_inference_amd import ops
    assert V * E * 2 <= 50e6
    rng = np.random.default_rng(1000 * E + V)
    x = rng.standard_normal((T_MAX, E)).astype(np.float16)
    w = (rng.standard_normal((V, E)) * 0.5).astype(np.float16)
    x[3] = 0
    x[:, [5, E - 1]] = 0
    w[[0, V - 1]] = 0
    w[:, 7] = 0
    assert (x < 0).any() and (x > 0).any() and (w < 0).any() and (w > 0).any()
    dw = ops.DeviceWeight(F16, w.view(np.uint8).reshape(-1), V, E)
    ref = np.stack([dw(x[t].astype(np.float32)) for t in range(T_MAX)])
    for a in (x, w, ref):
        a.setflags(write=False)
    return x, w, ref


@pytest.mark.parametrize("which_v", [0, 1], ids=["V37", "Vwaves+517"])
@pytest.mark.parametrize("E", WIDTHS)
def test_rows_equal_single_row_gemv_bits(E, which_v):
    from llm_inference_amd import ops
    V = vocab_sizes(E)[which_v]
    RB = ops.logits_rows_rb(E)
    assert RB >= 2
    x, w, ref = case(E, V)
    assert np.isfinite(ref).all() and (ref[3] == 0).all() and (ref[:, 0] == 0).all() and (ref != 0).any()
    for T in (1, RB, RB + 1, T_MAX):
        got = ops.logits_rows(x[:T], w)
        assert got.shape == (T, V) and got.dtype == np.float32
        np.testing.assert_array_equal(u32(got), u32(ref[:T]), err_msg=f"E = {E}, V = {V}, T = {T}")


def test_softcap_is_the_existing_softcap_of_the_single_row_result():
    """cap tanhf(l / cap) in f32 with glibc's tanhf (the soft-cap launch's arithmetic, csrc/glibc_math.h) applied on
    the host to the single-row GEMV's logits."""
    from llm_inference_amd import ops
    E, cap = 1152, np.float32(30.0)
    V = vocab_sizes(E)[1]
    x, w, ref = case(E, V)
    T = ops.logits_rows_rb(E) + 1
    scaled = (x[:T].astype(np.float32) * 8).astype(np.float16)  # logits well into tanh's bend
    dw = ops.DeviceWeight(F16, w.view(np.uint8).reshape(-1), V, E)
    plain = np.stack([dw(scaled[t].astype(np.float32)) for t in range(T)])
    assert np.abs(plain).max() > 30
    q = plain / cap
    assert q.dtype == np.float32
    want = cap * np.array([_libm.tanhf(float(v)) for v in q.reshape(-1)], np.float32).reshape(q.shape)
    assert want.dtype == np.float32
    np.testing.assert_array_equal(u32(ops.logits_rows(scaled, w, softcap=float(cap))), u32(want))
    np.testing.assert_array_equal(u32(ops.logits_rows(scaled, w)), u32(plain))  # softcap 0: none


def test_rows_are_independent():
    """Permuting the rows permutes the results; replacing every other row leaves a row's bits alone."""
    from llm_inference_amd import ops
    E = 2560
    V = vocab_sizes(E)[1]
    x, w, ref = case(E, V)
    T = 2 * ops.logits_rows_rb(E) + 3
    perm = np.random.default_rng(3).permutation(T)
    np.testing.assert_array_equal(u32(ops.logits_rows(x[:T][perm], w)), u32(ref[:T][perm]))
    other = np.random.default_rng(4).standard_normal((T, E)).astype(np.float16)
    for keep in (0, T // 2, T - 1):
        y = other.copy()
        y[keep] = x[keep]
        np.testing.assert_array_equal(u32(ops.logits_rows(y, w)[keep]), u32(ref[keep]))


@pytest.mark.parametrize("E", [136, 6272])
def test_unsupported_width(E):
    from llm_inference_amd import ops
    from llm_inference_amd._lib import LLMIError
    assert ops.logits_rows_rb(E) == 0
    with pytest.raises(LLMIError) as ei:
        ops.logits_rows(np.zeros((2, E), np.float16), np.zeros((5, E), np.float16))
    assert ei.value.status == "E_SIZE" and "E" in str(ei.value)
