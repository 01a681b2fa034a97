"""The kernels of lookup decoding for sampled rows at the op level, without a model:
ops.logits_rows_gather (csrc/k_gemv.hip gemv_f16_rows_gather + the soft-cap over the listed rows) against
ops.logits_rows' rows, bit for bit, and ops.sample_logits_rows (csrc/k_sample.hip, the token-row forms) against
tests/test_sampling.py's ref_sample, id for id.  Neither needs a tolerance."""
import functools

import numpy as np
import pytest

from test_sampling import ref_sample

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-12345.5)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def gemv_case(E, V, softcap):
    """70 activation rows, the table, and ops.logits_rows' rows: computed once per shape, read-only."""
    from llm_inference_amd import ops
    rng = np.random.default_rng(E + V)
    x = (rng.standard_normal((70, E)) * 0.5).astype(np.float16)
    w = (rng.standard_normal((V, E)) * 0.5).astype(np.float16)
    want = ops.logits_rows(x, w, softcap=softcap)
    for a in (x, w, want):
        a.setflags(write=False)
    return x, w, want


def waves_of(E):
    """The wave count of the GEMV's launch at a long table (csrc/k_gemv.hip launch_gemv_f16_rows)."""
    return 256 * 8 if E >= 2560 else 256 * 16


@pytest.mark.parametrize("E", [128, 2560, 5376])
def test_logits_rows_gather_equals_logits_rows(E):
    from llm_inference_amd import ops
    RB = ops.logits_rows_rb(E)
    assert RB == (8 if E <= 3840 else 4)
    rng = np.random.default_rng(7)
    # V = 37: fewer table rows than waves; V = waves + 517: every wave a second pass, the last one ragged
    shapes = [(37, 0.0), (37, 30.0), (waves_of(E) + 517, 0.0)]
    for V, softcap in shapes:
        x, w, want = gemv_case(E, V, softcap)
        for n in (0, 1, RB, RB + 1, 64):
            perm = rng.permutation(70)[:n]                      # distinct rows, out of order
            rep = rng.integers(0, 5, n)                         # a few rows, repeated
            for idx in (perm, rep):
                fill = np.full((64, V), SENTINEL, np.float32)
                got = ops.logits_rows_gather(x, w, idx, cap=64, softcap=softcap, out=fill)
                assert got.shape == (64, V)
                np.testing.assert_array_equal(u32(got[:n]), u32(want[idx]), err_msg=f"E {E} V {V} n {n}")
                assert (got[n:] == SENTINEL).all(), f"rows at and past n_idx written (E {E} V {V} n {n})"
    # a smaller cap: the grid covers cap rows only
    x, w, want = gemv_case(E, 37, 0.0)
    got = ops.logits_rows_gather(x, w, [69, 0, 3], cap=RB + 1, out=np.full((RB + 1, 37), SENTINEL, np.float32))
    np.testing.assert_array_equal(u32(got[:3]), u32(want[[69, 0, 3]]))
    assert (got[3:] == SENTINEL).all()


def test_logits_rows_gather_errors():
    from llm_inference_amd import ops
    from test_batch_decode import raises
    x = np.zeros((4, 128), np.float16)
    w = np.zeros((8, 128), np.float16)
    raises("E_RANGE", "(idx)", ops.logits_rows_gather, x, w, [0, 4])
    raises("E_RANGE", "(idx)", ops.logits_rows_gather, x, w, [-1])
    raises("E_RANGE", "(cap)", ops.logits_rows_gather, x, w, [0], cap=65)
    raises("E_RANGE", "(n_idx)", ops.logits_rows_gather, x, w, [0, 1, 2], cap=2)
    raises("E_SIZE", "multiple of 128", ops.logits_rows_gather, np.zeros((4, 136), np.float16),
           np.zeros((8, 136), np.float16), [0])


SAMPLERS = (dict(temperature=1.0, top_k=64, top_p=0.95, seed=101), dict(temperature=1.5, top_k=0, top_p=1.0, seed=202),
            dict(temperature=0.7, top_k=40, top_p=0.9, seed=303), dict(temperature=24.0, top_k=1, top_p=1.0, seed=404),
            dict(temperature=3.0, top_k=256, top_p=0.5, seed=(1 << 63) + 11))


@pytest.mark.parametrize("V", [37, 4100])
@pytest.mark.parametrize("R", [1, 9, 65, 512])
def test_sample_logits_rows_equals_reference(R, V):
    """Mixed samplers by row group (the loop's t / W mapping is one such), per-row positions, ended rows, and the
    logits the sampler treats specially: -inf, NaN, a row that is all NaN."""
    from llm_inference_amd import ops
    rng = np.random.default_rng(1000 * R + V)
    lg = (rng.standard_normal((R, V)) * 3).astype(np.float32)
    lg[0, 3] = -np.inf
    lg[0, 5] = np.nan
    lg[R // 2, rng.choice(V, V // 3, replace=False)] = -np.inf
    lg[R - 1, int(np.argmax(lg[R - 1]))] = np.nan
    if R >= 9:
        lg[4, :] = np.nan                                       # every logit NaN: token 0
        lg[7, 11] = np.inf                                      # a non-finite top logit: that token
    W = 8
    of = (np.arange(R) // W) % len(SAMPLERS)                    # groups of W consecutive rows share a sampler
    pos = rng.integers(0, 5000, R).astype(np.int32)
    ended = rng.random(R) < 0.25 if R > 1 else np.zeros(1, bool)
    pos[ended] = -1
    if R >= 65:
        pos[64] = 17                                            # the first row of the second chunk is live
    got = ops.sample_logits_rows(lg, SAMPLERS, of, pos)
    assert got.dtype == np.int32 and got.shape == (R,)
    n_live = 0
    for r in range(R):
        if pos[r] < 0:
            assert got[r] == -1, r
            continue
        sp = SAMPLERS[of[r]]
        want = ref_sample(lg[r], sp["temperature"], sp["top_k"], sp["top_p"], sp["seed"] & ((1 << 64) - 1), int(pos[r]))
        assert got[r] == want, (R, V, r, of[r], int(pos[r]))
        n_live += 1
    assert n_live >= 1
    if R >= 9 and pos[4] >= 0:
        assert got[4] == 0
    if R >= 9 and pos[7] >= 0:
        assert got[7] == 11


def test_sample_logits_rows_position_decides_the_draw():
    """The same logits row at 64 positions: the ids follow ref_sample at each position and are not all the same."""
    from llm_inference_amd import ops
    V = 4100
    row = (np.random.default_rng(2).standard_normal(V) * 3).astype(np.float32)
    lg = np.tile(row, (64, 1))
    pos = np.arange(100, 164, dtype=np.int32)
    got = ops.sample_logits_rows(lg, [SAMPLERS[0]], np.zeros(64, np.int32), pos)
    sp = SAMPLERS[0]
    want = [ref_sample(row, sp["temperature"], sp["top_k"], sp["top_p"], sp["seed"], int(p)) for p in pos]
    assert got.tolist() == want and len(set(want)) > 8


def test_sample_logits_rows_errors():
    from llm_inference_amd import ops
    from test_batch_decode import raises
    lg = np.zeros((2, 16), np.float32)
    raises("E_ARG", "temperature", ops.sample_logits_rows, lg, [dict(temperature=0.0)], [0, 0], [1, 2])
    raises("E_ARG", "samplers[1]", ops.sample_logits_rows, lg, [SAMPLERS[0], dict(temperature=1.0, top_k=300)], [0, 1],
           [1, 2])
    raises("E_RANGE", "(R)", ops.sample_logits_rows, np.zeros((513, 4), np.float32), [SAMPLERS[0]], [0] * 513, [1] * 513)
    with pytest.raises(ValueError):
        ops.sample_logits_rows(lg, [SAMPLERS[0]], [0, 1], [1, 2])
