"""Every weight type's GEMV and dequantize_row on signed, zero, subnormal and log-uniform block scales
(llm_inference_amd/synthetic.py SCALE_PROFILES) and on edge activations (an all-zero, a constant and a 1e-30 block, a
3e4 outlier, the all-zero x), against tests/golden/ops_edge_ref.npz, which tests/golden/gen_edge.py records from the
reference itself.  Everything else in the suite draws positive, normal scales within one decade; real files carry a
negative d in about half of their Q4_0 / Q5_0 / Q6_K blocks, d = 0 in all-zero blocks and subnormal K-quant d / dmin.

  * CPU: the oracle reproduces every entry bit for bit (so the model-level edge tests, which compare with the oracle,
    compare with the reference).
  * GPU, exact kernels: bit-identical.
  * GPU, fast GEMV: tests/test_hip_ops.py's bound, 1e-4 max|ref| + 1e-6, unchanged.  gen_edge.py asserts that the
    reference itself is within a quarter of it of the float64 sum (it measures under 1 % of it on every case).
"""
import functools
import os

import numpy as np
import pytest

import cases as K
from llm_inference_amd.gguf import TensorType as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEMV_IDS = [c[0] for c in K.EDGE_GEMV_CASES]
gpu = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "ops_edge_ref.npz")))
    assert g["gemv__names"].tolist() == GEMV_IDS, "cases.EDGE_GEMV_CASES and ops_edge_ref.npz differ: run gen_edge.py"
    for a in g.values():
        a.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(w, x, reference output) of a case, generated once and shared read-only by the tests of this module."""
    g = golden()
    i = GEMV_IDS.index(name)
    case = K.EDGE_GEMV_CASES[i]
    w, x = K.edge_gemv_inputs(*case, salt=int(g["gemv__salt"][i]))
    assert K.sha(w, x).encode() == g["gemv__sha"][i].tobytes(), "input generator drifted"
    w.setflags(write=False)
    x.setflags(write=False)
    return w, x, g[f"gemv__{name}__o"]


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def ops():
    from llm_inference_amd import ops as O
    O.init_ops(0)
    return O


# ---- the generator ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname,tt", K.EDGE_TYPES, ids=[t[0] for t in K.EDGE_TYPES])
def test_profiles_hold_what_they_promise(tname, tt):
    """Per type: "signed" keeps the positive profile's bytes but for the sign bits; "edge" puts a zero and a subnormal d
    into every row of at least 8 blocks, both signs of each and the smallest normal somewhere, and no |w| above the
    positive profile's; "wide" spans the f16 range below 1."""
    from llm_inference_amd.synthetic import _SCALE_FIELDS, random_tensor
    bsz, fields = _SCALE_FIELDS[tt]
    cols = 2560
    r = 16

    def scale_bits(w, off):
        return w.reshape(-1, bsz)[:, off:off + 2].copy().view(np.uint16).reshape(r, -1)

    pos = random_tensor(tt, r, cols, seed=5)
    sg = random_tensor(tt, r, cols, seed=5, scales="signed")
    diff = (pos ^ sg).reshape(-1, bsz)
    mask = np.zeros(bsz, np.uint8)
    for off in fields:
        mask[off + 1] = 0x80
        s = scale_bits(sg, off) >> 15
        assert 0.3 < s.mean() < 0.7
    assert (diff & ~mask == 0).all() and diff.any()
    if tt == T.Q4_K:  # independent signs
        assert ((scale_bits(sg, 0) ^ scale_bits(sg, 2)) >> 15).any()
    ed = random_tensor(tt, r, cols, seed=5, scales="edge")
    for off in fields[:1]:
        d = scale_bits(ed, off)
        mag = d & 0x7FFF
        assert (mag == 0).any(axis=1).all() and ((mag > 0) & (mag < 0x400)).any(axis=1).all()
        assert set(d[mag == 0].tolist()) == {0x0000, 0x8000}
        assert len(set((d[(mag > 0) & (mag < 0x400)] >> 15).tolist())) == 2
        assert (mag == 0x400).any()
    wd = random_tensor(tt, r, cols, seed=5, scales="wide")
    m = scale_bits(wd, fields[0]) & 0x7FFF
    assert m.max() <= 0x3C00 and (m < 0x400).any() and (m > 0x3000).any()
    if tt != T.Q4_0:  # (no dequantize_row for Q4_0; its |d (q - 8)| <= 8 |d| whatever the nibbles)
        from oracle.bind import Oracle
        orc = Oracle()
        rb = bsz * (cols // (32 if bsz < 100 else 256))
        top = max(np.abs(orc.dequantize_row(tt, ed[i * rb:(i + 1) * rb], cols)).max() for i in range(r))
        assert top <= _positive_max(tt) * (1 + 2.0 ** -10)  # (f16 rounding of the largest scale)


def _positive_max(tt):
    """max |w| the positive profile can draw: scale_hi = 0.02 and the largest quant (Q4_K: d sc q - dmin m with the
    two scale fields of opposite sign adds the min term to the largest quant's, 16 / 15 of the one-signed range)"""
    return {T.Q5_0: 0.02 / 2 * 16, T.Q8_0: 0.02 / 8 * 127, T.Q4_K: 0.02 / 16 * 63 * 16, T.Q6_K: 0.02 / 64 * 64 * 32}[tt]


def test_default_profile_is_todays_bytes():
    """scales="positive" draws nothing more: the committed hashes of ops_ref.npz (test_oracle_golden.py) pin the
    default; this pins the explicit keyword to it."""
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf, random_tensor
    for _n, tt in K.EDGE_TYPES:
        np.testing.assert_array_equal(random_tensor(tt, 3, 512, seed=9), random_tensor(tt, 3, 512, seed=9, scales="positive"))
    np.testing.assert_array_equal(build_gemma3_gguf(CONFIGS["tiny"], seed=7),
                                  build_gemma3_gguf(CONFIGS["tiny"], seed=7, scales="positive"))
    with pytest.raises(ValueError):
        random_tensor(T.Q4_0, 1, 32, scales="negative")


# ---- the oracle against the reference (CPU) -----------------------------------------------------------------------
@pytest.mark.parametrize("name", GEMV_IDS)
def test_oracle_gemv_bitexact(oracle, name):
    _n, tt, r, c, _p, _x = K.EDGE_GEMV_CASES[GEMV_IDS.index(name)]
    w, x, ref = inputs(name)
    np.testing.assert_array_equal(bits(oracle.mat_vec_mul(tt, w, r, c, x, n_threads=3)), bits(ref))


@pytest.mark.parametrize("tt,n", K.EDGE_DEQ_CASES)
def test_oracle_dequantize_bitexact(oracle, tt, n):
    np.testing.assert_array_equal(bits(oracle.dequantize_row(tt, K.edge_deq_input(tt, n), n)),
                                  bits(golden()[f"deq__{tt}_{n}"]))


def test_reference_sits_inside_the_fast_bound():
    """What gen_edge.py asserted when it wrote the file: the reference's own distance from the float64 sum is at most
    a quarter of the bound the fast kernels are held to."""
    g = golden()
    for i, name in enumerate(GEMV_IDS):
        assert g["gemv__ref_vs_f64"][i] <= K.fast_gemv_bound(g[f"gemv__{name}__o"]) / 4, name


# ---- the kernels (GPU) --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", GEMV_IDS)
def test_gemv_exact_bitwise(ops, name):
    _n, tt, r, c, _p, _x = K.EDGE_GEMV_CASES[GEMV_IDS.index(name)]
    w, x, ref = inputs(name)
    np.testing.assert_array_equal(bits(ops.mat_vec_mul_raw(tt, w, r, c, x, exact=True)), bits(ref))


@gpu
@pytest.mark.parametrize("name", GEMV_IDS)
def test_gemv_fast_tolerance(ops, name):
    _n, tt, r, c, _p, _x = K.EDGE_GEMV_CASES[GEMV_IDS.index(name)]
    w, x, ref = inputs(name)
    o = ops.mat_vec_mul_raw(tt, w, r, c, x, exact=False)
    err, bound = float(np.abs(o - ref).max()), K.fast_gemv_bound(ref)
    print(f"fast-vs-ref {name} {err:.4g} bound {bound:.4g} ratio {err / bound:.4g}")
    assert err <= bound


@gpu
@pytest.mark.parametrize("tt,n", K.EDGE_DEQ_CASES)
def test_dequantize_bitwise(ops, tt, n):
    np.testing.assert_array_equal(bits(ops.dequantize_row(tt, K.edge_deq_input(tt, n), n)),
                                  bits(golden()[f"deq__{tt}_{n}"]))


@gpu
@pytest.mark.parametrize("name", ["edge__q4_0_32x2560", "edge__q4_0_24x10240", "edge__q4_k_32x2560"])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
def test_device_weight_reuse(ops, name, exact):
    """The repacked device layouts (DeviceWeight keeps the weight resident): the same bits on three consecutive
    calls, the reference's in exact mode, inside the fast bound otherwise."""
    _n, tt, r, c, _p, _x = K.EDGE_GEMV_CASES[GEMV_IDS.index(name)]
    w, x, ref = inputs(name)
    dw = ops.DeviceWeight(tt, w, r, c)
    got = [dw(x, exact=exact) for _ in range(3)]
    np.testing.assert_array_equal(bits(got[1]), bits(got[0]))
    np.testing.assert_array_equal(bits(got[2]), bits(got[0]))
    if exact:
        np.testing.assert_array_equal(bits(got[0]), bits(ref))
    else:
        assert np.abs(got[0] - ref).max() <= K.fast_gemv_bound(ref)
