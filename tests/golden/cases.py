"""Deterministic golden-vector CASES shared by gen_golden.py (which runs the
reference itself, oracle/_ref) and the tests (oracle and HIP path).

Each case is (name, kind, params); ``make_inputs`` regenerates the inputs
from a seed with numpy's PCG64 (bit-stable for a given numpy), so only
outputs plus an input hash are committed (tests/golden/*.npz).
Shapes: reduced row counts at the real Gemma-3 n_cols (per-row arithmetic
depends only on n_cols).
"""
from __future__ import annotations

import hashlib

import numpy as np

from llm_inference_amd.gguf import TensorType as T
from llm_inference_amd.synthetic import random_tensor

# (name, ggml type, n_rows, n_cols)
GEMV_CASES = [
    ("q4_0_1152", T.Q4_0, 96, 1152),      # 1B q/gate-like
    ("q4_0_2560", T.Q4_0, 128, 2560),     # 4B q/k/v/gate/up
    ("q4_0_2048", T.Q4_0, 64, 2048),      # 4B attn_output
    ("q4_0_10240", T.Q4_0, 40, 10240),    # 4B ffn_down
    ("q4_0_6912", T.Q4_0, 40, 6912),      # 1B ffn_down
    ("q4_0_5376", T.Q4_0, 40, 5376),      # 27B q/k/v/gate/up
    ("q4_0_96", T.Q4_0, 7, 96),           # ragged tiny: 3 blocks, 7 rows
    ("q4_0_32", T.Q4_0, 5, 32),           # one block per row (ModelTest n_embd)
    ("q4_0_64", T.Q4_0, 9, 64),
    ("q8_0_1152", T.Q8_0, 64, 1152),
    ("q8_0_2560", T.Q8_0, 64, 2560),
    ("q8_0_32", T.Q8_0, 3, 32),
    ("q4_k_2560", T.Q4_K, 64, 2560),
    ("q6_k_2560", T.Q6_K, 64, 2560),
    ("q6_k_10240", T.Q6_K, 24, 10240),
    ("q5_0_1152", T.Q5_0, 64, 1152),
    ("bf16_640", T.BF16, 48, 640),
    ("f16_2560", T.F16, 200, 2560),       # logits-like
    ("f16_1152", T.F16, 130, 1152),
    ("f16_40", T.F16, 9, 40),             # n_cols % 32 != 0 tail path (ops.cpp:581-583)
]

QUANT_CASES = [("q8_0", 32 * 97), ("q8_0", 2560), ("q8_k", 2560), ("q8_k", 256 * 3)]
NORM_CASES = [2560, 256, 1152, 4]
ROPE_CASES = [  # (n_tokens, n_heads, head_dim, base, pos)
    (1, 8, 256, 10000.0, 0), (1, 8, 256, 10000.0, 517), (3, 4, 256, 1000000.0, 41),
    (1, 16, 128, 1000000.0, 4095), (1, 1, 4, 10000.0, 1),
]
DEQ_CASES = [(T.Q4_K, 2560), (T.Q6_K, 2560), (T.Q8_0, 1152), (T.Q5_0, 1152)]


def gemv_inputs(name, ttype, n_rows, n_cols):
    seed = int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)
    w = random_tensor(ttype, n_rows, n_cols, seed=seed)
    x = np.random.default_rng(seed + 1).standard_normal(n_cols).astype(np.float32)
    return w, x


# ---- signed / zero / subnormal block scales (synthetic.SCALE_PROFILES) and edge activations: gen_edge.py ----------
EDGE_PROFILES = ("signed", "edge", "wide")
EDGE_TYPES = (("q4_0", T.Q4_0), ("q5_0", T.Q5_0), ("q8_0", T.Q8_0), ("q4_k", T.Q4_K), ("q6_k", T.Q6_K))
# the smallest shapes at which a row kernel can go wrong (one row, fewer rows than a work-group's, more than one
# work-group; one block, an odd block count) and one real width per type
_EDGE_REAL = {"q4_0": ((32, 2560), (24, 10240)), "q5_0": ((40, 1152),), "q8_0": ((40, 1152),),
              "q4_k": ((32, 2560),), "q6_k": ((32, 2560), (24, 10240))}


def _edge_shapes(tname):
    cols = (256, 512) if tname.endswith("_k") else (32, 96)
    return tuple((r, c) for c in cols for r in (1, 7, 65)) + _EDGE_REAL[tname]


# (name, ggml type, n_rows, n_cols, scale profile, activation kind)
EDGE_GEMV_CASES = [(f"{p}__{tn}_{r}x{c}", tt, r, c, p, "normal")
                   for tn, tt in EDGE_TYPES for p in EDGE_PROFILES for r, c in _edge_shapes(tn)]
EDGE_GEMV_CASES += [(f"signed__{tn}_{r}x{c}__{xk}", tt, r, c, "signed", xk)
                    for tn, tt, (r, c) in (("q4_0", T.Q4_0, (32, 2560)), ("q8_0", T.Q8_0, (40, 1152)),
                                           ("q4_k", T.Q4_K, (32, 2560)))
                    for xk in ("edgex", "zerox")]
EDGE_DEQ_CASES = [(T.Q8_0, 2560), (T.Q5_0, 1152), (T.Q4_K, 2560), (T.Q6_K, 2560)]  # (no Q4_0 dequantize_row exists)


def edge_x(n, blk, rng):
    """N(0, 1) with, per quantization block of ``blk`` elements (32: Q8_0, 256: Q8_K): block 0 all zero (d = 0),
    block 1 a negative constant, block 2 all 1e-30 (a scale far below f16), block 3 one 3e4 outlier; for blk = 256
    also a zero and a constant 32-element sub-block (bsums) inside block 4."""
    x = rng.standard_normal(n).astype(np.float32)
    x[0:blk] = 0.0
    x[blk:2 * blk] = -3.0
    x[2 * blk:3 * blk] = 1e-30
    x[3 * blk + 5] = 3e4
    if blk == 256:
        x[4 * blk + 32:4 * blk + 64] = 0.0
        x[4 * blk + 96:4 * blk + 128] = -3.0
    return x


def edge_gemv_inputs(name, ttype, n_rows, n_cols, profile, xkind, salt=0):
    """salt: the try gen_edge.py settled on (stored beside the outputs as ``__salt``)."""
    seed = int(hashlib.sha256(f"{name}/{salt}".encode()).hexdigest()[:8], 16)
    w = random_tensor(ttype, n_rows, n_cols, seed=seed, scales=profile)
    rng = np.random.default_rng(seed + 1)
    if xkind == "normal":
        x = rng.standard_normal(n_cols).astype(np.float32)
    elif xkind == "edgex":
        x = edge_x(n_cols, 256 if ttype in (T.Q4_K, T.Q6_K) else 32, rng)
    else:
        x = np.zeros(n_cols, np.float32)
    return w, x


def edge_deq_input(ttype, n):
    return random_tensor(ttype, 1, n, seed=4100 + ttype, scales="edge")


def fast_gemv_bound(ref):
    """tests/test_hip_ops.py: fp32 reassociation of the same exact integer block dots."""
    return 1e-4 * float(np.abs(ref).max()) + 1e-6


def quant_input(kind, n, k=0):
    rng = np.random.default_rng(1000 + n + k)
    x = (rng.standard_normal(n) * rng.uniform(0.01, 30.0, size=n // 32).repeat(32)).astype(np.float32)
    x[:32] = 0.0            # an all-zero block: d = 0, id = 0 path (ops.cpp:130)
    x[40] = 1e-30           # tiny denormal-ish magnitude
    x[64:96] = -3.0         # constant negative block
    return x


def norm_input(n):
    return (np.random.default_rng(2000 + n).standard_normal(n) * 3).astype(np.float32)


def rope_input(nt, nh, hd):
    return np.random.default_rng(3000 + nt * 100000 + nh * 1000 + hd).standard_normal((nt, nh, hd)).astype(np.float32)


def deq_input(ttype, n):
    return random_tensor(ttype, 1, n, seed=4000 + ttype)


def f16_input(n=4096):
    rng = np.random.default_rng(5000)
    x = np.concatenate([
        rng.standard_normal(n).astype(np.float32) * np.float32(10.0) ** rng.integers(-9, 6, n).astype(np.float32),
        np.array([0.0, -0.0, 65504.0, 65520.0, 1e9, -1e9, 6e-8, 3e-8, 2.98e-8, 1e-40, np.inf, -np.inf], np.float32),
    ]).astype(np.float32)
    return x


def sha(*arrs) -> str:
    h = hashlib.sha256()
    for a in arrs:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()
