"""Generate tests/golden/ops_edge_ref.npz by running the REFERENCE ITSELF on weights with signed, zero, subnormal
and log-uniform block scales (llm_inference_amd/synthetic.py SCALE_PROFILES) and on edge activations.

Run in the build container (needs /root/reference):
    make -C oracle ref && python tests/golden/gen_edge.py
Per case of cases.EDGE_GEMV_CASES it records
    gemv__<name>__o    the reference's mat_vec_mul (bit patterns)
and, one row per case in the order of gemv__names (packed: a zip entry costs more than these values),
    gemv__sha          hash of the inputs
    gemv__salt         which try of the seed was kept (0 unless the check below failed)
    gemv__ref_vs_f64   max |reference - float64 sum|, the float64 sum being the dequantized weights times the
                       activation the reference's row really multiplies: its own Q8_0 blocks (Q4_0, Q8_0), its own
                       Q8_K blocks (Q4_K, Q6_K), x itself (Q5_0, ops.cpp:873-874)
and asserts ref_vs_f64 <= a quarter of the fast-GEMV bound the kernels are held to (cases.fast_gemv_bound), taking the
next salt if not: the reference alone sits well inside that bound.  Per case of cases.EDGE_DEQ_CASES it records the
reference's dequantize_row of one "edge" row.  No reference source or binary is committed; only this data file.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle.bind import Reference  # noqa: E402
from llm_inference_amd.gguf import TensorType as T, row_bytes  # noqa: E402
import cases as K  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
MAX_SALT = 8


def weights_f64(ref: Reference, tt, w, r, c) -> np.ndarray:
    if tt == T.Q4_0:  # the reference has no dequantize_q4_0_row: d (q - 8), elements 0..15 the low nibbles, 16..31 the high
        blk = w.reshape(r, c // 32, 18)
        d = blk[:, :, 0:2].copy().view(np.float16).astype(np.float64)
        q = np.concatenate([blk[:, :, 2:] & 15, blk[:, :, 2:] >> 4], axis=2).astype(np.float64) - 8.0
        return (d * q).reshape(r, c)
    rb = row_bytes(tt, c)
    return np.stack([ref.dequantize_row(tt, w[i * rb:(i + 1) * rb], c) for i in range(r)]).astype(np.float64)


def activation_f64(ref: Reference, tt, x) -> np.ndarray:
    if tt in (T.Q4_0, T.Q8_0):
        b = ref.quantize_q8_0(x).reshape(-1, 34)
        d = b[:, 0:2].copy().view(np.float16).astype(np.float64)
        return (d * b[:, 2:].view(np.int8).astype(np.float64)).reshape(-1)
    if tt in (T.Q4_K, T.Q6_K):  # block_q8_K: float d; int8 qs[256]; int16 bsums[16]
        b = ref.quantize_q8_k(x).reshape(-1, 292)
        d = b[:, 0:4].copy().view(np.float32).astype(np.float64)
        return (d * b[:, 4:260].view(np.int8).astype(np.float64)).reshape(-1)
    return x.astype(np.float64)


def gen(ref: Reference) -> dict:
    d = {}
    worst = {}
    shas, salts, errs = [], [], []
    for name, tt, r, c, prof, xk in K.EDGE_GEMV_CASES:
        for salt in range(MAX_SALT):
            w, x = K.edge_gemv_inputs(name, tt, r, c, prof, xk, salt)
            o = ref.mat_vec_mul(tt, w, r, c, x)
            assert np.isfinite(o).all(), name
            err = float(np.abs(o.astype(np.float64) - weights_f64(ref, tt, w, r, c) @ activation_f64(ref, tt, x)).max())
            if err <= K.fast_gemv_bound(o) / 4:
                break
            print(f"{name}: salt {salt}: ref_vs_f64 {err:.3g} > bound / 4 = {K.fast_gemv_bound(o) / 4:.3g}; next seed")
        else:
            raise AssertionError(f"{name}: no seed puts the reference inside a quarter of the fast-GEMV bound")
        d[f"gemv__{name}__o"] = o
        shas.append(np.frombuffer(K.sha(w, x).encode(), np.uint8))
        salts.append(salt)
        errs.append(err)
        rel = err / K.fast_gemv_bound(o)
        key = prof if xk == "normal" else xk
        worst[key] = max(worst.get(key, 0.0), rel)
    d["gemv__names"] = np.array([c[0] for c in K.EDGE_GEMV_CASES])
    d["gemv__sha"] = np.stack(shas)
    d["gemv__salt"] = np.array(salts, np.int32)
    d["gemv__ref_vs_f64"] = np.array(errs, np.float64)
    for tt, n in K.EDGE_DEQ_CASES:
        d[f"deq__{tt}_{n}"] = ref.dequantize_row(tt, K.edge_deq_input(tt, n), n)
    print("worst ref_vs_f64 / fast-GEMV bound:", {k: f"{v:.3g}" for k, v in worst.items()})
    return d


def main():
    ref = Reference(n_threads=4)
    path = os.path.join(OUT, "ops_edge_ref.npz")
    np.savez_compressed(path, **gen(ref))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
