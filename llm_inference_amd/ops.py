"""Python mirror of the reference's ops.h surface (ops.h:38-105), executed by
the HIP library through the C ABI (include/llmi.h).

Same names, argument meaning and error behaviour as the reference:
  * ``mat_vec_mul(o, w_tensor, gguf_file, x)`` resizes/fills ``o`` with
    W*x where W is the GGUF tensor (ops.cpp:933-956); a wrong ``len(x)``
    raises RuntimeError("mat_vec_mul_q4_0: input vector size mismatch"),
    an unsupported type RuntimeError("mat_vec_mul: unsupported tensor type N")
    (ops.cpp:196-198, 953-954);
  * ``rms_norm`` with eps <= 0 raises (the reference exit(1)s, ops.cpp:29-32).
Buffers are numpy arrays; everything is synchronous.  ``exact=True`` selects
the bit-exact AVX2-order kernels (LLMI_EXACT).
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from ._lib import LLMI_EXACT, LLMIError, check, lib, ptr
from .gguf import GGUFFile, TensorInfo, TensorType


def init_ops(device: int = 0) -> None:
    """init_ops(n_threads) (ops.cpp:21-24): selects the HIP device."""
    check(lib().llmi_init_ops(device))


def _f32(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32)


def _fill(o, vals: np.ndarray):
    if o is None:
        return vals
    if isinstance(o, list):
        o[:] = vals.tolist()
        return o
    o.resize(vals.shape, refcheck=False)
    o[...] = vals
    return o


def _raise(e: LLMIError):
    raise RuntimeError(str(e)) from e


def mat_vec_mul_raw(ttype: int, w, n_rows: int, n_cols: int, x, exact: bool = False) -> np.ndarray:
    w = np.ascontiguousarray(np.frombuffer(w, np.uint8) if not isinstance(w, np.ndarray) else w)
    x = _f32(x)
    o = np.zeros(n_rows, np.float32)
    try:
        check(lib().llmi_mat_vec_mul(ttype, ptr(w), n_rows, n_cols, ptr(x), x.size, ptr(o),
                                     LLMI_EXACT if exact else 0))
    except LLMIError as e:
        _raise(e)
    return o


def mat_vec_mul(o, w_tensor: TensorInfo, gguf_file: GGUFFile, x, exact: bool = False):
    """ops.cpp:933-956: n_rows = shape[1], n_cols = shape[0]."""
    if w_tensor.tensor_type == TensorType.F16:  # not in the reference dispatch
        raise RuntimeError(f"mat_vec_mul: unsupported tensor type {w_tensor.tensor_type}")
    w = np.frombuffer(gguf_file.get_tensor_data(w_tensor), np.uint8)
    vals = mat_vec_mul_raw(w_tensor.tensor_type, w, w_tensor.shape[1], w_tensor.shape[0], x, exact)
    return _fill(o, vals)


def mat_vec_mul_fp16(o, w, x, n_rows: int, n_cols: int, exact: bool = False):
    """ops.cpp:455-612 (w: n_rows*n_cols uint16 f16 bits)."""
    w = np.ascontiguousarray(w, np.uint16)
    if len(x) != n_cols:
        raise RuntimeError("mat_vec_mul_fp16: input vector size mismatch")
    if w.size != n_rows * n_cols:
        raise RuntimeError("mat_vec_mul_fp16: weight matrix size mismatch")
    return _fill(o, mat_vec_mul_raw(TensorType.F16, w.view(np.uint8), n_rows, n_cols, x, exact))


def quantize_row_q8_0(x) -> np.ndarray:
    """ops.cpp:116-139 -> 34-byte BlockQ8_0 blocks."""
    x = _f32(x)
    y = np.zeros(x.size // 32 * 34, np.uint8)
    check(lib().llmi_quantize_row_q8_0(ptr(x), x.size, ptr(y)))
    return y


def quantize_row_q8_k(x) -> np.ndarray:
    """ops.cpp:142-178 -> 292-byte block_q8_K blocks."""
    x = _f32(x)
    y = np.zeros(x.size // 256 * 292, np.uint8)
    check(lib().llmi_quantize_row_q8_k(ptr(x), x.size, ptr(y)))
    return y


def dequantize_row(ttype: int, blocks, n_cols: int) -> np.ndarray:
    """dequantize_{q4_k,q6_k,q8_0,q5_0}_row (ops.cpp:958-1082)."""
    b = np.ascontiguousarray(np.frombuffer(blocks, np.uint8) if not isinstance(blocks, np.ndarray) else blocks)
    o = np.zeros(n_cols, np.float32)
    check(lib().llmi_dequantize_row(ttype, ptr(b), n_cols, ptr(o)))
    return o


def rms_norm(o, x, eps: float, exact: bool = False):
    """ops.cpp:28-43."""
    x = _f32(x)
    out = np.zeros_like(x)
    try:
        check(lib().llmi_rms_norm(ptr(out), ptr(x), x.size, float(eps), LLMI_EXACT if exact else 0))
    except LLMIError as e:
        _raise(e)
    return _fill(o, out)


def softmax(x) -> np.ndarray:
    """ops.cpp:45-62 (in place on a copy; returns it)."""
    x = np.array(x, np.float32)
    check(lib().llmi_softmax(ptr(x), x.size))
    return x


def rope(tensor, n_rot: int, rope_freq_base: float, rope_freq_scale: float, pos: int) -> np.ndarray:
    """ops.cpp:67-95; tensor is [n_tokens][n_heads][head_dim]."""
    t = np.array(tensor, np.float32)
    if t.size == 0:
        return t
    nt, nh, hd = t.shape
    check(lib().llmi_rope(ptr(t), nt, nh, hd, n_rot, rope_freq_base, rope_freq_scale, pos))
    return t


def scale(tensor, scale_factor: float) -> np.ndarray:
    """ops.cpp:97-105."""
    t = np.array(tensor, np.float32)
    check(lib().llmi_scale(ptr(t), t.size, scale_factor))
    return t


def vec_scale_f16(y, v: float) -> np.ndarray:
    """ops.cpp:1084-1089 (y: uint16 f16 bits)."""
    y = np.array(y, np.uint16)
    check(lib().llmi_vec_scale_f16(ptr(y), y.size, v))
    return y


def vec_mad_f16(y, x, v: float) -> np.ndarray:
    """ops.cpp:1091-1099."""
    y = np.array(y, np.uint16)
    x = np.ascontiguousarray(x, np.uint16)
    check(lib().llmi_vec_mad_f16(ptr(y), ptr(x), y.size, v))
    return y


def attention(q, k, v, exact: bool = False) -> np.ndarray:
    """Decode attention of Model::run_attn (model.cpp:478-550).
    q: [n_head, hd] f32; k, v: [n_head_kv, n_keys, hd] uint16 f16 bits."""
    q = _f32(q)
    k = np.ascontiguousarray(k, np.uint16)
    v = np.ascontiguousarray(v, np.uint16)
    n_head, hd = q.shape
    n_kv, n_keys, _ = k.shape
    out = np.zeros_like(q)
    check(lib().llmi_attention(ptr(q), ptr(k), ptr(v), n_head, n_kv, n_keys, hd, ptr(out),
                               LLMI_EXACT if exact else 0))
    return out


def gelu_mul(gate, up) -> np.ndarray:
    """GELU(tanh)(gate) * up, model.cpp:892-899."""
    g, u = _f32(gate), _f32(up)
    out = np.zeros_like(g)
    check(lib().llmi_gelu_mul(ptr(g), ptr(u), g.size, ptr(out)))
    return out


def sample_logits(logits, pos: int, temperature: float, top_k: int = 0, top_p: float = 1.0, seed: int = 0,
                  details: bool = False):
    """llmi_sample_logits: one seeded temperature / top-k / top-p draw from a logits row with the decode loop's
    kernels.  Returns the token; details=True: (token, cand, cand_q, n_nucleus) -- the K'
    ordered candidate ids (int32), their integer weights (uint64) and the nucleus size."""
    import ctypes as C
    from ._lib import SAMPLE_MAX_K, Sampler
    lg = _f32(logits).reshape(-1)
    sp = Sampler(temperature, top_k, top_p, seed & 0xFFFFFFFFFFFFFFFF)
    tok = np.zeros(1, np.int32)
    cand = np.zeros(SAMPLE_MAX_K, np.int32)
    cq = np.zeros(SAMPLE_MAX_K, np.uint64)
    nc, nn = C.c_int(), C.c_int()
    check(lib().llmi_sample_logits(ptr(lg), lg.size, C.byref(sp), pos, ptr(tok), ptr(cand), ptr(cq), C.byref(nc),
                                   C.byref(nn)))
    if not details:
        return int(tok[0])
    return int(tok[0]), cand[:nc.value].copy(), cq[:nc.value].copy(), nn.value


def _f16_bits(a) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype == np.uint16:
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(a.astype(np.float16)).view(np.uint16)


def score_rows(x16, w16, targets=None, softcap: float = 0.0):
    """llmi_score_rows: the fused scorer alone.  x16 [T][E] and w16 [V][E] as float16 (or
    their uint16 bits); per row t of x16, from the logits x16[t] . w16[v] (after cap tanh(l / cap) when softcap > 0):
    the log-prob of targets[t] (0.0 for -1 or targets None), the log-sum-exp and the first-index argmax, as a
    ScoreResult.  E % 16 != 0 raises (LLMI_E_SIZE)."""
    from .score import ScoreResult
    x, w = _f16_bits(x16), _f16_bits(w16)
    if x.ndim != 2 or w.ndim != 2 or x.shape[1] != w.shape[1]:
        raise ValueError("score_rows: x16 [T][E] and w16 [V][E]")
    T, E = x.shape
    tg = None if targets is None else np.ascontiguousarray(targets, np.int32)
    if tg is not None and tg.shape != (T,):
        raise ValueError("score_rows: one target per row (-1: none)")
    lp, lse, am = np.zeros(T, np.float32), np.zeros(T, np.float32), np.zeros(T, np.int32)
    check(lib().llmi_score_rows(ptr(x), ptr(w), T, w.shape[0], E, float(softcap), ptr(tg) if tg is not None else None,
                                ptr(lp), ptr(lse), ptr(am)))
    return ScoreResult(lp, lse, am, tg if tg is not None else np.full(T, -1, np.int32))


def logits_rows_rb(E: int) -> int:
    """llmi_logits_rows_rb: the activation rows that share one read of the table in logits_rows at width E (0: the
    width is not supported).  No GPU work."""
    return int(lib().llmi_logits_rows_rb(int(E)))


def logits_rows(x16, w16, softcap: float = 0.0) -> np.ndarray:
    """llmi_logits_rows: the multi-row F16 logits GEMV alone.  x16 [T][E] and w16 [V][E] as
    float16 (or their uint16 bits); returns float32 [T][V] whose row t carries the bits of the fast F16
    mat_vec_mul of w16 with x16[t] (then cap tanh(l / cap) when softcap > 0).  E % 128 != 0 or E > 6144 raises
    (LLMI_E_SIZE)."""
    x, w = _f16_bits(x16), _f16_bits(w16)
    if x.ndim != 2 or w.ndim != 2 or x.shape[1] != w.shape[1]:
        raise ValueError("logits_rows: x16 [T][E] and w16 [V][E]")
    T, E = x.shape
    out = np.zeros((T, w.shape[0]), np.float32)
    check(lib().llmi_logits_rows(ptr(x), ptr(w), T, w.shape[0], E, float(softcap), ptr(out)))
    return out


def logits_rows_gather(x16, w16, idx, cap: int = 64, softcap: float = 0.0, out=None) -> np.ndarray:
    """llmi_logits_rows_gather: the gathered multi-row logits GEMV alone.  x16 [T][E], w16
    [V][E] as logits_rows; idx: at most cap (<= 64) row indices into x16, any order, repeats allowed.  Returns float32
    [cap][V]: row i < len(idx) carries the bits logits_rows gives row idx[i]; the rows at and past len(idx) are those of
    `out` (float32 [cap][V], default zeros), which the kernels must not write."""
    x, w = _f16_bits(x16), _f16_bits(w16)
    if x.ndim != 2 or w.ndim != 2 or x.shape[1] != w.shape[1]:
        raise ValueError("logits_rows_gather: x16 [T][E] and w16 [V][E]")
    T, E = x.shape
    ix = np.ascontiguousarray(idx, np.int32).reshape(-1)
    res = np.zeros((max(int(cap), 0), w.shape[0]), np.float32) if out is None else np.array(out, np.float32, order="C")
    if res.shape != (int(cap), w.shape[0]):
        raise ValueError("logits_rows_gather: out must be [cap][V]")
    check(lib().llmi_logits_rows_gather(ptr(x), ptr(w), T, w.shape[0], E, float(softcap), ptr(ix) if ix.size else None,
                                        ix.size, int(cap), ptr(res)))
    return res


def sample_logits_rows(logits, samplers, sampler_of_row, pos) -> np.ndarray:
    """llmi_sample_logits_rows: the lookup loop's sampler launches over R <= 512 logits rows [R][V] (DESIGN.md section
    16).  samplers: dicts of set_sampler's keywords (temperature > 0); row r draws with samplers[sampler_of_row[r]]
    at position pos[r].  Returns int32 [R]: sample_logits' token per row, -1 for a row with pos < 0."""
    from ._lib import Sampler
    lg = np.ascontiguousarray(logits, np.float32)
    if lg.ndim != 2:
        raise ValueError("sample_logits_rows: logits [R][V]")
    R, V = lg.shape
    of, ps = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (sampler_of_row, pos))
    if of.size != R or ps.size != R:
        raise ValueError("sample_logits_rows: one sampler index and one position per row")
    if R and (of.min() < 0 or of.max() >= len(samplers)):
        raise ValueError("sample_logits_rows: sampler_of_row names a sampler that was not given")
    arr = (Sampler * max(len(samplers), 1))()
    for i, sp in enumerate(samplers):
        arr[i] = Sampler(float(sp["temperature"]), int(sp.get("top_k", 0)), float(sp.get("top_p", 1.0)),
                         int(sp.get("seed", 0)) & 0xFFFFFFFFFFFFFFFF)
    ids = np.zeros(max(R, 1), np.int32)
    check(lib().llmi_sample_logits_rows(ptr(lg), R, V, arr, ptr(of), ptr(ps), ptr(ids)))
    return ids[:R]


def lookup_draft(history, ngram_max: int = 3, ngram_min: int = 1, draft_len: int = 7):
    """llmi_lookup_draft: the lookup loop's draft rule alone, by its kernel.  The draft is the
    continuation of the most recent earlier occurrence of the history's last n tokens, the longest n in
    ngram_max..ngram_min first, wrapping periodically at the history's end.  Returns (draft int32 [0 or draft_len],
    match_end, match_len); no match: (empty, -1, 0)."""
    import ctypes as C
    h = np.ascontiguousarray(history, np.int32).reshape(-1)
    d = np.full(max(int(draft_len), 1), -1, np.int32)
    n, me, ml = C.c_int(), C.c_int(), C.c_int()
    check(lib().llmi_lookup_draft(ptr(h) if h.size else None, h.size, int(ngram_max), int(ngram_min), int(draft_len),
                                  ptr(d), C.byref(n), C.byref(me), C.byref(ml)))
    return d[:n.value].copy(), me.value, ml.value


class DeviceWeight:
    """A GGUF weight uploaded once (llmi_weight_create); multiply many times."""

    def __init__(self, ttype: int, w, n_rows: int, n_cols: int):
        import ctypes as C
        self.ttype, self.n_rows, self.n_cols = ttype, n_rows, n_cols
        w = np.ascontiguousarray(np.frombuffer(w, np.uint8) if not isinstance(w, np.ndarray) else w)
        h = C.c_void_p()
        check(lib().llmi_weight_create(ttype, ptr(w), n_rows, n_cols, C.byref(h)))
        self.h = h

    def __call__(self, x, exact: bool = False) -> np.ndarray:
        x = _f32(x)
        o = np.zeros(self.n_rows, np.float32)
        check(lib().llmi_weight_mat_vec_mul(self.h, ptr(x), x.size, ptr(o), LLMI_EXACT if exact else 0))
        return o

    def dev(self, x_ptr: int, o_ptr: int, stream: Optional[int] = None, exact: bool = False) -> None:
        check(lib().llmi_weight_mat_vec_mul_dev(self.h, x_ptr, o_ptr, LLMI_EXACT if exact else 0, stream))

    def __del__(self):
        if getattr(self, "h", None):
            lib().llmi_weight_destroy(self.h)
            self.h = None
