"""Op-level parity: every kernel the decode graph (and the batched prefill)
launches, checked against the oracle from the DEVICE's own inputs to that
kernel (Model.trace -> llmi_session_trace), so an error in one fused role
cannot hide behind end-to-end drift.

Reference ops restated by the oracle (oracle/llmi_oracle.c, pinned to the
reference's outputs by tests/test_oracle_golden.py):
  embed + scale      model.cpp:240-344        rms_norm / run_norm  ops.cpp:28-43, model.cpp:346-423
  quantize_row_q8_0  ops.cpp:116-139          Q4_0 / Q8_0 GEMV     ops.cpp:188-451, 787-838
  q/k norm, rope     model.cpp:762-794, ops.cpp:67-95             run_attn  model.cpp:430-566
  GELU * up          model.cpp:885-901        residuals           model.cpp:843-858, 915-924
  F16 logits GEMV    ops.cpp:455-612          argmax              main.cpp:193-194

Tolerances (per tensor, why):
  GEMV outputs       |dev - orc| <= 1e-5 * max|orc|: the int8 block dots are
                     exact; only the f32 sum of nb block terms is reassociated
                     (nb * 2^-24 relative to the term magnitude, far below).
  norms / residuals  rtol 2e-6 of max: the squared-sum tree vs the serial fmaf chain.
  attention          vs the float64 restatement 2e-5 of max x sqrt(keys / 256) (fp32 split-K);
                     vs the reference's f16-accumulator algorithm: that algorithm's
                     own drift from exact math (measured on the same inputs) + 4e-5.
  Q8_0 blocks        bit-identical (same floats in, ops.cpp:116-139 exactly).

The batched prefill's non-GEMM kernels (OpChecker.prefill_ops; k_prefill.hip).  Kinds marked [b] hold EVERY
element to a bound and report the worst |dev - ref| / bound (<= 1 passes); the others report a relative error
of max as above; [=] is bit-identity (reported as 0).
  quantised rows [b] a device block (d16, q) of a reference row x_ref known to tol (absolute), d_ref = max|x_ref
                     block| / 127:  |d16 q - x_ref| <= (0.5 + 2^-10) d_ref + |q| (ulp_f16(d16)/2 + tol/127) + tol
                     -- 0.5 d_ref the rounding of x/d to an integer, 2^-10 d_ref the f32 rounding of x (1/d),
                     |q| ulp/2 the f16 rounding of the stored scale, |q| tol/127 the scale's share of the
                     producer's error (tol of the block's largest element).  Q8_K: d = max/127 per 256 elements, an
                     f32 (no f16 term).  f16 rows (x16 2^s = f16(d16 q 2^-s) 2^s): + 2^-11 |x| for the rounding of
                     the 18-bit product d16 q to f16, + 2^-25 2^s where that f16 is subnormal; q and d recovered
                     from the row (the block's largest element is d16 127).  And |q_dev - q_ref| <= 1 wherever
                     tol / d_ref < 0.25 (q_ref: the oracle's quantize_row_q8_0 / _q8_k of x_ref).
  token scales       2^s a power of two; the row's largest |x16| in [2^14, 2^15) widened by 2^-10 (d16 = f16(max/127)
                     and f16(d16 127 2^-s): two f16 roundings); 1 for an all-zero row; no inf / NaN (token_xs).
  pf_norm_in,        the quantised-row bound with tol = NORM_RTOL max|x_ref| (the norm's squared-sum tree); layer
  pf_norm_ffn [b]    0's input is the oracle's embedding row * f32(sqrt(E)), bit-exact arithmetic.
  pf_qk_q, pf_qk_k   |f16 - ref| <= 2^-10 |ref| + NORM_RTOL max|ref| per element (one f16 rounding + the squared-sum
  [b]                tree; the rope tables are the reference's own floats); pf_qk_v [=] f16(v); cache rows past
                     pos0 + T all zero (a fresh session's cache is zero-filled and nothing else writes there).
  pf_attn [b]        the quantised-row bound around the float64 causal attention of the device's f16 q / K / V with
                     tol_i = 2^-11 sum_t p_t |v_ti|                     (P rounded to f16 for the PV MFMA while
                                                                          l_run sums the unrounded p)
                           + 2^-25 sum_t |v_ti| / sum_t e^(s_t - max)   (f16 underflow of tiny p)
                           + max_i sum_t p_t e_t |v_ti - o_i|           (fp32 scores: score_sensitivity's e_t =
                                                                          2 sqrt(hd) 2^-24 sum_i |q_i k_ti|; with
                                                                          a soft-cap + 4 2^-24 |s_t| for tanhf, the
                                                                          division and the product)
                           + ATTN_F64_RTOL sqrt(max(1, keys/256)) max|o| (fp32 split sums, as the decode check)
  pf_resid_attn,     rtol NORM_RTOL of max (norm + one f32 add).
  pf_resid_ffn
  pf_gelu [b]        the quantised-row bound around the oracle's gelu_mul of the de-interleaved gate / up floats
                     with tol = 2^-22 max|hid|: not bit-identical, because the prefill's GELU kernels use the device
                     libm's tanhf (gelu_mul1<EXACT = false>), not glibc's -- Q8_K's f32 d shows the last-place
                     differences that Q8_0's f16 d and the integer quants absorb (OpChecker._gelu_rows).
  pf_tail            logits vs the oracle's output_norm + F16 GEMV of the final residual: GEMV_RTOL + 2 NORM_RTOL.
"""
from __future__ import annotations

import math
from collections import defaultdict

import numpy as np

from llm_inference_amd.gguf import GGUFFile, TensorType as TT

GEMV_RTOL = 1e-5
NORM_RTOL = 2e-6
ATTN_F64_RTOL = 2e-5
GELU_H = {1152: 32, 2560: 40, 3840: 32, 5376: 32}  # k_layer.hip gate/up interleave group by n_embd


def taps_by_layer(taps):
    """[(name, layer, bytes)] -> {(name, layer): [bytes, ...]} in launch order."""
    d = defaultdict(list)
    for name, layer, b in taps:
        d[(name, layer)].append(b)
    return d


def f32(b):
    return np.frombuffer(b, np.float32)


def granule_values(b):
    """{value, tag} 8-B granules -> the 32-bit values (as float32)."""
    return np.frombuffer(b, np.uint32).reshape(-1, 2)[:, 0].copy().view(np.float32)


def xblocks_to_q8_0(words: np.ndarray) -> np.ndarray:
    """Device XBlock rows (48 B: q[32] | d f32 | nsum8 | pad) -> reference
    BlockQ8_0 rows (34 B: d f16 | q[32], ops.h:89-92); checks nsum8."""
    w = np.ascontiguousarray(words, np.uint32).reshape(-1, 12)
    q = w[:, :8].copy().view(np.int8).reshape(-1, 32)
    d = w[:, 8].copy().view(np.float32)
    d16 = d.astype(np.float16)
    assert np.array_equal(d16.astype(np.float32), d), "XBlock scale is not an f16 value"
    nsum8 = w[:, 9].view(np.int32)
    assert np.array_equal(nsum8, -8 * q.astype(np.int32).sum(1)), "XBlock nsum8 != -8 sum(q)"
    out = np.zeros((w.shape[0], 34), np.uint8)
    out[:, :2] = d16.view(np.uint8).reshape(-1, 2)
    out[:, 2:] = q.view(np.uint8)
    return out.reshape(-1)


def xblocks_q8k_to_f32(words: np.ndarray) -> np.ndarray:
    """Device XBlock rows holding Q8_K quants (q8k_block_quad: d = the super-block's f32 d, nsum8 = the
    block's sum of q) -> x' = d q in f32; the reference's quantize_row_q8_k (ops.cpp:142-178) of x' gives back
    the same quants (its max element is d * (+-127)), so mat_vec_mul(w, x') is the reference's row dot on
    these blocks (to one ulp of d)."""
    w = np.ascontiguousarray(words, np.uint32).reshape(-1, 12)
    q = w[:, :8].copy().view(np.int8).reshape(-1, 32)
    d = w[:, 8].copy().view(np.float32)
    assert np.array_equal(w[:, 9].view(np.int32), q.astype(np.int32).sum(1)), "XBlock nsum8 != sum(q)"
    assert np.array_equal(d.reshape(-1, 8), np.repeat(d.reshape(-1, 8)[:, :1], 8, 1)), "Q8_K d differs in a super-block"
    mx, dsb = np.abs(q.reshape(-1, 256)).max(1), d.reshape(-1, 8)[:, 0]
    bad = np.nonzero((mx < 127) & ((dsb != 0) | (mx != 0)))[0]  # an all-zero x gives d = 0 and zero quants
    assert bad.size == 0, f"Q8_K super-blocks {bad[:8].tolist()} without a +-127 quant (max |q| {mx[bad[:8]].tolist()}, d {dsb[bad[:8]].tolist()})"
    return (d[:, None] * q.astype(np.float32)).astype(np.float32).reshape(-1)


def score_sensitivity(q, kc, vc):
    """First-order bound on the relative change of one head's exact attention output when every score carries
    an fp32-sized error e_t = 2 sqrt(hd) 2^-24 sum_i |q16_i k_ti|: max_i sum_t p_t e_t |v_ti - o_i| / max |o|."""
    q16 = np.asarray(q, np.float32).astype(np.float16).astype(np.float64)
    K = np.asarray(kc).view(np.float16).astype(np.float64)
    V = np.asarray(vc).view(np.float16).astype(np.float64)
    sc = K @ q16
    p = np.exp(sc - sc.max())
    p /= p.sum()
    o = p @ V
    e = 2.0 * math.sqrt(q16.size) * 2.0 ** -24 * (np.abs(K) @ np.abs(q16))
    return float(((p * e)[:, None] * np.abs(V - o[None, :])).sum(0).max() / max(float(np.abs(o).max()), 1e-30))


def rel_err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(float(np.abs(ref).max()), 1e-30))


def f16_ulp(d):
    """Spacing of the f16 grid at |d| (2^-24 in the subnormal range)."""
    return np.spacing(np.abs(np.asarray(d, np.float64)).astype(np.float16)).astype(np.float64)


def attn_key_splits(hd, G):
    """Key tiles per round of prefill_attn_mfma_kernel (the launcher's S: attn_g in k_prefill.hip)."""
    return 2 if hd >= 256 or (G == 4 and hd == 128) else 4


def attn_check_tokens(T, pos0, S, t0=0):
    """The query tokens prefill_ops checks: every token of the first and the last 32-query block and of each
    block whose number of key rounds (ceil(key tiles / S)) differs from the block's before it; every eighth
    token elsewhere; nothing before t0 (the last layer's trim)."""
    nqb = (T + 31) // 32
    rounds = [((pos0 + min(32 * b + 32, T) - 1) // 32 + 1 + S - 1) // S for b in range(nqb)]
    full = {0, nqb - 1} | {b for b in range(1, nqb) if rounds[b] != rounds[b - 1]}
    return [t for t in range(t0, T) if t // 32 in full or t % 8 == 0]


def act_rows(D, l, proj, n_t, xs, ncols, kq):
    """One pf_x_<proj> tap of n_t token rows (xs activation blocks each), its format from its size: XBlocks (48
    B: Q8_K quants on K-quant layers, else Q8_0; the blocks' invariants asserted) or f16 rows with the token
    scales 2^s of the pf_xs_<proj> tap (the attention's rows have none: 1)."""
    b = D[(f"pf_x_{proj}", l)][-1]
    rb = len(b) // n_t
    assert rb * n_t == len(b) and rb in (48 * xs, 64 * xs), f"activation rows of {len(b)} B for {n_t} tokens"
    if rb == 64 * xs:
        x16 = np.frombuffer(b, np.float16).reshape(n_t, xs * 32)[:, :ncols].astype(np.float64)
        assert np.isfinite(x16).all(), "token scales: an inf or NaN in an f16 row"
        ts = np.ones(n_t)
        if (f"pf_xs_{proj}", l) in D:
            ts = f32(D[(f"pf_xs_{proj}", l)][-1]).astype(np.float64)
            assert ts.size == n_t and np.all(ts > 0) and np.all(np.frexp(ts)[0] == 0.5), "token scales: powers of two"
            mx = np.abs(x16).max(1)
            ok = np.where(mx == 0, ts == 1.0, (mx >= 2.0 ** 14 * (1 - 2.0 ** -10)) & (mx < 2.0 ** 15 * (1 + 2.0 ** -10)))
            bad = np.nonzero(~ok)[0]
            assert bad.size == 0, (f"token scales: rows {bad[:8].tolist()} with max |x16| {mx[bad[:8]].tolist()} "
                                   f"outside [2^14, 2^15) (2^s {ts[bad[:8]].tolist()})")
        return {"kind": "f16", "x16": x16, "ts": ts, "bits": np.frombuffer(b, np.uint16).reshape(n_t, xs * 32)[:, :ncols]}
    w = np.ascontiguousarray(np.frombuffer(b, np.uint32).reshape(n_t, xs, 12)[:, : ncols // 32])
    (xblocks_q8k_to_f32 if kq else xblocks_to_q8_0)(w)  # the blocks' invariants
    return {"kind": "q8_k" if kq else "q8_0", "words": w,
            "q": w[:, :, :8].copy().view(np.int8).reshape(n_t, -1, 32).astype(np.float64),
            "d": w[:, :, 8].copy().view(np.float32).astype(np.float64)}


def quant_errors(R, x_ref, tol):
    """The quantisation-aware bound (module docstring): rows R (act_rows) against the reference rows x_ref
    [n_t][n] known to tol (absolute; a scalar, per row or per element).  Returns |dev - ref|, the bound, the
    device's quants times the sign of d, and the per-block mask tol / d_ref < 0.25."""
    n_t, n = x_ref.shape
    B = 256 if R["kind"] == "q8_k" else 32
    xr = np.asarray(x_ref, np.float64).reshape(n_t, n // B, B)
    tl = np.broadcast_to(np.asarray(tol, np.float64), (n_t, n)).reshape(xr.shape)
    d_ref = np.abs(xr).max(-1) / 127.0
    tol_b = tl.max(-1)
    extra = 0.0
    if R["kind"] == "f16":  # recover (d, q) of every block: its largest element is f16(d16 127 2^-s)
        x16 = R["x16"].reshape(xr.shape)
        ts = R["ts"][:, None]
        m = np.abs(x16).max(-1)
        ms = np.where(m > 0, m, 1.0)[..., None]
        qf = 127.0 * x16 / ms
        q = np.rint(qf)
        # x16 / m = (q / 127) (1 + e1) / (1 + e2), |e| <= 2^-11 (+ 2^-25 absolute where x16 is subnormal)
        assert np.all(np.abs(qf - q) <= np.abs(q) * 2.0 ** -10 * 1.001 + 127.0 * 2.0 ** -25 * 1.001 / ms), \
            "an f16 row is not f16(d q) of Q8_0 blocks"
        d = m * ts / 127.0
        xd = x16 * ts[..., None]
        extra = 2.0 ** -11 * np.abs(xd) + 2.0 ** -25 * ts[..., None]
        ulp = f16_ulp(d * (1 + 2.0 ** -10)) / 2  # d16 = f16(max / 127) is m 2^s / 127 to 2^-11: never the finer binade
    elif R["kind"] == "q8_0":
        q, d = R["q"], R["d"]
        xd = d[..., None] * q
        ulp = f16_ulp(d) / 2
    else:
        q = R["q"].reshape(xr.shape)
        d = R["d"][:, ::8]
        xd = d[..., None] * q
        ulp = np.zeros_like(d)
    bound = (0.5 + 2.0 ** -10) * d_ref[..., None] + np.abs(q) * (ulp + tol_b / 127.0)[..., None] + tl + extra
    near = (d_ref > 0) & (tol_b < 0.25 * d_ref)
    return np.abs(xd - xr), bound, q * np.where(d < 0, -1.0, 1.0)[..., None], near


class Weights:
    """Raw GGUF weights of a synthetic Gemma-3 file, by reference tensor name."""

    def __init__(self, buf: np.ndarray):
        self.g = GGUFFile(buf)

    def raw(self, name):
        t = self.g.tensor(name)
        return (np.frombuffer(self.g.get_tensor_data(t), np.uint8), t.tensor_type,
                int(t.shape[1]) if len(t.shape) > 1 else 1, int(t.shape[0]))

    def f32(self, name):
        return self.raw(name)[0].view(np.float32)

    def qkv(self, l):
        """q|k|v stacked as one weight (the session's fused qkv rows)."""
        parts = [self.raw(f"blk.{l}.attn_{p}.weight") for p in "qkv"]
        return np.concatenate([p[0] for p in parts]), parts[0][1], sum(p[2] for p in parts), parts[0][3]


class OpChecker:
    """Checks one traced decode step (or prefill) op by op; records the
    worst relative error per tensor kind in self.report."""

    def __init__(self, oracle, buf, cfg, max_ctx, threads=16, swa_pattern=None, softcap=0.0, gelu_h=None):
        """buf: the GGUF file's bytes, or an object with Weights' raw() / f32() (a test's stand-in); softcap: the
        file's attention.logit_softcapping; gelu_h: the gate/up interleave group where n_embd is not in GELU_H."""
        self.orc, self.cfg, self.max_ctx, self.th = oracle, cfg, max_ctx, threads
        self.swa_pattern = swa_pattern
        self.softcap, self.gelu_h = float(softcap), gelu_h
        self.w = buf if hasattr(buf, "raw") else Weights(buf)
        self.eps = float(np.float32(cfg.eps))
        self.report = defaultdict(float)

    def note(self, kind, err, tol):
        self.report[kind] = max(self.report[kind], err)
        assert err <= tol, f"{kind}: relative error {err:.3g} > {tol:.1g}"

    def norm(self, x, wname):  # run_norm: rms_norm then a separate multiply by the weight
        return self.orc.rms_norm(x, self.eps) * self.w.f32(wname)

    def gemv(self, w, x):
        data, tt, rows, cols = w
        return self.orc.mat_vec_mul(tt, data, rows, cols, x, self.th)

    def gemv_q8(self, w, xq34):
        data, tt, rows, cols = w
        return self.orc.mat_vec_mul_q8(tt, data, rows, cols, xq34, self.th)

    def swa(self, l):  # model.cpp:723-729: the file's pattern, else 5 local layers per global one
        return bool(self.swa_pattern[l]) if self.swa_pattern is not None else (l % 6) < 5

    def attention(self, l, qkv, kc, vc, pos, attn_dev):
        """q/k norm + rope + scale from the device's q|k|v rows, the device's KV
        cache (its row at pos checked against f16 of the oracle's k/v), then
        every head against both attention restatements."""
        c = self.cfg
        hd, nh, nkv = c.head_dim, c.n_head, c.n_head_kv
        q = qkv[: nh * hd].reshape(nh, hd)
        k = qkv[nh * hd: (nh + nkv) * hd].reshape(nkv, hd)
        v = qkv[(nh + nkv) * hd:].reshape(nkv, hd)
        base = 10000.0 if self.swa(l) else c.rope_base
        qn = np.stack([self.norm(q[h], f"blk.{l}.attn_q_norm.weight") for h in range(nh)])
        kn = np.stack([self.norm(k[h], f"blk.{l}.attn_k_norm.weight") for h in range(nkv)])
        qr = self.orc.rope(qn[None], hd, base, 1.0, pos)[0] * np.float32(1.0 / math.sqrt(hd))
        kr = self.orc.rope(kn[None], hd, base, 1.0, pos)[0]
        kc = kc.reshape(nkv, self.max_ctx, hd)
        vc = vc.reshape(nkv, self.max_ctx, hd)
        k16 = kc[:, pos].view(np.float16).astype(np.float32)
        self.note("kv_append_k", rel_err(k16, kr.astype(np.float16).astype(np.float32)), 2e-3)
        assert np.array_equal(vc[:, pos], v.astype(np.float16).view(np.uint16)), "V row at pos != f16(v)"
        g = nh // nkv
        got = attn_dev.reshape(nh, hd)
        ref64 = np.stack([self.orc.attn_head_f64(qr[h], kc[h // g, : pos + 1], vc[h // g, : pos + 1]) for h in range(nh)])
        refr = np.stack([self.orc.attn_head(qr[h], kc[h // g, : pos + 1], vc[h // g, : pos + 1]) for h in range(nh)])
        # fp32 split-K sums: rounding grows like sqrt(keys) (2e-5 up to 256 keys); plus the first-order effect of
        # fp32 scores (an error of ~2 sqrt(hd) 2^-24 sum_i |q_i k_i| per key, through p_t |v_t - o|): large
        # scores (centered K-quant weights) make the exact softmax itself that sensitive
        sens = max(score_sensitivity(qr[h], kc[h // g, : pos + 1], vc[h // g, : pos + 1]) for h in range(nh))
        self.report["attention_score_sensitivity"] = max(self.report["attention_score_sensitivity"], sens)
        self.note("attention_vs_f64", rel_err(got, ref64), ATTN_F64_RTOL * math.sqrt(max(1.0, (pos + 1) / 256.0)) + sens)
        # the reference's own f16 V accumulator drifts from exact math with the
        # key count (~1e-3 at 256 keys, ~7e-3 at 1100): the fast path may differ
        # from it by that drift plus its own distance to exact math
        ref_drift = rel_err(refr, ref64)
        self.report["reference_attention_drift"] = max(self.report["reference_attention_drift"], ref_drift)
        self.note("attention_vs_reference", rel_err(got, refr), ref_drift * 1.01 + 2 * ATTN_F64_RTOL)

    def q8k_blocks(self, words, x, what):
        """Device XBlocks holding Q8_K quants vs the reference's quantize_row_q8_k of x (ops.cpp:142-178),
        bit for bit: per 256-element super-block the f32 d and the 256 quants; returns x' = d q (f32)."""
        xf = xblocks_q8k_to_f32(words)
        w = np.ascontiguousarray(words, np.uint32).reshape(-1, 12)
        ref = np.frombuffer(self.orc.quantize_q8_k(x), np.uint8).reshape(-1, 292)
        assert np.array_equal(w[:, :8].copy().view(np.int8).reshape(-1, 256), ref[:, 4:260].view(np.int8)), \
            f"{what}: Q8_K quants"
        assert np.array_equal(w[:, 8].copy().view(np.float32).reshape(-1, 8)[:, 0], ref[:, :4].copy().view(np.float32)[:, 0]), \
            f"{what}: Q8_K d"
        return xf

    def decode_step(self, taps, pos, gen, token=None):
        """One traced decode step (llmi_session_trace, n_tokens = 1).  Q4_0 / Q8_0 layers read Q8_0 activation
        blocks; K-quant layers (Q4_K / Q6_K in the kq layout) read Q8_K blocks, checked against the reference's
        quantize_row_q8_k and dotted through the reference's mat_vec_mul_q4_k / _q6_k."""
        c = self.cfg
        E, F = c.n_embd, c.n_ff
        T = taps_by_layer(taps)
        one = lambda n, l: T[(n, l)][-1]
        block = ("qkv_g", 0) in T
        kq = self.w.raw("blk.0.attn_q.weight")[1] in (TT.Q4_K, TT.Q6_K)
        for l in range(c.n_layer):
            x = f32(one("attn_norm", l))
            if l == 0:
                if token is not None:  # embed_tokens + scale_embeddings (model.cpp:240-344), then attn_norm
                    data, tt, rows, cols = self.w.raw("token_embd.weight")
                    row = self.orc.dequantize_row(tt, data[token * (data.size // rows):(token + 1) * (data.size // rows)], cols)
                    emb = row * np.float32(math.sqrt(E))
                    assert np.array_equal(f32(one("inp_scaled", -1)), emb), "embedding row * sqrt(n_embd)"
                self.note("norm", rel_err(x, self.norm(f32(one("inp_scaled", -1)), "blk.0.attn_norm.weight")), NORM_RTOL)
            else:
                r_prev = f32(one("ffn_resid", l - 1))
                y = f32(one("down", l - 1))
                r = r_prev + self.norm(y, f"blk.{l - 1}.post_ffw_norm.weight")
                got_r = f32(one("attn_resid", l))
                self.note("residual", rel_err(got_r, r), NORM_RTOL)
                self.note("norm", rel_err(x, self.norm(got_r, f"blk.{l}.attn_norm.weight")), NORM_RTOL)
            wqkv = self.w.qkv(l)
            qkv = granule_values(one("qkv_g", l)) if block else f32(one("qkv", l))
            if kq:  # q, k, v per tensor (Q4_K_M: q|k Q4_K, v Q6_K); every row's dot is independent of the stacking
                xin = x
                if l == 0 and ("xq", 0) in T:  # layer 0 reads embed_norm's block_q8_K rows (292 B, ops.h:18-23)
                    b = np.frombuffer(one("xq", 0), np.uint8)
                    assert b.size == E // 256 * 292 and np.array_equal(b, self.orc.quantize_q8_k(x)), "embed_norm Q8_K blocks"
                    sb = b.reshape(-1, 292)
                    xin = (sb[:, :4].copy().view(np.float32) * sb[:, 4:260].view(np.int8).astype(np.float32)).reshape(-1)
                ref = np.concatenate([self.gemv(self.w.raw(f"blk.{l}.attn_{p}.weight"), xin) for p in "qkv"])
            elif l == 0 and ("xq", 0) in T:  # layer 0 reads embed_norm's Q8_0 blocks
                xq = xblocks_to_q8_0(np.frombuffer(one("xq", 0), np.uint32))
                assert np.array_equal(xq, self.orc.quantize_q8_0(x)), "embed_norm Q8_0 blocks"
                ref = self.gemv_q8(wqkv, xq)
            else:
                ref = self.gemv(wqkv, x)
            self.note("gemv_qkv", rel_err(qkv, ref), GEMV_RTOL)
            attn = f32(one("attn", l))
            self.attention(l, qkv, np.frombuffer(one("kc", l), np.uint16), np.frombuffer(one("vc", l), np.uint16),
                           pos, attn)
            xo_words = granule_values(one("xo_g", l)).view(np.uint32) if block else np.frombuffer(one("xo", l), np.uint32)
            o = f32(one("o", l))
            if kq:
                xof = self.q8k_blocks(xo_words[: c.n_head * c.head_dim // 32 * 12], attn, f"layer {l}: attention")
                self.note("gemv_o", rel_err(o, self.gemv(self.w.raw(f"blk.{l}.attn_output.weight"), xof)), GEMV_RTOL)
            else:
                xo = xblocks_to_q8_0(xo_words)
                assert np.array_equal(xo, self.orc.quantize_q8_0(attn)), f"layer {l}: attention Q8_0 blocks"
                self.note("gemv_o", rel_err(o, self.gemv_q8(self.w.raw(f"blk.{l}.attn_output.weight"), xo)), GEMV_RTOL)
            r_in = f32(one("attn_resid", l)) if l else f32(one("inp_scaled", -1))
            r2 = r_in + self.norm(o, f"blk.{l}.post_attention_norm.weight")
            got_r2 = f32(one("ffn_resid", l))
            self.note("residual", rel_err(got_r2, r2), NORM_RTOL)
            xf = f32(one("ffn_norm", l))
            self.note("norm", rel_err(xf, self.norm(got_r2, f"blk.{l}.ffn_norm.weight")), NORM_RTOL)
            gate = self.gemv(self.w.raw(f"blk.{l}.ffn_gate.weight"), xf)
            up = self.gemv(self.w.raw(f"blk.{l}.ffn_up.weight"), xf)
            hid = f32(one("hid", l))
            assert np.abs(hid).max() > 0, f"layer {l}: the FFN is dead (GELU output all zero): the check would be vacuous"
            # GELU(g) * u with g, u each within GEMV_RTOL of max: |d hid| <~ (|GELU'| + 1) max|g| max|u| GEMV_RTOL
            err = float(np.abs(hid - self.orc.gelu_mul(gate, up)).max()) / (float(np.abs(gate).max() * np.abs(up).max()) + 1e-30)
            self.note("gemv_gate_up_gelu", err, 3 * GEMV_RTOL)
            d = f32(one("down", l))
            self.note("gemv_down", rel_err(d, self.gemv(self.w.raw(f"blk.{l}.ffn_down.weight"), hid)), GEMV_RTOL)
        rf = f32(one("ffn_resid", c.n_layer - 1)) + self.norm(f32(one("down", c.n_layer - 1)),
                                                              f"blk.{c.n_layer - 1}.post_ffw_norm.weight")
        self.note("residual", rel_err(f32(one("final_resid", -1)), rf), NORM_RTOL)
        xn = f32(one("result_norm", -1))
        self.note("norm", rel_err(xn, self.norm(f32(one("final_resid", -1)), "output_norm.weight")), NORM_RTOL)
        logits = self.gemv(self.w.raw("token_embd.weight"), xn)
        if ("logits", -1) in T:
            self.note("gemv_logits_f16", rel_err(f32(one("logits", -1)), logits), GEMV_RTOL)
        tok = int(np.frombuffer(one("token", -1), np.int32)[0])
        top = np.sort(logits)[-2:]
        if top[1] - top[0] > 1e-5 * abs(top[1]):  # not a near-tie at f32 resolution: the id is determined
            assert tok == int(np.argmax(logits)), f"token {tok} vs oracle argmax {int(np.argmax(logits))}"
        return tok

    def prefill(self, taps, T_tok):
        """Traced batched prefill: every projection GEMM, token by token, from
        the device's own inputs -- Q8_0 blocks (int8 GEMM v5 vs the reference's
        per-token mat_vec_mul rows, GEMV tolerance) or f16 rows (the f16 GEMMs v7 /
        v6 vs the exactly dequantized weights times those f16 values, times the
        token's scale 2^s, in float64: the kernel's weights are f16(d (q - 8)),
        PREFILL16_RTOL).  Each tap's format from its size: the f16 path's last
        layer runs its one remaining token on the int8 path."""
        c = self.cfg
        E, F = c.n_embd, c.n_ff
        D = taps_by_layer(taps)
        H = GELU_H[E]
        xs = max(E, F, c.n_head * c.head_dim) // 32  # activation blocks per token (session pf_xs_)
        row_bytes = len(D[("pf_x_qkv", 0)][-1]) // T_tok
        assert row_bytes in (48 * xs, 64 * xs), f"prefill activation row of {row_bytes} B"
        for l in range(c.n_layer):
            for proj, names, ncols in (("qkv", [f"blk.{l}.attn_{p}.weight" for p in "qkv"], E),
                                       ("o", [f"blk.{l}.attn_output.weight"], c.n_head * c.head_dim),
                                       ("gate_up", None, E),
                                       ("down", [f"blk.{l}.ffn_down.weight"], F)):
                nbytes = len(D[(f"pf_x_{proj}", l)][-1])
                f16_rows = nbytes % (64 * xs) == 0 and (nbytes // (64 * xs) == T_tok or nbytes == 64 * xs)
                if f16_rows and row_bytes == 64 * xs:
                    self._prefill_f16_one(D, l, proj, names, ncols, nbytes // (64 * xs), H)
                else:
                    self._prefill_q8_one(D, l, proj, names, ncols, nbytes // (48 * xs), H)

    def bound(self, kind, err, bnd, what=""):
        """Every element's |dev - ref| within its bound; reports the worst err / bound."""
        err, bnd = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bnd, np.float64), np.shape(err))
        assert np.isfinite(err).all(), f"{kind}: {what}: a non-finite value"
        ratio = np.where(err > 0, err / np.maximum(bnd, 1e-300), 0.0)
        worst = float(ratio.max()) if ratio.size else 0.0
        self.report[kind] = max(self.report[kind], worst)
        if worst > 1.0:
            i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            raise AssertionError(f"{kind}: {what} element {tuple(int(j) for j in i)}: |dev - ref| {err[i]:.6g} > bound "
                                 f"{bnd[i]:.6g} ({int((ratio > 1).sum())} of {ratio.size} elements out)")

    def quant_rows(self, kind, D, l, proj, n_t, ncols, x_ref, tol):
        """pf_x_<proj> of layer l is an acceptable quantisation of the rows x_ref (the quantisation-aware bound of
        the module docstring, every element; the quants within 1 of the oracle's where tol / d_ref < 0.25)."""
        what = f"layer {l} pf_x_{proj}"
        c = self.cfg
        xs = max(c.n_embd, c.n_ff, c.n_head * c.head_dim) // 32  # activation blocks per token (session pf_xs_)
        try:
            R = act_rows(D, l, proj, n_t, xs, ncols, self.kq)
            err, bnd, qs, near = quant_errors(R, x_ref, tol)
        except AssertionError as e:
            raise AssertionError(f"{kind}: {what}: {e}") from None
        self.bound(kind, err, bnd, what)
        x32 = np.ascontiguousarray(x_ref, np.float32)
        if R["kind"] == "q8_k":
            ref = np.stack([np.frombuffer(self.orc.quantize_q8_k(r), np.uint8).reshape(-1, 292) for r in x32])
            q_ref = ref[:, :, 4:260].copy().view(np.int8).astype(np.float64)
            q_ref = q_ref * np.where(ref[:, :, :4].copy().view(np.float32) < 0, -1.0, 1.0)
        else:
            ref = np.stack([np.frombuffer(self.orc.quantize_q8_0(r), np.uint8).reshape(-1, 34) for r in x32])
            q_ref = ref[:, :, 2:].copy().view(np.int8).astype(np.float64)
        dq = np.abs(qs - q_ref) * near[..., None]
        assert dq.max() <= 1, f"{kind}: {what}: a quant {int(dq.max())} from the oracle's where tol < d_ref / 4"
        self.report[kind + "_rows_" + R["kind"]] = max(self.report[kind + "_rows_" + R["kind"]], float(dq.max()))
        return R

    def norm_rows(self, x, wname):
        return np.stack([self.norm(r, wname) for r in np.ascontiguousarray(x, np.float32)])

    def prefill_ops(self, taps, tokens, pos0):
        """One traced batched prefill of a single chunk (tokens at positions pos0.., T <= 512: one tap per name
        and layer): every non-GEMM launch of k_prefill.hip from the device's own tapped input to it, against
        float64 / the oracle -- the kinds, bounds and their derivations in the module docstring.  Per layer:
        pf_norm_in (embedding or residual -> attn_norm rows), pf_qk_q / _k / _v (q/k norm, rope with the layer's
        base, q scale, K/V append; cache rows past pos0 + T untouched: zero, a fresh session's cache being
        zero-filled), pf_attn, pf_resid_attn, pf_norm_ffn, pf_gelu, pf_resid_ffn; then pf_tail (final residual,
        output_norm, logits, token).  The last layer past its K/V append runs on the final token only (t0 = T - 1,
        and on the int8 path for Q4_0 / Q8_0 layers): the row counts and formats follow from the tap sizes.

        pf_attn checks every query token of the first and the last 32-query block and of each block in which
        the number of key rounds changes, every eighth token elsewhere (attn_check_tokens)."""
        c = self.cfg
        E, F, hd, nh, nkv, L = c.n_embd, c.n_ff, c.head_dim, c.n_head, c.n_head_kv, c.n_layer
        tokens = np.asarray(tokens, np.int64)
        T, g = tokens.size, nh // nkv
        assert 2 <= T <= 512, "one chunk of the batched prefill"
        D = taps_by_layer(taps)
        for (name, _l), v in D.items():
            assert not name.startswith("pf_") or len(v) == 1, f"{name}: {len(v)} taps (one chunk, no int8 redo)"
        self.kq = self.w.raw("blk.0.attn_q.weight")[1] in (TT.Q4_K, TT.Q6_K)
        H = self.gelu_h or GELU_H[E]
        S = attn_key_splits(hd, g)
        data, tt, rows, cols = self.w.raw("token_embd.weight")
        rb = data.size // rows
        resid = np.stack([self.orc.dequantize_row(tt, data[t * rb:(t + 1) * rb], cols) for t in tokens]) \
            * np.float32(math.sqrt(E))  # embed_tokens + scale_embeddings (model.cpp:240-344), bit-exact
        for l in range(L):
            t0 = T - 1 if l == L - 1 else 0  # the last layer's trim
            Tq = T - t0
            # 1. attn_norm rows
            xr = self.norm_rows(resid, f"blk.{l}.attn_norm.weight").astype(np.float64)
            self.quant_rows("pf_norm_in", D, l, "qkv", T, E, xr, NORM_RTOL * np.abs(xr).max(1, keepdims=True))
            # 2. q/k norm, rope, q scale, K/V append
            qkv = f32(D[("pf_qkv", l)][0]).reshape(T, (nh + 2 * nkv) * hd)
            base = 10000.0 if self.swa(l) else c.rope_base
            qn = self.norm_rows(qkv[:, : nh * hd].reshape(-1, hd), f"blk.{l}.attn_q_norm.weight").reshape(T, nh, hd)
            kn = self.norm_rows(qkv[:, nh * hd:(nh + nkv) * hd].reshape(-1, hd), f"blk.{l}.attn_k_norm.weight").reshape(T, nkv, hd)
            qr = (self.orc.rope(qn, hd, base, 1.0, pos0) * np.float32(1.0 / math.sqrt(hd))).astype(np.float64)
            kr = self.orc.rope(kn, hd, base, 1.0, pos0).astype(np.float64)
            v = qkv[:, (nh + nkv) * hd:].reshape(T, nkv, hd)
            q16 = np.frombuffer(D[("pf_q", l)][0], np.float16).reshape(T, nh, hd).astype(np.float64)
            kc = np.frombuffer(D[("kc", l)][-1], np.uint16).reshape(nkv, self.max_ctx, hd)
            vc = np.frombuffer(D[("vc", l)][-1], np.uint16).reshape(nkv, self.max_ctx, hd)
            k16 = kc[:, pos0:pos0 + T].view(np.float16).astype(np.float64).transpose(1, 0, 2)
            for kind, got, ref in (("pf_qk_q", q16, qr), ("pf_qk_k", k16, kr)):
                self.bound(kind, np.abs(got - ref), 2.0 ** -10 * np.abs(ref) + NORM_RTOL * np.abs(ref).max(-1, keepdims=True),
                           f"layer {l} (token, head, dim)")
            assert np.array_equal(vc[:, pos0:pos0 + T].transpose(1, 0, 2), v.astype(np.float16).view(np.uint16)), \
                f"pf_qk_v: layer {l}: V cache rows pos0.. != f16(v)"
            self.report["pf_qk_v"] = max(self.report["pf_qk_v"], 0.0)
            assert not kc[:, pos0 + T:].any() and not vc[:, pos0 + T:].any(), \
                f"pf_qk_untouched: layer {l}: a cache row past pos0 + T was written"
            # 3. causal attention in float64 from the device's f16 q / K / V
            sel = attn_check_tokens(T, pos0, S, t0)
            o_ref, o_tol = self.attn_f64(q16[sel], kc, vc, pos0 + np.asarray(sel))
            ro = np.asarray(sel) - t0
            R = self._attn_rows(D, l, Tq, ro, nh * hd)
            try:
                err, bnd, qs, near = quant_errors(R, o_ref.reshape(len(sel), -1), o_tol.reshape(len(sel), -1))
            except AssertionError as e:
                raise AssertionError(f"pf_attn: layer {l}: {e}") from None
            self.bound("pf_attn", err, bnd, f"layer {l} (checked query, block, element)")
            self.report["pf_attn_rows_" + R["kind"]] = 0.0
            # 4. post-attention norm + residual
            o = f32(D[("pf_o", l)][0]).reshape(Tq, E)
            ra = f32(D[("pf_resid_attn", l)][0]).reshape(Tq, E)
            ref = resid[t0:] + self.norm_rows(o, f"blk.{l}.post_attention_norm.weight")
            for t in range(Tq):
                self.note("pf_resid_attn", rel_err(ra[t], ref[t].astype(np.float64)), NORM_RTOL)
            # 5. ffn_norm rows
            xr = self.norm_rows(ra, f"blk.{l}.ffn_norm.weight").astype(np.float64)
            self.quant_rows("pf_norm_ffn", D, l, "gate_up", Tq, E, xr, NORM_RTOL * np.abs(xr).max(1, keepdims=True))
            # 6. GELU(gate) * up, de-interleaved by H, bit for bit
            gu = f32(D[("pf_gate_up", l)][0]).reshape(Tq, F // H, 2, H)
            hid = np.stack([self.orc.gelu_mul(r[:, 0].reshape(-1), r[:, 1].reshape(-1)) for r in gu])
            assert np.abs(hid).max() > 0, f"pf_gelu: layer {l}: the FFN is dead (GELU output all zero)"
            self._gelu_rows(D, l, Tq, F, hid)
            # 7. post-ffw norm + residual (before the last layer: every token)
            dn = f32(D[("pf_down", l)][0]).reshape(Tq, E)
            if l + 1 < L:
                rf = f32(D[("pf_resid_ffn", l)][0]).reshape(T, E)
                ref = ra + self.norm_rows(dn, f"blk.{l}.post_ffw_norm.weight")
                for t in range(T):
                    self.note("pf_resid_ffn", rel_err(rf[t], ref[t].astype(np.float64)), NORM_RTOL)
                resid = rf
        # 8. the tail: final residual -> output_norm -> F16 logits GEMV -> token
        final = ra[0] + self.norm(dn[0], f"blk.{L - 1}.post_ffw_norm.weight")
        logits = self.gemv(self.w.raw("token_embd.weight"), self.norm(final, "output_norm.weight"))
        if ("logits", -1) in D:
            self.note("pf_tail", rel_err(f32(D[("logits", -1)][-1]), logits.astype(np.float64)), GEMV_RTOL + 2 * NORM_RTOL)
        if ("token", -1) in D:
            tok = int(np.frombuffer(D[("token", -1)][-1], np.int32)[0])
            top = np.sort(logits)[-2:]
            if top[1] - top[0] > 1e-5 * abs(top[1]):  # decode_step's near-tie rule
                assert tok == int(np.argmax(logits)), f"pf_tail: token {tok} vs oracle argmax {int(np.argmax(logits))}"

    def attn_f64(self, q, kc, vc, qpos):
        """Float64 causal attention of the queries q [n][heads][hd] (scaled, f16 values) at positions qpos over
        the cache's keys 0..qpos: scores, the soft-cap c tanh(s / c) before the mask, softmax, P V; and the
        per-element tolerance tol_i of the module docstring (pf_attn).  Returns o, tol as [n][heads][hd]."""
        n, nh, hd = q.shape
        nkv = kc.shape[0]
        g, cap = nh // nkv, self.softcap
        nk = int(qpos.max()) + 1
        o, tol = np.zeros((n, nh, hd)), np.zeros((n, nh, hd))
        mask = np.arange(nk)[None, :] <= qpos[:, None]
        for h in range(nh):
            K = kc[h // g, :nk].view(np.float16).astype(np.float64)
            V = vc[h // g, :nk].view(np.float16).astype(np.float64)
            s = q[:, h] @ K.T
            if cap > 0.0:
                s = cap * np.tanh(s / cap)
            sm = np.where(mask, s, -np.inf)
            e = np.exp(sm - sm.max(1, keepdims=True))
            lsum = e.sum(1, keepdims=True)
            p = e / lsum
            oh = p @ V
            es = 2.0 * math.sqrt(hd) * 2.0 ** -24 * (np.abs(q[:, h]) @ np.abs(K).T)
            if cap > 0.0:
                es = es + 4.0 * 2.0 ** -24 * np.abs(s)
            sens = np.stack([((p[i] * es[i])[:, None] * np.abs(V - oh[i][None, :])).sum(0).max() for i in range(n)])
            omax = np.abs(oh).max(1)
            tol[:, h] = (2.0 ** -11 * (p @ np.abs(V)) + 2.0 ** -25 * (mask @ np.abs(V)) / lsum + sens[:, None]
                         + (ATTN_F64_RTOL * np.sqrt(np.maximum(1.0, (qpos + 1) / 256.0)) * omax)[:, None])
            o[:, h] = oh
            self.report["pf_attn_score_sensitivity"] = max(self.report["pf_attn_score_sensitivity"],
                                                           float((sens / np.maximum(omax, 1e-30)).max()))
        return o, tol

    def _attn_rows(self, D, l, Tq, rows, ncols):
        """The checked rows of pf_x_o (act_rows picks the format; the attention's f16 rows carry no scale)."""
        c = self.cfg
        xs = max(c.n_embd, c.n_ff, c.n_head * c.head_dim) // 32
        try:
            R = act_rows(D, l, "o", Tq, xs, ncols, self.kq)
        except AssertionError as e:
            raise AssertionError(f"pf_attn: layer {l}: {e}") from None
        return {k: (v[rows] if isinstance(v, np.ndarray) else v) for k, v in R.items()}

    def _gelu_rows(self, D, l, Tq, F, hid):
        """pf_x_down against the oracle's gelu_mul of the same gate / up floats.  NOT bit-identical on the device:
        the prefill's GELU kernels call gelu_mul1<EXACT = false> (common.h), the device libm's tanhf rather than
        glibc's (glibc_math.h is what is bit-checked, and only the exact engine uses it), so hid differs from the
        oracle's in the last place now and then.  The Q8_0 blocks and f16 rows absorb that almost always (integer
        quants, f16 d); Q8_K's f32 d = max / 127 shows it (mini-4b Q4_K, 70 tokens: the quants identical, one
        super-block's d not).  So, as the rows of the norms: the quantisation-aware bound, every
        element, with tol = 2^-22 max|hid| (tanhf to 2 ulp at |tanh| <= 1 through (0.5 x)(1 + t) u), and the
        quants within 1 of the oracle's; the rows that differ in any bit are counted
        (pf_gelu_rows_not_bit_identical)."""
        hid64 = hid.astype(np.float64)
        R = self.quant_rows("pf_gelu", D, l, "down", Tq, F, hid64, 2.0 ** -22 * np.abs(hid64).max(1, keepdims=True))
        differ = 0
        for t in range(Tq):
            if R["kind"] == "q8_k":
                ref = np.frombuffer(self.orc.quantize_q8_k(hid[t]), np.uint8).reshape(-1, 292)
                w = R["words"][t]
                # d = 1 / (-127 / max): max to tol, two f32 roundings
                dd, dr = w[::8, 8].copy().view(np.float32).astype(np.float64), ref[:, :4].copy().view(np.float32)[:, 0].astype(np.float64)
                self.bound("pf_gelu_q8k_d", np.abs(dd - dr), 2.0 ** -22 * np.abs(hid64[t]).max() / 127.0 + 2.0 ** -22 * np.abs(dr),
                           f"layer {l} token {t} super-block")
                differ += not (np.array_equal(w[:, :8].copy().view(np.int8).reshape(-1, 256), ref[:, 4:260].view(np.int8))
                               and np.array_equal(w[::8, 8].copy().view(np.float32), ref[:, :4].copy().view(np.float32)[:, 0]))
                continue
            ref = self.orc.quantize_q8_0(hid[t])
            if R["kind"] == "q8_0":
                differ += not np.array_equal(xblocks_to_q8_0(R["words"][t]), ref)
                continue
            b = ref.reshape(-1, 34)
            d = b[:, :2].copy().view(np.float16).astype(np.float32)  # f16(d) q 2^-s is exact in f32 (q8_f16_quad)
            want = ((d * np.float32(1.0 / R["ts"][t])) * b[:, 2:].view(np.int8).astype(np.float32)).astype(np.float16)
            differ += not np.array_equal(R["bits"][t], want.reshape(-1).view(np.uint16))
        self.report["pf_gelu_rows_not_bit_identical"] += differ

    def _prefill_q8_one(self, D, l, proj, names, ncols, n_t, H):
        c = self.cfg
        F = c.n_ff
        kq_types = (TT.Q4_K, TT.Q6_K)
        xs = np.frombuffer(D[(f"pf_x_{proj}", l)][-1], np.uint32).reshape(n_t, -1, 12)
        out = f32(D[(f"pf_{proj}", l)][-1]).reshape(n_t, -1)
        ws = [self.w.raw(n) for n in (names or [f"blk.{l}.ffn_gate.weight", f"blk.{l}.ffn_up.weight"])]
        kq = ws[0][1] in kq_types  # Q8_K activation blocks (K-quant layers), else Q8_0
        for t in range(n_t):
            if kq:
                try:
                    xf = xblocks_q8k_to_f32(xs[t, : ncols // 32])
                except AssertionError as e:
                    raise AssertionError(f"layer {l} {proj} token {t}: {e}") from None
                dot = lambda w: self.gemv(w, xf)  # noqa: E731
            else:
                xq = xblocks_to_q8_0(xs[t, : ncols // 32])
                dot = lambda w: self.gemv_q8(w, xq)  # noqa: E731
            if proj == "gate_up":
                g, u = dot(ws[0]), dot(ws[1])
                ref = np.concatenate([np.concatenate([g[k * H:(k + 1) * H], u[k * H:(k + 1) * H]])
                                      for k in range(F // H)])
            else:
                ref = np.concatenate([dot(w) for w in ws])
            self.note(f"prefill_gemm_{proj}", rel_err(out[t, : ref.size], ref), GEMV_RTOL)

    def _prefill_f16_one(self, D, l, proj, names, ncols, n_t, H):
        c = self.cfg
        F = c.n_ff
        x = np.frombuffer(D[(f"pf_x_{proj}", l)][-1], np.float16).reshape(n_t, -1)[:, :ncols].astype(np.float64)
        if (f"pf_xs_{proj}", l) in D:  # the rows' per-token scales 2^s (the attention's rows: none)
            ts = f32(D[(f"pf_xs_{proj}", l)][-1]).astype(np.float64)
            assert ts.size == n_t and np.all(ts > 0) and np.all(np.frexp(ts)[0] == 0.5), "token scales: powers of two"
            x = x * ts[:, None]
        out = f32(D[(f"pf_{proj}", l)][-1]).reshape(n_t, -1)
        if proj == "gate_up":
            g = self.dequant(self.w.raw(f"blk.{l}.ffn_gate.weight"))
            u = self.dequant(self.w.raw(f"blk.{l}.ffn_up.weight"))
            W = np.concatenate([np.concatenate([g[k * H:(k + 1) * H], u[k * H:(k + 1) * H]]) for k in range(F // H)])
        else:
            W = np.concatenate([self.dequant(self.w.raw(n)) for n in names])
        ref = x @ W.T
        for t in range(n_t):
            self.note(f"prefill_gemm16_{proj}", rel_err(out[t, : ref.shape[1]], ref[t]), PREFILL16_RTOL)

    def dequant(self, w):
        """Weight rows -> float64: Q4_0 in numpy, other types through the oracle's dequantize_row."""
        data, tt, rows, cols = w
        if tt == TT.Q4_0:
            return dequant_q4_0(w)
        rb = data.size // rows
        return np.stack([np.asarray(self.orc.dequantize_row(tt, data[i * rb:(i + 1) * rb], cols), np.float64)
                         for i in range(rows)])


PREFILL16_RTOL = 2e-3


def dequant_q4_0(w):
    """Q4_0 rows -> float64 (d * (q - 8); ops.h block layout: f16 d, 16 bytes, element i = low nibble of byte
    i, element i + 16 = high nibble)."""
    data, tt, rows, cols = w
    assert tt == TT.Q4_0, "f16 prefill GEMM check: Q4_0 weights only"
    b = data.reshape(rows, cols // 32, 18)
    d = b[:, :, :2].copy().view(np.float16).astype(np.float64)[:, :, 0]
    qs = b[:, :, 2:]
    q = np.concatenate([qs & 15, qs >> 4], axis=2).astype(np.float64) - 8.0
    return (q * d[:, :, None]).reshape(rows, cols)

