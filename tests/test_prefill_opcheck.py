"""The prefill op checker checked (OpChecker.prefill_ops, tests/oplevel.py), on the CPU: a synthetic set of taps
for a tiny made-up shape, every op restated here in float64 / through the oracle and quantised by the oracle, fed
to prefill_ops through a stand-in for the GGUF weights.  The clean taps must pass every check in all three row
formats; each named corruption of one tap must fail the named check -- which is what shows that the GPU tests
(tests/test_fused_ops.py test_ops_prefill_nongemm*) would notice a subtly wrong kernel.

Shapes: E = 64, hd = 64, 2 heads, 1 kv head, F = 128 (H = 32), T = 40, 2 layers (SWA then global rope base).
Three cases need another shape, each the smallest that can state them: Q8_K rows need 256-element super-blocks
(E = F = hd = 256); "a head reads the neighbouring kv head" needs two kv heads (4 heads, 2 kv heads); a gate/up
de-interleave group of 40 needs F a multiple of 40 and 32 (F = 160)."""
import math

import numpy as np
import pytest

from llm_inference_amd.gguf import TensorType as TT
from llm_inference_amd.synthetic import Gemma3Config
from oplevel import OpChecker, quant_errors, attn_check_tokens

MAX_CTX = 64
SWA = [True, False]


class StubWeights:
    """Stands in for oplevel.Weights: name -> (bytes, type, rows, cols)."""

    def __init__(self, t):
        self.t = t

    def raw(self, name):
        return self.t[name]

    def f32(self, name):
        return self.t[name][0].view(np.float32)


def make_cfg(E=64, F=128, nh=2, nkv=1, hd=64):
    return Gemma3Config("stub", 2, E, F, nh, nkv, hd, 32)


def make_weights(cfg, kq, seed=1):
    rng = np.random.default_rng(seed)
    E, hd = cfg.n_embd, cfg.head_dim

    def nw(n):
        return (rng.uniform(0.6, 1.4, n).astype(np.float32).view(np.uint8), TT.F32, 1, n)

    t = {"token_embd.weight": (rng.normal(0, 0.05, (cfg.vocab, E)).astype(np.float16).view(np.uint8).reshape(-1),
                               TT.F16, cfg.vocab, E),
         "output_norm.weight": nw(E),
         "blk.0.attn_q.weight": (np.zeros(0, np.uint8), TT.Q4_K if kq else TT.Q4_0, 0, E)}
    for l in range(cfg.n_layer):
        for n, k in (("attn_norm", E), ("attn_q_norm", hd), ("attn_k_norm", hd), ("post_attention_norm", E),
                     ("ffn_norm", E), ("post_ffw_norm", E)):
            t[f"blk.{l}.{n}.weight"] = nw(k)
    return StubWeights(t)


def xblock_rows(orc, x, fmt, xs):
    """Rows x [n][cols] -> the device's XBlock rows (Q8_0 or Q8_K quants from the oracle), xs blocks a row."""
    n, cols = x.shape
    w = np.zeros((n, xs, 12), np.uint32)
    for t in range(n):
        if fmt == "q8_k":
            b = np.frombuffer(orc.quantize_q8_k(x[t]), np.uint8).reshape(-1, 292)
            q = b[:, 4:260].copy().view(np.int8).reshape(-1, 32)
            d = np.repeat(b[:, :4].copy().view(np.float32)[:, 0], 8)
            ns = q.astype(np.int32).sum(1)
        else:
            b = np.frombuffer(orc.quantize_q8_0(x[t]), np.uint8).reshape(-1, 34)
            q = b[:, 2:].copy().view(np.int8)
            d = b[:, :2].copy().view(np.float16)[:, 0].astype(np.float32)
            ns = -8 * q.astype(np.int32).sum(1)
        w[t, : cols // 32, :8] = q.copy().view(np.uint32).reshape(-1, 8)
        w[t, : cols // 32, 8] = d.view(np.uint32)
        w[t, : cols // 32, 9] = ns.astype(np.int32).view(np.uint32)
    return w


def f16_rows(orc, x, xs, scaled):
    """Rows -> f16(f16(d) q 2^-s) of their Q8_0 blocks and the token scales 2^s (token_xs restated: the row's
    largest value lands in [2^14, 2^15); unscaled: s = 0)."""
    n, cols = x.shape
    out = np.zeros((n, xs * 32), np.float16)
    ts = np.ones(n, np.float32)
    for t in range(n):
        b = np.frombuffer(orc.quantize_q8_0(x[t]), np.uint8).reshape(-1, 34)
        d = b[:, :2].copy().view(np.float16).astype(np.float64)
        amax = float(np.abs(x[t]).max())
        if scaled and amax > 0:
            ts[t] = 2.0 ** (math.floor(math.log2(amax)) - 14)
        out[t, :cols] = (d / float(ts[t]) * b[:, 2:].copy().view(np.int8).astype(np.float64)).reshape(-1).astype(np.float16)
    return out, ts


def attention_rows(q16, kc, vc, pos0, g, tok_rows, hook=None):
    """Float64 causal attention, one query and head at a time (a loop: nothing shared with the checker's
    vectorised restatement).  hook(t, h) -> dict of deviations: 'keys' (the key indices used), 'kvh'."""
    T, nh, hd = q16.shape
    out = np.zeros((len(tok_rows), nh * hd))
    for r, t in enumerate(tok_rows):
        for h in range(nh):
            dev = hook(t, h) if hook else {}
            keys = dev.get("keys", np.arange(pos0 + t + 1))
            kvh = dev.get("kvh", h // g)
            K = kc[kvh, keys].view(np.float16).astype(np.float64)
            V = vc[kvh, keys].view(np.float16).astype(np.float64)
            s = K @ q16[t, h].astype(np.float64)
            p = np.exp(s - s.max())
            out[r, h * hd:(h + 1) * hd] = (p / p.sum()) @ V
    return out


def make_taps(orc, cfg, W, fmt, T=40, pos0=0, H=32, seed=7, attn_hook=None, qk_hook=None, gelu_h=None):
    """The taps Session::prefill_run produces, from this file's restatement of every non-GEMM op; the GEMM
    outputs (pf_qkv, pf_o, pf_gate_up, pf_down) are random: prefill_ops does not check them."""
    rng = np.random.default_rng(seed)
    E, F, hd, nh, nkv, L = cfg.n_embd, cfg.n_ff, cfg.head_dim, cfg.n_head, cfg.n_head_kv, cfg.n_layer
    g, xs = nh // nkv, max(E, F, nh * hd) // 32
    eps = float(np.float32(cfg.eps))
    norm = lambda x, n: np.stack([orc.rms_norm(r, eps) * W.f32(n) for r in np.ascontiguousarray(x, np.float32)])  # noqa: E731
    tokens = rng.integers(4, cfg.vocab, T)
    emb = W.raw("token_embd.weight")[0].view(np.float16).reshape(cfg.vocab, E)
    resid = emb[tokens].astype(np.float32) * np.float32(math.sqrt(E))
    taps = []

    def rows(name, sname, l, x, f, scaled=True):
        if f == "f16":
            x16, ts = f16_rows(orc, x, xs, scaled)
            taps.append((name, l, x16.tobytes()))
            if sname:
                taps.append((sname, l, ts.tobytes()))
        else:
            taps.append((name, l, xblock_rows(orc, x, f, xs).tobytes()))

    for l in range(L):
        last = l == L - 1
        t0 = T - 1 if last else 0
        rows("pf_x_qkv", "pf_xs_qkv", l, norm(resid, f"blk.{l}.attn_norm.weight"), fmt)
        qkv = rng.normal(0, 1.5, (T, (nh + 2 * nkv) * hd)).astype(np.float32)
        taps.append(("pf_qkv", l, qkv.tobytes()))
        base = 10000.0 if SWA[l] else cfg.rope_base
        dev = qk_hook(l) if qk_hook else {}
        qn = norm(qkv[:, : nh * hd].reshape(-1, hd), f"blk.{l}.attn_q_norm.weight").reshape(T, nh, hd)
        kn = norm(qkv[:, nh * hd:(nh + nkv) * hd].reshape(-1, hd), f"blk.{l}.attn_k_norm.weight").reshape(T, nkv, hd)
        q16 = (orc.rope(qn, hd, dev.get("base", base), 1.0, pos0) * np.float32(dev.get("qscale", 1.0 / math.sqrt(hd)))).astype(np.float16)
        k16 = orc.rope(kn, hd, dev.get("base", base), 1.0, pos0).astype(np.float16)
        v16 = qkv[:, (nh + nkv) * hd:].reshape(T, nkv, hd).astype(np.float16)
        kc = np.zeros((nkv, MAX_CTX, hd), np.uint16)
        vc = np.zeros((nkv, MAX_CTX, hd), np.uint16)
        kc[:, :pos0] = rng.normal(0, 1, (nkv, pos0, hd)).astype(np.float16).view(np.uint16)  # an earlier prompt's rows
        vc[:, :pos0] = rng.normal(0, 1, (nkv, pos0, hd)).astype(np.float16).view(np.uint16)
        kshift = dev.get("kshift", 0)
        kc[:, pos0 + kshift:pos0 + kshift + T] = k16.view(np.uint16).transpose(1, 0, 2)
        vc[:, pos0:pos0 + T] = v16.view(np.uint16).transpose(1, 0, 2)
        f = "q8_0" if last and fmt == "f16" else fmt  # the last layer past its K/V append: the int8 path
        o = attention_rows(q16, kc, vc, pos0, g, range(t0, T), attn_hook if attn_hook and attn_hook(-1, -1).get("layer", l) == l else None)
        taps += [("pf_q", l, q16.tobytes()), ("kc", l, kc.tobytes()), ("vc", l, vc.tobytes())]
        rows("pf_x_o", None, l, o.astype(np.float32), f, scaled=False)
        po = rng.normal(0, 1, (T - t0, E)).astype(np.float32)
        taps.append(("pf_o", l, po.tobytes()))
        ra = resid[t0:] + norm(po, f"blk.{l}.post_attention_norm.weight")
        taps.append(("pf_resid_attn", l, ra.tobytes()))
        rows("pf_x_gate_up", "pf_xs_gate_up", l, norm(ra, f"blk.{l}.ffn_norm.weight"), f)
        gu = rng.normal(0, 1, (T - t0, 2 * F)).astype(np.float32)
        taps.append(("pf_gate_up", l, gu.tobytes()))
        gh = gelu_h or H
        gg = gu.reshape(T - t0, F // gh, 2, gh)
        hid = np.stack([orc.gelu_mul(r[:, 0].reshape(-1), r[:, 1].reshape(-1)) for r in gg])
        rows("pf_x_down", "pf_xs_down", l, hid, f)
        dn = rng.normal(0, 1, (T - t0, E)).astype(np.float32)
        taps.append(("pf_down", l, dn.tobytes()))
        if not last:
            resid = ra + norm(dn, f"blk.{l}.post_ffw_norm.weight")
            taps.append(("pf_resid_ffn", l, resid.tobytes()))
    final = ra[0] + norm(dn[:1], f"blk.{L - 1}.post_ffw_norm.weight")[0]
    xn = norm(final[None], "output_norm.weight")[0]
    data, tt, r, cc = W.raw("token_embd.weight")
    logits = orc.mat_vec_mul(tt, data, r, cc, xn, 4)
    taps += [("logits", -1, logits.tobytes()), ("token", -1, np.array([int(np.argmax(logits))], np.int32).tobytes())]
    return taps, tokens


def checker(orc, cfg, W, H=32):
    return OpChecker(orc, W, cfg, MAX_CTX, threads=4, swa_pattern=SWA, gelu_h=H)


SHAPES = {"q8_0": {}, "f16": {}, "q8_k": dict(E=256, F=256, hd=256)}
KINDS = ("pf_norm_in", "pf_qk_q", "pf_qk_k", "pf_qk_v", "pf_attn", "pf_resid_attn", "pf_norm_ffn", "pf_gelu",
         "pf_resid_ffn", "pf_tail")


@pytest.mark.parametrize("fmt", ["q8_0", "f16", "q8_k"])
@pytest.mark.parametrize("pos0", [0, 5])
def test_clean_taps_pass(oracle, fmt, pos0):
    cfg = make_cfg(**SHAPES[fmt])
    W = make_weights(cfg, fmt == "q8_k")
    taps, tokens = make_taps(oracle, cfg, W, fmt, pos0=pos0)
    chk = checker(oracle, cfg, W)
    chk.prefill_ops(taps, tokens, pos0)
    for k in KINDS:
        assert k in chk.report, k
    assert f"pf_norm_in_rows_{fmt}" in chk.report and f"pf_gelu_rows_{fmt}" in chk.report
    if fmt == "f16":  # the last layer's single token on the int8 path
        assert "pf_gelu_rows_q8_0" in chk.report and "pf_attn_rows_q8_0" in chk.report


def test_selection_rule():
    """Edges are never skipped: first / last block whole, and the block where the key rounds change."""
    sel = attn_check_tokens(200, 0, 2)  # rounds per block: 1, 1, 2, 2, 3, 3, 4
    assert set(range(0, 32)) <= set(sel) and set(range(192, 200)) <= set(sel)
    assert set(range(64, 96)) <= set(sel) and set(range(128, 160)) <= set(sel)
    assert [t for t in range(32, 64) if t in sel] == [32, 40, 48, 56]
    assert attn_check_tokens(70, 0, 2, t0=69) == [69]


def _replace(taps, name, layer, fn):
    out = []
    for n, l, b in taps:
        out.append((n, l, fn(b) if (n, l) == (name, layer) else b))
    return out


def _xq_edit(fn, xs):
    def f(b):
        w = np.frombuffer(b, np.uint32).reshape(-1, xs, 12).copy()
        fn(w)
        return w.tobytes()
    return f


def _set_q(w, t, blk, q):
    w[t, blk, :8] = np.asarray(q, np.int8).view(np.uint32)
    w[t, blk, 9] = np.array([-8 * int(np.asarray(q, np.int32).sum())], np.int32).view(np.uint32)[0]


@pytest.fixture(scope="module")
def base(oracle):
    cfg = make_cfg()
    W = make_weights(cfg, False)
    taps, tokens = make_taps(oracle, cfg, W, "q8_0")
    return cfg, W, taps, tokens


@pytest.mark.parametrize("what", ["quant_off_by_2", "d_off_4_ulps", "swap_neighbours", "block_shifted"])
def test_quant_bound_rejects(oracle, base, what):
    cfg, W, taps, tokens = base
    xs = 4

    def edit(w):
        q = w[3, 1, :8].copy().view(np.int8).copy()
        if what == "quant_off_by_2":
            i = int(np.argmin(np.abs(q)))
            q[i] += 2
            _set_q(w, 3, 1, q)
        elif what == "d_off_4_ulps":
            d = w[3, 1, 8:9].copy().view(np.float32).astype(np.float16)
            w[3, 1, 8] = (d.view(np.uint16) + np.uint16(4)).view(np.float16).astype(np.float32).view(np.uint32)[0]
        elif what == "swap_neighbours":
            i = int(np.argmax(np.abs(np.diff(q.astype(np.int32)))))
            q[i], q[i + 1] = q[i + 1], q[i]
            _set_q(w, 3, 1, q)
        else:  # the row's blocks moved up by one
            w[3, :2] = w[3, [1, 0]]

    bad = _replace(taps, "pf_x_qkv", 0, _xq_edit(edit, xs))
    with pytest.raises(AssertionError, match="pf_norm_in"):
        checker(oracle, cfg, W).prefill_ops(bad, tokens, 0)


def test_quant_bound_holds_for_the_reference(oracle):
    """The oracle's own Q8_0 blocks meet the bound with tol = 0 at every scale, f16-subnormal d included."""
    rng = np.random.default_rng(3)
    for scale in (3e-6, 1e-3, 1.0, 3000.0):
        x = (rng.normal(0, scale, (64, 64))).astype(np.float32)
        w = xblock_rows(oracle, x, "q8_0", 2)
        R = {"kind": "q8_0", "q": w[:, :, :8].copy().view(np.int8).reshape(64, -1, 32).astype(np.float64),
             "d": w[:, :, 8].copy().view(np.float32).astype(np.float64)}
        err, bnd, _, _ = quant_errors(R, x.astype(np.float64), 0.0)
        assert np.all(err <= bnd), scale
        x16, ts = f16_rows(oracle, x, 2, True)
        R = {"kind": "f16", "x16": x16.astype(np.float64), "ts": ts.astype(np.float64)}
        err, bnd, _, _ = quant_errors(R, x.astype(np.float64), 0.0)
        assert np.all(err <= bnd), scale


def test_scale_check_rejects_doubled_scale(oracle):
    cfg = make_cfg()
    W = make_weights(cfg, False)
    taps, tokens = make_taps(oracle, cfg, W, "f16")
    # 2^(s+1) with the row written for it (values halved: the largest falls below 2^14)
    bad = _replace(taps, "pf_xs_qkv", 0, lambda b: (np.frombuffer(b, np.float32) * np.float32(2)).tobytes())
    bad = _replace(bad, "pf_x_qkv", 0, lambda b: (np.frombuffer(b, np.float16) * np.float16(0.5)).tobytes())
    with pytest.raises(AssertionError, match="pf_norm_in.*token scales"):
        checker(oracle, cfg, W).prefill_ops(bad, tokens, 0)
    # 2^(s+1) in the scale tap alone: every value of the row is twice the reference's
    bad = _replace(taps, "pf_xs_gate_up", 0, lambda b: (np.frombuffer(b, np.float32) * np.float32(2)).tobytes())
    with pytest.raises(AssertionError, match="pf_norm_ffn"):
        checker(oracle, cfg, W).prefill_ops(bad, tokens, 0)


@pytest.mark.parametrize("dev,kind", [(dict(kshift=1), "pf_qk_k"), (dict(base=1000000.0), "pf_qk_"),
                                      (dict(qscale=1.0), "pf_qk_q")])
def test_qk_rejects(oracle, dev, kind):
    """A K row written one position late; the global rope base on the SWA layer (layer 0); q left unscaled."""
    cfg = make_cfg()
    W = make_weights(cfg, False)
    taps, tokens = make_taps(oracle, cfg, W, "q8_0", pos0=5, qk_hook=lambda l: dev if l == 0 else {})
    with pytest.raises(AssertionError, match=kind):
        checker(oracle, cfg, W).prefill_ops(taps, tokens, 5)


@pytest.mark.parametrize("fmt", ["q8_0", "f16"])
@pytest.mark.parametrize("what", ["diag_masked", "next_admitted", "last_tile_dropped", "neighbour_kv_head"])
def test_attn_rejects(oracle, fmt, what):
    pos0 = 0 if what == "last_tile_dropped" else 5
    cfg = make_cfg(nh=4, nkv=2) if what == "neighbour_kv_head" else make_cfg()
    W = make_weights(cfg, False)

    def hook(t, h):
        if t < 0:
            return {"layer": 0}
        n = pos0 + t + 1
        if what == "diag_masked":
            return {"keys": np.arange(max(n - 1, 1))} if t == 17 else {}
        if what == "next_admitted":
            return {"keys": np.arange(n + 1)} if t == 17 else {}
        if what == "last_tile_dropped":
            return {"keys": np.arange(32 * ((n - 1) // 32))} if n > 32 else {}
        return {"kvh": 0} if h == 3 and t == 17 else {}

    taps, tokens = make_taps(oracle, cfg, W, fmt, pos0=pos0, attn_hook=hook)
    with pytest.raises(AssertionError, match="pf_attn"):
        checker(oracle, cfg, W).prefill_ops(taps, tokens, pos0)


@pytest.mark.parametrize("fmt", ["q8_0", "f16"])
def test_gelu_rejects_wrong_group(oracle, fmt):
    """Gate / up de-interleaved at H = 32 where the layout's group is 40 (F = 160: a multiple of both)."""
    cfg = make_cfg(F=160)
    W = make_weights(cfg, False)
    taps, tokens = make_taps(oracle, cfg, W, fmt, H=40)
    checker(oracle, cfg, W, H=40).prefill_ops(taps, tokens, 0)
    taps, tokens = make_taps(oracle, cfg, W, fmt, H=40, gelu_h=32)
    with pytest.raises(AssertionError, match="pf_gelu"):
        checker(oracle, cfg, W, H=40).prefill_ops(taps, tokens, 0)
