"""Score a random prompt on the device (Model.score) and time it.

    python scripts/score_prompt.py --config gemma-3-4b --n 512 [--reps 7] [--prefix-n 32]

Prints the prompt's nll and perplexity, then, warm (two untimed calls first), the median and the min .. max of
--reps synchronous calls of
  (a) score(prompt)            the fused path (or the row path if that is what the session runs),
  (b) forward(prompt)          the same prompt on the same session, last-token logits only,
  (c) time_kernel(9)           the fused scorer's two launches over the last chunk, with its FLOP and byte rates,
  (d) score(prompt) with LLMI_NO_PREFILL=1: the row path (token loop, full logits, f64 row reduce), same session,
and, with --prefix-n K, the only route without score(): one forward per prefix over the first K tokens.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_inference_amd.model import Model  # noqa: E402
from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf  # noqa: E402


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gemma-3-4b", choices=sorted(CONFIGS))
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--prefix-n", type=int, default=0, help="also time one forward per prefix over the first K tokens")
    a = ap.parse_args()
    os.environ.pop("LLMI_NO_PREFILL", None)
    cfg = CONFIGS[a.config]
    g = build_gemma3_gguf(cfg, seed=1234)
    m = Model(g, max_ctx=a.n + 8)
    prompt = np.concatenate([[2], np.random.default_rng(99).integers(4, cfg.vocab, a.n - 1)]).astype(np.int32)
    info = m.get_info()
    r = m.score(prompt)
    print(f"{a.config} n={a.n}: score_path {info.score_path}, nll {r.nll:.4f} over {r.count} targets, "
          f"perplexity {r.perplexity:.4f} (random weights; vocabulary {cfg.vocab})", flush=True)
    fmt = lambda t: f"{t[0]:.3f} ms (min {t[1]:.3f} .. max {t[2]:.3f})"  # noqa: E731
    ta = timed(lambda: m.score(prompt), a.reps)
    print(f"(a) score(prompt)   {fmt(ta)}", flush=True)
    tb = timed(lambda: m.forward(prompt, 0, want_logits=False), a.reps)
    print(f"(b) forward(prompt) {fmt(tb)}", flush=True)
    print(f"    (a) - (b) = {ta[0] - tb[0]:.3f} ms: the cost of scoring every position over a plain prompt", flush=True)
    m.score(prompt)  # the scorer's buffers hold the last chunk again
    us, by = m.time_kernel(9, max(a.reps, 3))
    if us > 0:
        chunk = int(os.environ.get("LLMI_PREFILL_CHUNK", "512"))
        t_last = a.n - (a.n - 1) // chunk * chunk
        flop = 2.0 * t_last * cfg.vocab * cfg.n_embd
        # roofline (MI355X: 2517 TFLOP/s dense f16 MFMA by the data sheet, about 6.3 TB/s of HBM achievable)
        t_flop, t_byte = flop / 2517e12 * 1e6, by / 6.3e12 * 1e6
        print(f"(c) time_kernel(9)  {us:.1f} us over the last chunk of {t_last} tokens: {flop / us / 1e6:.1f} TFLOP/s "
              f"(f16 MFMA), {by / us / 1e3:.1f} GB/s of table + rows ({by / 1e9:.3f} GB read once); least time "
              f"{max(t_flop, t_byte):.1f} us ({'FLOP' if t_flop > t_byte else 'byte'}-bound: {t_flop:.1f} us of MFMA, "
              f"{t_byte:.1f} us of HBM) = {max(t_flop, t_byte) / us:.3f} of the kernel time", flush=True)
    else:
        print("(c) time_kernel(9)  0 / 0: the row path is in use", flush=True)
    # the row path on the same session (LLMI_NO_PREFILL is read at the call), the two alternating
    os.environ["LLMI_NO_PREFILL"] = "1"
    assert m.get_info().score_path == 2
    r2 = m.score(prompt)  # (warm: the step graph is captured)
    fused_ms, row_ms = [], []
    for _ in range(max(3, a.reps // 2)):
        os.environ["LLMI_NO_PREFILL"] = "1"
        t0 = time.perf_counter()
        m.score(prompt)
        row_ms.append((time.perf_counter() - t0) * 1e3)
        os.environ.pop("LLMI_NO_PREFILL")
        t0 = time.perf_counter()
        m.score(prompt)
        fused_ms.append((time.perf_counter() - t0) * 1e3)
    td = (statistics.median(row_ms), min(row_ms), max(row_ms))
    tf = (statistics.median(fused_ms), min(fused_ms), max(fused_ms))
    print(f"(d) row path        {fmt(td)}, alternating with the fused path at {fmt(tf)}; row path nll {r2.nll:.4f}, "
          f"max |dlogprob| vs (a) {float(np.abs(r2.logprobs - r.logprobs).max()):.3g}, argmax equal at "
          f"{int((r2.argmax == r.argmax).sum())} of {a.n}", flush=True)
    print(f"    fused / row = {tf[0] / td[0]:.4f}; spreads {tf[2] - tf[1]:.3f} ms and {td[2] - td[1]:.3f} ms against a "
          f"difference of {td[0] - tf[0]:.3f} ms", flush=True)
    if a.prefix_n > 0:
        k = min(a.prefix_n, a.n)

        def per_prefix():
            for i in range(k):
                m.forward(prompt[:i + 1], 0)

        tp = timed(per_prefix, 3, warm=1)
        print(f"(e) one forward per prefix, first {k} tokens: {fmt(tp)} = {tp[0] / k:.3f} ms per position", flush=True)
    m.close()


if __name__ == "__main__":
    main()
