#!/usr/bin/env python3
"""Sampled decode against the greedy loop on the same GEMV (measurements).

    python scripts/bench_sampling.py [--config gemma-3-4b] [--prefill 512] [--steps 256] [--repeats 3]

One session with LLMI_FULL_LOGITS=1, so the greedy loop runs the full F16 logits GEMV + argmax + token feedback
-- the launches the sampled step replaces with its two.  After the prompt and a warm-up of both graphs:
  (a) Model.time_kernel(8) (the sampler's two launches) against time_kernel(1) (the logits GEMV);
  (b) tokens/s of `steps` greedy steps and of `steps` sampled steps (temperature 1, top_k 64, top_p 0.95), each
      `repeats` times from the same token and position.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--config", default="gemma-3-4b")
    p.add_argument("--prefill", type=int, default=512)
    p.add_argument("--steps", type=int, default=256)
    p.add_argument("--warmup", type=int, default=16)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--kernel-reps", type=int, default=50)
    p.add_argument("--exact", action="store_true")
    a = p.parse_args()
    os.environ["LLMI_FULL_LOGITS"] = "1"
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg = CONFIGS[a.config]
    g = build_gemma3_gguf(cfg, seed=1234)
    m = Model(g, exact=a.exact, max_ctx=a.prefill + a.steps + a.warmup + 8)
    assert m.info.screened_logits == 0
    rng = np.random.default_rng(1)
    prompt = np.concatenate([[2], rng.integers(4, cfg.vocab, a.prefill - 1)]).astype(np.int32)
    m.forward(prompt, 0, want_logits=False)
    first, pos = m.last_argmax, a.prefill
    sampler = dict(temperature=1.0, top_k=64, top_p=0.95, seed=1)

    def run(sp, steps):
        m.set_sampler(sp)
        m.sync()
        t0 = time.perf_counter()
        m.enqueue(first, pos, steps)
        ids = m.sync(steps)
        return steps / (time.perf_counter() - t0), ids

    run(None, a.warmup)
    run(sampler, a.warmup)
    greedy, sampled = [], []
    for _ in range(a.repeats):  # interleaved: clock and thermal drift hit both alike
        greedy.append(run(None, a.steps)[0])
        kpt_g = m.get_info().kernels_per_token
        sampled.append(run(sampler, a.steps)[0])
        kpt_s = m.get_info().kernels_per_token
    us_gemv, by_gemv = m.time_kernel(1, a.kernel_reps)
    us_samp, by_samp = m.time_kernel(8, a.kernel_reps)
    ms_g, ms_s = 1e3 / np.mean(greedy), 1e3 / np.mean(sampled)
    print(json.dumps({
        "config": cfg.name, "exact": a.exact, "vocab": cfg.vocab, "prefill": a.prefill, "steps": a.steps,
        "logits_gemv_us": round(us_gemv, 2), "logits_gemv_gbps": round(by_gemv / us_gemv / 1e3, 1),
        "sampler_us": round(us_samp, 2), "sampler_over_gemv": round(us_samp / us_gemv, 4),
        "greedy_full_logits_tok_s": [round(x, 2) for x in greedy],
        "sampled_tok_s": [round(x, 2) for x in sampled],
        "greedy_ms_per_token": round(ms_g, 4), "sampled_ms_per_token": round(ms_s, 4),
        "sampled_minus_greedy_us": round((ms_s - ms_g) * 1e3, 2),
        "greedy_spread_us": round((1e3 / min(greedy) - 1e3 / max(greedy)) * 1e3, 2),
        "kernels_per_token": {"greedy_full_logits": kpt_g, "sampled": kpt_s}}))
    m.close()


if __name__ == "__main__":
    main()
