#!/usr/bin/env python3
"""Several sequences per step against the single-sequence decode loop (measurements).

    python scripts/bench_batch.py [--config gemma-3-4b] [--prefill 512] [--steps 64] [--repeats 5]

One session, one process.  A `prefill`-token prompt goes through forward() and is copied to every KV slot, so each
row decodes at the same context.  After a warm-up of every loop:
  (a) tokens/s of `steps` greedy steps of Model.generate (the single-sequence decode graph), `repeats` times;
  (b) for each B: the time per step and the aggregate tokens/s of Model.batch_generate over B rows, `repeats` times,
      interleaved with (a) so that clock and thermal drift hit both alike;
  (c) Model.time_kernel(10) (the multi-sequence attention, per layer) and time_kernel(9) (the fused scorer over the
      step's B rows) after each B's runs; what is left of the step is the GEMMs at T = B, the norms, the GELU and the
      q/k launch.
Medians, with the min..max spread.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def med(xs):
    return float(np.median(xs))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--config", default="gemma-3-4b")
    p.add_argument("--prefill", type=int, default=512)
    p.add_argument("--steps", type=int, default=64)
    p.add_argument("--warmup", type=int, default=8)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--kernel-reps", type=int, default=20)
    p.add_argument("--batches", default="1,2,4,8,16,32,64")
    a = p.parse_args()
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg = CONFIGS[a.config]
    batches = [int(b) for b in a.batches.split(",")]
    g = build_gemma3_gguf(cfg, seed=1234)
    m = Model(g, max_ctx=a.prefill + a.steps + 8)
    rng = np.random.default_rng(1)
    prompt = np.concatenate([[2], rng.integers(4, cfg.vocab, a.prefill - 1)]).astype(np.int32)
    m.forward(prompt, 0, want_logits=False)
    first, pos = m.last_argmax, a.prefill
    m.reserve_sequences(max(batches))
    for s in range(1, max(batches)):
        m.copy_sequence(s, 0, a.prefill)
    n_layer = m.info.n_layer

    def single(steps):
        m.sync()
        t0 = time.perf_counter()
        m.generate(first, pos, steps)
        return time.perf_counter() - t0

    def batch(B, steps):
        m.sync()
        t0 = time.perf_counter()
        m.batch_generate([first] * B, list(range(B)), [pos] * B, steps)
        return time.perf_counter() - t0

    single(a.warmup)
    for B in batches:
        batch(B, a.warmup)
    t_single, rows = [], []
    for B in batches:
        tb = []
        for _ in range(a.repeats):
            t_single.append(single(a.steps))
            tb.append(batch(B, a.steps))
        us_attn, by_attn = m.time_kernel(10, a.kernel_reps)
        us_score, _ = m.time_kernel(9, a.kernel_reps)
        step_us = med(tb) / a.steps * 1e6
        rows.append({"B": B, "step_us": round(step_us, 1),
                     "step_us_min_max": [round(min(tb) / a.steps * 1e6, 1), round(max(tb) / a.steps * 1e6, 1)],
                     "tok_s": round(B * a.steps / med(tb), 1),
                     "attn_us_per_layer": round(us_attn, 2), "attn_gbps": round(by_attn / max(us_attn, 1e-9) / 1e3, 1),
                     "attn_us_per_step": round(us_attn * n_layer, 1), "scorer_us": round(us_score, 1),
                     "rest_us": round(step_us - us_attn * n_layer - us_score, 1)})
    single_tok_s = a.steps / med(t_single)
    for r in rows:
        r["vs_sequential"] = round(r["tok_s"] / single_tok_s, 3)
    wins = [r["B"] for r in rows if r["vs_sequential"] > 1.0]
    print(json.dumps({
        "config": cfg.name, "prefill": a.prefill, "steps": a.steps, "repeats": a.repeats,
        "single_generate_tok_s": round(single_tok_s, 1),
        "single_generate_tok_s_min_max": [round(a.steps / max(t_single), 1), round(a.steps / min(t_single), 1)],
        "single_step_us": round(1e6 / single_tok_s, 1),
        "batch": rows, "smallest_B_beating_sequential": min(wins) if wins else None}))
    m.close()


if __name__ == "__main__":
    main()
