#!/usr/bin/env python3
"""Sampling inside the batch loop against the greedy batch loop and against host-side sampling (DESIGN.md section 13,
measurements).

    python scripts/bench_batch_sampling.py [--config gemma-3-4b] [--prefill 512] [--steps 32] [--repeats 5]
    python scripts/bench_batch_sampling.py --baseline     # only calls that exist without the sampled loop

scripts/bench_batch.py's workload: one session, a `prefill`-token prompt copied to every KV slot, so each row decodes
at the same context.  After a warm-up of every loop, for each B:
  (a) the time per step of Model.batch_generate(..., samplers=...) (temperature 1, top_k 64, top_p 0.95, a seed per
      row), `repeats` times;
  (b) the greedy Model.batch_generate step from the same process, interleaved with (a);
  (c) Model.time_kernel(11): the multi-row logits GEMV + select + finalize over the step's rows, its bytes, and
      time_kernel(1) (the single-row logits GEMV) beside it.
--baseline measures, per B, what host-side sampling costs per step: Model.batch_forward(want_logits=True), a numpy
top-k / softmax draw per row, the drawn ids fed back -- and the greedy step, interleaved.  It uses no call of the
sampled loop, so it also runs on a checkout that does not have it.
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


def host_sample(logits, rng, top_k=64):
    """One draw per row from the top_k logits' softmax (temperature 1)."""
    idx = np.argpartition(logits, -top_k, axis=1)[:, -top_k:]
    l = np.take_along_axis(logits, idx, axis=1).astype(np.float64)
    p = np.exp(l - l.max(axis=1, keepdims=True))
    c = np.cumsum(p, axis=1)
    j = (c < rng.random((logits.shape[0], 1)) * c[:, -1:]).sum(axis=1)
    return np.take_along_axis(idx, np.minimum(j, top_k - 1)[:, None], axis=1)[:, 0].astype(np.int32)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--config", default="gemma-3-4b")
    p.add_argument("--prefill", type=int, default=512)
    p.add_argument("--steps", type=int, default=32)
    p.add_argument("--warmup", type=int, default=4)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--kernel-reps", type=int, default=20)
    p.add_argument("--batches", default="1,8,32,64")
    p.add_argument("--baseline", action="store_true")
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
    table_bytes = cfg.vocab * cfg.n_embd * 2

    def greedy(B, steps):
        m.sync()
        t0 = time.perf_counter()
        m.batch_generate([first] * B, list(range(B)), [pos] * B, steps)
        return time.perf_counter() - t0

    def sampled(B, steps):
        sps = [dict(temperature=1.0, top_k=64, top_p=0.95, seed=1000 + b) for b in range(B)]
        m.sync()
        t0 = time.perf_counter()
        m.batch_generate([first] * B, list(range(B)), [pos] * B, steps, samplers=sps)
        return time.perf_counter() - t0

    def host(B, steps):
        hr = np.random.default_rng(7)
        tok = np.full(B, first, np.int32)
        m.sync()
        t0 = time.perf_counter()
        for i in range(steps):
            r = m.batch_forward(tok, list(range(B)), [pos + i] * B, want_logits=True)
            tok = host_sample(r.logits, hr)
        return time.perf_counter() - t0

    loop = host if a.baseline else sampled
    for B in batches:
        greedy(B, a.warmup)
        loop(B, a.warmup)
    rows = []
    for B in batches:
        tg, ts = [], []
        for _ in range(a.repeats):
            tg.append(greedy(B, a.steps))
            ts.append(loop(B, a.steps))
        us = lambda t: round(t / a.steps * 1e6, 1)  # noqa: E731
        row = {"B": B, "greedy_step_us": us(med(tg)), "greedy_step_us_min_max": [us(min(tg)), us(max(tg))]}
        key = "host_sampled_step_us" if a.baseline else "sampled_step_us"
        row[key] = us(med(ts))
        row[key + "_min_max"] = [us(min(ts)), us(max(ts))]
        row["over_greedy_us"] = round(row[key] - row["greedy_step_us"], 1)
        row["tok_s"] = round(B * a.steps / med(ts), 1)
        if not a.baseline:
            us11, by11 = m.time_kernel(11, a.kernel_reps)
            reads = round((by11 - B * cfg.vocab * 4) / table_bytes)
            row.update({"select_us": round(us11, 1), "table_reads": reads,
                        "select_gbps": round(by11 / max(us11, 1e-9) / 1e3, 1),
                        "select_us_per_table_read": round(us11 / max(reads, 1), 1),
                        "select_share_of_step": round(us11 / row[key], 3)})
        rows.append(row)
    us1, by1 = m.time_kernel(1, a.kernel_reps)
    print(json.dumps({
        "config": cfg.name, "prefill": a.prefill, "steps": a.steps, "repeats": a.repeats,
        "mode": "baseline: batch_forward(want_logits) + host draw" if a.baseline else "sampled batch loop",
        "single_row_logits_gemv_us": round(us1, 1), "single_row_logits_gemv_gbps": round(by1 / max(us1, 1e-9) / 1e3, 1),
        "batch": rows}))
    m.close()


if __name__ == "__main__":
    main()
