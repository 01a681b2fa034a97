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

    python scripts/bench_batch.py --shared [--prompts 512,2048] [--batches 8,32,64]

The shared-prefix form: one prompt through forward(), Model.share_prefix into B - 1 further
slots, then `steps` greedy steps of batch_generate over the B rows -- `repeats` times with the grouping on and, in the
same process and interleaved, off (LLMI_BATCH_SHARED=0: the same rows through the unshared launches).  After each
(prompt, B): time_kernel(16) (the shared form) and time_kernel(10) (the unshared form) over the last step's rows.
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


def shared(a, cfg, g):
    from llm_inference_amd.model import Model
    batches = [int(b) for b in a.batches.split(",")]
    rows = []
    for P in [int(x) for x in a.prompts.split(",")]:
        m = Model(g, max_ctx=P + a.steps + 8)
        rng = np.random.default_rng(1)
        prompt = np.concatenate([[2], rng.integers(4, cfg.vocab, P - 1)]).astype(np.int32)
        m.forward(prompt, 0, want_logits=False)
        first = m.last_argmax
        m.reserve_sequences(max(batches))
        for s in range(1, max(batches)):
            m.share_prefix(s, 0, P)

        def run(B, steps, on):
            os.environ["LLMI_BATCH_SHARED"] = "1" if on else "0"
            m.sync()
            t0 = time.perf_counter()
            m.batch_generate([first] * B, list(range(B)), [P] * B, steps)
            return (time.perf_counter() - t0) / steps * 1e6

        for B in batches:
            run(B, a.warmup, True), run(B, a.warmup, False)
            on, off = [], []
            for _ in range(a.repeats):
                off.append(run(B, a.steps, False))
                on.append(run(B, a.steps, True))
            us16, by16 = m.time_kernel(16, a.kernel_reps)
            us10, by10 = m.time_kernel(10, a.kernel_reps)
            rows.append({"prompt": P, "B": B,
                         "step_us_shared": round(med(on), 1), "step_us_shared_min_max": [round(min(on), 1), round(max(on), 1)],
                         "step_us_unshared": round(med(off), 1),
                         "step_us_unshared_min_max": [round(min(off), 1), round(max(off), 1)],
                         "attn_us_per_layer_shared": round(us16, 2), "attn_us_per_layer_unshared": round(us10, 2),
                         "attn_kv_bytes_shared": by16, "attn_kv_bytes_unshared": by10,
                         "attn_speedup": round(us10 / max(us16, 1e-9), 2), "step_speedup": round(med(off) / med(on), 3)})
        m.close()
    os.environ.pop("LLMI_BATCH_SHARED", None)
    print(json.dumps({"config": cfg.name, "mode": "shared", "steps": a.steps, "repeats": a.repeats, "rows": rows}))


def qtable(a):
    """--table q8_0: Gemma-3 1B with Q8_0 layers and a Q8_0 output table, batch_qtable on.
    Per B, greedy and sampled: the step time with the multi-row logits launch and the rows reduce
    (LLMI_BATCH_QTABLE_ROWS=1: at every B) and with one launch_gemv + one row reduce per row (=0), interleaved."""
    from llm_inference_amd.gguf import TensorType as TT
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg = CONFIGS["gemma-3-1b"]
    batches = [int(b) for b in a.batches.split(",")]
    m = Model(build_gemma3_gguf(cfg, seed=1234, wtype=TT.Q8_0, embd_type=TT.Q8_0), max_ctx=a.prefill + a.steps + 8,
              batch_qtable=True)
    rng = np.random.default_rng(1)
    prompt = np.concatenate([[2], rng.integers(4, cfg.vocab, a.prefill - 1)]).astype(np.int32)
    m.forward(prompt, 0, want_logits=False)
    first, pos = m.last_argmax, a.prefill
    m.reserve_sequences(max(batches))
    for s in range(1, max(batches)):
        m.copy_sequence(s, 0, a.prefill)
    sp = dict(temperature=0.8, top_k=40, top_p=0.95, seed=7)

    def run(B, steps, multi, sampled):
        os.environ["LLMI_BATCH_QTABLE_ROWS"] = "1" if multi else "0"
        m.sync()
        t0 = time.perf_counter()
        m.batch_generate([first] * B, list(range(B)), [pos] * B, steps, samplers=sp if sampled else None)
        return (time.perf_counter() - t0) / steps * 1e6

    rows = []
    for B in batches:
        for sampled in (False, True):
            run(B, a.warmup, True, sampled), run(B, a.warmup, False, sampled)
            on, off = [], []
            for _ in range(a.repeats):
                off.append(run(B, a.steps, False, sampled))
                on.append(run(B, a.steps, True, sampled))
            r = {"B": B, "mode": "sampled" if sampled else "greedy",
                 "step_us_multi": round(med(on), 1), "step_us_multi_min_max": [round(min(on), 1), round(max(on), 1)],
                 "step_us_per_row": round(med(off), 1),
                 "step_us_per_row_min_max": [round(min(off), 1), round(max(off), 1)],
                 "step_speedup": round(med(off) / med(on), 3)}
            if sampled:  # time_kernel(11): the logits launches + select + finalize over the last step's rows
                for name, v in (("multi", "1"), ("per_row", "0")):
                    os.environ["LLMI_BATCH_QTABLE_ROWS"] = v
                    us, by = m.time_kernel(11, a.kernel_reps)
                    r["logits_select_us_" + name], r["logits_bytes_" + name] = round(us, 1), by
            rows.append(r)
    os.environ.pop("LLMI_BATCH_QTABLE_ROWS", None)
    print(json.dumps({"config": cfg.name, "mode": "table q8_0", "prefill": a.prefill, "steps": a.steps,
                      "repeats": a.repeats, "rows": rows}))
    m.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--config", default="gemma-3-4b")
    p.add_argument("--prefill", type=int, default=512)
    p.add_argument("--steps", type=int, default=64)
    p.add_argument("--warmup", type=int, default=8)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--kernel-reps", type=int, default=20)
    p.add_argument("--batches", default=None)
    p.add_argument("--shared", action="store_true")
    p.add_argument("--prompts", default="512,2048")
    p.add_argument("--table", default="f16", choices=["f16", "q8_0"])
    a = p.parse_args()
    if a.table == "q8_0":
        a.batches = a.batches or "1,8,32,64"
        return qtable(a)
    a.batches = a.batches or ("8,32,64" if a.shared else "1,2,4,8,16,32,64")
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg = CONFIGS[a.config]
    batches = [int(b) for b in a.batches.split(",")]
    g = build_gemma3_gguf(cfg, seed=1234)
    if a.shared:
        return shared(a, cfg, g)
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
