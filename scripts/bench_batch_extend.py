#!/usr/bin/env python3
"""Ragged batch steps against the paths they replace (measurements).

    python scripts/bench_batch_extend.py [--config gemma-3-4b] [--repeats 5] [--out profiles/r10_bench_batch_extend.json]

One process, one session (synthetic weights), a warm-up of every path, then `repeats` timed runs of each, interleaved;
medians with the min..max spread, wall-clock milliseconds around synchronous calls:
  (a) 8 prompts of 512 tokens into 8 slots by Model.prefill_sequences, against forward + copy_sequence per prompt;
  (b) one step of 32 decode rows at position 512 plus one 128-token span (Model.batch_extend), against the same work
      as a batch_forward step followed by forward + copy_sequence of the 128 tokens;
  (c) a 5-token "all" span per slot at B = 8 (draft verification), against 5 batch_forward steps;
  (d) Model.time_kernel(12) for step (b)'s attention: the span form, and the per-token form under
      LLMI_BATCH_SPAN_ROWS=1.
Writes the JSON to --out and prints it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(ts):
    return {"median_ms": round(float(np.median(ts)) * 1e3, 3),
            "min_max_ms": [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--config", default="gemma-3-4b")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--kernel-reps", type=int, default=20)
    p.add_argument("--out", default=os.path.join("profiles", "r10_bench_batch_extend.json"))
    a = p.parse_args()
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg = CONFIGS[a.config]
    m = Model(build_gemma3_gguf(cfg, seed=1234), max_ctx=512 + 128 + 8)
    m.reserve_sequences(34)
    rng = np.random.default_rng(1)
    prompts = [np.concatenate([[2], rng.integers(4, cfg.vocab, 511)]).astype(np.int32) for _ in range(8)]
    chunk = rng.integers(4, cfg.vocab, 128).astype(np.int32)
    drafts = rng.integers(4, cfg.vocab, (8, 5)).astype(np.int32)
    dec = rng.integers(4, cfg.vocab, 32).astype(np.int32)

    def timed(fn):
        m.sync()
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    # (a) slots 1..8
    def a_extend():
        m.prefill_sequences(prompts, list(range(1, 9)))

    def a_parent():
        for i, x in enumerate(prompts):
            m.forward(x, 0, want_logits=False)
            m.copy_sequence(1 + i, 0, 512)

    # (b) decode rows on slots 1..32 (512 rows each: the first prompt copied), the span on slot 33
    def b_setup():
        m.forward(prompts[0], 0, want_logits=False)
        for s in range(1, 33):
            m.copy_sequence(s, 0, 512)

    def b_extend():
        m.batch_extend([[int(t)] for t in dec] + [chunk], list(range(1, 34)), [512] * 32 + [0], out=["last"] * 32 + ["none"])

    def b_parent():
        m.batch_forward(dec, list(range(1, 33)), [512] * 32)
        m.forward(chunk, 0, want_logits=False)
        m.copy_sequence(33, 0, 128)

    # (c) slots 1..8 at position 512
    def c_extend():
        m.batch_extend(list(drafts), list(range(1, 9)), [512] * 8, out="all")

    def c_parent():
        for i in range(5):
            m.batch_forward(drafts[:, i], list(range(1, 9)), [512 + i] * 8)

    res = {"config": cfg.name, "repeats": a.repeats}
    for name, setup, new, old in (("a_prefill_8x512", None, a_extend, a_parent),
                                  ("b_32_decode_rows_plus_128_token_span", b_setup, b_extend, b_parent),
                                  ("c_verify_5_drafts_x8", b_setup, c_extend, c_parent)):
        if setup:
            setup()
        new()
        old()  # warm-up of both paths
        tn, to = [], []
        for _ in range(a.repeats):
            tn.append(timed(new))
            to.append(timed(old))
        res[name] = {"extend": stats(tn), "parent_path": stats(to),
                     "parent_over_extend": round(float(np.median(to) / np.median(tn)), 3)}
    # (d) step (b)'s attention, both forms
    b_setup()
    b_extend()
    us, by = m.time_kernel(12, a.kernel_reps)
    runs = [m.time_kernel(12, a.kernel_reps)[0] for _ in range(a.repeats)]
    os.environ["LLMI_BATCH_SPAN_ROWS"] = "1"
    b_extend()
    del os.environ["LLMI_BATCH_SPAN_ROWS"]
    m.time_kernel(12, a.kernel_reps)
    runs1 = [m.time_kernel(12, a.kernel_reps)[0] for _ in range(a.repeats)]
    res["d_attention_of_step_b_us_per_layer"] = {
        "bytes_per_layer": by,
        "span_form": {"median_us": round(float(np.median(runs)), 2), "min_max_us": [round(min(runs), 2), round(max(runs), 2)]},
        "per_token_form": {"median_us": round(float(np.median(runs1)), 2),
                           "min_max_us": [round(min(runs1), 2), round(max(runs1), 2)]},
        "per_token_over_span": round(float(np.median(runs1) / np.median(runs)), 3)}
    res["prefill_f16_redo"] = m.get_info().prefill_f16_redo
    m.close()
    out = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out + "\n")
    print(out)


if __name__ == "__main__":
    main()
