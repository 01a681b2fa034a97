#!/usr/bin/env python3
"""Lookup decoding against the greedy batch loop (measurements).

    python scripts/bench_batch_lookup.py [--config gemma-3-4b] [--repeats 5] [--out profiles/r11_bench_batch_lookup.json]

One process, one session (synthetic weights, Q4_0), 512-token prompts in B slots, B in {1, 8, 32}.  Per B the greedy
loop (Model.batch_generate, n_new steps) and the lookup loop (Model.batch_generate_lookup, max_new = n_new) at draft_len
3 and 7 run interleaved after a warm-up of each, `repeats` times; medians with the min..max spread, wall-clock
milliseconds around the synchronous calls, divided by the steps each call ran.  Reported per (B, draft_len): both step
times, the tokens per step the lookup call reached, Model.time_kernel(13) and the break-even acceptance -- the emitted
tokens per step at which the lookup loop equals the greedy loop, lookup step / greedy step.

The synthetic model's greedy ids are one constant id from the first step on, so after the first two steps (a wrong
draft from the prompt's repeated last token, then none) every draft is accepted: the tokens per step printed here sit
just below the upper bound draft_len + 1 and say nothing about acceptance on real text, which has not been measured.
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
    return {"median_ms": round(float(np.median(ts)) * 1e3, 4),
            "min_max_ms": [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--config", default="gemma-3-4b")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--n-new", type=int, default=64)
    p.add_argument("--kernel-reps", type=int, default=20)
    p.add_argument("--out", default=os.path.join("profiles", "r11_bench_batch_lookup.json"))
    a = p.parse_args()
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg = CONFIGS[a.config]
    n_new = a.n_new
    m = Model(build_gemma3_gguf(cfg, seed=1234), max_ctx=512 + n_new + 8)
    m.reserve_sequences(33)
    rng = np.random.default_rng(1)
    prompt = np.concatenate([[2], rng.integers(4, cfg.vocab, 511)]).astype(np.int32)
    prompt[-2] = prompt[-1]  # the history ends in a repeat: a draft from the first step on
    m.forward(prompt[:-1], 0, want_logits=False)
    for s in range(1, 33):
        m.copy_sequence(s, 0, 511)

    def timed(fn):
        m.sync()
        t0 = time.perf_counter()
        r = fn()
        return time.perf_counter() - t0, r

    res = {"config": cfg.name, "repeats": a.repeats, "n_new": n_new, "prompt_tokens": 512,
           "note": "the synthetic model's greedy ids are one constant id from the first step on (see ids_head), so after "
                   "the first two steps every draft is accepted: tokens_per_step_synthetic is an upper-bound figure (the "
                   "bound itself is draft_len + 1); acceptance on real text has not been measured", "cases": []}
    for B in (1, 8, 32):
        slots, pos = list(range(1, B + 1)), [511] * B
        first, hists = [int(prompt[-1])] * B, [prompt] * B

        def greedy():
            return m.batch_generate(first, slots, pos, n_new)

        for D in (3, 7):
            def lookup():
                return m.batch_generate_lookup(hists, slots, pos, n_new, draft_len=D)

            want = greedy()
            got = lookup()  # warm-up of both paths, and the ids
            assert all(x.tolist() == want[:, b].tolist() for b, x in enumerate(got.ids)), "ids differ from batch_generate"
            tg, tl = [], []
            for _ in range(a.repeats):
                tg.append(timed(greedy)[0] / n_new)
                t, r = timed(lookup)
                tl.append(t / r.steps)
            us = [m.time_kernel(13, a.kernel_reps) for _ in range(a.repeats)]
            g, l = float(np.median(tg)), float(np.median(tl))
            res["cases"].append({
                "B": B, "draft_len": D, "token_rows_per_step": B * (D + 1), "lookup_steps": r.steps,
                "greedy_step": stats(tg), "lookup_step": stats(tl),
                "tokens_per_step_upper_bound": D + 1, "tokens_per_step_synthetic": round(n_new / r.steps, 3),
                "drafted": int(r.drafted[0]), "accepted": int(r.accepted[0]),
                "last_prompt_token": int(prompt[-1]), "ids_head": got.ids[0][:12].tolist(),
                "lookup_kernel_us": round(float(np.median([u for u, _ in us])), 2), "lookup_kernel_bytes": us[0][1],
                "break_even_tokens_per_step": round(l / g, 3),
                "speedup_upper_bound": round((D + 1) * g / l, 3),
                "speedup_synthetic": round(g * n_new / (l * r.steps), 3)})
    res["prefill_f16_redo"] = m.get_info().prefill_f16_redo
    m.close()
    out = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out + "\n")
    print(out)


if __name__ == "__main__":
    main()
