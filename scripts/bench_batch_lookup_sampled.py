#!/usr/bin/env python3
"""Lookup decoding for sampled rows against the sampled batch loop (measurements).

    python scripts/bench_batch_lookup_sampled.py [--config gemma-3-4b] [--repeats 5]
                                                 [--out profiles/r12_bench_batch_lookup_sampled.json]

One process, one session (synthetic weights, Q4_0), 512-token prompts in B slots, B in {1, 8, 32}, temperature 1 /
top_k 64 / top_p 0.95 with a seed per row.  Per (B, draft_len in {3, 7}) these loops run interleaved after a warm-up
of each, `repeats` times; medians with the min..max spread, wall-clock milliseconds around the synchronous calls,
divided by the steps each call ran:

  sampled     Model.batch_generate(samplers=...), n_new steps: the baseline (one token per row and step);
  lookup      Model.batch_generate_lookup_sampled, max_new = n_new, the prompt as the history;
  no_gather   the same call under LLMI_LOOKUP_NO_GATHER=1 (the logits of every token row);
  no_draft    histories of distinct tokens and ngram_min = ngram_max = 8 over 8 steps, so that no step has a draft and
              every step's live token rows are the B current tokens -- against the baseline over the same 8 steps;
              with and without the list.

Reported per case: the step times, their ratio to the baseline (the break-even emitted tokens per step), the tokens
per step the call reached, Model.time_kernel(14) with the live rows and the table reads of the step it timed.

What the synthetic model accepts at temperature 1 is a property of that model (its logits are peaked and its ids
repeat), not a result: tokens_per_step_synthetic says nothing about acceptance on real text.
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
    p.add_argument("--out", default=os.path.join("profiles", "r12_bench_batch_lookup_sampled.json"))
    a = p.parse_args()
    from llm_inference_amd import ops
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg = CONFIGS[a.config]
    n_new, n_bare = a.n_new, 8
    m = Model(build_gemma3_gguf(cfg, seed=1234), max_ctx=512 + n_new + 8)
    m.reserve_sequences(33)
    rng = np.random.default_rng(1)
    prompt = np.concatenate([[2], rng.integers(4, cfg.vocab, 511)]).astype(np.int32)
    prompt[-2] = prompt[-1]  # the history ends in a repeat: a draft from the first step on
    m.forward(prompt[:-1], 0, want_logits=False)
    for s in range(1, 33):
        m.copy_sequence(s, 0, 511)
    bare = np.concatenate([np.arange(1000, 1040), prompt[-1:]]).astype(np.int32)  # distinct tokens: no match
    rb = ops.logits_rows_rb(cfg.n_embd)
    table = cfg.vocab * cfg.n_embd * 2

    def timed(fn):
        m.sync()
        t0 = time.perf_counter()
        r = fn()
        return time.perf_counter() - t0, r

    def kernel(T, gather):
        """time_kernel(14) and the step it timed: (us, bytes, live rows, table reads)."""
        us = [m.time_kernel(14, a.kernel_reps) for _ in range(a.repeats)]
        by = us[0][1]
        if gather:
            n = next(n for n in range(T + 1) if -(-n // rb) * table + n * cfg.vocab * 4 == by)
        else:
            n = T
        reads = round((by - n * cfg.vocab * 4) / table)
        return {"us": round(float(np.median([u for u, _ in us])), 2), "bytes": by, "rows": n, "table_reads": reads}

    def no_gather(fn):
        os.environ["LLMI_LOOKUP_NO_GATHER"] = "1"
        try:
            return fn()
        finally:
            del os.environ["LLMI_LOOKUP_NO_GATHER"]

    res = {"config": cfg.name, "repeats": a.repeats, "n_new": n_new, "prompt_tokens": 512, "rows_per_table_read": rb,
           "sampler": {"temperature": 1.0, "top_k": 64, "top_p": 0.95, "seed": "1000 + row"},
           "note": "acceptance on the synthetic model at temperature 1 is a property of that model (peaked logits, "
                   "repeating ids), not a result: tokens_per_step_synthetic says nothing about real text; the bound is "
                   "draft_len + 1", "cases": []}
    for B in (1, 8, 32):
        slots, pos = list(range(1, B + 1)), [511] * B
        first, hists, bares = [int(prompt[-1])] * B, [prompt] * B, [bare] * B
        sps = [dict(temperature=1.0, top_k=64, top_p=0.95, seed=1000 + b) for b in range(B)]

        def sampled(n=n_new):
            return m.batch_generate(first, slots, pos, n, samplers=sps)

        for D in (3, 7):
            T = B * (D + 1)

            def lookup():
                return m.batch_generate_lookup_sampled(hists, slots, pos, n_new, sps, draft_len=D)

            def nodraft():
                return m.batch_generate_lookup_sampled(bares, slots, pos, n_bare, sps, draft_len=D, ngram_max=8,
                                                       ngram_min=8)

            want = sampled()
            got = lookup()  # warm-up of every path, and the ids
            assert all(x.tolist() == want[:, b].tolist() for b, x in enumerate(got.ids)), "ids differ from batch_generate"
            got_ng = no_gather(lookup)
            assert [x.tolist() for x in got_ng.ids] == [x.tolist() for x in got.ids], "ids differ without the list"
            nd = nodraft()
            assert nd.drafted.sum() == 0 and nd.steps == n_bare
            assert all(x.tolist() == want[:n_bare, b].tolist() for b, x in enumerate(nd.ids))
            no_gather(nodraft), sampled(n_bare)
            ts, tl, tn, ts8, td, tdn = [], [], [], [], [], []
            for _ in range(a.repeats):
                ts.append(timed(sampled)[0] / n_new)
                t, r = timed(lookup)
                tl.append(t / r.steps)
                t, rn = timed(lambda: no_gather(lookup))
                tn.append(t / rn.steps)
                ts8.append(timed(lambda: sampled(n_bare))[0] / n_bare)
                td.append(timed(nodraft)[0] / n_bare)
                tdn.append(timed(lambda: no_gather(nodraft))[0] / n_bare)
            lookup()
            k_l = kernel(T, True)
            no_gather(lookup)
            k_n = kernel(T, False)
            nodraft()
            k_d = kernel(T, True)
            s, l, n_, s8, d, dn = (float(np.median(x)) for x in (ts, tl, tn, ts8, td, tdn))
            print(f"B {B} draft_len {D}: sampled {s * 1e3:.2f} ms, lookup {l * 1e3:.2f} ms", file=sys.stderr, flush=True)
            res["cases"].append({
                "B": B, "draft_len": D, "token_rows_per_step": T, "lookup_steps": r.steps,
                "sampled_step": stats(ts), "lookup_step": stats(tl), "lookup_step_no_gather": stats(tn),
                "break_even_tokens_per_step": round(l / s, 3), "break_even_no_gather": round(n_ / s, 3),
                "tokens_per_step_upper_bound": D + 1, "tokens_per_step_synthetic": round(n_new / r.steps, 3),
                "drafted": int(r.drafted[0]), "accepted": int(r.accepted[0]), "ids_head": got.ids[0][:12].tolist(),
                "speedup_synthetic": round(s * n_new / (l * r.steps), 3),
                "select_kernel": k_l, "select_kernel_no_gather": k_n,
                "no_draft": {"steps": n_bare, "sampled_step": stats(ts8), "lookup_step": stats(td),
                             "lookup_step_no_gather": stats(tdn), "gap_ms": round((d - s8) * 1e3, 4),
                             "gap_no_gather_ms": round((dn - s8) * 1e3, 4), "ratio": round(d / s8, 3),
                             "ratio_no_gather": round(dn / s8, 3), "select_kernel": k_d}})
    res["prefill_f16_redo"] = m.get_info().prefill_f16_redo
    m.close()
    out = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out + "\n")
    print(out)


if __name__ == "__main__":
    main()
