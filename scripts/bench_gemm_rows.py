#!/usr/bin/env python3
"""The skinny GEMMs against the tiled launches they replace (DESIGN.md sections 17 and 18), in one process, alternating:

  (a) Model.time_kernel(15) -- the four projections' GEMMs of every layer at the row count of a batch step -- as a
      whole and per projection (LLMI_GR_ONLY), default against LLMI_PG_SKINNY=0: median of --repeats with min..max,
      us per layer, and the share of --hbm-gbps the weight bytes reach;
  (b) the batch_generate step at the same B, default against LLMI_PG_SKINNY=0.

--quant q8_0 builds the model with Q8_0 layers and --int8 runs the session with LLMI_PREFILL_F16=0: both put every
projection on the int8 GEMMs (section 18), and the skinny side then runs with LLMI_GR_I8_T=32 so that every row count
up to 32 reaches the skinny int8 kernel whatever the committed switch is.

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PROJ = ("qkv", "o", "gate_up", "down")


def stat(xs):
    return {"med": round(float(np.median(xs)), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--config", default="gemma-3-4b")
    p.add_argument("--prefill", type=int, default=512)
    p.add_argument("--steps", type=int, default=32)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--kernel-reps", type=int, default=5)
    p.add_argument("--batches", default="1,8,32,64")
    p.add_argument("--hbm-gbps", type=float, default=8000.0)
    p.add_argument("--quant", default="q4_0", choices=("q4_0", "q8_0"))
    p.add_argument("--int8", action="store_true")
    a = p.parse_args()
    i8 = a.int8 or a.quant == "q8_0"
    if a.int8:
        os.environ["LLMI_PREFILL_F16"] = "0"
    from llm_inference_amd.gguf import TensorType
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg = CONFIGS[a.config]
    wtype = TensorType.Q8_0 if a.quant == "q8_0" else TensorType.Q4_0
    batches = [int(b) for b in a.batches.split(",")]
    m = Model(build_gemma3_gguf(cfg, seed=1234, wtype=wtype), max_ctx=a.prefill + a.steps + 8)
    rng = np.random.default_rng(1)
    prompt = np.concatenate([[2], rng.integers(4, cfg.vocab, a.prefill - 1)]).astype(np.int32)
    m.forward(prompt, 0, want_logits=False)
    first, pos = m.last_argmax, a.prefill
    m.reserve_sequences(max(batches))
    for s in range(1, max(batches)):
        m.copy_sequence(s, 0, a.prefill)

    def mode(skinny):
        os.environ.pop("LLMI_PG_SKINNY", None)
        os.environ.pop("LLMI_GR_I8_T", None)
        if not skinny:
            os.environ["LLMI_PG_SKINNY"] = "0"
        elif i8:
            os.environ["LLMI_GR_I8_T"] = "32"

    def step(B):
        m.sync()
        t0 = time.perf_counter()
        m.batch_generate([first] * B, list(range(B)), [pos] * B, a.steps)
        return (time.perf_counter() - t0) / a.steps * 1e6

    def kern(only):
        os.environ.pop("LLMI_GR_ONLY", None)
        if only is not None:
            os.environ["LLMI_GR_ONLY"] = str(only)
        r = m.time_kernel(15, a.kernel_reps)
        os.environ.pop("LLMI_GR_ONLY", None)
        return r

    rows = []
    for B in batches:
        for sk in (True, False):  # warm both forms at this row count
            mode(sk)
            step(B)
            kern(None)
        st = {True: [], False: []}
        kt = {(sk, o): [] for sk in (True, False) for o in (None, 0, 1, 2, 3)}
        by = {}
        for _ in range(a.repeats):
            for sk in (True, False):
                mode(sk)
                st[sk].append(step(B))
                for o in (None, 0, 1, 2, 3):
                    us, by[o] = kern(o)
                    kt[(sk, o)].append(us)
        row = {"B": B, "step_us": {"skinny": stat(st[True]), "tiled": stat(st[False])}, "gemm_us_per_layer": {}}
        for o in (None, 0, 1, 2, 3):
            s_, t_ = stat(kt[(True, o)]), stat(kt[(False, o)])
            row["gemm_us_per_layer"]["all" if o is None else PROJ[o]] = {
                "skinny": s_, "tiled": t_, "weight_bytes": by[o],
                "skinny_hbm_share": round(by[o] / max(s_["med"], 1e-9) / 1e3 / a.hbm_gbps, 3)}
        rows.append(row)
    mode(True)
    os.environ.pop("LLMI_GR_I8_T", None)
    print(json.dumps({"config": cfg.name, "quant": a.quant, "int8": i8, "prefill": a.prefill, "steps": a.steps, "repeats": a.repeats,
                      "hbm_gbps": a.hbm_gbps, "rows": rows}))
    m.close()


if __name__ == "__main__":
    main()
