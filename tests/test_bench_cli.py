"""bench.py's command line on a reduced model: a plain run prints the headline line only, --dump-outputs writes
what the timed steps returned (and the next position's logits), and --full adds the measurements that take runs
of their own without changing what the timed path computes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG, PREFILL, WARMUP, STEPS = "mini-4b", 40, 3, 6
FULL_ONLY = ("kernel_families", "logits_gemv", "exact", "cpu_baseline", "parity_vs_reference")


def _bench(out_dir, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", CFG,
                        "--prefill", str(PREFILL), "--warmup", str(WARMUP), "--steps", str(STEPS),
                        "--dump-outputs", str(out_dir)] + list(extra), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    assert sorted(os.listdir(out_dir)) == ["next_logits.npy", "tokens.npy"]
    return (json.loads(lines[0]), np.load(os.path.join(out_dir, "tokens.npy")),
            np.load(os.path.join(out_dir, "next_logits.npy")))


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _bench(tmp_path_factory.mktemp("plain"))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_only(plain):
    line = plain[0]
    assert line["unit"] == "tokens/s" and line["higher_is_better"] is True and "q4_0" in line["dtype"]
    assert line["metric"].startswith("decode tokens/sec") and line["steps"] == STEPS and line["warmup"] == WARMUP
    # value and ms_per_step are the same measurement of one stream; ms_per_step is printed to 1e-4 ms, so a
    # step of 0.02 ms or more is off by at most 2.5e-3 of itself
    assert line["ms_per_step"] >= 0.02
    assert line["value"] * line["ms_per_step"] == pytest.approx(1000.0, rel=5e-3)
    assert not [k for k in FULL_ONLY if k in line] and "prefill_warm_s" not in line["timing_detail"]
    assert line["roofline"] is None


@pytest.mark.gpu
def test_dump_outputs_are_what_the_timed_steps_returned(plain):
    import bench
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    _, toks, logits = plain
    cfg = CONFIGS[CFG]
    assert toks.dtype == np.float64 and toks.shape == (STEPS,)
    assert logits.dtype == np.float32 and logits.shape == (cfg.vocab,)
    m = Model(build_gemma3_gguf(cfg, seed=1234), max_ctx=PREFILL + WARMUP + STEPS + 8)
    m.forward(bench.bench_prompt(cfg, PREFILL), 0, want_logits=False)
    m.enqueue(m.last_argmax, PREFILL, WARMUP)
    warm = m.sync(WARMUP)
    m.enqueue(int(warm[-1]), PREFILL + WARMUP, STEPS)
    want = m.sync(STEPS)
    want_logits = m.forward(want[-1:], PREFILL + WARMUP + STEPS)
    m.close()
    np.testing.assert_array_equal(toks, want.astype(np.float64))
    np.testing.assert_array_equal(logits.view(np.uint32), want_logits.view(np.uint32))


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements(plain, tmp_path):
    line, toks, logits = _bench(tmp_path, "--full", "--no-cpu-baseline")
    assert {"kernel_families", "logits_gemv", "exact"} <= set(line) and "prefill_warm_s" in line["timing_detail"]
    assert {"attention_block", "gate_up", "down"} <= set(line["kernel_families"])
    assert line["roofline"]["kernel"].split(":")[0] in line["kernel_families"]
    assert line["exact"]["steps"] == STEPS and line["exact"]["value"] > 0
    # the timed path is the same one, --full or not
    np.testing.assert_array_equal(toks, plain[1])
    np.testing.assert_array_equal(logits.view(np.uint32), plain[2].view(np.uint32))
