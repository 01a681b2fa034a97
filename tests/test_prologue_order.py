"""The prologue orders of the 4B decode launches (layer_body.h ORD, switch LLMI_PRO_ORDER=parent|barrier|split) hold
every tap of the traced decode step to the same bytes.

`barrier` puts one raw s_barrier between a work-group's prologue operand loads and its first weight loads, `split`
also issues the head's weight passes in groups between the prologue's steps.  Both move loads in program order only:
no operand, summation order or rounding changes, so the check is equality, not a tolerance -- hid, down, the qkv
granules (by value) and the merged attention blocks (xo_g words 0..9) among every other tap, as
test_ffn_geometry.py holds the tail-offset switch.

Shapes (scales="edge": zero blocks, negative and subnormal block scales in every row; a 40-token prompt, 2 traced
decode steps, seed 51, max_ctx 128):
* mini-4b -- the widths the switch acts on: the qkv role (80 blocks, PRO; standalone and inside the attention
  block), gate_up (80, GELU; H = 40 hidden units per work-group, so a work-group's units straddle the Q8_0 blocks of
  hid) and down (320, QUANT); prologue rounds with out-of-bounds slots; layer 0 runs PLAIN, later layers PRO;
* mini-4b-launches -- the same with LLMI_NO_BLOCK=1, the session's switch that keeps qkv, attention and o as three
  launches: the qkv role's standalone instances instead of the attention block's;
* mini-1b and mini-27b -- no entry of theirs has the instances: the switch must be inert.
Widths outside the launch table do not reach these launches, so there are no other shapes to try.
"""
import numpy as np
import pytest

from oplevel import granule_values

pytestmark = pytest.mark.gpu

SHAPES = {"mini-1b": ("mini-1b", False), "mini-4b": ("mini-4b", False), "mini-4b-launches": ("mini-4b", True),
          "mini-27b": ("mini-27b", False)}
N_PROMPT, N_DECODE, MAX_CTX, SEED = 40, 2, 128, 51
_runs = {}
_gguf = {}  # the last model built (the orders of one shape run back to back)


def _steps(shape, monkeypatch, order):
    """The traced decode steps of one shape under one order (taps per step), computed once and left unchanged."""
    key = (shape, order)
    if key in _runs:
        return _runs[key]
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    name, no_block = SHAPES[shape]
    cfg = CONFIGS[name]
    if name not in _gguf:
        _gguf.clear()
        _gguf[name] = build_gemma3_gguf(cfg, seed=SEED, swa_pattern=[True, False], scales="edge")
    g = _gguf[name]
    monkeypatch.delenv("LLMI_FFN_TAIL", raising=False)
    monkeypatch.setenv("LLMI_PRO_ORDER", order)
    if no_block:
        monkeypatch.setenv("LLMI_NO_BLOCK", "1")
    else:
        monkeypatch.delenv("LLMI_NO_BLOCK", raising=False)
    m = Model(g, max_ctx=MAX_CTX)
    prompt = np.random.default_rng(SEED).integers(4, cfg.vocab, N_PROMPT).astype(np.int32)
    taps = m.trace(prompt, 0)
    tok = int(np.frombuffer([b for n, l, b in taps if n == "token"][-1], np.int32)[0])
    steps, pos = [], N_PROMPT
    for _ in range(N_DECODE):
        taps = m.trace([tok], pos, gen=True)
        steps.append([(n, l, bytes(b)) for n, l, b in taps])
        tok = int(np.frombuffer([b for n, l, b in taps if n == "token"][-1], np.int32)[0])
        pos += 1
    m.close()
    _runs[key] = (steps, cfg.n_layer)
    return _runs[key]


@pytest.mark.parametrize("order", ["barrier", "split"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_prologue_order_bits_equal_parent(monkeypatch, shape, order):
    """Every tap of every step equal byte for byte with the parent order (granule taps, *_g, by their values: their
    other words are the launch's tag, which counts launches)."""
    new, n_layer = _steps(shape, monkeypatch, order)
    old, _ = _steps(shape, monkeypatch, "parent")
    assert len(new) == len(old) == N_DECODE
    seen = {"hid": 0, "down": 0, "qkv": 0, "qkv_g": 0, "xo_g": 0}
    for s, (a, b) in enumerate(zip(new, old)):
        assert [(n, l) for n, l, _ in a] == [(n, l) for n, l, _ in b], f"step {s}: the launches differ"
        for (n, l, x), (_, _, y) in zip(a, b):
            if n.endswith("_g"):
                x, y = granule_values(x).view(np.uint32), granule_values(y).view(np.uint32)
                if n == "xo_g":  # XBlock words: 8 of quants, d, nsum8 and two pads nothing writes or reads
                    x, y = x.reshape(-1, 12)[:, :10], y.reshape(-1, 12)[:, :10]
                x, y = x.tobytes(), y.tobytes()
            assert x == y, f"step {s}: tap {n} of layer {l} differs from the parent order ({order})"
            if n in seen:
                seen[n] += 1
    assert seen["hid"] == seen["down"] == n_layer * N_DECODE, seen
    if shape == "mini-4b":  # the attention block runs, its hand-offs are tapped
        assert seen["qkv_g"] == seen["xo_g"] == n_layer * N_DECODE, seen
    if shape == "mini-4b-launches":  # the three launches: the qkv rows as plain floats, no granules
        assert seen["qkv"] == n_layer * N_DECODE and seen["qkv_g"] == 0, seen

