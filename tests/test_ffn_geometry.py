"""The decode FFN launches (gate_up with the GELU epilogue, down with the QUANT prologue) through the op-level
harness (tests/oplevel.py, as test_fused_ops.py's test_ops_*), on scales="edge" weights (synthetic.SCALE_PROFILES:
zero blocks, negative and subnormal block scales in every row, the construction of test_ops_edge_scales):

* against the oracle from the device's own inputs, with OpChecker's bounds unchanged (gemv_gate_up_gelu, gemv_down);
* bit for bit against the same steps with LLMI_FFN_TAIL=late, the switch that restores the launches as they were
  before the tail passes' offsets were fixed ahead of the head issue (k_layer.hip fn_late): the change moves
  no operand and no summation, so every tap of the step is held to equality, not to a tolerance.

Shapes: the launch table (k_layer.hip kLayerCfgs) has GELU / QUANT entries for the Gemma-3 widths only, and
OpChecker.decode_step reads the fused step's taps, so the shapes are the table's: mini-1b (1152 x 6912: H = 32, the
smallest entries; their tail issue is untouched and the switch is inert, which the equality pins), mini-4b (2560 x
10240: the entries the switch acts on, H = 40 hidden units per work-group, so a work-group's units straddle the
32-element blocks of hid) and mini-27b (5376 x 21504: multi-chunk entries, rows over 672 work-groups).  Widths such
as 64 x 80 or 160 x 320 cannot be put through these launches: a Q4_0 row is whole 32-element blocks (an 80-column
down weight does not exist), and widths outside the table run the unfused kernels, whose steps the harness does
not read.
"""
import numpy as np
import pytest

from oplevel import OpChecker, granule_values

pytestmark = pytest.mark.gpu

SHAPES = {"mini-1b": ("name", "mini-1b"), "mini-4b": ("name", "mini-4b"), "mini-27b": ("name", "mini-27b")}
# test_ops_edge_scales' run (tests/test_fused_ops.py): a 40-token prompt, 2 decode steps, seed 51.  (A 9-token
# prompt with seed 61 put mini-27b's ATTENTION check, which this change does not touch, at 4.17e-5 against its 4e-5
# bound before any FFN launch was reached.)
N_PROMPT, N_DECODE, MAX_CTX, SEED = 40, 2, 128, 51
_runs = {}


def _cfg(shape):
    from llm_inference_amd.synthetic import CONFIGS, Gemma3Config
    kind, v = SHAPES[shape]
    return CONFIGS[v] if kind == "name" else Gemma3Config("ffn-" + shape, *v)


def _steps(shape, oracle, monkeypatch, late):
    """The traced decode steps of one shape (taps per step), computed once per (shape, switch) and left unchanged;
    the default run is checked op by op as it goes."""
    key = (shape, late)
    if key in _runs:
        return _runs[key]
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import build_gemma3_gguf
    cfg = _cfg(shape)
    swa = [True, False]
    g = build_gemma3_gguf(cfg, seed=SEED, swa_pattern=swa, scales="edge")
    if late:
        monkeypatch.setenv("LLMI_FFN_TAIL", "late")
    else:
        monkeypatch.delenv("LLMI_FFN_TAIL", raising=False)
    m = Model(g, max_ctx=MAX_CTX)
    chk = None if late else OpChecker(oracle, g, cfg, MAX_CTX, swa_pattern=swa)
    prompt = np.random.default_rng(SEED).integers(4, cfg.vocab, N_PROMPT).astype(np.int32)
    taps = m.trace(prompt, 0)
    tok = int(np.frombuffer([b for n, l, b in taps if n == "token"][-1], np.int32)[0])
    steps, pos = [], N_PROMPT
    for _ in range(N_DECODE):
        taps = m.trace([tok], pos, gen=True)
        steps.append([(n, l, bytes(b)) for n, l, b in taps])
        if chk is not None:
            chk.decode_step(taps, pos, gen=True, token=tok)
        tok = int(np.frombuffer([b for n, l, b in taps if n == "token"][-1], np.int32)[0])
        pos += 1
    m.close()
    _runs[key] = (steps, chk)
    return _runs[key]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_ffn_ops_against_oracle(oracle, monkeypatch, shape):
    """gate_up (GELU role) and down (QUANT role) of every layer and step within OpChecker's bounds of the oracle."""
    steps, chk = _steps(shape, oracle, monkeypatch, late=False)
    print(shape, {k: f"{v:.2e}" for k, v in sorted(chk.report.items())})
    assert "gemv_gate_up_gelu" in chk.report and "gemv_down" in chk.report
    names = {n for n, l, b in steps[0]}
    assert "hid" in names and "down" in names


@pytest.mark.parametrize("shape", list(SHAPES))
def test_ffn_bits_equal_late_tail(oracle, monkeypatch, shape):
    """Every tap of every step -- hid and down among them -- equal byte for byte with and without the switch
    (granule taps, *_g, by their values: their other words are the launch's tag, which counts launches)."""
    new, _ = _steps(shape, oracle, monkeypatch, late=False)
    old, _ = _steps(shape, oracle, monkeypatch, late=True)
    assert len(new) == len(old) == N_DECODE
    n_ffn = 0
    for s, (a, b) in enumerate(zip(new, old)):
        assert [(n, l) for n, l, _ in a] == [(n, l) for n, l, _ in b], f"step {s}: the launches differ"
        for (n, l, x), (_, _, y) in zip(a, b):
            if n.endswith("_g"):
                x, y = granule_values(x).view(np.uint32), granule_values(y).view(np.uint32)
                if n == "xo_g":  # XBlock words: 8 of quants, d, nsum8 and two pads nothing writes or reads
                    x, y = x.reshape(-1, 12)[:, :10], y.reshape(-1, 12)[:, :10]
                x, y = x.tobytes(), y.tobytes()
            assert x == y, f"step {s}: tap {n} of layer {l} differs from the late-tail launch"
            n_ffn += n in ("hid", "down")
    assert n_ffn == 2 * _cfg(shape).n_layer * N_DECODE
