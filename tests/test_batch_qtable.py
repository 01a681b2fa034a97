"""Batch steps on a Q8_0 output table, opt-in (LLMI_BATCH_QTABLE / Model(batch_qtable=True)).

Row contract, no tolerance: a row's logits are those of forward(the row's whole sequence, 0) on a single-sequence
session of the same file (no flag: the parent commit's path), its arg-max their first-index arg-max, its lse the f64
row reduce of them -- max, sum of exp(l - max), M + log(sum), rounded once to f32; restated here in numpy f64 (the
kernel's summation order moves the f64 value by parts in 1e16, far below the f32 rounding), and the per-row launch
(LLMI_BATCH_QTABLE_ROWS=0) must give the rows launch's bits.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CTX = 128
LENS = (1, 2, 33, 70)  # a one-token prompt (forward's decode step), two tokens, past a 32-key tile, past 64
SLOTS = (2, 0, 3, 1)
LAYERS = ["Q8_0", "Q4_0"]
PROMPTS = [tuple(int(t) for t in np.random.default_rng(11).integers(4, 2048, n)) for n in LENS]


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def gguf(layers):
    from llm_inference_amd.gguf import TensorType as TT
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    return build_gemma3_gguf(CONFIGS["mini-1b"], seed=21, wtype=getattr(TT, layers), embd_type=TT.Q8_0)


@functools.lru_cache(maxsize=None)
def reference(layers):
    """forward(x, 0)'s logits on one single-sequence session per file, each sequence computed once."""
    from llm_inference_amd.model import Model
    ref = Model(gguf(layers), max_ctx=CTX)

    @functools.lru_cache(maxsize=None)
    def logits(seq):
        lg = ref.forward(np.array(seq, np.int32), 0)
        lg.setflags(write=False)
        return lg
    return logits


def model(layers, n_seq):
    from llm_inference_amd.model import Model
    m = Model(gguf(layers), max_ctx=CTX, batch_qtable=True)
    m.reserve_sequences(n_seq)
    assert m.get_info().n_seq == n_seq and m.get_info().score_path == 2
    return m


def check_rows(layers, seqs, logits, argmax, lse, what):
    for i, seq in enumerate(seqs):
        want = reference(layers)(tuple(seq))
        x = want.astype(np.float64)
        if logits is not None:
            np.testing.assert_array_equal(u32(logits[i]), u32(want), err_msg=f"{what}: logits of row {i}")
        assert argmax[i] == int(np.argmax(want)), f"{what}: arg-max of row {i}"
        assert u32(lse[i]) == u32(np.float32(x.max() + np.log(np.exp(x - x.max()).sum()))), f"{what}: lse of row {i}"


def test_refusal_unchanged_without_the_flag():
    from llm_inference_amd._lib import LLMIError
    from llm_inference_amd.model import Model
    m = Model(gguf("Q8_0"), max_ctx=CTX)
    with pytest.raises(LLMIError) as ei:
        m.reserve_sequences(2)
    assert ei.value.status == "E_ARG" and "F16 output table" in str(ei.value) and m.get_info().n_seq == 1
    m.close()


@pytest.mark.parametrize("rows_env", [None, "0"], ids=["default", "per-row"])
@pytest.mark.parametrize("layers", LAYERS)
def test_batch_forward_rows_equal_forward(layers, rows_env, monkeypatch):
    if rows_env is not None:
        monkeypatch.setenv("LLMI_BATCH_QTABLE_ROWS", rows_env)
    nxt = [7, 8, 9, 10]
    m = model(layers, 4)
    pre = m.prefill_sequences(PROMPTS, SLOTS)
    check_rows(layers, PROMPTS, None, pre.argmax, pre.lse, "prefill_sequences")
    seqs = [p + (t,) for p, t in zip(PROMPTS, nxt)]
    for order in ([0, 1, 2, 3], [3, 2, 1, 0]):
        got = m.batch_forward([nxt[i] for i in order], [SLOTS[i] for i in order], [LENS[i] for i in order],
                              want_logits=True)
        check_rows(layers, [seqs[i] for i in order], got.logits, got.argmax, got.lse, f"order {order}")
    m.close()


@pytest.mark.parametrize("layers", LAYERS)
def test_batch_generate_greedy_and_sampled(layers):
    from llm_inference_amd import ops
    ps, steps = PROMPTS[1:], 12
    sp = dict(temperature=0.9, top_k=40, top_p=0.95, seed=5)

    def chain(seq, sampler, stop):
        out = []
        while len(out) < steps:
            lg = reference(layers)(tuple(seq))
            tok = int(np.argmax(lg)) if sampler is None else ops.sample_logits(lg, len(seq) - 1, **sampler)
            out.append(tok)
            if tok == stop:
                break
            seq = seq + (tok,)
        return out + [-1] * (steps - len(out))

    stop = chain(ps[1], None, -1)[5]  # row 1 stops at step 5 at the latest
    m = model(layers, 4)
    for samplers in (None, [None, None, sp]):
        m.prefill_sequences([p[:-1] for p in ps], SLOTS[1:])
        got = m.batch_generate([p[-1] for p in ps], SLOTS[1:], [len(p) - 1 for p in ps], steps, stop=[stop],
                               samplers=samplers)
        want = np.array([chain(p, samplers and samplers[b], stop) for b, p in enumerate(ps)]).T
        assert (want[:, 1] == -1).any()
        np.testing.assert_array_equal(got, want)
    m.close()


def test_batch_extend_all_rows_cross_the_64_row_chunk():
    span, dec = PROMPTS[3], PROMPTS[2]
    m = model("Q8_0", 2)
    m.prefill_sequences([dec[:-1]], [0])
    got = m.batch_extend([span, dec[-1:]], [1, 0], [0, len(dec) - 1], out=["all", "last"], want_logits=True)
    m.close()
    assert got.argmax.size == 71
    check_rows("Q8_0", [span[:i + 1] for i in range(len(span))] + [dec], got.logits, got.argmax, got.lse, "extend")


def test_lookup_sampled_equals_batch_generate():
    ps = [p + p[-8:] for p in PROMPTS[2:]]  # (a repeated tail: the n-gram search finds drafts)
    sps = [dict(temperature=0.8, top_k=20, top_p=0.9, seed=3), None]
    rows = ([0, 1], [len(p) - 1 for p in ps])
    m = model("Q8_0", 2)
    m.prefill_sequences([p[:-1] for p in ps], rows[0])
    want = m.batch_generate([p[-1] for p in ps], *rows, 10, samplers=sps)
    m.prefill_sequences([p[:-1] for p in ps], rows[0])
    got = m.batch_generate_lookup_sampled(ps, *rows, 10, sps, draft_len=3)
    m.close()
    for b in range(2):
        np.testing.assert_array_equal(got.ids[b], want[:, b])
