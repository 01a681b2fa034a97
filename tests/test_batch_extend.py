"""Ragged batch steps (llmi_session_batch_extend): spans of consecutive tokens, each on its own
KV slot at its own start position, in one step.

The row contract needs no tolerance.  If K/V rows 0..pos-1 of a slot were written by the batched prefill, by batch steps
or by earlier spans for x[0..pos), then for every token row at position p of a span running x[pos..pos+n) an output
row's argmax / lse are the last entries of Model.score(x[:p + 1]) and its logits Model.forward(x[:p + 1], 0) on a
single-sequence session -- whatever the other spans, the split into spans and calls, the slots, the span order,
LLMI_PREFILL_ATTN_KS and LLMI_BATCH_SPAN_ROWS.  The reference side is a Model that never reserves a slot.

Every test asserts that the f16-redo counter did not move, so the bits compared are the f16 path's.

mini-27b (head_dim 128: the attention's other key-split table) runs with LLMI_PG6=1 on both sides.  The batched
prefill picks the f16 GEMM of a wide projection by the launch's token rows (v7's 128 x 128 tiles once rows / 128 x
ceil(T / 128) reaches 512, v6 below), and the two sum K in different orders: on mini-27b (gate_up: 43008 rows) the
single-sequence session's own bits for a position change once its prompt is longer than 128 tokens --
score(x[:130])[:100] differs from score(x[:100]) there (measured on the parent commit) -- so score(x) and
forward(x[:p + 1], 0) no longer describe one row.  With one GEMM for every T the reference is a function of the row
again and the comparison is the attention's.  mini-1b never reaches the switch and mini-4b only past 384 token rows,
which no step here has; they run as they are.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CTX = 512
SEED = 21
# (pos, n): each side of a 32-key tile, a block that ends exactly on a tile edge, a span that crosses a query-block edge
# and the ks = 4 round boundary, a partial last block, position 0 as an output row (and, in the preloads, as none)
SPANS = ((0, 1), (0, 33), (5, 27), (30, 4), (31, 1), (96, 40), (0, 130))
# decode rows beside them: n = 1 spans at test_batch_decode.POS
DECODE = ((0, 1), (31, 1), (32, 1), (127, 1), (129, 1))
SLOTS = (3, 0, 4, 1, 2, 6, 5, 7, 8, 9, 10, 11)
N_SLOTS = 12
ENV_KEYS = ("LLMI_NO_PREFILL", "LLMI_PREFILL_CHUNK", "LLMI_PREFILL_FULL_LAST", "LLMI_PREFILL_ATTN_KS",
            "LLMI_PREFILL_ATTN_V1", "LLMI_PREFILL_F16", "LLMI_BATCH_SPAN_ROWS", "LLMI_PG6", "LLMI_PG7")
MODEL_ENV = {"mini-27b": {"LLMI_PG6": 1}}  # one prefill GEMM for every T (the module docstring)
CHAIN = (100, 101, 102, 103)  # chain_gguf


@contextlib.contextmanager
def env(**kv):
    """LLMI_* variables the library reads at the call, restored afterwards."""
    old = {k: os.environ.get(k) for k in ENV_KEYS}
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    for k, v in kv.items():
        os.environ[k] = str(v)
    try:
        yield
    finally:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def gguf(cfg_name):
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    return build_gemma3_gguf(CONFIGS[cfg_name], seed=SEED)


def vocab_of(cfg_name):
    from llm_inference_amd.synthetic import CONFIGS
    return CONFIGS[cfg_name].vocab


@functools.lru_cache(maxsize=None)
def chain_gguf(cfg_name):
    """test_batch_decode.chain_gguf's construction: four rows of the (tied, F16) token table rewritten so that the
    greedy sequence is CHAIN[0] -> CHAIN[1] -> CHAIN[2] -> CHAIN[3] -> CHAIN[3] (as built, the random model's greedy id
    is always its input token).  With u0..u3 the original, nearly orthogonal rows,
        w0 = u0,  w1 = 1.5 u0 + u1,  w2 = u0 + 2.5 u1 + u2,  w3 = 2.5 u1 + 3 u2 + u3.
    The tests read the sequence off the single-sequence reference and assert this shape before using it."""
    from llm_inference_amd.gguf import GGUFFile
    from llm_inference_amd.synthetic import CONFIGS
    cfg = CONFIGS[cfg_name]
    g = np.array(gguf(cfg_name), copy=True)
    f = GGUFFile(g)
    t = f.tensor("token_embd.weight")
    off = f.data_section_start + t.tensor_offset
    tab = g[off:off + cfg.vocab * cfg.n_embd * 2].view(np.float16).reshape(cfg.vocab, cfg.n_embd)
    u = tab[list(CHAIN)].astype(np.float32)
    coef = np.array([[1, 0, 0, 0], [1.5, 1, 0, 0], [1, 2.5, 1, 0], [0, 2.5, 3, 1]], np.float32)
    tab[list(CHAIN)] = (coef @ u).astype(np.float16)
    g.setflags(write=False)
    return g


def logit_rows(pos, n):
    """The positions of a span whose logits are compared: its last row and three inner rows."""
    return sorted({pos, pos + n // 3, pos + (2 * n) // 3, pos + n - 1})


@functools.lru_cache(maxsize=None)
def span_case(cfg_name, ks=None):
    """One sequence per span of SPANS + DECODE and the single-sequence session's results for it: every position's
    argmax / lse from one score(x), the logits of logit_rows by forward(x[:p + 1], 0).  Computed once per (model,
    key-split setting), read-only."""
    from llm_inference_amd.model import Model
    rng = np.random.default_rng(17)
    spans = SPANS + DECODE
    xs = [rng.integers(4, vocab_of(cfg_name), pos + n).astype(np.int32) for pos, n in spans]
    kv = dict(MODEL_ENV.get(cfg_name, {}))
    if ks is not None:
        kv["LLMI_PREFILL_ATTN_KS"] = ks
    am, lse, lg = [], [], []
    with env(**kv):
        ref = Model(gguf(cfg_name), max_ctx=CTX)
        for x, (pos, n) in zip(xs, spans):
            sc = ref.score(x)
            am.append(np.array(sc.argmax, np.int32))
            lse.append(np.array(sc.lse, np.float32))
            lg.append({p: ref.forward(x[:p + 1], 0) for p in logit_rows(pos, n)})
        assert ref.get_info().prefill_f16_redo == 0
        ref.close()
    return dict(spans=spans, xs=xs, kv=kv, argmax=am, lse=lse, logits=lg)


def preload(m, c, idx):
    """x[:pos] of every span that starts past 0, into its slot, with no outputs (position 0 as a non-output row): calls
    of at most 256 token rows, below mini-4b's GEMM switch (the module docstring)."""
    calls, rows = [[]], 0
    for i in idx:
        pos = c["spans"][i][0]
        if pos > 0:
            if rows + pos > 256:
                calls.append([])
                rows = 0
            calls[-1].append(i)
            rows += pos
    for pre in calls:
        if pre:
            r = m.batch_extend([c["xs"][i][:c["spans"][i][0]] for i in pre], [SLOTS[i] for i in pre], [0] * len(pre),
                               out="none")
            assert r.argmax.size == 0 and r.offsets.tolist() == [0] * (len(pre) + 1)


def run_spans(m, c, idx):
    return m.batch_extend([c["xs"][i][c["spans"][i][0]:] for i in idx], [SLOTS[i] for i in idx],
                          [c["spans"][i][0] for i in idx], out="all", want_logits=True)


def assert_spans(got, c, idx, what):
    assert got.offsets[-1] == sum(c["spans"][i][1] for i in idx) == got.argmax.size == got.lse.size == got.logits.shape[0]
    for k, i in enumerate(idx):
        pos, n = c["spans"][i]
        o = int(got.offsets[k])
        assert got.offsets[k + 1] - o == n
        msg = f"{what}: span {i} (pos {pos}, n {n})"
        np.testing.assert_array_equal(got.argmax[o:o + n], c["argmax"][i][pos:pos + n], err_msg=msg)
        np.testing.assert_array_equal(u32(got.lse[o:o + n]), u32(c["lse"][i][pos:pos + n]), err_msg=msg)
        for p, want in c["logits"][i].items():
            np.testing.assert_array_equal(u32(got.logits[o + p - pos]), u32(want), err_msg=f"{msg}, logits at {p}")


def no_redo(m):
    assert m.get_info().prefill_f16_redo == 0, "the f16 path overflowed: the bits compared would be the int8 path's"


def read_kv(m, slot, cfg_name):
    """test_batch_decode.read_kv: every layer's K and V cache of a slot, [layer][n_head_kv][CTX][head_dim] uint16,
    through Model.trace's kc / vc taps -- the slot is copied into slot 0 and a two-token prompt traced there, which
    rewrites rows 0 and 1 only, so rows 2.. are the slot's.  Slot 0 is clobbered."""
    from llm_inference_amd.synthetic import CONFIGS
    cfg = CONFIGS[cfg_name]
    if slot != 0:
        m.copy_sequence(0, slot, CTX)
    tr = m.trace([5, 6], 0)
    shape = (cfg.n_head_kv, CTX, cfg.head_dim)
    kc = np.stack([np.frombuffer(b, np.uint16).reshape(shape) for n, _l, b in tr if n == "kc"])
    vc = np.stack([np.frombuffer(b, np.uint16).reshape(shape) for n, _l, b in tr if n == "vc"])
    assert kc.shape[0] == cfg.n_layer and vc.shape[0] == cfg.n_layer
    return kc, vc


# ---------------------------------------------------------------------------
# 1. the span contract
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b", "mini-27b"])
def test_spans_equal_single_sequence_bits(cfg_name):
    from llm_inference_amd.model import Model
    c = span_case(cfg_name)
    idx = list(range(len(SPANS)))
    with env(**c["kv"]):
        m = Model(gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(N_SLOTS)
        preload(m, c, idx)
        got = run_spans(m, c, idx)
        no_redo(m)
        m.close()
    assert_spans(got, c, idx, f"{cfg_name}: one call")


# ---------------------------------------------------------------------------
# 2. independence of the step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b", "mini-27b"])
def test_spans_independent_of_the_step(cfg_name):
    """The same spans alone, in reversed order, and mixed into one call with five n = 1 decode rows."""
    from llm_inference_amd.model import Model
    c = span_case(cfg_name)
    ns = len(SPANS)
    every = list(range(ns + len(DECODE)))
    with env(**c["kv"]):
        m = Model(gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(N_SLOTS)
        preload(m, c, every)
        for i in range(ns):
            assert_spans(run_spans(m, c, [i]), c, [i], "alone")
        rev = list(range(ns))[::-1]
        assert_spans(run_spans(m, c, rev), c, rev, "reversed")
        mixed = [7, 0, 1, 8, 2, 3, 9, 4, 10, 5, 6, 11]
        assert_spans(run_spans(m, c, mixed), c, mixed, "mixed with decode rows")
        # "last" and "none" beside "all": only the compaction differs
        outs = ["last", "all", "none", "last", "all", "last", "last"]
        got = m.batch_extend([c["xs"][i][SPANS[i][0]:] for i in range(ns)], [SLOTS[i] for i in range(ns)],
                             [SPANS[i][0] for i in range(ns)], out=outs, want_logits=True)
        no_redo(m)
        m.close()
    assert got.offsets.tolist() == [0, 1, 34, 34, 35, 36, 37, 38]
    for k, o in enumerate(outs):
        pos, n = SPANS[k]
        at = int(got.offsets[k])
        if o == "last":
            assert got.argmax[at] == c["argmax"][k][-1] and u32(got.lse)[at] == u32(c["lse"][k])[-1], k
            np.testing.assert_array_equal(u32(got.logits[at]), u32(c["logits"][k][pos + n - 1]))
        elif o == "all":
            np.testing.assert_array_equal(got.argmax[at:at + n], c["argmax"][k][pos:])
            np.testing.assert_array_equal(u32(got.lse[at:at + n]), u32(c["lse"][k][pos:]))


@pytest.mark.parametrize("ks", [1, 8])
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b", "mini-27b"])
def test_spans_under_other_key_splits(cfg_name, ks):
    """LLMI_PREFILL_ATTN_KS = 1 (no merge launch) and 8, against a single-sequence session under the same setting."""
    from llm_inference_amd.model import Model
    c = span_case(cfg_name, ks)
    every = list(range(len(SPANS) + len(DECODE)))
    with env(**c["kv"]):
        m = Model(gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(N_SLOTS)
        preload(m, c, every)
        got = run_spans(m, c, every)
        no_redo(m)
        m.close()
    assert_spans(got, c, every, f"{cfg_name}: ks = {ks}")


@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b", "mini-27b"])
def test_spans_through_the_per_token_attention(cfg_name):
    """LLMI_BATCH_SPAN_ROWS=1: the step's attention through the per-token multi-sequence form gives the same bits."""
    from llm_inference_amd.model import Model
    c = span_case(cfg_name)
    every = list(range(len(SPANS) + len(DECODE)))
    with env(LLMI_BATCH_SPAN_ROWS=1, **c["kv"]):
        m = Model(gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(N_SLOTS)
        preload(m, c, every)
        got = run_spans(m, c, every)
        no_redo(m)
        m.close()
    assert_spans(got, c, every, f"{cfg_name}: per-token attention")


# ---------------------------------------------------------------------------
# 3. the K/V rows a span leaves
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_kv_rows_equal_forwards(cfg_name):
    from llm_inference_amd.model import Model
    x = np.random.default_rng(23).integers(4, vocab_of(cfg_name), 200).astype(np.int32)
    with env():
        m = Model(gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(4)
        m.batch_extend([x], [3], [0], out="none")
        kc1, vc1 = read_kv(m, 3, cfg_name)
        no_redo(m)
        m.close()
        m = Model(gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(4)
        m.forward(x, 0, want_logits=False)
        m.copy_sequence(3, 0, 200)
        kc0, vc0 = read_kv(m, 3, cfg_name)
        no_redo(m)
        m.close()
    np.testing.assert_array_equal(kc1[:, :, 2:200], kc0[:, :, 2:200])
    np.testing.assert_array_equal(vc1[:, :, 2:200], vc0[:, :, 2:200])
    assert kc0[:, :, 2:200].any() and vc0[:, :, 2:200].any()
    assert not kc1[:, :, 200:].any() and not vc1[:, :, 200:].any(), "rows at and past pos + n are not touched"


# ---------------------------------------------------------------------------
# 4. chunking and continuation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_chunking_is_exact(cfg_name):
    """A 300-token prompt as spans 7 + 64 + 129 + 100 over four calls, through prefill_sequences, and as one call."""
    from llm_inference_amd.model import Model
    x = np.random.default_rng(29).integers(4, vocab_of(cfg_name), 300).astype(np.int32)
    with env():
        ref = Model(gguf(cfg_name), max_ctx=CTX)
        sc = ref.score(x)
        ref.close()
        m = Model(gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(4)
        p = 0
        for n, out in ((7, "none"), (64, "none"), (129, "none"), (100, "last")):
            a = m.batch_extend([x[p:p + n]], [1], [p], out=out)
            p += n
        b = m.prefill_sequences([x], [2])
        d = m.batch_extend([x], [3], [0])
        kv = [read_kv(m, s, cfg_name) for s in (1, 2, 3)]
        no_redo(m)
        m.close()
    for r, what in ((a, "four calls"), (b, "prefill_sequences"), (d, "one call")):
        assert r.argmax.shape == (1,) and r.argmax[0] == sc.argmax[-1], what
        assert u32(r.lse)[0] == u32(sc.lse)[-1], what
    for kc, vc in kv[1:]:
        np.testing.assert_array_equal(kc[:, :, 2:300], kv[0][0][:, :, 2:300])
        np.testing.assert_array_equal(vc[:, :, 2:300], kv[0][1][:, :, 2:300])
        assert not kc[:, :, 300:].any() and not vc[:, :, 300:].any()


@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_batch_generate_continues_an_extended_slot(cfg_name):
    from llm_inference_amd.model import Model
    y = np.random.default_rng(37).integers(4, vocab_of(cfg_name), 34).astype(np.int32)
    y[-1] = CHAIN[0]
    with env():
        m = Model(chain_gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(3)
        m.forward(y[:-1], 0, want_logits=False)
        m.copy_sequence(2, 0, 33)
        last = m.prefill_sequences([y[:-1]], [1])
        assert last.argmax.shape == (1,)
        out = m.batch_generate([int(y[-1])] * 2, [1, 2], [33, 33], 6)
        no_redo(m)
        m.close()
    assert out[:4, 1].tolist() == [CHAIN[1], CHAIN[2], CHAIN[3], CHAIN[3]], out[:, 1]  # the chain: the ids do change
    np.testing.assert_array_equal(out[:, 0], out[:, 1])


# ---------------------------------------------------------------------------
# 5. draft verification
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_draft_verification(cfg_name):
    """Five draft tokens at position 64, right for two tokens and then wrong; then a restart at the first wrong position
    with the right token, over the stale rows."""
    from llm_inference_amd.model import Model
    V = vocab_of(cfg_name)
    rng = np.random.default_rng(43)
    prefix = rng.integers(4, V, 64).astype(np.int32)
    wrong = [int(t) for t in rng.integers(200, V, 2)]
    span = np.array([CHAIN[0], CHAIN[1], CHAIN[2]] + wrong, np.int32)  # CHAIN[0], then drafts: 2 right, 2 wrong
    x = np.concatenate([prefix, span])
    fixed = np.concatenate([prefix, [CHAIN[0], CHAIN[1], CHAIN[2], CHAIN[3]]]).astype(np.int32)
    with env():
        ref = Model(chain_gguf(cfg_name), max_ctx=CTX)
        sc = ref.score(x)
        sc2 = ref.score(fixed)
        lg2 = ref.forward(fixed, 0)
        ref.close()
        # the chain: the right ids are known
        assert sc.argmax[64:67].tolist() == [CHAIN[1], CHAIN[2], CHAIN[3]] and wrong[0] != CHAIN[3]
        m = Model(chain_gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(3)
        m.prefill_sequences([prefix], [2])
        got = m.batch_extend([span], [2], [64], out="all")
        np.testing.assert_array_equal(got.argmax, sc.argmax[64:])
        np.testing.assert_array_equal(u32(got.lse), u32(sc.lse[64:]))
        # accepted: the drafts that equal the previous row's id -- two -- and the third row's own id, the right token
        drafts = span[1:]
        n_ok = 0
        while n_ok < 4 and got.argmax[n_ok] == drafts[n_ok]:
            n_ok += 1
        assert n_ok == 2 and got.argmax[n_ok] == CHAIN[3]
        again = m.batch_extend([[int(got.argmax[n_ok])]], [2], [64 + n_ok + 1], want_logits=True)
        no_redo(m)
        m.close()
    assert again.argmax[0] == sc2.argmax[-1] and u32(again.lse)[0] == u32(sc2.lse)[-1]
    np.testing.assert_array_equal(u32(again.logits[0]), u32(lg2))


# ---------------------------------------------------------------------------
# 6. errors and refusals
# ---------------------------------------------------------------------------
def raises(status, word, fn, *a, **k):
    from llm_inference_amd._lib import LLMIError
    with pytest.raises(LLMIError) as ei:
        fn(*a, **k)
    assert ei.value.status == status and word in str(ei.value), (ei.value.status, str(ei.value))


def raw_extend(m, tokens, spans, n_spans=None):
    """The C entry point with no outputs; spans: (slot, pos, n_tokens, out) tuples or None."""
    from llm_inference_amd._lib import Span, check, lib, ptr
    t = None if tokens is None else np.ascontiguousarray(tokens, np.int32)
    arr = None if spans is None else (Span * max(len(spans), 1))(*[Span(*s) for s in spans])
    n = len(spans) if n_spans is None else n_spans
    check(lib().llmi_session_batch_extend(m.h, ptr(t) if t is not None else None, arr, n, None, None, None))


def test_argument_errors():
    from llm_inference_amd.model import Model
    cfg_name = "mini-1b"
    V = vocab_of(cfg_name)
    with env():
        m = Model(gguf(cfg_name), max_ctx=64)
        raises("E_ARG", "seq_reserve", m.batch_extend, [[5]], [0], [0])
        m.reserve_sequences(4)
        raises("E_RANGE", "n_spans", raw_extend, m, [5], [(0, 0, 1, 0)], 0)
        raises("E_RANGE", "n_spans", m.batch_extend, [[5]] * 5, [0, 1, 2, 3, 0], [0] * 5)
        raises("E_ARG", "duplicate slot", m.batch_extend, [[5], [6, 7]], [2, 2], [0, 0])
        raises("E_RANGE", "slot", m.batch_extend, [[5], [6]], [0, 4], [0, 0])
        raises("E_RANGE", "slot", m.batch_extend, [[5], [6]], [0, -1], [0, 0])
        raises("E_ARG", "n_tokens", m.batch_extend, [[5], []], [0, 1], [0, 0])
        raises("E_ARG", "out", raw_extend, m, [5], [(0, 0, 1, 3)])
        raises("E_ARG", "out", raw_extend, m, [5], [(0, 0, 1, -1)])
        raises("E_RANGE", "pos", m.batch_extend, [[5]], [0], [-1])
        raises("E_RANGE", "pos", m.batch_extend, [[5, 6]], [0], [63])
        raises("E_RANGE", "pos", m.batch_extend, [[5]], [0], [64])
        raises("E_RANGE", "tokens", m.batch_extend, [[5, V]], [0], [0])
        raises("E_RANGE", "tokens", m.batch_extend, [[5], [-1]], [0, 1], [0, 0])
        raises("E_ARG", "tokens", raw_extend, m, None, [(0, 0, 1, 0)])
        raises("E_ARG", "spans", raw_extend, m, [5], None, 1)
        # more than LLMI_BATCH_TOKENS_MAX token rows: nine spans of 60
        m.reserve_sequences(9)
        raises("E_RANGE", "n_tokens", m.batch_extend, [[5] * 60] * 9, list(range(9)), [0] * 9, out="none")
        # batch_forward keeps its duplicate-slot refusal
        raises("E_ARG", "slots", m.batch_forward, [5, 6], [2, 2], [0, 0])
        # a call whose spans are all "none" takes NULL outputs
        raw_extend(m, [5, 6, 7], [(1, 0, 3, 2)])
        r = m.batch_extend([[5, 6, 7], [8]], [1, 2], [0, 0], out="none")
        assert r.argmax.size == 0 and r.lse.size == 0 and r.logits is None and r.offsets.tolist() == [0, 0, 0]
        # the session still works, single-sequence and batched
        x = np.array([5, 6, 7, 9], np.int32)
        want = m.score(x)
        got = m.batch_extend([[9]], [1], [3])
        assert got.argmax[0] == want.argmax[-1] and u32(got.lse)[0] == u32(want.lse)[-1]
        no_redo(m)
        m.close()


def test_refusals_come_from_seq_reserve():
    from llm_inference_amd.gguf import TensorType as TT
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    with env():
        m = Model(build_gemma3_gguf(CONFIGS["tiny"], seed=7), exact=True, max_ctx=64)
        raises("E_ARG", "exact", m.reserve_sequences, 2)
        raises("E_ARG", "seq_reserve", m.batch_extend, [[5, 6]], [0], [0])
        m.close()
        gk = build_gemma3_gguf(CONFIGS["mini-4b"], seed=SEED, wtype=TT.Q4_K, wtypes={"v": TT.Q6_K, "down": TT.Q6_K})
        m = Model(gk, max_ctx=64)
        raises("E_ARG", "K-quant", m.reserve_sequences, 2)
        raises("E_ARG", "seq_reserve", m.batch_extend, [[5, 6]], [0], [0])
        m.close()


# ---------------------------------------------------------------------------
# 7. time_kernel(12)
# ---------------------------------------------------------------------------
def test_time_kernel_span_attention():
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS
    cfg_name = "mini-4b"
    cfg = CONFIGS[cfg_name]
    c = span_case(cfg_name)
    idx = list(range(len(SPANS)))
    # per layer: K and V rows 0 .. last position of every query block (32 tokens of a span), once per block, f16
    rows = sum(pos + min(j + 32, n) for pos, n in SPANS for j in range(0, n, 32))
    want = float(rows * 2 * cfg.n_head_kv * cfg.head_dim * 2)
    with env():
        m = Model(gguf(cfg_name), max_ctx=CTX)
        assert m.time_kernel(12, 2) == (0.0, 0.0)
        m.reserve_sequences(N_SLOTS)
        assert m.time_kernel(12, 2) == (0.0, 0.0)
        preload(m, c, idx)
        run_spans(m, c, idx)
        us, by = m.time_kernel(12, 3)
        print(f"time_kernel(12), span form: {us:.1f} us per layer for {by:.0f} bytes")
        assert us > 0.0 and by == want
        # the launch leaves the step's outputs as they were: the spans again, same bits
        assert_spans(run_spans(m, c, idx), c, idx, "after timing")
        with env(LLMI_BATCH_SPAN_ROWS=1):
            run_spans(m, c, idx)
            us1, by1 = m.time_kernel(12, 3)
        print(f"time_kernel(12), per-token form: {us1:.1f} us per layer for {by1:.0f} bytes")
        assert us1 > 0.0 and by1 == want
        # batch_forward's hook is its own
        assert m.time_kernel(10, 2) == (0.0, 0.0)
        no_redo(m)
        m.close()
