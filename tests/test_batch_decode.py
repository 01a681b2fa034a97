"""Several sequences per step (llmi_session_seq_* / llmi_session_batch_*).

The row contract needs no tolerance: if K/V rows 0..p-1 of a slot were written by the batched prefill or by batch steps
for tokens x[0..p), a batch step running x[p] at position p of that slot gives the bits of the last position of
Model.score(x[:p + 1]) / Model.forward(x[:p + 1], 0) on a single-sequence session -- whatever B, the other rows, the
slot and the row order.  The reference side is a Model that never reserves a slot (the parent commit's paths).
"""
import contextlib
import functools
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CTX = 512
POS = (0, 31, 32, 127, 129)   # each side of a 32-key tile and of a full round of ks = 4 tiles
SLOTS = (3, 0, 4, 1, 2)
ENV_KEYS = ("LLMI_NO_PREFILL", "LLMI_PREFILL_CHUNK", "LLMI_PREFILL_FULL_LAST", "LLMI_PREFILL_ATTN_KS",
            "LLMI_PREFILL_ATTN_V1", "LLMI_PREFILL_F16")


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
    return build_gemma3_gguf(CONFIGS[cfg_name], seed=21)


def vocab_of(cfg_name):
    from llm_inference_amd.synthetic import CONFIGS
    return CONFIGS[cfg_name].vocab


@functools.lru_cache(maxsize=None)
def contract_case(cfg_name, ks=None):
    """The five prompts and, per prompt, the single-sequence session's last position: (argmax, lse, logits).
    Computed once per (model, key-split setting), read-only."""
    from llm_inference_amd.model import Model
    rng = np.random.default_rng(11)
    prompts = [rng.integers(4, vocab_of(cfg_name), p + 1).astype(np.int32) for p in POS]
    kv = {} if ks is None else {"LLMI_PREFILL_ATTN_KS": ks}
    am, lse, lg = [], [], []
    with env(**kv):
        ref = Model(gguf(cfg_name), max_ctx=CTX)
        for x in prompts:
            sc = ref.score(x)
            am.append(int(sc.argmax[-1]))
            lse.append(sc.lse[-1])
            lg.append(ref.forward(x, 0))
        ref.close()
    lg = np.stack(lg)
    lg.setflags(write=False)
    return dict(prompts=prompts, kv=kv, argmax=np.array(am, np.int32), lse=np.array(lse, np.float32), logits=lg)


def load_prefixes(m, prompts, slots):
    """x[:-1] of every prompt through forward() (slot 0), copied to its slot; the row that lives in slot 0 last."""
    order = sorted(range(len(prompts)), key=lambda i: slots[i] == 0)
    for i in order:
        p = len(prompts[i]) - 1
        if p > 0:
            m.forward(prompts[i][:p], 0, want_logits=False)
            m.copy_sequence(slots[i], 0, p)


def rows_of(prompts, slots, idx):
    return ([int(prompts[i][-1]) for i in idx], [slots[i] for i in idx], [len(prompts[i]) - 1 for i in idx])


def assert_rows(got, c, idx, what, logits=True):
    np.testing.assert_array_equal(got.argmax, c["argmax"][idx], err_msg=what)
    np.testing.assert_array_equal(u32(got.lse), u32(c["lse"][idx]), err_msg=what)
    if logits:
        np.testing.assert_array_equal(u32(got.logits), u32(c["logits"][idx]), err_msg=what)


def read_kv(m, slot, cfg_name):
    """Every layer's K and V cache of a slot, [layer][n_head_kv][CTX][head_dim] uint16, through Model.trace's kc / vc
    taps: the slot is copied into slot 0 and a two-token prompt traced there, which rewrites rows 0 and 1 only --
    so rows 2.. are the slot's.  Slot 0 is clobbered."""
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
# 1. rows equal the single-sequence bits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b", "mini-27b"])
def test_rows_equal_single_sequence_bits(cfg_name):
    from llm_inference_amd.model import Model
    c = contract_case(cfg_name)
    with env():
        m = Model(gguf(cfg_name), max_ctx=CTX)
        assert m.get_info().n_seq == 1
        m.reserve_sequences(5)
        assert m.get_info().n_seq == 5
        load_prefixes(m, c["prompts"], SLOTS)
        idx = list(range(5))
        got = m.batch_forward(*rows_of(c["prompts"], SLOTS, idx), want_logits=True)
        m.close()
    assert_rows(got, c, idx, f"{cfg_name}: B = 5")


# ---------------------------------------------------------------------------
# 2. independence of the batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b", "mini-27b"])
def test_rows_independent_of_the_batch(cfg_name):
    """The same rows alone (B = 1), reversed, and inside B = 33 (across the 32-token MFMA tile) among unrelated rows."""
    from llm_inference_amd.model import Model
    c = contract_case(cfg_name)
    V = vocab_of(cfg_name)
    with env():
        m = Model(gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(5)
        load_prefixes(m, c["prompts"], SLOTS)
        for i in range(5):
            assert_rows(m.batch_forward(*rows_of(c["prompts"], SLOTS, [i]), want_logits=True), c, [i], f"B = 1, row {i}")
        rev = [4, 3, 2, 1, 0]
        assert_rows(m.batch_forward(*rows_of(c["prompts"], SLOTS, rev), want_logits=True), c, rev, "reversed")
        # B = 33: the five rows at indices on both sides of the 32-row tile, the rest unrelated rows on slots 5..32
        m.reserve_sequences(33)  # (a larger reserve keeps the existing slots' rows)
        assert m.get_info().n_seq == 33
        where = {0: 0, 7: 1, 16: 2, 31: 3, 32: 4}
        rng = np.random.default_rng(5)
        tok, sl, ps, spare = [], [], [], iter(range(5, 33))
        for b in range(33):
            if b in where:
                t, s, p = rows_of(c["prompts"], SLOTS, [where[b]])
                tok, sl, ps = tok + t, sl + s, ps + p
            else:
                tok.append(int(rng.integers(4, V)))
                sl.append(next(spare))
                ps.append(int(rng.integers(0, 200)))
        got = m.batch_forward(tok, sl, ps, want_logits=True)
        m.close()
    at = list(where)
    np.testing.assert_array_equal(got.argmax[at], c["argmax"])
    np.testing.assert_array_equal(u32(got.lse[at]), u32(c["lse"]))
    np.testing.assert_array_equal(u32(got.logits[at]), u32(c["logits"]))


@pytest.mark.parametrize("ks", [1, 8])
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b", "mini-27b"])
def test_rows_under_other_key_splits(cfg_name, ks):
    """LLMI_PREFILL_ATTN_KS = 1 (no merge launch) and 8: batch rows against a single-sequence session under the same
    setting."""
    from llm_inference_amd.model import Model
    c = contract_case(cfg_name, ks)
    with env(**c["kv"]):
        m = Model(gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(5)
        load_prefixes(m, c["prompts"], SLOTS)
        idx = list(range(5))
        got = m.batch_forward(*rows_of(c["prompts"], SLOTS, idx), want_logits=True)
        m.close()
    assert_rows(got, c, idx, f"{cfg_name}: ks = {ks}")


# ---------------------------------------------------------------------------
# 3. / 4. the loop and its stop ids
# ---------------------------------------------------------------------------
LOOP_LEN = (1, 6, 34, 131)  # prompt lengths: the first row starts at position 0
LOOP_SLOTS = (2, 4, 1, 3)   # (slot 0 stays free: read_kv uses it)
N_STEPS = 6
CHAIN = (100, 101, 102, 103)  # chain_gguf
CHAIN_ROW = 2


@functools.lru_cache(maxsize=None)
def chain_gguf(cfg_name):
    """The synthetic model with four rows of its (tied, F16) token table rewritten.  As built, the random model's
    greedy id is always its input token (the tied table dominates the logits), so no greedy sequence ever changes.
    With u0..u3 the original, nearly orthogonal rows of the CHAIN tokens, the rows become
        w0 = u0,  w1 = 1.5 u0 + u1,  w2 = u0 + 2.5 u1 + u2,  w3 = 2.5 u1 + 3 u2 + u3,
    for which <w_next, w_t / |w_t|> exceeds every other row's product when t is fed: t0 -> t1 -> t2 -> t3 -> t3.
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


@functools.lru_cache(maxsize=None)
def loop_case(cfg_name, seed):
    """Prompts and the reference ids: iterate score(x).argmax[-1] and append, on a single-sequence session.
    ids[b][i] = row b's id after step i; lse likewise; one step more than N_STEPS (what batch_forward continues to)."""
    from llm_inference_amd.model import Model
    rng = np.random.default_rng(100 + seed)
    prompts = [rng.integers(4, vocab_of(cfg_name), n).astype(np.int32) for n in LOOP_LEN]
    prompts[CHAIN_ROW][-1] = CHAIN[0]
    ids = np.zeros((len(prompts), N_STEPS + 1), np.int32)
    lse = np.zeros((len(prompts), N_STEPS + 1), np.float32)
    with env():
        ref = Model(chain_gguf(cfg_name), max_ctx=CTX)
        for b, x in enumerate(prompts):
            x = list(x)
            for i in range(N_STEPS + 1):
                sc = ref.score(np.array(x, np.int32))
                ids[b, i], lse[b, i] = sc.argmax[-1], sc.lse[-1]
                x.append(int(ids[b, i]))
        ref.close()
    return dict(prompts=prompts, ids=ids, lse=lse)


@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_batch_generate_equals_iterated_score(cfg_name):
    from llm_inference_amd.model import Model
    c = loop_case(cfg_name, 0)
    first, sl, ps = rows_of(c["prompts"], LOOP_SLOTS, range(4))
    with env():
        m = Model(chain_gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(5)
        load_prefixes(m, c["prompts"], LOOP_SLOTS)
        out = m.batch_generate(first, sl, ps, N_STEPS)
        assert out.shape == (N_STEPS, 4) and out.dtype == np.int32
        np.testing.assert_array_equal(out, c["ids"][:, :N_STEPS].T)
        # the K/V rows the loop appended carry the same bits: the next step continues from them
        nxt = m.batch_forward(out[-1], sl, [p + N_STEPS for p in ps])
        m.close()
    np.testing.assert_array_equal(nxt.argmax, c["ids"][:, N_STEPS])
    np.testing.assert_array_equal(u32(nxt.lse), u32(c["lse"][:, N_STEPS]))


def pick_stop(ids):
    """(row, stop id): the row first emits the id at step 2 and some other row never emits it."""
    for r in range(ids.shape[0]):
        s = int(ids[r, 2])
        if s in ids[r, :2]:
            continue
        if any(q != r and s not in ids[q, :N_STEPS] for q in range(ids.shape[0])):
            return r, s
    return None


@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_stop_ids(cfg_name):
    from llm_inference_amd.model import Model
    c = loop_case(cfg_name, 0)
    pick = pick_stop(c["ids"])
    assert pick, ("no row first emits an id at step 2 which another row never emits", c["ids"].tolist())
    r, stop = pick
    ids = c["ids"][:, :N_STEPS]
    first, sl, ps = rows_of(c["prompts"], LOOP_SLOTS, range(4))
    with env():
        m = Model(chain_gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(6)
        # junk in the stopped row's slot first, so that "appends nothing" is visible: 200 rows of another sequence
        m.forward(np.random.default_rng(9).integers(4, vocab_of(cfg_name), 200).astype(np.int32), 0, want_logits=False)
        m.copy_sequence(LOOP_SLOTS[r], 0, 200)
        load_prefixes(m, c["prompts"], LOOP_SLOTS)
        kc0, vc0 = read_kv(m, LOOP_SLOTS[r], cfg_name)
        out = m.batch_generate(first, sl, ps, N_STEPS, stop=[stop])
        kc1, vc1 = read_kv(m, LOOP_SLOTS[r], cfg_name)
        m.close()
    never = 0
    for b in range(4):
        hit = np.flatnonzero(ids[b] == stop)
        if hit.size == 0:
            never += 1
            np.testing.assert_array_equal(out[:, b], ids[b], err_msg=f"row {b} never stops")
        else:
            k = int(hit[0])
            np.testing.assert_array_equal(out[:k + 1, b], ids[b, :k + 1], err_msg=f"row {b} up to its stop id")
            assert (out[k + 1:, b] == -1).all(), (b, out[:, b])
    assert never >= 1 and int(np.flatnonzero(ids[r] == stop)[0]) == 2
    # step 2 ran at ps[r] + 2 and emitted the stop id, which would have taken ps[r] + 3
    cut = max(ps[r] + 3, 2)
    np.testing.assert_array_equal(kc1[:, :, cut:], kc0[:, :, cut:])
    np.testing.assert_array_equal(vc1[:, :, cut:], vc0[:, :, cut:])
    lo = max(ps[r], 2)
    assert (kc1[:, :, lo:cut] != kc0[:, :, lo:cut]).any(), "the steps before the stop appended their rows"


# ---------------------------------------------------------------------------
# 5. fork
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_fork(cfg_name):
    from llm_inference_amd.model import Model
    rng = np.random.default_rng(31)
    V = vocab_of(cfg_name)
    x = rng.integers(4, V, 40).astype(np.int32)
    forced = rng.integers(4, V, (2, 2)).astype(np.int32)  # [branch][step]
    with env():
        ref = Model(gguf(cfg_name), max_ctx=CTX)
        want = [[ref.score(np.concatenate([x, forced[br, :i + 1]])) for i in range(2)] for br in range(2)]
        ref.close()
        m = Model(gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(3)
        m.forward(x, 0, want_logits=False)
        m.copy_sequence(1, 0, 40)
        kc0, vc0 = read_kv(m, 1, cfg_name)
        m.copy_sequence(2, 1, 40)
        for i in range(2):
            got = m.batch_forward(forced[:, i], [1, 2], [40 + i, 40 + i])
            for br in range(2):
                assert got.argmax[br] == want[br][i].argmax[-1], (br, i)
                assert u32(got.lse)[br] == u32(want[br][i].lse)[-1], (br, i)
        kc1, vc1 = read_kv(m, 1, cfg_name)
        m.close()
    np.testing.assert_array_equal(kc1[:, :, 2:40], kc0[:, :, 2:40])
    np.testing.assert_array_equal(vc1[:, :, 2:40], vc0[:, :, 2:40])
    assert (kc1[:, :, 40:42] != kc0[:, :, 40:42]).any()


# ---------------------------------------------------------------------------
# 6. slot 0 is still the session
# ---------------------------------------------------------------------------
def test_slot0_is_still_the_session():
    from llm_inference_amd.model import Model
    cfg_name = "mini-4b"
    c = contract_case(cfg_name)
    prompt = np.random.default_rng(41).integers(4, vocab_of(cfg_name), 70).astype(np.int32)
    slots = (3, 7, 4, 1, 2)

    def single(m):
        lg = m.forward(prompt, 0)
        gen = m.generate(int(np.argmax(lg)), len(prompt), 5)
        sc = m.score(prompt)
        return lg, gen, sc

    with env():
        fresh = Model(gguf(cfg_name), max_ctx=CTX)
        want = single(fresh)
        fresh.close()
        m = Model(gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(8)
        load_prefixes(m, c["prompts"], slots)
        idx = list(range(5))
        assert_rows(m.batch_forward(*rows_of(c["prompts"], slots, idx), want_logits=True), c, idx, "before")
        m.batch_generate(*rows_of(c["prompts"], slots, idx), 3)
        got = single(m)
        np.testing.assert_array_equal(u32(got[0]), u32(want[0]))
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[2].argmax, want[2].argmax)
        np.testing.assert_array_equal(u32(got[2].lse), u32(want[2].lse))
        np.testing.assert_array_equal(u32(got[2].logprobs), u32(want[2].logprobs))
        # and the reverse: batch rows after those calls
        assert_rows(m.batch_forward(*rows_of(c["prompts"], slots, idx), want_logits=True), c, idx, "after")
        m.close()


# ---------------------------------------------------------------------------
# 7. errors and refusals
# ---------------------------------------------------------------------------
def raises(status, word, fn, *a, **k):
    from llm_inference_amd._lib import LLMIError
    with pytest.raises(LLMIError) as ei:
        fn(*a, **k)
    assert ei.value.status == status and word in str(ei.value), (ei.value.status, str(ei.value))


def test_argument_errors():
    import ctypes as C

    from llm_inference_amd._lib import SessionInfo
    from llm_inference_amd.model import Model
    cfg_name = "mini-1b"
    V = vocab_of(cfg_name)
    assert C.sizeof(SessionInfo) == 136
    with env():
        m = Model(gguf(cfg_name), max_ctx=64)
        assert m.get_info().n_seq == 1
        raises("E_ARG", "seq_reserve", m.batch_forward, [5], [0], [0])
        raises("E_ARG", "seq_reserve", m.batch_generate, [5], [0], [0], 2)
        raises("E_ARG", "seq_reserve", m.copy_sequence, 1, 0, 4)
        raises("E_RANGE", "n_seq", m.reserve_sequences, 0)
        raises("E_RANGE", "n_seq", m.reserve_sequences, 65)
        m.reserve_sequences(4)
        assert m.get_info().n_seq == 4
        raises("E_RANGE", "slots", m.batch_forward, [5, 6], [0, 4], [0, 0])
        raises("E_RANGE", "slots", m.batch_forward, [5, 6], [0, -1], [0, 0])
        raises("E_ARG", "slots", m.batch_forward, [5, 6], [2, 2], [0, 0])
        raises("E_RANGE", "(B)", m.batch_forward, [5] * 5, [0, 1, 2, 3, 0], [0] * 5)
        raises("E_RANGE", "tokens", m.batch_forward, [5, V], [0, 1], [0, 0])
        raises("E_RANGE", "tokens", m.batch_generate, [-1], [0], [0], 2)
        raises("E_RANGE", "pos + n_steps", m.batch_forward, [5], [0], [64])
        raises("E_RANGE", "pos + n_steps", m.batch_forward, [5], [0], [-1])
        raises("E_RANGE", "pos + n_steps", m.batch_generate, [5], [0], [60], 5)
        raises("E_ARG", "n_stop", m.batch_generate, [5], [0], [0], 2, stop=[1, 2, 3, 4, 5])
        raises("E_RANGE", "dst", m.copy_sequence, 4, 0, 4)
        raises("E_RANGE", "src", m.copy_sequence, 0, 9, 4)
        raises("E_RANGE", "n_pos", m.copy_sequence, 1, 0, 65)
        # the session still works, single-sequence and batched
        x = np.array([5, 6, 7], np.int32)
        want = m.score(x)
        m.copy_sequence(2, 0, 2)
        got = m.batch_forward([7], [2], [2])
        assert got.argmax[0] == want.argmax[-1] and u32(got.lse)[0] == u32(want.lse)[-1]
        assert m.batch_generate([7], [2], [2], 4).shape == (4, 1)
        m.close()


def test_refusals():
    from llm_inference_amd._lib import LLMIError
    from llm_inference_amd.gguf import TensorType as TT
    from llm_inference_amd.model import Model, TPGroup
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    g = gguf("mini-1b")
    x = np.array([5, 6, 7], np.int32)
    with env():
        m = Model(build_gemma3_gguf(CONFIGS["tiny"], seed=7), exact=True, max_ctx=64)
        raises("E_ARG", "exact", m.reserve_sequences, 2)
        assert m.get_info().n_seq == 1 and m.forward(x, 0).shape == (m.vocab,)
        m.close()
        m = Model(build_gemma3_gguf(CONFIGS["mini-1b"], seed=21, embd_type=TT.Q8_0), max_ctx=64)
        raises("E_ARG", "F16 output table", m.reserve_sequences, 2)
        assert m.get_info().n_seq == 1 and m.score(x).count == 2
        m.close()
        # K-quant layers: their prefill hands the attention's outputs on as Q8_K blocks (or, LLMI_PREFILL_F16=1, falls
        # back to them for an overflowed row), which the multi-sequence attention does not write
        gk = build_gemma3_gguf(CONFIGS["mini-4b"], seed=21, wtype=TT.Q4_K, wtypes={"v": TT.Q6_K, "down": TT.Q6_K})
        for kv in ({}, {"LLMI_PREFILL_F16": 1}):
            with env(**kv):
                m = Model(gk, max_ctx=64)
                raises("E_ARG", "K-quant", m.reserve_sequences, 2)
                assert m.get_info().n_seq == 1 and m.score(x).count == 2
                m.close()
        # head_dim 64: the multi-sequence kernels are built for 128 and 256
        m = Model(build_gemma3_gguf(CONFIGS["tiny"], seed=7), max_ctx=64)
        raises("E_ARG", "head_dim", m.reserve_sequences, 2)
        assert m.get_info().n_seq == 1 and m.forward(x, 0).shape == (m.vocab,)
        m.close()
    with env(LLMI_NO_PREFILL=1):
        m = Model(g, max_ctx=64)
        raises("E_ARG", "LLMI_NO_PREFILL", m.reserve_sequences, 2)
        assert m.get_info().n_seq == 1 and m.score(x).count == 2
        m.close()
    with env():
        grp = TPGroup(2)
        got = [None, None]

        def rank(r):
            try:
                mr = Model(g, max_ctx=64, tp_rank=r, tp_size=2, tp_group=grp)
                try:
                    mr.reserve_sequences(2)
                except LLMIError as e:
                    got[r] = (e.status, str(e), mr.get_info().n_seq)
                mr.close()
            except Exception as e:  # noqa: BLE001 -- reported below
                got[r] = ("unexpected", repr(e), None)

        th = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join(300)
        grp.close()
    for st in got:
        assert st is not None and st[0] == "E_ARG" and "tensor-parallel" in st[1] and st[2] == 1, got


# ---------------------------------------------------------------------------
# 8. time_kernel(10)
# ---------------------------------------------------------------------------
def test_time_kernel_batch_attention():
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS
    cfg_name = "mini-4b"
    cfg = CONFIGS[cfg_name]
    c = contract_case(cfg_name)
    with env():
        m = Model(gguf(cfg_name), max_ctx=CTX)
        assert m.time_kernel(10, 2) == (0.0, 0.0)
        m.reserve_sequences(5)
        assert m.time_kernel(10, 2) == (0.0, 0.0)
        load_prefixes(m, c["prompts"], SLOTS)
        idx = list(range(5))
        m.batch_forward(*rows_of(c["prompts"], SLOTS, idx))
        us, by = m.time_kernel(10, 3)
        # the launch still leaves the step's outputs as they were: the rows again, same bits
        assert_rows(m.batch_forward(*rows_of(c["prompts"], SLOTS, idx), want_logits=True), c, idx, "after timing")
        m.close()
    # per layer: K and V rows 0 .. pos[b] of every row, f16
    want = sum(p + 1 for p in POS) * 2 * cfg.n_head_kv * cfg.head_dim * 2
    print(f"time_kernel(10): {us:.1f} us per layer for {by:.0f} bytes")
    assert us > 0.0 and by == float(want)
