"""Per-row seeded sampling inside the batched decode loop (llmi_session_batch_generate_sampled).

The contract needs no tolerance: a row that runs x[p] at position p of its slot emits exactly the sampling rule of
section 10.1 (tests/test_sampling.py ref_sample, imported, not restated) applied to forward(x[0..p], 0)'s logits on a
fresh single-sequence session, with pos = p and the row's own sampler -- whatever B, the other rows and their
samplers, the slot, the row order and the chunking of n_steps.  A row without a sampler is greedy: its ids are
batch_generate's.  The reference side is a Model that never reserves a slot.
"""
import dataclasses
import functools

import numpy as np
import pytest

from test_batch_decode import CTX, LOOP_LEN, LOOP_SLOTS, N_STEPS, env, load_prefixes, pick_stop, raises, read_kv, rows_of
from test_sampling import ref_sample

pytestmark = pytest.mark.gpu

# The synthetic models' logits are peaked, so the temperature is chosen by measuring the reference alone
# (reference_rows below, no batch call involved): entries of the 4 x 6 (row, step) table whose sampled id differs
# from the arg-max of the same logits, seed-13 models, the samplers below at base temperature T --
#   T                         8    16    24    32    48
#   mini-1b    (of 24)       12    21    23    23    23
#   mini-4b    (of 24)        1     9    15    18    22
#   vocab4100  (of 18)       10    17    17    17    17
#   softcap    (of 18)       13    17    17    17    17
# The tests require a quarter (6 of 24; the B = 3 variants 5 of 18).  16 passes it on mini-4b by 3 entries only;
# 24 leaves the arg-max in more than half of the entries on every model, so LOOP_T = 24.  At 24 the fork's two seeds
# differ in all 6 steps on both models and pick_stop finds a row (mini-1b row 0, mini-4b row 1).
LOOP_T = 24.0


def samplers_at(T):
    """One sampler per row: four seeds, four (temperature, top_k, top_p)."""
    return (dict(temperature=T, top_k=64, top_p=0.95, seed=101), dict(temperature=1.5 * T, top_k=0, top_p=1.0, seed=202),
            dict(temperature=T, top_k=40, top_p=0.9, seed=303), dict(temperature=1.5 * T, top_k=64, top_p=0.95, seed=404))


SAMPLERS = samplers_at(LOOP_T)
FORK_ROW, FORK_SEED, FORK_SLOT = 2, 909, 0  # the fork: row 2's prompt again in slot 0 with another seed


@functools.lru_cache(maxsize=None)
def gguf(name):
    """mini-1b / mini-4b as tests/test_sampling.py builds them (seed 13), and its two variants of mini-1b."""
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    if name == "vocab4100":
        return build_gemma3_gguf(dataclasses.replace(CONFIGS["mini-1b"], vocab=4100), seed=13)
    if name == "softcap":
        return build_gemma3_gguf(CONFIGS["mini-1b"], seed=13, extra_meta={"attention.final_logit_softcapping": 30.0})
    return build_gemma3_gguf(CONFIGS[name], seed=13)


def vocab_of(name):
    from llm_inference_amd.synthetic import CONFIGS
    return 4100 if name == "vocab4100" else CONFIGS["mini-1b" if name == "softcap" else name].vocab


def reference_rows(ref, prompts, samplers, steps):
    """Per row, iterate tok = ref_sample(forward(x, 0), sp, pos = len(x) - 1) and append (sampler None: the
    arg-max).  Returns ids [B][steps] and the arg-max of the same logits [B][steps]."""
    ids = np.zeros((len(prompts), steps), np.int32)
    amax = np.zeros((len(prompts), steps), np.int32)
    for b, (x0, sp) in enumerate(zip(prompts, samplers)):
        x = [int(t) for t in x0]
        for i in range(steps):
            lg = ref.forward(np.array(x, np.int32), 0)
            amax[b, i] = int(np.argmax(lg))
            ids[b, i] = amax[b, i] if sp is None else ref_sample(lg, sp["temperature"], sp["top_k"], sp["top_p"],
                                                                 sp["seed"], len(x) - 1)
            x.append(int(ids[b, i]))
    return ids, amax


@functools.lru_cache(maxsize=None)
def case(name, T=LOOP_T):
    """The prompts (lengths LOOP_LEN, or its first three for the B = 3 variants) and the reference's ids on a
    single-sequence session: sampled (with the arg-max of the same logits), the fork's second branch, and top_k = 1.
    Computed once per model, read-only."""
    from llm_inference_amd.model import Model
    n = 3 if name in ("vocab4100", "softcap") else 4
    rng = np.random.default_rng(500)
    prompts = [rng.integers(4, vocab_of(name), k).astype(np.int32) for k in LOOP_LEN[:n]]
    sps = samplers_at(T)[:n]
    with env():
        ref = Model(gguf(name), max_ctx=CTX)
        ids, amax = reference_rows(ref, prompts, sps, N_STEPS)
        out = dict(prompts=prompts, samplers=sps, ids=ids, amax=amax, off=int((ids != amax).sum()))
        if n == 4:
            fork_sp = dict(sps[FORK_ROW], seed=FORK_SEED)
            out["fork_sp"] = fork_sp
            out["fork_ids"] = reference_rows(ref, [prompts[FORK_ROW]], [fork_sp], N_STEPS)[0][0]
            k1 = [dict(sp, top_k=1) for sp in sps]
            out["k1_ids"], k1_amax = reference_rows(ref, prompts, k1, N_STEPS)
            assert (out["k1_ids"] == k1_amax).all()  # iterated argmax(forward(x))
        ref.close()
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def loaded(name, n_seq=5):
    from llm_inference_amd.model import Model
    c = case(name)
    m = Model(gguf(name), max_ctx=CTX)
    m.reserve_sequences(n_seq)
    load_prefixes(m, c["prompts"], LOOP_SLOTS)
    return m, c


def assert_inputs_leave_the_argmax(c, name):
    n = c["ids"].size
    print(f"{name}: {c['off']} of {n} reference ids leave the arg-max")
    assert 4 * c["off"] >= n, (name, c["off"], n)


# ---------------------------------------------------------------------------
# 1. rows equal the reference, whatever the batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mini-1b", "mini-4b"])
def test_sampled_rows_equal_reference(name):
    c = case(name)
    assert_inputs_leave_the_argmax(c, name)
    B = len(c["prompts"])
    with env():
        m, _ = loaded(name)
        out = m.batch_generate(*rows_of(c["prompts"], LOOP_SLOTS, range(B)), N_STEPS, samplers=list(c["samplers"]))
        m.close()
    assert out.shape == (N_STEPS, B) and out.dtype == np.int32
    np.testing.assert_array_equal(out, c["ids"].T)


@pytest.mark.parametrize("name", ["mini-1b", "mini-4b"])
def test_rows_independent_of_the_batch(name):
    """The same rows alone (B = 1), in reversed order, and inside B = 33 among unrelated rows with samplers of their
    own (two of them greedy)."""
    c = case(name)
    assert_inputs_leave_the_argmax(c, name)
    V = vocab_of(name)
    with env():
        m, _ = loaded(name)
        for b in range(4):
            out = m.batch_generate(*rows_of(c["prompts"], LOOP_SLOTS, [b]), N_STEPS, samplers=[c["samplers"][b]])
            np.testing.assert_array_equal(out[:, 0], c["ids"][b], err_msg=f"B = 1, row {b}")
        rev = [3, 2, 1, 0]
        out = m.batch_generate(*rows_of(c["prompts"], LOOP_SLOTS, rev), N_STEPS, samplers=[c["samplers"][b] for b in rev])
        np.testing.assert_array_equal(out, c["ids"][rev].T, err_msg="reversed")
        m.reserve_sequences(33)
        where = {0: 0, 8: 1, 9: 2, 32: 3}  # both sides of a block of 8 logits rows and of the 32-token MFMA tile
        rng = np.random.default_rng(6)
        tok, sl, ps, sps, spare = [], [], [], [], iter([0] + list(range(5, 33)))
        for b in range(33):
            if b in where:
                t, s, p = rows_of(c["prompts"], LOOP_SLOTS, [where[b]])
                tok, sl, ps = tok + t, sl + s, ps + p
                sps.append(c["samplers"][where[b]])
            else:
                tok.append(int(rng.integers(4, V)))
                sl.append(next(spare))
                ps.append(int(rng.integers(0, 200)))
                sps.append(None if b in (3, 20) else dict(temperature=float(rng.uniform(0.5, 40)),
                                                          top_k=int(rng.integers(0, 257)), seed=int(rng.integers(1 << 40))))
        out = m.batch_generate(tok, sl, ps, N_STEPS, samplers=sps)
        m.close()
    np.testing.assert_array_equal(out[:, list(where)], c["ids"].T, err_msg="inside B = 33")


@pytest.mark.parametrize("name", ["mini-1b", "mini-4b"])
def test_chunked_steps_continue_from_the_appended_rows(name):
    c = case(name)
    assert_inputs_leave_the_argmax(c, name)
    first, sl, ps = rows_of(c["prompts"], LOOP_SLOTS, range(4))
    with env():
        m, _ = loaded(name)
        a = m.batch_generate(first, sl, ps, 3, samplers=list(c["samplers"]))
        b = m.batch_generate(a[-1], sl, [p + 3 for p in ps], 3, samplers=list(c["samplers"]))
        m.close()
    np.testing.assert_array_equal(np.concatenate([a, b]), c["ids"].T)


@pytest.mark.parametrize("name", ["mini-1b", "mini-4b"])
def test_fork_with_two_seeds(name):
    c = case(name)
    assert (c["fork_ids"] != c["ids"][FORK_ROW]).any(), "the two seeds give the same ids on the reference"
    x = c["prompts"][FORK_ROW]
    p = len(x) - 1
    with env():
        m, _ = loaded(name)
        m.copy_sequence(FORK_SLOT, LOOP_SLOTS[FORK_ROW], p)
        out = m.batch_generate([int(x[-1])] * 2, [LOOP_SLOTS[FORK_ROW], FORK_SLOT], [p, p], N_STEPS,
                               samplers=[c["samplers"][FORK_ROW], c["fork_sp"]])
        m.close()
    np.testing.assert_array_equal(out[:, 0], c["ids"][FORK_ROW])
    np.testing.assert_array_equal(out[:, 1], c["fork_ids"])


# ---------------------------------------------------------------------------
# 2. greedy rows, top_k = 1
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mini-1b", "mini-4b"])
def test_mixed_and_all_greedy_rows(name):
    c = case(name)
    assert_inputs_leave_the_argmax(c, name)
    rows = rows_of(c["prompts"], LOOP_SLOTS, range(4))
    with env():
        m, _ = loaded(name)
        greedy = m.batch_generate(*rows, N_STEPS)
        mixed = m.batch_generate(*rows, N_STEPS, samplers=[None, c["samplers"][1], None, c["samplers"][3]])
        zero_t = m.batch_generate(*rows, N_STEPS, samplers=[dict(temperature=0.0), c["samplers"][1], None, None])
        all_greedy = m.batch_generate(*rows, N_STEPS, samplers=[None] * 4)
        m.close()
    np.testing.assert_array_equal(mixed[:, [0, 2]], greedy[:, [0, 2]])
    np.testing.assert_array_equal(mixed[:, [1, 3]], c["ids"][[1, 3]].T)
    np.testing.assert_array_equal(zero_t[:, [0, 2, 3]], greedy[:, [0, 2, 3]])  # temperature 0 is a greedy row
    np.testing.assert_array_equal(zero_t[:, 1], c["ids"][1])
    np.testing.assert_array_equal(all_greedy, greedy)


@pytest.mark.parametrize("name", ["mini-1b", "mini-4b"])
def test_top_k_1_is_iterated_argmax(name):
    c = case(name)
    with env():
        m, _ = loaded(name)
        out = m.batch_generate(*rows_of(c["prompts"], LOOP_SLOTS, range(4)), N_STEPS,
                               samplers=[dict(sp, top_k=1) for sp in c["samplers"]])
        m.close()
    np.testing.assert_array_equal(out, c["k1_ids"].T)


# ---------------------------------------------------------------------------
# 3. stop ids
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mini-1b", "mini-4b"])
def test_stop_ids(name):
    cfg_name = name
    c = case(name)
    assert_inputs_leave_the_argmax(c, name)
    ids = c["ids"]
    pick = pick_stop(ids)
    assert pick, ("no row first emits an id at step 2 which another row never emits", ids.tolist())
    r, stop = pick
    first, sl, ps = rows_of(c["prompts"], LOOP_SLOTS, range(4))
    with env():
        from llm_inference_amd.model import Model
        m = Model(gguf(name), max_ctx=CTX)
        m.reserve_sequences(6)
        # junk in the stopped row's slot first, so that "appends nothing" is visible: 200 rows of another sequence
        m.forward(np.random.default_rng(9).integers(4, vocab_of(name), 200).astype(np.int32), 0, want_logits=False)
        m.copy_sequence(LOOP_SLOTS[r], 0, 200)
        load_prefixes(m, c["prompts"], LOOP_SLOTS)
        kc0, vc0 = read_kv(m, LOOP_SLOTS[r], cfg_name)
        out = m.batch_generate(first, sl, ps, N_STEPS, stop=[stop], samplers=list(c["samplers"]))
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
# 4. a ragged vocabulary, a final soft-cap
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vocab4100", "softcap"])
def test_ragged_vocab_and_final_softcap(name):
    """B = 3 on mini-1b with a 4100-row vocabulary (two select work-groups per row, the second ragged) and with
    attention.final_logit_softcapping 30 (the soft-cap launch over the B x V block), against the reference."""
    c = case(name)
    assert_inputs_leave_the_argmax(c, name)
    with env():
        m, _ = loaded(name)
        out = m.batch_generate(*rows_of(c["prompts"], LOOP_SLOTS, range(3)), N_STEPS, samplers=list(c["samplers"]))
        m.close()
    np.testing.assert_array_equal(out, c["ids"].T)


# ---------------------------------------------------------------------------
# 5. errors, time_kernel(11)
# ---------------------------------------------------------------------------
def test_errors():
    from llm_inference_amd._lib import LLMIError, check, lib, ptr
    from llm_inference_amd.model import Model
    name = "mini-1b"
    V = vocab_of(name)
    sp = dict(temperature=1.0, top_k=64, top_p=0.95, seed=1)
    with env():
        m = Model(gguf(name), max_ctx=64)
        raises("E_ARG", "seq_reserve", m.batch_generate, [5], [0], [0], 2, samplers=sp)
        m.reserve_sequences(4)
        # a null samplers pointer
        one = np.array([5], np.int32)
        zero = np.zeros(1, np.int32)
        out = np.zeros(2, np.int32)
        with pytest.raises(LLMIError) as ei:
            check(lib().llmi_session_batch_generate_sampled(m.h, ptr(one), ptr(zero), ptr(zero), 1, 2, None, 0, None,
                                                            ptr(out)))
        assert ei.value.status == "E_ARG" and "samplers" in str(ei.value)
        # bad fields: the message names the field and the row
        for kw, field in [(dict(temperature=-0.5), "temperature"), (dict(temperature=float("nan")), "temperature"),
                          (dict(temperature=1.0, top_k=-3), "top_k"), (dict(temperature=1.0, top_k=300), "top_k"),
                          (dict(temperature=1.0, top_p=0.0), "top_p"), (dict(temperature=1.0, top_p=1.01), "top_p"),
                          (dict(temperature=1.0, top_p=float("nan")), "top_p")]:
            with pytest.raises(LLMIError) as ei:
                m.batch_generate([5, 6, 7], [0, 1, 2], [0, 0, 0], 2, samplers=[sp, None, kw])
            assert ei.value.status == "E_ARG" and field in str(ei.value) and "samplers[2]" in str(ei.value), str(ei.value)
        # every refusal of batch_generate
        raises("E_RANGE", "slots", m.batch_generate, [5, 6], [0, 4], [0, 0], 2, samplers=sp)
        raises("E_ARG", "slots", m.batch_generate, [5, 6], [2, 2], [0, 0], 2, samplers=sp)
        raises("E_RANGE", "(B)", m.batch_generate, [5] * 5, [0, 1, 2, 3, 0], [0] * 5, 2, samplers=sp)
        raises("E_RANGE", "tokens", m.batch_generate, [-1], [0], [0], 2, samplers=sp)
        raises("E_RANGE", "tokens", m.batch_generate, [V], [0], [0], 2, samplers=sp)
        raises("E_RANGE", "pos + n_steps", m.batch_generate, [5], [0], [60], 5, samplers=sp)
        raises("E_RANGE", "pos + n_steps", m.batch_generate, [5], [0], [-1], 2, samplers=sp)
        raises("E_ARG", "n_stop", m.batch_generate, [5], [0], [0], 2, stop=[1, 2, 3, 4, 5], samplers=sp)
        raises("E_RANGE", "stop", m.batch_generate, [5], [0], [0], 2, stop=[V], samplers=sp)
        # the session still works, and the session's own sampler was never touched
        assert m.batch_generate([7], [2], [0], 4, samplers=sp).shape == (4, 1)
        assert m.batch_generate([7], [2], [0], 0, samplers=sp).shape == (0, 1)
        assert m.get_info().sampling == 0
        m.close()
    with env(LLMI_NO_PREFILL=1):
        m = Model(gguf(name), max_ctx=64)
        raises("E_ARG", "LLMI_NO_PREFILL", m.reserve_sequences, 2)
        raises("E_ARG", "seq_reserve", m.batch_generate, [5], [0], [0], 2, samplers=sp)
        m.close()


def test_time_kernel_batch_sampling():
    from llm_inference_amd import ops
    from llm_inference_amd.synthetic import CONFIGS
    name = "mini-4b"
    cfg = CONFIGS[name]
    c = case(name)
    rows = rows_of(c["prompts"], LOOP_SLOTS, range(4))
    with env():
        m, _ = loaded(name, n_seq=12)
        assert m.time_kernel(11, 2) == (0.0, 0.0)
        m.batch_generate(*rows, 2)  # a greedy batch step is not a sampled one
        assert m.time_kernel(11, 2) == (0.0, 0.0)
        out = m.batch_generate(*rows, N_STEPS, samplers=list(c["samplers"]))
        us, by = m.time_kernel(11, 3)
        # the launches feed nothing back: the same call again gives the same ids
        again = m.batch_generate(*rows, N_STEPS, samplers=list(c["samplers"]))
        # B = 9 on slots of their own: two reads of the table at this width
        m.batch_generate([5] * 9, [0] + list(range(5, 12)) + [4], [0] * 9, 1, samplers=c["samplers"][0])
        us9, by9 = m.time_kernel(11, 2)
        m.close()
    np.testing.assert_array_equal(out, c["ids"].T)
    np.testing.assert_array_equal(again, out)
    rb = ops.logits_rows_rb(cfg.n_embd)
    table = cfg.vocab * cfg.n_embd * 2
    print(f"time_kernel(11): {us:.1f} us for {by:.0f} bytes (B = 4), {us9:.1f} us for {by9:.0f} bytes (B = 9), RB = {rb}")
    assert rb == 8
    assert us > 0.0 and by == float(table + 4 * cfg.vocab * 4)
    assert us9 > 0.0 and by9 == float(2 * table + 9 * cfg.vocab * 4)
