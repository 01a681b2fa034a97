"""Lookup decoding (llmi_session_batch_generate_lookup / llmi_lookup_draft): n-gram drafts
verified inside the device batch loop.

The contract needs no tolerance: under section 12's row contract on the slots' K/V, ids[b] equals row b's ids of
batch_generate(first = hist[b][-1], slots, pos, max_new, stop) on the same state, up to and including the row's stop
id -- whatever the histories, draft_len, the n-gram bounds, B, the other rows, the row order and LLMI_LOOKUP_SYNC.
The reference ids come from batch_generate on a Model that never calls the new code; steps / drafted / accepted are
compared with the host simulation of the rule (tests/test_batch_lookup_host.py) driven by those reference ids.

Every case asserts that the f16-redo counter did not move.  Every step here has B (draft_len + 1) <= 128 token rows,
below mini-4b's GEMM switch (384 rows; mini-1b has none), and mini-27b runs with LLMI_PG6=1 on both sides, as
tests/test_batch_extend.py does and explains: one prefill GEMM for every row count.
"""
import contextlib
import functools
import os

import numpy as np
import pytest
from test_batch_decode import CHAIN, chain_gguf, gguf, raises, read_kv, vocab_of
from test_batch_lookup_host import ref_lookup_draft, simulate

pytestmark = pytest.mark.gpu
CTX = 512
ENV_KEYS = ("LLMI_NO_PREFILL", "LLMI_PREFILL_CHUNK", "LLMI_PREFILL_FULL_LAST", "LLMI_PREFILL_ATTN_KS",
            "LLMI_PREFILL_ATTN_V1", "LLMI_PREFILL_F16", "LLMI_BATCH_SPAN_ROWS", "LLMI_PG6", "LLMI_PG7", "LLMI_LOOKUP_SYNC")
MODEL_ENV = {"mini-27b": {"LLMI_PG6": 1}}
SLOTS = (2, 4, 1, 3)  # (slot 0 stays free: read_kv uses it)
T0, T1, T2, T3 = CHAIN


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


def rand_tokens(rng, V, n):
    """n distinct-ish random ids outside CHAIN."""
    x = rng.integers(4, V, n).astype(np.int32)
    x[np.isin(x, CHAIN)] = 104
    return x


@functools.lru_cache(maxsize=None)
def chain_rows(cfg_name):
    """Four prompts on the chain model (t0 -> t1 -> t2 -> t3 -> t3; any other token repeats itself):
    A  ... t0 t1 t2 x y ... t0      the draft after t0 is t1 t2 x: two right, the third wrong
    B  ... q z ... q                the only match proposes z, but q repeats: none right
    C  random                       no match in step 1, then its own repeats
    S  ... t0 t1 t2 t3 t3 t3 w ... t0   the draft is right five tokens deep (the stop-id case cuts it at t3)"""
    V = vocab_of(cfg_name)
    rng = np.random.default_rng(21)
    r = lambda n: rand_tokens(rng, V, n)  # noqa: E731
    x, y, q, z, w = (int(v) for v in rng.choice(np.arange(200, V), 5, replace=False))
    cat = lambda *p: np.concatenate([np.atleast_1d(np.asarray(a, np.int32)) for a in p])  # noqa: E731
    a = cat(r(20), [T0, T1, T2, x, y], r(6), [T0])
    b = cat(r(40), [q, z], r(25), [q])
    c = r(131)
    s = cat(r(10), [T0, T1, T2, T3, T3, T3, w], r(5), [T0])
    for p in (a, b, c, s):  # the planted tokens appear only where planted
        p.setflags(write=False)
    assert (a == T0).sum() == 2 and (b == q).sum() == 2 and (s == T0).sum() == 2 and x != T3 and z != q
    return [a, b, c, s]


@functools.lru_cache(maxsize=None)
def random_rows(cfg_name, lens=(6, 34, 70, 131)):
    """Random prompts whose last token occurs nowhere before it: the first step has no draft."""
    rng = np.random.default_rng(121)
    rows = [rand_tokens(rng, vocab_of(cfg_name), n) for n in lens]
    for x in rows:
        x[-1] = min(set(range(200, 200 + len(x) + 1)) - set(x[:-1].tolist()))
    return rows


def preload(m, prompts, slots, junk=None):
    """x[:-1] of every prompt into its slot, in batch_extend calls of at most 256 token rows (below the GEMM switch).
    junk: a slot that first receives 200 rows of another sequence, as test_batch_decode.test_stop_ids does."""
    if junk is not None:
        m.forward(np.random.default_rng(9).integers(4, m.vocab, 200).astype(np.int32), 0, want_logits=False)
        m.copy_sequence(junk, 0, 200)
    call, rows = [], 0
    todo = [(x[:-1], s, 0) for x, s in zip(prompts, slots)]
    while todo:
        x, s, p = todo.pop(0)
        n = min(len(x), 256 - rows)
        if n < len(x):
            todo.insert(0, (x[n:], s, p + n))
        if n:
            call.append((x[:n], s, p))
            rows += n
        if call and (rows == 256 or not todo):
            # (a slot at most once per call: a prompt cut in two goes into two calls)
            m.batch_extend([c[0] for c in call], [c[1] for c in call], [c[2] for c in call], out="none")
            call, rows = [], 0


def cut(col, stop):
    """A batch_generate column as the ids the row emitted: up to and including its stop id."""
    ids = []
    for t in col.tolist():
        if t < 0:
            break
        ids.append(t)
        if t in stop:
            break
    return ids


_REF = {}


def reference(cfg_name, key, prompts, max_new, stop=(), kv=None, chain=True, want_kv=None):
    """Row ids of batch_generate on a Model that never runs the new code, computed once per case and shared; want_kv: a
    row whose slot's K/V caches are returned as well."""
    from llm_inference_amd.model import Model
    k = (cfg_name, key, max_new, tuple(stop), tuple(sorted((kv or {}).items())), chain, want_kv)
    if k not in _REF:
        with env(**dict(MODEL_ENV.get(cfg_name, {}), **(kv or {}))):
            ref = Model((chain_gguf if chain else gguf)(cfg_name), max_ctx=CTX)
            ref.reserve_sequences(5)
            preload(ref, prompts, SLOTS)
            out = ref.batch_generate([int(x[-1]) for x in prompts], SLOTS[:len(prompts)],
                                     [len(x) - 1 for x in prompts], max_new, stop=list(stop))
            assert ref.get_info().prefill_f16_redo == 0
            kvs = read_kv(ref, SLOTS[want_kv], cfg_name) if want_kv is not None else None
            ref.close()
        _REF[k] = ([cut(out[:, b], stop) for b in range(len(prompts))], kvs)
    return _REF[k]


def greedy_from(ids):
    """simulate()'s greedy(prefix) from a row's reference ids: the id after the row has run [cur] + ids[:n]; -1 for a
    prefix that left the greedy path or runs past the row's end (the rule emits none of those: it stops at the first
    wrong draft, cuts after the stop id and drafts at most remaining - 1 tokens)."""
    def greedy(p):
        n = len(p) - 1
        return ids[n] if n < len(ids) and list(p[1:]) == list(ids[:n]) else -1
    return greedy


def expect(hist, ids, max_new, D, N=3, nmin=1, stop=(), max_steps=0, trace=None):
    """The loop simulated on the host, the model replaced by the reference ids."""
    sim = simulate(hist, greedy_from(list(ids)), max_new, D, N, nmin, stop, max_steps, trace)
    assert -1 not in sim[0]
    return sim


def run(m, hists, slots, pos, max_new, **kw):
    r = m.batch_generate_lookup(hists, slots, pos, max_new, **kw)
    assert m.get_info().prefill_f16_redo == 0, "the f16 path overflowed: the bits compared would be the int8 path's"
    assert len(r.ids) == len(hists) and all(x.dtype == np.int32 for x in r.ids)
    return r


def assert_rows(r, hists, ref_ids, max_new, D, what, idx=None, **kw):
    """ids equal the reference's and steps / drafted / accepted the simulation's, for the rows idx of the call."""
    idx = range(len(hists)) if idx is None else idx
    steps = 0
    for k, b in enumerate(idx):
        sim = expect(hists[k], ref_ids[k], max_new, D, **kw)
        assert r.ids[b].tolist() == sim[0], (what, k, r.ids[b].tolist(), sim[0])
        if not kw.get("max_steps"):
            assert sim[0] == ref_ids[k], (what, k)
        assert (int(r.drafted[b]), int(r.accepted[b])) == sim[2:], (what, k, r.drafted[b], r.accepted[b], sim)
        steps = max(steps, sim[1])
    return steps


# ---------------------------------------------------------------------------
# 1. op level: the draft rule by the kernel
# ---------------------------------------------------------------------------
def test_lookup_draft_equals_the_rule():
    from llm_inference_amd import ops
    rng = np.random.default_rng(21)
    cases = []
    for L in (1, 2, 33, 257, 512):  # across one wave, one work-group pass and two
        cases.append((rng.integers(0, 3, L), 3, 1, 7))
        cases.append((rng.integers(0, 50, L), 8, 1, 31))
        cases.append((np.arange(L), 3, 1, 7))                      # no match
    cases += [
        ([4, 9, 5, 6, 9], 3, 1, 4),                                # a match only at n = 1
        ([1, 2, 9, 8, 2, 7, 1, 2], 3, 1, 2),                       # longer and older against shorter and newer
        ([1, 2, 9, 8, 2, 7, 1, 2], 1, 1, 2),
        ([5, 5], 3, 1, 9),                                         # the continuation wraps: period 1
        ([7, 1, 2, 3, 1, 2, 3, 1], 3, 1, 11),                      # ... and period 3
        ([4, 9, 5, 6, 9], 3, 2, 4),                                # ngram_min = 2 rejects the n = 1 match
        ([4, 9, 5, 6, 4, 9], 3, 2, 4),
        ([4, 9, 5, 6, 9], 3, 1, 1), ([4, 9, 5, 6, 9], 3, 1, 31),   # draft_len 1 and 31
        (np.tile([3, 1, 4, 1, 5, 9, 2, 6], 40), 8, 8, 31),         # n = 8 on a long periodic history
    ]
    n_match = 0
    for h, N, nmin, D in cases:
        want = ref_lookup_draft(h, N, nmin, D)
        d, e, ml = ops.lookup_draft(h, N, nmin, D)
        assert (d.tolist(), e, ml) == want, (list(h)[:16], len(h), N, nmin, D)
        n_match += bool(want[0])
    assert n_match >= 12
    raises("E_RANGE", "(draft_len)", ops.lookup_draft, [1, 2], 3, 1, 32)
    raises("E_RANGE", "(draft_len)", ops.lookup_draft, [1, 2], 3, 1, 0)
    raises("E_RANGE", "(ngram_max)", ops.lookup_draft, [1, 2], 9, 1, 4)
    raises("E_RANGE", "(ngram_min)", ops.lookup_draft, [1, 2], 3, 4, 4)
    raises("E_RANGE", "(ngram_min)", ops.lookup_draft, [1, 2], 3, 0, 4)
    raises("E_ARG", "(hist)", ops.lookup_draft, [], 3, 1, 4)


# ---------------------------------------------------------------------------
# 2. full acceptance: the random model repeats its input
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_full_acceptance(cfg_name):
    from llm_inference_amd.model import Model
    prompts = random_rows(cfg_name)
    pos = [len(x) - 1 for x in prompts]
    max_new, D = 20, 7
    ref_ids, _ = reference(cfg_name, "random", prompts, max_new, chain=False)
    for b, x in enumerate(prompts):  # the simulation shows every draft accepted after the first step
        tr = []
        sim = expect(x, ref_ids[b], max_new, D, trace=tr)
        assert tr[0][0] == [] and all(len(out) == len(d) + 1 and d for d, out in tr[1:]) and sim[2] == sim[3] > 0
    with env():
        m = Model(gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(5)
        preload(m, prompts, SLOTS)
        r = run(m, prompts, SLOTS, pos, max_new, draft_len=D)
        m.close()
    steps = assert_rows(r, prompts, ref_ids, max_new, D, cfg_name)
    assert r.steps == steps == 4 and all(len(x) == max_new for x in r.ids)


# ---------------------------------------------------------------------------
# 3. rejection and partial acceptance, and what the slot holds afterwards
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_rejection_and_partial_acceptance(cfg_name):
    from llm_inference_amd.model import Model
    prompts = chain_rows(cfg_name)
    pos = [len(x) - 1 for x in prompts]
    max_new, D = 9, 3
    ref_ids, (kcr, vcr) = reference(cfg_name, "chain", prompts, max_new, want_kv=0)
    # row A: the draft after t0 is t1 t2 x and the greedy ids are t1 t2 t3 -- 2 of 3 accepted
    tr = []
    expect(prompts[0], ref_ids[0], max_new, D, trace=tr)
    assert ref_ids[0][:4] == [T1, T2, T3, T3] and tr[0][0][:2] == [T1, T2] and tr[0][0][2] != T3
    assert tr[0][1] == [T1, T2, T3]
    # row B: its only match proposes a wrong first token -- 0 accepted
    tr = []
    expect(prompts[1], ref_ids[1], max_new, D, trace=tr)
    assert len(tr[0][0]) == D and tr[0][0][0] != ref_ids[1][0] and len(tr[0][1]) == 1
    with env():
        m = Model(chain_gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(5)
        preload(m, prompts, SLOTS, junk=SLOTS[0])
        kc0, vc0 = read_kv(m, SLOTS[0], cfg_name)
        r = run(m, prompts, SLOTS, pos, max_new, draft_len=D)
        kc1, vc1 = read_kv(m, SLOTS[0], cfg_name)
        m.close()
    assert_rows(r, prompts, ref_ids, max_new, D, cfg_name)
    assert 0 < r.accepted[0] < r.drafted[0] and r.accepted[1] < r.drafted[1]
    # row A's slot: rows pos .. pos + n_out - 1 carry batch_generate's bits; rows at and past pos + max_new are the junk
    lo, hi = pos[0], pos[0] + len(r.ids[0])
    assert len(r.ids[0]) == max_new
    np.testing.assert_array_equal(kc1[:, :, lo:hi], kcr[:, :, lo:hi])
    np.testing.assert_array_equal(vc1[:, :, lo:hi], vcr[:, :, lo:hi])
    np.testing.assert_array_equal(kc1[:, :, pos[0] + max_new:], kc0[:, :, pos[0] + max_new:])
    np.testing.assert_array_equal(vc1[:, :, pos[0] + max_new:], vc0[:, :, pos[0] + max_new:])
    assert (kc1[:, :, lo:hi] != kc0[:, :, lo:hi]).any()


# ---------------------------------------------------------------------------
# 4. independence
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_rows_independent_of_the_call(cfg_name):
    """The same rows alone, reversed, inside B = 16 among unrelated rows (16 x 8 = 128 token rows), with draft_len 1,
    4 and 31 (4 x 32 = 128 token rows), LLMI_LOOKUP_SYNC 1 and 64, and with a garbage history."""
    from llm_inference_amd.model import Model
    prompts = chain_rows(cfg_name)
    pos = [len(x) - 1 for x in prompts]
    max_new = 12
    ref_ids, _ = reference(cfg_name, "chain", prompts, max_new)
    V = vocab_of(cfg_name)
    rng = np.random.default_rng(5)
    with env():
        m = Model(chain_gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(17)
        preload(m, prompts, SLOTS)
        for b in range(4):
            r = run(m, [prompts[b]], [SLOTS[b]], [pos[b]], max_new, draft_len=7)
            assert_rows(r, [prompts[b]], [ref_ids[b]], max_new, 7, f"alone, row {b}")
        rev = [3, 2, 1, 0]
        r = run(m, [prompts[b] for b in rev], [SLOTS[b] for b in rev], [pos[b] for b in rev], max_new, draft_len=7)
        assert_rows(r, [prompts[b] for b in rev], [ref_ids[b] for b in rev], max_new, 7, "reversed")
        for D in (1, 4, 31):
            r = run(m, prompts, SLOTS, pos, max_new, draft_len=D)
            assert_rows(r, prompts, ref_ids, max_new, D, f"draft_len {D}")
        for N, nmin in ((8, 1), (2, 2)):
            r = run(m, prompts, SLOTS, pos, max_new, draft_len=7, ngram_max=N, ngram_min=nmin)
            assert_rows(r, prompts, ref_ids, max_new, 7, f"n-gram {nmin}..{N}", N=N, nmin=nmin)
        for sync in (1, 64):
            with env(LLMI_LOOKUP_SYNC=sync):
                r = run(m, prompts, SLOTS, pos, max_new, draft_len=7)
            steps = assert_rows(r, prompts, ref_ids, max_new, 7, f"LLMI_LOOKUP_SYNC {sync}")
            assert r.steps == steps
        # a garbage history with the right last token: the same ids, fewer drafts accepted
        good = run(m, prompts, SLOTS, pos, max_new, draft_len=7)
        junk = [np.concatenate([rand_tokens(rng, V, 30), x[-1:]]) for x in prompts]
        r = run(m, junk, SLOTS, pos, max_new, draft_len=7)
        assert_rows(r, junk, ref_ids, max_new, 7, "garbage history")
        assert r.accepted.sum() < good.accepted.sum() and r.steps > good.steps
        # B = 16: the four rows at 0, 5, 10, 15, unrelated rows on slots 5..16 around them
        where = {0: 0, 5: 1, 10: 2, 15: 3}
        others = [rand_tokens(rng, V, int(n)) for n in rng.integers(3, 20, 12)]
        spare = list(range(5, 17))
        preload(m, others, spare)
        hs, sl, ps = [], [], []
        for b in range(16):
            if b in where:
                k = where[b]
                hs.append(prompts[k]), sl.append(SLOTS[k]), ps.append(pos[k])
            else:
                x = others.pop()
                hs.append(x), sl.append(spare.pop()), ps.append(len(x) - 1)
        r = run(m, hs, sl, ps, max_new, draft_len=7)
        assert_rows(r, prompts, ref_ids, max_new, 7, "inside B = 16", idx=list(where))
        m.close()


@pytest.mark.parametrize("ks", [1, 8])
def test_rows_under_other_key_splits(ks):
    from llm_inference_amd.model import Model
    cfg_name = "mini-4b"
    prompts = chain_rows(cfg_name)
    pos = [len(x) - 1 for x in prompts]
    max_new = 12
    kv = {"LLMI_PREFILL_ATTN_KS": ks}
    ref_ids, _ = reference(cfg_name, "chain", prompts, max_new, kv=kv)
    with env(**kv):
        m = Model(chain_gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(5)
        preload(m, prompts, SLOTS)
        r = run(m, prompts, SLOTS, pos, max_new, draft_len=7)
        m.close()
    assert_rows(r, prompts, ref_ids, max_new, 7, f"ks = {ks}")


# ---------------------------------------------------------------------------
# 5. stop ids
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_stop_id_inside_an_accepted_draft(cfg_name):
    from llm_inference_amd.model import Model
    prompts = chain_rows(cfg_name)
    pos = [len(x) - 1 for x in prompts]
    max_new, D, stop = 12, 7, (T3,)
    free, _ = reference(cfg_name, "chain", prompts, max_new)
    ref_ids, _ = reference(cfg_name, "chain", prompts, max_new, stop=stop)
    # row S: without the stop id its first step accepts t1 t2 t3 t3 t3 -- the stop id lands inside that draft
    tr = []
    expect(prompts[3], free[3], max_new, D, trace=tr)
    assert tr[0][1][:5] == [T1, T2, T3, T3, T3] and len(tr[0][1]) >= 5
    assert ref_ids[3] == [T1, T2, T3] and ref_ids[0] == [T1, T2, T3]
    assert len(ref_ids[1]) == len(ref_ids[2]) == max_new, "the other rows run on"
    with env():
        m = Model(chain_gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(5)
        preload(m, prompts, SLOTS)
        r = run(m, prompts, SLOTS, pos, max_new, draft_len=D, stop=stop)
        # the raw call: n_out and the -1 fill
        from llm_inference_amd._lib import Lookup, check, lib, ptr
        from llm_inference_amd.model import marshal_lookup
        tok, hl, sl, p = marshal_lookup(prompts, SLOTS, pos)
        out, n_out = np.zeros((4, max_new), np.int32), np.zeros(4, np.int32)
        st = np.array(stop, np.int32)
        import ctypes as C
        lk = Lookup(D, 3, 1, max_new)
        check(lib().llmi_session_batch_generate_lookup(m.h, ptr(tok), ptr(hl), ptr(sl), ptr(p), 4, C.byref(lk), 0, ptr(st),
                                                       1, ptr(out), ptr(n_out), None))
        m.close()
    assert_rows(r, prompts, ref_ids, max_new, D, cfg_name, stop=stop)
    assert n_out.tolist() == [3, max_new, max_new, 3]
    for b in range(4):
        assert out[b, :n_out[b]].tolist() == ref_ids[b] and (out[b, n_out[b]:] == -1).all()


# ---------------------------------------------------------------------------
# 6. the budget
# ---------------------------------------------------------------------------
def test_budget():
    from llm_inference_amd.model import Model
    cfg_name = "mini-4b"
    # row 0 ends at max_ctx exactly: pos + max_new == CTX
    max_new, D = 12, 7
    prompts = random_rows(cfg_name, lens=(CTX - max_new + 1, 34, 70))
    pos = [len(x) - 1 for x in prompts]
    assert pos[0] + max_new == CTX
    ref_ids, _ = reference(cfg_name, "budget", prompts, max_new, chain=False)
    with env():
        m = Model(gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(5)
        preload(m, prompts, SLOTS)
        # max_new ends inside a draft: 1 + 8 ids, then a draft cut to the 3 ids left
        r = run(m, prompts, SLOTS[:3], pos, max_new, draft_len=D)
        steps = assert_rows(r, prompts, ref_ids, max_new, D, "max_new inside a draft")
        assert r.steps == steps == 3 and all(len(x) == max_new for x in r.ids)
        assert r.drafted.tolist() == [9, 9, 9] and r.accepted.tolist() == [9, 9, 9]
        # max_steps before max_new: short, and a prefix of the reference
        r = run(m, prompts, SLOTS[:3], pos, max_new, draft_len=D, max_steps=2)
        assert_rows(r, prompts, ref_ids, max_new, D, "max_steps = 2", max_steps=2)
        assert r.steps == 2
        for b in range(3):
            assert len(r.ids[b]) == 9 and r.ids[b].tolist() == ref_ids[b][:9]
        r = run(m, prompts, SLOTS[:3], pos, 1, draft_len=D)  # max_new = 1: no draft at all
        assert [x.tolist() for x in r.ids] == [ids[:1] for ids in ref_ids] and r.drafted.sum() == 0 and r.steps == 1
        m.close()


# ---------------------------------------------------------------------------
# 7. head_dim 128
# ---------------------------------------------------------------------------
def test_mini_27b():
    from llm_inference_amd.model import Model
    cfg_name = "mini-27b"
    prompts = chain_rows(cfg_name)
    pos = [len(x) - 1 for x in prompts]
    max_new, D = 9, 7
    ref_ids, _ = reference(cfg_name, "chain", prompts, max_new)
    assert ref_ids[0][:4] == [T1, T2, T3, T3]
    with env(**MODEL_ENV[cfg_name]):
        m = Model(chain_gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(5)
        preload(m, prompts, SLOTS)
        r = run(m, prompts, SLOTS, pos, max_new, draft_len=D)
        m.close()
    assert_rows(r, prompts, ref_ids, max_new, D, cfg_name)
    assert 0 < r.accepted[0] < r.drafted[0]


# ---------------------------------------------------------------------------
# 8. errors
# ---------------------------------------------------------------------------
def test_argument_errors():
    from llm_inference_amd.model import Model
    cfg_name = "mini-1b"
    V = vocab_of(cfg_name)
    h = [5, 6, 7]
    with env():
        m = Model(gguf(cfg_name), max_ctx=64)
        f = m.batch_generate_lookup
        raises("E_ARG", "seq_reserve", f, [h], [0], [2], 4)
        m.reserve_sequences(4)
        raises("E_RANGE", "(B)", f, [h] * 5, [0, 1, 2, 3, 0], [2] * 5, 4)
        raises("E_RANGE", "(slots)", f, [h, h], [0, 4], [2, 2], 4)
        raises("E_RANGE", "(slots)", f, [h, h], [0, -1], [2, 2], 4)
        raises("E_ARG", "(slots)", f, [h, h], [2, 2], [2, 2], 4)
        raises("E_ARG", "(n_stop)", f, [h], [0], [2], 4, stop=[1, 2, 3, 4, 5])
        raises("E_RANGE", "(stop)", f, [h], [0], [2], 4, stop=[V])
        raises("E_RANGE", "(draft_len)", f, [h], [0], [2], 4, draft_len=0)
        raises("E_RANGE", "(draft_len)", f, [h], [0], [2], 4, draft_len=32)
        raises("E_RANGE", "(ngram_max)", f, [h], [0], [2], 4, ngram_max=9)
        raises("E_RANGE", "(ngram_max)", f, [h], [0], [2], 4, ngram_max=0)
        raises("E_RANGE", "(ngram_min)", f, [h], [0], [2], 4, ngram_min=0)
        raises("E_RANGE", "(ngram_min)", f, [h], [0], [2], 4, ngram_max=2, ngram_min=3)
        raises("E_RANGE", "(max_new)", f, [h], [0], [2], 0)
        m.reserve_sequences(17)
        raises("E_RANGE", "(B * (draft_len + 1))", f, [h] * 17, list(range(17)), [2] * 17, 4, draft_len=31)
        raises("E_RANGE", "(hist_len)", f, [h, []], [0, 1], [2, 2], 4)
        raises("E_RANGE", "(hist)", f, [[5, V]], [0], [2], 4)
        raises("E_RANGE", "(hist)", f, [[-1, 5]], [0], [2], 4)
        raises("E_RANGE", "(pos)", f, [h], [0], [0], 4)
        raises("E_RANGE", "position 0", f, [h], [0], [0], 4)
        raises("E_RANGE", "(pos)", f, [h], [0], [-3], 4)
        raises("E_RANGE", "(pos + max_new)", f, [h], [0], [61], 4)
        raises("E_ARG", "(max_steps)", f, [h], [0], [2], 4, max_steps=-1)
        # the session still works: the same ids as batch_generate
        x = np.array([5, 6, 7], np.int32)
        m.forward(x[:2], 0, want_logits=False)
        m.copy_sequence(2, 0, 2)
        want = m.batch_generate([7], [2], [2], 4)[:, 0]
        got = f([x], [2], [2], 4)
        assert got.ids[0].tolist() == want.tolist() and m.get_info().prefill_f16_redo == 0
        m.close()


# ---------------------------------------------------------------------------
# 9. time_kernel(13)
# ---------------------------------------------------------------------------
def test_time_kernel_lookup_step():
    from llm_inference_amd.model import Model
    cfg_name = "mini-4b"
    prompts = random_rows(cfg_name)
    pos = [len(x) - 1 for x in prompts]
    max_new = 12
    ref_ids, _ = reference(cfg_name, "random12", prompts, max_new, chain=False)
    with env():
        m = Model(gguf(cfg_name), max_ctx=CTX)
        assert m.time_kernel(13, 2) == (0.0, 0.0)
        m.reserve_sequences(5)
        assert m.time_kernel(13, 2) == (0.0, 0.0)
        preload(m, prompts, SLOTS)
        r = run(m, prompts, SLOTS, pos, max_new)
        us, by = m.time_kernel(13, 3)
        # the launch changes no state: the call again gives the same result
        r2 = run(m, prompts, SLOTS, pos, max_new)
        m.close()
    assert_rows(r, prompts, ref_ids, max_new, 7, "before timing")
    assert [x.tolist() for x in r2.ids] == [x.tolist() for x in r.ids] and r2.steps == r.steps
    # the history tokens read: every row's history as the call left it, 4 bytes each
    want = 4 * sum(len(x) + len(ids) for x, ids in zip(prompts, r.ids))
    print(f"time_kernel(13): {us:.1f} us for {by:.0f} bytes")
    assert us > 0.0 and by == float(want)
