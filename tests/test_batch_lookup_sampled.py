"""Lookup decoding for sampled rows (llmi_session_batch_generate_lookup_sampled): a draft token
is accepted when it equals the row's seeded draw at that token's own position.

The contract needs no tolerance: under section 12's row contract on the slots' K/V, ids[b] equals row b's ids of
batch_generate(first = hist[b][-1], slots, pos, max_new, stop, samplers=samplers) on the same state, up to and
including the row's stop id -- whatever the histories, draft_len, the n-gram bounds, B, the other rows and their
samplers, the row order, LLMI_LOOKUP_SYNC and LLMI_LOOKUP_NO_GATHER.  The reference ids come from batch_generate on a
Model that never calls the new code; steps / drafted / accepted are compared with the host simulation of the rule
(tests/test_batch_lookup_host.py) driven by those reference ids.

The model never reads the history, so the tests steer acceptance through the history alone: the reference ids
r[0..n) are computed first, then histories are built whose most recent match of the current suffix continues with
r[0] r[1] ... (full acceptance), r[0] r[1] x (two of three), y != r[0] (none), or which have no match at all (empty
drafts: every live token row is a row's current token).

The sampled reference must not be the greedy sequence in disguise.  Entries of the 4 x 12 (row, step) table whose
sampled id differs from the arg-max of the same logits / the fewest distinct ids of a row, seed-13 models,
tests/test_batch_sampling.py's samplers at base temperature T, measured on the reference Model alone
(reference_counts below; no call of the new code involved) --
    T                        24        48        96       192
    mini-1b    (of 48)    47 / 11   48 / 11
    mini-4b    (of 48)    35 / 7    46 / 10
    mini-27b   (of 48)     8 / 1    32 / 5    44 / 10   47 / 11
The tests require a third (16 of 48) and three distinct ids in every row.  test_batch_sampling.py's LOOP_T = 24
passes on mini-1b and mini-4b; mini-27b stays on the arg-max there (one row never leaves token 200), so it runs at 48,
where two thirds of the entries leave it and its rows still repeat ids (drafts from a row's own tail get accepted).

Every case asserts that the f16-redo counter did not move.  Every step here has B (draft_len + 1) <= 128 token rows,
below mini-4b's GEMM switch, and mini-27b runs with LLMI_PG6=1 on both sides (tests/test_batch_extend.py explains).
"""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest
from test_batch_decode import CTX, raises, read_kv, vocab_of
from test_batch_lookup import MODEL_ENV, SLOTS, assert_rows, cut, env, expect, preload, rand_tokens, random_rows
from test_batch_sampling import LOOP_T, gguf, samplers_at

pytestmark = pytest.mark.gpu
MAX_NEW = 12
LENS = (6, 34, 70, 131)
TEMP = {"mini-1b": LOOP_T, "mini-4b": LOOP_T, "mini-27b": 48.0}
FORK_ROW, FORK_SEED, FORK_SLOT = 2, 909, 0


@contextlib.contextmanager
def lookup_env(no_gather=False, **kv):
    """test_batch_lookup.env plus LLMI_LOOKUP_NO_GATHER, which the library reads at the call."""
    old = os.environ.pop("LLMI_LOOKUP_NO_GATHER", None)
    if no_gather:
        os.environ["LLMI_LOOKUP_NO_GATHER"] = "1"
    try:
        with env(**kv):
            yield
    finally:
        os.environ.pop("LLMI_LOOKUP_NO_GATHER", None)
        if old is not None:
            os.environ["LLMI_LOOKUP_NO_GATHER"] = old


def columns(out, stop=()):
    return [cut(out[:, b], stop) for b in range(out.shape[1])]


@functools.lru_cache(maxsize=None)
def case(cfg_name, lens=LENS, kv=(), T=None):
    """The prompts and everything the reference Model says about them, computed once per (model, prompt lengths,
    environment) and shared: the sampled ids with the arg-max of the same logits, row 0's K/V caches after that run,
    the mixed, top_k = 1, stop-id and forked variants."""
    from llm_inference_amd.model import Model
    T = TEMP[cfg_name] if T is None else T
    prompts = random_rows(cfg_name, lens)
    n = len(prompts)
    sps = list(samplers_at(T)[:n])
    first, pos, slots = [int(x[-1]) for x in prompts], [len(x) - 1 for x in prompts], list(SLOTS[:n])
    c = dict(prompts=prompts, samplers=sps, first=first, pos=pos, slots=slots)
    with env(**dict(MODEL_ENV.get(cfg_name, {}), **dict(kv))):
        ref = Model(gguf(cfg_name), max_ctx=CTX)
        ref.reserve_sequences(5)
        preload(ref, prompts, slots)
        gen = lambda sp, stop=(): columns(ref.batch_generate(first, slots, pos, MAX_NEW, stop=list(stop), samplers=sp),  # noqa: E731
                                          stop)
        ids = c["ids"] = gen(sps)
        assert all(len(x) == MAX_NEW for x in ids)
        c["kv"] = read_kv(ref, slots[0], cfg_name)
        # the arg-max of the same logits: the spans [cur, r[0..n-1)] at the same positions carry forward's logits bits
        ex = ref.batch_extend([[first[b]] + ids[b][:-1] for b in range(n)], slots, pos, out="all", want_logits=True)
        c["amax"] = [np.argmax(ex.logits[ex.offsets[b]:ex.offsets[b + 1]], axis=1).tolist() for b in range(n)]
        c["greedy"] = columns(ref.batch_generate(first, slots, pos, MAX_NEW))
        if n == 4:
            c["mixed_sps"] = [None, sps[1], None, sps[3]]
            c["mixed"] = gen(c["mixed_sps"])
            c["k1_sps"] = [dict(sp, top_k=1) for sp in sps]
            c["k1"] = gen(c["k1_sps"])
            # a stop id that some row first emits at step 2..6: inside the first step's accepted draft (draft_len 7)
            hit = [(b, k) for b in range(n) for k in range(2, 7) if ids[b][k] not in ids[b][:k]]
            if hit:
                c["stop_row"], c["stop_at"] = hit[0]
                c["stop"] = (ids[hit[0][0]][hit[0][1]],)
                c["stop_ids"] = gen(sps, c["stop"])
            c["fork_sp"] = dict(sps[FORK_ROW], seed=FORK_SEED)
            ref.copy_sequence(FORK_SLOT, slots[FORK_ROW], pos[FORK_ROW])
            out = ref.batch_generate([first[FORK_ROW]] * 2, [slots[FORK_ROW], FORK_SLOT], [pos[FORK_ROW]] * 2, MAX_NEW,
                                     samplers=[sps[FORK_ROW], c["fork_sp"]])
            c["fork_ids"] = columns(out)
        assert ref.get_info().prefill_f16_redo == 0
        ref.close()
    return c


def reference_counts(c):
    """(entries whose sampled id leaves the arg-max, entries, the fewest distinct ids of a row)."""
    off = sum(a != b for r, am in zip(c["ids"], c["amax"]) for a, b in zip(r, am))
    return off, sum(len(r) for r in c["ids"]), min(len(set(r)) for r in c["ids"])


def assert_reference_is_sampled(c, name):
    off, n, distinct = reference_counts(c)
    print(f"{name}: {off} of {n} reference ids leave the arg-max; at least {distinct} distinct ids per row")
    assert 3 * off >= n, (name, off, n)
    assert distinct >= 3, (name, distinct)


# histories: f = filler tokens that occur nowhere else (not in r, not in the prompt)
def fillers(cfg_name, avoid, n=40):
    free = [t for t in range(200, vocab_of(cfg_name)) if t not in avoid]
    return free[:n]


def hist_full(cur, r, f):
    """... f0 f1 cur r0 r1 r2 ... | f2 f0 f1 cur: the 3-gram before the end matches once, its continuation is r."""
    return [f[0], f[1], cur] + list(r) + [f[2], f[0], f[1], cur]


def hist_partial(cur, r, f):
    """... cur r0 r1 x, x != r2: two of the first three draft tokens are right."""
    return [f[0], f[1], cur, r[0], r[1], f[3], f[4], f[5], f[2], f[0], f[1], cur]


def hist_none(cur, r, f):
    """... cur y, y != r0: no draft token is right."""
    return [f[0], f[1], cur, f[3], f[4], f[5], f[6], f[2], f[0], f[1], cur]


def hist_nomatch(cur, r, f):
    """Distinct tokens: the first step finds no match and drafts nothing."""
    return f[10:30] + [cur]


def histories(cfg_name, c, kinds, ids=None):
    ids = c["ids"] if ids is None else ids
    out = []
    for b, kind in enumerate(kinds):
        f = fillers(cfg_name, set(ids[b]) | set(c["prompts"][b].tolist()))
        out.append(np.array(kind(c["first"][b], ids[b], f), np.int32))
    return out


def fresh(cfg_name, c, n_seq=5, junk=None):
    from llm_inference_amd.model import Model
    m = Model(gguf(cfg_name), max_ctx=CTX)
    m.reserve_sequences(n_seq)
    preload(m, c["prompts"], c["slots"], junk=junk)
    return m


def run(m, hists, slots, pos, samplers, max_new=MAX_NEW, **kw):
    r = m.batch_generate_lookup_sampled(hists, slots, pos, max_new, samplers, **kw)
    assert m.get_info().prefill_f16_redo == 0, "the f16 path overflowed: the bits compared would be the int8 path's"
    assert len(r.ids) == len(hists) and all(x.dtype == np.int32 for x in r.ids)
    return r


def traces(hists, ids, D, **kw):
    tr = []
    for h, r in zip(hists, ids):
        t = []
        expect(h, r, MAX_NEW, D, trace=t, **kw)
        tr.append(t)
    return tr


# ---------------------------------------------------------------------------
# 1. the reference samples
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b", "mini-27b"])
def test_reference_is_not_the_greedy_sequence(cfg_name):
    c = case(cfg_name)
    assert_reference_is_sampled(c, cfg_name)
    assert c["ids"] != c["greedy"]


# ---------------------------------------------------------------------------
# 2. acceptance steered through the history, and what the slot holds afterwards
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_acceptance_follows_the_history(cfg_name):
    c = case(cfg_name)
    assert_reference_is_sampled(c, cfg_name)
    D = 3
    hists = histories(cfg_name, c, [hist_partial, hist_none, hist_nomatch, hist_full])
    tr = traces(hists, c["ids"], D)
    r0 = c["ids"][0]
    assert tr[0][0] == (r0[:2] + [hists[0][5]], r0[:3]) and hists[0][5] != r0[2]   # two of three accepted
    assert len(tr[1][0][0]) == D and tr[1][0][0][0] != c["ids"][1][0] and len(tr[1][0][1]) == 1  # none accepted
    assert tr[2][0][0] == []                                                        # no match: an empty draft
    r3 = c["ids"][3]
    assert tr[3][0] == (r3[:D], r3[:D + 1])                                         # the draft accepted whole
    with lookup_env():
        m = fresh(cfg_name, c, junk=c["slots"][0])
        kc0, vc0 = read_kv(m, c["slots"][0], cfg_name)
        r = run(m, hists, c["slots"], c["pos"], c["samplers"], draft_len=D)
        kc1, vc1 = read_kv(m, c["slots"][0], cfg_name)
        m.close()
    steps = assert_rows(r, hists, c["ids"], MAX_NEW, D, cfg_name)
    assert r.steps == steps
    assert 2 <= r.accepted[0] < r.drafted[0] and r.accepted[1] < r.drafted[1] and r.accepted[3] >= D
    assert [len(x) for x in r.ids] == [MAX_NEW] * 4
    # row 0's slot: rows pos .. pos + n_out - 1 carry batch_generate's bits; rows at and past pos + max_new are the junk
    kcr, vcr = c["kv"]
    lo, hi = c["pos"][0], c["pos"][0] + MAX_NEW
    np.testing.assert_array_equal(kc1[:, :, lo:hi], kcr[:, :, lo:hi])
    np.testing.assert_array_equal(vc1[:, :, lo:hi], vcr[:, :, lo:hi])
    np.testing.assert_array_equal(kc1[:, :, hi:], kc0[:, :, hi:])
    np.testing.assert_array_equal(vc1[:, :, hi:], vc0[:, :, hi:])
    assert (kc1[:, :, lo:hi] != kc0[:, :, lo:hi]).any()


@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_full_acceptance_and_no_draft(cfg_name):
    c = case(cfg_name)
    D = 7
    full = histories(cfg_name, c, [hist_full] * 4)
    bare = histories(cfg_name, c, [hist_nomatch] * 4)
    assert all(t[0][0] == [] for t in traces(bare, c["ids"], D))  # step 1: B live token rows
    tr = traces(full, c["ids"], D)
    # step 1 accepts seven drafts; whatever step 2 drafts is cut to the 3 ids left: max_new ends inside a draft
    assert all(t[0] == (r[:D], r[:D + 1]) and len(t[1][0]) in (0, 3) for t, r in zip(tr, c["ids"]))
    with lookup_env():
        m = fresh(cfg_name, c)
        r = run(m, full, c["slots"], c["pos"], c["samplers"], draft_len=D)
        steps = assert_rows(r, full, c["ids"], MAX_NEW, D, "full acceptance")
        assert r.steps == steps and (r.accepted >= D).all()
        r = run(m, bare, c["slots"], c["pos"], c["samplers"], draft_len=D)
        steps = assert_rows(r, bare, c["ids"], MAX_NEW, D, "no match")
        assert r.steps == steps
        m.close()


# ---------------------------------------------------------------------------
# 3. independence
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_rows_independent_of_the_call(cfg_name):
    """The same rows alone, reversed, inside B = 16 among unrelated rows with samplers of their own (16 x 8 = 128 token
    rows), with draft_len 1, 4 and 31 (4 x 32 = 128 token rows: two chunks of compact rows), LLMI_LOOKUP_SYNC 1 and
    64, and without the live-row list (LLMI_LOOKUP_NO_GATHER=1)."""
    c = case(cfg_name)
    assert_reference_is_sampled(c, cfg_name)
    ids, slots, pos, sps = c["ids"], c["slots"], c["pos"], c["samplers"]
    hists = histories(cfg_name, c, [hist_partial, hist_none, hist_nomatch, hist_full])
    V = vocab_of(cfg_name)
    rng = np.random.default_rng(5)
    with lookup_env():
        m = fresh(cfg_name, c, n_seq=17)
        for b in range(4):
            r = run(m, [hists[b]], [slots[b]], [pos[b]], [sps[b]], draft_len=7)
            assert_rows(r, [hists[b]], [ids[b]], MAX_NEW, 7, f"alone, row {b}")
        rev = [3, 2, 1, 0]
        r = run(m, [hists[b] for b in rev], [slots[b] for b in rev], [pos[b] for b in rev], [sps[b] for b in rev])
        assert_rows(r, [hists[b] for b in rev], [ids[b] for b in rev], MAX_NEW, 7, "reversed")
        for D in (1, 4, 31):
            r = run(m, hists, slots, pos, sps, draft_len=D)
            assert_rows(r, hists, ids, MAX_NEW, D, f"draft_len {D}")
        for sync in (1, 64):
            with lookup_env(LLMI_LOOKUP_SYNC=sync):
                r = run(m, hists, slots, pos, sps)
            steps = assert_rows(r, hists, ids, MAX_NEW, 7, f"LLMI_LOOKUP_SYNC {sync}")
            assert r.steps == steps
        for D in (7, 31):
            with lookup_env(no_gather=True):
                r = run(m, hists, slots, pos, sps, draft_len=D)
            assert_rows(r, hists, ids, MAX_NEW, D, f"LLMI_LOOKUP_NO_GATHER, draft_len {D}")
        # B = 16: the four rows at 0, 5, 10, 15, unrelated rows on slots 5..16 around them, two of them greedy
        where = {0: 0, 5: 1, 10: 2, 15: 3}
        others = [rand_tokens(rng, V, int(n)) for n in rng.integers(3, 20, 12)]
        spare = list(range(5, 17))
        preload(m, others, spare)
        hs, sl, ps, sp = [], [], [], []
        for b in range(16):
            if b in where:
                k = where[b]
                hs.append(hists[k]), sl.append(slots[k]), ps.append(pos[k]), sp.append(sps[k])
            else:
                x = others.pop()
                hs.append(x), sl.append(spare.pop()), ps.append(len(x) - 1)
                sp.append(None if b in (3, 12) else dict(temperature=float(rng.uniform(0.5, 40)),
                                                         top_k=int(rng.integers(0, 257)), seed=int(rng.integers(1 << 40))))
        r = run(m, hs, sl, ps, sp)
        assert_rows(r, hists, ids, MAX_NEW, 7, "inside B = 16", idx=list(where))
        m.close()


@pytest.mark.parametrize("ks", [1, 8])
def test_rows_under_other_key_splits(ks):
    cfg_name = "mini-4b"
    kv = {"LLMI_PREFILL_ATTN_KS": ks}
    c = case(cfg_name, kv=tuple(kv.items()))
    hists = histories(cfg_name, c, [hist_partial, hist_none, hist_nomatch, hist_full])
    with lookup_env(**kv):
        m = fresh(cfg_name, c)
        r = run(m, hists, c["slots"], c["pos"], c["samplers"])
        m.close()
    assert_rows(r, hists, c["ids"], MAX_NEW, 7, f"ks = {ks}")


# ---------------------------------------------------------------------------
# 4. greedy rows, top_k = 1, two seeds
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_mixed_and_all_greedy_rows(cfg_name):
    c = case(cfg_name)
    slots, pos = c["slots"], c["pos"]
    assert [c["mixed"][b] for b in (0, 2)] == [c["greedy"][b] for b in (0, 2)]
    assert [c["mixed"][b] for b in (1, 3)] == [c["ids"][b] for b in (1, 3)]
    mixed_h = histories(cfg_name, c, [hist_full, hist_partial, hist_partial, hist_full], ids=c["mixed"])
    greedy_h = histories(cfg_name, c, [hist_full, hist_partial, hist_none, hist_nomatch], ids=c["greedy"])
    k1_h = histories(cfg_name, c, [hist_full, hist_partial, hist_none, hist_nomatch], ids=c["k1"])
    with lookup_env():
        m = fresh(cfg_name, c)
        r = run(m, mixed_h, slots, pos, c["mixed_sps"])
        assert_rows(r, mixed_h, c["mixed"], MAX_NEW, 7, "mixed rows")
        r = run(m, mixed_h, slots, pos, [dict(temperature=0.0), c["samplers"][1], None, c["samplers"][3]])
        assert_rows(r, mixed_h, c["mixed"], MAX_NEW, 7, "temperature 0 is a greedy row")
        with lookup_env(no_gather=True):
            r = run(m, mixed_h, slots, pos, c["mixed_sps"])
        assert_rows(r, mixed_h, c["mixed"], MAX_NEW, 7, "mixed rows, LLMI_LOOKUP_NO_GATHER")
        # every row greedy: batch_generate_lookup's result
        want = m.batch_generate_lookup(greedy_h, slots, pos, MAX_NEW)
        r = run(m, greedy_h, slots, pos, [None] * 4)
        assert_rows(r, greedy_h, c["greedy"], MAX_NEW, 7, "all greedy")
        assert [x.tolist() for x in r.ids] == [x.tolist() for x in want.ids] and r.steps == want.steps
        assert r.drafted.tolist() == want.drafted.tolist() and r.accepted.tolist() == want.accepted.tolist()
        # top_k = 1: the draw has one candidate
        r = run(m, k1_h, slots, pos, c["k1_sps"])
        assert_rows(r, k1_h, c["k1"], MAX_NEW, 7, "top_k = 1")
        m.close()


@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_fork_with_two_seeds(cfg_name):
    c = case(cfg_name)
    a, b = c["fork_ids"]
    assert a == c["ids"][FORK_ROW] and a != b, "the two seeds give the same ids on the reference"
    slot, p = c["slots"][FORK_ROW], c["pos"][FORK_ROW]
    f = fillers(cfg_name, set(a) | set(b) | set(c["prompts"][FORK_ROW].tolist()))
    cur = c["first"][FORK_ROW]
    hists = [np.array(hist_full(cur, a, f), np.int32), np.array(hist_full(cur, a, f), np.int32)]  # b drafts a's ids
    with lookup_env():
        m = fresh(cfg_name, c)
        m.copy_sequence(FORK_SLOT, slot, p)
        r = run(m, hists, [slot, FORK_SLOT], [p, p], [c["samplers"][FORK_ROW], c["fork_sp"]])
        m.close()
    assert_rows(r, hists, [a, b], MAX_NEW, 7, "fork")
    assert r.accepted[0] >= 7


# ---------------------------------------------------------------------------
# 5. stop ids, the budget
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_stop_id_inside_an_accepted_draft(cfg_name):
    from llm_inference_amd._lib import Lookup, check, lib, ptr
    from llm_inference_amd.model import marshal_lookup, marshal_samplers, normalize_samplers
    c = case(cfg_name)
    assert "stop" in c, "no row first emits an id at step 2..6"
    stop, k, row = c["stop"], c["stop_at"], c["stop_row"]
    want = c["stop_ids"]
    assert want[row] == c["ids"][row][:k + 1] and 2 <= k < 7
    hists = histories(cfg_name, c, [hist_full] * 4)  # (drafts of the ids the rows would emit without the stop id)
    tr = traces(hists, c["ids"], 7)
    assert len(tr[row][0][1]) == 8, "without the stop id the row's first step accepts seven drafts: the id lands inside"
    with lookup_env():
        m = fresh(cfg_name, c)
        r = run(m, hists, c["slots"], c["pos"], c["samplers"], stop=stop)
        tok, hl, sl, p = marshal_lookup(hists, c["slots"], c["pos"])
        out, n_out = np.zeros((4, MAX_NEW), np.int32), np.zeros(4, np.int32)
        st = np.array(stop, np.int32)
        lk = Lookup(7, 3, 1, MAX_NEW)
        arr = marshal_samplers(normalize_samplers(c["samplers"], 4))
        check(lib().llmi_session_batch_generate_lookup_sampled(m.h, ptr(tok), ptr(hl), ptr(sl), ptr(p), 4, C.byref(lk), 0,
                                                               ptr(st), 1, arr, ptr(out), ptr(n_out), None))
        m.close()
    assert_rows(r, hists, want, MAX_NEW, 7, cfg_name, stop=stop)
    assert n_out.tolist() == [len(x) for x in want] and n_out[row] == k + 1
    for b in range(4):
        assert out[b, :n_out[b]].tolist() == want[b] and (out[b, n_out[b]:] == -1).all()


def test_budget():
    cfg_name = "mini-4b"
    lens = (CTX - MAX_NEW + 1, 34, 70)
    c = case(cfg_name, lens=lens)
    assert c["pos"][0] + MAX_NEW == CTX  # row 0 ends at max_ctx exactly
    hists = histories(cfg_name, c, [hist_full] * 3)
    with lookup_env():
        m = fresh(cfg_name, c)
        r = run(m, hists, c["slots"], c["pos"], c["samplers"])
        steps = assert_rows(r, hists, c["ids"], MAX_NEW, 7, "max_new inside a draft")
        assert r.steps == steps and (r.accepted >= 7).all() and [len(x) for x in r.ids] == [MAX_NEW] * 3
        r = run(m, hists, c["slots"], c["pos"], c["samplers"], max_steps=1)
        assert_rows(r, hists, c["ids"], MAX_NEW, 7, "max_steps = 1", max_steps=1)
        assert r.steps == 1 and [x.tolist() for x in r.ids] == [ids[:8] for ids in c["ids"]]
        r = run(m, hists, c["slots"], c["pos"], c["samplers"], max_new=1)  # max_new = 1: no draft at all
        assert [x.tolist() for x in r.ids] == [ids[:1] for ids in c["ids"]] and r.drafted.sum() == 0 and r.steps == 1
        m.close()


# ---------------------------------------------------------------------------
# 6. head_dim 128
# ---------------------------------------------------------------------------
def test_mini_27b():
    cfg_name = "mini-27b"
    c = case(cfg_name)
    assert_reference_is_sampled(c, cfg_name)
    hists = histories(cfg_name, c, [hist_partial, hist_none, hist_nomatch, hist_full])
    with lookup_env(**MODEL_ENV[cfg_name]):
        m = fresh(cfg_name, c)
        r = run(m, hists, c["slots"], c["pos"], c["samplers"], draft_len=3)
        with lookup_env(no_gather=True, **MODEL_ENV[cfg_name]):
            r2 = run(m, hists, c["slots"], c["pos"], c["samplers"], draft_len=3)
        m.close()
    assert_rows(r, hists, c["ids"], MAX_NEW, 3, cfg_name)
    assert_rows(r2, hists, c["ids"], MAX_NEW, 3, cfg_name + ", LLMI_LOOKUP_NO_GATHER")
    assert 2 <= r.accepted[0] < r.drafted[0] and r.accepted[3] >= 3


# ---------------------------------------------------------------------------
# 7. errors
# ---------------------------------------------------------------------------
def test_argument_errors():
    from llm_inference_amd._lib import LLMIError, Lookup, check, lib, ptr
    from llm_inference_amd.model import Model
    cfg_name = "mini-1b"
    V = vocab_of(cfg_name)
    h = [5, 6, 7]
    sp = dict(temperature=1.0, top_k=64, top_p=0.95, seed=1)
    with lookup_env():
        m = Model(gguf(cfg_name), max_ctx=64)
        f = lambda hs, sl, ps, n, **kw: m.batch_generate_lookup_sampled(hs, sl, ps, n, kw.pop("samplers", sp), **kw)  # noqa: E731
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
        # the samplers: a null pointer; a bad field names the field and the row
        tok, one, two = np.array(h, np.int32), np.array([3], np.int32), np.array([2], np.int32)
        out, n_out = np.zeros(4, np.int32), np.zeros(1, np.int32)
        lk = Lookup(7, 3, 1, 4)
        with pytest.raises(LLMIError) as ei:
            check(lib().llmi_session_batch_generate_lookup_sampled(m.h, ptr(tok), ptr(one), ptr(two), ptr(two), 1,
                                                                   C.byref(lk), 0, None, 0, None, ptr(out), ptr(n_out),
                                                                   None))
        assert ei.value.status == "E_ARG" and "(samplers)" in str(ei.value)
        for kw, field in [(dict(temperature=-0.5), "temperature"), (dict(temperature=float("nan")), "temperature"),
                          (dict(temperature=1.0, top_k=-3), "top_k"), (dict(temperature=1.0, top_k=300), "top_k"),
                          (dict(temperature=1.0, top_p=0.0), "top_p"), (dict(temperature=1.0, top_p=1.01), "top_p")]:
            with pytest.raises(LLMIError) as ei:
                f([h, h, h], [0, 1, 2], [2, 2, 2], 4, samplers=[sp, None, kw])
            assert ei.value.status == "E_ARG" and field in str(ei.value) and "samplers[2]" in str(ei.value), str(ei.value)
        # the session still works: the same ids as the sampled batch loop, and its own sampler was never touched
        x = np.array([5, 6, 7], np.int32)
        m.forward(x[:2], 0, want_logits=False)
        m.copy_sequence(2, 0, 2)
        want = m.batch_generate([7], [2], [2], 4, samplers=sp)[:, 0]
        got = f([x], [2], [2], 4)
        assert got.ids[0].tolist() == want.tolist() and m.get_info().prefill_f16_redo == 0
        assert m.get_info().sampling == 0
        m.close()


# ---------------------------------------------------------------------------
# 8. time_kernel(14)
# ---------------------------------------------------------------------------
def test_time_kernel_lookup_select():
    from llm_inference_amd import ops
    from llm_inference_amd.synthetic import CONFIGS
    cfg_name = "mini-4b"
    cfg = CONFIGS[cfg_name]
    c = case(cfg_name)
    D = 7
    hists = histories(cfg_name, c, [hist_partial, hist_none, hist_nomatch, hist_full])
    tr = traces(hists, c["ids"], D)
    last = max(len(t) for t in tr)
    n_live = sum(1 + len(t[-1][0]) for t in tr if len(t) == last)  # the last step's live token rows
    rb = ops.logits_rows_rb(cfg.n_embd)
    table = cfg.vocab * cfg.n_embd * 2
    with lookup_env():
        m = fresh(cfg_name, c)
        assert m.time_kernel(14, 2) == (0.0, 0.0)
        m.batch_generate_lookup(hists, c["slots"], c["pos"], MAX_NEW)  # a greedy lookup step is not a sampled one
        assert m.time_kernel(14, 2) == (0.0, 0.0)
        r = run(m, hists, c["slots"], c["pos"], c["samplers"], draft_len=D)
        us, by = m.time_kernel(14, 3)
        # the launches change no state: the call again gives the same result
        r2 = run(m, hists, c["slots"], c["pos"], c["samplers"], draft_len=D)
        with lookup_env(no_gather=True):
            run(m, hists, c["slots"], c["pos"], c["samplers"], draft_len=D)
            us_all, by_all = m.time_kernel(14, 3)
        m.close()
    assert_rows(r, hists, c["ids"], MAX_NEW, D, "before timing")
    assert [x.tolist() for x in r2.ids] == [x.tolist() for x in r.ids] and r2.steps == r.steps == last
    print(f"time_kernel(14): {us:.1f} us for {by:.0f} bytes ({n_live} live rows of {4 * (D + 1)}, RB = {rb}); "
          f"without the list {us_all:.1f} us for {by_all:.0f} bytes")
    assert rb == 8 and 1 <= n_live < 4 * (D + 1)
    assert us > 0.0 and by == float(-(-n_live // rb) * table + n_live * cfg.vocab * 4)
    T = 4 * (D + 1)
    assert us_all > 0.0 and by_all == float(-(-T // rb) * table + T * cfg.vocab * 4)
