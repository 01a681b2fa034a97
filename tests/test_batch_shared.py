"""Shared-prefix attention for batch steps (llmi_session_seq_share / Model.share_prefix).

The row contract of section 12 is unchanged and needs no tolerance: a batch row's argmax / lse / logits are the bits of
Model.score / Model.forward of the row's whole prefix on a single-sequence session, whether the step read the forked
prompt's K/V once per group or once per row.  The reference Model never reserves a slot.

mini-4b and mini-27b run the contract cases with LLMI_PG6=1 on both sides, as tests/test_batch_extend.py does: a prompt
past 384 tokens (128 on mini-27b) takes another f16 GEMM than a batch step ("The GEMM switch").
By default the host groups only as many rows as measured faster (section 19.5); the tests of small groups lower that to
2 with LLMI_BATCH_SHARED_MIN_ROWS, the 33-row test runs with the default.
"""
import functools

import numpy as np
import pytest

from test_batch_decode import CHAIN, CTX, chain_gguf, gguf, u32, vocab_of
from test_batch_extend import env

pytestmark = pytest.mark.gpu


@pytest.fixture
def small_groups(monkeypatch):
    monkeypatch.setenv("LLMI_BATCH_SHARED_MIN_ROWS", "2")


MODEL_ENV = {"mini-4b": {"LLMI_PG6": 1}, "mini-27b": {"LLMI_PG6": 1}}
OWN = (0, 1, 31, 33, 100)  # tokens each slot runs past the shared prefix before the checked step (slot 0: the leader)


@functools.lru_cache(maxsize=None)
def fork_case(cfg_name, n_pos, ks=None):
    """One prompt of n_pos tokens, five continuations of it, and the single-sequence session's last position of each
    continuation: (argmax, lse, logits).  Computed once per case, read-only."""
    from llm_inference_amd.model import Model
    rng = np.random.default_rng(1000 + n_pos)
    V = vocab_of(cfg_name)
    base = rng.integers(4, V, n_pos).astype(np.int32)
    seqs = [np.concatenate([base, rng.integers(4, V, own + 1).astype(np.int32)]) for own in OWN]
    kv = dict(MODEL_ENV.get(cfg_name, {}), **({} if ks is None else {"LLMI_PREFILL_ATTN_KS": ks}))
    am, lse, lg = [], [], []
    with env(**kv):
        ref = Model(gguf(cfg_name), max_ctx=CTX)
        for x in seqs:
            sc = ref.score(x)
            am.append(int(sc.argmax[-1]))
            lse.append(sc.lse[-1])
            lg.append(ref.forward(x, 0))
        ref.close()
    lg = np.stack(lg)
    lg.setflags(write=False)
    return dict(base=base, seqs=seqs, kv=kv, argmax=np.array(am, np.int32), lse=np.array(lse, np.float32), logits=lg)


def fork_and_extend(m, c, n_pos):
    """The prompt into slot 0, shared into slots 1..4, every slot then run to its own length by batch steps."""
    m.forward(c["base"], 0, want_logits=False)
    for s in range(1, 5):
        m.share_prefix(s, 0, n_pos)
    for j in range(max(OWN)):
        live = [s for s in range(5) if j < OWN[s]]
        m.batch_forward([int(c["seqs"][s][n_pos + j]) for s in live], live, [n_pos + j] * len(live))


def shared_bytes(cfg_name, groups, rows):
    """time_kernel(16)'s count: K and V rows [0, P) once per group and P_b .. pos of every row, P the floor of the
    group's length to the layer's round of 32 S keys; groups: (length, rows of the group), rows: positions."""
    from llm_inference_amd.synthetic import CONFIGS
    cfg = CONFIGS[cfg_name]
    S = 2 if cfg.head_dim >= 256 or cfg.n_head // cfg.n_head_kv == 4 else 4
    row = 2 * cfg.n_head_kv * cfg.head_dim * 2
    own = {b: 0 for b in range(len(rows))}
    total = 0
    for length, members in groups:
        P = length // (32 * S) * (32 * S)
        total += P * row
        own.update({b: P for b in members})
    return total + sum((p + 1 - own[b]) * row for b, p in enumerate(rows))


CASES = [(c, None) for c in ("mini-1b", "mini-4b", "mini-27b")] + [("mini-4b", 1), ("mini-4b", 8)]


@pytest.mark.parametrize("n_pos", [128, 129, 200, 320])
@pytest.mark.parametrize("cfg_name,ks", CASES)
def test_forked_rows_equal_single_sequence_bits(cfg_name, ks, n_pos, small_groups):
    """Exactly one and two rounds, one key past a round, a floor that differs between S = 2 and S = 4, several rounds
    per work-group; the rows in order, reversed, and beside two unlinked rows; also under LLMI_PREFILL_ATTN_KS 1 / 8."""
    from llm_inference_amd.model import Model
    c = fork_case(cfg_name, n_pos, ks)
    tok = [int(x[-1]) for x in c["seqs"]]
    pos = [n_pos + own for own in OWN]
    with env(**c["kv"]):
        m = Model(gguf(cfg_name), max_ctx=CTX)
        m.reserve_sequences(7)
        fork_and_extend(m, c, n_pos)
        fwd = m.batch_forward(tok, list(range(5)), pos, want_logits=True)
        us, by = m.time_kernel(16, 1)
        by10 = m.time_kernel(10, 1)[1]
        rev = m.batch_forward(tok[::-1], list(range(5))[::-1], pos[::-1], want_logits=True)
        mix = m.batch_forward([7] + tok[:2] + [9] + tok[2:], [5, 0, 1, 6, 2, 3, 4], [40] + pos[:2] + [150] + pos[2:],
                              want_logits=True)
        m.close()
    for what, got, idx in (("in order", fwd, slice(None)), ("reversed", rev, slice(None, None, -1)),
                           ("mixed", mix, [1, 2, 4, 5, 6])):
        np.testing.assert_array_equal(got.argmax[idx], c["argmax"], err_msg=what)
        np.testing.assert_array_equal(u32(got.lse[idx]), u32(c["lse"]), err_msg=what)
        np.testing.assert_array_equal(u32(got.logits[idx]), u32(c["logits"]), err_msg=what)
    # the path is taken: one group of the five rows, the leader's own row bounding it at n_pos
    assert us > 0 and 0 < by < by10
    assert by == shared_bytes(cfg_name, [(n_pos, range(5))], pos)


def test_group_of_32_and_a_row_that_falls_back(monkeypatch):
    """33 followers of one leader: a group of 32 and one row on its own; against the same call unshared."""
    from llm_inference_amd.model import Model
    rng = np.random.default_rng(3)
    base = rng.integers(4, vocab_of("mini-4b"), 200).astype(np.int32)
    tok = rng.integers(4, vocab_of("mini-4b"), 33).tolist()
    with env():
        m = Model(gguf("mini-4b"), max_ctx=CTX)
        m.reserve_sequences(34)
        m.forward(base, 0, want_logits=False)
        for s in range(1, 34):
            m.share_prefix(s, 0, 200)
        got = m.batch_forward(tok, list(range(1, 34)), [200] * 33)
        by = m.time_kernel(16, 1)[1]
        monkeypatch.setenv("LLMI_BATCH_SHARED", "0")
        ref = m.batch_forward(tok, list(range(1, 34)), [200] * 33)
        off = m.time_kernel(16, 1)
        m.close()
    np.testing.assert_array_equal(got.argmax, ref.argmax)
    np.testing.assert_array_equal(u32(got.lse), u32(ref.lse))
    assert by == shared_bytes("mini-4b", [(200, range(32))], [200] * 33) and off == (0.0, 0.0)


@pytest.mark.parametrize("sampled", [False, True])
def test_loop_over_a_shared_group(sampled, small_groups):
    """batch_generate for 40 steps over a forked prompt, one row stopping, against the same loop after copy_sequence;
    the chain-rewritten token table makes the ids move."""
    from llm_inference_amd.model import Model
    rng = np.random.default_rng(8)
    base = rng.integers(4, vocab_of("mini-4b"), 140).astype(np.int32)
    first = [CHAIN[0], 50, 60, CHAIN[1]]
    samplers = [None, dict(temperature=1.0, top_k=64, seed=5), None, None] if sampled else None
    outs = []
    with env():
        m = Model(chain_gguf("mini-4b"), max_ctx=CTX)
        m.reserve_sequences(5)
        for fork in (m.share_prefix, m.copy_sequence):
            m.forward(base, 0, want_logits=False)
            for s in range(1, 5):
                fork(s, 0, 140)
            outs.append(m.batch_generate(first, [1, 2, 3, 4], [140] * 4, 40, stop=[CHAIN[2]], samplers=samplers))
            grouped = m.time_kernel(16, 1)[1] > 0
            assert grouped == (fork == m.share_prefix)
        m.close()
    np.testing.assert_array_equal(outs[0], outs[1])
    assert outs[0][0, 0] == CHAIN[1] and outs[0][1, 0] == CHAIN[2] and (outs[0][2:, 0] == -1).all()
    assert (outs[0][:, 2] >= 0).all()


def test_a_write_to_the_leader_trims_the_links(small_groups):
    """Position 150 of slot 0 is rewritten after two slots shared 200 rows of it: their steps still see their own
    prefix (the group reads 128 rows of slot 0, not 192), and slot 0 sees its new one."""
    from llm_inference_amd.model import Model
    rng = np.random.default_rng(17)
    V = vocab_of("mini-4b")
    base = rng.integers(4, V, 200).astype(np.int32)
    other = int((base[150] + 1 - 4) % (V - 4) + 4)
    seqs = [np.concatenate([base, [11]]), np.concatenate([base, [12]]), np.concatenate([base[:150], [other, 13]])]
    with env():
        ref = Model(gguf("mini-4b"), max_ctx=CTX)
        want = [ref.score(x) for x in seqs]
        ref.close()
        m = Model(gguf("mini-4b"), max_ctx=CTX)
        m.reserve_sequences(4)
        m.forward(base, 0, want_logits=False)
        m.share_prefix(2, 0, 200)
        m.share_prefix(3, 0, 200)
        m.batch_forward([other], [0], [150])
        got = m.batch_forward([11, 12], [2, 3], [200, 200])  # (without slot 0's row, whose position would bound the group)
        by = m.time_kernel(16, 1)[1]
        got0 = m.batch_forward([13], [0], [151])
        m.close()
    np.testing.assert_array_equal(np.append(got.argmax, got0.argmax), [int(w.argmax[-1]) for w in want])
    np.testing.assert_array_equal(u32(np.append(got.lse, got0.lse)), u32([w.lse[-1] for w in want]))
    assert by == shared_bytes("mini-4b", [(150, range(2))], [200, 200])
