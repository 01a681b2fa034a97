"""Top-N alternatives of scoring (llmi_session_score_top / llmi_score_rows_top; csrc/k_score_top.hip; DESIGN.md
section 11.6): ids exactly, log-probs within tests/test_score.py's derived log-prob bound 2 B_t + eps_t
(+ 2 CAP_ULPS under a soft-cap) of logit - logsumexp in float64.

Op-level data are small integers (x in 1..3, w in -3..3, E <= 192): every product and partial sum is an integer below
2^24, exact in f32 in any order, so float64 x @ w.T decides ids, order and ties with no tolerance."""
import functools

import numpy as np
import pytest
from test_score import env, logits_scores, ref_scores, table16, taps

pytestmark = pytest.mark.gpu
SHAPES = [(1, 40, 16), (3, 129, 80), (130, 1000, 64), (5, 4200, 192)]


def lp_bound(ref):
    return 2 * ref["B"] + ref["eps"] + 2 * ref["cap_ulps"]


def top_of(l, n):
    """[T][n] ids, descending by value, ties by lower id."""
    return np.stack([np.lexsort((np.arange(l.shape[1]), -row))[:n] for row in l])


@functools.lru_cache(maxsize=None)
def int_case(T, V, E):
    """Rows 127, 128 and V - 1 share the largest possible logit; 36 (>= N + 3) rows of one tile share the next one;
    34 more random rows are made non-negative with a positive first column, so the leading N + 1 logits are > 0."""
    rng = np.random.default_rng(V + E)
    x = rng.integers(1, 4, (T, E)).astype(np.float16)
    w = rng.integers(-3, 4, (V, E)).astype(np.float16)
    lead = rng.choice(V, min(V, 34), replace=False)
    w[lead] = np.abs(w[lead])
    w[lead, 0] = 1
    eq0 = 260 if V > 300 else 2
    w[eq0:eq0 + 36] = 2
    w[[r for r in (127, 128, V - 1) if r < V]] = 3
    return x, w, ref_scores(x, w, np.full(T, -1))


@pytest.mark.parametrize("n", [1, 5, 32])
@pytest.mark.parametrize("T,V,E", SHAPES)
def test_score_rows_top_exact(T, V, E, n):
    from llm_inference_amd.ops import score_rows, score_rows_top
    x, w, ref = int_case(T, V, E)
    n = min(n, V)
    want = top_of(ref["l"], n + 1 if n < V else n)
    assert (np.take_along_axis(ref["l"], want, 1) > 0).all()  # no signed zero near the top
    got = score_rows_top(x, w, n)
    np.testing.assert_array_equal(got.top_ids, want[:, :n])
    np.testing.assert_array_equal(got.top_ids[:, 0], got.argmax)
    err = np.abs(got.top_logprobs - (np.take_along_axis(ref["l"], want[:, :n], 1) - ref["lse"][:, None]))
    print(f"T={T} V={V} E={E} N={n}: worst error / bound {float((err / lp_bound(ref)[:, None]).max()):.3g}")
    assert (err <= lp_bound(ref)[:, None]).all()
    base = score_rows(x, w)
    for name in ("lse", "argmax"):
        np.testing.assert_array_equal(getattr(got, name).view(np.uint32), getattr(base, name).view(np.uint32))
    if n >= 3:  # the target's log-prob and its slot are one expression
        tg = score_rows_top(x, w, n, got.top_ids[:, 2].copy())
        np.testing.assert_array_equal(tg.top_logprobs[:, 2].view(np.uint32), tg.logprobs.view(np.uint32))
    if T > 5:  # rows 0..4 alone: the same ids and bits
        few = score_rows_top(x[:5], w, n)
        np.testing.assert_array_equal(few.top_ids, got.top_ids[:5])
        np.testing.assert_array_equal(few.top_logprobs.view(np.uint32), got.top_logprobs[:5].view(np.uint32))


def test_score_rows_top_one_leader_per_tile():
    """33 tiles, each with one leader, the leaders strictly descending in tile order 32, 31, ...: the 32 picked tiles
    are all needed, and the one left out is the right one."""
    from llm_inference_amd.ops import score_rows_top
    T, V, E = 2, 4200, 64
    rng = np.random.default_rng(12)
    x = rng.integers(1, 4, (T, E)).astype(np.float16)
    w = rng.integers(-3, 3, (V, E)).astype(np.float16)
    rows = 128 * np.arange(33) + rng.integers(0, 104, 33)
    for j, row in enumerate(rows[::-1]):
        w[row] = 3
        w[row, :j] = 2
    got = score_rows_top(x, w, 32)
    np.testing.assert_array_equal(got.top_ids, np.tile(rows[::-1][:32], (T, 1)))
    np.testing.assert_array_equal(got.top_ids, top_of(x.astype(np.float64) @ w.astype(np.float64).T, 32))


@pytest.mark.parametrize("n", [1, 5, 32])
def test_score_rows_top_softcap(n):
    """cap 30, random f16 data, N + 1 planted leaders whose pre-cap logits step down by >= 0.5 from about 96: orders of
    magnitude above the f32 error of an 80-term chain, and the order survives the cap in float32 and float64."""
    from llm_inference_amd.ops import score_rows_top
    T, V, E, cap = 3, 129, 80, 30.0
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((T, E)) * 0.25).astype(np.float16)
    x[:, 0] = 8
    w = (rng.standard_normal((V, E)) * 0.05).astype(np.float16)
    rows = rng.permutation(V)[:n + 1]
    w[:, 0] = 0
    w[rows, 0] = (12.0 - 0.25 * np.arange(n + 1)).astype(np.float16)  # column 0 adds 96, 94, ... (steps of 2)
    ref = ref_scores(x, w, np.full(T, -1), softcap=cap)
    pre = x.astype(np.float64) @ w.astype(np.float64).T
    want = top_of(pre, n + 1)
    assert (np.sort(want, 1) == np.sort(rows)).all()
    assert (-np.diff(np.take_along_axis(pre, want, 1), axis=1) >= 0.5).all()
    for dt in (np.float32, np.float64):
        capped = dt(cap) * np.tanh(np.take_along_axis(pre, want, 1).astype(dt) / dt(cap))
        assert (np.diff(capped, axis=1) < 0).all()
    got = score_rows_top(x, w, n, softcap=cap)
    np.testing.assert_array_equal(got.top_ids, want[:, :n])
    err = np.abs(got.top_logprobs - (np.take_along_axis(ref["l"], want[:, :n], 1) - ref["lse"][:, None]))
    assert (err <= lp_bound(ref)[:, None]).all(), float((err / lp_bound(ref)[:, None]).max())
    if n >= 3:  # under the cap too, the target's log-prob and its slot are one expression on one chain
        tg = score_rows_top(x, w, n, got.top_ids[:, 2].copy(), softcap=cap)
        np.testing.assert_array_equal(tg.top_logprobs[:, 2].view(np.uint32), tg.logprobs.view(np.uint32))


def test_session_fused_path():
    """600 tokens in two chunks: the session's outputs are the op's on the very rows the scorer read."""
    from llm_inference_amd.model import Model
    from llm_inference_amd.ops import score_rows_top
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg = CONFIGS["mini-1b"]
    g = build_gemma3_gguf(cfg, seed=21)
    prompt = np.random.default_rng(3).integers(4, cfg.vocab, 600).astype(np.int32)
    with env():
        m = Model(g, max_ctx=1024)
        assert m.get_info().score_path == 1
        x16 = taps(m.trace(prompt, 0, score=True), "sc_x16", np.float16).reshape(600, cfg.n_embd)
        plain, r = m.score(prompt), m.score_top(prompt, 5)
        m.close()
    assert plain.top_ids is None and plain.top_logprobs is None and r.top_ids.shape == (600, 5)
    np.testing.assert_array_equal(r.top_ids[:, 0], r.argmax)
    op = score_rows_top(x16, table16(g, cfg), 5)
    np.testing.assert_array_equal(r.top_ids, op.top_ids)
    np.testing.assert_array_equal(r.top_logprobs.view(np.uint32), op.top_logprobs.view(np.uint32))
    for name in ("logprobs", "lse", "argmax"):
        np.testing.assert_array_equal(getattr(r, name).view(np.uint32), getattr(plain, name).view(np.uint32))


def test_session_row_path():
    """An exact-mode session reduces forward's own f32 logits row per position."""
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg = CONFIGS["mini-1b"]
    g = build_gemma3_gguf(cfg, seed=21)
    prompt = np.random.default_rng(4).integers(4, cfg.vocab, 6).astype(np.int32)
    with env():
        m = Model(g, exact=True, max_ctx=64)
        assert m.get_info().score_path == 2
        r = m.score_top(prompt, 5)
        for i in range(len(prompt)):
            lg = m.forward(prompt[:i + 1], 0)
            want = top_of(lg[None, :], 5)[0]
            ref = logits_scores(lg.astype(np.float64)[None, :], [-1])
            np.testing.assert_array_equal(r.top_ids[i], want)
            assert (np.abs(r.top_logprobs[i] - (lg[want].astype(np.float64) - ref["lse"][0])) <= ref["eps"][0]).all()
        m.close()


def test_top_n_errors():
    from llm_inference_amd._lib import LLMIError
    from llm_inference_amd.model import Model
    from llm_inference_amd.ops import score_rows_top
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    x, w = np.zeros((2, 32), np.float16), np.zeros((5, 32), np.float16)
    with env():
        m = Model(build_gemma3_gguf(CONFIGS["mini-1b"], seed=21), max_ctx=64)
        calls = [lambda k=k: score_rows_top(x, w, k) for k in (-1, 33, 6)] + \
                [lambda k=k: m.score_top([5, 6, 7], k) for k in (-1, 33)]
        for call in calls:
            with pytest.raises(LLMIError) as ei:
                call()
            assert ei.value.status == "E_RANGE" and "top_n" in str(ei.value)
        assert m.score_top([5, 6, 7], 2).top_ids.shape == (3, 2)  # and the session still works
        m.close()
