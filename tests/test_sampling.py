"""Seeded temperature / top-k / top-p sampling (csrc/sample.h, csrc/k_sample.hip).

The rule is integer wherever order could matter, so the device result is a pure function of the logits' bits, the
parameters, the seed and the position.  `ref_sample` below restates it in numpy and Python integers (expf from the
host's libm: np.exp on float32 differs from glibc's expf in the last bit) and shares no code with the library:

  1. candidates: the top K' = min(K, non-NaN logits) ids by (logit descending, id ascending), +0 and -0 tying;
     none: token 0; a non-finite top logit: the token is c_0 (weights 2^32, 0, 0, ...).
  2. t_i = (l[c_i] - l[c_0]) / T in f32, w_i = expf(t_i), q_i = floor(w_i 2^32), Q_j = q_0 + ... + q_j.
  3. top_p < 1: thr = trunc(double(top_p) double(Q_last)), n = the smallest count >= 1 with Q_{n-1} >= thr; else K'.
  4. z = splitmix64(seed + (pos + 1) 0x9E3779B97F4A7C15), u = z >> 40, r = (u Q_{n-1}) >> 24, the token is c_j for
     the smallest j with Q_j > r.

CPU tests check the rule itself (statistics, the temperature limit); GPU tests check the kernels against it bit
for bit at the op level, then the decode loop against a host loop of forward() + ref_sample.
"""
import ctypes
import math

import numpy as np
import pytest

_libm = ctypes.CDLL("libm.so.6")
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]
M64 = (1 << 64) - 1
MAX_K = 256


def ref_candidates(logits, top_k):
    l = np.asarray(logits, np.float32)
    K = MAX_K if top_k == 0 else top_k
    ids = np.nonzero(~np.isnan(l))[0]
    order = np.lexsort((ids, -l[ids]))  # primary: logit descending (IEEE compare: +0 == -0), then id ascending
    return ids[order][:K].astype(np.int64)


def ref_weights(logits, cand, T):
    l = np.asarray(logits, np.float32)
    if len(cand) == 0:
        return []
    l0 = l[cand[0]]
    if not np.isfinite(l0):
        return [1 << 32] + [0] * (len(cand) - 1)
    with np.errstate(all="ignore"):
        t = (l[cand] - l0) / np.float32(T)  # one f32 subtraction, one f32 division
    assert t.dtype == np.float32
    return [int(math.floor(float(_libm.expf(float(x))) * 4294967296.0)) for x in t]


def ref_nucleus(q, top_p):
    Q = np.cumsum(np.array(q, dtype=object)).tolist() if q else []
    if not Q:
        return Q, 0
    n = len(Q)
    if np.float32(top_p) < 1:
        thr = int(float(np.float32(top_p)) * float(Q[-1]))
        n = next(i + 1 for i, v in enumerate(Q) if v >= thr)
    return Q, n


def ref_draw(Q, n, seed, pos):
    z = (seed + (pos + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    u = z >> 40
    r = (u * Q[n - 1]) >> 24
    return next(j for j in range(n) if Q[j] > r)


def ref_sample(logits, T, top_k, top_p, seed, pos):
    cand = ref_candidates(logits, top_k)
    if len(cand) == 0:
        return 0
    Q, n = ref_nucleus(ref_weights(logits, cand, T), top_p)
    return int(cand[ref_draw(Q, n, seed, pos)])


# ---------------------------------------------------------------------------------------------------------------
# CPU: the rule
# ---------------------------------------------------------------------------------------------------------------
def test_reference_statistics():
    """20,000 positions at the model card's parameters: every nucleus token's count within 5 sigma of N q_i / Q,
    nothing drawn outside the nucleus."""
    V, N = 4099, 20000
    l = (np.random.default_rng(11).standard_normal(V) * 3).astype(np.float32)
    cand = ref_candidates(l, 64)
    q = ref_weights(l, cand, 1.0)
    Q, n = ref_nucleus(q, 0.95)
    assert 1 < n <= 64
    counts = np.zeros(len(cand), np.int64)
    for pos in range(N):
        counts[ref_draw(Q, n, 0x5EED, pos)] += 1
    assert counts[n:].sum() == 0
    p = np.array([q[i] / Q[n - 1] for i in range(n)], np.float64)
    z = (counts[:n] - N * p) / np.sqrt(N * p * (1 - p))
    print(f"nucleus {n} tokens, largest |z| {np.abs(z).max():.2f}")
    assert np.abs(z).max() < 5.0
    # and the whole function agrees with its parts
    assert ref_sample(l, 1.0, 64, 0.95, 0x5EED, 17) == int(cand[ref_draw(Q, n, 0x5EED, 17)])


def test_reference_temperature_limit():
    l = (np.random.default_rng(12).standard_normal(4099) * 3).astype(np.float32)
    for pos in range(64):
        assert ref_sample(l, 1e-3, 0, 1.0, 3, pos) == int(np.argmax(l))


def test_reference_single_token():
    for pos in range(8):
        assert ref_sample(np.array([-2.5], np.float32), 1.0, 64, 0.95, 9, pos) == 0


# ---------------------------------------------------------------------------------------------------------------
# GPU: the kernels at the op level
# ---------------------------------------------------------------------------------------------------------------
PARAMS = [(1.0, 64, 0.95), (0.7, 40, 1.0), (1.5, 0, 0.5), (1e-3, 256, 1.0), (100.0, 256, 1e-6), (1.0, 1, 1.0)]


def _check_against_ref(l, T, k, p, seed, positions):
    from llm_inference_amd import ops
    cand = ref_candidates(l, k)
    q = ref_weights(l, cand, T)
    Q, n = ref_nucleus(q, p)
    for pos in positions:
        tok, dc, dq, dn = ops.sample_logits(l, pos, T, k, p, seed, details=True)
        assert dc.tolist() == cand.tolist(), (T, k, p, pos)
        assert [int(x) for x in dq] == q, (T, k, p, pos)
        assert dn == n, (T, k, p, pos)
        want = int(cand[ref_draw(Q, n, seed, pos)]) if len(cand) else 0
        assert tok == want, (T, k, p, pos)
    return cand, q, n


@pytest.mark.gpu
@pytest.mark.parametrize("V", [1, 5, 255, 256, 257, 4099, 262144])
def test_sample_logits_matches_reference(V):
    l = (np.random.default_rng(100 + V % 97).standard_normal(V) * 3).astype(np.float32)
    for i, (T, k, p) in enumerate(PARAMS):
        _check_against_ref(l, T, k, p, 0xC0FFEE + i, range(32))


@pytest.mark.gpu
@pytest.mark.parametrize("V", [262208, 524289])
def test_sample_logits_long_rows(V):
    """Past 262,144 logits the selection takes 8, then (past 524,288) 16 logits per thread: Gemma-3 4B's own
    262,208-row vocabulary, and the first row length of the widest form."""
    l = (np.random.default_rng(V % 89).standard_normal(V) * 3).astype(np.float32)
    _check_against_ref(l, 1.0, 64, 0.95, 21, range(4))
    _check_against_ref(l, 1.5, 0, 0.5, 22, range(2))


@pytest.mark.gpu
def test_sample_logits_edge_logits():
    from llm_inference_amd import ops
    V = 4099
    rng = np.random.default_rng(5)
    base = (rng.standard_normal(V) * 3).astype(np.float32)
    pos4 = range(4)
    # all equal: the ids decide
    l = np.full(V, 1.25, np.float32)
    cand, _, _ = _check_against_ref(l, 1.0, 0, 1.0, 1, pos4)
    assert cand.tolist() == list(range(256))
    # every value twice, V / 2 apart
    l = base.copy()
    h = V // 2
    l[h:2 * h] = l[:h]
    cand, _, _ = _check_against_ref(l, 1.0, 0, 0.95, 2, pos4)
    assert cand[1] == cand[0] + h  # the top value's twin follows it
    # a block of -inf (and fewer finite logits than top_k)
    l = base.copy()
    l[100:4000] = -np.inf
    _check_against_ref(l, 1.0, 0, 0.95, 3, pos4)
    _check_against_ref(l, 0.7, 64, 1.0, 3, pos4)
    # +0 / -0 at the top: a tie, the lower id first
    l = -np.abs(base) - 1
    l[300], l[200] = 0.0, -0.0
    cand, _, _ = _check_against_ref(l, 1.0, 64, 1.0, 4, pos4)
    assert cand[:2].tolist() == [200, 300]
    # scattered NaNs are never candidates
    l = base.copy()
    nan = rng.choice(V, 1500, replace=False)
    l[nan] = np.nan
    l[int(np.nanargmax(l)) ^ 1] = np.nan
    cand, _, _ = _check_against_ref(l, 1.0, 0, 1.0, 5, pos4)
    assert not set(cand.tolist()) & set(np.nonzero(np.isnan(l))[0].tolist())
    # fewer non-NaN logits than top_k
    l = np.full(V, np.nan, np.float32)
    l[[7, 4098, 1024]] = [1.0, 2.0, 1.0]
    cand, _, _ = _check_against_ref(l, 1.0, 64, 1.0, 6, pos4)
    assert cand.tolist() == [4098, 7, 1024]
    # all NaN: token 0
    tok, dc, dq, dn = ops.sample_logits(np.full(V, np.nan, np.float32), 3, 1.0, 64, 0.95, 7, details=True)
    assert (tok, len(dc), dn) == (0, 0, 0)
    # top logit +inf: the token is c_0
    l = base.copy()
    l[[77, 1234]] = np.inf
    for pos in range(8):
        assert ops.sample_logits(l, pos, 1.0, 64, 0.95, 8) == 77
    _check_against_ref(l, 1.0, 64, 0.95, 8, pos4)


@pytest.mark.gpu
def test_sample_logits_threshold_of_zero_prefix():
    """A work-group that takes all its keys down to -inf (or a finite logit <= -2^127) selects with a threshold key
    of 0: fewer non-NaN logits than top_k in the row, or in a ragged last chunk of the selection."""
    inf = np.inf
    for row in ([-inf, -1.0], [1.0, 2.0, -inf, 0.5, 3.0], [1.0, -3e38], [-inf, -inf], [-3e38, -3.2e38, -inf]):
        l = np.array(row, np.float32)
        _check_against_ref(l, 1.0, 64, 0.95, 31, range(8))
        _check_against_ref(l, 0.7, 0, 1.0, 32, range(4))
    l = np.array([-inf, -1.0], np.float32)
    assert _check_against_ref(l, 1.0, 64, 1.0, 33, range(4))[0].tolist() == [1, 0]
    # V = 4099: the last chunk is ids 4096..4098; the row maximum sits there beside a -inf
    base = (np.random.default_rng(6).standard_normal(4099) * 3).astype(np.float32)
    l = base.copy()
    l[4097], l[4098] = 50.0, -inf
    for k in (1, 64, 0):
        cand, _, _ = _check_against_ref(l, 1.0, k, 0.95, 34, range(4))
        assert cand[0] == 4097
    l[4096] = -3e38
    _check_against_ref(l, 1.0, 64, 1.0, 35, range(4))
    # Gemma-3 4B's 262,208 rows at k = 64: a last chunk of 64 ids, all taken, one of them -inf
    l = (np.random.default_rng(7).standard_normal(262208) * 3).astype(np.float32)
    l[262150], l[262200] = 40.0, -inf
    cand, _, _ = _check_against_ref(l, 1.0, 64, 0.95, 36, range(4))
    assert cand[0] == 262150


@pytest.mark.gpu
def test_sample_logits_errors():
    from llm_inference_amd import ops
    from llm_inference_amd._lib import LLMIError
    l = np.zeros(16, np.float32)
    for kw, field in [(dict(temperature=-1.0), "temperature"), (dict(temperature=float("nan")), "temperature"),
                      (dict(temperature=1.0, top_k=-1), "top_k"), (dict(temperature=1.0, top_k=257), "top_k"),
                      (dict(temperature=1.0, top_p=0.0), "top_p"), (dict(temperature=1.0, top_p=1.5), "top_p"),
                      (dict(temperature=1.0, top_p=float("nan")), "top_p")]:
        with pytest.raises(LLMIError) as e:
            ops.sample_logits(l, 0, **kw)
        assert e.value.status == "E_ARG" and field in str(e.value), (kw, str(e.value))


# ---------------------------------------------------------------------------------------------------------------
# GPU: the decode loop
# ---------------------------------------------------------------------------------------------------------------
LOOP_T = 24.0  # see test_decode_loop_matches_host_loop
SAMPLER = dict(temperature=LOOP_T, top_k=64, top_p=0.95, seed=7)


def _gguf(cfg_name, seed):
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    cfg = CONFIGS[cfg_name]
    return cfg, build_gemma3_gguf(cfg, seed=seed)


def _start(m, cfg, seed):
    prompt = np.random.default_rng(seed).integers(4, cfg.vocab, 9).astype(np.int32)
    lg = m.forward(prompt, 0)
    return int(np.argmax(lg)), len(prompt)


def _host_loop(m, first, pos, steps, sp):
    ids, greedy, tok = [], [], first
    for i in range(steps):
        lg = m.forward(np.array([tok], np.int32), pos + i)
        tok = ref_sample(lg, sp["temperature"], sp["top_k"], sp["top_p"], sp["seed"], pos + i)
        ids.append(tok)
        greedy.append(int(np.argmax(lg)))
    return ids, greedy


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("cfg_name", ["mini-1b", "mini-4b"])
def test_decode_loop_matches_host_loop(cfg_name, exact):
    """48 sampled steps on the device against forward() + ref_sample on a second session of the same kind.
    Temperature LOOP_T = 24: the synthetic models' logits are peaked (the oracle's, seed 13, the prompt below: top
    logit ~25 against ~6 for mini-1b, ~85 against ~9 for mini-4b), so at T = 1 and T = 8 the reference sampler alone
    never left mini-4b's arg-max in 48 steps (mini-1b: 0 and 40), at T = 16 in 14 steps (47), at T = 24 in 33 (47),
    at T = 32 in 40 (48).  24 is the first value with a margin over the required quarter (12) on both models."""
    from llm_inference_amd.model import Model
    cfg, g = _gguf(cfg_name, 13)
    host = Model(g, max_ctx=128, exact=exact)
    first, pos = _start(host, cfg, 2)
    want, greedy = _host_loop(host, first, pos, 48, SAMPLER)
    host.close()
    off = sum(a != b for a, b in zip(want, greedy))
    print(f"{cfg_name} exact={exact}: {off} of 48 steps leave the arg-max")
    assert off >= 12
    m = Model(g, max_ctx=128, exact=exact)
    assert _start(m, cfg, 2) == (first, pos)
    m.set_sampler(**SAMPLER)
    assert m.get_info().sampling == 1
    got = m.generate(first, pos, 48)
    assert got.tolist() == want
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("case", ["vocab4100", "softcap"])
def test_decode_loop_ragged_vocab_and_final_softcap(case, exact):
    """The sampled step with two select work-groups (a 4100-row vocabulary: ids 4096..4099 are a ragged second
    chunk) and on a model with attention.final_logit_softcapping (the logits GEMV without a folded arg-max key,
    then the soft-cap launch, then the sampler), against the host loop.  Same temperature as above."""
    import dataclasses
    from llm_inference_amd.model import Model
    from llm_inference_amd.synthetic import CONFIGS, build_gemma3_gguf
    if case == "vocab4100":
        cfg = dataclasses.replace(CONFIGS["mini-1b"], vocab=4100)
        g = build_gemma3_gguf(cfg, seed=13)
    else:
        cfg = CONFIGS["mini-1b"]
        g = build_gemma3_gguf(cfg, seed=13, extra_meta={"attention.final_logit_softcapping": 30.0})
    host = Model(g, max_ctx=128, exact=exact)
    first, pos = _start(host, cfg, 2)
    want, greedy = _host_loop(host, first, pos, 32, SAMPLER)
    host.close()
    off = sum(a != b for a, b in zip(want, greedy))
    print(f"{case} exact={exact}: {off} of 32 steps leave the arg-max")
    assert off >= 8
    m = Model(g, max_ctx=128, exact=exact)
    assert _start(m, cfg, 2) == (first, pos)
    m.set_sampler(**SAMPLER)
    assert m.generate(first, pos, 32).tolist() == want
    m.close()


@pytest.mark.gpu
def test_seed_chunking_and_no_graph():
    from llm_inference_amd.model import Model
    cfg, g = _gguf("mini-1b", 13)
    m = Model(g, max_ctx=128)
    first, pos = _start(m, cfg, 3)
    a = m.generate(first, pos, 16, sampler=SAMPLER)
    assert m.get_info().sampling == 0  # generate(sampler=...) restores the session's own
    b = m.generate(first, pos, 16, sampler=SAMPLER)
    assert a.tolist() == b.tolist()
    c = m.generate(first, pos, 16, sampler=dict(SAMPLER, seed=8))
    assert a.tolist() != c.tolist()
    m.set_sampler(**SAMPLER)
    d1 = m.generate(first, pos, 8)
    d2 = m.generate(int(d1[-1]), pos + 8, 8)
    assert d1.tolist() + d2.tolist() == a.tolist()
    m.close()
    e = Model(g, max_ctx=128, use_graph=False)
    assert _start(e, cfg, 3) == (first, pos)
    assert e.generate(first, pos, 16, sampler=SAMPLER).tolist() == a.tolist()
    e.close()


@pytest.mark.gpu
def test_top_k_1_is_greedy_and_restore():
    """top_k = 1 at any temperature is the greedy loop, ties included (test_logits_screen.py's duplicated rows: the
    lower id of each tied pair); set_sampler(None) restores the greedy step."""
    from llm_inference_amd.gguf import GGUFFile
    from llm_inference_amd.model import Model
    cfg, g = _gguf("mini-4b", 17)
    f = GGUFFile(g)
    t = f.tensor("token_embd.weight")
    s0 = f.data_section_start + t.tensor_offset
    e = g[s0:s0 + t.nbytes].view(np.float16).reshape(cfg.vocab, cfg.n_embd)
    h = cfg.vocab // 2
    e[h:2 * h] = e[:h]
    m = Model(g, max_ctx=128)
    first, pos = _start(m, cfg, 5)
    greedy = m.generate(first, pos, 32)
    kpt = m.get_info().kernels_per_token
    assert (greedy < h).all()
    for T in (0.3, 1.0, 5.0):
        m.set_sampler(temperature=T, top_k=1, top_p=0.9, seed=1)
        assert m.generate(first, pos, 32).tolist() == greedy.tolist()
    assert m.get_info().sampling == 1
    m.set_sampler(None)
    info = m.get_info()
    assert (info.sampling, info.kernels_per_token) == (0, kpt)
    assert m.generate(first, pos, 32).tolist() == greedy.tolist()
    assert m.get_info().kernels_per_token == kpt
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
def test_forward_after_sampled_generate_matches_fresh(exact):
    """test_session_state.py's pattern: a sampled decode loop (and the sampler's timing hook) leaves nothing behind."""
    from llm_inference_amd.model import Model
    cfg, g = _gguf("mini-4b", 606)
    rng = np.random.default_rng(7)
    prompt = np.concatenate([[2], rng.integers(4, cfg.vocab, 39)]).astype(np.int32)
    forced = rng.integers(4, cfg.vocab, 4).astype(np.int32)

    def parity(m):
        out = [m.forward(prompt, 0)]
        for i, t in enumerate(forced):
            out.append(m.forward(np.array([t], np.int32), len(prompt) + i))
        return np.stack(out), m.last_argmax

    fresh = Model(g, max_ctx=256, exact=exact)
    want, want_am = parity(fresh)
    fresh.close()
    m = Model(g, max_ctx=256, exact=exact)
    m.forward(prompt, 0, want_logits=False)
    m.set_sampler(**SAMPLER)
    m.generate(m.last_argmax, len(prompt), 24)
    us, by = m.time_kernel(8, 2)
    assert us > 0 and by == cfg.vocab * 4
    got, got_am = parity(m)  # forward ignores the sampler: the logits and the greedy arg-max
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got_am == want_am == int(np.argmax(want[-1]))
    m.close()


@pytest.mark.gpu
def test_sampler_errors():
    import threading
    from llm_inference_amd._lib import LLMIError
    from llm_inference_amd.model import Model, TPGroup
    cfg, g = _gguf("mini-1b", 13)
    m = Model(g, max_ctx=64)
    for kw, field in [(dict(temperature=-0.5), "temperature"), (dict(temperature=float("nan")), "temperature"),
                      (dict(temperature=1.0, top_k=-3), "top_k"), (dict(temperature=1.0, top_k=300), "top_k"),
                      (dict(temperature=1.0, top_p=0.0), "top_p"), (dict(temperature=1.0, top_p=1.01), "top_p"),
                      (dict(temperature=1.0, top_p=float("nan")), "top_p")]:
        with pytest.raises(LLMIError) as e:
            m.set_sampler(**kw)
        assert e.value.status == "E_ARG" and field in str(e.value), (kw, str(e.value))
    assert m.get_info().sampling == 0
    m.set_sampler(temperature=0.0)  # 0: greedy
    assert m.get_info().sampling == 0
    m.close()
    # a tensor-parallel session refuses a sampler
    grp = TPGroup(2)
    res = [None, None]

    def rank(r):
        try:
            t = Model(g, max_ctx=64, tp_rank=r, tp_size=2, tp_group=grp)
            try:
                t.set_sampler(**SAMPLER)
                res[r] = "accepted"
            except LLMIError as e:
                res[r] = (e.status, str(e))
            t.close()
        except Exception as e:  # noqa: BLE001 -- reported below
            res[r] = repr(e)

    th = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    grp.close()
    for r in res:
        assert isinstance(r, tuple) and r[0] == "E_ARG" and "tensor-parallel" in r[1], res
