"""Python mirror of the reference's Model (model.h:72-153) backed by the
device session of include/llmi.h.

    m = Model(gguf_bytes)                 # Model(GGUFFile&)  model.cpp:13-56
    logits = m.forward([tok, ...], pos)   # Model::forward     model.cpp:706-1049
    ids = m.generate(first, pos, n)       # main.cpp:172-224 greedy loop, on device
    m.set_sampler(temperature=1.0, top_k=64, top_p=0.95, seed=1)   # ... or seeded sampling in the same loop
    m.reserve_sequences(8)                # KV slots: several sequences per step
    ids = m.batch_generate(firsts, slots, positions, n)   # int32 [n, B], greedy, on device
    ids = m.batch_generate(firsts, slots, positions, n, samplers=dict(temperature=1.0, top_k=64, seed=1))  # sampled
    last = m.prefill_sequences(prompts, slots)            # prompts straight into their slots
    r = m.batch_extend([chunk, [tok], drafts], [0, 1, 2], [128, 40, 64], out=["none", "last", "all"])  # a ragged step
    r = m.batch_generate_lookup(histories, slots, positions, max_new=64)   # greedy ids, n-gram drafts (section 15)
    r = m.batch_generate_lookup_sampled(histories, slots, positions, 64, samplers=dict(temperature=0.7, seed=1))  # (16)
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence

import numpy as np

from ._lib import (BATCH_TOKENS_MAX, LLMI_EXACT, LLMI_EXACT_KQ, LLMI_NO_GRAPH, LLMI_TP_PEER, PEER_HANDLE_BYTES, SPAN_ALL,
                   SPAN_LAST, SPAN_NONE, TP_ID_BYTES, TRACE_FN, Lookup, LookupStats, Sampler, SessionInfo, SessionOpts,
                   Span, check, lib, ptr)
from .gguf import GGUFFile
from .score import ScoreResult, resolve_targets


def tp_unique_id() -> bytes:
    """A new RCCL communicator id (rank 0 makes it and sends it to the others)."""
    b = C.create_string_buffer(TP_ID_BYTES)
    check(lib().llmi_tp_unique_id(b))
    return b.raw


class TPGroup:
    """Ranks of one tensor-parallel group sharing ONE device (tests: RCCL
    refuses two ranks per GPU).  Each rank's session is driven by its own
    host thread; the all-gathers are the push exchange split around host
    barriers (LLMI_TP_EXCHANGE=copy: device-to-device copies)."""

    def __init__(self, size: int):
        h = C.c_void_p()
        check(lib().llmi_tp_group_create(size, C.byref(h)))
        self.h = h
        self.size = size

    def close(self):
        if getattr(self, "h", None):
            lib().llmi_tp_group_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


SAMPLER_KEYS = ("temperature", "top_k", "top_p", "seed")  # Model.set_sampler's keywords


def normalize_samplers(samplers, B: int):
    """Model.batch_generate's `samplers` argument as None (the greedy call) or a list of B entries, each None (a
    greedy row) or a dict with every one of set_sampler's keywords (its defaults filled in).  One dict applies to
    every row; a sequence must have B entries (ValueError otherwise, as for an unknown keyword or no temperature)."""
    if samplers is None:
        return None

    def one(sp):
        if sp is None:
            return None
        if not isinstance(sp, dict):
            raise ValueError("samplers: each entry is a dict of set_sampler's keywords or None")
        extra = set(sp) - set(SAMPLER_KEYS)
        if extra:
            raise ValueError(f"samplers: unknown keyword(s) {sorted(extra)}")
        if sp.get("temperature") is None:
            raise ValueError("samplers: a sampler needs a temperature (None entry: a greedy row)")
        return dict(temperature=float(sp["temperature"]), top_k=int(sp.get("top_k", 0)),
                    top_p=float(sp.get("top_p", 1.0)), seed=int(sp.get("seed", 0)))

    if isinstance(samplers, dict):
        return [one(samplers) for _ in range(B)]
    sps = [one(sp) for sp in samplers]
    if len(sps) != B:
        raise ValueError(f"samplers: {len(sps)} entries for {B} rows")
    return sps


def marshal_samplers(sps):
    """normalize_samplers' list as the ctypes array of llmi_sampler the batch calls take: a None entry (a greedy row)
    becomes temperature 0, a seed is reduced to 64 bits."""
    arr = (Sampler * max(len(sps), 1))()
    for b, sp in enumerate(sps):
        arr[b] = Sampler(0.0, 0, 1.0, 0) if sp is None else Sampler(sp["temperature"], sp["top_k"], sp["top_p"],
                                                                   sp["seed"] & 0xFFFFFFFFFFFFFFFF)
    return arr


@dataclass
class BatchResult:
    """Model.batch_forward: per row the greedy id, the log-sum-exp of its logits and (want_logits) the logits."""
    argmax: np.ndarray            # int32 [B]
    lse: np.ndarray               # float32 [B]
    logits: Optional[np.ndarray]  # float32 [B, vocab] or None


@dataclass
class ExtendResult:
    """Model.batch_extend: the output rows compacted in span order -- span i's are [offsets[i], offsets[i + 1])."""
    argmax: np.ndarray            # int32 [n_out]
    lse: np.ndarray               # float32 [n_out]
    logits: Optional[np.ndarray]  # float32 [n_out, vocab] or None
    offsets: np.ndarray           # int64 [n_spans + 1]


@dataclass
class LookupResult:
    """Model.batch_generate_lookup: per row the ids it emitted (batch_generate's, cut after a stop id); the steps in
    which some row was live; per row the draft tokens run and the ids emitted past the first of each step."""
    ids: list                     # B int32 arrays
    steps: int
    drafted: np.ndarray           # int32 [B]
    accepted: np.ndarray          # int32 [B]


def marshal_lookup(histories, slots, pos):
    """Model.batch_generate_lookup's rows as llmi_session_batch_generate_lookup takes them: (the histories
    concatenated int32, hist_len int32 [B], slots int32 [B], pos int32 [B])."""
    hs = [np.ascontiguousarray(x, np.int32).reshape(-1) for x in histories]
    sl, p = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (slots, pos))
    if not (len(hs) == sl.size == p.size):
        raise ValueError("histories, slots and pos must have one entry per row")
    hl = np.array([x.size for x in hs], np.int32)
    tokens = np.concatenate(hs).astype(np.int32) if hs else np.zeros(0, np.int32)
    return tokens, hl, sl, p


SPAN_OUT = {"last": SPAN_LAST, "all": SPAN_ALL, "none": SPAN_NONE}


def marshal_extend(seqs, slots, pos, out="last"):
    """Model.batch_extend's arguments as llmi_session_batch_extend takes them: (tokens int32 -- the spans' tokens
    concatenated, a ctypes array of Span, offsets int64 [n_spans + 1] of the spans' output rows).  out: one of
    "last" | "all" | "none", or one value per span."""
    seqs = [np.ascontiguousarray(x, np.int32).reshape(-1) for x in seqs]
    sl, p = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (slots, pos))
    outs = [out] * len(seqs) if isinstance(out, str) else list(out)
    if not (len(seqs) == sl.size == p.size == len(outs)):
        raise ValueError("seqs, slots, pos and (as a sequence) out must have one entry per span")
    for o in outs:
        if o not in SPAN_OUT:
            raise ValueError(f"out: {o!r} is none of 'last', 'all', 'none'")
    arr = (Span * max(len(seqs), 1))()
    offsets = np.zeros(len(seqs) + 1, np.int64)
    for i, (x, o) in enumerate(zip(seqs, outs)):
        arr[i] = Span(int(sl[i]), int(p[i]), x.size, SPAN_OUT[o])
        offsets[i + 1] = offsets[i] + (x.size if o == "all" else 1 if o == "last" else 0)
    tokens = np.concatenate(seqs).astype(np.int32) if seqs else np.zeros(0, np.int32)
    return tokens, arr, offsets


class PlannedSpan(NamedTuple):
    """One span of plan_extend_calls: tokens [start, start + n_tokens) of prompt `prompt`, at positions pos .. of its
    slot; out "last" for the prompt's final span, "none" for every other."""
    prompt: int
    slot: int
    pos: int
    start: int
    n_tokens: int
    out: str


def plan_extend_calls(lengths, slots, pos=0, max_tokens=BATCH_TOKENS_MAX):
    """Model.prefill_sequences' plan: prompts of `lengths` tokens, prompt i into slot slots[i] from position pos (one
    int, or one per prompt), as a list of batch_extend calls, each a list of PlannedSpan.  A call carries at most
    max_tokens token rows and a slot at most once; a long prompt is cut into consecutive spans across calls, short
    ones share a call; in prompt order.  ValueError: an empty prompt, a slot given twice, a negative position."""
    lengths = [int(n) for n in lengths]
    slots = [int(s) for s in slots]
    starts = [int(pos)] * len(lengths) if np.isscalar(pos) else [int(q) for q in pos]
    if not (len(lengths) == len(slots) == len(starts)):
        raise ValueError("lengths, slots and pos must have one entry per prompt")
    if max_tokens < 1:
        raise ValueError("max_tokens must be at least 1")
    if any(n < 1 for n in lengths):
        raise ValueError("an empty prompt has no last token")
    if len(set(slots)) != len(slots):
        raise ValueError("each prompt needs a slot of its own")
    if any(q < 0 for q in starts):
        raise ValueError("negative position")
    calls, cur, room = [], [], max_tokens
    for i, n in enumerate(lengths):
        done = 0
        while done < n:
            if room == 0:
                calls.append(cur)
                cur, room = [], max_tokens
            take = min(n - done, room)
            cur.append(PlannedSpan(i, slots[i], starts[i] + done, done, take, "last" if done + take == n else "none"))
            done += take
            room -= take
    if cur:
        calls.append(cur)
    return calls


class Model:
    def __init__(self, gguf, device: int = 0, exact: bool = False, max_ctx: int = 4096,
                 use_graph: bool = True, attn_split: int = 0, tp_rank: int = 0, tp_size: int = 1,
                 tp_id: Optional[bytes] = None, tp_group: Optional["TPGroup"] = None, tp_peer: bool = False,
                 exact_kq: bool = False):
        """tp_id (RCCL, one process per GPU), tp_group (ranks on one device,
        one host thread each) or tp_peer (one process per GPU, the one-shot
        push exchange: peer_handle() / peer_connect() before the first
        forward) makes this session rank tp_rank of a row-sharded
        tensor-parallel group of tp_size (include/llmi.h).  exact_kq (with
        exact): K-quant layers run on the exact-order engine too
        (LLMI_EXACT_KQ; the environment's LLMI_EXACT_KQ=1 does the same)."""
        buf = gguf if isinstance(gguf, np.ndarray) else np.frombuffer(gguf, np.uint8)
        buf = np.ascontiguousarray(buf)
        self._tp_id = C.create_string_buffer(bytes(tp_id), TP_ID_BYTES) if tp_id is not None else None
        if tp_id is not None and len(tp_id) != TP_ID_BYTES:
            raise ValueError(f"tp_id must be {TP_ID_BYTES} bytes")
        self._tp_group = tp_group  # keep the group alive as long as the session
        flags = (LLMI_EXACT if exact else 0) | (0 if use_graph else LLMI_NO_GRAPH) | (LLMI_TP_PEER if tp_peer else 0) | \
            (LLMI_EXACT_KQ if exact_kq else 0)
        opts = SessionOpts(device, flags,
                           max_ctx, attn_split, tp_rank, tp_size,
                           C.cast(self._tp_id, C.c_void_p) if self._tp_id is not None else None,
                           tp_group.h.value if tp_group is not None else None)
        h = C.c_void_p()
        check(lib().llmi_session_create(ptr(buf), buf.size, C.byref(opts), C.byref(h)))
        self.h = h
        self.gguf = GGUFFile(buf)  # host-side metadata view (tokenizer etc.)
        self.info = self.get_info()
        self.vocab = self.info.vocab
        self._sampler = None

    def get_info(self) -> SessionInfo:
        info = SessionInfo()
        check(lib().llmi_session_get_info_sized(self.h, C.byref(info), C.sizeof(info)))
        return info

    def forward(self, tokens: Sequence[int], pos: int, want_logits: bool = True):
        t = np.ascontiguousarray(tokens, np.int32)
        lg = np.zeros(self.vocab, np.float32) if want_logits else None
        am = np.zeros(1, np.int32)
        check(lib().llmi_session_forward(self.h, ptr(t), t.size, pos, ptr(lg) if lg is not None else None, ptr(am)))
        self.last_argmax = int(am[0])
        return lg

    def dump(self, tokens: Sequence[int], pos: int, path: str) -> None:
        """llmi_session_dump: forward one token at a time, appending the
        reference's --verbose intermediates (print_tensor format) to `path`."""
        t = np.ascontiguousarray(tokens, np.int32)
        check(lib().llmi_session_dump(self.h, ptr(t), t.size, pos, path.encode()))

    def score(self, tokens: Sequence[int], pos: int = 0, targets: Optional[Sequence[int]] = None) -> ScoreResult:
        """llmi_session_score: run the tokens as forward() does and return, for every position, the log-prob of
        its target (default: the next token; -1 = none), the log-sum-exp of its logits and its greedy id
        (.logprobs / .lse / .argmax, and .nll / .perplexity over the positions with a target)."""
        t = np.ascontiguousarray(tokens, np.int32)
        tg = None if targets is None else np.ascontiguousarray(targets, np.int32)
        if tg is not None and tg.shape != t.shape:
            raise ValueError("targets must have one id per token (-1: no target)")
        lp, lse, am = np.zeros(t.size, np.float32), np.zeros(t.size, np.float32), np.zeros(t.size, np.int32)
        check(lib().llmi_session_score(self.h, ptr(t), t.size, pos, ptr(tg) if tg is not None else None,
                                       ptr(lp), ptr(lse), ptr(am)))
        self.last_argmax = int(am[-1])
        return ScoreResult(lp, lse, am, resolve_targets(t, tg))

    def perplexity(self, tokens: Sequence[int]) -> float:
        """exp(nll / count) of the tokens after the first, each scored given the ones before it."""
        return self.score(tokens).perplexity

    def trace(self, tokens: Sequence[int], pos: int, gen: bool = False, score: bool = False) -> list:
        """llmi_session_trace: run the launches forward() (or, gen=True, one
        decode-loop step; score=True: score()) performs, eagerly, and return what each launch
        produced as [(name, layer, bytes)] in launch order (op-level parity
        tests compare each against the oracle from the device's own inputs)."""
        t = np.ascontiguousarray(tokens, np.int32)
        out = []

        def cb(_user, name, layer, data, nbytes):
            out.append((name.decode(), int(layer), C.string_at(data, nbytes)))

        fn = TRACE_FN(cb)  # kept alive for the duration of the call
        check(lib().llmi_session_trace(self.h, ptr(t), t.size, pos, (1 if gen else 0) | (2 if score else 0), fn, None))
        return out

    def set_sampler(self, sampler: Optional[dict] = None, *, temperature: Optional[float] = None, top_k: int = 0,
                    top_p: float = 1.0, seed: int = 0) -> None:
        """llmi_session_set_sampler: generate / enqueue draw each token by seeded temperature / top-k / top-p
        sampling instead of taking the argmax.  set_sampler(None) (or temperature 0)
        restores greedy decoding.  A dict of the same keywords is accepted as the positional argument."""
        if sampler is not None:
            return self.set_sampler(**sampler)
        if temperature is None:
            check(lib().llmi_session_set_sampler(self.h, None))
            self._sampler = None
        else:
            sp = Sampler(temperature, top_k, top_p, seed & 0xFFFFFFFFFFFFFFFF)
            check(lib().llmi_session_set_sampler(self.h, C.byref(sp)))
            self._sampler = dict(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed) if temperature else None
        self.info = self.get_info()

    def generate(self, first: int, pos: int, n_steps: int, sampler: Optional[dict] = None) -> np.ndarray:
        """sampler (a dict of set_sampler's keywords): set for this call only, the session's own restored after."""
        out = np.zeros(max(n_steps, 1), np.int32)
        if sampler is None:
            check(lib().llmi_session_generate(self.h, first, pos, n_steps, ptr(out)))
            return out[:n_steps]
        before = self._sampler
        self.set_sampler(**sampler)
        try:
            check(lib().llmi_session_generate(self.h, first, pos, n_steps, ptr(out)))
        finally:
            self.set_sampler(before)
        return out[:n_steps]

    def reserve_sequences(self, n: int) -> None:
        """llmi_session_seq_reserve: KV slots 0..n-1 (slot 0 is the session's own cache, where forward() / score()
        leave a prompt); may be called again with a larger n."""
        check(lib().llmi_session_seq_reserve(self.h, n))
        self.info = self.get_info()

    def copy_sequence(self, dst: int, src: int, n_pos: int) -> None:
        """llmi_session_seq_copy: K/V rows [0, n_pos) of every layer, slot src -> slot dst (moves or forks a prompt)."""
        check(lib().llmi_session_seq_copy(self.h, dst, src, n_pos))

    def _batch_rows(self, tokens, slots, pos):
        t, sl, p = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (tokens, slots, pos))
        if not (t.size == sl.size == p.size):
            raise ValueError("tokens, slots and pos must have one entry per row")
        return t, sl, p

    def batch_forward(self, tokens: Sequence[int], slots: Sequence[int], pos: Sequence[int],
                      want_logits: bool = False) -> BatchResult:
        """llmi_session_batch_forward: one step for B rows -- row b runs tokens[b] at position pos[b] of slot
        slots[b].  Each row's results are, bit for bit, the last position of score() / forward() of the same prompt
        on a single-sequence session.  want_logits: [B, vocab] logits for host-side
        sampling (slow: one output-table read per row)."""
        t, sl, p = self._batch_rows(tokens, slots, pos)
        am, lse = np.zeros(t.size, np.int32), np.zeros(t.size, np.float32)
        lg = np.zeros((t.size, self.vocab), np.float32) if want_logits else None
        check(lib().llmi_session_batch_forward(self.h, ptr(t), ptr(sl), ptr(p), t.size,
                                               ptr(lg) if lg is not None else None, ptr(am), ptr(lse)))
        return BatchResult(am, lse, lg)

    def batch_extend(self, seqs, slots: Sequence[int], pos: Sequence[int], out="last",
                     want_logits: bool = False) -> ExtendResult:
        """llmi_session_batch_extend: one ragged step -- span i runs the tokens seqs[i] at positions pos[i] .. of
        slot slots[i]: a prompt chunk, one decode row or draft tokens to verify, all sharing the step's pass over
        the weights.  out ("last" | "all" | "none", or one per span) selects each span's output rows; every output
        row carries the bits of score() / forward() of the same prefix on a single-sequence session (DESIGN.md
        section 14)."""
        t, arr, offsets = marshal_extend(seqs, slots, pos, out)
        n_out = int(offsets[-1])
        am, lse = np.zeros(max(n_out, 1), np.int32), np.zeros(max(n_out, 1), np.float32)
        lg = np.zeros((n_out, self.vocab), np.float32) if want_logits and n_out else None
        check(lib().llmi_session_batch_extend(self.h, ptr(t) if t.size else None, arr, len(offsets) - 1,
                                              ptr(lg) if lg is not None else None, ptr(am) if n_out else None,
                                              ptr(lse) if n_out else None))
        if want_logits and lg is None:
            lg = np.zeros((0, self.vocab), np.float32)
        return ExtendResult(am[:n_out], lse[:n_out], lg, offsets)

    def prefill_sequences(self, prompts, slots: Sequence[int], pos=0) -> BatchResult:
        """Prompts straight into their KV slots by batch_extend calls of at most LLMI_BATCH_TOKENS_MAX token rows
        (plan_extend_calls: long prompts cut into consecutive spans across calls, short ones packed several per
        call).  Returns each prompt's last greedy id and log-sum-exp (.argmax / .lse, one entry per prompt)."""
        prompts = [np.ascontiguousarray(x, np.int32).reshape(-1) for x in prompts]
        am, lse = np.zeros(len(prompts), np.int32), np.zeros(len(prompts), np.float32)
        for call in plan_extend_calls([x.size for x in prompts], slots, pos, BATCH_TOKENS_MAX):
            r = self.batch_extend([prompts[sp.prompt][sp.start:sp.start + sp.n_tokens] for sp in call],
                                  [sp.slot for sp in call], [sp.pos for sp in call], [sp.out for sp in call])
            for i, sp in enumerate(call):
                if sp.out == "last":
                    am[sp.prompt], lse[sp.prompt] = r.argmax[r.offsets[i]], r.lse[r.offsets[i]]
        return BatchResult(am, lse, None)

    def batch_generate(self, first: Sequence[int], slots: Sequence[int], pos: Sequence[int], n_steps: int,
                       stop: Sequence[int] = (), samplers=None) -> np.ndarray:
        """llmi_session_batch_generate: the greedy loop for B rows on the device; returns int32 [n_steps, B].  A row
        that emits one of `stop` (at most 4 ids) keeps that id, then -1, and appends nothing more to its slot.
        samplers (llmi_session_batch_generate_sampled): one dict of set_sampler's keywords
        for every row, or a sequence of B dicts / None entries (None: a greedy row); each sampled row draws its ids
        by seeded temperature / top-k / top-p sampling at its own positions, inside the same device loop."""
        t, sl, p = self._batch_rows(first, slots, pos)
        st = np.ascontiguousarray(stop, np.int32).reshape(-1)
        out = np.zeros((max(n_steps, 1), max(t.size, 1)), np.int32)
        sps = normalize_samplers(samplers, t.size)
        if sps is None:
            check(lib().llmi_session_batch_generate(self.h, ptr(t), ptr(sl), ptr(p), t.size, n_steps,
                                                    ptr(st) if st.size else None, st.size, ptr(out)))
            return out[:n_steps]
        arr = (Sampler * max(len(sps), 1))()
        for b, sp in enumerate(sps):  # a greedy row: temperature 0
            arr[b] = Sampler(0.0, 0, 1.0, 0) if sp is None else Sampler(sp["temperature"], sp["top_k"], sp["top_p"],
                                                                       sp["seed"] & 0xFFFFFFFFFFFFFFFF)
        check(lib().llmi_session_batch_generate_sampled(self.h, ptr(t), ptr(sl), ptr(p), t.size, n_steps,
                                                        ptr(st) if st.size else None, st.size, arr, ptr(out)))
        return out[:n_steps]

    def batch_generate_lookup(self, histories, slots: Sequence[int], pos: Sequence[int], max_new: int,
                              draft_len: int = 7, ngram_max: int = 3, ngram_min: int = 1, stop: Sequence[int] = (),
                              max_steps: int = 0) -> LookupResult:
        """llmi_session_batch_generate_lookup: batch_generate's greedy ids with n-gram drafts verified inside the
        device loop.  histories[b]: row b's token history, whose last token runs at pos[b] of
        slot slots[b] (batch_generate's first[b]); the rest only steers the drafts.  Every step runs the current token
        and up to draft_len draft tokens per row -- the continuation of the most recent earlier occurrence of the
        history's last ngram_max..ngram_min tokens -- and emits one id plus every accepted draft.  ids[b] equals row
        b's ids of batch_generate(first, slots, pos, max_new, stop), cut after its stop id; max_steps (0: max_new)
        bounds the steps."""
        tokens, hl, sl, p = marshal_lookup(histories, slots, pos)
        st = np.ascontiguousarray(stop, np.int32).reshape(-1)
        B = hl.size
        out = np.full((max(B, 1), max(int(max_new), 1)), -1, np.int32)
        n_out = np.zeros(max(B, 1), np.int32)
        lk = Lookup(int(draft_len), int(ngram_max), int(ngram_min), int(max_new))
        stats = LookupStats()
        check(lib().llmi_session_batch_generate_lookup(self.h, ptr(tokens) if tokens.size else None, ptr(hl), ptr(sl),
                                                       ptr(p), B, C.byref(lk), int(max_steps),
                                                       ptr(st) if st.size else None, st.size, ptr(out), ptr(n_out),
                                                       C.byref(stats)))
        return LookupResult([out[b, :n_out[b]].copy() for b in range(B)], int(stats.steps),
                            np.array(stats.drafted[:B], np.int32), np.array(stats.accepted[:B], np.int32))

    def batch_generate_lookup_sampled(self, histories, slots: Sequence[int], pos: Sequence[int], max_new: int,
                                      samplers, draft_len: int = 7, ngram_max: int = 3, ngram_min: int = 1,
                                      stop: Sequence[int] = (), max_steps: int = 0) -> LookupResult:
        """llmi_session_batch_generate_lookup_sampled: batch_generate_lookup for sampled rows.
        samplers as in batch_generate: one dict of set_sampler's keywords for every row, or a sequence of B dicts /
        None entries (None: a greedy row).  A draft token is accepted when it equals the row's seeded draw at that
        token's own position, so ids[b] equals row b's ids of batch_generate(first, slots, pos, max_new, stop,
        samplers=samplers), cut after its stop id -- bit for bit, whatever the histories and draft_len."""
        tokens, hl, sl, p = marshal_lookup(histories, slots, pos)
        st = np.ascontiguousarray(stop, np.int32).reshape(-1)
        B = hl.size
        if samplers is None:
            raise ValueError("samplers: None (batch_generate_lookup is the greedy call)")
        arr = marshal_samplers(normalize_samplers(samplers, B))
        out = np.full((max(B, 1), max(int(max_new), 1)), -1, np.int32)
        n_out = np.zeros(max(B, 1), np.int32)
        lk = Lookup(int(draft_len), int(ngram_max), int(ngram_min), int(max_new))
        stats = LookupStats()
        check(lib().llmi_session_batch_generate_lookup_sampled(
            self.h, ptr(tokens) if tokens.size else None, ptr(hl), ptr(sl), ptr(p), B, C.byref(lk), int(max_steps),
            ptr(st) if st.size else None, st.size, arr, ptr(out), ptr(n_out), C.byref(stats)))
        return LookupResult([out[b, :n_out[b]].copy() for b in range(B)], int(stats.steps),
                            np.array(stats.drafted[:B], np.int32), np.array(stats.accepted[:B], np.int32))

    def enqueue(self, first: int, pos: int, n_steps: int) -> None:
        check(lib().llmi_session_enqueue(self.h, first, pos, n_steps))

    def sync(self, n: int = 0) -> Optional[np.ndarray]:
        out = np.zeros(max(n, 1), np.int32)
        check(lib().llmi_session_sync(self.h, ptr(out) if n else None, n))
        return out[:n] if n else None

    def peer_handle(self) -> bytes:
        """This rank's push-exchange mailbox handle (LLMI_PEER_HANDLE_BYTES)."""
        b = C.create_string_buffer(PEER_HANDLE_BYTES)
        check(lib().llmi_session_peer_handle(self.h, b))
        return b.raw

    def peer_connect(self, handles: Sequence[bytes]) -> None:
        """Every rank's peer_handle(), in rank order."""
        if len(handles) != self.info.tp_size or any(len(h) != PEER_HANDLE_BYTES for h in handles):
            raise ValueError(f"need {self.info.tp_size} handles of {PEER_HANDLE_BYTES} bytes")
        b = C.create_string_buffer(b"".join(handles), PEER_HANDLE_BYTES * len(handles))
        check(lib().llmi_session_peer_connect(self.h, b))

    def time_kernel(self, which: int, reps: int):
        us, by = C.c_double(), C.c_double()
        check(lib().llmi_session_time_kernel(self.h, which, reps, C.byref(us), C.byref(by)))
        return us.value, by.value

    def close(self):
        if getattr(self, "h", None):
            lib().llmi_session_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()
