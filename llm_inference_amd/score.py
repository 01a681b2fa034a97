"""Result of teacher-forced scoring (Model.score / ops.score_rows; include/llmi.h llmi_session_score)."""
from __future__ import annotations

import math

import numpy as np


class ScoreResult:
    """Per position i: logprobs[i] = log p(targets[i] | tokens[:i + 1]) (0.0 where the position has no target),
    lse[i] = log sum_v exp(logit_i[v]), argmax[i] = the greedy id (first maximal index).  targets holds the ids
    that were scored, -1 = none."""

    def __init__(self, logprobs, lse, argmax, targets):
        self.logprobs = np.asarray(logprobs, np.float32)
        self.lse = np.asarray(lse, np.float32)
        self.argmax = np.asarray(argmax, np.int32)
        self.targets = np.asarray(targets, np.int32)

    @property
    def count(self) -> int:
        """Positions with a target."""
        return int((self.targets >= 0).sum())

    @property
    def nll(self) -> float:
        """-sum of logprobs over the positions with a target, summed in float64."""
        return float(-self.logprobs[self.targets >= 0].astype(np.float64).sum())

    @property
    def perplexity(self) -> float:
        """exp(nll / count); nan when no position has a target."""
        n = self.count
        return math.exp(self.nll / n) if n else float("nan")


def resolve_targets(tokens: np.ndarray, targets) -> np.ndarray:
    """llmi_session_score's rule for targets == NULL: the next token, the last position has none."""
    if targets is not None:
        t = np.ascontiguousarray(targets, np.int32)
        if t.shape != tokens.shape:
            raise ValueError("targets must have one id per token (-1: no target)")
        return t
    return np.concatenate([tokens[1:], [-1]]).astype(np.int32)
