"""Float64 oracle of the CTC forced alignment and transcript scoring (test helper, not a test module).

Blank 0, target y of U tokens, extended target e[2 u + 1] = y[u], e[even] = 0, S = 2 U + 1 states.  State s at frame t is entered from s,
s - 1 and - when s is odd and e[s] != e[s - 2] - s - 2; the path starts in state 0 or 1 and ends in S - 1 or S - 2.  ``forward`` sums the
paths (log-sum-exp), ``viterbi`` takes the best one with the smaller step winning ties (stay, +1, +2) and the end state S - 1 winning when
v[S - 1] >= v[S - 2].  ``check_path`` tells whether a frame -> target-index labelling is a path of this trellis.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from ctc_beam_ref import brute_force, ctc_log_prob, logp64, lse  # noqa: F401  (re-exported for the tests)

NEG = -np.inf


def _trellis(lp, length, y):
    lp = np.asarray(lp, dtype=np.float64)
    length = lp.shape[0] if length is None else max(0, min(int(length), lp.shape[0]))
    y = [int(c) for c in y]
    ext = np.zeros(2 * len(y) + 1, dtype=np.int64)
    ext[1::2] = y
    skip = np.zeros(len(ext), dtype=bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    return lp, length, y, ext, skip


def status_of(length: int, y, vocab: int) -> int:
    """0 ok, 2 a token outside 1 .. vocab - 1, 1 fewer frames than tokens + adjacent equal pairs."""
    y = [int(c) for c in y]
    if any(c < 1 or c >= vocab for c in y):
        return 2
    return 1 if length < len(y) + sum(a == b for a, b in zip(y[:-1], y[1:])) else 0


def _shift(a, k):
    return np.concatenate([np.full(k, NEG), a])[:len(a)]


def forward(lp, length: Optional[int], y) -> float:
    """log P(y | lp[:length]): the CTC forward algorithm in float64 (-inf when no path exists)."""
    lp, length, y, ext, skip = _trellis(lp, length, y)
    a = np.full(len(ext), NEG)
    a[0] = 0.0                                     # the virtual frame -1: state 0
    for t in range(length):
        a = lse(lse(a, _shift(a, 1)), np.where(skip, _shift(a, 2), NEG)) + lp[t, ext]
    if length == 0:
        return 0.0 if not y else NEG
    return float(lse(a[-1], a[-2])) if len(a) > 1 else float(a[-1])


def viterbi(lp, length: Optional[int], y) -> Dict:
    """-> score (float64), states (length,) the best path, frame_token (length,) target index or -1, margin: the smallest difference
    between the chosen and the best other finite predecessor along the path (and between the two end states; inf: nothing to decide)."""
    lp, length, y, ext, skip = _trellis(lp, length, y)
    n = len(ext)
    v = np.full(n, NEG)
    v[0] = 0.0
    back = np.zeros((length, n), dtype=np.int8)
    gaps = np.zeros((length, n), dtype=np.float32)          # chosen predecessor minus the best other finite one (inf: none)
    for t in range(length):
        c = np.stack([v, _shift(v, 1), np.where(skip, _shift(v, 2), NEG)])
        best, step = c[0].copy(), np.zeros(n, dtype=np.int8)
        for k in (1, 2):                           # strict >: the smaller step wins ties
            m = c[k] > best
            best[m], step[m] = c[k][m], k
        c[step, np.arange(n)] = NEG
        other = c.max(axis=0)
        with np.errstate(invalid="ignore"):
            gaps[t] = np.where(np.isfinite(other) & np.isfinite(best), best - other, np.inf)
        back[t] = step
        v = best + lp[t, ext]
    if length == 0:
        return {"score": 0.0 if not y else NEG, "states": np.zeros(0, dtype=np.int64), "frame_token": np.zeros(0, dtype=np.int64), "margin": np.inf}
    s = n - 1
    margin = np.inf
    if n > 1:
        if v[n - 2] > v[n - 1]:
            s = n - 2
        if np.isfinite(v[n - 1]) and np.isfinite(v[n - 2]):
            margin = abs(v[n - 1] - v[n - 2])
    score = float(v[s])
    states = np.zeros(length, dtype=np.int64)
    for t in range(length - 1, -1, -1):
        states[t] = s
        margin = min(margin, float(gaps[t, s]))
        s -= int(back[t, s])
    return {"score": score, "states": states, "frame_token": np.where(states % 2 == 1, states // 2, -1), "margin": float(margin)}


def check_path(frame_token, y) -> Optional[str]:
    """None when frame_token (target index per frame, -1 = blank) is a path of y's trellis, else what is wrong with it."""
    ft = [int(c) for c in frame_token]
    y = [int(c) for c in y]
    n = 2 * len(y) + 1
    if not ft:
        return None if not y else "no frames"
    # blanks carry no state of their own: a blank after token u (or after the blank that followed it) is state 2 u + 2
    states, s = [], 0
    for t, c in enumerate(ft):
        if c >= len(y) or c < -1:
            return "frame %d: index %d" % (t, c)
        if c >= 0:
            s = 2 * c + 1
        elif s % 2 == 1:
            s += 1
        states.append(s)
    if states[0] > 1:
        return "starts in state %d" % states[0]
    if states[-1] < n - 2:
        return "ends in state %d of %d" % (states[-1], n)
    for t in range(1, len(states)):
        d = states[t] - states[t - 1]
        if d < 0 or d > 2:
            return "frame %d: step %d" % (t, d)
        if d == 2 and (states[t] % 2 == 0 or y[states[t] // 2] == y[states[t] // 2 - 1]):
            return "frame %d: skip into state %d" % (t, states[t])
    return None


def path_logp(lp, frame_token, y) -> float:
    """The float64 log-probability of the path frame_token (target index per frame, -1 = blank)."""
    lp = np.asarray(lp, dtype=np.float64)
    return float(sum(lp[t, 0 if c < 0 else int(y[int(c)])] for t, c in enumerate(frame_token)))
