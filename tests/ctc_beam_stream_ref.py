"""The specification of the streaming CTC prefix beam search (test helper, not a test module): tests/ctc_beam_ref.py's search, chunked, with the carried
state explicit - the members of the beam in rank order, each with its token string, pb and pnb, and nothing else.

``ChunkedSearch.push(rows)`` advances one stream by the frames of a push with the frame step of ``ctc_beam_ref.beam_search`` (every candidate evaluated,
prefix identity = the token string), written on its pieces (``lse``; the callers make the rows with ``logp64`` / ``logp32``), in the same order of
operations: after any pushes the beam equals ``beam_search`` on the concatenated rows exactly (strings, order, pb, pnb, scores).
``stable_prefix(beam)`` is the longest common prefix of all members: every member of a later beam is a member of this one or an extension of one, so every later
hypothesis of every rank begins with it.

``schedule(pattern, lens)`` holds the push patterns, shared with the GPU test: a list of rounds, each a list of (stream, frames) in the order the round lists
its streams.  A stream that is not in a round is not listed in that push; (stream, 0) is a zero-frame push: the beam is read, not changed.

``fault``: what a wrong carry would do at a push boundary (before every push but a stream's first) - the tests show that each changes the result.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from ctc_beam_ref import NEG, lse

PATTERNS = ("whole", "ones", "first1", "uneven", "gaps", "subsets")
FAULTS = ("swap_pb_pnb", "cut_to_best", "resort_by_last", "frames_off_by_one", "drop_state")
UNEVEN = (5, 1, 7, 2, 3, 11)


def start():
    """The beam of a stream that never had a frame: the empty prefix, pb = 0, pnb = -inf."""
    return [((), 0.0, NEG)]


def step(members, row: np.ndarray, beam: int):
    """One frame of ctc_beam_ref.beam_search (shortcut = False, slot_identity = False) on members [(prefix, pb, pnb)] -> the next members."""
    row = np.asarray(row, dtype=np.float64)
    v, n = row.shape[0], len(members)
    s = np.array([lse(pb, pnb) for _, pb, pnb in members], dtype=np.float64)
    index = {p: k for k, (p, _, _) in enumerate(members)}
    mpb = row[0] + s
    mnb = np.array([row[p[-1]] + pnb if p else NEG for p, _, pnb in members], dtype=np.float64)
    ext_s, ext_last, ext_canon, ext_par = [], [], [], []
    for i, (p, pb, pnb) in enumerate(members):
        last = p[-1] if p else -1
        terms = row + s[i]
        if last >= 0:
            terms[last] = row[last] + pb
        plain = np.ones(v, dtype=bool)
        plain[0] = False
        for c in [m[0][-1] for m in members if m[0] and m[0][:-1] == p]:
            k = index[p + (c,)]
            mnb[k] = lse(mnb[k], terms[c])
            plain[c] = False
        cs = np.nonzero(plain)[0]
        ext_s.append(terms[cs])
        ext_last.append(cs)
        ext_canon.append(n + i * v + cs)
        ext_par.append(np.full(cs.shape, i))
    msc = lse(mpb, mnb)
    all_s = np.concatenate([msc] + ext_s)
    all_last = np.concatenate([np.array([m[0][-1] if m[0] else -1 for m in members])] + ext_last)
    all_canon = np.concatenate([np.arange(n)] + ext_canon)
    all_par = np.concatenate([np.full(n, -1)] + ext_par)
    all_pb = np.concatenate([mpb] + [np.full(e.shape, NEG) for e in ext_s])
    all_nb = np.concatenate([mnb] + ext_s)
    rank = np.lexsort((all_canon, all_last, -all_s))
    new = []
    for j in rank[:beam]:
        if all_par[j] < 0:
            new.append((members[all_canon[j]][0], all_pb[j], all_nb[j]))
        else:
            new.append((members[int(all_par[j])][0] + (int(all_last[j]),), all_pb[j], all_nb[j]))
    return new


def stable_prefix(members) -> tuple:
    """The longest common prefix of all members' token strings."""
    strs = [m[0] for m in members]
    n = min(len(p) for p in strs)
    for i in range(n):
        if any(p[i] != strs[0][i] for p in strs):
            return strs[0][:i]
    return strs[0][:n]


def scores(members) -> np.ndarray:
    return np.array([lse(pb, pnb) for _, pb, pnb in members], dtype=np.float64)


class ChunkedSearch:
    """One stream: the carried beam, and ``push``."""

    def __init__(self, beam: int, fault: Optional[str] = None):
        assert fault is None or fault in FAULTS
        self.beam, self.fault = beam, fault
        self.members = start()
        self.frames = 0
        self.beams = []                              # the beam after every frame: [(prefix, pb, pnb)]

    def _boundary(self):
        f, m = self.fault, self.members
        if f == "swap_pb_pnb":
            self.members = [(p, pnb, pb) for p, pb, pnb in m]
        elif f == "cut_to_best":
            self.members = m[:1]
        elif f == "resort_by_last":
            self.members = sorted(m, key=lambda x: x[0][-1] if x[0] else -1)
        elif f == "drop_state":
            self.members = start()

    def push(self, rows: np.ndarray):
        """rows (k, V) log-probabilities, k >= 0 -> the members after the push."""
        rows = np.asarray(rows, dtype=np.float64)
        if self.frames > 0:
            self._boundary()
        for t in range(rows.shape[0]):
            self.members = step(self.members, rows[t], self.beam)
            self.beams.append(list(self.members))
        self.frames += rows.shape[0]
        return self.members


def schedule(pattern: str, lens: Sequence[int], seed: int = 0) -> List[List[Tuple[int, int]]]:
    """The rounds of a pattern for streams of `lens` frames; every stream's frames sum to its length."""
    n = len(lens)
    if pattern == "whole":
        return [[(b, lens[b]) for b in range(n)]]
    if pattern == "ones":
        return [[(b, 1) for b in range(n) if r < lens[b]] for r in range(max(lens))]
    if pattern == "first1":
        return [[(b, min(1, lens[b])) for b in range(n)], [(b, lens[b] - 1) for b in range(n) if lens[b] > 1]]
    if pattern in ("uneven", "gaps"):
        rounds, done, r = [], [0] * n, 0
        while any(done[b] < lens[b] for b in range(n)):
            cur = []
            for b in range(n):
                if done[b] >= lens[b]:
                    continue
                k = min(UNEVEN[(r + b) % len(UNEVEN)], lens[b] - done[b])
                if pattern == "gaps" and (r + b) % 3 == 1:
                    k = 0                             # the stream is listed without frames
                cur.append((b, k))
                done[b] += k
            rounds.append(cur)
            r += 1
        if pattern == "gaps":
            rounds.append([(b, 0) for b in range(n)])            # the hypothesis read without new audio, finished streams included
        return rounds
    if pattern == "subsets":
        rng = np.random.default_rng(1234 + seed)
        rounds, done = [], [0] * n
        while any(done[b] < lens[b] for b in range(n)):
            live = [b for b in range(n) if done[b] < lens[b]]
            pick = [b for b in live if rng.random() < 0.6] or [live[int(rng.integers(len(live)))]]
            pick = [pick[i] for i in rng.permutation(len(pick))]
            cur = []
            for b in pick:
                k = min(int(rng.integers(1, 7)), lens[b] - done[b])
                cur.append((b, k))
                done[b] += k
            rounds.append(cur)
        return rounds
    raise ValueError(pattern)


def run(lp: Sequence[np.ndarray], pattern: str, beam: int, fault: Optional[str] = None, seed: int = 0):
    """Streams with the log-probability rows lp[b] (T_b, V) through a pattern -> (searches, history); history[b]: the members after every push that listed
    stream b.  frames_off_by_one: every push but a stream's first starts one frame late and ends one frame late (the last frame twice at the end)."""
    lens = [x.shape[0] for x in lp]
    srch = [ChunkedSearch(beam, fault) for _ in lens]
    done = [0] * len(lens)
    hist = [[] for _ in lens]
    for rnd in schedule(pattern, lens, seed):
        for b, k in rnd:
            lo, hi = done[b], done[b] + k
            if fault == "frames_off_by_one" and lo > 0 and k > 0:
                idx = np.minimum(np.arange(lo + 1, hi + 1), lens[b] - 1)
                rows = lp[b][idx]
            else:
                rows = lp[b][lo:hi]
            hist[b].append(list(srch[b].push(rows)))
            done[b] = hi
    assert done == lens
    return srch, hist
