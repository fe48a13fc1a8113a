"""Float64 oracle of the CTC prefix beam search (test helper, not a test module).

ctcdecode's CTCBeamDecoder as the reference's ModelCTC.beam_search_decoding calls it (models/model_ctc.py:138-181: blank 0,
cutoff_top_n = V, cutoff_prob 1, no n-gram scorer).  A prefix is a token string without blanks with pb / pnb = log P(ending in a
blank / a non-blank) and score s = lse(pb, pnb).  Per frame, with lp = logP[t], every member P of the beam gives
    b'(P) = lp[0] + s(P),   nb'(P) = lp[last(P)] + pnb(P) (P not empty),
    for c != 0, Q = P c:   nb'(Q) (+)= lp[c] + (pb(P) if c == last(P) else s(P))
((+)= is a log-sum-exp; a Q that is not a member starts at -inf and is a candidate even when its term is -inf).  The best ``beam``
candidates survive, ordered by score desc, then last token asc (the empty prefix counts as -1), then the canonical index (the
members in rank order, then the extensions by (parent rank, token)).  After the last frame the beam is in that order.

Prefix identity is the token string.  ``slot_identity=True`` instead identifies a prefix by (the node of its parent, token), with a
fresh node whenever a prefix enters the beam: a prefix that left the beam and comes back then no longer merges with a longer member
built on its old node.  That mode exists only to show that the re-entry fixtures tell the two apart.

``shortcut=True`` evaluates, per member, only its ``beam`` best plain extensions among the frame's 2 beam + 1 most probable tokens
(lp desc, id asc), plus the repeat extension and the merges - what the kernel evaluates.  Every candidate is evaluated otherwise.
"""
from __future__ import annotations

import itertools
from typing import Dict, List, Optional

import numpy as np
import torch

NEG = -np.inf


def lse(a, b):
    m = np.maximum(a, b)
    with np.errstate(invalid="ignore"):
        r = m + np.log1p(np.exp(-np.abs(a - b)))
    return np.where(m == NEG, NEG, r)


def logp64(logits, tmp: float = 1.0) -> np.ndarray:
    """float64 log-softmax of fp32 logits / tmp (the specification's logP without fp32 rounding)."""
    x = torch.as_tensor(logits).double() / tmp
    return torch.log_softmax(x, dim=-1).numpy()


def logp32(logits, tmp: float = 1.0) -> np.ndarray:
    """The reference's own logP: (logits / tmp).softmax(-1).log() in fp32 (-inf where the fp32 probability is 0), as float64."""
    x = torch.as_tensor(logits).float() / tmp
    return x.softmax(dim=-1).log().double().numpy()


def beam_search(lp: np.ndarray, length: Optional[int], beam: int, shortcut: bool = False, slot_identity: bool = False,
                trace: bool = False) -> Dict:
    """lp: (T, V) float64 log-probabilities of one utterance.  -> dict: prefixes (ranked tuples), pb, pnb, score (float64 arrays),
    gap (the smallest decision gap: score at rank beam - 1 minus score at rank beam at every frame's cut, and the differences of
    consecutive final ranks; inf when nothing was ever decided), beams (per frame, when ``trace``: list of (prefix, pb, pnb))."""
    lp = np.asarray(lp, dtype=np.float64)
    t_all, v = lp.shape
    length = t_all if length is None else max(0, min(int(length), t_all))
    # members: (prefix, pb, pnb, node, parent node); node ids matter only in slot_identity mode
    members = [((), 0.0, NEG, 0, -1)]
    next_node = 1
    gap = np.inf
    beams = []
    k_top = min(2 * beam + 1, v)
    for t in range(length):
        row = lp[t]
        n = len(members)
        s = np.array([lse(pb, pnb) for _, pb, pnb, _, _ in members], dtype=np.float64)
        if slot_identity:      # (parent node, token); a prefix entering the beam gets a fresh node below
            index = {(par, p[-1]): k for k, (p, _, _, _, par) in enumerate(members) if p}
            ident = lambda i, c: (members[i][3], c)
        else:
            index = {p: k for k, (p, _, _, _, _) in enumerate(members)}
            ident = lambda i, c: members[i][0] + (c,)
        mpb = row[0] + s
        mnb = np.array([row[p[-1]] + pnb if p else NEG for p, _, pnb, _, _ in members], dtype=np.float64)
        order = np.lexsort((np.arange(v), -row))                 # tokens by (lp desc, id asc)
        top = order[:k_top]
        ext_s, ext_last, ext_canon, ext_par = [], [], [], []
        for i, (p, pb, pnb, node, _) in enumerate(members):
            last = p[-1] if p else -1
            terms = row + s[i]
            if last >= 0:
                terms[last] = row[last] + pb
            plain = np.ones(v, dtype=bool)
            plain[0] = False
            children = [m[0][-1] for m in members if m[0] and ((m[4] == node) if slot_identity else m[0][:-1] == p)]
            for c in children:
                k = index[ident(i, c)]
                mnb[k] = lse(mnb[k], terms[c])
                plain[c] = False
            if shortcut:
                keep = np.zeros(v, dtype=bool)
                if last >= 0 and plain[last]:
                    keep[last] = True
                plain_top = [c for c in top if plain[c] and c != last][:beam]
                keep[plain_top] = True
                plain &= keep
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
        if len(rank) > beam:
            with np.errstate(invalid="ignore"):
                d = all_s[rank[beam - 1]] - all_s[rank[beam]]
            gap = min(gap, d if np.isfinite(d) else (0.0 if all_s[rank[beam - 1]] == all_s[rank[beam]] else np.inf))
        new = []
        for j in rank[:beam]:
            if all_par[j] < 0:
                p, _, _, node, par = members[all_canon[j]]
                new.append((p, all_pb[j], all_nb[j], node, par))
            else:
                i = int(all_par[j])
                new.append((members[i][0] + (int(all_last[j]),), all_pb[j], all_nb[j], next_node, members[i][3]))
                next_node += 1
        members = new
        if trace:
            beams.append([(p, pb, pnb) for p, pb, pnb, _, _ in members])
    sc = np.array([lse(pb, pnb) for _, pb, pnb, _, _ in members], dtype=np.float64)
    for a, b in zip(sc[:-1], sc[1:]):
        if np.isfinite(a) and np.isfinite(b):
            gap = min(gap, a - b)
    return {"prefixes": [m[0] for m in members], "pb": np.array([m[1] for m in members]), "pnb": np.array([m[2] for m in members]),
            "score": sc, "gap": gap, "beams": beams}


def brute_force(lp: np.ndarray, length: Optional[int] = None) -> Dict[tuple, float]:
    """log P(labelling) for every labelling reachable by some alignment of the first ``length`` frames (all V^T alignments)."""
    lp = np.asarray(lp, dtype=np.float64)
    t_all, v = lp.shape
    length = t_all if length is None else length
    out: Dict[tuple, float] = {}
    for path in itertools.product(range(v), repeat=length):
        lab, prev = [], 0
        for c in path:
            if c != 0 and c != prev:
                lab.append(c)
            prev = c
        w = float(sum(lp[t, c] for t, c in enumerate(path)))
        key = tuple(lab)
        out[key] = float(lse(out[key], w)) if key in out else w
    return out


def all_labellings(v: int, t: int) -> List[tuple]:
    """Every token string (no blanks) of length <= t over tokens 1 .. v - 1."""
    out = [()]
    for n in range(1, t + 1):
        out += list(itertools.product(range(1, v), repeat=n))
    return out


def ctc_log_prob(lp: np.ndarray, length: int, tokens) -> float:
    """-ctc_loss in float64: log of the total probability of ``tokens`` over the first ``length`` frames."""
    x = torch.as_tensor(np.asarray(lp, dtype=np.float64)[:length]).unsqueeze(1)
    tgt = torch.tensor([list(tokens)], dtype=torch.long) if len(tokens) else torch.zeros(1, 0, dtype=torch.long)
    loss = torch.nn.functional.ctc_loss(x, tgt, torch.tensor([length]), torch.tensor([len(tokens)]), blank=0, reduction="none",
                                        zero_infinity=False)
    return -float(loss[0])
