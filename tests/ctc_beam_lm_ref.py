"""Float64 oracle of the CTC prefix beam search with neural-LM shallow fusion (test helper, not a test module).

The acoustic recursion is tests/ctc_beam_ref.py's: pb / pnb per prefix, s = lse(pb, pnb).  The LM score of a token string P is
    L(()) = 0,   L(P c) = L(P) + row_P[c],   row_P = log_softmax(fc(h_P) / lm_tmp),   h_P = the LSTM state after reading [0] + P
(``LanguageModel``'s convention; tests/lm_ref.py's ``step``), a function of the string alone.  Candidates are ranked by
    total(Q) = s(Q) + lm_weight * L(Q) + length_bonus * |Q|
desc, then last token asc (the empty prefix counts as -1), then the canonical index (members in rank order, then the extensions by
(parent rank, token)).  At lm_weight = 0 and length_bonus = 0 this is ``ctc_beam_ref.beam_search``.

``shortcut=True`` evaluates, per member, only its ``beam`` best plain extensions (not blank, not last(P), P c not a member) by
a_P[c] = lp[c] + lm_weight * row_P[c] (a desc, id asc), plus the repeat extension and the merges - what the kernel evaluates.  Every
candidate is evaluated otherwise.

``LmRows`` serves the rows, cached by string: in float64 (lm_ref.step) or, ``float32=True``, from torch's own float32 Embedding + nn.LSTM +
Linear + log_softmax (as float64 values) - the reference arithmetic whose decisions the GPU fixtures must share with the float64 ones.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

import ctc_beam_ref
import lm_ref
from ctc_beam_ref import NEG, lse


class LmRows:
    """row(P) = log_softmax(fc(h_P) / lm_tmp) as a float64 array, L(P); both cached by the token string."""

    def __init__(self, sd: Dict[str, np.ndarray], lm_tmp: float = 1.0, float32: bool = False):
        self.sd, self.tmp, self.float32 = sd, float(lm_tmp), float32
        self._state, self._row, self._L = {}, {}, {(): 0.0}
        self.evaluations = 0
        if float32:
            v, h = sd["fc.weight"].shape
            layers = lm_ref.num_layers(sd)
            t = {k: torch.from_numpy(np.asarray(x)) for k, x in sd.items()}
            self._emb = torch.nn.Embedding(v, h)
            self._rnn = torch.nn.LSTM(h, h, layers, batch_first=True)
            self._fc = torch.nn.Linear(h, v)
            self._emb.load_state_dict({"weight": t["decoder.embedding.weight"]})
            self._rnn.load_state_dict({k[len("decoder.rnn."):]: x for k, x in t.items() if k.startswith("decoder.rnn.")})
            self._fc.load_state_dict({"weight": t["fc.weight"], "bias": t["fc.bias"]})

    def _eval(self, p: tuple):
        tok = p[-1] if p else 0
        prev = None
        if p:
            self.row(p[:-1])
            prev = self._state[p[:-1]]
        self.evaluations += 1
        if self.float32:
            with torch.no_grad():
                y, state = self._rnn(self._emb(torch.tensor([[tok]])), prev)
                row = torch.log_softmax(self._fc(y)[0, 0] / self.tmp, dim=-1).double().numpy()
        else:
            logits, state = lm_ref.step(self.sd, [tok], prev)
            row = lm_ref.log_softmax(logits[0] / self.tmp)
        self._state[p], self._row[p] = state, row

    def row(self, p: tuple) -> np.ndarray:
        if p not in self._row:
            self._eval(p)
        return self._row[p]

    def L(self, p: tuple) -> float:
        if p not in self._L:
            self._L[p] = self.L(p[:-1]) + float(self.row(p[:-1])[p[-1]])
        return self._L[p]


def total_of(s, L, n, w, bonus):
    if s == NEG:
        return NEG
    return s + (w * L if w else 0.0) + (bonus * n if bonus else 0.0)


def beam_search(lp: np.ndarray, length: Optional[int], beam: int, rows: Optional[LmRows], lm_weight: float, length_bonus: float = 0.0,
                shortcut: bool = False, trace: bool = False) -> Dict:
    """lp: (T, V) float64 log-probabilities of one utterance -> dict: prefixes (ranked tuples), pb, pnb, score (= s), lm (= L), total (float64
    arrays), gap (the smallest decision gap on totals: rank beam - 1 minus rank beam at every frame's cut, and the differences of consecutive
    final ranks; inf when nothing was ever decided; cuts between two totals of -inf are decided by the indices and do not count), entered (prefixes that entered the beam as an extension, over the utterance), reentries (those
    of them that had been in the beam before), beams (per frame, when ``trace``: list of (prefix, pb, pnb, L, total))."""
    lp = np.asarray(lp, dtype=np.float64)
    t_all, v = lp.shape
    length = t_all if length is None else max(0, min(int(length), t_all))
    w, bonus = float(lm_weight), float(length_bonus)
    Lof = (lambda p: rows.L(p)) if (rows is not None and w) else (lambda p: 0.0)
    members = [((), 0.0, NEG)]
    seen = {()}
    gap = np.inf
    entered = reentries = 0
    beams = []
    for t in range(length):
        row = lp[t]
        n = len(members)
        s = np.array([float(lse(pb, pnb)) for _, pb, pnb in members], dtype=np.float64)
        index = {p: k for k, (p, _, _) in enumerate(members)}
        mpb = row[0] + s
        mnb = np.array([row[p[-1]] + pnb if p else NEG for p, _, pnb in members], dtype=np.float64)
        ext_s, ext_last, ext_canon, ext_par, ext_tot = [], [], [], [], []
        for i, (p, pb, pnb) in enumerate(members):
            last = p[-1] if p else -1
            terms = row + s[i]
            if last >= 0:
                terms[last] = row[last] + pb
            plain = np.ones(v, dtype=bool)
            plain[0] = False
            for q, _, _ in members:
                if q and q[:-1] == p:
                    k = index[q]
                    mnb[k] = lse(mnb[k], terms[q[-1]])
                    plain[q[-1]] = False
            lmrow = rows.row(p) if (rows is not None and w) else np.zeros(v)
            if shortcut:
                keep = np.zeros(v, dtype=bool)
                if last >= 0 and plain[last]:
                    keep[last] = True
                a = row + w * lmrow
                order = np.lexsort((np.arange(v), -a))
                keep[[c for c in order if plain[c] and c != last][:beam]] = True
                plain &= keep
            cs = np.nonzero(plain)[0]
            Lp = Lof(p)
            ext_s.append(terms[cs])
            ext_last.append(cs)
            ext_canon.append(n + i * v + cs)
            ext_par.append(np.full(cs.shape, i))
            ext_tot.append(np.array([total_of(terms[c], Lp + lmrow[c], len(p) + 1, w, bonus) for c in cs], dtype=np.float64))
        msc = lse(mpb, mnb)
        mtot = np.array([total_of(float(msc[k]), Lof(members[k][0]), len(members[k][0]), w, bonus) for k in range(n)], dtype=np.float64)
        all_s = np.concatenate([msc] + ext_s)
        all_tot = np.concatenate([mtot] + ext_tot)
        all_last = np.concatenate([np.array([m[0][-1] if m[0] else -1 for m in members])] + ext_last)
        all_canon = np.concatenate([np.arange(n)] + ext_canon)
        all_par = np.concatenate([np.full(n, -1)] + ext_par)
        all_pb = np.concatenate([mpb] + [np.full(e.shape, NEG) for e in ext_s])
        all_nb = np.concatenate([mnb] + ext_s)
        rank = np.lexsort((all_canon, all_last, -all_tot))
        if len(rank) > beam:
            hi, lo = all_tot[rank[beam - 1]], all_tot[rank[beam]]
            with np.errstate(invalid="ignore"):
                d = hi - lo
            if np.isfinite(d):                   # -inf against -inf (a prefix that has no mass yet) is decided by the indices, not by arithmetic
                gap = min(gap, d)
        new = []
        for j in rank[:beam]:
            if all_par[j] < 0:
                p = members[all_canon[j]][0]
            else:
                p = members[int(all_par[j])][0] + (int(all_last[j]),)
                entered += 1
                reentries += p in seen
                seen.add(p)
            new.append((p, all_pb[j], all_nb[j]))
        members = new
        if trace:
            beams.append([(p, pb, pnb, Lof(p), total_of(float(lse(pb, pnb)), Lof(p), len(p), w, bonus)) for p, pb, pnb in members])
    sc = np.array([float(lse(pb, pnb)) for _, pb, pnb in members], dtype=np.float64)
    lm = np.array([Lof(p) for p, _, _ in members], dtype=np.float64)
    tot = np.array([total_of(sc[k], lm[k], len(members[k][0]), w, bonus) for k in range(len(members))], dtype=np.float64)
    for a, b in zip(tot[:-1], tot[1:]):
        if np.isfinite(a) and np.isfinite(b):
            gap = min(gap, a - b)
    return {"prefixes": [m[0] for m in members], "pb": np.array([m[1] for m in members]), "pnb": np.array([m[2] for m in members]),
            "score": sc, "lm": lm, "total": tot, "gap": gap, "entered": entered, "reentries": reentries, "beams": beams}


def rescored_best(lp: np.ndarray, length: Optional[int], beam: int, rows: LmRows, lm_weight: float, length_bonus: float = 0.0) -> tuple:
    """The best of the LM-blind search's n-best after rescoring (``ModelCTC.rescore_nbest``'s rule): what fusion is not."""
    ref = ctc_beam_ref.beam_search(lp, length, beam)
    tot = [total_of(float(s), rows.L(p), len(p), lm_weight, length_bonus) for p, s in zip(ref["prefixes"], ref["score"])]
    return ref["prefixes"][int(np.argmax(tot))]
