"""Float64 restatement of the reference's RNN-T beam search (test helper, not a test module).

Transducer.beam_search_decoding of burchim/EfficientConformer (models/transducer.py:188-327) without the LM and n-gram terms:
per frame A = B, B = []; until B holds ``beam`` hypotheses pop the hypothesis of A with the largest score / len(prediction)
(first maximum in list order), evaluate the decoder on (prediction[-1], state) and the joint on (f[t], g), logP =
(logits / tmp).softmax().log(), and append a child for each of the top ``beam`` entries: blank -> B (same prediction and state),
any other label -> A (label appended, state = the decoder's new one).  The answer is the best hypothesis of B.

Built on oracle.ref_transducer.lstm_step / joint_logits, evaluated in float64.  Besides the tokens it reports the best score, the
expansions (pops) per frame and whether ``max_expansions`` pops left B short in some frame (the reference would loop on).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from oracle.ref_transducer import joint_logits, lstm_step


def _sd64(sd: Dict, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    return {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(v)).to(dtype)
            for k, v in sd.items() if k.startswith(("decoder.", "joint_network."))}


def beam_decode(sd: Dict, f: torch.Tensor, f_len, beam: int, tmp: float = 1.0, max_expansions: Optional[int] = None, dtype=torch.float64):
    """-> list (one per utterance) of dicts: tokens (without the start token), score (float64 logp_score of the answer),
    expansions (pops per frame), capped (True when a frame needed more than max_expansions pops; tokens then []).
    dtype: torch.float32 evaluates the same program in float32 (what the reference's own rounding does to it)."""
    sd = _sd64(sd, dtype)
    hd = sd["decoder.rnn.weight_hh_l0"].shape[1]
    f = f.to(dtype)
    out = []
    with torch.no_grad():
        for b in range(f.shape[0]):
            zero = (torch.zeros(hd, dtype=dtype), torch.zeros(hd, dtype=dtype))
            # a hypothesis: prediction, score, state (h, c) the decoder runs from, and the memo of that decoder step (a blank child
            # keeps its parent's prediction and state, so its decoder output is the parent's)
            B = [{"pred": [0], "score": 0.0, "state": zero, "dec": None}]
            expansions: List[int] = []
            capped = False
            for t in range(int(f_len[b])):
                A, B = B, []
                pops = 0
                while len(B) < beam:
                    if max_expansions is not None and pops >= max_expansions:
                        capped = True
                        break
                    best = max(A, key=lambda h: h["score"] / len(h["pred"]))
                    A.remove(best)
                    pops += 1
                    if best["dec"] is None:
                        best["dec"] = lstm_step(sd, best["pred"][-1], *best["state"])
                    h, c = best["dec"]
                    logits = joint_logits(sd, f[b, t], h) / tmp
                    logp = logits.softmax(-1).log()
                    vals, labels = torch.topk(logp, beam)
                    for v, lab in zip(vals.tolist(), labels.tolist()):
                        if lab == 0:
                            B.append({"pred": best["pred"], "score": best["score"] + v, "state": best["state"], "dec": best["dec"]})
                        else:
                            A.append({"pred": best["pred"] + [lab], "score": best["score"] + v, "state": (h, c), "dec": None})
                expansions.append(pops)
                if capped:
                    break
            if capped:
                out.append({"tokens": [], "score": 0.0, "expansions": expansions, "capped": True})
                continue
            best = max(B, key=lambda h: h["score"] / len(h["pred"]))
            out.append({"tokens": best["pred"][1:], "score": best["score"], "expansions": expansions, "capped": False})
    return out
