"""Float64 restatement of the reference's RNN-T beam search WITH its neural-LM shallow fusion term (test helper, not a test module).

Transducer.beam_search_decoding of burchim/EfficientConformer (models/transducer.py:188-327) without the n-gram terms: the loop of
tests/rnnt_beam_ref.py, and at every expansion the language model runs beside the prediction network,

    logits_lm, hidden_lm = lm.decode(prediction[-1], hidden_state_lm)
    logP = (logits / tmp).softmax().log() + lm_weight * (logits_lm / lm_tmp).softmax().log()

before the top ``beam`` entries are taken; a label child takes hidden_lm, a blank child keeps its parent's LM state (transducer.py:291-306).

Built on oracle.ref_transducer.lstm_step / joint_logits and tests/lm_ref.step (the float64 LM oracle).  A blank child keeps its parent's
prediction, decoder state and LM state, so both its decoder output and its LM row are the parent's: they are memoised per hypothesis, which is
the reference's arithmetic evaluated once.  ``dtype=torch.float32`` evaluates the same program in float32 (the LM step then by the float32
twin of lm_ref.step below): what the reference's own rounding does to it.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

import lm_ref
from oracle.ref_transducer import joint_logits, lstm_step
from rnnt_beam_ref import _sd64


def lm_step_torch(lm_sd: Dict[str, torch.Tensor], layers: int, token: int, state):
    """lm_ref.step's formulas for one token in the dtype of the tensors `lm_sd`: -> (logits (V,), (h, c) each (L, H))."""
    dtype = lm_sd["fc.weight"].dtype
    hd = lm_sd["fc.weight"].shape[1]
    h, c = (torch.zeros(layers, hd, dtype=dtype), torch.zeros(layers, hd, dtype=dtype)) if state is None else (state[0].clone(), state[1].clone())
    x = lm_sd["decoder.embedding.weight"][token]
    for l in range(layers):
        g = (lm_sd["decoder.rnn.weight_ih_l%d" % l] @ x + lm_sd["decoder.rnn.bias_ih_l%d" % l]
             + lm_sd["decoder.rnn.weight_hh_l%d" % l] @ h[l] + lm_sd["decoder.rnn.bias_hh_l%d" % l])
        i, f, gg, o = torch.sigmoid(g[:hd]), torch.sigmoid(g[hd:2 * hd]), torch.tanh(g[2 * hd:3 * hd]), torch.sigmoid(g[3 * hd:])
        c[l] = f * c[l] + i * gg
        h[l] = o * torch.tanh(c[l])
        x = h[l]
    return lm_sd["fc.weight"] @ x + lm_sd["fc.bias"], (h, c)


def _lm_step(lm_sd: Dict[str, torch.Tensor], layers: int, token: int, state, dtype):
    """lm.decode of one token: -> (logits (V,), (h, c)).  float64: tests/lm_ref.step; any other dtype: lm_step_torch."""
    if dtype != torch.float64:
        return lm_step_torch(lm_sd, layers, token, state)
    np_state = None if state is None else (state[0][:, None, :], state[1][:, None, :])
    logits, (h, c) = lm_ref.step({k: v.numpy() for k, v in lm_sd.items()}, [token], np_state)
    return torch.from_numpy(logits[0]), (h[:, 0], c[:, 0])


def beam_decode_lm(sd: Dict, lm_sd: Dict, f: torch.Tensor, f_len, beam: int, lm_weight: float, tmp: float = 1.0, lm_tmp: float = 1.0,
                   max_expansions: Optional[int] = None, dtype=torch.float64):
    """-> list (one per utterance) of dicts: tokens (without the start token), score (logp_score of the answer), expansions (pops per frame),
    lm_steps (LM evaluations), capped (True when a frame needed more than max_expansions pops; tokens then [])."""
    sd = _sd64(sd, dtype)
    lm_t = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).to(dtype) for k, v in lm_sd.items()}
    layers = lm_ref.num_layers(lm_sd)
    hd = sd["decoder.rnn.weight_hh_l0"].shape[1]
    w = torch.tensor(lm_weight, dtype=dtype)
    f = f.to(dtype)
    out = []
    with torch.no_grad():
        for b in range(f.shape[0]):
            zero = (torch.zeros(hd, dtype=dtype), torch.zeros(hd, dtype=dtype))
            # a hypothesis: prediction, score, decoder state, LM state, and the memo of its evaluation (decoder output, LM log-probabilities, new LM state)
            B = [{"pred": [0], "score": 0.0, "state": zero, "lm": None, "memo": None}]
            expansions: List[int] = []
            capped, lm_steps = False, 0
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
                    if best["memo"] is None:
                        dec = lstm_step(sd, best["pred"][-1], *best["state"])
                        lm_logits, lm_new = _lm_step(lm_t, layers, best["pred"][-1], best["lm"], dtype)
                        lm_steps += 1
                        best["memo"] = (dec, (lm_logits.to(dtype) / lm_tmp).softmax(-1).log(), lm_new)
                    (h, c), logp_lm, lm_new = best["memo"]
                    logits = joint_logits(sd, f[b, t], h) / tmp
                    logp = logits.softmax(-1).log()
                    logp = logp + w * logp_lm
                    vals, labels = torch.topk(logp, beam)
                    for v, lab in zip(vals.tolist(), labels.tolist()):
                        if lab == 0:
                            B.append({"pred": best["pred"], "score": best["score"] + v, "state": best["state"], "lm": best["lm"], "memo": best["memo"]})
                        else:
                            A.append({"pred": best["pred"] + [lab], "score": best["score"] + v, "state": (h, c), "lm": lm_new, "memo": None})
                expansions.append(pops)
                if capped:
                    break
            if capped:
                out.append({"tokens": [], "score": 0.0, "expansions": expansions, "lm_steps": lm_steps, "capped": True})
                continue
            best = max(B, key=lambda h: h["score"] / len(h["pred"]))
            out.append({"tokens": best["pred"][1:], "score": best["score"], "expansions": expansions, "lm_steps": lm_steps, "capped": False})
    return out
