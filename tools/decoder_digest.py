"""Digest of what the decoder entries compute: one line `entry | case | SHA-256` over everything the entry returns, on seeded synthetic weights and inputs.

    python tools/decoder_digest.py

Checking a change of the decoders' kernels (csrc/rnnt*.hip, lm.hip, ctc_beam.hip, ctc_align.hip, decode_common.h): run this on the tree before and on the tree
after ON THE SAME GPU and compare the lines - every decoder is deterministic, so equal arithmetic gives equal bytes.  Only the public Python API is used (the
file runs on older trees), one process.  The cases are small and chosen for the code paths:
  Transducer (De, H, J, V) = (48, 32, 32, 40): K16 = 2, one 16-block of weight loads in flight, no cluster shape; (48, 64, 64, 40): K16 = 4, V = 2.5 tiles (a
  clamped, masked last tile and an odd tile count); (48, 128, 128, 50): K16 = 8, the 8-deep loads.  T = 13 with lengths 0 .. 13; greedy at B = 7 and, with
  cluster_decode -1 / 0 / 1, at B = 19; beam 1 / 4 / 16 under beam_eval_batch 1 / 16; lattice + align at u_max 0 and 5 on 45 cells (no multiple of 32) with one
  transcript holding token V (status 2) and one with tokens but no frames (status 1), Viterbi and forward-only.
  LM (H, L, V) = (32, 1, 40), (64, 2, 50): N = 5 / 17 / 40 (the three lm_lstm_step_kernel instances), u_max 6 with lengths 0 .. 6 and one refused sequence,
  temperature 1 and 0.7; score, token_logprobs, decode (the full-logits head) and forward.
  CTC beam search and alignment: B = 3 with a zero-length utterance, V = 40, beam 1 / 4 / 32.  The three instances of the search (csrc/ctc_beam_search.h): plain;
  fused with an LM (32, 1, 40), with its traces; resumed per stream, pushed whole, one frame at a time and in uneven pushes with one that has no frames.
"""
from __future__ import annotations

import copy
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from efficientconformer_amd import LanguageModel, ModelCTC, Transducer, named_config, synth  # noqa: E402

DEV = "cuda:0"
T = 13
BLANK_BIAS = 3.0      # at the tests' 1.2 the beam 1 / beam 4 lines of different widths hashed alike; at 3.0 every utterance ends with status 0 and the lines differ


def digest(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        a = t.detach().cpu().contiguous().numpy()
        h.update(str((a.dtype, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def emit(entry: str, case: str, *tensors):
    torch.cuda.synchronize()
    print("%-16s | %-73s | %s" % (entry, case, digest(*tensors)), flush=True)


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def transducer(h: int, j: int, v: int):
    cfg = copy.deepcopy(named_config("TinyTransducer"))
    cfg["decoder_params"].update(dim_model=h, vocab_size=v)
    cfg["joint_params"].update(dim_model=j)
    if "tokenizer_params" in cfg:
        cfg["tokenizer_params"]["vocab_size"] = v
    m = Transducer.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, 11, None, prefix="encoder.")
    sd.update(synth.make_transducer_state_dict(m.encoder.plan.dim_out, cfg["decoder_params"], cfg["joint_params"], 11, blank_bias=BLANK_BIAS))
    m.load_state_dict({k: torch.from_numpy(a) for k, a in sd.items()})
    return m.to(DEV), m.encoder.plan.dim_out


def transducer_cases(h: int, j: int, v: int):
    m, de = transducer(h, j, v)
    name = "(%d, %d, %d, %d)" % (de, h, j, v)
    g = rng(100 + h)
    f19 = torch.from_numpy(g.standard_normal((19, T, de)).astype(np.float32)).to(DEV)
    len19 = torch.from_numpy(np.array([13, 0, 7, 13, 1, 12, 5] + list(g.integers(0, T + 1, 12)), dtype=np.int64)).to(DEV)
    emit("rnnt_greedy", "%s B=7" % name, *m.decode_encoded(f19[:7], len19[:7]))
    for mode in (-1, 0, 1):
        m.set_decode_option("cluster_decode", mode)
        emit("rnnt_greedy", "%s B=19 cluster_decode=%d" % (name, mode), *m.decode_encoded(f19, len19))
    m.set_decode_option("cluster_decode", -1)
    for batch in (1, 16):
        m.set_decode_option("beam_eval_batch", batch)
        for beam in (1, 4, 16):
            out = m.decode_encoded_beam(f19[:7], len19[:7], beam)
            emit("rnnt_beam", "%s B=7 beam=%d beam_eval_batch=%d status=%s" % (name, beam, batch, "".join(str(int(s)) for s in out[3].cpu())), *out)
    # lattice: T_b (U_b + 1) cells = 13*1 + 5*3 + 0 (refused) + 0 (no frames) + 1*6 + 11*1 = 45
    f_len = torch.tensor([13, 5, 9, 0, 1, 11], dtype=torch.int64, device=DEV)
    y_len = torch.tensor([0, 2, 3, 2, 5, 0], dtype=torch.int64, device=DEV)
    y = torch.from_numpy(g.integers(1, v, (6, 5)).astype(np.int32)).to(DEV)
    y[2, 1] = v                                                       # a token outside the vocabulary: status 2
    for u in (0, 5):
        yl = torch.clamp(y_len, max=u)
        lpb, lpl, st = m.lattice(f19[:6], f_len, y[:, :u].contiguous(), yl)
        emit("rnnt_lattice", "%s B=6 u_max=%d" % (name, u), lpb, lpl, st)
        for scores_only in (False, True):
            out = m.align_lattice(lpb, lpl, f_len, yl, scores_only=scores_only, status=st)
            emit("rnnt_align", "%s B=6 u_max=%d %s" % (name, u, "forward-only" if scores_only else "viterbi"), *[out[k] for k in sorted(out)])


def lm_cases(h: int, layers: int, v: int):
    params = dict(arch="RNN", vocab_size=v, dim_model=h, num_layers=layers)
    m = LanguageModel(params)
    m.load_state_dict({k: torch.from_numpy(a) for k, a in synth.make_lm_state_dict(params, 5).items()})
    m = m.to(DEV)
    name = "(%d, %d, %d)" % (h, layers, v)
    g = rng(200 + h)
    for n in (5, 17, 40):
        y = torch.from_numpy(g.integers(1, v, (n, 6)).astype(np.int32)).to(DEV)
        y_len = torch.from_numpy((np.arange(n) % 7).astype(np.int64)).to(DEV)
        y[n - 1, 0] = 0                                                # n - 1 has length >= 1 for n = 5 / 17 / 40: a refused sequence
        for tmp in (1.0, 0.7):
            emit("lm_score", "%s N=%d tmp=%.1f" % (name, n, tmp), m.score(y, y_len, tmp))
            emit("lm_token_logp", "%s N=%d tmp=%.1f" % (name, n, tmp), *m.token_logprobs(y, y_len, tmp))
        tok = torch.from_numpy(g.integers(0, v, (n, 1)).astype(np.int64)).to(DEV)
        logits, (hh, cc) = m.decode(tok)
        logits2, (hh2, cc2) = m.decode(tok, (hh, cc))
        emit("lm_decode", "%s N=%d" % (name, n), logits, hh, cc, logits2, hh2, cc2)
        emit("lm_forward", "%s N=%d" % (name, n), m((y.clamp(min=1, max=v - 1), torch.clamp(y_len, max=6), None)))


def ctc_cases():
    m = ModelCTC.from_config(named_config("Tiny"))
    g = rng(300)
    v, t = 40, 29
    logits = torch.from_numpy((3.0 * g.standard_normal((3, t, v))).astype(np.float32)).to(DEV)
    lens = torch.tensor([29, 0, 17], dtype=torch.int64, device=DEV)
    for beam in (1, 4, 32):
        emit("ctc_beam", "B=3 T=29 V=40 beam=%d" % beam, *m.decode_logits_beam(logits, lens, beam))
    traced = lambda dicts: [torch.from_numpy(np.ascontiguousarray(d[k])) for d in dicts if d is not None for k in sorted(d)]
    # the fused search: one small LM, a length bonus; everything returned and the workspace's traces (L and total per frame and rank, L per trie node)
    lm_params = dict(arch="RNN", vocab_size=v, dim_model=32, num_layers=1)
    lm = LanguageModel(lm_params)
    lm.load_state_dict({k: torch.from_numpy(a) for k, a in synth.make_lm_state_dict(lm_params, 5).items()})
    lm = lm.to(DEV)
    for beam in (1, 4, 32):
        out = m.decode_logits_beam_lm(logits, lens, beam, lm=lm, lm_weight=0.5, lm_tmp=1.0, length_bonus=0.3)
        emit("ctc_beam_lm", "B=3 T=29 V=40 beam=%d LM (32, 1, 40) w=0.5 bonus=0.3" % beam, *out, *traced(m.last_beam_trace()))
    # the search resumed per stream: every push's outputs and trace, one line per push pattern (cuts between the pushes; 5, 5: a push without frames)
    for beam in (1, 4, 32):
        for name, cuts in (("whole", [0, t]), ("one frame at a time", list(range(t + 1))), ("5 + 0 + 1 + 11 + 12", [0, 5, 5, 6, 17, t])):
            st = m.open_beam_decode_stream(3, t, beam, device=DEV)
            seen = []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                seen += list(st.push(logits[:, lo:hi], torch.clamp(lens - lo, min=0, max=hi - lo)))
                seen += traced(st.last_push_trace())
            emit("ctc_beam_stream", "B=3 T=29 V=40 beam=%d pushes: %s" % (beam, name), *seen)
    y = torch.from_numpy(g.integers(1, v, (3, 7)).astype(np.int32)).to(DEV)
    y[0, 3] = y[0, 2]                                                 # a repeated token: needs a blank between
    y_len = torch.tensor([7, 0, 5], dtype=torch.int64, device=DEV)
    for u in (0, 7):
        for scores_only in (False, True):
            out = m.align_logits(logits, lens, y[:, :u].contiguous(), torch.clamp(y_len, max=u), scores_only=scores_only)
            emit("ctc_align", "B=3 T=29 V=40 u_max=%d %s" % (u, "forward-only" if scores_only else "viterbi"), *[out[k] for k in sorted(out)])
    bad = y.clone()
    bad[2, 1] = v                                                     # status 2
    lens2 = torch.tensor([29, 3, 17], dtype=torch.int64, device=DEV)
    out = m.align_logits(logits, lens2, bad, torch.tensor([7, 6, 5], dtype=torch.int64, device=DEV))      # utterance 1: more tokens than frames (status 1)
    emit("ctc_align", "B=3 T=29 V=40 u_max=7 refused rows", *[out[k] for k in sorted(out)])


def main():
    for h, j, v in ((32, 32, 40), (64, 64, 40), (128, 128, 50)):
        transducer_cases(h, j, v)
    for h, layers, v in ((32, 1, 40), (64, 2, 50)):
        lm_cases(h, layers, v)
    ctc_cases()


if __name__ == "__main__":
    with torch.no_grad():
        main()
