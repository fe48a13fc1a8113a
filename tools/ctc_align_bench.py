#!/usr/bin/env python3
"""CTC forced alignment / transcript scoring cost (effconf_ctc_align): EfficientConformerCTC-Small (synthetic weights, bf16 path) on
ragged LibriSpeech-like mel batches (the length generator of tools/ctc_beam_bench.py), B = 256, V = 256, targets = the greedy labels of
the same logits.  Per batch size: ms per ``align_logits`` (emissions + Viterbi + forward + spans), per scoring-only call (emissions +
forward), per greedy head (fc + argmax + collapse) of the same batch, and per host ``ctc_loss`` in float64 on the logits INCLUDING their
copy to the host - what log P(y | x) cost before.  Medians of timed runs.

    python tools/ctc_align_bench.py [--batches 256] [--reps 5] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientconformer_amd import ModelCTC, named_config, synth  # noqa: E402


def build():
    cfg = named_config("EfficientConformerCTCSmall")
    m = ModelCTC.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, 0, cfg["tokenizer_params"]["vocab_size"], prefix="encoder.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def host_ctc_loss(logits, enc_len, labels, label_len):
    lp = torch.log_softmax(logits.cpu().double(), dim=-1).transpose(0, 1)          # the D2H copy is part of the cost
    return -torch.nn.functional.ctc_loss(lp, labels.cpu().long(), enc_len.cpu(), label_len.cpu().long(), blank=0, reduction="none")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    m = build()
    rows = []
    for b in [int(x) for x in args.batches.split(",")]:
        ml = np.maximum(16, synth.libri_lengths(b, seed=11) // 160).astype(np.int64)
        mel, ml = synth.make_mel(b, 80, int(ml.max()), ml.tolist(), seed=4321)
        mel, ml = torch.from_numpy(mel).cuda(), torch.from_numpy(ml).cuda()
        with torch.no_grad():
            enc, enc_len, _ = m.encoder.forward_mel(mel, ml)
            logits, labels, label_len = m._head(enc, enc_len, want_logits=True)
        t = int(logits.shape[1])
        u = max(1, int(label_len.max()))
        tg, tl = labels[:, :u].contiguous(), label_len.to(torch.int64)
        out = m.align_logits(logits, enc_len, tg, tl)
        want = host_ctc_loss(logits, enc_len, tg, tl)
        got = out["log_likelihood"].cpu().double()
        assert int(out["status"].abs().max()) == 0
        err = float(((got - want).abs() / (1 + want.abs())).max())
        assert err <= 1e-5, err
        ms_align = timed(lambda: m.align_logits(logits, enc_len, tg, tl), args.reps)
        ms_score = timed(lambda: m.align_logits(logits, enc_len, tg, tl, scores_only=True), args.reps)
        ms_greedy = timed(lambda: m._head(enc, enc_len), args.reps)
        ms_host = timed(lambda: host_ctc_loss(logits, enc_len, tg, tl), max(1, args.reps // 2))
        row = dict(batch=b, vocab=int(logits.shape[2]), t_max=t, u_max=u, frames=int(enc_len.sum()), tokens=int(tl.sum()),
                   ms_align=round(ms_align, 3), ms_score_only=round(ms_score, 3), ms_greedy_head=round(ms_greedy, 3),
                   ms_host_ctc_loss_f64=round(ms_host, 3), host_over_score_only=round(ms_host / ms_score, 1),
                   max_rel_err_vs_host=float("%.2e" % err))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
