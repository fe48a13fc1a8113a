#!/usr/bin/env python3
"""CTC prefix beam search cost (effconf_ctc_beam): EfficientConformerCTC-Small (synthetic weights, bf16 path) on ragged
LibriSpeech-like mel batches (the length generator of tools/rnnt_beam_bench.py), B = 16 / 64 / 256 and beams 1 / 4 / 16.  Per
configuration: ms per decode of the head's logits (median of timed runs), the greedy head (fc + argmax + collapse) of the same batch
and the encoder forward for scale, and the candidates scored per frame.

    python tools/ctc_beam_bench.py [--batches 16,64,256] [--beams 1,4,16] [--reps 5] [--json OUT]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,64,256")
    ap.add_argument("--beams", default="1,4,16")
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
            logits, _, _ = m._head(enc, enc_len, want_logits=True)
        t = int(logits.shape[1])
        assert t <= 200, t
        ms_enc = timed(lambda: m.encoder.forward_mel(mel, ml), args.reps)
        ms_greedy = timed(lambda: m._head(enc, enc_len), args.reps)
        frames = int(enc_len.sum())
        for beam in [int(x) for x in args.beams.split(",")]:
            m.decode_logits_beam(logits, enc_len, beam)
            tr = m.last_beam_trace()
            ms = timed(lambda: m.decode_logits_beam(logits, enc_len, beam), args.reps)
            row = dict(batch=b, beam=beam, frames=frames, t_max=t, ms_beam=round(ms, 3), ms_greedy_head=round(ms_greedy, 3),
                       beam_over_greedy=round(ms / ms_greedy, 2), ms_encoder=round(ms_enc, 3),
                       candidates_per_frame=round(sum(u["candidates"] for u in tr) / frames, 2),
                       us_per_frame_longest=round(1e3 * ms / t, 2))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
