#!/usr/bin/env python3
"""RNN-T beam search cost (effconf_rnnt_beam): Transducer-Medium with blank bias 1.2 on the native encoder's output for ragged
LibriSpeech-like mel batches, B = 16 / 64 / 256 and beams 4 / 16.  Per configuration: ms per decode (median of timed runs), evaluation batches per
frame, the share of evaluated hypotheses never popped, beam_eval_batch 1 against 16, and the greedy decode of the same batch for scale.

    python tools/rnnt_beam_bench.py [--batches 16,64,256] [--beams 4,16] [--reps 3] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientconformer_amd import Transducer, named_config, synth  # noqa: E402


def build(blank_bias):
    cfg = named_config("EfficientConformerTransducerMedium")
    m = Transducer.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, 0, None, prefix="encoder.")
    sd.update(synth.make_transducer_state_dict(m.encoder.plan.dim_out, cfg["decoder_params"], cfg["joint_params"], 0, blank_bias=blank_bias))
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
    ap.add_argument("--beams", default="4,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    m = build(1.2)
    rows = []
    for b in [int(x) for x in args.batches.split(",")]:
        # the native encoder's output for seeded mel of LibriSpeech-like lengths (1.5 .. 16 s, 10 ms mel frames)
        ml = np.maximum(16, synth.libri_lengths(b, seed=11) // 160).astype(np.int64)
        mel, ml = synth.make_mel(b, 80, int(ml.max()), ml.tolist(), seed=4321)
        with torch.no_grad():
            f, fl, _ = m.encoder.forward_mel(torch.from_numpy(mel).cuda(), torch.from_numpy(ml).cuda())
        f, fl = f.float().contiguous(), fl.to(torch.int64)
        t = int(f.shape[1])
        greedy = timed(lambda: m.decode_encoded(f, fl), args.reps)
        for beam in [int(x) for x in args.beams.split(",")]:
            res = {}
            for nb in (16, 1):
                m.set_decode_option("beam_eval_batch", nb)
                out = m.decode_encoded_beam(f, fl, beam)
                st = m.last_beam_stats().astype(np.int64)
                ms = timed(lambda: m.decode_encoded_beam(f, fl, beam), args.reps if nb == 16 else 1)
                res[nb] = (ms, st, out)
            m.set_decode_option("beam_eval_batch", 16)
            (ms16, st, out16), (ms1, st1, out1) = res[16], res[1]
            same = torch.equal(out16[0], out1[0]) and torch.equal(out16[2], out1[2])
            frames = int(st[:, 3].sum())
            row = dict(batch=b, beam=beam, frames=frames, t_max=t, ms_eval_batch_16=round(ms16, 2), ms_eval_batch_1=round(ms1, 2),
                       ms_greedy=round(greedy, 2), beam_over_greedy=round(ms16 / greedy, 2),
                       eval_batches_per_frame=round(float(st[:, 0].sum()) / frames, 3),
                       evaluated_per_frame=round(float(st[:, 1].sum()) / frames, 3),
                       expansions_per_frame=round(float(st[:, 2].sum()) / frames, 3),
                       evaluated_never_popped=round(1.0 - float(st[:, 2].sum()) / float(st[:, 1].sum()), 4),
                       tokens_per_frame=round(float(out16[1].sum()) / frames, 3),
                       status_nonzero=int((out16[3] != 0).sum()), eval_batch_1_identical=bool(same))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
