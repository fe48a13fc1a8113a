#!/usr/bin/env python3
"""Cost of the RNN-T beam search with neural-LM shallow fusion (effconf_rnnt_beam_lm): Transducer-Medium on the native encoder's output for a ragged
LibriSpeech-like mel batch (B = 256), beams 4 / 16, with synthetic LSTM LMs of the transducer's vocabulary at 1024 x 2 and 4096 x 3 (LM-RNN's widths).
Per configuration: ms per batch (median of timed runs), search launches (an LM step runs between two of them), chunks of the batch, the share of the GPU
kernel time spent in the LM's kernels (torch.profiler over one more run: lm_* against rnnt_beam_lm_kernel and the rest), capped utterances, and beside
it the plain beam search (effconf_rnnt_beam) of the same batch - of this tree and, with --parent DIR, of another checkout's package (a directory that
holds a built ``efficientconformer_amd``; the plain search is then timed in a fresh child process that imports from there).

    python tools/rnnt_beam_lm_bench.py [--batch 256] [--beams 4,16] [--lms 1024x2,4096x3] [--reps 3] [--parent DIR] [--out profiles/rnnt_beam_lm_bench.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = "EfficientConformerTransducerMedium"


def build(pkg, blank_bias):
    cfg = pkg.named_config(MODEL)
    m = pkg.Transducer.from_config(cfg)
    sd = pkg.synth.make_state_dict(m.encoder.plan, 0, None, prefix="encoder.")
    sd.update(pkg.synth.make_transducer_state_dict(m.encoder.plan.dim_out, cfg["decoder_params"], cfg["joint_params"], 0, blank_bias=blank_bias))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda(), cfg["decoder_params"]["vocab_size"]


def encoded(pkg, m, batch):
    """The native encoder's output for seeded mel of LibriSpeech-like lengths (1.5 .. 16 s, 10 ms mel frames), as tools/rnnt_beam_bench.py."""
    ml = np.maximum(16, pkg.synth.libri_lengths(batch, seed=11) // 160).astype(np.int64)
    mel, ml = pkg.synth.make_mel(batch, 80, int(ml.max()), ml.tolist(), seed=4321)
    with torch.no_grad():
        f, fl, _ = m.encoder.forward_mel(torch.from_numpy(mel).cuda(), torch.from_numpy(ml).cuda())
    return f.float().contiguous(), fl.to(torch.int64)


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


def plain_rows(pkg, batch, beams, reps, blank_bias, tag):
    m, _ = build(pkg, blank_bias)
    f, fl = encoded(pkg, m, batch)
    rows = []
    for beam in beams:
        out = m.decode_encoded_beam(f, fl, beam)
        ms = timed(lambda: m.decode_encoded_beam(f, fl, beam), reps)
        rows.append(dict(search="plain (%s)" % tag, batch=batch, beam=beam, frames=int(fl.sum()), ms=round(ms, 2), status_nonzero=int((out[3] != 0).sum()),
                         tokens=int(out[1].sum())))
    return rows


def kernel_shares(fn):
    """{lm, search, other}: summed GPU time of the kernels of one call of fn, by name."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    tot = {"lm": 0.0, "search": 0.0, "other": 0.0}
    for e in prof.key_averages():
        us = float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))
        key = "search" if "rnnt_beam" in e.key else ("lm" if "lm_" in e.key else "other")
        tot[key] += us
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--beams", default="4,16")
    ap.add_argument("--lms", default="1024x2,4096x3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blank-bias", type=float, default=1.2)
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--parent", default=None, help="a checkout of another commit with its library built: its plain search is timed beside")
    ap.add_argument("--plain-only", default=None, help="(internal) time the plain search with the package under this directory and print JSON rows")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    beams = [int(x) for x in args.beams.split(",")]
    sys.path.insert(0, args.plain_only or ROOT)
    import efficientconformer_amd as pkg
    import efficientconformer_amd.synth  # noqa: F401  (pkg.synth)
    if args.plain_only:
        assert os.path.realpath(os.path.dirname(pkg.__file__)).startswith(os.path.realpath(args.plain_only)), pkg.__file__
        print("ROWS " + json.dumps(plain_rows(pkg, args.batch, beams, args.reps, args.blank_bias, "parent")))
        return
    lines = []

    def say(row):
        s = json.dumps(row)
        lines.append(s)
        print(s, flush=True)
    if args.parent:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", os.path.abspath(args.parent), "--batch", str(args.batch), "--beams", args.beams,
                            "--reps", str(args.reps), "--blank-bias", str(args.blank_bias)], capture_output=True, text=True, timeout=900)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("ROWS ")]
        if r.returncode != 0 or not got:
            sys.exit("the parent's plain search failed:\n" + r.stderr[-2000:])
        for row in json.loads(got[0][5:]):
            say(row)
    for row in plain_rows(pkg, args.batch, beams, args.reps, args.blank_bias, "this tree"):
        say(row)
    m, vocab = build(pkg, args.blank_bias)
    f, fl = encoded(pkg, m, args.batch)
    for spec in args.lms.split(","):
        dim, layers = (int(x) for x in spec.split("x"))
        params = dict(arch="RNN", vocab_size=vocab, dim_model=dim, num_layers=layers)
        lm = pkg.LanguageModel(params)
        lm.load_state_dict({k: torch.from_numpy(t) for k, t in pkg.synth.make_lm_state_dict(params, 0).items()})
        lm = lm.cuda()
        for beam in beams:
            run = lambda: m.decode_encoded_beam_lm(f, fl, beam, lm=lm, lm_weight=args.lm_weight)
            out = run()
            rounds = m.last_beam_rounds()
            st = m.last_beam_stats().astype(np.int64)
            ms = timed(run, args.reps)
            share = kernel_shares(run)
            total = sum(share.values())
            say(dict(search="fused", lm=spec, lm_weight=args.lm_weight, batch=args.batch, beam=beam, frames=int(fl.sum()), ms=round(ms, 2), chunks=len(rounds),
                     search_launches=int(sum(rounds)), lm_evaluations=int(st[:, 1].sum()), expansions=int(st[:, 2].sum()),
                     kernel_ms=round(total / 1e3, 2), lm_share_of_kernel_time=round(share["lm"] / total, 4) if total else None,
                     search_share_of_kernel_time=round(share["search"] / total, 4) if total else None,
                     status_nonzero=int((out[3] != 0).sum()), tokens=int(out[1].sum())))
        del lm
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# tools/rnnt_beam_lm_bench.py: %s, blank bias %.1f, one JSON row per configuration\n" % (MODEL, args.blank_bias))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
