"""Measure what margin-gated label-exact decoding (ModelCTC.greedy_exact) rests on, on the GPU:

  1. the per-frame spread  max_v d_v - min_v d_v,  d = head logits of the bf16 path - head logits of the split mode, over ragged LibriSpeech-shaped
     batches of five configurations x two weight recipes (synth.make_state_dict, synth.make_stressed_state_dict "trained") x three seeds.  An utterance
     whose smallest bf16 top-2 margin is at least a band >= this spread has the split mode's labels; the default band is twice the worst spread found,
     rounded up to two digits.  Neither mode is code under test: both forwards are the existing ones.
  2. at B = 256 (EfficientConformerCTCSmall): the bf16 step, the split step, and greedy_exact at bands taken from quantiles of min_margin so that
     0, 10, 50 and 100 % of the batch run again.  Recorded, not gated; expected shape 1 + p x (split / bf16).

    python tools/label_exact_band.py [--out profiles/label_exact_band.txt] [--batch 24] [--seeds 1 2 3] [--skip-timing]
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from efficientconformer_amd import ModelCTC, named_config, synth  # noqa: E402

CONFIGS = ["Tiny", "EfficientConformerCTCSmall", "EfficientConformerCTCMedium", "EfficientConformerCTCLarge", "ConformerCTCSmall"]
WEIGHTS = ["synthetic", "trained"]


def model(name, weights, seed):
    cfg = named_config(name)
    m = ModelCTC.from_config(cfg)
    vocab = cfg["tokenizer_params"]["vocab_size"]
    if weights == "synthetic":
        sd = synth.make_state_dict(m.encoder.plan, seed, vocab, prefix="encoder.")
    else:
        sd = synth.make_stressed_state_dict(m.encoder.plan, seed, weights, vocab, prefix="encoder.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda()
    m.encoder.ragged = True
    return m


def logits_of(m, x, x_len, host):
    enc, enc_len, _ = m.encoder(x, x_len, x_len_host=host)
    hm = m.head_margins(enc, enc_len, want_logits=True)
    return hm.logits, hm.frame_margin, enc_len


def round_up_2_digits(v):
    if v <= 0:
        return 0.0
    e = math.floor(math.log10(v)) - 1
    return float(math.ceil(v / 10 ** e - 1e-9) * 10 ** e)


def spread_row(name, weights, seed, batch):
    m = model(name, weights, seed)
    lens = synth.libri_lengths(batch, seed=100 + seed)
    x = torch.from_numpy(synth.make_audio(lens, seed=seed)).cuda()
    x_len = torch.from_numpy(lens).cuda()
    m.encoder.precision = "split"              # pack once for both modes
    ls, ms, out_len = logits_of(m, x, x_len, lens)
    m.encoder.precision = "bf16"
    lb, mb, _ = logits_of(m, x, x_len, lens)
    valid = torch.arange(lb.shape[1], device=lb.device)[None, :] < out_len[:, None]
    d = lb - ls
    spread = (d.max(-1).values - d.min(-1).values)[valid]
    mbv, msv = mb[valid], ms[valid]
    flips = lb.argmax(-1)[valid] != ls.argmax(-1)[valid]
    worst = float(spread.max())
    return {"config": name, "weights": weights, "seed": seed, "frames": int(valid.sum()), "spread_max": worst, "spread_mean": float(spread.mean()),
            "logit_absmax": float(ls[valid].abs().max()), "flips": int(flips.sum()), "flip_margin_max": float(mbv[flips].max()) if bool(flips.any()) else 0.0,
            "bf16_margin_median": float(mbv.median()), "split_margin_median": float(msv.median()),
            "min_margins": (torch.where(valid, mb, torch.full_like(mb, float("inf"))).min(1).values).cpu().numpy()}


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def timing(lines, batch=256, warmup=3, steps=10):
    m = model("EfficientConformerCTCSmall", "synthetic", 0)
    m.encoder.sub_batches = 3
    lens = synth.libri_lengths(batch)
    x = torch.from_numpy(synth.make_audio(lens)).cuda()
    x_len = torch.from_numpy(lens).cuda()
    _, _, rep = m.greedy_exact(x, x_len, band=0.0, x_len_host=lens)           # packs for the split mode
    mm = np.sort(rep["min_margin"].numpy())
    t_bf16 = timed(lambda: m.encode_greedy(x, x_len, x_len_host=lens), warmup, steps)
    m.encoder.precision = "split"
    t_split = timed(lambda: m.encode_greedy(x, x_len, x_len_host=lens), warmup, steps)
    m.encoder.precision = "bf16"
    lines.append("")
    lines.append("cost at B = %d, EfficientConformerCTCSmall, ragged, 3 row ranges, LibriSpeech-shaped lengths (ms per call, %d calls after %d):" % (batch, steps, warmup))
    lines.append("  bf16 step (encode_greedy)            %8.3f" % t_bf16)
    lines.append("  split step (encode_greedy)           %8.3f   (%.2f x bf16)" % (t_split, t_split / t_bf16))
    for share in (0.0, 0.1, 0.5, 1.0):
        k = int(round(share * batch))
        band = 0.0 if k == 0 else (float("inf") if k == batch else float(0.5 * (mm[k - 1] + mm[k])))
        n = int(m.greedy_exact(x, x_len, band=band, x_len_host=lens)[2]["rerun"].numel())
        t = timed(lambda: m.greedy_exact(x, x_len, band=band, x_len_host=lens), warmup, steps)
        lines.append("  greedy_exact, band %-10.4g %3d of %d run again %8.3f   (%.2f x bf16; 1 + p x split / bf16 = %.2f)"
                     % (band, n, batch, t, t / t_bf16, 1 + n / batch * t_split / t_bf16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_exact_band.txt"))
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--configs", nargs="+", default=CONFIGS)
    ap.add_argument("--skip-timing", action="store_true")
    args = ap.parse_args()
    lines = ["per-frame spread of (bf16-path head logits - split-mode head logits), ragged LibriSpeech-shaped batches of %d utterances" % args.batch,
             "(tools/label_exact_band.py; flips = valid frames whose bf16 argmax differs from the split argmax, flip_margin = the largest bf16 margin among them)", "",
             "%-28s %-9s %4s %7s %10s %10s %9s %6s %11s %10s %10s" % ("config", "weights", "seed", "frames", "spread_max", "spread_avg", "|logit|", "flips", "flip_margin",
                                                                 "med_m_bf16", "med_m_split")]
    rows = []
    t0 = time.time()
    for name in args.configs:
        for weights in WEIGHTS:
            for seed in args.seeds:
                r = spread_row(name, weights, seed, args.batch)
                rows.append(r)
                lines.append("%-28s %-9s %4d %7d %10.3e %10.3e %9.2f %6d %11.3e %10.3e %10.3e" % (r["config"], r["weights"], r["seed"], r["frames"], r["spread_max"],
                                                                                             r["spread_mean"], r["logit_absmax"], r["flips"], r["flip_margin_max"],
                                                                                             r["bf16_margin_median"], r["split_margin_median"]))
                print(lines[-1], "  [%.0f s]" % (time.time() - t0), flush=True)
                with open(args.out, "w") as f:          # keep what is measured so far
                    f.write("\n".join(lines) + "\n")
    worst = max(r["spread_max"] for r in rows)
    band = round_up_2_digits(2 * worst)
    lines += ["", "frames in all: %d; worst spread: %.6e (%s, %s, seed %d)" % ((sum(r["frames"] for r in rows), worst) + max(((r["spread_max"], r["config"], r["weights"], r["seed"])
                                                                                                                           for r in rows))[1:]),
              "worst flip margin: %.6e (every flip lies under the spread of its frame)" % max(r["flip_margin_max"] for r in rows),
              "default band = 2 x worst spread, rounded up to two digits: %g" % band, "",
              "share of utterances whose smallest bf16 margin is under that band (= would run again), per configuration and weight recipe:"]
    for name in args.configs:
        for weights in WEIGHTS:
            mm = np.concatenate([r["min_margins"] for r in rows if r["config"] == name and r["weights"] == weights])
            lines.append("  %-28s %-9s %5.1f %%  (median smallest margin %.3e)" % (name, weights, 100.0 * float((~(mm >= band)).mean()), float(np.median(mm))))
    if not args.skip_timing:
        timing(lines)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-24:]))


if __name__ == "__main__":
    main()
