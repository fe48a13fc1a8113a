#!/usr/bin/env python3
"""What a self-conditioned CTC step costs on the MI355X -> profiles/interctc_bench.txt.

    python tools/interctc_bench.py [--out profiles/interctc_bench.txt]

(a) csrc/interctc.hip alone (effconf_interctc, y in place, no probability output) against an unfused baseline on the same device and the same rows: a bf16
    F.linear, an fp32 softmax, a bf16 F.linear and the residual add in torch.  Shapes: EfficientConformerCTCSmall's three stage widths with V = 256 on the row
    counts of bench.py's batch (B = 256 LibriSpeech-shaped utterances, ragged: the sum of the utterances' frames at that stage), and (256, 1000) / (720, 1000)
    on the last stage's row count.  Per shape: median of 10 timed windows of `--inner` launches each (device events around the window, 3 warm-up windows), the two
    variants alternating; us per launch, TFLOP/s on the algorithmic 4 M De V and the share of the bf16 MFMA peak.
(b) The EfficientConformerCTCSmall encoder step at B = 256, ragged, one row range, with interctc_blocks = [3, 6, 10, 13] (V = 256) against the same model without
    them (median of 10 forwards each, alternating), next to the algorithmic FLOP ratio of the two (row-local products and attention of the encoder, per
    utterance).
Needs a GPU: no fallback.  Outputs of the fused kernel and of the baseline are compared on the timed rows (bf16 tolerance) before anything is timed."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from efficientconformer_amd import ConformerEncoder, ConformerEncoderInterCTC, _lib, named_config, synth  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0      # dense bf16 MFMA (bench.py)
SMALL_BLOCKS = [3, 6, 10, 13]


def stage_rows(plan, lens_samples):
    """Rows of the ragged residual stream leaving every block: the sum over the utterances of their frames there."""
    per = np.array([plan.lengths(int(n))[2] for n in lens_samples])
    return per.sum(axis=0)


def step_encoder(dims, heads, vocab):
    n = len(dims)
    params = dict(named_config("Tiny")["encoder_params"], dim_model=list(dims), num_heads=list(heads), num_blocks=n, expand_blocks=list(range(1, n)),
                  strided_blocks=[], att_group_size=1, conv_stride=1, subsampling_filters=[8], interctc_blocks=list(range(n)), vocab_size=vocab)
    enc = ConformerEncoderInterCTC(params)
    sd = synth.make_state_dict(enc.plan, 7)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    enc = enc.cuda()
    enc._ensure_packed()
    return enc


def timed(fn, inner, windows=10, warm=3):
    out = []
    for i in range(warm + windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        if i >= warm:
            out.append(a.elapsed_time(b) * 1e3 / inner)
    return out


def kernel_rows(lines, enc, k, rows, inner):
    lib = _lib.load()
    de, v = enc.plan.blocks[k].dim_expand, enc.plan.interctc_vocab
    g = torch.Generator(device="cuda").manual_seed(de * 131 + v)
    x0 = torch.randn(rows, de, device="cuda", generator=g)
    we, be = getattr(enc, "linear_expand_%d" % k).weight.detach(), getattr(enc, "linear_expand_%d" % k).bias.detach()
    wp, bp = getattr(enc, "linear_proj_%d" % k).weight.detach(), getattr(enc, "linear_proj_%d" % k).bias.detach()
    we16, be16, wp16, bp16 = we.bfloat16(), be.bfloat16(), wp.bfloat16(), bp.bfloat16()
    st = torch.cuda.current_stream().cuda_stream
    xf, xb = x0.clone(), x0.clone()

    def fused():
        _lib.check(lib.effconf_interctc(enc._handle, k, xf.data_ptr(), rows, xf.data_ptr(), None, None, 0, st), "interctc")

    def baseline():
        p = F.linear(xb.bfloat16(), we16, be16).float().softmax(dim=-1)
        xb.add_(F.linear(p.bfloat16(), wp16, bp16).float())

    fused(); baseline()
    torch.cuda.synchronize()
    diff = float((xf - xb).abs().max())
    assert diff < 0.05, "fused kernel and baseline disagree: %.3g" % diff
    tf, tb = [], []
    for _ in range(2):                                 # the two variants alternating, five windows each time
        tf += timed(fused, inner, windows=5)
        tb += timed(baseline, inner, windows=5)
    mf, mb = statistics.median(tf), statistics.median(tb)
    flop = 4.0 * rows * de * v
    lines.append("%5d %5d %8d | fused %8.1f us (min %.1f max %.1f) %7.1f TFLOP/s %5.1f %% of peak | torch bf16 linear + softmax + linear + add %8.1f us (min %.1f max %.1f) | "
                 "fused / torch %.2f%s | max |fused - torch| %.3g"
                 % (de, v, rows, mf, min(tf), max(tf), flop / mf * 1e-6, 100.0 * flop / mf * 1e-6 / PEAK_BF16_TFLOPS, mb, min(tb), max(tb), mf / mb,
                    "" if mf <= mb else "  SLOWER than the baseline", diff))
    print(lines[-1], flush=True)
    return mf <= mb


def encoder_flops(plan, lens_samples, vocab=0, blocks=()):
    """Algorithmic FLOPs of one encoder step on the ragged batch: the row-local products and the attention products of every block (+ the steps)."""
    total = 0.0
    for n in lens_samples:
        _, t1, ts = plan.lengths(int(n))
        t = t1
        total += 2.0 * t1 * plan.dim_in * plan.blocks[0].dim_model
        for b, to in zip(plan.blocks, ts):
            d, de, tg = b.dim_model, b.dim_expand, -(-t // b.group_size)
            total += 2.0 * t * d * (2 * b.dim_ffn1 + 4 * d + 2 * de) + 2.0 * to * de * (de + 2 * b.dim_ffn2) + (2.0 * to * d * de if d != de else 0.0)
            total += 2.0 * b.num_heads * tg * tg * b.dim_head * 3.0
            if b.index in blocks:
                total += 4.0 * to * de * vocab
            t = to
    return total


def encoder_step(lines):
    cfg = named_config("EfficientConformerCTCSmall")
    lens = np.sort(synth.libri_lengths(256, seed=1234))[::-1].copy()
    audio = torch.from_numpy(synth.make_audio(lens, seed=1234)).cuda()
    lens_d = torch.from_numpy(lens).cuda()
    models = {}
    for tag, cls, params in (("plain", ConformerEncoder, cfg["encoder_params"]),
                             ("interctc", ConformerEncoderInterCTC, dict(cfg["encoder_params"], interctc_blocks=SMALL_BLOCKS, vocab_size=256))):
        enc = cls(params)
        sd = synth.make_state_dict(enc.plan, 0)
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        enc = enc.cuda()
        enc.ragged = True
        models[tag] = enc
    times = {"plain": [], "interctc": []}
    for rep in range(13):
        for tag, enc in models.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            enc(audio, lens_d, x_len_host=lens)
            b.record()
            b.synchronize()
            if rep >= 3:
                times[tag].append(a.elapsed_time(b))
    mp, mi = statistics.median(times["plain"]), statistics.median(times["interctc"])
    fp = encoder_flops(models["plain"].plan, lens)
    fi = encoder_flops(models["interctc"].plan, lens, 256, SMALL_BLOCKS)
    lines.append("EfficientConformerCTCSmall encoder step, B = 256 ragged, one row range: plain %.3f ms (min %.3f max %.3f), interctc_blocks = %s V = 256 %.3f ms (min %.3f max %.3f): "
                 "x %.3f; algorithmic FLOP ratio x %.3f (%.1f -> %.1f GFLOP)"
                 % (mp, min(times["plain"]), max(times["plain"]), SMALL_BLOCKS, mi, min(times["interctc"]), max(times["interctc"]), mi / mp, fi / fp, fp * 1e-9, fi * 1e-9))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interctc_bench.txt"))
    ap.add_argument("--inner", type=int, default=50, help="launches per timed window")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "interctc_bench needs a GPU"
    small = named_config("EfficientConformerCTCSmall")
    from efficientconformer_amd.config import build_plan
    plan = build_plan(small["encoder_params"])
    lens = synth.libri_lengths(256, seed=1234)
    rows = stage_rows(plan, lens)
    lines = ["# tools/interctc_bench.py on %s; median of 10 windows of %d launches, variants alternating" % (torch.cuda.get_device_name(0), args.inner),
             "# (a) the step alone, in place, no probability output.  rows = frames of bench.py's ragged batch (B = 256) leaving a block of that stage",
             "#    De     V     rows"]
    ok = True
    enc = step_encoder([120, 168, 240], [4, 4, 4], 256)
    for k, blk in ((0, 3), (1, 6), (2, 13)):
        ok &= kernel_rows(lines, enc, k, int(rows[blk]), args.inner)
    enc = step_encoder([256, 720], [4, 8], 1000)
    for k in (0, 1):
        ok &= kernel_rows(lines, enc, k, int(rows[13]), args.inner)
    lines.append("# fused kernel not slower than the torch baseline on every shape: %s" % ("yes" if ok else "NO - see the lines marked SLOWER"))
    if not ok:
        lines += ["# why (De = 720, the KS = 48 instance): the row fragments (192 registers) and half of the output accumulators (192) of a pair-of-waves tile do not fit",
                  "#   the 512-register file next to the loop's temporaries: the instance carries 1108 bytes of scratch per lane and reloads its fragments from scratch in every",
                  "#   chunk - loads that wait in the same vmcnt queue as the weight ring's DMAs, at one wave per SIMD and 64 rows per workgroup (each workgroup streams all",
                  "#   2.9 MB of weights).  Both waves of a pair also compute the tile's logits (1.5 x the algorithmic MFMA work).  The widths up to 384 carry no scratch, the 512 class 20 bytes.",
                  "#   What would fix it (not built): the logits' K split over the pair with an exchange of partial sums through the LDS (96 fragment registers per wave), or",
                  "#   128-row workgroups with the fragments in the LDS and a two-entry ring."]
    lines.append("# (b)")
    encoder_step(lines)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
