#!/usr/bin/env python3
"""Cost of the CTC prefix beam search with neural-LM shallow fusion (effconf_ctc_beam_lm): B = 256 LibriSpeech-shaped synthetic peaked logits with
vocabulary 1000 (tools/lm_bench.py's generator, so the plain search's time is comparable with profiles/lm_bench.txt), beams 4 / 16, with synthetic LSTM LMs
at 1024 x 2 and 4096 x 3 (LM-RNN's widths).  Per configuration, medians of `--reps` timed runs after a warm-up, all in this run on the same inputs:
  * the fused decode (``decode_logits_beam_lm``), its search launches (an LM step runs between two of them), the LM evaluations it asked for in all
    (one per prefix that entered a beam) and per round, and the share of the GPU kernel time spent in the LM's kernels (torch.profiler over one more run);
  * the plain search (``decode_logits_beam``) and the plain search + ``rescore_nbest`` - the two routes that existed - and the LM evaluations rescoring
    makes (one per token of every hypothesis);
  * whether the fused best and the rescored best differ, per utterance (they answer different questions; this is not an accuracy figure).

    python tools/ctc_beam_lm_bench.py [--batch 256] [--beams 4,16] [--lms 1024x2,4096x3] [--reps 3] [--out profiles/ctc_beam_lm_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientconformer_amd import LanguageModel, ModelCTC, named_config, synth  # noqa: E402

VOCAB = 1000
TOKENS_PER_FRAME = 0.45
LM_WEIGHT = 0.5


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def peaked_logits(batch, seed=1234):
    """tools/lm_bench.py's inputs: a random transcript per utterance at random frames of blank-dominated logits (+ noise); 40 ms frames."""
    frames = (synth.libri_lengths(batch, seed) // 640).astype(np.int64)
    rng = np.random.Generator(np.random.PCG64(seed))
    t = int(frames.max())
    logits = rng.standard_normal((batch, t, VOCAB)).astype(np.float32)
    logits[:, :, 0] += 7.0
    for b, n in enumerate(frames):
        at = np.sort(rng.choice(int(n), max(1, int(TOKENS_PER_FRAME * n)), replace=False))
        logits[b, at, 0] -= 7.0
        logits[b, at, rng.integers(1, VOCAB, len(at))] += 6.0
    return logits, frames


def kernel_shares(fn):
    """{lm, search, other}: summed GPU time (us) of the kernels of one call of fn, by name."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    tot = {"lm": 0.0, "search": 0.0, "other": 0.0}
    for e in prof.key_averages():
        us = float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))
        key = "search" if "ctc_beam" in e.key else ("lm" if "lm_" in e.key else "other")
        tot[key] += us
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--beams", default="4,16")
    ap.add_argument("--lms", default="1024x2,4096x3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    ctc = ModelCTC.from_config(named_config("EfficientConformerCTCSmall"))
    logits, frames = peaked_logits(a.batch)
    logits, frames = torch.from_numpy(logits).cuda(), torch.from_numpy(frames).cuda()
    say("ctc_beam_lm_bench: %s, B %d, vocabulary %d, T %d (mean %.0f frames), lm_weight %.2f, reps %d (median [min .. max] ms)"
        % (torch.cuda.get_device_name(0), a.batch, VOCAB, logits.shape[1], float(frames.float().mean()), LM_WEIGHT, a.reps))
    for spec in a.lms.split(","):
        h, layers = (int(x) for x in spec.split("x"))
        params = dict(arch="RNN", vocab_size=VOCAB, dim_model=h, num_layers=layers)
        lm = LanguageModel(params)
        lm.load_state_dict({k: torch.from_numpy(t) for k, t in synth.make_lm_state_dict(params, 0).items()})
        lm = lm.cuda()
        for beam in [int(x) for x in a.beams.split(",")]:
            say("--- LM %d x %d, beam %d" % (h, layers, beam))
            tokens, token_len, am = ctc.decode_logits_beam(logits, frames, beam)
            pm = timed(lambda: ctc.decode_logits_beam(logits, frames, beam), a.reps)
            say("plain search (decode_logits_beam): %.2f [%.2f .. %.2f] ms" % pm)
            best, _, _ = ctc.rescore_nbest(tokens, token_len, am, lm=lm, lm_weight=LM_WEIGHT)
            rm = timed(lambda: ctc.rescore_nbest(*ctc.decode_logits_beam(logits, frames, beam), lm=lm, lm_weight=LM_WEIGHT), a.reps)
            resc_evals = int(token_len.sum())
            say("plain search + rescore_nbest: %.2f [%.2f .. %.2f] ms; LM evaluations %d (one per token of %d hypotheses)" % (rm + (resc_evals, a.batch * beam)))
            fused = lambda: ctc.decode_logits_beam_lm(logits, frames, beam, lm=lm, lm_weight=LM_WEIGHT)
            ft, fl = fused()[:2]
            rounds = ctc.last_beam_rounds()
            evals = sum(u["lm_rows"] for u in ctc.last_beam_trace())
            fm = timed(fused, a.reps)
            sh = kernel_shares(fused)
            allk = max(sum(sh.values()), 1e-9)
            say("fused search (decode_logits_beam_lm): %.2f [%.2f .. %.2f] ms; search launches %s (chunks %d); LM evaluations %d = %.1f per utterance, "
                "%.1f live columns per LM step of %d; LM kernels %.1f %% of the GPU kernel time (search %.1f %%)"
                % (fm + (rounds, len(rounds), evals, evals / a.batch, evals / max(sum(rounds), 1), a.batch * beam // len(rounds), 100 * sh["lm"] / allk,
                         100 * sh["search"] / allk)))
            idx = torch.arange(a.batch, device=tokens.device)
            differ = int(((tokens[idx, best] != ft[:, 0]).any(dim=1) | (token_len[idx, best] != fl[:, 0])).sum())
            say("ratios: fused / plain %.1f, fused / (plain + rescoring) %.2f, LM evaluations fused / rescoring %.3f; best hypothesis differs from the "
                "rescored one on %d of %d utterances" % (fm[0] / pm[0], fm[0] / rm[0], evals / max(resc_evals, 1), differ, a.batch))
        del lm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
