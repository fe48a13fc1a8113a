#!/usr/bin/env python3
"""N-best rescoring cost of the LSTM language model (effconf_lm_score, csrc/lm.hip): B = 256 utterances x beam 16 = 4096 hypotheses, the n-best
of the CTC beam search itself on LibriSpeech-shaped synthetic logits (synth.libri_lengths -> frames of 40 ms; a transcript of ~0.45 tokens per
frame written into blank-dominated, peaked logits with vocabulary 1000), scored by
  * (H 1024, L 2, V 1000) and
  * LM-RNN (configs/LM-RNN.json: 4096 x 3, V 1000),
both on synthetic weights.  Timed with a host clock around work that ends in a device synchronise, medians of `--reps` runs after a warm-up:
  * ``LanguageModel.score`` on the 4096 hypotheses trimmed to the longest one (the class's chunking included), and ``ModelCTC.rescore_nbest`` on the
    n-best as the search returns it (padded to the T frames of the logits): the call users make;
  * a PyTorch-ROCm fp32 baseline on the same inputs - what a user could do before: nn.Embedding + nn.LSTM + nn.Linear + log_softmax + gather +
    masked sum, `--torch-chunk` hypotheses at a time (the (n, U, V) logits of a chunk exist in memory); its scores are compared with the kernels' first;
  * ``ModelCTC.decode_logits_beam`` alone, the search that produced the n-best.
Reported per model: the median, the share of the fp32 matrix peak (157.3 TFLOP/s) reached on the useful work (2 flops per weight and scored token:
4H * H for layer 0, 4H * 2H per further layer, V * H for the head) and on the N x u_max rectangle ("issued": what a schedule that runs every
sequence for u_max steps would issue; column tiles whose sequences are all finished are skipped, so this share is an upper bound of the pipe's real
use), and the weight bytes a step streams at least once.

    python tools/lm_bench.py [--batch 256] [--beam 16] [--reps 10] [--models small,lmrnn] [--out profiles/lm_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientconformer_amd import LanguageModel, ModelCTC, named_config, synth  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12          # v_mfma_f32_16x16x4_f32, MI355X spec
MODELS = {"small": dict(arch="RNN", vocab_size=1000, dim_model=1024, num_layers=2),
          "lmrnn": dict(arch="RNN", vocab_size=1000, dim_model=4096, num_layers=3)}
TOKENS_PER_FRAME = 0.45
VOCAB = 1000


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
    """(logits (B, T, V) f32, frames (B,) i64): a random transcript per utterance at random frames of blank-dominated logits (+ noise)."""
    frames = (synth.libri_lengths(batch, seed) // 640).astype(np.int64)            # 40 ms per encoder frame
    rng = np.random.Generator(np.random.PCG64(seed))
    t = int(frames.max())
    logits = rng.standard_normal((batch, t, VOCAB)).astype(np.float32)
    logits[:, :, 0] += 7.0
    for b, n in enumerate(frames):
        at = np.sort(rng.choice(int(n), max(1, int(TOKENS_PER_FRAME * n)), replace=False))
        logits[b, at, 0] -= 7.0
        logits[b, at, rng.integers(1, VOCAB, len(at))] += 6.0
    return logits, frames


def torch_scores(lm, tokens, lens, chunk):
    out = []
    with torch.no_grad():
        for lo in range(0, tokens.shape[0], chunk):
            y, n = tokens[lo:lo + chunk].long(), lens[lo:lo + chunk]
            x = torch.nn.functional.pad(y, (1, 0))[:, :-1]
            h, _ = lm.decoder.rnn(lm.decoder.embedding(x))
            lp = torch.log_softmax(lm.fc(h) / lm.lm_tmp, dim=-1).gather(2, y[:, :, None])[:, :, 0]
            mask = torch.arange(y.shape[1], device=y.device)[None, :] < n[:, None]
            out.append((lp * mask).sum(dim=1))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--beam", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--models", default="small,lmrnn")
    ap.add_argument("--torch-chunk", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say("lm_bench: %s, B %d x beam %d, vocabulary %d, reps %d (median [min .. max] ms)" % (torch.cuda.get_device_name(0), a.batch, a.beam, VOCAB, a.reps))
    ctc = ModelCTC.from_config(named_config("EfficientConformerCTCSmall"))
    logits, frames = peaked_logits(a.batch)
    logits, frames = torch.from_numpy(logits).cuda(), torch.from_numpy(frames).cuda()
    tokens, token_len, am = ctc.decode_logits_beam(logits, frames, a.beam)
    say("decode_logits_beam alone (T %d): %.2f [%.2f .. %.2f] ms" % ((logits.shape[1],) + timed(lambda: ctc.decode_logits_beam(logits, frames, a.beam), a.reps)))
    n = a.batch * a.beam
    u_max = int(token_len.max())
    flat, flat_len = tokens.reshape(n, -1)[:, :max(u_max, 1)].contiguous(), token_len.reshape(n).long()
    total_tokens = int(flat_len.sum())
    say("hypotheses: %d, u_max %d, tokens %d (mean %.1f), frames per utterance mean %.0f" % (n, u_max, total_tokens, total_tokens / n, float(frames.float().mean())))
    for name in a.models.split(","):
        params = MODELS[name]
        h, layers, v = params["dim_model"], params["num_layers"], params["vocab_size"]
        lm = LanguageModel(params)
        lm.load_state_dict({k: torch.from_numpy(t) for k, t in synth.make_lm_state_dict(params, 0).items()})
        lm = lm.cuda()
        weights = 4 * h * h * (2 * layers - 1) + v * h
        say("--- %s: H %d, L %d, V %d; weight bytes per step %.1f MB; %d hypotheses per native call" % (name, h, layers, v, weights * 4 / 1e6, lm.chunk_size()))
        score = lm.score(flat, flat_len)
        torch.cuda.synchronize()
        med, lo, hi = timed(lambda: lm.score(flat, flat_len), a.reps)
        useful, issued = 2.0 * weights * total_tokens, 2.0 * weights * n * u_max
        say("LanguageModel.score: %.2f [%.2f .. %.2f] ms; %.1f TFLOP useful = %.1f %% of the fp32 matrix peak, %.1f TFLOP issued = %.1f %%"
            % (med, lo, hi, useful / 1e12, 100 * useful / (med * 1e-3) / FP32_MATRIX_PEAK, issued / 1e12, 100 * issued / (med * 1e-3) / FP32_MATRIX_PEAK))
        rm, rl, rh = timed(lambda: ctc.rescore_nbest(tokens, token_len, am, lm=lm, lm_weight=0.5), a.reps)
        say("ModelCTC.rescore_nbest (the n-best as the search returns it, padded to T %d: no trim, no host copy of the lengths): %.2f [%.2f .. %.2f] ms"
            % (tokens.shape[2], rm, rl, rh))
        for chunk in (a.torch_chunk, a.torch_chunk // 4, a.torch_chunk // 16):
            try:
                base = torch_scores(lm, flat, flat_len, chunk)
                d = (base - score).abs()
                say("torch fp32 baseline agrees: max |score difference| %.3g (largest |score| %.1f)" % (float(d.max()), float(score.abs().max())))
                bm, bl, bh = timed(lambda: torch_scores(lm, flat, flat_len, chunk), a.reps)
                say("torch fp32 baseline (nn.LSTM + Linear + log_softmax + gather, %d per chunk): %.2f [%.2f .. %.2f] ms = %.2f x the native call"
                    % (chunk, bm, bl, bh, bm / med))
                break
            except Exception as e:                  # the baseline is a comparison, not the product: say so, try smaller chunks, go on
                say("torch fp32 baseline failed at %d per chunk: %s: %s" % (chunk, type(e).__name__, str(e)[:300]))
        del lm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
