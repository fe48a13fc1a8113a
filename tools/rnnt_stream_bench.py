#!/usr/bin/env python3
"""What a streaming Transducer push costs on the MI355X -> profiles/rnnt_stream_bench.txt.

    python tools/rnnt_stream_bench.py [--out profiles/rnnt_stream_bench.txt] [--streams 1 16 64] [--chunks 24 48 96] [--seconds 10] [--repeats 5]

EfficientConformerTransducer-Medium, causal (unlimited left context), synthetic weights with the blank bias 1.2 of bench.py (about one token per three encoder
frames); 1 / 16 / 64 streams that all receive the same number of mel frames per push (24 / 48 / 96 frames = 0.24 / 0.48 / 0.96 s) until `--seconds` of audio
are in.  Per configuration, per push (host time around a synchronised call, so the Python staging, the id / length copies and the D2H copy of the tokens are
in it):
  encoder      ``StreamingEncoder.push_mel`` of the session
  decode       the resumed greedy decode of the push's new encoder frames (``StreamingTransducer._decode``: effconf_rnnt_greedy_resume + the token lists)
  tokens       emitted per push and stream
  whole        what the session replaces: ``decode_encoded`` of every stream's whole prefix of encoder frames at the same points (the route the library picks
               for the batch: per-utterance kernel at 1 stream, the 8 x 8 x 2 cluster decode from 16) - the mean over the pushes and the last, longest one
Each figure: the median over `--repeats` passes through the whole utterance, with the spread (max - min) / median of the passes beside it.  The first pass
(allocations, the positional tables) is not counted.  Needs a GPU: no fallback."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from efficientconformer_amd import Transducer, _lib, named_config, synth  # noqa: E402

BLANK_BIAS = 1.2


def make_model():
    cfg = named_config("EfficientConformerTransducerMedium")
    cfg["encoder_params"] = dict(cfg["encoder_params"], causal=True)
    m = Transducer.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, 0, None, prefix="encoder.")
    sd.update(synth.make_transducer_state_dict(m.encoder.plan.dim_out, cfg["decoder_params"], cfg["joint_params"], 0, blank_bias=BLANK_BIAS))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, 1e3 * (time.perf_counter() - t0)


def session_pass(m, mel, chunk, frames):
    """-> mean encoder ms per push, mean decode ms per push, tokens per push and stream, the encoder rows of every push."""
    B = mel.shape[0]
    sess = m.open_stream(B, max_frames=frames)
    enc_ms, dec_ms, ntok, outs = [], [], 0, []
    for lo in range(0, frames, chunk):
        n = min(chunk, frames - lo)
        (out, out_len), te = timed(lambda: sess.session.push_mel(mel[:, :, lo: lo + n], [n] * B, [lo + n >= frames] * B))
        new, td = timed(lambda: sess._decode(out, out_len))
        enc_ms.append(te)
        dec_ms.append(td)
        ntok += sum(len(t) for t in new)
        outs.append(out)
    sess.session.close()
    return statistics.mean(enc_ms), statistics.mean(dec_ms), ntok / (len(enc_ms) * B), outs


def whole_pass(m, outs):
    """decode_encoded of the prefix after every push -> mean ms per push, ms of the last one, ms of every one."""
    ms = []
    for i in range(len(outs)):
        prefix = torch.cat(outs[:i + 1], 1).contiguous()
        if prefix.shape[1] == 0:
            continue

        def run():
            tokens, token_len = m.decode_encoded(prefix, None)
            return tokens.cpu(), token_len.cpu()
        ms.append(timed(run)[1])
    return statistics.mean(ms), ms[-1], ms


def med_spread(vals):
    md = statistics.median(vals)
    return md, (max(vals) - min(vals)) / md if md else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_stream_bench.txt"))
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--chunks", type=int, nargs="+", default=[24, 48, 96])
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rnnt_stream_bench needs a GPU"
    frames = int(a.seconds * 100)
    m = make_model()
    lib = _lib.load()
    route = {0: "per-utterance", 1: "8x8x2", 2: "16x16x1"}
    lines = ["rnnt_stream_bench: EfficientConformerTransducer-Medium causal, %d mel frames (%.1f s) per stream, blank bias %.1f, median of %d passes (spread = (max - min) / median)"
             % (frames, a.seconds, BLANK_BIAS, a.repeats),
             "streams | chunk frames | encoder ms/push (spread) | resumed decode ms/push (spread) | decode / encoder | tokens/push/stream | whole decode of the prefix: "
             "mean ms/push (spread) | at the last push ms (spread) | its route"]
    for B in a.streams:
        mel, _ = synth.make_mel(B, m.encoder.plan.n_mels, frames, [frames] * B, seed=4321)
        mel = torch.from_numpy(mel).cuda()
        for chunk in a.chunks:
            outs = session_pass(m, mel, chunk, frames)[3]
            whole_pass(m, outs)
            sv = [session_pass(m, mel, chunk, frames)[:3] for _ in range(a.repeats)]
            wv = [whole_pass(m, outs) for _ in range(a.repeats)]
            (em, es), (dm, ds) = med_spread([s[0] for s in sv]), med_spread([s[1] for s in sv])
            (wm, ws), (lm, ls) = med_spread([w[0] for w in wv]), med_spread([w[1] for w in wv])
            line = "%7d | %12d | %8.3f (%4.1f %%) | %8.3f (%4.1f %%) | %5.2f | %6.2f | %8.3f (%4.1f %%) | %8.3f (%4.1f %%) | %s" % (
                B, chunk, em, 100 * es, dm, 100 * ds, dm / em, sv[0][2], wm, 100 * ws, lm, 100 * ls, route[lib.effconf_rnnt_greedy_route(m._rnnt, B)])
            print(line, flush=True)
            lines.append(line)
            if len(wv[-1][2]) <= 12:
                detail = "        whole decode at every push of the last pass, ms: " + " ".join("%.2f" % v for v in wv[-1][2])
                print(detail, flush=True)
                lines.append(detail)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
