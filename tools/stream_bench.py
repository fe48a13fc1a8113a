#!/usr/bin/env python3
"""What chunked streaming costs on the MI355X -> profiles/stream_bench.txt.

    python tools/stream_bench.py [--out profiles/stream_bench.txt] [--streams 1 16 64] [--chunks 24 48 96] [--seconds 10] [--repeats 5]

EfficientConformerCTC-Small, causal, left_context 64 and unlimited; 1 / 16 / 64 streams that all receive the same number of mel frames per push (chunks of
24 / 48 / 96 frames = 0.24 / 0.48 / 0.96 s) until `--seconds` of audio are in.  Per configuration:
  session      ms per push of ``StreamingEncoder.push_mel`` (host time around a synchronised push, so the Python staging and the descriptor copy are in it), the
               real-time factor = push time / audio seconds of a push (per stream: all streams advance together), and the share of the push's kernel time that
               the per-launch profiler attributes to the attention class (stream_attention_kernel and nothing else in a session round)
  re-encode    what a user of the whole-utterance entry has to do instead: ``forward_mel`` of the whole prefix at every chunk, same encoder and batch
Each figure: the median over `--repeats` passes through the whole utterance, with the spread (max - min) / median of the passes beside it.  The first pass
(allocations, the positional tables) is not counted.  Needs a GPU: no fallback."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from efficientconformer_amd import ConformerEncoder, _lib, named_config, synth  # noqa: E402


def make_encoder(left):
    cfg = named_config("EfficientConformerCTCSmall")
    params = dict(cfg["encoder_params"], causal=True)
    if left is not None:
        params["left_context"] = left
    enc = ConformerEncoder(params)
    sd = synth.make_state_dict(enc.plan, 0, cfg["tokenizer_params"]["vocab_size"])
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if not k.startswith("fc.")}, strict=False)
    return enc.cuda()


def attention_share(enc):
    lib, h = _lib.load(), enc._handle
    tot, att = 0.0, 0.0
    for ci in range(8):
        ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        _lib.check(lib.effconf_profile_read(h, ci, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)), "profile_read")
        tot += ms.value
        att += ms.value if ci == 5 else 0.0
    return att / tot if tot else float("nan")


def session_pass(enc, mel, chunk, frames):
    B = mel.shape[0]
    sess = enc.open_stream(B, max_frames=frames)
    times = []
    for lo in range(0, frames, chunk):
        n = min(chunk, frames - lo)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sess.push_mel(mel[:, :, lo: lo + n], [n] * B, [lo + n >= frames] * B)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    sess.close()
    return 1e3 * statistics.mean(times)


def reencode_pass(enc, mel, chunk, frames):
    B = mel.shape[0]
    times = []
    for lo in range(0, frames, chunk):
        hi = min(lo + chunk, frames)
        prefix = mel[:, :, :hi].contiguous()
        ln = torch.full((B,), hi, dtype=torch.int64, device=mel.device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc.forward_mel(prefix, ln)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return 1e3 * statistics.mean(times)


def med_spread(vals):
    m = statistics.median(vals)
    return m, (max(vals) - min(vals)) / m if m else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bench.txt"))
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--chunks", type=int, nargs="+", default=[24, 48, 96])
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "stream_bench needs a GPU"
    frames = int(a.seconds * 100)
    lines = ["stream_bench: EfficientConformerCTC-Small causal, %d mel frames (%.1f s) per stream, median of %d passes (spread = (max - min) / median)" % (frames, a.seconds, a.repeats),
             "left_context | streams | chunk frames | session ms/push (spread) | RTF | attention share of kernel time | re-encode ms/chunk (spread) | re-encode / session"]
    for left in (64, None):
        enc = make_encoder(left)
        lib = _lib.load()
        for B in a.streams:
            mel, _ = synth.make_mel(B, 80, frames, [frames] * B, seed=4321)
            mel = torch.from_numpy(mel).cuda()
            for chunk in a.chunks:
                session_pass(enc, mel, chunk, frames)
                reencode_pass(enc, mel, chunk, frames)
                sv = [session_pass(enc, mel, chunk, frames) for _ in range(a.repeats)]
                rv = [reencode_pass(enc, mel, chunk, frames) for _ in range(a.repeats)]
                _lib.check(lib.effconf_profile_enable(enc._handle, 1), "profile_enable")
                session_pass(enc, mel, chunk, frames)
                share = attention_share(enc)
                _lib.check(lib.effconf_profile_enable(enc._handle, 0), "profile_enable")
                (sm, ss), (rm, rs) = med_spread(sv), med_spread(rv)
                line = "%12s | %7d | %12d | %8.3f (%4.1f %%) | %.4f | %5.1f %% | %8.3f (%4.1f %%) | %5.1fx" % (
                    "unlimited" if left is None else left, B, chunk, sm, 100 * ss, sm / (10.0 * chunk), 100 * share, rm, 100 * rs, rm / sm)
                print(line, flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
