#!/usr/bin/env python3
"""What a resumed CTC beam-search push costs on the MI355X -> profiles/ctc_beam_stream_bench.txt.

    python tools/ctc_beam_stream_bench.py [--out profiles/ctc_beam_stream_bench.txt] [--streams 1 16 64] [--chunks 24 48 96] [--beams 4 16] [--seconds 10] [--repeats 5]

EfficientConformerCTC-Small, causal (unlimited left context), synthetic weights; 1 / 16 / 64 streams that all receive the same number of mel frames per push
(24 / 48 / 96 frames) until `--seconds` of audio are in.  One pass of ``ModelCTC.open_stream(beam_size=..)`` through the utterance records the head logits of
every push (``last_push_logits``); the decode is then timed on those logits alone, so the figures are the search's and not the encoder's:
  resumed      ``CtcBeamStreamState.push`` of the first and of the last chunk of the utterance (the chunks between them are pushed untimed)
  prefix       ``decode_logits_beam`` of the whole logit prefix at the same two points: the only way to the same answer without a carried beam
Host time around a synchronised call (the id / length copies of a push are in it; no copy of the results to the host).  Each figure: the median over `--repeats`
passes after one warm-up pass, with the spread (max - min) / median beside it.  Below the table: whether the push is flat in the utterance's length (last /
first), the ratio of the prefix decode to the push at the end of the utterance, and the push's cost per logit frame beside the whole-utterance kernel's
(profiles/ctc_beam_bench.txt: 18 us per frame at beam 16, 6.9 us at beam 1).  Needs a GPU: no fallback."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from efficientconformer_amd import ModelCTC, named_config, synth  # noqa: E402


def make_model():
    cfg = named_config("EfficientConformerCTCSmall")
    cfg["encoder_params"] = dict(cfg["encoder_params"], causal=True)
    m = ModelCTC.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, 0, cfg["tokenizer_params"]["vocab_size"], prefix="encoder.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, 1e3 * (time.perf_counter() - t0)


def record_logits(m, mel, chunk, frames, beam):
    """The session once through the utterance -> the (B, rows, V) logits of every push that produced rows."""
    B = mel.shape[0]
    sess = m.open_stream(B, max_frames=frames, beam_size=beam)
    out = []
    for lo in range(0, frames, chunk):
        n = min(chunk, frames - lo)
        sess.push_mel(mel[:, :, lo: lo + n], [n] * B, [lo + n >= frames] * B)
        if sess.last_push_logits is not None:
            lg, ln, active = sess.last_push_logits
            assert active == list(range(B)) and bool((ln == lg.shape[1]).all())
            out.append(lg)
    sess.session.close()
    return out


def resumed_pass(m, pushes, beam):
    """-> ms of the first push, ms of the last push."""
    B, rows = pushes[0].shape[0], sum(p.shape[1] for p in pushes)
    st = m.open_beam_decode_stream(B, rows, beam)
    _, first = timed(lambda: st.push(pushes[0], None))
    for p in pushes[1:-1]:
        st.push(p, None)
    _, last = timed(lambda: st.push(pushes[-1], None))
    return first, last


def prefix_pass(m, pushes, beam):
    whole = torch.cat(pushes, 1).contiguous()
    _, first = timed(lambda: m.decode_logits_beam(pushes[0], None, beam))
    _, last = timed(lambda: m.decode_logits_beam(whole, None, beam))
    return first, last


def med_spread(vals):
    md = statistics.median(vals)
    return md, (max(vals) - min(vals)) / md if md else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_beam_stream_bench.txt"))
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--chunks", type=int, nargs="+", default=[24, 48, 96])
    ap.add_argument("--beams", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ctc_beam_stream_bench needs a GPU"
    frames = int(a.seconds * 100)
    m = make_model()
    lines = ["ctc_beam_stream_bench: EfficientConformerCTC-Small causal, %d mel frames (%.1f s) per stream, median of %d passes after a warm-up pass (spread = (max - min) / median)"
             % (frames, a.seconds, a.repeats),
             "streams | beam | chunk mel frames | logit frames/push | utterance logit frames | resumed push ms: first (spread) | last (spread) | last / first | "
             "prefix decode ms: first (spread) | at the end (spread) | prefix / push at the end | push us per logit frame: first | last | whole-utterance kernel us per frame"]
    for B in a.streams:
        mel, _ = synth.make_mel(B, m.encoder.plan.n_mels, frames, [frames] * B, seed=4321)
        mel = torch.from_numpy(mel).cuda()
        for beam in a.beams:
            for chunk in a.chunks:
                pushes = record_logits(m, mel, chunk, frames, beam)
                rows, total = pushes[0].shape[1], sum(p.shape[1] for p in pushes)
                resumed_pass(m, pushes, beam)
                prefix_pass(m, pushes, beam)
                rv = [resumed_pass(m, pushes, beam) for _ in range(a.repeats)]
                pv = [prefix_pass(m, pushes, beam) for _ in range(a.repeats)]
                (rf, rfs), (rl, rls) = med_spread([r[0] for r in rv]), med_spread([r[1] for r in rv])
                (pf, pfs), (pl, pls) = med_spread([p[0] for p in pv]), med_spread([p[1] for p in pv])
                line = "%7d | %4d | %5d | %3d | %4d | %7.3f (%4.1f %%) | %7.3f (%4.1f %%) | %5.2f | %7.3f (%4.1f %%) | %7.3f (%4.1f %%) | %6.1f | %6.1f | %6.1f | %6.1f" % (
                    B, beam, chunk, rows, total, rf, 100 * rfs, rl, 100 * rls, rl / rf, pf, 100 * pfs, pl, 100 * pls, pl / rl, 1e3 * rf / rows,
                    1e3 * rl / pushes[-1].shape[1], 1e3 * pl / total)
                print(line, flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
