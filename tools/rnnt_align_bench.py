#!/usr/bin/env python3
"""RNN-T lattice scoring / forced alignment cost (effconf_rnnt_lattice + effconf_rnnt_align): EfficientConformerTransducerMedium
(synthetic weights, bf16 encoder path) on one ragged LibriSpeech-shaped batch (synth.libri_lengths), B = 256, random transcripts of
0.31 tokens per encoder frame (~60 tokens on ~190 frames).

Timed with a host clock around work that ends in a device synchronise, medians of `--reps` runs after a warm-up of every shape:
  * ``lattice`` (prediction network + the two Linear GEMMs + the joint kernel), ``align_lattice`` (forward + Viterbi + back-trace),
    ``align_lattice(scores_only=True)`` (forward alone) and the two in sequence;
  * the Transducer's encoder step (forward_mel) on the same batch;
  * a PyTorch-ROCm fp32 baseline - what a user could do before: nn.LSTM over the packed transcripts, then per chunk of utterances
    ``tanh(fe + gd)``, ``linear``, ``log_softmax``, ``gather`` of the two columns, and the forward recursion over the anti-diagonals in
    torch (one batched step per diagonal).  The baseline's planes and log-likelihoods are compared with the kernels' first.
Per-kernel times come from a profiler run of their own: run this tool under ``rocprofv3 --kernel-trace --stats`` with ``--profile-only``
(lattice + align only), then pass the database to the timing run with ``--kernel-db``; the report then lists each kernel's average and,
for the joint kernel, its share of the fp32 matrix peak (2 cells J V flops over 157.3 TFLOP/s).

    python tools/rnnt_align_bench.py [--batch 256] [--reps 10] [--out profiles/rnnt_align_bench.txt] [--kernel-db DB] [--profile-only]
"""
import argparse
import os
import sqlite3
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientconformer_amd import Transducer, named_config, synth  # noqa: E402

NAME = "EfficientConformerTransducerMedium"
FP32_MATRIX_PEAK = 157.3e12          # v_mfma_f32_16x16x4_f32, MI355X spec
TOKENS_PER_FRAME = 0.31


def build():
    cfg = named_config(NAME)
    m = Transducer.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, 0, None, prefix="encoder.")
    sd.update(synth.make_transducer_state_dict(m.encoder.plan.dim_out, cfg["decoder_params"], cfg["joint_params"], 0, blank_bias=1.2))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda(), cfg


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


# ---------------------------------------------------------------------------------------------------------------- the torch baseline
def torch_planes(m, f, f_len, tg, tl, chunk=8):
    """The same planes with torch ops in fp32, `chunk` utterances at a time (the (b, T, U + 1, V) logits of a chunk exist in memory)."""
    b, t, _ = f.shape
    e = tg.shape[1] + 1
    jn = m.joint_network
    yp = torch.nn.functional.pad(tg.long(), (1, 0))
    emb = m.decoder.embedding(yp)
    packed = torch.nn.utils.rnn.pack_padded_sequence(emb, (tl + 1).cpu(), batch_first=True, enforce_sorted=False)
    g, _ = torch.nn.utils.rnn.pad_packed_sequence(m.decoder.rnn(packed)[0], batch_first=True, total_length=e)
    fe, gd = jn.linear_encoder(f), jn.linear_decoder(g)
    lpb = torch.zeros(b, t, e, dtype=torch.float32, device=f.device)
    lpl = torch.zeros(b, t, e, dtype=torch.float32, device=f.device)
    ar_t, ar_u = torch.arange(t, device=f.device), torch.arange(e, device=f.device)
    for lo in range(0, b, chunk):
        hi = min(b, lo + chunk)
        tc, uc = int(f_len[lo:hi].max()), int(tl[lo:hi].max()) + 1          # the chunk's own rectangle (lengths are sorted)
        if tc == 0:
            continue
        z = torch.tanh(fe[lo:hi, :tc, None, :] + gd[lo:hi, None, :uc, :])
        lp = torch.log_softmax(jn.linear_joint(z) / m.tmp, dim=-1)
        idx = torch.nn.functional.pad(tg[lo:hi, :uc - 1].long(), (0, 1))[:, None, :, None].expand(hi - lo, tc, uc, 1)
        inside = (ar_t[None, :tc, None] < f_len[lo:hi, None, None]) & (ar_u[None, None, :uc] <= tl[lo:hi, None, None])
        lab = lp.gather(3, idx)[..., 0].masked_fill(ar_u[None, None, :uc] == tl[lo:hi, None, None], float("-inf"))
        lpb[lo:hi, :tc, :uc] = torch.where(inside, lp[..., 0], torch.zeros((), device=f.device))
        lpl[lo:hi, :tc, :uc] = torch.where(inside, lab, torch.zeros((), device=f.device))
    return lpb, lpl


def torch_forward(lpb, lpl, f_len, tl):
    """log P(y | x) from the planes: the forward recursion, one batched torch step per anti-diagonal d = t + u."""
    b, t, e = lpb.shape
    dev = lpb.device
    ninf = torch.full((), float("-inf"), device=dev)
    ar_t, ar_u = torch.arange(t, device=dev), torch.arange(e, device=dev)
    inside = (ar_t[None, :, None] < f_len[:, None, None]) & (ar_u[None, None, :] <= tl[:, None, None])
    nd = t + e - 1
    tt = torch.arange(nd, device=dev)[:, None] - ar_u[None, :]                         # frame of (diagonal, column)
    ok = ((tt >= 0) & (tt < t))[None]
    tix = tt.clamp(0, t - 1)[None].expand(b, nd, e)
    sb = torch.where(ok & inside.gather(1, tix), lpb.gather(1, tix), ninf)             # sb[b, d, u] = lp_blank[b, d - u, u]
    sl = torch.where(ok & inside.gather(1, tix), lpl.gather(1, tix), ninf)
    alpha = torch.full((b, e), float("-inf"), device=dev)
    alpha[:, 0] = 0.0
    last = (f_len - 1 + tl).clamp(min=0)
    rows = torch.arange(b, device=dev)
    end_blank = lpb[rows, (f_len - 1).clamp(min=0), tl]
    ll = torch.where(last == 0, alpha[rows, tl] + end_blank, ninf)
    for d in range(1, nd):
        stay = alpha + sb[:, d - 1]
        lab = torch.nn.functional.pad((alpha + sl[:, d - 1])[:, :-1], (1, 0), value=float("-inf"))
        alpha = torch.logaddexp(stay, lab)
        ll = torch.where(last == d, alpha[rows, tl] + end_blank, ll)
    return torch.where(f_len > 0, ll, torch.where(tl == 0, torch.zeros((), device=dev), ninf))


# ---------------------------------------------------------------------------------------------------------------- report
def kernel_rows(db):
    c = sqlite3.connect(db)
    rows = c.execute("select name, total_calls, total_duration, average from top_kernels").fetchall()
    keep = [r for r in rows if any(k in r[0] for k in ("rnnt_", "sgemm_nt"))]
    return [(n, calls, tot, avg) for n, calls, tot, avg in keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-db", default=None)
    ap.add_argument("--profile-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rnnt_align_bench: needs a GPU (a timing taken anywhere else says nothing)")
    m, cfg = build()
    b = args.batch
    vocab, jdim = cfg["decoder_params"]["vocab_size"], cfg["joint_params"]["dim_model"]
    ml = np.maximum(16, synth.libri_lengths(b, seed=11) // 160).astype(np.int64)
    mel, ml = synth.make_mel(b, 80, int(ml.max()), ml.tolist(), seed=4321)
    mel, ml = torch.from_numpy(mel).cuda(), torch.from_numpy(ml).cuda()
    with torch.no_grad():
        f, f_len, _ = m.encoder.forward_mel(mel, ml)
    f = f.float().contiguous()
    rng = np.random.default_rng(5)
    ul = np.minimum(1023, np.round(f_len.cpu().numpy() * TOKENS_PER_FRAME)).astype(np.int64)
    tg = np.zeros((b, int(ul.max())), dtype=np.int32)
    for i, u in enumerate(ul):
        tg[i, :u] = rng.integers(1, vocab, u)
    tg, tl = torch.from_numpy(tg).cuda(), torch.from_numpy(ul).cuda()
    cells = int((f_len * (tl + 1)).sum())
    flops = 2.0 * cells * jdim * vocab

    def native(scores_only=False):
        lpb, lpl, st = m.lattice(f, f_len, tg, tl)
        return lpb, lpl, m.align_lattice(lpb, lpl, f_len, tl, scores_only=scores_only, status=st)

    if args.profile_only:
        for _ in range(3):
            native()
        torch.cuda.synchronize()
        print("profile run: 3 x (lattice + align_lattice), %d cells" % cells)
        return

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# RNN-T lattice scoring / forced alignment: %s, B = %d, T_max = %d (mean %.0f), U_max = %d (mean %.0f), J = %d, V = %d"
        % (NAME, b, f.shape[1], float(f_len.float().mean()), tg.shape[1], float(tl.float().mean()), jdim, vocab))
    say("# cells = sum T_b (U_b + 1) = %d (padded rectangle: %d); joint GEMM = 2 cells J V = %.3f TFLOP" % (cells, b * f.shape[1] * (tg.shape[1] + 1), flops / 1e12))
    with torch.no_grad():
        lpb, lpl, out = native()
        assert int(out["status"].abs().max()) == 0
        tb, tlab = torch_planes(m, f, f_len, tg, tl)
        fin = torch.isfinite(tlab)
        assert torch.equal(fin, torch.isfinite(lpl))
        dev_planes = max(float((tb - lpb).abs().max()), float((tlab[fin] - lpl[fin]).abs().max()))
        tll = torch_forward(tb, tlab, f_len, tl)
        dev_ll = float(((tll - out["log_likelihood"]).abs() / (1 + tll.abs())).max())
        say("# kernels vs the torch fp32 baseline on this batch: planes max |diff| %.3g, log-likelihood max rel diff %.3g" % (dev_planes, dev_ll))
        assert dev_planes <= 1e-4 and dev_ll <= 1e-5, (dev_planes, dev_ll)
        res = {}
        res["encoder step (forward_mel)"] = timed(lambda: m.encoder.forward_mel(mel, ml), args.reps)
        res["lattice (prediction net + Linear GEMMs + joint kernel)"] = timed(lambda: m.lattice(f, f_len, tg, tl), args.reps)
        st0 = out["status"]
        res["align_lattice (forward + Viterbi + back-trace)"] = timed(lambda: m.align_lattice(lpb, lpl, f_len, tl, status=st0), args.reps)
        res["align_lattice scores only (forward)"] = timed(lambda: m.align_lattice(lpb, lpl, f_len, tl, scores_only=True, status=st0), args.reps)
        res["native total: lattice + align_lattice"] = timed(lambda: native(), args.reps)
        res["native total, scores only"] = timed(lambda: native(True), args.reps)
        res["torch fp32 baseline: planes (chunks of 8)"] = timed(lambda: torch_planes(m, f, f_len, tg, tl), max(3, args.reps // 2))
        res["torch fp32 baseline: forward recursion"] = timed(lambda: torch_forward(tb, tlab, f_len, tl), max(3, args.reps // 2))
        res["torch fp32 baseline total (scores only)"] = timed(lambda: torch_forward(*torch_planes(m, f, f_len, tg, tl), f_len, tl), max(3, args.reps // 2))
    say("%-62s %10s %10s %10s" % ("host clock to device synchronise, ms", "median", "min", "max"))
    for k, (med, lo, hi) in res.items():
        say("%-62s %10.3f %10.3f %10.3f" % (k, med, lo, hi))
    nat, base = res["native total, scores only"][0], res["torch fp32 baseline total (scores only)"][0]
    say("# scores only, native / torch baseline: %.3f / %.3f ms = %.2fx %s" % (nat, base, base / nat, "faster" if nat < base else "SLOWER than the baseline"))
    lat = res["lattice (prediction net + Linear GEMMs + joint kernel)"][0]
    say("# the whole lattice call against the fp32 matrix peak: %.3f TFLOP / %.3f ms = %.1f TFLOP/s = %.1f %% of 157.3 (end to end, not a kernel's share)"
        % (flops / 1e12, lat, flops / lat / 1e9, 100 * flops / (lat * 1e-3) / FP32_MATRIX_PEAK))
    if args.kernel_db:
        say("# kernels (rocprofv3 --kernel-trace --stats, a run of its own: 3 x (lattice + align_lattice)); microseconds")
        say("%-70s %6s %12s %12s" % ("kernel", "calls", "total_us", "avg_us"))
        for n, calls, tot, avg in kernel_rows(args.kernel_db):
            say("%-70s %6d %12.1f %12.1f" % (n[:70], calls, tot, avg))
            if "rnnt_joint" in n:
                say("#   joint kernel: %.3f TFLOP / %.1f us = %.1f TFLOP/s = %.1f %% of the fp32 matrix peak (157.3 TFLOP/s; bound: fp32 MFMA rate)"
                    % (flops / 1e12, avg, flops / (avg * 1e-6) / 1e12, 100 * flops / (avg * 1e-6) / FP32_MATRIX_PEAK))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
