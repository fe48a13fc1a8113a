#!/usr/bin/env python3
"""Headline benchmark: mel-frames/s through the EfficientConformerCTC-Small encoder (+ CTC greedy head).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" is one pass of the hot path (ConformerEncoder.forward: mel frontend -> conv subsampling -> 15
Conformer blocks, then fc + argmax + CTC collapse) over one synthetic LibriSpeech-shaped batch that is
already resident in HBM (default: 256 utterances per GPU, `--streams 3`).  `--streams S` runs the batch as S contiguous row
ranges on S HIP streams inside ConformerEncoder.forward (`sub_batches`, efficientconformer_amd/encoders.py): every kernel of the
path is a one-round launch that alternates HBM-bound load/store bursts with compute, and a second stream fills one's bursts with the
other's compute (+10-13 %, bit-identical to `--streams 1`; the mel frontend stays one launch: HISTORY.md section 5).

Multi-GPU: one process per GPU.  `--gpus N` without a torchrun environment re-executes this script under
`python -m torch.distributed.run --nproc-per-node N` (the reference spawns one process per GPU the same way: main.py:217-220);
under torchrun (the driver's launch line) WORLD_SIZE must equal --gpus.  Utterances shard across ranks (weak scaling: B utterances
per GPU); the only data-path collective is the RCCL all-gather of encoder outputs, issued PER ROW RANGE on a comm stream as soon
as that range's last kernel is enqueued (efficientconformer_amd/dist.py), so range 0 is on the wire during range 1's last stage
and range 1's collective overlaps the head of range 0 and the next step's encoder.  The CTC head consumes the gathered chunks
(every rank ends up with the labels of the GLOBAL batch) on a head stream; `--gather labels` gathers label ids instead.
Rank 0 prints ONE JSON line.  `value` counts VALID (un-padded) mel frames of all ranks per second; `ms_per_step` is the wall clock of one
timed step.  A plain run only sets up, warms up, times the K steps and prints that line.  `--full` adds the un-timed legs after the timed
region: `check` (the last step against each row range / utterance run alone and against the oracle), `roofline` + `kernel_classes`,
`reference_batch_semantics` and `cpu_baseline`.  `--dump-outputs DIR` writes what the last timed step returned (encoder outputs, lengths,
labels) as DIR/<name>.npy; the inputs are seeded, so two builds run with the same arguments can be compared output for output.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time



def _wants_ranks(argv):
    """--gpus N > 1, a torchrun environment with WORLD_SIZE > 1, or --force-dist: the multi-rank code path (a process group exists)."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or "--force-dist" in argv:
        return True
    for i, a in enumerate(argv):
        if a == "--gpus" and i + 1 < len(argv):
            return argv[i + 1].isdigit() and int(argv[i + 1]) > 1
        if a.startswith("--gpus="):
            return a[7:].isdigit() and int(a[7:]) > 1
    return False


# Multi-rank processes: eight hardware queues instead of the runtime's four, set BEFORE the HIP runtime initialises (it reads the variable
# once).  HIP multiplexes streams onto GPU_MAX_HW_QUEUES queues; the forward uses three streams (caller's + two side streams) and an RCCL
# process group brings its own - with four queues the step of a rank that merely HOLDS a process group is 7.2 ms instead of 5.5 (measured
# on RCCL with one rank: `bench.py --force-dist`, profiles/r4_02_rccl_one_rank.txt), with eight it is 5.55.  N = 1 runs keep the default.
if _wants_ranks(sys.argv):
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from efficientconformer_amd import ModelCTC, Transducer, _lib, named_config, synth  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0     # dense MFMA bf16, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0
# stated tolerance of the bf16 path on LayerNorm-ed O(1) encoder outputs: 1.5x the worst measured over all configs (0.039 max / 0.008 mean;
# rounds 1 - 3 stated 0.10 / 0.012, three times the measurement: a regression could not fail it).  split = fp16 operand pairs on the fp16
# matrix pipe (csrc/split.hip: products accurate to ~2^-21), fp32 = fp32 operands on the fp32 matrix pipe: both label-exact modes share a bound.
TOL_BF16 = (0.06, 0.010)


def tolerance(precision):
    return {"bf16": TOL_BF16, "split": (2e-4, 2e-5), "fp32": (2e-4, 2e-5)}[precision]      # measured: split 5.3e-6 / 9.7e-7, fp32 4.8e-6 / 7.6e-7


PROF_CLASSES = ["mel", "subsample_conv", "gemm_ffn", "gemm_other", "layernorm", "attention", "dwconv", "misc"]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--model", default="EfficientConformerCTCSmall")
    ap.add_argument("--batch", type=int, default=256, help="utterances per GPU per step")
    ap.add_argument("--workload", default="libri", choices=["libri", "fixed"],
                    help="libri: lognormal LibriSpeech-shaped lengths (SURVEY.md 8d W-libri); fixed: 10 s each")
    ap.add_argument("--streams", type=int, default=3,
                    help="ConformerEncoder.sub_batches: contiguous row ranges of the batch on concurrent HIP streams")
    ap.add_argument("--ranges", type=int, default=0,
                    help="row ranges per GPU (0: one per stream); more ranges than streams = finer length buckets, range i on stream i %% streams")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--gather", default="outputs", choices=["outputs", "labels"],
                    help="N > 1: all-gather the encoder outputs before the CTC head (north_star) or the label ids after it")
    ap.add_argument("--wire", default="auto", choices=["auto", "fp32", "bf16"],
                    help="dtype of the gathered encoder outputs on xGMI; auto = bf16 on the bf16 path (half the bytes; the rounding, 2^-9 relative, "
                         "is an order below the bf16 encoder's own output error), fp32 with --precision fp32")
    ap.add_argument("--pipeline-gather", type=int, default=-1, choices=[-1, 0, 1],
                    help="N > 1, --gather outputs: 1 = dist.ShardedEncoder(pipelined=True): a row range's all-gather is issued asynchronously and "
                         "its CTC head runs one step later on that range's stream, so the collective is on the wire under the whole next "
                         "step's encoder; 0 = the head waits for its collective inside the step; -1 (default) = 1")
    ap.add_argument("--range-frames", default="",
                    help="ragged batches: share of the valid frames per row range in percent, e.g. 40,35,25 (default: equal shares); ranges that "
                         "finish at different times put their collectives under another range's encoder kernels")
    ap.add_argument("--balanced-split", action="store_true",
                    help="cut the row ranges for equal PADDED FRAMES per range instead of equal utterance counts (measured: no gain at B = 256)")
    ap.add_argument("--cuts", default="", help="explicit row boundaries of the ranges, e.g. 80,168 (tuning; overrides --balanced-split)")
    ap.add_argument("--no-trim", action="store_true",
                    help="pad every row range to the whole batch's longest utterance (round-1 workload) instead of its own longest")
    ap.add_argument("--subsample", type=int, default=-1, choices=[-1, 0, 1, 2, 3],
                    help="conv subsampling + Linear: 0 separate kernels, 1 sublinear.hip, 2 sublinear2.hip (wide front ends: sublinear3.hip), 3 sublinear3.hip (-1: the library default = 2)")
    ap.add_argument("--attention", type=int, default=-1, choices=[-1, 0, 1, 2],
                    help="attention kernel: 0 attention.hip, 1 / 2 attention2.hip variants (-1: the library's default = 1)")
    ap.add_argument("--wide-gemm", type=int, default=-1, choices=[-1, 0, 1, 2, 3],
                    help="tiled GEMM layers: 0 tile by shape, 1 gemm.hip only, 2 / 3 gemm256.hip 256x256 / 256x128 wherever it applies (-1: default = 0)")
    ap.add_argument("--opt", action="append", default=[], help="library option name=value (effconf_encoder_set_option), repeatable (tuning)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="process-group backend for N > 1 (nccl = RCCL over xGMI; gloo + --one-device: N ranks on ONE GPU, a test of the multi-rank path)")
    ap.add_argument("--one-device", action="store_true", help="every rank uses cuda:0 (tests on a single-GPU box; never a benchmark)")
    ap.add_argument("--force-dist", action="store_true",
                    help="N = 1: run the multi-rank code path all the same - a one-rank process group (RCCL), per-range all-gather, head on the gathered "
                         "chunk: what the protocol costs on the real backend when nothing has to cross xGMI (a diagnostic, not the N = 1 line)")
    ap.add_argument("--ragged", type=int, default=-1, choices=[-1, 0, 1],
                    help="1: ConformerEncoder.ragged - every utterance at its own length in one concatenated row space (no pad frames; an utterance's "
                         "output = the reference's for that utterance alone); 0: row ranges padded to their longest utterance (round 2's workload); "
                         "-1 (default): 1 where the model supports it (one-layer subsampler, bf16 path, libri workload)")
    ap.add_argument("--no-check", action="store_true",
                    help="skip the un-timed self-check of the benchmarked step (single-stream per-range rerun + oracle samples)")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32", "split"],
                    help="bf16: bf16 MFMA operands / fp32 accumulate (default); fp32: the library's label-exact mode on the fp32 matrix pipe; "
                         "split: the label-exact mode on the fp16 matrix pipe (operands split into two fp16 numbers, three MFMAs per product)")
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU work: build the batch plan, join the process group (gloo) and print the JSON skeleton (CPU tests)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run the un-timed legs: the self-check (`check`), the roofline leg (`roofline`, `kernel_classes`), "
                         "the reference's collated-batch semantics and the CPU baseline (`cpu_baseline`); --no-check / --no-roofline / "
                         "--no-cpu-baseline drop single legs.  Without --full a run sets up, warms up, times the steps and prints the result line")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the timed path returned in its last timed step as DIR/<name>.npy (float32; integer arrays as float64), "
                         "at most 64 MB in all: larger outputs are cut to a fixed, seeded sample of rows (DIR/<name>_rows.npy lists them)")
    args = ap.parse_args()
    if not args.full:
        args.no_check = args.no_roofline = args.no_cpu_baseline = True
    return args


def launch_ranks(args):
    """`python bench.py --gpus N` outside torchrun: re-execute under torch.distributed.run with N local ranks (one per GPU)."""
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % args.gpus,
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on this driver (RCCL needs it)
    env.setdefault("GPU_MAX_HW_QUEUES", "8")               # see the top of this file: three forward streams + the process group's need more than four queues
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
    return subprocess.call(cmd, env=env)


RNNT_BLANK_BIAS = 1.2         # synthetic joint bias of the blank: ~1 token per 3 encoder frames (synth.make_transducer_state_dict)


def build_model(name):
    cfg = named_config(name)
    if cfg["model_type"] == "Transducer":
        model = Transducer.from_config(cfg)
        sd = synth.make_state_dict(model.encoder.plan, 0, None, prefix="encoder.")
        sd.update(synth.make_transducer_state_dict(model.encoder.plan.dim_out, cfg["decoder_params"], cfg["joint_params"], 0,
                                                   blank_bias=RNNT_BLANK_BIAS))
    else:
        model = ModelCTC.from_config(cfg)
        sd = synth.make_state_dict(model.encoder.plan, 0, cfg["tokenizer_params"]["vocab_size"], prefix="encoder.")
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return cfg, model, sd


def make_batch(args, rank, world=1):
    if args.workload == "fixed":
        lens = np.full(args.batch, 160000, dtype=np.int64)
        lmax = 160000
    else:
        lens = synth.libri_lengths(args.batch, seed=1234 + rank)
        # every rank pads to the longest utterance of the GLOBAL batch (seeds are known, so no exchange is needed): the
        # all-gather of encoder outputs needs one shape on all ranks, exactly as a data-parallel collate would give it
        lmax = max(int(synth.libri_lengths(args.batch, seed=1234 + r).max()) for r in range(world))
    audio = synth.make_audio(lens, seed=1234 + rank)
    if audio.shape[1] < lmax:
        audio = np.pad(audio, ((0, 0), (0, lmax - audio.shape[1])))
    return audio, lens


def balanced_cuts(frames_desc, nsub):
    """Row boundaries [0, c1, .., B] of `nsub` contiguous ranges of a length-sorted (descending) batch with the smallest possible
    largest padded work (rows x the range's longest utterance, in frames): min-max partition by dynamic programming."""
    n = len(frames_desc)
    f = [int(v) for v in frames_desc]
    inf = float("inf")
    best = [[inf] * (n + 1) for _ in range(nsub + 1)]       # best[k][i]: rows [0, i) in k ranges
    arg = [[0] * (n + 1) for _ in range(nsub + 1)]
    best[0][0] = 0
    for k in range(1, nsub + 1):
        for i in range(k, n + 1):
            for lo in range(k - 1, i):
                if best[k - 1][lo] == inf:
                    continue
                v = max(best[k - 1][lo], (i - lo) * f[lo])
                if v < best[k][i]:
                    best[k][i], arg[k][i] = v, lo
    cuts, i = [n], n
    for k in range(nsub, 0, -1):
        i = arg[k][i]
        cuts.append(i)
    return cuts[::-1]


def head(model, enc, enc_len):
    if isinstance(model, Transducer):        # RNN-T greedy (transducer.py:139-186); <= 256 utterances per call: the cluster decode's automatic range
        out = None
        for i in range(0, enc.shape[0], 256):
            out = model.decode_encoded(enc[i:i + 256].contiguous(), enc_len[i:i + 256].contiguous())
        return out
    _, labels, label_len = model._head(enc, enc_len)                 # fc + argmax + CTC collapse (model_ctc.py:90-133)
    return labels, label_len


def step(model, audio, lens, range_pad=None, **kw):
    enc, enc_len, _ = model.encoder(audio, lens, range_pad=range_pad, **kw)
    labels, label_len = head(model, enc, enc_len)
    return enc, enc_len, labels, label_len


DUMP_BUDGET = 63_000_000     # bytes of the .npy payloads of --dump-outputs (64 MB in all with the headers)


def step_outputs(model, last, multi, args):
    """name -> tensor: what the timed path handed its caller in the last timed step (rank 0's view on the multi-rank path)."""
    lab = ("tokens", "token_len") if isinstance(model, Transducer) else ("labels", "label_len")
    if multi and args.gather == "outputs":
        out = {}
        for i, ch in enumerate(last["chunks"]):
            out.update({"range%d_encoder_out" % i: ch.out, "range%d_encoder_out_len" % i: ch.out_len,
                        "range%d_%s" % (i, lab[0]): ch.labels[0], "range%d_%s" % (i, lab[1]): ch.labels[1]})
        return out
    out = {"encoder_out": last["enc"][0], "encoder_out_len": last["enc"][1], lab[0]: last["labels"][0], lab[1]: last["labels"][1]}
    if "gathered_labels" in last:
        out.update({"gathered_" + lab[0]: last["gathered_labels"][0], "gathered_" + lab[1]: last["gathered_labels"][1]})
    return out


def dump_outputs(path, tensors, budget=DUMP_BUDGET, seed=0):
    """Write every tensor as <path>/<name>.npy: floating tensors as float32, integer ones as float64 (exact).  If the whole exceeds `budget`
    bytes, every array of two or more dimensions keeps the same fraction of its rows, chosen by a generator seeded with `seed` (arrays with
    the same number of rows keep the same rows), and <name>_rows.npy lists them: the same arguments write the same files."""
    os.makedirs(path, exist_ok=True)
    size = lambda t: t.numel() * (4 if t.is_floating_point() else 8)
    small = sum(size(t) for t in tensors.values() if t.dim() < 2)
    big = sum(size(t) for t in tensors.values() if t.dim() >= 2)
    frac = 1.0 if small + big <= budget else max(0.0, budget - small - 8 * sum(t.shape[0] for t in tensors.values() if t.dim() >= 2)) / big
    for name, t in tensors.items():
        t = t.detach()
        if t.dim() >= 2 and frac < 1.0:
            k = max(1, int(t.shape[0] * frac))
            rows = np.sort(np.random.default_rng(seed).choice(t.shape[0], k, replace=False))
            np.save(os.path.join(path, name + "_rows.npy"), rows.astype(np.float64))
            t = t[torch.from_numpy(rows).to(t.device)]
        a = t.float().cpu().numpy() if t.is_floating_point() else t.cpu().numpy().astype(np.float64)
        np.save(os.path.join(path, name + ".npy"), a)


def self_check_transducer(model, sd, plan, audio, lens, lens_np, last):
    """Transducer configurations: the last timed step's token ids against (1) the one-workgroup-per-utterance decode kernel on the same
    encoder output (identical), (2) the oracle's greedy loop (oracle/ref_transducer.py = transducer.py:139-186) on the same encoder
    output for sampled utterances (identical: the head is fp32), and the encoder output of those utterances against the oracle encoder
    run on each ALONE (bf16 tolerance)."""
    from oracle import ref_encoder as R
    from oracle import ref_transducer as RT
    enc, enc_len = last["enc"]
    tok, tok_len = last["labels"]
    torch.cuda.synchronize()
    osd = {k[len("encoder."):] if k.startswith("encoder.") else k: torch.from_numpy(v) for k, v in sd.items()}
    model.set_decode_option("cluster_decode", 0)
    try:
        ref_tok, ref_n = model.decode_encoded(enc, enc_len)
    finally:
        model.set_decode_option("cluster_decode", -1)
    same_kernel = bool(torch.equal(ref_n, tok_len) and torch.equal(ref_tok, tok))
    b_all = enc.shape[0]
    rows = sorted({0, b_all // 3, 2 * b_all // 3, b_all - 1})
    want, margins = RT.greedy_decode(osd, enc[rows].cpu(), enc_len[rows].cpu(), model.max_consec_dec_step, with_margins=True)
    got = [tok[r, :int(tok_len[r])].cpu().tolist() for r in rows]
    seq_equal = got == want
    worst_max = worst_mean = 0.0
    for r in rows[1:3]:
        li = int(lens_np[r])
        with torch.no_grad():
            ref, ref_len = R.encoder(audio[r:r + 1, :li].cpu(), lens[r:r + 1].cpu(), osd, plan)
        d = (enc[r:r + 1, :ref.shape[1]].cpu() - ref).abs()
        worst_max, worst_mean = max(worst_max, float(d.max())), max(worst_mean, float(d.mean()))
    finite = bool(torch.isfinite(enc).all())
    ok = same_kernel and seq_equal and finite and worst_max <= TOL_BF16[0] and worst_mean <= TOL_BF16[1]
    return {"ok": bool(ok), "finite": finite, "tokens_identical_to_the_per_utterance_decode_kernel": same_kernel,
            "oracle_utterances": len(rows), "token_sequences_identical_to_oracle_greedy_on_the_same_encoder_output": bool(seq_equal),
            "oracle_tokens": int(sum(len(w) for w in want)), "smallest_top2_logit_margin": float(min(margins)),
            "encoder_max_abs_err_vs_oracle": worst_max, "encoder_mean_abs_err_vs_oracle": worst_mean, "tolerance": {"max": TOL_BF16[0], "mean": TOL_BF16[1]},
            "note": "token ids of the last timed step (cluster decode); oracle = oracle/ref_transducer.py greedy loop on this step's encoder "
                    "output rows, oracle/ref_encoder.py on two sampled utterances alone"}


def edit_distance(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def self_check(model, sd, plan, audio, lens, lens_np, cuts, range_pad, nsub, last, args):
    """Verify the outputs of the LAST timed step.  Returns the `check` object of the JSON line; ok = every comparison passed."""
    from oracle import ref_encoder as R
    enc, enc_len = last["enc"]
    labels, label_len = last["labels"]
    torch.cuda.synchronize()
    tol_max, tol_mean = tolerance(args.precision)
    osd = {k[len("encoder."):] if k.startswith("encoder.") else k: torch.from_numpy(v) for k, v in sd.items()}
    saved = (model.encoder.sub_batches, model.encoder.trim_sub_batches)
    model.encoder.sub_batches, model.encoder.trim_sub_batches = 1, False
    bit_ok, finite = True, bool(torch.isfinite(enc).all())
    worst_max = worst_mean = 0.0
    n_oracle = flips = frames = dist = nlab = 0
    seq_equal = True
    ragged = bool(getattr(model.encoder, "ragged", False))
    model.encoder.ragged = False
    try:
        if ragged:        # every sampled utterance ALONE (B = 1, rectangular path): bit-identical; the oracle on that utterance alone
            b_all = audio.shape[0]
            for r in sorted({0, 1, b_all // 5, 2 * b_all // 5, b_all // 2, 3 * b_all // 5, 4 * b_all // 5, b_all - 2, b_all - 1}):
                li = int(lens_np[r])
                alone, alone_len, _ = model.encoder(audio[r:r + 1, :li].contiguous(), lens[r:r + 1].contiguous())
                _, lab, n = model._head(alone, alone_len)
                ti = alone.shape[1]
                bit_ok = bit_ok and int(enc_len[r]) == ti and torch.equal(enc[r, :ti], alone[0]) and float(enc[r, ti:].abs().sum()) == 0.0 and \
                    int(label_len[r]) == int(n[0]) and torch.equal(labels[r, :ti], lab[0, :ti])
                with torch.no_grad():
                    ref, ref_len = R.encoder(audio[r:r + 1, :li].cpu(), lens[r:r + 1].cpu(), osd, plan)
                    ref_logits = R.ctc_logits(ref, osd)
                    want = R.ctc_greedy(ref_logits, ref_len)
                got = enc[r:r + 1, :ref.shape[1]].cpu()
                d = (got - ref).abs()
                worst_max, worst_mean = max(worst_max, float(d.max())), max(worst_mean, float(d.mean()))
                n_oracle += 1
                am = R.ctc_logits(got, osd).argmax(-1)
                t = int(ref_len[0])
                flips += int((am[0, :t] != ref_logits[0, :t].argmax(-1)).sum()); frames += t
                mine = labels[r, :int(label_len[r])].cpu().tolist()
                dist += edit_distance(mine, want[0]); nlab += len(want[0])
                seq_equal = seq_equal and mine == want[0]
        for i in range(0 if ragged else nsub):
            lo, hi = cuts[i], cuts[i + 1]
            ni = range_pad[i] if range_pad else audio.shape[1]
            alone, alone_len, _ = model.encoder(audio[lo:hi, :ni].contiguous(), lens[lo:hi].contiguous())
            _, lab, n = model._head(alone, alone_len)
            ti = alone.shape[1]
            bit_ok = bit_ok and torch.equal(enc[lo:hi, :ti], alone) and float(enc[lo:hi, ti:].abs().sum()) == 0.0 and \
                torch.equal(enc_len[lo:hi], alone_len) and torch.equal(label_len[lo:hi], n) and torch.equal(labels[lo:hi, :ti], lab)
            rows = sorted({lo, lo + (hi - lo) // 3, lo + 2 * (hi - lo) // 3, hi - 1})
            with torch.no_grad():
                ref, ref_len = R.encoder(audio[rows, :ni].cpu(), lens[rows].cpu(), osd, plan)
                ref_logits = R.ctc_logits(ref, osd)
                want = R.ctc_greedy(ref_logits, ref_len)
            got = enc[rows, :ref.shape[1]].cpu()
            d = (got - ref).abs()
            worst_max, worst_mean = max(worst_max, float(d.max())), max(worst_mean, float(d.mean()))
            n_oracle += len(rows)
            am = R.ctc_logits(got, osd).argmax(-1)
            for j, r in enumerate(rows):
                t = int(ref_len[j])
                flips += int((am[j, :t] != ref_logits[j, :t].argmax(-1)).sum()); frames += t
                mine = labels[r, :int(label_len[r])].cpu().tolist()
                dist += edit_distance(mine, want[j]); nlab += len(want[j])
                seq_equal = seq_equal and mine == want[j]
    finally:
        model.encoder.sub_batches, model.encoder.trim_sub_batches = saved
        model.encoder.ragged = ragged
    ok = bit_ok and finite and worst_max <= tol_max and worst_mean <= tol_mean and (args.precision == "bf16" or seq_equal)
    return {"ok": bool(ok), "finite": finite,
            ("bit_identical_to_each_sampled_utterance_run_alone" if ragged else "bit_identical_to_each_range_run_alone_on_one_stream"): bool(bit_ok),
            "oracle_utterances": n_oracle, "max_abs_err_vs_oracle": worst_max, "mean_abs_err_vs_oracle": worst_mean,
            "tolerance": {"max": tol_max, "mean": tol_mean},
            "argmax_flips_vs_oracle": flips, "frames_compared": frames, "label_edit_distance_vs_oracle": dist, "oracle_labels": nlab,
            "label_sequences_identical_to_oracle": bool(seq_equal),
            # north_star: "CTC greedy-decode label sequences bit-identical".  `ok` requires it only in the label-exact modes (--precision split / fp32); on the
            # bf16 path it is REPORTED here, never implied: a bf16 line with this field false does not meet that sentence
            "label_exact_requirement": ("required and met" if seq_equal else "REQUIRED AND NOT MET") if args.precision != "bf16"
                                       else ("met on the sampled utterances (not guaranteed: bf16 operands)" if seq_equal else
                                             "NOT MET on this path: %d argmax flips in %d frames, label edit distance %d of %d (use --precision split)" % (flips, frames, dist, nlab)),
            "note": "encoder output + greedy labels of the last timed step; oracle = fp32 CPU restatement of the reference (oracle/ref_encoder.py) "
                    + ("on each sampled utterance ALONE (batch size 1: what a ragged batch computes; the reference's collated batch differs from it "
                       "by the pad-frame leakage of SURVEY.md 8a)" if ragged else "on sampled utterances collated with their range's longest utterance")}


def self_check_sharded(model, sd, plan, audio, lens, lens_np, cuts, range_pad, nsub, last, args, world):
    """N > 1 (--gather outputs): what rank 0 holds after the LAST timed step - the gathered chunk of every row range (all ranks' rows) and
    the labels its head computed from them - against un-timed reruns on rank 0: (1) rank 0's own rows - ragged: sampled utterances run
    ALONE, rectangular: every row range alone - equal bit for bit after the wire rounding (fp32 wire: bit-identical to the producer);
    (2) ragged: one utterance of up to three OTHER ranks, regenerated from its seed and run alone here; (3) the oracle on rank 0's samples.
    (Reference sharding: main.py:33-35, 217-220; model_ctc.py:70-75.)"""
    from oracle import ref_encoder as R
    torch.cuda.synchronize()
    chunks = last["chunks"]
    heads = [ch.labels for ch in chunks]
    tol_max, tol_mean = tolerance(args.precision)
    if args.wire == "bf16":
        tol_max += 2.0 ** -7            # + the wire rounding of O(1) outputs (values up to ~4: half an ulp = 2^-7)
    osd = {k[len("encoder."):] if k.startswith("encoder.") else k: torch.from_numpy(v) for k, v in sd.items()}
    enc_ = model.encoder
    saved = (enc_.sub_batches, enc_.trim_sub_batches, enc_.ragged, enc_.sub_batch_bounds)
    ragged = bool(enc_.ragged)
    enc_.sub_batches, enc_.trim_sub_batches, enc_.ragged, enc_.sub_batch_bounds = 1, False, False, None
    to_wire = (lambda t: t.to(torch.bfloat16)) if args.wire == "bf16" else (lambda t: t)
    bit_ok, others_ok, finite = True, True, True
    worst_max = worst_mean = 0.0
    n_oracle = n_other = flips = frames = dist_ = nlab = 0
    seq_equal = True

    def alone_vs_chunk(ch, hd, row, x, xl, li, oracle):
        nonlocal bit_ok, worst_max, worst_mean, n_oracle, flips, frames, dist_, nlab, seq_equal
        al, al_len, _ = enc_(x[:, :li].contiguous(), xl.contiguous())
        ti = al.shape[1]
        got = ch.out[row]
        _, lab, nl = model._head(to_wire(al).float(), al_len)
        same = int(ch.out_len[row]) == ti and torch.equal(got[:ti], to_wire(al[0])) and float(got[ti:].float().abs().sum()) == 0.0 and \
            int(hd[1][row]) == int(nl[0]) and torch.equal(hd[0][row, :ti], lab[0, :ti])
        if oracle:
            with torch.no_grad():
                ref, ref_len = R.encoder(x[:, :li].cpu(), xl.cpu(), osd, plan)
                ref_logits = R.ctc_logits(ref, osd)
                want = R.ctc_greedy(ref_logits, ref_len)
            g = got[:ref.shape[1]].float().cpu().unsqueeze(0)
            d = (g - ref).abs()
            worst_max, worst_mean = max(worst_max, float(d.max())), max(worst_mean, float(d.mean()))
            n_oracle += 1
            t = int(ref_len[0])
            flips += int((R.ctc_logits(g, osd).argmax(-1)[0, :t] != ref_logits[0, :t].argmax(-1)).sum()); frames += t
            mine = hd[0][row, :int(hd[1][row])].cpu().tolist()
            dist_ += edit_distance(mine, want[0]); nlab += len(want[0])
            seq_equal = seq_equal and mine == want[0]
        return same
    try:
        for ch, hd in zip(chunks, heads):
            n = ch.hi - ch.lo
            finite = finite and bool(torch.isfinite(ch.out.float()).all())
            if ragged:
                for j in sorted({0, n // 2, n - 1}):
                    r = ch.lo + j
                    bit_ok = alone_vs_chunk(ch, hd, j, audio[r:r + 1], lens[r:r + 1], int(lens_np[r]), True) and bit_ok
            else:
                i = cuts.index(ch.lo)
                ni = range_pad[i] if range_pad else audio.shape[1]
                al, al_len, _ = enc_(audio[ch.lo:ch.hi, :ni].contiguous(), lens[ch.lo:ch.hi].contiguous())
                _, lab, nl = model._head(to_wire(al).float(), al_len)
                ti = al.shape[1]
                bit_ok = bit_ok and torch.equal(ch.out[:n, :ti], to_wire(al)) and float(ch.out[:n, ti:].float().abs().sum()) == 0.0 and \
                    torch.equal(ch.out_len[:n], al_len) and torch.equal(hd[1][:n], nl) and torch.equal(hd[0][:n, :ti], lab)
                rows = sorted({0, n // 2, n - 1})
                with torch.no_grad():
                    ref, ref_len = R.encoder(audio[[ch.lo + j for j in rows], :ni].cpu(), lens[[ch.lo + j for j in rows]].cpu(), osd, plan)
                    ref_logits = R.ctc_logits(ref, osd)
                    want = R.ctc_greedy(ref_logits, ref_len)
                g = ch.out[rows, :ref.shape[1]].float().cpu()
                d = (g - ref).abs()
                worst_max, worst_mean = max(worst_max, float(d.max())), max(worst_mean, float(d.mean()))
                n_oracle += len(rows)
                am = R.ctc_logits(g, osd).argmax(-1)
                for q, j in enumerate(rows):
                    t = int(ref_len[q])
                    flips += int((am[q, :t] != ref_logits[q, :t].argmax(-1)).sum()); frames += t
                    mine = hd[0][j, :int(hd[1][j])].cpu().tolist()
                    dist_ += edit_distance(mine, want[q]); nlab += len(want[q])
                    seq_equal = seq_equal and mine == want[q]
        if ragged:          # rows that came over the wire from OTHER ranks: regenerate that rank's batch from its seed, run one utterance alone
            ch, hd = chunks[0], heads[0]
            n = ch.hi - ch.lo
            for rr in range(1, min(world, 4)):
                a_np, l_np = make_batch(args, rr, world)
                r = ch.lo
                xa = torch.from_numpy(a_np[r:r + 1]).to(audio.device); xl = torch.from_numpy(l_np[r:r + 1]).to(audio.device)
                others_ok = alone_vs_chunk(ch, hd, rr * n, xa, xl, int(l_np[r]), False) and others_ok
                n_other += 1
    finally:
        enc_.sub_batches, enc_.trim_sub_batches, enc_.ragged, enc_.sub_batch_bounds = saved
    ok = bit_ok and others_ok and finite and worst_max <= tol_max and worst_mean <= tol_mean and (args.precision == "bf16" or seq_equal)
    return {"ok": bool(ok), "finite": finite, "world": world, "wire": args.wire,
            "rank0_rows_of_every_gathered_chunk_equal_their_rerun_alone_after_wire_rounding": bool(bit_ok),
            "rows_received_from_other_ranks_equal_that_utterance_run_alone_here": bool(others_ok), "other_rank_utterances": n_other,
            "oracle_utterances": n_oracle, "max_abs_err_vs_oracle": worst_max, "mean_abs_err_vs_oracle": worst_mean,
            "tolerance": {"max": tol_max, "mean": tol_mean},
            "argmax_flips_vs_oracle": flips, "frames_compared": frames, "label_edit_distance_vs_oracle": dist_, "oracle_labels": nlab,
            "label_sequences_identical_to_oracle": bool(seq_equal),
            "note": "rank 0 after the last timed step: gathered encoder outputs (wire dtype) + the labels its head computed from them; "
                    "oracle = oracle/ref_encoder.py on sampled utterances of rank 0 (" + ("each alone" if ragged else "collated with their range") + ")"}



def host_cpu():
    """(model string, physical cores, logical cpus) of the host the baseline runs on."""
    model, cores = "unknown", set()
    try:
        phys = core = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model == "unknown":
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                phys = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                core = line.split(":", 1)[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    cores.add((phys, core))
                phys = core = None
    except OSError:
        pass
    logical = os.cpu_count() or 1
    return model, (len(cores) or logical), logical


def cpu_baseline(sd, plan, budget_s=24.0):
    """The oracle (CPU port of the reference path, oracle/ref_encoder.py) on the host cores, BASELINE.md section 3: same timed
    region (audio -> encoder -> fc -> greedy labels), W-fixed B = 4 (10 s utterances) for torch.set_num_threads in {1, 8, 16, 32,
    all physical cores}, then a W-libri B = 4 sample and W-fixed B = 32 at the best thread count.  The headline `value` is the
    best W-fixed B = 4 rate; every measurement is listed.  Bounded to about `budget_s` seconds."""
    from oracle import ref_encoder as R
    osd = {k[len("encoder."):] if k.startswith("encoder.") else k: torch.from_numpy(v) for k, v in sd.items()}
    model, phys, logical = host_cpu()
    rnnt = "decoder.embedding.weight" in sd
    if rnnt:
        from oracle import ref_transducer as RT

    def measure(lens_np, seed, threads, seconds):
        torch.set_num_threads(threads)
        lens = torch.from_numpy(lens_np)
        audio = torch.from_numpy(synth.make_audio(lens_np, seed=seed))
        frames = int((lens // plan.hop_length + 1).sum())

        def run():
            with torch.no_grad():
                x, l = R.encoder(audio, lens, osd, plan)
                if rnnt:
                    return RT.greedy_decode(osd, x, l, 5)
                return R.ctc_greedy(R.ctc_logits(x, osd), l)
        run()
        times = []
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < seconds or len(times) < 2:
            t1 = time.perf_counter()
            run()
            times.append(time.perf_counter() - t1)
        return frames / float(np.median(times)), len(times)

    prev = torch.get_num_threads()
    runs = []
    fixed4 = np.full(4, 160000, dtype=np.int64)
    cand = sorted({t for t in (1, 8, 16, 32, phys) if t <= logical})
    per = budget_s * 0.6 / len(cand)
    for t in cand:
        v, n = measure(fixed4, 1234, t, per)
        runs.append({"workload": "W-fixed B=4 (10 s)", "threads": t, "value": v, "iters": n})
    best = max(runs, key=lambda r: r["value"])
    v, n = measure(np.sort(synth.libri_lengths(4, seed=1234))[::-1].copy(), 1234, best["threads"], budget_s * 0.15)
    runs.append({"workload": "W-libri B=4", "threads": best["threads"], "value": v, "iters": n})
    v, n = measure(np.full(32, 160000, dtype=np.int64), 1234, best["threads"], budget_s * 0.25)
    runs.append({"workload": "W-fixed B=32 (10 s)", "threads": best["threads"], "value": v, "iters": n})
    torch.set_num_threads(prev)
    one = [r for r in runs if r["threads"] == 1][0]
    same = [r for r in runs if r["workload"] == "W-libri B=4"][0]
    # `value` = the SAME workload as the GPU line (W-libri: LibriSpeech-shaped lengths, collated and padded as the reference does), a B = 4 sample of it at the
    # best thread count; the W-fixed figures (the reference's own eval_time shape) are listed beside it
    return {"value": same["value"], "unit": "mel-frames/s (valid)", "cores": same["threads"], "kind": "port",
            "cpu_model": model, "physical_cores": phys, "logical_cpus": logical, "single_thread_value": one["value"],
            "sample": "fp32 torch oracle (oracle/ref_encoder.py: audio -> mel -> encoder -> fc -> greedy labels) on a B = 4 sample of the GPU line's workload "
                      "(W-libri lengths, seed 1234, sorted, zero-padded to the longest as the reference's collate does; valid frames counted), median of %d "
                      "passes on %d threads - the best thread count of the W-fixed B = 4 sweep over %s threads (all runs listed)" % (same["iters"], same["threads"], cand),
            "w_fixed_b4_best_value": best["value"],
            "same_workload_sample_value": same["value"],
            "runs": runs}


def _nccl_version():
    """RCCL's version as torch reports it (None if this build does not expose it: never a reason to fail a multi-rank run)."""
    try:
        v = torch.cuda.nccl.version()
        return ".".join(str(x) for x in v) if isinstance(v, (tuple, list)) else str(v)
    except Exception:
        return None


def pmc_traffic(args, kernel_prefix):
    """HBM bytes per launch of the dominant kernel class from the committed PMC passes (profiles/pmc_traffic.json, written
    by tools/pmc_summary.py from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs of this same command).  Counters
    cannot be read from inside the timed process, so this is only filled when the run matches the profiled configuration."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if not os.path.exists(path) or kernel_prefix is None:
        return None
    d = json.load(open(path))
    if (d.get("model"), d.get("batch"), d.get("workload"), d.get("streams", 1)) != (args.model, args.batch, args.workload, max(args.streams, 1)):
        return None
    import re
    calls = tot = 0
    for name, k in d["kernels"].items():
        if re.search(kernel_prefix, name):
            calls += k["calls"]
            tot += k["calls"] * (k["fetch_x2_bytes"] + k["write_bytes"])
    return tot / calls if calls else None


# kernel class -> (what it is, bounding roofline, rocprof kernel-name pattern for the PMC traffic)
CLASS_INFO = {
    "mel": ("mel_kernel (log-mel frontend)", "hbm", r"mel_kernel"),
    "subsample_conv": ("conv subsampling (sublinear2_kernel / sublinear3_kernel / sublinear_kernel: fused 3x3 conv + Linear, sxf_sublin_kernel in split mode; subsample_conv_* for two layers)", "mfma", r"sublinear[23]?_kernel|sxf_sublin_kernel|subsample_conv"),
    "gemm_ffn": ("FFN-carrying kernels: chain_kernel A (pointwise-2 + FFN2 + block norm + next FFN1 + attention pre-norm + QKV in one pass over "
                 "the rows); ffn_fused_kernel / gemm_kernel where a chain is not supported", "mfma", r"chain_kernel<\d+, \d+, \d+, [123],|chain2_kernel<\d+, [123],|chain3_kernel<\d+, [123],|ffn_fused_kernel"),
    "gemm_other": ("chain_kernel B (attention output projection + conv-module LayerNorm + pointwise-1 + GLU), rs_gemm / gemm_kernel projections", "mfma",
                   r"chain_kernel<\d+, \d+, \d+, 0,|chain2_kernel<\d+, 0,|rs_gemm_kernel|gemm_kernel"),
    "layernorm": ("layernorm_kernel", "hbm", r"layernorm_kernel"),
    "attention": ("relpos_attention2_kernel / relpos_attention_kernel (grouped relative-position MHSA, QK^T + QE^T + softmax + PV)", "mfma", r"relpos_attention2?_kernel"),
    "dwconv": ("dwconv_mfma_kernel / dwconv_kernel (depthwise conv + BN + Swish)", "hbm", r"dwconv(_mfma)?_kernel"),
    "misc": ("lengths / pad rows / casts", "hbm", None),
}


def result_skeleton(args, world, value, ms_per_step, gb, extra_cfg):
    extra_cfg = dict(extra_cfg)
    padding = extra_cfg.pop("_padding", "")
    label = args.model.replace("EfficientConformer", "EffConformer").replace("CTCSmall", "CTC-Small")
    return {
        "metric": "audio-frames/sec through encoder, %s, 1/2/4/8 GPU" % label,
        "value": value, "unit": "mel-frames/s (valid, 10 ms hop)",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": {"bf16": "bf16", "fp32": "f32", "split": "f16x2 (split fp32 operands, fp32 accumulate)"}[args.precision], "data": "synthetic",
        "config": dict({"workload": "%s: %s, B=%d utterances/GPU%s, %s lengths, audio in HBM -> encoder out + greedy labels"
                                    % (args.model, {"bf16": "bf16 operands / fp32 accumulate", "fp32": "fp32 operands (label-exact mode)",
                                                    "split": "fp32 tensors, every product on the fp16 matrix pipe with split operands x = h + l / 2048 (label-exact mode, 3 MFMAs per product)"}[args.precision],
                                       args.batch,
                                       " (the largest single-GPU batch measured; SURVEY.md 8d lists B in {4, 32, 128}: --batch 128 is 0.79 x this rate, profiles/r5_31_bench_b128.json)" if args.batch == 256 else "",
                                       ("lognormal 1.5-16 s (LibriSpeech-shaped), sorted desc; " + padding)
                                       if args.workload == "libri" else "10 s"),
                        "global_batch": gb, "streams_per_gpu": args.streams}, **extra_cfg),
    }


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    multi = world > 1 or args.force_dist          # the multi-rank code path (process group, ShardedEncoder)
    if args.force_dist and world == 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29517")
        os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d: launch N ranks with `python bench.py --gpus N` or with "
                         "torch.distributed.run --nproc-per-node N ... bench.py --gpus N" % (args.gpus, world))
    dist = None
    if multi:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")

    if args.dry_run:           # CPU-only plumbing check (tests): same launcher, same batch plan, gloo instead of RCCL
        if multi:
            dist.init_process_group("gloo")
        audio_np, lens_np = make_batch(args, rank, world)
        t = torch.tensor([float(audio_np.shape[1]), float((lens_np // 160 + 1).sum())], dtype=torch.float64)
        lo = t.clone()
        if multi:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        if rank == 0:
            r = result_skeleton(args, world, 0.0, 0.0, args.batch * world, {"parallelism": "dp%d" % world, "_padding": "dry run"})
            r.update({"dry_run": True, "padded_samples_equal_on_all_ranks": bool(t[0] == lo[0] * world), "valid_frames_per_step": float(t[1])})
            print(json.dumps(r))
        if multi:
            dist.barrier()
            dist.destroy_process_group()
        return

    assert torch.cuda.is_available(), "bench.py needs a GPU (HIP path only)"
    dev = torch.device("cuda", 0 if args.one_device else local_rank)
    torch.cuda.set_device(dev)
    if multi:
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")

    cfg, model, sd = build_model(args.model)
    if args.ragged < 0:
        args.ragged = int(args.precision in ("bf16", "split") and args.workload == "libri" and not args.no_trim)      # round 6: the split mode takes ragged batches
    model.encoder.precision = args.precision
    model = model.to(dev)
    plan = model.encoder.plan
    audio_np, lens_np = make_batch(args, rank, world)
    audio, lens = torch.from_numpy(audio_np).to(dev), torch.from_numpy(lens_np).to(dev)
    valid_frames = int((lens_np // plan.hop_length + 1).sum())
    padded_frames = int(args.batch * (audio_np.shape[1] // plan.hop_length + 1))

    # Sub-batch streams live in the library's host layer (ConformerEncoder.sub_batches): the batch runs as `--streams` contiguous
    # row ranges on concurrent HIP streams and is joined before forward() returns.
    nsub = max(args.ranges, 1) if args.ranges > 0 else max(args.streams, 1)
    model.encoder.sub_batches = nsub
    model.encoder.sub_batch_streams = max(args.streams, 1)
    # Row ranges padded to their own longest utterance (ConformerEncoder.trim_sub_batches): the batch is length-sorted, so range i
    # of every rank is padded to the longest utterance any rank holds in range i (known from the seeds: no exchange, equal shapes)
    model.encoder.ragged = bool(args.ragged)
    model.encoder.trim_sub_batches = not args.ragged and not args.no_trim and nsub > 1 and args.workload == "libri"
    range_pad = None
    cuts = [args.batch * i // nsub for i in range(nsub + 1)]
    if args.batch >= 32 * nsub:      # ConformerEncoder's own default boundaries (multiples of 16 rows)
        cuts = [c - c % 16 for c in cuts[:-1]] + [args.batch]
    if model.encoder.trim_sub_batches:
        all_lens = [synth.libri_lengths(args.batch, seed=1234 + r) for r in range(world)]
        if args.balanced_split:
            # the batch is sorted by length: cut it so that every range holds about the same number of PADDED frames (rows x the range's
            # longest utterance) - the long utterances' range gets fewer rows.  Greedy on rank 0's lengths; the same cuts on every rank.
            fr = all_lens[0] // plan.hop_length + 1
            cuts = balanced_cuts(fr, nsub)
            model.encoder.sub_batch_bounds = cuts[1:-1]
        if args.cuts:
            cuts = [0] + [int(v) for v in args.cuts.split(",")] + [args.batch]
            model.encoder.sub_batch_bounds = cuts[1:-1]
        model.encoder.sub_batch_bounds = cuts[1:-1]      # the boundaries range_pad is computed for
        range_pad = [max(int(l[cuts[i]:cuts[i + 1]].max()) for l in all_lens) for i in range(nsub)]
        padded_frames = int(sum((cuts[i + 1] - cuts[i]) * (range_pad[i] // plan.hop_length + 1) for i in range(nsub)))
    if args.attention >= 0:
        model.encoder.set_option("attention_v2", args.attention)
    if args.subsample >= 0:
        model.encoder.set_option("fuse_subsample", args.subsample)
    if args.wide_gemm >= 0:
        model.encoder.set_option("wide_gemm", args.wide_gemm)
    for opt in args.opt:                                      # tuning: any library option, e.g. --opt chain_max_dim=192
        k, v = opt.split("=")
        model.encoder.set_option(k, int(v))
    if args.ragged and nsub > 1 and (multi or args.range_frames):
        # every rank must cut the SAME row ranges (the per-range collectives are fixed-size): frame-balanced (or --range-frames shares) cuts
        # computed from the MEAN cumulative valid frames over the ranks' batches - all known from the seeds, so no exchange is needed
        fr = np.mean([np.cumsum(synth.libri_lengths(args.batch, seed=1234 + r) // plan.hop_length + 1) for r in range(world)], axis=0) \
            if args.workload == "libri" else np.cumsum(np.full(args.batch, 1001.0))
        shares = [float(v) for v in args.range_frames.split(",")] if args.range_frames else [100.0 / nsub] * nsub
        if len(shares) != nsub:
            raise SystemExit("--range-frames needs one share per row range (%d)" % nsub)
        acc, cuts = 0.0, [0]
        for i in range(nsub - 1):
            acc += shares[i] / sum(shares)
            c = int(np.searchsorted(fr, acc * fr[-1]))
            c = (c + 4) // 8 * 8 if args.batch >= 16 * nsub else c
            cuts.append(max(cuts[-1] + 1, min(args.batch - (nsub - 1 - i), c)))
        cuts.append(args.batch)
        model.encoder.sub_batch_bounds = cuts[1:-1]
    hkw = {"x_len_host": lens_np} if args.ragged else {}       # ragged batches size their grids from the lengths on the host
    if args.ragged:
        padded_frames = valid_frames                            # no pad frames exist (an utterance's rows are only rounded up to the group size)
    sharded = None
    if multi:
        from efficientconformer_amd.dist import ShardedEncoder
        if args.wire == "auto":
            args.wire = "bf16" if args.precision == "bf16" else "fp32"
        if args.pipeline_gather < 0:
            args.pipeline_gather = 1
        sharded = ShardedEncoder(model.encoder, wire_dtype=torch.bfloat16 if args.wire == "bf16" else None,
                                 pipelined=bool(args.pipeline_gather) and args.gather == "outputs")
    last = {}

    def full_step():
        if not multi:
            if isinstance(model, Transducer):
                enc, enc_len, _ = model.encoder(audio, lens, range_pad=range_pad, **hkw)
                last["labels"] = head(model, enc, enc_len)
            else:      # fc + argmax + collapse of every row range on that range's stream (ModelCTC.encode_greedy)
                enc, enc_len, labels, label_len = model.encode_greedy(audio, lens, range_pad=range_pad, **hkw)
                last["labels"] = (labels, label_len)
            last["enc"] = (enc, enc_len)
            return
        if args.gather == "outputs":
            # encoder on this rank's utterances; per-row-range all-gather issued from each range's stream (dist.py); the head consumes
            # the gathered chunk on that same stream (no extra streams: see dist.py on the four-stream budget)
            def consume(ch):          # the CTC head on a gathered chunk, on its row range's stream (pipelined: one step after its collective was issued)
                # bf16 wire + CTC head: the gathered bf16 rows go to the head as they are (effconf_ctc_greedy_bf16: labels identical to the fp32-input
                # head on the widened values, tests/test_gpu_round4.py); the transducer decode and the exact modes take fp32 rows
                direct = ch.out.dtype == torch.float32 or (ch.out.dtype == torch.bfloat16 and not isinstance(model, Transducer))
                ch.labels = head(model, ch.out if direct else ch.out.float(), ch.out_len)
            g = sharded.encode_shard(audio, lens, args.batch * world, range_pad=range_pad, consumer=consume, **hkw)
            last["chunks"] = g.chunks
        else:
            # the head per row range on that range's stream, then ONE small collective of the label ids on the caller's stream
            enc, enc_len, labels, label_len = model.encode_greedy(audio, lens, range_pad=range_pad, **hkw)
            gl = labels.new_empty((world,) + tuple(labels.shape)); gn = label_len.new_empty((world,) + tuple(label_len.shape))
            from efficientconformer_amd.dist import _all_gather
            _all_gather(gl, labels)
            _all_gather(gn, label_len)
            last["labels"], last["enc"], last["gathered_labels"] = (labels, label_len), (enc, enc_len), (gl, gn)

    def drain():                       # pipelined gather: the last step's collectives are consumed here (inside the timed region)
        if sharded is not None:
            sharded.flush()

    for _ in range(args.warmup):
        full_step()
    drain()
    if multi:
        dist.barrier()
    torch.cuda.synchronize()
    # per-step distribution: one event per step on the caller's stream (every step joins its range streams there); no synchronisation
    # inside the timed region - `value` comes from the wall clock around all K steps
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(args.steps):
        full_step()
        marks[i + 1].record()
    drain()
    torch.cuda.synchronize()
    if multi:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    tot = torch.tensor([elapsed, float(valid_frames), float(padded_frames)], dtype=torch.float64, device=dev)
    if multi:
        mx = tot.clone()
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)
        elapsed = float(mx[0])
    all_valid, all_padded = float(tot[1]), float(tot[2])
    if rank == 0 and args.dump_outputs:            # un-timed, before any other leg runs a forward
        dump_outputs(args.dump_outputs, step_outputs(model, last, multi, args))

    # what every rank's transport looked like (the driver's SCALE record should show that RCCL saw N ranks): backend and
    # communicator size as torch.distributed reports them, GPU_MAX_HW_QUEUES as this process exported it before the HIP runtime started, the device,
    # and the bytes this rank put on the wire per step (its shard of every row range's all-gather)
    transport = None
    if multi:
        if args.gather == "outputs" and last.get("chunks"):
            mine = sum(int(ch.out.numel()) * ch.out.element_size() + int(ch.out_len.numel()) * ch.out_len.element_size() for ch in last["chunks"]) // world
        elif last.get("gathered_labels"):
            mine = sum(int(t.numel()) * t.element_size() for t in last["gathered_labels"]) // world
        else:
            mine = 0
        info = {"rank": rank, "backend": dist.get_backend(), "comm_nranks": dist.get_world_size(), "device": str(dev),
                "device_name": torch.cuda.get_device_name(dev), "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"),
                "HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"),
                "nccl_version": _nccl_version() if dist.get_backend() == "nccl" else None,
                "wire_bytes_sent_per_step": mine, "wire_bytes_received_per_step": mine * (world - 1)}
        gathered = [None] * world
        dist.all_gather_object(gathered, info)
        transport = gathered

    result = None
    if rank == 0:
        par = "dp%d%s (utterance shards" % (world, ", ALL RANKS ON ONE GPU over gloo: a functional test, not a benchmark" if args.one_device else "")
        if multi:
            par += ", RCCL all-gather of %s per row range on a comm stream, wire %s%s" % ("encoder outputs" if args.gather == "outputs" else "label ids", args.wire,
                   ", pipelined: the head of a gathered chunk runs one step later" if (sharded is not None and sharded.pipelined) else "")
        step_ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
        pct = lambda q: step_ms[min(len(step_ms) - 1, int(q * len(step_ms)))]
        result = result_skeleton(args, world, all_valid * args.steps / elapsed, 1000.0 * elapsed / args.steps, args.batch * world,
                                 {"padded_frames_per_s": all_padded * args.steps / elapsed, "parallelism": par + ")",
                                  "step_ms": {"p10": pct(0.10), "median": pct(0.50), "p90": pct(0.90), "note": "HIP events between steps on the caller's stream (rank 0); "
                                              "ms_per_step / value are wall clock over all steps"},
                                  "padded_fraction": 1.0 - all_valid / all_padded,
                                  "_padding": "ragged: every utterance at its own length in one concatenated row space per row range (no pad frames; outputs = the "
                                              "reference's for each utterance alone)" if args.ragged else
                                              ("each of the %d row ranges zero-padded to ITS longest utterance (length bucketing inside the forward)" % nsub) if range_pad
                                              else "zero-padded to the batch's longest utterance",
                                  "row_ranges": ("%d row ranges per GPU (rows %s), each padded to ITS longest utterance %s samples (length bucketing inside "
                                                 "the forward; --no-trim pads all to the batch maximum as in round 1)" % (nsub, cuts, range_pad)) if range_pad
                                                else ("%d ragged row range(s) per GPU, cut for equal valid frames" % nsub) if args.ragged
                                                else "%d row range(s) per GPU padded to the batch maximum" % nsub})
        if isinstance(model, Transducer):
            result["config"]["workload"] += " (RNN-T greedy token ids, synthetic blank bias %.1f)" % RNNT_BLANK_BIAS
        if transport is not None:
            result["transport"] = transport

    # ---- self-check of the benchmarked step (un-timed): the step's outputs against (1) every row range run ALONE on one stream
    #      (bit-identical) and (2) the oracle = the reference path on sampled utterances of each range, collated with the range's
    #      longest utterance (pad frames are live), within the bf16 tolerance of tests/test_gpu_encoder.py
    if rank == 0 and not args.no_check:
        if multi and args.gather == "outputs" and not isinstance(model, Transducer):
            result["check"] = self_check_sharded(model, sd, plan, audio, lens, lens_np, cuts, range_pad, nsub, last, args, world)
        elif isinstance(model, Transducer):
            if not multi:
                result["check"] = self_check_transducer(model, sd, plan, audio, lens, lens_np, last)
        else:
            result["check"] = self_check(model, sd, plan, audio, lens, lens_np, cuts, range_pad, nsub, last, args)
            if multi:      # --gather labels: this rank's slice of the gathered label ids is its own head output
                gl, gn = last["gathered_labels"]
                same = bool(torch.equal(gl[rank], last["labels"][0]) and torch.equal(gn[rank], last["labels"][1]))
                result["check"]["gathered_label_ids_of_this_rank_equal_its_head_output"] = same
                result["check"]["ok"] = bool(result["check"]["ok"] and same)

    # ---- roofline leg: the same steps again with every launch bracketed by HIP events on the launch stream
    if rank == 0 and not args.no_roofline:
        lib = _lib.load()
        h = model.encoder._handle
        _lib.check(lib.effconf_profile_enable(h, 1), "profile_enable")
        nprof = min(args.steps, 5)

        def read_classes():
            torch.cuda.synchronize()
            out = {}
            for ci, cname in enumerate(PROF_CLASSES):
                ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
                _lib.check(lib.effconf_profile_read(h, ci, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)), "profile_read")
                out[cname] = {"ms_per_step": ms.value / nprof, "launches_per_step": n.value / nprof,
                              "gflop_per_step": fl.value / nprof / 1e9, "alg_mb_per_step": by.value / nprof / 1e6}
            return out
        # Launch durations, two launch shapes, both on ONE stream (no neighbour kernel on the chip; with S streams in flight an event pair also
        # brackets the time its kernel queues behind another stream's: reported as `in_flight`, not a kernel duration):
        #   "timed"      the launches of the TIMED region - the step's row ranges, same rows per launch - one range after the other.  This is
        #                the shape `roofline.achieved / frac / traffic` describe and the one the rocprofv3 --pmc pass of the same command shows
        #                (counter collection serialises dispatches): profiles/rN_pmc_hbm_traffic.txt, second table.
        #   "full_batch" ragged batches only: the whole batch as ONE range (launches three times the size, every one alone on the chip) -
        #                rounds 3's roofline leg; kept as `roofline.full_batch_launch` so that the two rounds stay comparable.
        def serial_steps(n, one_range):
            for _ in range(n):
                if args.ragged:
                    model.encoder.sub_batches = 1 if one_range else nsub
                    model.encoder.sub_batch_streams = 1          # every range on the caller's stream, one after the other
                    step_greedy()
                    continue
                model.encoder.sub_batches = 1                    # rectangular ranges: each range as its own forward
                for i in range(nsub):
                    lo, hi = cuts[i], cuts[i + 1]
                    step(model, audio[lo:hi, :range_pad[i]].contiguous() if range_pad else audio[lo:hi], lens[lo:hi])

        def step_greedy():        # the timed step's own call (head per range on the range's stream); Transducer: encoder + decode
            if isinstance(model, Transducer):
                step(model, audio, lens, range_pad, **hkw)
            else:
                model.encode_greedy(audio, lens, range_pad=range_pad, **hkw)

        def profiled(one_range):
            # one un-profiled pass first: this leg runs on the caller's stream with its own (fresh) workspaces - first-touch costs of those
            # allocations landed inside single event brackets otherwise (one run in three reported a 2x class time)
            _lib.check(lib.effconf_profile_enable(h, 0), "profile_enable")
            serial_steps(1, one_range)
            torch.cuda.synchronize()
            _lib.check(lib.effconf_profile_enable(h, 1), "profile_enable")
            serial_steps(nprof, one_range)
            return read_classes()
        saved_sub = (model.encoder.sub_batches, model.encoder.sub_batch_streams)
        per = profiled(False)
        per_full = profiled(True) if (args.ragged and nsub > 1) else None
        model.encoder.sub_batches, model.encoder.sub_batch_streams = saved_sub
        # the dominant class is the one that takes the most time in THIS model's step (gemm_ffn for Small; Large's tiled GEMMs too)
        dom_name = max(PROF_CLASSES, key=lambda c: per[c]["ms_per_step"])
        flight = None
        if nsub > 1:
            _lib.check(lib.effconf_profile_enable(h, 0), "profile_enable")
            step_greedy()
            torch.cuda.synchronize()
            _lib.check(lib.effconf_profile_enable(h, 1), "profile_enable")
            for _ in range(nprof):
                step_greedy()
            flight = read_classes()[dom_name]
        _lib.check(lib.effconf_profile_enable(h, 0), "profile_enable")
        for table in (per, per_full):
            for cname, c in (table or {}).items():      # every class against its BINDING roofline: min(MFMA peak, arithmetic intensity x HBM peak)
                ms = max(c["ms_per_step"], 1e-9)
                tf, gbs = c["gflop_per_step"] / ms, c["alg_mb_per_step"] / ms                                    # achieved TFLOP/s, GB/s (algorithmic flop / bytes)
                inten = c["gflop_per_step"] * 1e3 / c["alg_mb_per_step"] if c["alg_mb_per_step"] > 0 else 0.0     # flop per byte
                ridge = PEAK_BF16_TFLOPS * 1e3 / PEAK_HBM_GBS                                                    # 312 flop / B
                bound = "mfma" if (CLASS_INFO[cname][1] == "mfma" and inten >= ridge) else "hbm"
                c["bound"] = bound
                c["intensity_flop_per_byte"] = inten
                c["achieved"] = tf if bound == "mfma" else gbs                                                   # TFLOP/s | GB/s
                c["frac"] = c["achieved"] / (PEAK_BF16_TFLOPS if bound == "mfma" else PEAK_HBM_GBS) if c["launches_per_step"] else 0.0
                if CLASS_INFO[cname][1] == "mfma":
                    c["mfma_tflops"], c["mfma_frac"] = tf, tf / PEAK_BF16_TFLOPS                                 # the matrix-pipe view of a GEMM-carrying class, whatever binds it
        dom = per[dom_name]
        n_l = max(dom["launches_per_step"], 1)
        if isinstance(model, Transducer):      # decode leg on its own (torch events: it is launched on torch's current stream)
            enc, enc_len, _ = model.encoder(audio, lens)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(nprof):
                toks, tok_len = model.decode_encoded(enc, enc_len)
            e1.record()
            torch.cuda.synchronize()
            dec_ms = e0.elapsed_time(e1) / nprof
            e0.record()
            for _ in range(nprof):
                model.encoder(audio, lens, range_pad=range_pad, **hkw)
            e1.record()
            torch.cuda.synchronize()
            enc_ms = e0.elapsed_time(e1) / nprof
            per["rnnt_greedy"] = {"ms_per_step": dec_ms, "launches_per_step": 2,
                                  "tokens_per_step": int(tok_len.sum()), "encoder_frames_per_step": int(enc_len.sum())}
            # the encoder by the headline metric, the greedy decode as utterances/s, each timed alone
            result["transducer_legs"] = {"encoder_valid_mel_frames_per_s": valid_frames / (enc_ms * 1e-3), "encoder_ms": enc_ms,
                                         "decode_utterances_per_s": args.batch / (dec_ms * 1e-3), "decode_ms": dec_ms,
                                         "decode_tokens_per_s": int(tok_len.sum()) / (dec_ms * 1e-3),
                                         "note": "each leg alone on one stream after the timed region; `value` is the whole step (encoder + decode)"}
        tot_ms = sum(c["ms_per_step"] for k, c in per.items() if k in PROF_CLASSES)
        tot_gf = sum(c["gflop_per_step"] for k, c in per.items() if k in PROF_CLASSES)
        result["roofline"] = {"kernel": "%s: %s" % (dom_name, CLASS_INFO[dom_name][0]),
                              "bound": dom["bound"], "achieved": dom["achieved"],
                              "peak": PEAK_BF16_TFLOPS if dom["bound"] == "mfma" else PEAK_HBM_GBS,
                              "unit": "TFLOP/s" if dom["bound"] == "mfma" else "GB/s",
                              "frac": dom["frac"], "traffic": pmc_traffic(args, CLASS_INFO[dom_name][2]),
                              "traffic_unit": "HBM bytes per launch (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, profiles/pmc_traffic.json)",
                              "alg_bytes_per_launch": 1e6 * dom["alg_mb_per_step"] / n_l,
                              "avg_launch_ms": dom["ms_per_step"] / n_l, "launches_per_step": n_l,
                              "alg_gflop_per_launch": dom["gflop_per_step"] / n_l,
                              "alg_hbm_gbs": dom["alg_mb_per_step"] / max(dom["ms_per_step"], 1e-9),
                              "share_of_step": dom["ms_per_step"] / max(tot_ms, 1e-9),
                              "whole_step": {"sum_kernel_ms": tot_ms, "alg_gflop": tot_gf, "wall_ms": result["ms_per_step"],
                                             "mfma_frac": tot_gf / max(result["ms_per_step"], 1e-9) / PEAK_BF16_TFLOPS,
                                             "mfma_frac_of_serial_kernel_time": tot_gf / max(tot_ms, 1e-9) / PEAK_BF16_TFLOPS,
                                             "note": "mfma_frac = algorithmic flop of one step / wall step time / 2.5 PF (padded frames: the work the kernels do)"},
                              "launch_shape": "the timed region's launches (its %d row range(s), same rows per launch), one range after the other on ONE stream" % nsub,
                              "note": "dominant class = most time per step; HIP events around every launch of the class on the launch stream, %d extra "
                                      "steps after the timed region, the step's %d row ranges one after the other on one stream (the launches of the timed "
                                      "region, none overlapping); kernel_classes lists every class against its own bound.  Reproduce from profiles/: the "
                                      "kernel durations of the --pmc pass of this command (dispatches serialised; second table of rN_pmc_hbm_traffic.txt), "
                                      "profiled with --no-check so that no other launch shape dilutes the averages" % (nprof, nsub)}
        if per_full:
            df = per_full[dom_name]
            nf = max(df["launches_per_step"], 1)
            result["roofline"]["full_batch_launch"] = {
                "achieved": df["achieved"], "frac": df["frac"], "avg_launch_ms": df["ms_per_step"] / nf, "launches_per_step": nf,
                "alg_gflop_per_launch": df["gflop_per_step"] / nf, "alg_bytes_per_launch": 1e6 * df["alg_mb_per_step"] / nf,
                "sum_kernel_ms": sum(c["ms_per_step"] for k, c in per_full.items() if k in PROF_CLASSES),
                "note": "the same class with the whole ragged batch as ONE row range on one stream (launches %d x the size; round 3's roofline leg "
                        "reported this shape as `frac`): NOT a launch of the timed region" % nsub}
            result["kernel_classes_full_batch_launch"] = per_full
        if flight:
            result["roofline"]["in_flight"] = {"event_bracket_ms": flight["ms_per_step"] / max(flight["launches_per_step"], 1),
                                               "note": "event pairs around the same launches with the %d row ranges in flight on %d streams, as in the timed "
                                                       "region: includes the time a kernel queues behind the other stream's kernel" % (nsub, nsub)}
        result["kernel_classes"] = per

    # ---- the reference's COLLATED-batch semantics beside the ragged headline (un-timed leg like the roofline one): utils/preprocessing.py:33-45
    #      zero-pads a batch to its longest utterance and encoders.py:107-140 runs every pad frame (they leak into valid frames).  `value` runs ragged
    #      (each utterance = the reference on it ALONE); these are the same batch, same kernels, with the pad frames computed: the whole batch padded to its maximum
    #      (`no_trim`: round 1's workload) and each row range padded to ITS maximum (`ragged0`: round 2's).  Valid frames / s, wall clock over a few steps.
    if rank == 0 and world == 1 and args.ragged and not args.no_roofline and not isinstance(model, Transducer) and args.workload == "libri":
        enc_ = model.encoder
        saved = (enc_.ragged, enc_.trim_sub_batches, enc_.sub_batch_bounds, enc_.sub_batches, enc_.sub_batch_streams)
        ref_sem = {}
        try:
            rcuts = [args.batch * i // nsub for i in range(nsub + 1)]
            if args.batch >= 32 * nsub:
                rcuts = [c_ - c_ % 16 for c_ in rcuts[:-1]] + [args.batch]
            nrep = max(3, min(args.steps, 8))
            for name, trim in (("no_trim", False), ("ragged0", True)):
                enc_.ragged, enc_.sub_batches, enc_.sub_batch_streams = False, nsub, max(args.streams, 1)
                enc_.trim_sub_batches = bool(trim and nsub > 1)
                enc_.sub_batch_bounds = rcuts[1:-1] if enc_.trim_sub_batches else None
                rp = [int(lens_np[rcuts[i]:rcuts[i + 1]].max()) for i in range(nsub)] if enc_.trim_sub_batches else None
                for _ in range(2):
                    model.encode_greedy(audio, lens, range_pad=rp)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(nrep):
                    model.encode_greedy(audio, lens, range_pad=rp)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t1) / nrep
                pf = (sum((rcuts[i + 1] - rcuts[i]) * (rp[i] // plan.hop_length + 1) for i in range(nsub)) if rp
                      else args.batch * (audio_np.shape[1] // plan.hop_length + 1))
                ref_sem[name] = {"valid_frames_per_s": valid_frames / dt, "ms_per_step": 1000.0 * dt, "padded_fraction": 1.0 - valid_frames / pf}
            ref_sem["note"] = ("the same batch with the reference's collated-batch semantics (pad frames computed and live): no_trim = the whole batch zero-padded to its longest "
                               "utterance (utils/preprocessing.py:33-45), ragged0 = each of the %d row ranges padded to ITS longest; %d steps each after the timed region, "
                               "wall clock; the headline `value` is the ragged batch (every utterance alone, no pad frames)" % (nsub, nrep))
        finally:
            enc_.ragged, enc_.trim_sub_batches, enc_.sub_batch_bounds, enc_.sub_batches, enc_.sub_batch_streams = saved
        result["reference_batch_semantics"] = ref_sem

    if rank == 0 and world == 1 and not args.no_cpu_baseline:      # reported at N = 1 only (task contract)
        result["cpu_baseline"] = cpu_baseline(sd, plan)

    if rank == 0:
        print(json.dumps(result))
    if multi:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0 and result.get("check") and not result["check"]["ok"]:
        sys.exit("bench.py: self-check of the benchmarked step FAILED: %s" % json.dumps(result["check"]))


if __name__ == "__main__":
    main()
