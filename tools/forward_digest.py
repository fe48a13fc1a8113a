"""Digest of what the encoder's forward entries compute: one JSON line per case with the SHA-256 of the output, of `out_len`, of the attention maps where
requested and - with a trace arena attached - the ordered list of trace entries (name, rows, cols, ld, dtype, SHA-256 of the bytes).

    python tools/forward_digest.py                    # the whole table
    python tools/forward_digest.py --compact          # the trace list folded into its count and one SHA-256 (the form kept in profiles/)
    python tools/forward_digest.py Tiny               # the cases of one model
    python tools/forward_digest.py --front-end        # only the front-end cases (front_end_cases)
    python tools/forward_digest.py --block-routes     # only the per-block route cases (block_routes_cases)

Checking a change of the host side (csrc/encoder.hip, forward_*.hip): run this on the tree before and on the tree after ON THE SAME GPU and compare the lines; a
forward that enqueues the same kernels with the same arguments in the same order gives the same bytes.  Weights: the recipe of tools/pack_digest.py; inputs:
synth.make_mel / synth.make_audio from a fixed seed.  The batch is the smallest at which every route can still go wrong: 3 utterances of 97 / 64 / 33 mel frames -
97 gives 49 frames after the subsampling, no multiple of the group size 3, so the chunk padding and the `Tp != T` row maps run.  A refused call is a line too
(its error text).  The workspace is filled with a fixed byte pattern before every forward: rows a kernel leaves unwritten are part of the trace.
"""
from __future__ import annotations

import copy
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pack_digest  # noqa: E402
from efficientconformer_amd import _lib, synth  # noqa: E402

MODELS = ["Tiny", "EfficientConformerCTCSmall", "ConformerCTCSmall", "EfficientConformerCTCMedium"]
FRAMES, LENGTHS = 97, [97, 64, 33]
CONTEXT_MODEL = "EfficientConformerCTCSmall"      # the audio, finite-context, causal and E-cache cases
ARENA_BYTES = 1 << 27


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


class Handle:
    """A finalized encoder of `model` packed for `precision`, with its plan; context: overrides of the plan's causal / left_context."""

    def __init__(self, lib, model: str, precision: str, **context):
        self.lib, self.model, self.precision = lib, model, precision
        plan, vocab, sd = pack_digest.state_dict(model)
        plan = copy.copy(plan)
        for k, v in context.items():
            setattr(plan, k, v)
        if context.get("causal"):
            plan.right_context = 0
        self.plan = plan
        self.h = pack_digest.create(lib, plan, vocab, precision, sd)
        _lib.check(lib.effconf_encoder_finalize(self.h), "finalize", lib)

    def option(self, name: str, value: int):
        _lib.check(self.lib.effconf_encoder_set_option(self.h, name.encode(), value), "set_option(%s)" % name, self.lib)

    def close(self):
        self.lib.effconf_encoder_destroy(self.h)


def forward(hd: Handle, *, ragged=False, audio=False, trace=False, maps=False, repeat=1) -> dict:
    """One forward (the last of `repeat` on one workspace) -> the digest fields."""
    lib, h, plan, dev = hd.lib, hd.h, hd.plan, "cuda:0"
    B = len(LENGTHS)
    if audio:
        lens = np.asarray([(t - 1) * plan.hop_length for t in LENGTHS], dtype=np.int64)
        x = torch.from_numpy(synth.make_audio(lens, seed=5)).to(dev)
    else:
        mel, lens = synth.make_mel(B, plan.n_mels, FRAMES, LENGTHS, seed=4321)
        x = torch.from_numpy(mel).to(dev)
    n = x.shape[-1]
    host_len = (C.c_int64 * B)(*[int(v) for v in lens])
    dev_len = torch.from_numpy(lens).to(dev)
    frames = lib.effconf_encoder_out_frames(h, n, int(audio))
    nbytes = lib.effconf_encoder_workspace_bytes_ragged(h, host_len, B, n, int(audio)) if ragged else lib.effconf_encoder_workspace_bytes(h, B, n, int(audio))
    ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
    out = torch.zeros(B, frames, plan.blocks[-1].dim_expand, dtype=torch.float32, device=dev)
    out_len = torch.zeros(B, dtype=torch.int64, device=dev)
    arena, att = None, []
    if trace:
        arena = torch.zeros(ARENA_BYTES, dtype=torch.uint8, device=dev)
        _lib.check(lib.effconf_encoder_set_trace(h, arena.data_ptr(), arena.numel()), "set_trace", lib)
    if maps:
        nb = len(plan.blocks)
        heads, tg = (C.c_int32 * nb)(), (C.c_int32 * nb)()
        _lib.check(lib.effconf_encoder_attention_dims(h, n, int(audio), heads, tg), "attention_dims", lib)
        att = [torch.zeros(B, heads[k], tg[k], tg[k], dtype=torch.float32, device=dev) for k in range(nb)]
        _lib.check(lib.effconf_encoder_set_attention_outputs(h, (C.c_void_p * nb)(*[a.data_ptr() for a in att]), nb), "set_attention_outputs", lib)
    stream = torch.cuda.current_stream().cuda_stream
    res = {}
    try:
        ws.fill_(0xA5)
        for _ in range(repeat):
            if ragged:
                rc = lib.effconf_encoder_forward_ragged(h, x.data_ptr(), dev_len.data_ptr(), host_len, B, n, int(audio), out.data_ptr(), frames, out_len.data_ptr(),
                                                        ws.data_ptr(), ws.numel(), stream)
            else:
                fn = lib.effconf_encoder_forward if audio else lib.effconf_encoder_forward_mel
                rc = fn(h, x.data_ptr(), dev_len.data_ptr(), B, n, out.data_ptr(), out_len.data_ptr(), ws.data_ptr(), ws.numel(), stream)
            if rc != 0:
                return {"error": lib.effconf_last_error().decode()}
        torch.cuda.synchronize()
        res["out"], res["out_len"] = sha(out), sha(out_len)
        if maps:
            res["maps"] = [sha(a) for a in att]
        if trace:
            entries = []
            for i in range(lib.effconf_encoder_trace_count(h)):
                name = C.create_string_buffer(64)
                off, rows, cols, ld, dt = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
                _lib.check(lib.effconf_encoder_trace_entry(h, i, name, C.byref(off), C.byref(rows), C.byref(cols), C.byref(ld), C.byref(dt)), "trace_entry", lib)
                size = rows.value * ld.value * (2 if dt.value == 1 else 4)
                entries.append([name.value.decode(), rows.value, cols.value, ld.value, dt.value, sha(arena[off.value:off.value + size])])
            res["trace"] = entries
        return res
    finally:
        torch.cuda.synchronize()
        if trace:
            lib.effconf_encoder_set_trace(h, None, 0)
        if maps:
            lib.effconf_encoder_set_attention_outputs(h, None, 0)


def model_cases(precision: str):
    """(label, forward arguments, options) of one handle: every layout x trace combination its mode takes."""
    cases = []
    layouts = [False, True] if precision in ("bf16", "split") else [False]
    for ragged in layouts:
        for trace in ("off", "on", "fused") if precision == "split" else ("off", "on"):
            cases.append(("%s trace=%s" % ("ragged" if ragged else "rect", trace), dict(ragged=ragged, trace=trace != "off"), {"trace_fused": int(trace == "fused")} if precision == "split" else {}))
    if precision == "bf16":      # the chain shapes the defaults never take at this batch size; last on the handle, each case sets both options (they persist)
        for label, opts in (("chain_small_m=0", {"chain_small_m": 0, "chain_pair": 5}),      # the 8- and 4-wave shapes on a nearly empty workgroup: the row clamp
                            ("chain_pair=0", {"chain_small_m": 4096, "chain_pair": 0}),         # chain.hip's own KS = 16 instances, kpad at D = 240 among them
                            ("chain_small_m=0 chain_pair=0", {"chain_small_m": 0, "chain_pair": 0})):
            for ragged in (False, True):
                cases.append(("%s %s trace=on" % ("ragged" if ragged else "rect", label), dict(ragged=ragged, trace=True), opts))
    if precision != "bf16":      # attention maps: the scores-in-memory kernels in either label-exact mode
        for trace in ("off", "on"):
            cases.append(("rect maps trace=%s" % trace, dict(maps=True, trace=trace == "on"), {"trace_fused": 0} if precision == "split" else {}))
    return cases


def context_cases():
    """(label, precision, plan overrides, forward arguments, options) on CONTEXT_MODEL."""
    out = []
    for p in pack_digest.PRECISIONS:
        out.append(("audio rect", p, {}, dict(audio=True, trace=True), {}))
        if p != "fp32":
            out.append(("audio ragged", p, {}, dict(audio=True, ragged=True, trace=True), {}))
        out.append(("left_context=12", p, {"left_context": 12}, dict(trace=True), {}))
        out.append(("causal", p, {"causal": True}, dict(trace=True), {}))             # fp32: the refusal
        if p != "fp32":
            out.append(("causal ragged", p, {"causal": True}, dict(ragged=True), {}))
            out.append(("E cache, second forward", p, {}, dict(repeat=2), {"cache_pos_embeddings": 1}))
            out.append(("E cache, second forward, ragged", p, {}, dict(ragged=True, repeat=2), {"cache_pos_embeddings": 1}))
    return out


def front_end_cases():
    """(model, precision, [(label, options)]): every route of the bf16 front-end dispatcher and all four tile counts (1 / 4 / 6 / 12) of both chunked front-end
    kernels (sublinear3.hip, sxf_sub.hip); each case runs rectangular and ragged with a trace (split: trace_fused, so the fused kernel is what runs)."""
    sub = lambda fuse, auto=1: {"fuse_subsample": fuse, "sub3_auto": auto}
    out = [("EfficientConformerCTCSmall", "bf16", [("fuse_subsample=%d" % f, sub(f)) for f in (0, 1, 2, 3)]),
           ("EfficientConformerCTCMedium", "bf16", [("sub3_auto=%d" % a, sub(2, a)) for a in (0, 1)]),
           ("EfficientConformerCTCLarge", "bf16", [("defaults", {})]),
           ("Tiny", "bf16", [("fuse_subsample=3", sub(3))]),
           ("ConformerCTCSmall", "bf16", [("two layers", {})])]
    out += [(m, "split", [("fused front end", {"trace_fused": 1})]) for m in ("Tiny", "EfficientConformerCTCSmall", "EfficientConformerCTCMedium", "EfficientConformerCTCLarge")]
    return out


def block_routes_cases():
    """(model, precision, [(label, options)]): the per-block routes of the bf16 schedule (csrc/routes.h: block_routes, attention_route) the defaults do not take -
    per-module kernels instead of the chains (all of them, the wide stages only, the tail + head pair only), chain.hip instead of chain2.hip / chain3.hip,
    attention.hip and the 4-wave attention2.hip, the VALU depthwise kernel; Medium's D = 360 stage on the row-stationary and on the tiled kernels, and both forced
    tile widths of the tiled GEMMs.  Options persist on a handle, so every case sets the whole set; each runs rectangular and ragged with a trace."""
    small = {"fuse_chain": 1, "chain_pair": 5, "chain_full_max": 192, "chain_max_dim": 256, "attention_v2": 1, "dwconv_mfma": 1}
    medium = {"tiled_auto": 1, "wide_gemm": 0}
    one = lambda base, name, v: ("%s=%d" % (name, v), {**base, name: v})
    return [("EfficientConformerCTCSmall", "bf16", [one(small, *nv) for nv in (("fuse_chain", 0), ("chain_pair", 0), ("chain_full_max", 0), ("chain_max_dim", 128),
                                                                                ("attention_v2", 0), ("attention_v2", 2), ("dwconv_mfma", 0))]),
            ("EfficientConformerCTCMedium", "bf16", [("defaults", medium)] + [one(medium, *nv) for nv in (("tiled_auto", 0), ("tiled_auto", 2), ("wide_gemm", 2), ("wide_gemm", 3))])]


def emit(compact: bool, head: dict, res: dict):
    if compact and "trace" in res:
        t = res.pop("trace")
        res["trace"] = {"entries": len(t), "names": sorted({e[0].split(".")[-1] for e in t}), "sha": hashlib.sha256(json.dumps(t).encode()).hexdigest()}
    print(json.dumps({**head, **res}), flush=True)


def main(argv):
    compact = "--compact" in argv
    only = [a for a in argv if not a.startswith("--")]
    lib = _lib.load()
    for model in MODELS:
        if "--front-end" in argv or "--block-routes" in argv or (only and model not in only):
            continue
        for precision in pack_digest.PRECISIONS:
            hd = Handle(lib, model, precision)
            try:
                for label, kw, opts in model_cases(precision):
                    for k, v in opts.items():
                        hd.option(k, v)
                    emit(compact, {"model": model, "precision": precision, "case": label}, forward(hd, **kw))
            finally:
                hd.close()
    sections = [("front end", front_end_cases())] * ("--block-routes" not in argv) + [("block routes", block_routes_cases())] * ("--front-end" not in argv)
    for section, (model, precision, cases) in [(name, c) for name, cs in sections for c in cs]:
        if only and model not in only:
            continue
        hd = Handle(lib, model, precision)
        try:
            for label, opts in cases:
                for k, v in opts.items():
                    hd.option(k, v)
                for ragged in (False, True):
                    emit(compact, {"model": model, "precision": precision, "case": "%s, %s, %s" % (section, label, "ragged" if ragged else "rect")}, forward(hd, ragged=ragged, trace=True))
        finally:
            hd.close()
    if "--front-end" not in argv and "--block-routes" not in argv and (not only or CONTEXT_MODEL in only):
        for label, precision, ctx, kw, opts in context_cases():
            hd = Handle(lib, CONTEXT_MODEL, precision, **ctx)
            try:
                for k, v in opts.items():
                    hd.option(k, v)
                emit(compact, {"model": CONTEXT_MODEL, "precision": precision, "case": label}, forward(hd, **kw))
            finally:
                hd.close()


if __name__ == "__main__":
    main(sys.argv[1:])
