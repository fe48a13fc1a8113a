"""Dry run of the weight packing on the CPU: one JSON line per case with the digest of everything `effconf_encoder_finalize` would upload.

    python tools/pack_digest.py                       # the parity table: 12 shipped configurations + Tiny, bf16 / fp32 / split, stressed profiles, one refusal
    python tools/pack_digest.py Tiny:split EfficientConformerCTCSmall:bf16:trained

`effconf_debug_pack_digest` (include/effconf_debug.h, libeffconf_debug.so) runs every packing step of csrc/pack.hip on the loaded host tensors and hashes each
buffer where `upload` would copy it to the device; no HIP call is made, so this runs on a machine without a GPU.  Weights: the recipe of
tests/test_gpu_exact_and_sweep.py::_model (CTC head, vocab capped at 256, seed 7), optionally a profile of synth.make_stressed_state_dict.  Checking a packing change:
run this on the tree before and on the tree after ON THE SAME MACHINE (the sinusoid and mel tables go through libm) and compare the lines.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from efficientconformer_amd import _lib, named_config, synth  # noqa: E402
from efficientconformer_amd.config import build_plan  # noqa: E402

SHIPPED = ["ConformerCTCSmall", "ConformerCTCMedium", "ConformerCTCLarge", "ConformerTransducerSmall", "ConformerTransducerMedium",
           "ConformerTransducerLarge", "EfficientConformerCTCSmall", "EfficientConformerCTCMedium", "EfficientConformerCTCLarge",
           "EfficientConformerTransducerSmall", "EfficientConformerTransducerMedium", "EfficientConformerTransducerLarge"]
STRESSED = ["EfficientConformerCTCSmall", "EfficientConformerCTCMedium", "ConformerCTCSmall"]
PRECISIONS = ("bf16", "fp32", "split")
SEED = 7


def state_dict(name: str, profile: str = ""):
    """(plan, vocab, state dict without the `encoder.` prefix + fc.*) of the sweep tests' recipe; profile "refused": one weight beyond the split images' range."""
    cfg = named_config(name)
    plan = build_plan(cfg["encoder_params"])
    vocab = min(256, cfg["tokenizer_params"]["vocab_size"])
    if profile in synth.STRESS_PROFILES:
        sd = synth.make_stressed_state_dict(plan, SEED, profile, vocab)
    else:
        sd = synth.make_state_dict(plan, SEED, vocab)
    if profile == "refused":
        sd["blocks.1.convolution_module.layers.7.weight"][3, 5, 0] = 70000.0
    return plan, vocab, sd


def create(lib, plan, vocab: int, precision: str, sd):
    """A handle with the configuration of `plan`, the precision's packing option and every tensor loaded; not finalized."""
    blocks = (_lib.EcBlock * len(plan.blocks))()
    for i, b in enumerate(plan.blocks):
        blocks[i] = _lib.EcBlock(b.dim_model, b.dim_expand, b.dim_ffn1 // b.dim_model, b.num_heads, b.kernel_size, b.group_size, b.max_pos, b.conv_stride)
    cfg = _lib.EcConfig()
    cfg.n_mels, cfg.sample_rate, cfg.n_fft, cfg.win_length, cfg.hop_length = plan.n_mels, plan.sample_rate, plan.n_fft, plan.win_length, plan.hop_length
    cfg.normalize, cfg.mean, cfg.std, cfg.sub_layers = int(plan.normalize), plan.mean, plan.std, plan.sub_layers
    for i in range(4):
        cfg.sub_filters[i] = plan.sub_filters[i] if i < len(plan.sub_filters) else 0
    cfg.num_blocks, cfg.blocks, cfg.vocab_size = len(plan.blocks), C.cast(blocks, C.POINTER(_lib.EcBlock)), vocab
    cfg.causal, cfg.left_context, cfg.right_context = int(plan.causal), min(plan.left_context, 1 << 30), min(plan.right_context, 1 << 30)
    h = lib.effconf_encoder_create(C.byref(cfg))
    if not h:
        raise _lib.EffconfError("effconf_encoder_create: %s" % lib.effconf_last_error().decode())
    _lib.check(lib.effconf_encoder_set_option(h, b"exact_fp32", PRECISIONS.index(precision)), "set_option(exact_fp32)", lib)
    for key, v in sd.items():
        if key.endswith("num_batches_tracked"):
            continue
        arr = np.ascontiguousarray(v, dtype=np.float32)
        shape = (C.c_int64 * max(arr.ndim, 1))(*arr.shape)
        _lib.check(lib.effconf_encoder_load_tensor(h, key.encode(), arr.ctypes.data_as(C.c_void_p), shape, arr.ndim), "load_tensor(%s)" % key, lib)
    return h


def dry_run(lib, h):
    """(rc, digest, buffers, bytes) of one dry run of the packing on handle h."""
    digest, buffers, nbytes = C.c_uint64(0), C.c_int64(0), C.c_int64(0)
    rc = lib.effconf_debug_pack_digest(h, C.byref(digest), C.byref(buffers), C.byref(nbytes))
    return rc, digest.value, buffers.value, nbytes.value


def run_case(lib, name: str, precision: str, profile: str = "") -> dict:
    plan, vocab, sd = state_dict(name, profile)
    h = create(lib, plan, vocab, precision, sd)
    try:
        t0 = time.perf_counter()
        rc, digest, buffers, nbytes = dry_run(lib, h)
        dt = time.perf_counter() - t0
        out = {"model": name, "precision": precision, "profile": profile or "synthetic", "digest": "%016x" % digest, "buffers": buffers, "bytes": nbytes,
               "seconds": round(dt, 3)}
        if rc != 0:
            out["error"] = lib.effconf_last_error().decode()
        return out
    finally:
        lib.effconf_encoder_destroy(h)


def parity_cases():
    cases = [(n, p, "") for n in ["Tiny"] + SHIPPED for p in PRECISIONS]
    cases += [(n, p, prof) for n in STRESSED for prof in synth.STRESS_PROFILES for p in PRECISIONS]
    return cases + [("EfficientConformerCTCSmall", "split", "refused")]


def main(argv):
    lib = _lib.load_debug()
    cases = [tuple((a.split(":") + ["", ""])[:3]) for a in argv] or parity_cases()
    for name, precision, profile in cases:
        print(json.dumps(run_case(lib, name, precision or "bf16", profile)), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
