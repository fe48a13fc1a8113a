"""Test reference of the self-conditioned CTC encoders (no tests in here): the reference's ``ConformerEncoderInterCTC`` (models/encoders.py:144-215)
composed from oracle/ref_encoder.py's Conformer block plus the three lines of the step, the rounding-aware stage of csrc/interctc.hip built on
oracle/ref_bf16.py's ``q``, and the two weight recipes of the goldens.

The step after a listed block k, on the block's output rows x (.., De):

    z = linear_expand_k(x);  p = softmax(z);  x' = x + linear_proj_k(p)

The kernel's contract (``interctc_stage``): z = q(x) q(We)^T + be with an fp32 accumulator, p = softmax(z) in fp32, x' = x + P~ q(Wp)^T + bp with
P~ the probabilities as bf16 operands.  The kernel rounds exp(z - m) against its RUNNING maximum and divides by the row sum after the product, which
cannot be reproduced exactly: as with ``round_p`` in oracle/ref_bf16.py the float64 reference leaves p un-rounded and the rounding belongs to the
noise model only."""
from __future__ import annotations

import os
import sys
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from efficientconformer_amd import synth  # noqa: E402
from efficientconformer_amd.config import build_plan, named_config  # noqa: E402
from oracle import ref_bf16 as RB  # noqa: E402
from oracle import ref_encoder as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TINY_BLOCKS = [1, 3, 5]          # both transition blocks and the last block of Tiny
TINY_VOCAB = 32
WEIGHT_SEED = 7
BATCHES = ((47, [47, 40, 23]), (100, [100, 77, 52]))      # the two batches of tests/golden/tiny_T*.npz
RECIPES = ("flat", "peaky")
PEAKY_SCALE, PEAKY_BIAS = 8.0, 6.0


def peaky(sd: Dict[str, np.ndarray], blocks, prefix: str = "") -> Dict[str, np.ndarray]:
    """The peaky recipe: linear_expand_k.weight x 8 and linear_expand_k.bias[0] += 6 for every listed block (a copy).  On Tiny the probabilities then
    reach p.max() = 1.0 and p.min() ~ 1e-20: what a trained model's confident frames look like, and what the max subtraction and the online rescale of
    the kernel have to survive."""
    out = {k: np.array(v, copy=True) for k, v in sd.items()}
    for k in blocks:
        out[prefix + "linear_expand_%d.weight" % k] = (out[prefix + "linear_expand_%d.weight" % k] * np.float32(PEAKY_SCALE)).astype(np.float32)
        out[prefix + "linear_expand_%d.bias" % k][0] += np.float32(PEAKY_BIAS)
    return out


def tiny_params(blocks=None, vocab: int = TINY_VOCAB) -> dict:
    """encoder_params of the Tiny InterCTC encoder of the goldens."""
    return dict(named_config("Tiny")["encoder_params"], interctc_blocks=list(TINY_BLOCKS if blocks is None else blocks), vocab_size=vocab)


def tiny_state_dict(recipe: str, prefix: str = "") -> Dict[str, np.ndarray]:
    """Key-seeded weights (seed 7) of the Tiny InterCTC encoder + its ``fc`` head, in the given recipe."""
    plan = build_plan(tiny_params(), interctc=True)
    sd = synth.make_state_dict(plan, WEIGHT_SEED, TINY_VOCAB, prefix=prefix)
    return peaky(sd, TINY_BLOCKS, prefix) if recipe == "peaky" else sd


def tiny_mel(tm: int, lens):
    return synth.make_mel(len(lens), 80, tm, lens, seed=4321 + tm)


def load_golden(recipe: str, tm: int):
    return np.load(os.path.join(GOLDEN, "interctc_tiny_%s_T%d.npz" % (recipe, tm)))


def _w(sd, key, dtype):
    v = sd[key]
    return (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).to(dtype)


def step(x: torch.Tensor, sd, k: int):
    """The three lines of the reference in x's dtype -> (x', p)."""
    p = F.linear(x, _w(sd, "linear_expand_%d.weight" % k, x.dtype), _w(sd, "linear_expand_%d.bias" % k, x.dtype)).softmax(dim=-1)
    return x + F.linear(p, _w(sd, "linear_proj_%d.weight" % k, x.dtype), _w(sd, "linear_proj_%d.bias" % k, x.dtype)), p


def encoder_from_mel(mel: torch.Tensor, mel_len: Optional[torch.Tensor], sd, plan, dtype: torch.dtype = torch.float32, trace: Optional[dict] = None):
    """The composed oracle: oracle.ref_encoder.encoder_from_mel's loop with the step after every block of plan.interctc_blocks
    -> (x (B, T_out, D_last), out_len, [p_k (B, T_k, V)]).  ``trace`` also receives blocks.k.x_interctc / blocks.k.interctc_p."""
    if dtype != torch.float32:
        sd = R.cast_state_dict(sd, dtype)
        mel = mel.to(dtype)
    x, lens = R.subsample(mel, mel_len, sd, plan.sub_layers)
    x = F.linear(x.transpose(1, 2), R._t(sd, "linear.weight"), R._t(sd, "linear.bias"))
    probs: List[torch.Tensor] = []
    for bp in plan.blocks:
        x = R.conformer_block(x, lens, sd, bp, trace, plan)
        if bp.conv_stride > 1 and lens is not None:
            lens = torch.div(lens - 1, bp.conv_stride, rounding_mode="floor") + 1
        if bp.index in plan.interctc_blocks:
            x, p = step(x, sd, bp.index)
            probs.append(p)
            if trace is not None:
                trace["blocks.%d.x_interctc" % bp.index], trace["blocks.%d.interctc_p" % bp.index] = x, p
    return x, lens, probs


def interctc_stage(x: torch.Tensor, sd, k: int, dtype, round_p: bool, *, order=None, round_exp: bool = False, drop_bp: bool = False,
                   round_logits: bool = False):
    """The rounding-aware stage of csrc/interctc.hip in ``dtype`` arithmetic from the fp32 rows x (.., De) -> (x', p).
    round_p: the second product's operand is q(p) (noise model) instead of p (the float64 reference).
    Variants (what tests/test_interctc_host.py feeds the stage checker with): ``order`` - a permutation pair (of De, of V) applied to the K axis of the two
    products (another summation order of the same sums); ``round_exp`` - q(exp(z - max)) is the operand and the division by the row sum follows the
    product (the kernel's order); ``drop_bp`` - a kernel that forgets linear_proj's bias; ``round_logits`` - one that rounds the logits to bf16."""
    x = x.to(dtype)
    we, be = RB.q(_w(sd, "linear_expand_%d.weight" % k, dtype)), _w(sd, "linear_expand_%d.bias" % k, dtype)
    wp, bp = RB.q(_w(sd, "linear_proj_%d.weight" % k, dtype)), _w(sd, "linear_proj_%d.bias" % k, dtype)
    a = RB.q(x)
    if order is not None:
        z = a[..., order[0]] @ we[:, order[0]].T + be
    else:
        z = a @ we.T + be
    if round_logits:
        z = RB.q(z)
    e = torch.exp(z - z.max(dim=-1, keepdim=True).values)
    s = e.sum(dim=-1, keepdim=True)
    p = e / s
    if round_exp:
        op, post = (RB.q(e) if round_p else e), s
    else:
        op, post = (RB.q(p) if round_p else p), None
    prod = op[..., order[1]] @ wp[:, order[1]].T if order is not None else op @ wp.T
    if post is not None:
        prod = prod / post
    y = x + prod if drop_bp else x + prod + bp
    return y, p


def stage_refs(x: torch.Tensor, sd, k: int):
    """(r64, [r32 noise runs]) of the stage as tests hold a kernel to it with oracle.ref_bf16.stage_ratios: r64 = the float64 stage with p un-rounded;
    the noise runs = float32 with q(p), in the natural and in the reversed summation order.  Each entry is the pair (x', p)."""
    de, v = int(x.shape[-1]), int(np.asarray(sd["linear_expand_%d.bias" % k]).shape[0])
    rev = (torch.arange(de - 1, -1, -1), torch.arange(v - 1, -1, -1))
    r64 = interctc_stage(x, sd, k, torch.float64, False)
    r32 = [interctc_stage(x, sd, k, torch.float32, True), interctc_stage(x, sd, k, torch.float32, True, order=rev)]
    return r64, r32


def stage_weights(de: int, v: int, k: int, seed: int, recipe: str) -> Dict[str, np.ndarray]:
    """Key-seeded weights of ONE step of width (de, v) in the given recipe (for kernel-alone tests and the stage checker's self-test)."""
    sd = {}
    for name, shape, kind in (("linear_expand_%d.weight" % k, (v, de), "weight"), ("linear_expand_%d.bias" % k, (v,), "bias"),
                              ("linear_proj_%d.weight" % k, (de, v), "weight"), ("linear_proj_%d.bias" % k, (de,), "bias")):
        sd[name] = synth.make_tensor("%dx%d.%s" % (de, v, name), shape, kind, seed)
    return peaky(sd, [k]) if recipe == "peaky" else sd
