"""ORACLE — test infrastructure only: the bf16 path's arithmetic contract, stage by stage, in plain torch on the CPU.

The statement of record of WHERE the bf16 path (efficientconformer_amd/csrc: chain.hip, chain2.hip, chain3.hip, rsgemm.hip, gemm.hip,
attention2.hip, attention.hip, conv.hip, conv2.hip, sublinear.hip, sublinear2.hip, sublinear3.hip) rounds to bf16.  Every function is one stage between two points of the debug trace
(ConformerEncoder.trace_forward_mel), takes that stage's INPUT tensor(s), the float32 reference state dict (keys without ``encoder.``),
the BlockPlan and ``dtype``, and evaluates the stage in ``dtype`` arithmetic with the one rounding helper ``q`` applied at exactly the
kernels' rounding points.  ``dtype = torch.float64`` is the reference; ``dtype = torch.float32`` is the noise model (what a correct
kernel may differ by: float32 summation order and the bf16 ties it flips).  ``rnd = ident`` switches every rounding off: the stages chained
are then oracle/ref_encoder.py in other words (tests/test_ref_bf16_host.py).  No library call and none of the C++ packers are used.

Conventions
* Stages whose output the kernels store as bf16 (qkv, pos_e, attention, glu, depthwise) return the value BEFORE that last rounding; the
  stored number is ``q`` of it.  Their bf16 inputs are taken as they are (already bf16 numbers in the trace).
* ``folded``: how the LayerNorm in front of a Linear is applied.
  True  (fused chains): weight q(float32(W * gamma)) - product in float32, then rounded - bias b + float32(sum_k W[n][k] beta[k]) with the sum
        in double, operand q((x - mean) * rstd) without gamma / beta.  pack.hip pack_linear ("W diag(gamma), b + W beta (fp32, before the
        bf16 rounding)", the bf16_rn(rows[n][src] * ln_g[src]) line and the double accumulator below it); chain.hip ln_stats (two-pass, eps
        1e-6, pad-column correction of the variance) and norm_frags (pack_bf2(fmaf(x, rstd, -mean * rstd))).
  False (per-module kernels: norm.hip launch_layernorm, the prologue LayerNorm of rsgemm.hip): operand q(LN(x) * gamma + beta), weight q(W).
* FFN: hidden q(swish(.)) (chain.hip ffn_stage: pack_bf2(swishf_(h[r]), ...)), second weight q(W2 / 2) and bias b2 / 2 (pack.hip
  pack_ffn2_permuted(..., 0.5f) and the ``hb`` vectors next to it; the per-module kernel multiplies by alpha = 0.5 after the product, which is
  the same number), accumulated onto the float32 residual row.  Block-final LayerNorm: float32, affine, not rounded (gamma / beta in the chains'
  constant block, chain.hip ln_inplace).
* Chain B: x += att_o . q(Wo)^T + bo, then glu = q(a * sigmoid(b)) of the pointwise-1 product on the (folded) conv-module LayerNorm (chain.hip:
  "a * sigmoid(b) for channels ..." / pack_bf2(o[0], o[1])).
* Depthwise convolution: BatchNorm folded into taps and bias in float32 (pack.hip bn_fold, conv_bn_fold and the "[k][De] fp32" table), bf16 input, output
  q(swish(.)).  conv_res of transition blocks: q(x[::s]) (norm.hip launch_cast_rows) times q(W), float32 out.
* Q / K / V: qu = q(Q + b + u), k = q(K + b), v = q(V + b) (chain.hip: pack_bf2(acc + ua.x, ...) with the bias as the accumulator's initial value;
  gemm.hip EPI_QKV_NAT: "if (which == 0) add += p.u[nc]"); chunk-padding rows qu = q(u), k = v = 0 (attention.hip attn_pad_rows_nat_kernel /
  attn_pad_rows_ragged_kernel).  In the attention kernel qv = q(float(qu) + float32(v - u)) - a second rounding (attention2.hip, the
  pack_bf2(... + da.x ...) lines; the table v - u is built in float32 in pack.hip, dvu_table -> ``W.dvu``).  E = q(q(sinusoid rows) . q(Wpos)^T + bpos)
  (pack.hip build_pos_table: bf16_rn(std::sin(a)); launch_gemm(pe, EPI_BF16)).  Scores, softmax and P V are not rounded here; ``round_p``
  rounds exp(s - rowmax) to bf16 before P V - the kernel rounds P against its RUNNING maximum, which cannot be reproduced exactly, so
  ``round_p`` belongs to the noise model only.
* Front end (conv.hip + gemm.hip, sublinear.hip, sublinear2.hip, sublinear3.hip, conv2.hip + gemm.hip), one contract for all five routes:
  - Layer 1: BatchNorm2d folded into the nine taps and the bias in float32 - scale = gamma / sqrt(var + 1e-5f), shift = beta - mean * scale (pack.hip
    bn_fold), tap = w * scale, bias = b * scale + shift (pack.hip conv_bn_fold: ``(double)w[...] * sc[ch]``, exact, rounded once to float32 /
    ``b[ch] * sc[ch] + sh[ch]``) - float32 mel, float32 accumulation, Swish, then ONE rounding to bf16: conv.hip
    subsample_conv_kernel ``pack_bf2(swishf_(acc[0][tl]), swishf_(acc[1][tl]))``, sublinear.hip ``pa[i] = make_uint4(pack_bf2(r[0], r[1]), ...)``,
    sublinear2.hip ``y[e] = swishf_(cv[8 * j + e])`` / ``xf[2 * g + j] = ... pack_bf2(y[0], y[1])``, sublinear3.hip ``q.hh[pr] = pack_bf2(q.x[2 * pr], ...)``,
    conv2.hip subsample_conv_cl_kernel ``pack_bf2(r0, r1)``.  Nothing else is rounded: taps, bias and mel stay float32 numbers.
  - ``conv="split"`` (sublinear2.hip, sublinear3.hip: the convolution on the matrix pipe): both operands as hi + lo with hi = the float32 number with
    its low 16 bits cleared (sublinear2.hip split_hi, sublinear3.hip hi_bits, pack.h bf16_pair_trunc ``u >> 16``) and lo = q(x - hi)
    (``pack_bf2(v[2 * e] - __uint_as_float(h0), ...)``, bf16_pair_trunc ``bf16_rn(f - bf16_value(*hi))``), the sum W_hi P_hi + W_hi P_lo + W_lo P_hi - the lo lo term, 2^-14 of a
    product at most, is dropped - and the folded bias as tap slot 9 against a patch entry of 1.0 (pack.hip ``(*tab)[(size_t)ch * 16 + 9] = tbias[ch]`` /
    ``tap_enc(tbias[ch], at + 9, ...)``, sublinear2.hip ``tp[1] = 1.0f``).  An evaluation of the same contract to ~2^-14 of sum |w| |p|: it belongs to the noise
    model only, the float64 reference is the exact convolution.
  - Time padding: zeros in front of frame 0 and behind the utterance's own last mel frame where lengths are given (ragged batches: conv.hip
    ``tmb = rag_tm ? rag_tm[b] : Tm``, sublinear3.hip ``Tv = p.mel_len ? p.mel_len[b] : p.Tm``, conv2.hip ``Tmb``); a rectangular batch reads the rectangle as it
    is, pad frames included.  Frequency padding: zero rows at -1 and n_mels.
  - Layer 2 of the two-layer subsampler (conv2.hip conv2_igemm_kernel) from the stored bf16 layer-1 image, which a ragged batch zero-fills behind every
    utterance's own (len - 1) / 2 + 1 frames (subsample_conv_cl_kernel ``t < T1b ? swishf_(a.x) : 0.f``): weight q(float32(w2 * scale2)) (pack.hip
    conv_bn_fold + sub2_conv_image ``bf16_rn((float)wf[...])``), float32 bias b2 * scale2 + shift2 added after the sum, Swish, bf16 store (``f2bf(swishf_(acc[mi][ni][r] + bz))``).
  - Linear: act . q(W)^T + b with a float32 bias, float32 out (pack.hip pack_linear, sublinear_image, sublinear2_images and front_chunks: bf16_rn(lw[...])).
    The K orders of those images ((fc * Cp + c) * 8 + e; permuted per 16; accumulator order of 32-channel chunks; (f2, c)) are the packers' business:
    ``front_linear`` contracts in the reference's feature order c * F' + f (modules.py:247) and nothing else, which is what makes a wrong permutation visible.
  The trace holds ``subsample`` (the last layer's bf16 activation) where separate kernels write it - fuse_subsample = 0, front ends without a fused
  kernel, ragged batches off the matrix-pipe routes, the two-layer subsampler (whose layer-1 image is ``subsample1``) - and nothing between mel and
  ``linear`` on the fused routes, where the activation only exists in registers.

Masking, the relative-to-absolute gather, the streaming band and the sinusoid rows are oracle/ref_encoder.py's own code (relpos_scores,
rel_sinusoid_rows, rel_sinusoid_rows_causal): this module adds roundings, nothing else.

Two hooks serve the split mode's noise model (oracle/ref_split.py) and change nothing unless set: every matrix product of a stage goes through ``_mm``
(``product_like``: another evaluation of a . w^T, e. g. fp16 operand pairs) and front_conv(conv="split") takes its operand splitters from ``_SPLIT_OPS``.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import ref_encoder as R


def q(x: torch.Tensor) -> torch.Tensor:
    """bf16 round-to-nearest-even of the value, kept in x's dtype."""
    return x.float().to(torch.bfloat16).to(x.dtype)


def ident(x: torch.Tensor) -> torch.Tensor:
    """``rnd = ident``: no rounding anywhere (and no float32 detour in the folds): the un-rounded oracle."""
    return x


def _w(sd, key, dtype) -> torch.Tensor:
    v = sd[key]
    v = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))
    return v.to(dtype)


_HW = None      # None: torch's own functions.  An int s: float32 runs use the kernels' float32 formulas with s ulps on the hardware functions


class hardware_like:
    """``with hardware_like(s):`` the float32-arithmetic runs inside evaluate LayerNorm and sigmoid by the KERNELS' float32 formulas instead of
    torch's - chain.hip ln_stats / norm_frags: mean = sum / D, rstd = rsqrt(sum((x - mean)^2) / D + eps), operand x * rstd + (-mean * rstd);
    common.h sigmoidf_: rcp(1 + exp2(-1.44269504 x)) - with the results of the hardware's rsqrt and rcp(1 + exp2) moved by s float32 ulps
    (v_rsq_f32, v_rcp_f32 and v_exp_f32 are good to about one ulp each; see f32_runs for the range of s).  These are legitimate float32 evaluations of the
    same contract that torch's float32 functions do not cover; the parity tests take the noise of a stage over torch's float32 run AND these.
    float64 runs are not affected (the formulas are the same mathematics)."""

    def __init__(self, ulps: int):
        self.ulps = int(ulps)

    def __enter__(self):
        global _HW
        self.prev, _HW = _HW, self.ulps

    def __exit__(self, *a):
        global _HW
        _HW = self.prev


_MM = None      # None: the plain product.  A function (a, w, kind) -> a . w^T: another evaluation of the same product (oracle/ref_split.py, noise models only)


class product_like:
    """``with product_like(fn):`` every matrix product of the stages below is evaluated by fn(a, w, kind) - a (..., K), w (N, K), ``kind`` the name of the
    product ("ffn1", "ffn2", "qkv", "pw1", "pos", "out", "res", "pw2", "linear") - instead of a @ w.T.  oracle/ref_split.py: the split mode's operand pairs."""

    def __init__(self, fn):
        self.fn = fn

    def __enter__(self):
        global _MM
        self.prev, _MM = _MM, self.fn

    def __exit__(self, *a):
        global _MM
        _MM = self.prev


def _mm(a: torch.Tensor, w: torch.Tensor, kind: str) -> torch.Tensor:
    return a @ w.T if _MM is None else _MM(a, w, kind)


def _exp(x: torch.Tensor) -> torch.Tensor:
    """exp of the softmax; under hardware_like(s) in float32: sx_common.h sx_expf (two-part x log2(e), exp2, first-order correction) moved by s ulps."""
    if _HW is not None and x.dtype == torch.float32:
        l2e, l2e_lo = 1.44269502162933349609375, 1.925963033500011e-08
        t = x * l2e
        c = (x.double() * l2e - t.double()).float() + x * l2e_lo          # fmaf(x, L2E, -t): the exact residual of the rounded product
        e = torch.exp2(t) * (1.0 + _HW * 2.0 ** -23)
        return e * (c * 0.693147180559945) + e
    return torch.exp(x)


def ln_plain(x: torch.Tensor) -> torch.Tensor:
    """(x - mean) * rstd, two-pass statistics, eps 1e-6 (chain.hip ln_stats)."""
    if _HW is not None and x.dtype == torch.float32:
        d = x.shape[-1]
        mean = x.sum(-1, keepdim=True) / d
        rstd = torch.rsqrt(((x - mean) ** 2).sum(-1, keepdim=True).clamp_min(0.0) / d + R.LN_EPS) * (1.0 + _HW * 2.0 ** -23)
        return x * rstd + (-mean * rstd)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) * torch.rsqrt(var + R.LN_EPS)


def sigmoid(x: torch.Tensor) -> torch.Tensor:
    if _HW is not None and x.dtype == torch.float32:
        return (1.0 / (1.0 + torch.exp2(-1.44269504088896 * x))) * (1.0 + _HW * 2.0 ** -23)
    return torch.sigmoid(x)


def ln_linear(x: torch.Tensor, sd, wkey: str, bkey: str, ln: str, dtype, folded: bool, rnd: Callable = q, conv1x1: bool = False, kind: str = "") -> torch.Tensor:
    """Linear(LayerNorm(x)) with the LayerNorm ``ln`` (.weight / .bias) folded into the weight (``folded``) or applied to the operand."""
    x = x.to(dtype)
    wsel = (lambda t: t[:, :, 0]) if conv1x1 else (lambda t: t)
    if rnd is ident:
        a = ln_plain(x) * _w(sd, ln + ".weight", dtype) + _w(sd, ln + ".bias", dtype)
        return _mm(a, wsel(_w(sd, wkey, dtype)), kind) + _w(sd, bkey, dtype)
    w32, b32 = wsel(_w(sd, wkey, torch.float32)), _w(sd, bkey, torch.float32)
    g32, be32 = _w(sd, ln + ".weight", torch.float32), _w(sd, ln + ".bias", torch.float32)
    if folded:
        w = rnd((w32 * g32[None, :]).to(dtype))
        b = (b32 + (w32.double() @ be32.double()).float()).to(dtype)
        a = rnd(ln_plain(x))
    else:
        w = rnd(w32.to(dtype))
        b = b32.to(dtype)
        a = rnd(ln_plain(x) * g32.to(dtype) + be32.to(dtype))
    return _mm(a, w, kind) + b


def swish(h):
    return h * sigmoid(h)


def ffn(x: torch.Tensor, sd, prefix: str, dtype, folded: bool, rnd: Callable = q, fault: Optional[Callable] = None) -> torch.Tensor:
    """x + 1/2 FFN(x) on float32 residual rows (..., D).  ``fault`` (tests only): a hook (name, value) -> replacement or None, called with
    "hidden" (swish(h) before its rounding -> the rounded hidden) and "product" ((hidden, q(W2 / 2), W2) -> hidden . W2^T)."""
    x = x.to(dtype)
    h = ln_linear(x, sd, prefix + ".layers.1.weight", prefix + ".layers.1.bias", prefix + ".layers.0", dtype, folded, rnd, kind="ffn1")
    h = swish(h)
    hq = fault("hidden", h) if fault else None
    h = rnd(h) if hq is None else hq
    w2raw = _w(sd, prefix + ".layers.4.weight", dtype)
    w2 = rnd(0.5 * w2raw)
    prod = fault("product", (h, w2, w2raw)) if fault else None
    if prod is None:
        prod = _mm(h, w2, "ffn2")
    return x + prod + 0.5 * _w(sd, prefix + ".layers.4.bias", dtype)


# ------------------------------------------------------------------ front end: Conv2dSubsampling + Linear
def bn_fold2d(sd, layer: int, ft, eps: float = R.BN_EPS) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(weight, scale, folded bias) of subsampling layer ``layer`` in ``ft`` arithmetic (the kernels: float32): scale = gamma / sqrt(var + eps),
    bias = b * scale + (beta - mean * scale).  ``eps`` other than BN_EPS: tests only."""
    p = "subsampling_module.layers.%d" % layer
    sc = _w(sd, p + ".1.weight", ft) / torch.sqrt(_w(sd, p + ".1.running_var", ft) + eps)
    sh = _w(sd, p + ".1.bias", ft) - _w(sd, p + ".1.running_mean", ft) * sc
    return _w(sd, p + ".0.weight", ft), sc, _w(sd, p + ".0.bias", ft) * sc + sh


def split_hi_lo(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The matrix-pipe front ends' operand split of float32 numbers: hi = x with its low 16 bits cleared, lo = q(x - hi)."""
    x = x.float().contiguous()
    hi = (x.view(torch.int32) & -65536).view(torch.float32)
    return hi, q(x - hi)


_SPLIT_OPS = None      # None: split_hi_lo for both operands of front_conv(conv="split").  (weight splitter, patch splitter): oracle/ref_split.py's fp16 pairs


def mask_time(x: torch.Tensor, lens: Optional[torch.Tensor]) -> torch.Tensor:
    """x (..., T) with zeros behind every utterance's own ``lens[b]`` frames (None: as it is)."""
    if lens is None:
        return x
    keep = torch.arange(x.shape[-1])[None, :] < torch.as_tensor(lens).reshape(-1, 1)
    return x * keep.reshape([x.shape[0]] + [1] * (x.dim() - 2) + [x.shape[-1]]).to(x.dtype)


def front_conv(mel: torch.Tensor, mel_len: Optional[torch.Tensor], sd, plan, dtype, rnd: Callable = q, conv: str = "fp32") -> torch.Tensor:
    """mel (B, n_mels, Tm) -> layer 1 of the subsampler (B, C, n_mels / 2, (Tm - 1) / 2 + 1) before its bf16 store: the 3 x 3 stride-2 pad-1 convolution
    with the BatchNorm folded in float32, Swish.  ``mel_len``: the time-side zero padding starts behind each utterance's own frames (frames behind
    (len - 1) / 2 + 1 of the result are then the convolution of zeros: callers take the utterance's own).  ``conv="split"``: the matrix-pipe formula
    (module docstring), float32 operands - noise model only."""
    x = mask_time(mel.to(dtype), mel_len).unsqueeze(1)
    if rnd is ident:
        p = "subsampling_module.layers.0"
        h = F.conv2d(x, _w(sd, p + ".0.weight", dtype), _w(sd, p + ".0.bias", dtype), stride=2, padding=1)
        h = F.batch_norm(h, _w(sd, p + ".1.running_mean", dtype), _w(sd, p + ".1.running_var", dtype), _w(sd, p + ".1.weight", dtype),
                         _w(sd, p + ".1.bias", dtype), False, 0.0, R.BN_EPS)
        return swish(h)
    w, sc, bias = bn_fold2d(sd, 0, torch.float32)
    w9 = w * sc[:, None, None, None]
    if conv == "fp32":
        return swish(F.conv2d(x, w9.to(dtype), bias.to(dtype), stride=2, padding=1))
    assert conv == "split", conv
    bsz, _, f, t = x.shape
    pt = F.unfold(x.float(), 3, padding=1, stride=2)                                         # (B, 9, F1 * T1)
    pt = torch.cat([pt, torch.ones_like(pt[:, :1])], 1)                                      # slot 9: the bias's 1.0
    wt = torch.cat([w9.reshape(-1, 9), bias[:, None]], 1)                                    # (C, 10)
    wsplit, psplit = _SPLIT_OPS or (split_hi_lo, split_hi_lo)
    (whi, wlo), (phi, plo) = wsplit(wt), psplit(pt)
    mm = lambda a, b: torch.einsum("cj,bjl->bcl", a.to(dtype), b.to(dtype))
    h = mm(whi, phi) + mm(whi, plo) + mm(wlo, phi)
    return swish(h.reshape(bsz, -1, (f - 1) // 2 + 1, (t - 1) // 2 + 1))


def front_conv2(act1: torch.Tensor, sd, plan, dtype, rnd: Callable = q) -> torch.Tensor:
    """act1 (B, C, F1, T1): the STORED bf16 layer-1 image (zero behind an utterance's own frames in ragged batches) -> layer 2 of the two-layer
    subsampler (B, C1, F1 / 2, (T1 - 1) / 2 + 1) before its bf16 store: weight q(float32(w2 * scale2)), float32 bias, zero rows outside the image, Swish."""
    x = act1.to(dtype)
    if rnd is ident:
        p = "subsampling_module.layers.1"
        h = F.conv2d(x, _w(sd, p + ".0.weight", dtype), _w(sd, p + ".0.bias", dtype), stride=2, padding=1)
        h = F.batch_norm(h, _w(sd, p + ".1.running_mean", dtype), _w(sd, p + ".1.running_var", dtype), _w(sd, p + ".1.weight", dtype),
                         _w(sd, p + ".1.bias", dtype), False, 0.0, R.BN_EPS)
        return swish(h)
    w, sc, bias = bn_fold2d(sd, 1, torch.float32)
    return swish(F.conv2d(x, rnd((w * sc[:, None, None, None]).to(dtype)), bias.to(dtype), stride=2, padding=1))


def feature_rows(act: torch.Tensor) -> torch.Tensor:
    """(B, C, F', T) -> (B, T, C * F') in the reference's feature order c * F' + f (modules.py:247, encoders.py:113)."""
    b, c, f, t = act.shape
    return act.reshape(b, c * f, t).transpose(1, 2)


def front_linear(act: torch.Tensor, sd, plan, dtype, rnd: Callable = q) -> torch.Tensor:
    """act (..., K): the STORED bf16 subsampler output in the reference's feature order -> act . q(W)^T + b, float32 rows (..., D0)."""
    return _mm(act.to(dtype), rnd(_w(sd, "linear.weight", dtype)), "linear") + _w(sd, "linear.bias", dtype)


def front_end(mel: torch.Tensor, mel_len: Optional[torch.Tensor], sd, plan, dtype, rnd: Callable = q, conv: str = "fp32",
              trace: Optional[dict] = None) -> torch.Tensor:
    """mel (B, n_mels, Tm) -> the trace entry ``linear`` (B, T1, D0): the stages above chained, every bf16-stored intermediate rounded.  ``mel_len``
    (ragged batches): padding at the utterance's own length; rows behind an utterance's own frames are not part of the contract.  ``trace`` receives
    ``subsample`` (B, T1, K), the stored activation in the reference's feature order."""
    a = rnd(front_conv(mel, mel_len, sd, plan, dtype, rnd, conv))
    if plan.sub_layers == 2:
        if mel_len is not None:
            a = mask_time(a, torch.div(torch.as_tensor(mel_len) - 1, 2, rounding_mode="floor") + 1)
        a = rnd(front_conv2(a, sd, plan, dtype, rnd))
    a = feature_rows(a)
    if trace is not None:
        trace["subsample"] = a
    return front_linear(a, sd, plan, dtype, rnd)


# ------------------------------------------------------------------ attention side
def qkv(x_ffn1: torch.Tensor, sd, bp, dtype, folded: bool, rnd: Callable = q) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """x_ffn1 (..., D) float32 rows -> (Q + b + u, K + b, V + b) before the bf16 store."""
    pm = "blocks.%d.multi_head_self_attention_module" % bp.index
    out = []
    for nm in ("query_layer", "key_layer", "value_layer"):
        out.append(ln_linear(x_ffn1, sd, pm + ".mhsa." + nm + ".weight", pm + ".mhsa." + nm + ".bias", pm + ".norm", dtype, folded, rnd, kind="qkv"))
    return out[0] + _w(sd, pm + ".mhsa.u", dtype), out[1], out[2]


def pad_rows(qu: torch.Tensor, k: torch.Tensor, v: torch.Tensor, sd, bp, rnd: Callable = q):
    """(B, T, D) STORED q / k / v -> (B, Tp, D) with the chunk-padding rows of the contract: qu = q(u), k = v = 0."""
    t = qu.shape[1]
    tp = (t + bp.group_size - 1) // bp.group_size * bp.group_size
    if tp == t:
        return qu, k, v
    u = rnd(_w(sd, "blocks.%d.multi_head_self_attention_module.mhsa.u" % bp.index, qu.dtype))
    return (torch.cat([qu, u.expand(qu.shape[0], tp - t, -1)], 1), F.pad(k, (0, 0, 0, tp - t)), F.pad(v, (0, 0, 0, tp - t)))


def pos_rows(tp: int, bp, dtype, causal: bool = False, rnd: Callable = q, shift: int = 0) -> torch.Tensor:
    """The sinusoid rows the positional projection reads: ref_encoder's rows in ``dtype`` arithmetic, rounded.  The kernels' table is built in
    float32 (pack.hip build_pos_table): an angle of up to ~1000 rad carries 6e-5 of float32 error, which moves a few of the rounded sines to
    the neighbouring bf16 number - a difference the float32 run of this function has too, so the noise model contains it.
    ``shift`` (tests only): the fault "positional rows shifted by one"."""
    ft = dtype
    if shift:
        big = R.rel_sinusoid_rows_causal(tp + shift, bp.dim_model, ft) if causal else R.rel_sinusoid_rows(tp + shift, bp.dim_model, bp.group_size, ft)
        n = tp if causal else 2 * tp - bp.group_size
        return rnd(big[:n].to(dtype))
    rows = R.rel_sinusoid_rows_causal(tp, bp.dim_model, ft) if causal else R.rel_sinusoid_rows(tp, bp.dim_model, bp.group_size, ft)
    return rnd(rows.to(dtype))


def pos_e(tp: int, sd, bp, dtype, causal: bool = False, rnd: Callable = q, shift: int = 0) -> torch.Tensor:
    """E before its bf16 store: q(rows) . q(Wpos)^T + bpos, (2Tp - G, D); causal (Tp, D)."""
    m = "blocks.%d.multi_head_self_attention_module.mhsa.pos_layer" % bp.index
    return _mm(pos_rows(tp, bp, dtype, causal, rnd, shift), rnd(_w(sd, m + ".weight", dtype)), "pos") + _w(sd, m + ".bias", dtype)


def attention(qu: torch.Tensor, k: torch.Tensor, v: torch.Tensor, e: torch.Tensor, lens: Optional[torch.Tensor], t: int, sd, bp, dtype,
              rnd: Callable = q, round_p: bool = False, plan=None, exact_qv: bool = False, key_shift: int = 0):
    """qu, k, v (B, Tp, D) and e (2Tp - G | Tp, D): the STORED bf16 operands, chunk-padding rows included; t frames before the padding;
    lens valid frames per utterance (None: all t).  Returns (o, env) (B, t, D): the attention output before its bf16 store and the
    envelope sum_j p_ij |v_j| of every output element.  ``plan``: an EncoderPlan with causal / streaming contexts (as ref_encoder.conformer_block).
    Tests only: ``exact_qv`` builds qv without its rounding, ``key_shift`` moves the key mask by that many groups."""
    pm = "blocks.%d.multi_head_self_attention_module.mhsa." % bp.index
    if rnd is ident:
        dvu = _w(sd, pm + "v", dtype) - _w(sd, pm + "u", dtype)
    else:
        dvu = _w(sd, pm + "v", torch.float32) - _w(sd, pm + "u", torch.float32)
    ctx = {}
    if plan is not None and (plan.causal or plan.left_context < (1 << 30) or plan.right_context < (1 << 30)):
        ctx = dict(causal=plan.causal, left=plan.left_context, right=plan.right_context, mask_stride=bp.mask_stride)
    return attention_operands(qu, k, v, e, dvu, lens, t, bp.num_heads, bp.group_size, dtype, rnd, round_p, exact_qv, key_shift, ctx)


DEAD_ROW = -5e8     # a score row whose maximum lies below this carries the -1e9 of the mask on every key


def attention_operands(qu: torch.Tensor, k: torch.Tensor, v: torch.Tensor, e: torch.Tensor, dvu: torch.Tensor, lens: Optional[torch.Tensor], t: int,
                       heads: int, group: int, dtype, rnd: Callable = q, round_p: bool = False, exact_qv: bool = False, key_shift: int = 0,
                       ctx: Optional[dict] = None, edit_scores: Optional[Callable] = None, dead_rows: str = "auto"):
    """``attention`` on explicit operands: dvu (D,) = v - u as the kernel holds it (float32 numbers; rnd = ident: any), ``ctx`` the keyword arguments
    relpos_scores takes for causal / streaming contexts.
    Dead rows - queries whose every key is masked (the whole band in the padding; every query of an empty utterance): the reference adds -1e9 to every
    score of the row in float32, which IS -1e9 for |s| < 32, so its softmax is uniform over all Tg key groups, the chunk-padding group included
    (attentions.py:701; the kernels: attention2.hip ``tile_dead``).  float64 keeps s - 1e9 apart, so dead_rows = "auto" sets those rows' scores to 0 in
    float64 runs and leaves float32 runs as they come out; "keep" never touches them (tests/test_attention_cases_host.py proves the two equal).
    Tests only: ``edit_scores(s, again)`` returns the scores to use instead of s (B, H, Tg, Tg) - again(e=None, **ctx) evaluates relpos_scores on the same
    operands with another table / other contexts - the hook the injected faults of tests/attention_cases.py go through."""
    qu, k, v, e, dvu = qu.to(dtype), k.to(dtype), v.to(dtype), e.to(dtype), dvu.to(dtype)
    bsz, tp, dim = qu.shape
    g, h = group, heads
    qv = qu + dvu if (rnd is ident or exact_qv) else rnd(qu + dvu)
    ctx = dict(ctx or {})
    ml = lens
    if key_shift:
        ml = (lens if lens is not None else torch.full((bsz,), t)) + key_shift * g
    s = R.relpos_scores(qu, qv, k, e, ml, t, h, g, **ctx)
    if edit_scores is not None:
        s = edit_scores(s, lambda table=None, **kw: R.relpos_scores(qu, qv, k, e if table is None else table.to(dtype), ml, t, h, g, **dict(ctx, **kw)))
    if dead_rows == "auto" and dtype == torch.float64:
        s = torch.where(s.amax(-1, keepdim=True) < DEAD_ROW, torch.zeros_like(s), s)
    tg, d = tp // g, g * dim // h
    vh = v.reshape(bsz, tg, h, d).transpose(1, 2)
    pr = _exp(s - s.amax(-1, keepdim=True))
    den = pr.sum(-1, keepdim=True)
    if round_p and rnd is not ident:
        pr = rnd(pr)
    o = (pr @ vh) / den
    env = (pr @ vh.abs()) / den
    un = lambda z: z.transpose(1, 2).reshape(bsz, tp, dim)[:, :t]
    return un(o), un(env)


def out_proj(x_ffn1: torch.Tensor, att_o: torch.Tensor, sd, bp, dtype, rnd: Callable = q) -> torch.Tensor:
    """x_mhsa = x_ffn1 + att_o . q(Wo)^T + bo  (att_o: the stored bf16 attention output)."""
    m = "blocks.%d.multi_head_self_attention_module.mhsa.output_layer" % bp.index
    return x_ffn1.to(dtype) + _mm(att_o.to(dtype), rnd(_w(sd, m + ".weight", dtype)), "out") + _w(sd, m + ".bias", dtype)


# ------------------------------------------------------------------ convolution side
def glu(x_mhsa: torch.Tensor, sd, bp, dtype, folded: bool, rnd: Callable = q) -> torch.Tensor:
    """a * sigmoid(b) of the pointwise-1 product, before its bf16 store (..., De)."""
    p = "blocks.%d.convolution_module.layers" % bp.index
    h = ln_linear(x_mhsa, sd, p + ".2.weight", p + ".2.bias", p + ".0", dtype, folded, rnd, conv1x1=True, kind="pw1")
    a, b = h.chunk(2, dim=-1)
    return a * sigmoid(b)


def depthwise(g: torch.Tensor, sd, bp, dtype, causal: bool = False, rnd: Callable = q, shift: int = 0) -> torch.Tensor:
    """g (B, T, De): the STORED bf16 GLU output of utterances that all have T frames -> swish(BatchNorm(depthwise conv)) (B, To, De) before the
    bf16 store.  Taps and bias with the BatchNorm folded in float32.  ``shift`` (tests only): taps moved by that many frames."""
    p = "blocks.%d.convolution_module.layers" % bp.index
    ft = dtype if rnd is ident else torch.float32
    sc = _w(sd, p + ".5.weight", ft) / torch.sqrt(_w(sd, p + ".5.running_var", ft) + R.BN_EPS)
    taps = (_w(sd, p + ".4.weight", ft)[:, 0, :] * sc[:, None]).to(dtype)
    bias = (_w(sd, p + ".4.bias", ft) * sc + (_w(sd, p + ".5.bias", ft) - _w(sd, p + ".5.running_mean", ft) * sc)).to(dtype)
    ks = bp.kernel_size
    half = (ks - 1) // 2
    lo, hi = (ks - 1, 0) if causal else (half, half)
    h = F.pad(g.to(dtype).transpose(1, 2), (lo + shift, max(hi - shift, 0)))
    h = F.conv1d(h, taps[:, None, :], bias, stride=bp.conv_stride, groups=taps.shape[0])
    to = (g.shape[1] - 1) // bp.conv_stride + 1
    return swish(h)[:, :, :to].transpose(1, 2)


def conv_res(x_mhsa: torch.Tensor, sd, bp, dtype, rnd: Callable = q) -> torch.Tensor:
    """The residual branch around the convolution module of (B, T, D) rows: identity, or on transition blocks q(x[::s]) . q(W)^T + b."""
    x = x_mhsa.to(dtype)
    if not bp.transition:
        return x[:, ::bp.conv_stride]
    m = "blocks.%d.conv_res.1" % bp.index
    return _mm(rnd(x[:, ::bp.conv_stride]), rnd(_w(sd, m + ".weight", dtype)[:, :, 0]), "res") + _w(sd, m + ".bias", dtype)


def chain_a(res: torch.Tensor, dw: torch.Tensor, sd, bp, next_bp, dtype, folded: bool, folded_next: Optional[bool] = None, rnd: Callable = q,
            fault: Optional[Callable] = None) -> dict:
    """res (..., De) float32 residual rows (conv_res's output), dw (..., De) the STORED bf16 depthwise output ->
    {"x_conv": res + dw . q(Wpw2)^T + b, "out": LayerNorm(x_conv + 1/2 FFN2), "x_ffn1": out + 1/2 FFN1 of block ``next_bp`` (absent for the last)}.
    ``fault`` (tests only): the hook of ``ffn`` for FFN2, also called with "ln_out" (the block LayerNorm's input -> its output)."""
    p = "blocks.%d" % bp.index
    c = p + ".convolution_module.layers.7"
    x = res.to(dtype) + _mm(dw.to(dtype), rnd(_w(sd, c + ".weight", dtype)[:, :, 0]), "pw2") + _w(sd, c + ".bias", dtype)
    out = {"x_conv": x}
    x = ffn(x, sd, p + ".feed_forward_module2", dtype, folded, rnd, fault)
    y = fault("ln_out", x) if fault else None
    if y is None:
        y = ln_plain(x) * _w(sd, p + ".norm.weight", dtype) + _w(sd, p + ".norm.bias", dtype)
    out["out"] = y
    if next_bp is not None:
        out["x_ffn1"] = ffn(y, sd, "blocks.%d.feed_forward_module1" % next_bp.index, dtype, folded if folded_next is None else folded_next, rnd)
    return out


# ------------------------------------------------------------------ the stages chained: a whole encoder from the front end's output
def encoder_from_linear(x: torch.Tensor, lens: Optional[torch.Tensor], sd, plan, dtype, rnd: Callable = q, folded=True,
                        trace: Optional[dict] = None, faults: Optional[dict] = None) -> torch.Tensor:
    """x (B, T, D0): the front end's output (trace entry ``linear``) -> the encoder output (B, T_out, D_last), every stage above in sequence,
    each bf16-stored intermediate rounded with ``rnd``.  With rnd = ident this is ref_encoder.encoder_from_mel behind its Linear.
    ``folded``: bool, or a function of the stage width (the fused chains' widths).  ``trace`` receives what the bf16 path's debug trace holds,
    under its names, as (B, rows, columns) (``e``: (rows, columns)).  ``faults`` (tests only): {(block, stage): keyword arguments for that stage}."""
    fold = folded if callable(folded) else (lambda width: bool(folded))
    faults = faults or {}
    x = x.to(dtype)
    b0 = plan.blocks[0]
    x = ffn(x, sd, "blocks.0.feed_forward_module1", dtype, fold(b0.dim_model), rnd)
    nb = len(plan.blocks)
    for i, bp in enumerate(plan.blocks):
        p = "blocks.%d" % bp.index
        t = x.shape[1]
        tp = (t + bp.group_size - 1) // bp.group_size * bp.group_size
        fin, fout = fold(bp.dim_model), fold(bp.dim_expand)
        qu, k, v = (rnd(z) for z in qkv(x, sd, bp, dtype, fin, rnd))
        qu, k, v = pad_rows(qu, k, v, sd, bp, rnd)
        e = rnd(pos_e(tp, sd, bp, dtype, plan.causal, rnd, **faults.get((i, "pos_e"), {})))
        o, _ = attention(qu, k, v, e, lens, t, sd, bp, dtype, rnd, plan=plan, **faults.get((i, "attention"), {}))
        o = rnd(o)
        xm = out_proj(x, o, sd, bp, dtype, rnd)
        g = rnd(glu(xm, sd, bp, dtype, fin, rnd))
        dw = rnd(depthwise(g, sd, bp, dtype, plan.causal, rnd, **faults.get((i, "depthwise"), {})))
        res = conv_res(xm, sd, bp, dtype, rnd)
        nbp = plan.blocks[i + 1] if i + 1 < nb else None
        st = chain_a(res, dw, sd, bp, nbp, dtype, fout, fold(nbp.dim_model) if nbp is not None else None, rnd, **faults.get((i, "chain_a"), {}))
        if trace is not None:
            for nm, val in (("x_ffn1", x), ("qu", qu), ("k", k), ("v", v), ("e", e), ("att_o", o), ("x_mhsa", xm), ("glu", g), ("dw", dw),
                            ("x_conv", st["x_conv"]), ("out", st["out"])):
                trace[p + "." + nm] = val
        x = st["x_ffn1"] if nbp is not None else st["out"]
        if bp.conv_stride > 1 and lens is not None:
            lens = torch.div(lens - 1, bp.conv_stride, rounding_mode="floor") + 1
    return x


# ------------------------------------------------------------------ statistics of the parity tests (tests/test_ref_bf16_host.py, tests/test_gpu_bf16_rounding.py)
def rel(got: torch.Tensor, ref: torch.Tensor) -> Tuple[float, float]:
    """The project's relative error: max and mean of |got - ref| over the tensor, divided by max(|ref|.max(), 1)."""
    d = (got.double() - ref.double()).abs()
    s = max(float(ref.abs().max()), 1.0)
    return float(d.max()) / s, float(d.mean()) / s


def stage_ratios(got: torch.Tensor, r64: torch.Tensor, r32: torch.Tensor, k_len: int, bf16_out: bool, share_factor: float = 4.0) -> dict:
    """statistic / bound of one stage (> 1: over the bound), ``got`` = the stored output under test, r64 / r32 = the stage's reference in
    float64 / float32 arithmetic from the SAME inputs, before the output's rounding.
    "max":  rel(got, r64).max  / max(4 * rel(n32, r64).max,  sqrt(K) 2^-23);   "mean": rel(got, r64).mean / max(8 * rel(n32, r64).mean, sqrt(K) 2^-23)
    with n32 = r32 (float32 outputs) or q(r32) (bf16 outputs).  bf16 outputs with a ``share_factor``: "share" = (1 - share(got == q(r64))) /
    (share_factor * (1 - share(q(r32) == q(r64)))).  "noise_max" / "noise_mean": the same statistics over the raw noise (no factor, no floor)."""
    runs = list(r32) if isinstance(r32, (list, tuple)) else [r32]
    floor = float(k_len) ** 0.5 * 2.0 ** -23
    noise = [rel(q(r) if bf16_out else r, r64) for r in runs]
    nmax, nmean = max(n[0] for n in noise), sum(n[1] for n in noise) / len(noise)
    gmax, gmean = rel(got, r64)
    out = {"max": gmax / max(4.0 * nmax, floor), "mean": gmean / max(8.0 * nmean, floor),
           "noise_max": gmax / max(nmax, 1e-300), "noise_mean": gmean / max(nmean, 1e-300),
           "single_max": gmax / max(4.0 * noise[0][0], floor), "single_mean": gmean / max(8.0 * noise[0][1], floor)}
    if bf16_out and share_factor:
        want = q(r64).double()
        miss_n = sum(1.0 - float((q(r).double() == want).double().mean()) for r in runs) / len(runs)
        miss_g = 1.0 - float((got.double() == want).double().mean())
        out["share"] = 0.0 if miss_g == 0.0 else (miss_g / (share_factor * miss_n) if miss_n > 0.0 else float("inf"))
        miss_1 = 1.0 - float((q(runs[0]).double() == want).double().mean())
        out["single_share"] = 0.0 if miss_g == 0.0 else (miss_g / (share_factor * miss_1) if miss_1 > 0.0 else float("inf"))
    return out


def worst_element(got: torch.Tensor, ref: torch.Tensor, scale: Optional[torch.Tensor] = None) -> str:
    """Where a stage is worst: row, column, row tile (row // 32) and column tile (column // 32) of the largest |got - ref| (/ scale)."""
    d = (got.double() - ref.double()).abs()
    if scale is not None:
        d = d / scale.double()
    d = d.reshape(-1, d.shape[-1])
    i = int(d.argmax())
    r, c = i // d.shape[1], i % d.shape[1]
    return "worst element row %d col %d (row tile %d, column tile %d): got %.9g want %.9g" % (
        r, c, r // 32, c // 32, float(got.reshape(-1, d.shape[1])[r, c]), float(ref.reshape(-1, d.shape[1])[r, c]))


def f32_runs(fn: Callable) -> list:
    """The float32 noise runs of one stage: fn() under torch's float32 functions and under hardware_like(s), s = 0, +-1, +-2.
    Why +-2: the LayerNorm-ed operand x * rstd - mean * rstd is a composition of a rounded sum and division (the mean), a one-ulp rsqrt, two
    rounded products and a rounded sum - about 2 float32 ulps of the operand in all; exp2(-1.4427 x) carries |x| ulps of its argument's rounding
    into the sigmoid, again about 2 ulps at the |x| <= 8 where the sigmoid is not yet 0 or 1.  An operand within that distance of a bf16 tie may
    round either way in a correct kernel, and ONE such operand moves 10 - 40 % of the bf16 outputs of its row by a unit; torch's float32 run alone
    samples a single point of that interval."""
    out = [fn()]
    for ulps in (0, 1, -1, 2, -2):
        with hardware_like(ulps):
            out.append(fn())
    return out
