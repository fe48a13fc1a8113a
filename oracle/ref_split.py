"""ORACLE - test infrastructure only: the split mode's arithmetic (precision = "split"), as a noise model for oracle/ref_bf16.py's stages.

The split mode's contract is "no rounding anywhere": its float64 REFERENCE is ref_bf16's stage functions with ``rnd = ident`` (chained, they are
oracle/ref_encoder.py; tests/test_ref_bf16_host.py and tests/test_ref_split_host.py).  Nothing of a stage is restated here.  What this module adds is what a
CORRECT split kernel may differ from that reference by: the operand pairs of the fp16 matrix pipe, written down once with the source line of every step, and
plugged into the same stage functions through ref_bf16.product_like (every matrix product) and ref_bf16._SPLIT_OPS (the front end's convolution).

The kernels' arithmetic
* Same-scale pair (sx_common.h split2s; sxf_chain.hip, sxf_sub.hip, sxf.hip): the operand times its power-of-two scale S, h = fp16 toward zero
  (``__builtin_amdgcn_cvt_pkrtz``: v_cvt_pkrtz_f16_f32 truncates and saturates at 65504), l = fp16 round-to-nearest of x S - h (``__builtin_convertvector``).
  Scales, per operand class (split-mode operand envelopes): SA = 2^8 LayerNorm-ed rows and Swish outputs (sxf_chain.hip: SA, SR, SW -
  acc_to_frags(acc, mean, rstd * SA, SA, ...), swish_frags ``(z * SA) * rcp``; sxf_sub.hip:25 hidden activation), SR = 2^6 operands that are not LayerNorm-ed - the
  attention output and the depthwise output (sxf_chain.hip:33, acc_to_frags(acc, 0.f, SR, SR, ...)), SP = 2^6 the mel patch (sxf_sub.hip:25), SQK = SV_ = 2^8
  Q + u, K, E, V and SP_ = 2^10 the probabilities (sxf.hip:26), SW = 2^10 every weight image (pack.h f16_pair_s10: ws = float(w 1024), h = (_Float16)ws - round to
  nearest -, l = fp16(ws - h)).
* Product = a_h w_h + a_h w_l + a_l w_h, fp32 accumulation (sxf_chain.hip g1: one accumulator per product kind, summed ``(h1 + h2) + h3``), the scale undone by
  one exact multiply (UNS = 1 / (SA SW), UNS_R = 1 / (SR SW)).  The l l' term is dropped.
* Per-module form (split.hip sx_gemm_kernel; sx_common.h split2): x = h + l / 2048 with h = fp16 toward zero of the UNSCALED value, l = fp16((x - h) 2048)
  clamped to +-65000; weights h = fp16(w), l = fp16((w - h) 2048) (pack.h f16_pair_2048, pack.hip split_pair_image); two accumulators acc = a_h w_h and
  acx = a_h w_l + a_l w_h, result fmaf(acx, 1 / 2048, acc) (split.hip:135-137, 189).  It runs the positional projection and conv_res on every route, and every
  product where the fused kernels are off or not built (D = 360 .. 720).
* LayerNorm: sxf_chain.hip row_stats (mean = sum / D, rstd = rsqrtf(sum (x - mean)^2 / D + 1e-6)) and apply_ln / acc_to_frags ((x - mean) rstd): the float32
  formulas ref_bf16.hardware_like already evaluates, with the rsqrt moved by s ulps.  gamma / beta of a pre-norm are folded into the weight image and its bias
  column (pack.hip f1_chunk: ``g ? wv * g[f] : wv``, ``bsum += wv * beta[f]`` in double) - ref_bf16.ln_linear's ``folded`` form, taken here with
  ``rnd = keep`` (an identity that is not ``ident``).  The bias column is itself a split pair against the operand 1.0: 2^-23 of the bias, not modelled.
* exp / reciprocal: sx_common.h sx_expf (x log2(e) in two parts, v_exp_f32, first-order correction) and sx_rcp (v_rcp_f32 + one Newton step) in the GLU, the
  depthwise Swish (sxf.hip:459, 485) and chain B's GLU (sxf_chain.hip:588); the FFN Swish of the chains uses the same exp without the constant's low part and a
  plain v_rcp_f32 (sxf_chain.hip swish_frags).  Both are ref_bf16.sigmoid under hardware_like(s): rcp(1 + exp2(-x log2 e)) moved by s ulps.  The SOFTMAX does not
  call sx_expf: scores are kept in log2 units (sxf.hip:117 ``c2 = log2(e) / sqrt(d) / SQK^2``) and go through v_exp_f32 directly (sxf.hip:259) - ref_bf16._exp
  under hardware_like evaluates the sx_expf formula, an equally good float32 evaluation of exp.

``split_runs(fn)``: the noise runs of one stage, fn(dtype, rnd) - torch's float32 run, the hardware_like(s) runs, and the emulated runs (hardware_like(s) with
the products above).  The parity tests multiply the worst / mean noise of these runs by the project's 4 / 8.

The element-wise term (tests/split_parity.py adds it to the classical 2 K 2^-23 (|a| |w|^T + |x| + |b|))
From split2s: h truncates x S to 11 significant bits, so 0 <= (x S - h) sign(x) < ulp(h) <= 2^-10 |x S|; l rounds that remainder to nearest, |l| <= 2^-10 |x S|,
and since the remainder is below ulp(h) = 2^(e - 10) (|x S| >= 2^e) its own half-ulp is at most 2^(e - 22) <= 2^-22 |x S|: representation error <= 2^-22 |x|
+ 2^-25 / S, the second term where l is a subnormal fp16 number (quantum 2^-24; the split2s comment: "contributes < 2^-25 S^-1 absolutely").  Weight images round
h to nearest: |l'| <= 2^-11 |w S'|, representation error <= 2^-23 |w| + 2^-25 / S'.  With a^ = (h + l) / S:
  |a w - (a_h w_h + a_h w_l + a_l w_h) / (S S')| <= |a - a^| |w| + |a^| |w - w^| + |l l'| / (S S')
                                                 <= (2^-22 + 2^-23 + 2^-21) |a| |w| + 2^-25 (|w| / S + |a| / S')  <  2^-20 |a| |w| + 2^-25 (|w| / S + |a| / S').
The per-module form truncates both h the same way on the activation side and scales l by 2048 before rounding (no underflow above 2^-36): inside the same
expression with S = S' = 2048.  ``split_term`` evaluates it; tests/test_ref_split_host.py holds the emulation (exact accumulation) inside it and above 1 / 50 of it.
"""
from __future__ import annotations

from typing import Callable, Iterable, Optional

import torch

from . import ref_bf16 as Q
from .ref_bf16 import hardware_like, ident, product_like

F64, F32 = torch.float64, torch.float32
SA, SR, SW, SP, SQK, SV_, SP_ = 256.0, 64.0, 1024.0, 64.0, 256.0, 256.0, 1024.0
LO_SCALE = 2048.0
# the scale of the activation operand of every product the fused kernels run (sxf_chain.hip, sxf_sub.hip)
FUSED_SCALE = {"ffn1": SA, "ffn2": SA, "qkv": SA, "pw1": SA, "linear": SA, "out": SR, "pw2": SR}
CHAIN_KINDS = frozenset(("ffn1", "ffn2", "qkv", "pw1", "out", "pw2"))      # split_chain = 1 at a width the chains are built for
FFN_KINDS = frozenset(("ffn1", "ffn2"))                                     # split_chain = 0, split_ffn = 1: the FFN-only form of sxf_chain.hip's chain A only
NO_KINDS = frozenset()                                                      # every product on split.hip


def keep(x: torch.Tensor) -> torch.Tensor:
    """An identity that is not ``ident``: ref_bf16's stages then take their kernel-shaped forms (folded LayerNorm, float32 folds) without any rounding."""
    return x


def pkrtz(x: torch.Tensor) -> torch.Tensor:
    """fp16 toward zero of float32 numbers, as float32 (v_cvt_pkrtz_f16_f32): 11 significant bits, quantum 2^-24 below 2^-14, saturation at 65504."""
    x = x.float().contiguous()
    normal = (x.view(torch.int32) & -8192).view(torch.float32)               # the low 13 mantissa bits cleared
    sub = torch.trunc(x * 2.0 ** 24) * 2.0 ** -24
    return torch.where(x.abs() < 2.0 ** -14, sub, normal).clamp(-65504.0, 65504.0)


def rn16(x: torch.Tensor) -> torch.Tensor:
    """fp16 round-to-nearest-even of float32 numbers, as float32."""
    return x.float().to(torch.float16).float()


def split2s(xs: torch.Tensor, lo_bits: int = 11):
    """sx_common.h split2s on already scaled values: (h, l).  ``lo_bits`` (tests only): l keeps that many of its 11 significant bits (a mis-scaled l that
    lands in fp16's subnormal range: formed at 2^-6 of its scale next to the underflow threshold it keeps 5)."""
    xs = xs.float()
    h = pkrtz(xs)
    l = rn16(xs - h)
    if lo_bits < 11:
        m, e = torch.frexp(l)
        l = torch.ldexp(torch.round(m * 2.0 ** lo_bits) * 2.0 ** -lo_bits, e)
    return h, l


def split2(x: torch.Tensor):
    """sx_common.h split2: (h, l) with x = h + l / 2048."""
    x = x.float()
    h = pkrtz(x)
    return h, rn16(((x - h) * LO_SCALE).clamp(-65000.0, 65000.0))


def weight_same(w: torch.Tensor):
    """pack.h f16_pair_s10, the element of the fused images: ws = float(w 1024), h = fp16(ws), l = fp16(ws - h)."""
    ws = (w.double() * SW).float()
    h = rn16(ws)
    return h, rn16(ws - h)


def weight_module(w: torch.Tensor):
    """pack.h f16_pair_2048, per-module images: h = fp16(w), l = fp16((w - h) 2048)."""
    w = w.float()
    h = rn16(w)
    return h, rn16((w - h) * LO_SCALE)


class Emu:
    """The split product as ref_bf16.product_like's function: (a, w, kind) -> a . w^T by the kernels' three MFMAs.  ``fused``: the kinds that run on the
    same-scale kernels (the others: split.hip's form).  Accumulation in a's dtype (float32: the kernels'; float64: the operand pairs alone, exactly summed).
    ``chunk``: contract in chunks of that many k, one after the other (another summation order: the stand-in kernels of tests/test_ref_split_host.py).
    ``fault`` (tests only): (kind, planes) -> None, may edit planes = {"ah", "al", "wh", "wl"} ((rows, K) / (N, K), scaled) in place; ``post``: (kind, product)
    -> product; ``lo_bits``: see split2s."""

    def __init__(self, fused: Iterable[str] = CHAIN_KINDS, chunk: Optional[int] = None, fault: Optional[Callable] = None, lo_bits: int = 11,
                 post: Optional[Callable] = None):
        self.fused, self.chunk, self.fault, self.lo_bits, self.post = frozenset(fused), chunk, fault, lo_bits, post

    def planes(self, a, w, kind):
        if kind in self.fused:
            s = FUSED_SCALE[kind]
            ah, al = split2s(a.float() * s, self.lo_bits)
            wh, wl = weight_same(w)
            return {"ah": ah, "al": al, "wh": wh, "wl": wl}, 1.0 / (s * SW), 1.0
        ah, al = split2(a)
        wh, wl = weight_module(w)
        return {"ah": ah, "al": al, "wh": wh, "wl": wl}, 1.0, 1.0 / LO_SCALE

    def __call__(self, a: torch.Tensor, w: torch.Tensor, kind: str) -> torch.Tensor:
        dt = a.dtype
        p, uns, lo_inv = self.planes(a, w, kind)
        if self.fault is not None:
            self.fault(kind, p)
        ah, al, wh, wl = (p[n].to(dt) for n in ("ah", "al", "wh", "wl"))
        k = ah.shape[-1]
        step = self.chunk or k
        main = corr = None
        for c in range(0, k, step):
            sl = slice(c, c + step)
            m = ah[..., sl] @ wh[:, sl].T
            x = ah[..., sl] @ wl[:, sl].T + al[..., sl] @ wh[:, sl].T
            main, corr = (m, x) if main is None else (main + m, corr + x)
        out = (main + corr) * uns if lo_inv == 1.0 else corr * lo_inv + main      # same scale: one sum, an exact multiply | split.hip: fmaf(acx, 1 / 2048, acc)
        return out if self.post is None else self.post(kind, out)


class split_front:
    """``with split_front():`` ref_bf16.front_conv(conv="split") splits its operands as sxf_sub.hip does: taps (and the folded bias in tap 9) at SW like every
    weight image, the mel patch (and the constant 1.0 of tap 9) at SP; the values are returned unscaled (powers of two: exact)."""

    def __enter__(self):
        self.prev = Q._SPLIT_OPS
        wsp = lambda w: tuple(z / SW for z in weight_same(w))
        psp = lambda x: tuple(z / SP for z in split2s(x.float() * SP))
        Q._SPLIT_OPS = (wsp, psp)

    def __exit__(self, *a):
        Q._SPLIT_OPS = self.prev


def pair22(x: torch.Tensor, scale: float) -> torch.Tensor:
    """h + l of the same-scale pair, unscaled: the 22 bits of an operand the attention kernel's images keep (sxf.hip pack kernels, SQK / SV_)."""
    h, l = split2s(x.float() * scale)
    return ((h.double() + l.double()) / scale).to(x.dtype)


def split_runs(fn: Callable, fused: Iterable[str] = CHAIN_KINDS, front: bool = False) -> list:
    """The noise runs of one stage.  fn(dtype, rnd) evaluates the stage (rnd = ident: the plain form; rnd = keep: the kernels' form, e. g. the folded LayerNorm;
    a ``conv=`` keyword is passed where ``front``): torch's float32 run, the same under hardware_like(s), s = 0, +-1, +-2 (ref_bf16.f32_runs says why +-2), and
    the emulated runs - the operand pairs of this module under hardware_like(0, +-2)."""
    call = (lambda rnd, conv: fn(F32, rnd, conv=conv)) if front else (lambda rnd, conv: fn(F32, rnd))
    runs = [call(ident, "fp32")]
    for s in (0, 1, -1, 2, -2):
        with hardware_like(s):
            runs.append(call(ident, "fp32"))
    for s in (0, 2, -2):
        with hardware_like(s), product_like(Emu(fused)), split_front():
            runs.append(call(keep, "split"))
    return runs


def stand_in(fn: Callable, fused: Iterable[str] = CHAIN_KINDS, front: bool = False, ulps: int = 1, **emu) -> torch.Tensor:
    """A correct kernel on the CPU: the emulation in ANOTHER summation order (chunks of 32 k, one after the other, as the chains walk their weight chunks)
    and with the hardware functions at an ulp shift no noise run uses.  ``emu``: Emu's fault keywords."""
    with hardware_like(ulps), product_like(Emu(fused, chunk=32, **emu)), split_front():
        return fn(F32, keep, conv="split") if front else fn(F32, keep)


def split_term(a_abs: torch.Tensor, w_abs: torch.Tensor, sa: float, sw: float = SW) -> torch.Tensor:
    """The element-wise bound of the split representation on a (rows, K) . (N, K)^T product (module docstring):
    2^-20 |a| |w|^T + 2^-25 (sum_k |w| / sa + sum_k |a| / sw)."""
    a_abs, w_abs = a_abs.double(), w_abs.double()
    return 2.0 ** -20 * (a_abs @ w_abs.T) + 2.0 ** -25 * (w_abs.sum(-1)[None, :] / sa + a_abs.sum(-1, keepdim=True) / sw)
