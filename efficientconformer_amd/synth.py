"""Deterministic synthetic weights and inputs (no checkpoints or datasets are reachable offline).

Weights: a *key-seeded* generator — every state-dict key gets its own
``numpy`` PCG64 stream seeded with ``crc32(key) ^ seed`` — so the same tensors
are produced in the build container (where the golden vectors are captured from
the reference, tools/make_goldens.py) and on the GPU box.  numpy's PCG64 +
``standard_normal`` is specified to be reproducible across platforms, unlike
``torch.randn``.

Inputs follow SURVEY.md section 8(d): mel ~ N(-5.65, 4.23^2) (the dataset statistics
recorded in the reference configs, configs/EfficientConformerCTCSmall.json:36-37),
audio = 0.1*randn clipped to [-1, 1] and zeroed beyond each length (collate
zero-pad, reference utils/preprocessing.py:38), lengths sorted descending
(utils/preprocessing.py:33).
"""
from __future__ import annotations

import math
import zlib
from typing import Dict, List

import numpy as np

from . import params as P
from .config import EncoderPlan


def _rng(key: str, seed: int) -> np.random.Generator:
    return np.random.Generator(np.random.PCG64((zlib.crc32(key.encode()) ^ seed) & 0xFFFFFFFF))


def make_tensor(key: str, shape, kind: str, seed: int) -> np.ndarray:
    g = _rng(key, seed)
    if kind == P.W:
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else int(shape[0])
        return (g.standard_normal(shape) / math.sqrt(fan_in)).astype(np.float32)
    if kind == P.B:
        return (0.02 * g.standard_normal(shape)).astype(np.float32)
    if kind == P.GAMMA:
        return (1.0 + 0.1 * g.standard_normal(shape)).astype(np.float32)
    if kind == P.BETA:
        return (0.1 * g.standard_normal(shape)).astype(np.float32)
    if kind == P.RMEAN:
        return (0.2 * g.standard_normal(shape)).astype(np.float32)
    if kind == P.RVAR:
        return g.uniform(0.5, 1.5, shape).astype(np.float32)
    if kind == P.NBT:
        return np.zeros(shape, dtype=np.int64)
    if kind == P.UV:
        return (0.1 * g.standard_normal(shape)).astype(np.float32)
    if kind == P.EMB:                      # nn.Embedding init N(0, 1) with the padding_idx = 0 row zeroed (decoders.py:46)
        e = g.standard_normal(shape).astype(np.float32)
        e[0] = 0.0
        return e
    raise ValueError(kind)


def make_state_dict(plan: EncoderPlan, seed: int = 0, vocab: int | None = None, prefix: str = "") -> Dict[str, np.ndarray]:
    """Key-seeded weights for the encoder (keys without prefix unless given) and optional ``fc`` head."""
    sd = {}
    for key, shape, kind in P.param_specs(plan):
        sd[prefix + key] = make_tensor(key, shape, kind, seed)
    if vocab is not None:
        for key, shape, kind in P.head_specs(plan, vocab):
            sd[key] = make_tensor(key, shape, kind, seed)
    return sd


def make_transducer_state_dict(dim_encoder: int, decoder_params: dict, joint_params: dict, seed: int = 0,
                               blank_bias: float = 0.0) -> Dict[str, np.ndarray]:
    """Key-seeded prediction / joint network weights (keys ``decoder.*`` / ``joint_network.*``).

    ``blank_bias`` is added to the blank logit's bias: with purely random weights the blank wins 1/V of the decisions and
    greedy decoding emits ``max_consec_dec_step`` tokens on every frame (a useful stress case, but not what a trained
    model does); ~1.2 gives the roughly 1 token per 3-4 encoder frames of a trained LibriSpeech model."""
    sd = {}
    for key, shape, kind in P.transducer_specs(dim_encoder, decoder_params, joint_params):
        sd[key] = make_tensor(key, shape, kind, seed)
    sd["joint_network.linear_joint.bias"][0] += np.float32(blank_bias)
    return sd


def make_lm_state_dict(lm_params: dict, seed: int = 0, bias=None) -> Dict[str, np.ndarray]:
    """Key-seeded LanguageModel weights (keys ``decoder.embedding.weight``, ``decoder.rnn.*_l{k}``, ``fc.*``).  The embedding row of id 0 is zero
    (padding_idx = 0, decoders.py:46).  ``bias``: None, or a (vocab,) array added to ``fc.bias`` - the unigram preference a trained LM has and
    purely random weights lack (tests choose one under which rescoring moves some winners and keeps others)."""
    sd = {key: make_tensor("lm." + key, shape, kind, seed) for key, shape, kind in P.lm_specs(lm_params)}
    if bias is not None:
        sd["fc.bias"] = (sd["fc.bias"] + np.asarray(bias, dtype=np.float32)).astype(np.float32)
    return sd


def make_mel(batch: int, n_mels: int, tm: int, lengths: List[int] | None = None, seed: int = 4321):
    """Seeded mel batch (B, n_mels, Tm) float32 + int64 mel lengths (sorted descending)."""
    g = np.random.Generator(np.random.PCG64(seed))
    mel = (-5.6501 + 4.2280 * g.standard_normal((batch, n_mels, tm))).astype(np.float32)
    if lengths is None:
        lengths = [tm] * batch
    lens = np.asarray(sorted(lengths, reverse=True), dtype=np.int64)
    assert lens.max() <= tm
    return mel, lens


def libri_lengths(batch: int, seed: int = 1234, sample_rate: int = 16000) -> np.ndarray:
    """'LibriSpeech-shaped' utterance lengths in samples (SURVEY.md section 8d W-libri):
    16000 * clip(lognormal(ln 11, 0.45), 1.5, 16.0) s, sorted descending within the batch."""
    g = np.random.Generator(np.random.PCG64(seed))
    sec = np.clip(g.lognormal(math.log(11.0), 0.45, batch), 1.5, 16.0)
    return np.sort((sec * sample_rate).astype(np.int64))[::-1].copy()


def make_audio(lengths, seed: int = 1234) -> np.ndarray:
    """Audio (B, L_max) float32: 0.1*randn clipped to [-1,1], rows zeroed beyond each length."""
    lengths = np.asarray(lengths, dtype=np.int64)
    g = np.random.Generator(np.random.PCG64(seed ^ 0x5EED))
    x = np.clip(0.1 * g.standard_normal((len(lengths), int(lengths.max())), dtype=np.float32), -1.0, 1.0)
    for b, n in enumerate(lengths):
        x[b, n:] = 0.0
    return x


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Stressed parameter sets: statistics of trained checkpoints and values at the split-precision images' limits
# ---------------------------------------------------------------------------------------------------------------------------------------------

SPLIT_IMG_LIMIT = 65000.0 / 1024.0   # largest |folded value| the fused split images hold (csrc/pack.h: w * 2^10 as two fp16 halves, kSplitImgMax)
STRESS_PROFILES = ("trained", "boundary")


def silence_floor_mel(batch: int, n_mels: int, tm: int, lengths: List[int] | None = None, seed: int = 4321):
    """``make_mel`` with runs of digital silence and a few loud frames: every utterance gets one or two runs of 5 - 40 frames at the
    log floor log(1e-9) = -20.72 (modules.py:96 on an all-zero spectrum) and 1 - 3 frames at +12 (a clipped, full-scale burst)."""
    mel, lens = make_mel(batch, n_mels, tm, lengths, seed)
    g = np.random.Generator(np.random.PCG64(seed ^ 0x51E7))
    floor, loud = np.float32(math.log(1e-9)), np.float32(12.0)
    for b, n in enumerate(lens):
        n = int(n)
        for _ in range(int(g.integers(1, 3))):
            run = int(min(n, g.integers(5, 41)))
            t0 = int(g.integers(0, n - run + 1))
            mel[b, :, t0:t0 + run] = floor
        for t in g.integers(0, n, int(g.integers(1, 4))):
            mel[b, :, int(t)] = loud + g.standard_normal(n_mels).astype(np.float32)
    return mel, lens


def fold_bn(sd: Dict[str, np.ndarray], prefix: str):
    """BatchNorm(eval) as per-channel (scale, shift) in float32 - the fold of csrc/pack.hip bn_fold."""
    s = (sd[prefix + ".weight"] / np.sqrt(sd[prefix + ".running_var"] + np.float32(1e-5))).astype(np.float32)
    return s, (sd[prefix + ".bias"] - sd[prefix + ".running_mean"] * s).astype(np.float32)


def split_image_values(plan: EncoderPlan, sd: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """Every value the fused split images hold, folded as csrc/pack.hip folds them at finalize (before the 2^10 scale), by image:
    ``sub.taps`` (conv tap x BN scale), ``sub.shift`` (BN shift + conv bias x BN scale, tap 9), ``linear``; per block k ``ffn{1,2}.w1`` (gamma W1),
    ``ffn{1,2}.bias`` (b1 + W1 beta), ``ffn{1,2}.w2`` (W2 / 2), ``pw1.w`` / ``pw1.bias`` (conv LayerNorm folded), ``qkv.w`` / ``qkv.bias``
    (attention LayerNorm folded), ``wo``, ``pw2``."""
    out: Dict[str, np.ndarray] = {}
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    if plan.sub_layers == 1:
        p = "subsampling_module.layers.0"
        sc, sh = fold_bn(sd, p + ".1")
        w = sd[p + ".0.weight"].reshape(len(sc), 9)
        out["sub.taps"] = f64(w) * f64(sc)[:, None]
        out["sub.shift"] = f64(sh + sd[p + ".0.bias"] * sc)
        out["linear"] = f64(sd["linear.weight"])

    def folded(wkey, bkey, lnkey):
        w, b = f64(sd[wkey]).reshape(sd[wkey].shape[0], -1), f64(sd[bkey])
        return w * f64(sd[lnkey + ".weight"])[None, :], b + w @ f64(sd[lnkey + ".bias"])
    for bp in plan.blocks:
        pb = "blocks.%d" % bp.index
        for i, ff in ((1, ".feed_forward_module1.layers."), (2, ".feed_forward_module2.layers.")):
            out["%s.ffn%d.w1" % (pb, i)], out["%s.ffn%d.bias" % (pb, i)] = folded(pb + ff + "1.weight", pb + ff + "1.bias", pb + ff + "0")
            out["%s.ffn%d.w2" % (pb, i)] = 0.5 * f64(sd[pb + ff + "4.weight"])
        cm, mh = pb + ".convolution_module.layers.", pb + ".multi_head_self_attention_module."
        out[pb + ".pw1.w"], out[pb + ".pw1.bias"] = folded(cm + "2.weight", cm + "2.bias", cm + "0")
        ws, bs = zip(*(folded(mh + "mhsa.%s_layer.weight" % n, mh + "mhsa.%s_layer.bias" % n, mh + "norm") for n in ("query", "key", "value")))
        out[pb + ".qkv.w"], out[pb + ".qkv.bias"] = np.concatenate(ws), np.concatenate(bs)
        out[pb + ".wo"] = f64(sd[mh + "mhsa.output_layer.weight"])
        out[pb + ".pw2"] = f64(sd[cm + "7.weight"]).reshape(bp.dim_expand, -1)
    return out


def _boundary(plan: EncoderPlan, sd: Dict[str, np.ndarray]) -> None:
    """Profile ``boundary``: synthetic weights except for one folded value of each fused split image moved ACROSS the images' limit
    (|w| < 65000 / 1024 = 63.48 after folding; csrc/pack.h kSplitImgMax) to ~100, and one moved just below it.  Targets the fused images of
    sxf_sub.hip (conv tap x BN scale, BN shift), sxf_chain.hip (gamma W1, the bias column b1 + W1 beta) and sxf_chain.hip's
    pointwise-1 (gamma W, conv-module LayerNorm folded).  The values below the limit are as close to it as the ACTIVATION envelopes allow on
    the tests' inputs: 60 for biases / shifts and for the pointwise-1 gate row (sigmoid input); 40 for gamma W1 (the Swish operand, |x| < 255,
    sees 40 x a LayerNorm-ed value); 12 for a subsampler tap (the Swish operand sees 12 x |mel| <= 12 x 20.7).  Block 0 carries the FFN1 and
    pointwise-1 values across the limit, the last block the ones below it (FFN2, pointwise-1)."""
    first, last = plan.blocks[0], plan.blocks[-1]
    if plan.sub_layers == 1:
        p = "subsampling_module.layers.0"
        sc, _ = fold_bn(sd, p + ".1")
        w = sd[p + ".0.weight"]
        w[0, 0, 1, 1] = np.float32(100.0 / sc[0])                    # channel 0, centre tap: across
        w[1, 0, 1, 1] = np.float32(12.0 / sc[1])                     # channel 1: below, within the Swish operand's envelope
        for ch, target in ((2, 100.0), (3, 60.0)):                   # folded shift (tap 9) = beta - rm sc + cb sc
            sd[p + ".1.bias"][ch] = np.float32(target - (sd[p + ".0.bias"][ch] - sd[p + ".1.running_mean"][ch]) * sc[ch])

    def ffn_pair(bp, ff, w_target, b_target):
        pf = "blocks.%d.%s.layers." % (bp.index, ff)
        g, beta, w1, b1 = sd[pf + "0.weight"], sd[pf + "0.bias"], sd[pf + "1.weight"], sd[pf + "1.bias"]
        w1[0, 0] = np.float32(w_target / g[0])                       # hidden unit 0, input 0: gamma W1
        b1[1] = np.float32(b_target - float(np.dot(w1[1].astype(np.float64), beta.astype(np.float64))))   # hidden unit 1: b1 + W1 beta

    def pw1(bp, target):
        cm = "blocks.%d.convolution_module.layers." % bp.index
        de = bp.dim_expand
        sd[cm + "2.weight"][de, 0, 0] = np.float32(target / sd[cm + "0.weight"][0])    # first GATE row (GLU sigmoid input), input 0
    ffn_pair(first, "feed_forward_module1", 100.0, 100.0)
    pw1(first, 100.0)
    ffn_pair(last, "feed_forward_module2", 40.0, 60.0)
    pw1(last, 60.0)


def _trained(plan: EncoderPlan, sd: Dict[str, np.ndarray], seed: int) -> None:
    """Profile ``trained``: statistics a trained checkpoint plausibly has, inside every documented envelope (split-mode operand envelopes):
    LayerNorm gains log-normal in [0.05, 5] and shifts +-1 (the range the LayerNorm-ed operand envelopes |x| < 255 are stated for); biases +-0.5;
    3 % of every weight's rows x 4; u / v +-1; Q / K scaled until the content term of the attention logits reaches 20 (the relative-position term adds to it) (deferred softmax rescale, attention2.hip RESCALE_T);
    a common offset of 160 on the residual stream through linear.bias (|row mean| / std >> 30 at block 0's LayerNorms: the pad-corrected
    variance of the chain kernels); three residual channels driven to |x| ~ 50 - 200 by the last block through the FFN2 / pointwise-2 /
    out-proj output rows; 5 % near-dead channels (conv weights x 1e-2) in the subsampler and every depthwise convolution, and BatchNorm statistics
    CALIBRATED - running mean / var = the batch statistics of the BN input over a calibration batch, stage by stage with the oracle (the
    subsampler shift absorbs the mel mean; dead channels get running_var ~ 1e-4 of the others: the bf16 BN folds)."""
    for key, shape, kind in P.param_specs(plan):
        g = _rng("trained/" + key, seed)
        a = sd[key]
        if kind == P.GAMMA:
            a[...] = np.clip(np.exp(0.5 * g.standard_normal(shape)), 0.05, 5.0)
        elif kind == P.BETA:
            a[...] = g.uniform(-1.0, 1.0, shape)
        elif kind == P.B:
            a[...] = g.uniform(-0.5, 0.5, shape)
        elif kind == P.UV:
            a[...] = g.uniform(-1.0, 1.0, shape)
        elif kind == P.W and len(shape) >= 2:
            rows = g.choice(shape[0], max(1, int(0.03 * shape[0])), replace=False)
            a[rows] *= np.float32(4.0)
    dead = lambda key, n: _rng("trained/dead/" + key, seed).choice(n, max(1, int(round(0.05 * n))), replace=False)
    for l in range(plan.sub_layers):
        k = "subsampling_module.layers.%d.0.weight" % l
        sd[k][dead(k, sd[k].shape[0])] *= np.float32(1e-2)
    for bp in plan.blocks:
        k = "blocks.%d.convolution_module.layers.4.weight" % bp.index
        sd[k][dead(k, bp.dim_expand)] *= np.float32(1e-2)
    sd["linear.bias"] += np.float32(160.0)
    lb = plan.blocks[-1]
    pb, de = "blocks.%d" % lb.index, lb.dim_expand
    for j, ch in enumerate(_rng("trained/outliers", seed).choice(de, 3, replace=False)):
        sign = np.float32(1.0 if j % 2 == 0 else -1.0)
        sd[pb + ".feed_forward_module2.layers.4.bias"][ch] += sign * np.float32(80.0)   # x 1/2 on the stream
        sd[pb + ".convolution_module.layers.7.bias"][ch] += sign * np.float32(40.0)
        sd[pb + ".convolution_module.layers.7.weight"][ch] *= np.float32(4.0)
        if lb.dim_model == de:
            sd[pb + ".multi_head_self_attention_module.mhsa.output_layer.bias"][ch] += sign * np.float32(30.0)
    _calibrate(plan, sd, seed)


def _calibrate(plan: EncoderPlan, sd: Dict[str, np.ndarray], seed: int, logit_target: float = 20.0) -> None:
    """Stage by stage in block order on a rectangular calibration batch (every frame valid): BatchNorm running statistics := the batch mean /
    (biased) variance of the BN input; Q / K weights and biases scaled by one factor per block so that the largest |logit| of the content term
    (Q + u) K / sqrt(d) reaches ``logit_target``.  Test data generation only: runs the float32 oracle (oracle/ref_encoder.py)."""
    import torch
    import torch.nn.functional as F
    from oracle import ref_encoder as R
    mel, lens = make_mel(2, plan.n_mels, 160, seed=seed ^ 0xCA1B)
    t = {k: torch.from_numpy(v) for k, v in sd.items()}          # views: updates below write through to sd
    with torch.no_grad():
        x = torch.from_numpy(mel).unsqueeze(1)
        for l in range(plan.sub_layers):
            p = "subsampling_module.layers.%d" % l
            h = F.conv2d(x, t[p + ".0.weight"], t[p + ".0.bias"], stride=2, padding=1)
            t[p + ".1.running_mean"][:] = h.mean(dim=(0, 2, 3))
            t[p + ".1.running_var"][:] = h.var(dim=(0, 2, 3), unbiased=False)
            h = F.batch_norm(h, t[p + ".1.running_mean"], t[p + ".1.running_var"], t[p + ".1.weight"], t[p + ".1.bias"], False, 0.0, R.BN_EPS)
            x = h * torch.sigmoid(h)
        b_, c_, f_, tt = x.shape
        x = F.linear(x.reshape(b_, c_ * f_, tt).transpose(1, 2), t["linear.weight"], t["linear.bias"])
        for bp in plan.blocks:
            pb = "blocks.%d" % bp.index
            mh = pb + ".multi_head_self_attention_module"
            xf = x + 0.5 * R.ffn(x, t, pb + ".feed_forward_module1")
            hn = F.layer_norm(xf, (bp.dim_model,), t[mh + ".norm.weight"], t[mh + ".norm.bias"], R.LN_EPS)
            q = F.linear(hn, t[mh + ".mhsa.query_layer.weight"], t[mh + ".mhsa.query_layer.bias"]) + t[mh + ".mhsa.u"]
            k = F.linear(hn, t[mh + ".mhsa.key_layer.weight"], t[mh + ".mhsa.key_layer.bias"])
            dh = bp.dim_model // bp.num_heads
            qh = q.reshape(b_, -1, bp.num_heads, dh).transpose(1, 2)
            kh = k.reshape(b_, -1, bp.num_heads, dh).transpose(1, 2)
            top = float((qh @ kh.transpose(2, 3)).abs().max()) / math.sqrt(bp.dim_head)
            s = math.sqrt(logit_target / max(top, 1e-6))
            for n in ("query_layer", "key_layer"):
                t[mh + ".mhsa.%s.weight" % n].mul_(s)
                t[mh + ".mhsa.%s.bias" % n].mul_(s)
            trace = {}
            R.conformer_block(x, None, t, bp, trace, plan)
            cm = pb + ".convolution_module"
            h = R.conv_module_pre_bn(trace[pb + ".x_mhsa"], t, cm, bp.kernel_size, bp.conv_stride, plan.causal)
            t[cm + ".layers.5.running_mean"][:] = h.mean(dim=(0, 2))
            t[cm + ".layers.5.running_var"][:] = h.var(dim=(0, 2), unbiased=False)
            x = R.conformer_block(x, None, t, bp, None, plan)


def make_stressed_state_dict(plan: EncoderPlan, seed: int, profile: str, vocab: int | None = None, prefix: str = "") -> Dict[str, np.ndarray]:
    """``make_state_dict`` followed by the changes of ``profile`` (``trained`` or ``boundary``; see ``_trained`` / ``_boundary``).  Deterministic:
    every random draw is key-seeded like ``make_tensor``'s, the calibration runs on a seeded mel batch.  ``make_state_dict`` itself is untouched
    (the golden vectors and the benchmark depend on it byte for byte)."""
    if profile not in STRESS_PROFILES:
        raise ValueError("profile must be one of %s" % (STRESS_PROFILES,))
    sd = make_state_dict(plan, seed, vocab)
    if profile == "trained":
        _trained(plan, sd, seed)
    else:
        _boundary(plan, sd)
    return {(prefix + k if not k.startswith("fc.") else k): v for k, v in sd.items()}
