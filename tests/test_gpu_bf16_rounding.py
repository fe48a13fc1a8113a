"""-m gpu: every bf16 kernel against the rounding-aware reference (oracle/ref_bf16.py), stage by stage, teacher forced.

One forward through ``trace_forward_mel``; then per block and stage the reference is computed FROM THE GPU'S OWN TRACED INPUTS of that stage
(no error is carried from one stage to the next) in float64 and, as the noise model, in float32 arithmetic, and the GPU's traced output of the
stage is held to

* float32 outputs: rel(gpu, r64).max <= 4 rel(r32, r64).max and rel(gpu, r64).mean <= 8 rel(r32, r64).mean, neither bound below
  sqrt(K) 2^-23 of the magnitude (K = the stage's longest contraction);
* bf16 outputs: the same on the stored values (noise = q(r32) against the un-rounded r64) plus the share of elements equal to q(r64) at least
  1 - 4 (1 - share(q(r32) == q(r64))) (attention: factor 2, r32 with P rounded to bf16);
* out-projection, element-wise: |gpu - r64| <= 2 K 2^-23 (|a| |w|^T + |x| + |b|);  depthwise, element-wise: |gpu - r64| < 2^-8 |r64| + 2e-5 and
  at least 95 % of the elements equal to q(r64);  attention, element-wise: |gpu - r64| <= 2^-7 sum_j p_ij |v_j| + 2e-5.

The factors are fixed; the noise they multiply is computed here from the reference, never from the kernel: over torch's float32 run and five runs on
the kernels' own float32 formulas with the hardware functions moved by 0, +-1, +-2 ulps (ref_bf16.f32_runs says why a single float32 run is no estimate
of its own expectation: the share is a counting statistic driven by a handful of operand ties per tensor).  Every valid row of every utterance
counts; chunk-padding rows of qu / k / v are compared with their contract (q(u), zeros); group-padding rows of a ragged batch's row space are
excluded by the row map and their count is asserted.  Each case prints the worst statistic / noise ratio of every stage
(profiles/bf16_rounding_parity.txt holds those lines of the first passing run).

Routes: the fused chains (folded LayerNorm) wherever the stage width allows - asserted per block through `x_conv` being absent from the trace - in their
2-wave and 8-wave forms (chain_small_m = 0 / 1 << 30, or the row count), chain3 / chain2 against chain.hip at padded width 256 (chain_pair = 5 / 0), the
per-module kernels (fuse_chain = 0 and Medium's D = 360 stage), attention.hip and the VALU depthwise kernel (attention_v2 = 0, dwconv_mfma = 0; strided blocks
always), one causal and one streaming configuration, synthetic and `trained` weights.  The Q / K / V and GLU route (folded or per-module) leaves no trace
entry: it is asserted through the data (the other route's reference must fit worse; tests/bf16_parity.py).

What the first runs found (measured before the fixes; all inside the un-rounded 0.02 / 0.003 tests): (1) `trained` profile, block 0 (stream mean 160,
deviation 1): 8 % of the Q / K / V outputs and 2.4 % of the GLU outputs not the correctly rounded number, 2.1 - 2.6 x the share bound - the chains' LayerNorm
variance summed the pad columns' (0 - mean)^2 and subtracted pad * mean^2 afterwards (chain.hip ln_stats; fixed by masking the pad pieces).  (2) `trained`
profile, EfficientConformerCTC-Small: the matrix-pipe depthwise kernel up to 1.84 x the element-wise 2^-8 |r| + 2e-5 (bf16 hi + lo tap pairs on folded taps of
12 - 800 in L2 norm; blocks with |taps|_2 > 6 in some channel now run the kernel's three-plane instantiation, which the two `trained` cases of
EfficientConformerCTC-Small keep under test).  The figures after the fixes are in profiles/bf16_rounding_parity.txt."""
import numpy as np
import pytest
import torch

from efficientconformer_amd import ModelCTC, named_config, synth
from bf16_parity import check_trace
from oracle import ref_bf16 as Q

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


def _model(name, profile, extra):
    cfg = named_config(name)
    if extra:
        cfg["encoder_params"] = dict(cfg["encoder_params"], **extra)
    m = ModelCTC.from_config(cfg)
    vocab = cfg["tokenizer_params"]["vocab_size"]
    if profile == "synthetic":
        sd = synth.make_state_dict(m.encoder.plan, 7, vocab, prefix="encoder.")
    else:
        sd = synth.make_stressed_state_dict(m.encoder.plan, 7, profile, vocab, prefix="encoder.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    osd = {k[len("encoder."):] if k.startswith("encoder.") else k: v for k, v in sd.items()}
    return m.cuda(), osd


# name, mel frames, lengths, ragged, options, encoder_params overrides, weight profile
_L4 = [700, 561, 330, 97]
# Tiny's tensors are 24 .. 48 columns wide: the share of correctly rounded outputs is a counting statistic (one flipped tie of a LayerNorm-ed operand moves
# 10 - 40 % of a row's outputs), and at a few hundred rows the float32 runs expect less than one such event per tensor - nothing a factor can be applied to.
# Twelve utterances give 7212 rows at stage 0 (more than chain_small_m = 4096: the 8-wave shapes by row count), 3606 and 1206 at the later stages.
_T12 = [1201, 1100, 1003, 950, 801, 700, 561, 330, 250, 97, 33, 12]
CASES = [
    ("Tiny", 1201, _T12, False, {}, {}, "synthetic"),
    ("Tiny", 1201, _T12, True, {}, {}, "synthetic"),
    ("Tiny", 1201, _T12, False, {"chain_small_m": 0}, {}, "synthetic"),
    ("Tiny", 1201, _T12, True, {"chain_small_m": 1 << 30}, {}, "synthetic"),
    ("Tiny", 1201, _T12, False, {"attention_v2": 0, "dwconv_mfma": 0}, {}, "trained"),
    ("EfficientConformerCTCSmall", 700, _L4, False, {}, {}, "synthetic"),
    ("EfficientConformerCTCSmall", 700, _L4, True, {}, {}, "synthetic"),
    ("EfficientConformerCTCSmall", 700, _L4, False, {"chain_small_m": 0}, {}, "synthetic"),
    ("EfficientConformerCTCSmall", 700, _L4, True, {"chain_small_m": 0, "chain_pair": 0}, {}, "synthetic"),
    ("EfficientConformerCTCSmall", 700, _L4, True, {"chain_small_m": 0}, {}, "trained"),
    ("EfficientConformerCTCSmall", 700, _L4, False, {"chain_pair": 0}, {}, "trained"),
    ("EfficientConformerCTCSmall", 700, _L4, False, {"fuse_chain": 0}, {}, "synthetic"),
    ("EfficientConformerCTCSmall", 700, _L4, False, {"attention_v2": 0, "dwconv_mfma": 0}, {}, "synthetic"),
    ("EfficientConformerCTCMedium", 520, [520, 401, 263, 97], False, {}, {}, "synthetic"),
    ("EfficientConformerCTCMedium", 520, [520, 401, 263, 97], True, {"chain_small_m": 0}, {}, "synthetic"),
    ("ConformerCTCSmall", 520, [520, 401, 263, 97], False, {}, {}, "synthetic"),
    ("ConformerCTCSmall", 520, [520, 401, 263, 97], True, {"chain_small_m": 0}, {}, "synthetic"),
    ("EfficientConformerCTCSmall", 700, _L4, False, {}, {"causal": True}, "synthetic"),
    ("EfficientConformerCTCSmall", 700, _L4, True, {}, {"left_context": 64, "right_context": 8}, "synthetic"),
]


def _id(c):
    return "-".join([c[0], "ragged" if c[3] else "rect"] + ["%s=%d" % kv for kv in sorted(c[4].items())] + ["%s=%s" % kv for kv in sorted(c[5].items())] + [c[6]])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_bf16_stage_vs_the_rounding_aware_reference(case):
    name, tm, lens, ragged, opts, extra, profile = case
    torch.set_num_threads(16)
    m, sd = _model(name, profile, extra)
    enc, plan = m.encoder, m.encoder.plan
    for k, v in opts.items():
        enc.set_option(k, v)
    enc.ragged = ragged
    mel, ln = synth.make_mel(len(lens), plan.n_mels, tm, lens, seed=5021 + tm)
    out, out_len, got = enc.trace_forward_mel(torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda(), arena_bytes=1 << 29)
    rep = check_trace(got, out_len.cpu().tolist(), plan, sd, ln, tm, ragged, opts.get("fuse_chain", 1), _id(case))
    rep.finish()
