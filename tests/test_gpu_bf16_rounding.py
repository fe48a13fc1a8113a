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
always), one causal and one streaming configuration at 700 frames and three at 1001 (key blocks skipped from the left, tiles of live and dead rows, 64-wide heads under a band), synthetic and `trained` weights.  The Q / K / V and GLU route (folded or per-module) leaves no trace
entry: it is asserted through the data (the other route's reference must fit worse; tests/bf16_parity.py).

The front end and block 0's first FFN (tests/bf16_parity.py check_front, run by every case of both tests): where separate kernels write the subsampler's
activation (`subsample`, `subsample1`) the convolution(s) and the Linear each from their own traced input - `conv` / `conv2`: the bf16 statistics plus element-wise
one bf16 ulp + 2 K 2^-23 (sum |w| |p| + |b|) 1.1, `linear`: the float32 statistics plus the out-projection's summation bound; on the fused routes one stage
mel -> `linear` (`front`) whose noise is the float32 runs of ref_bf16.front_end with the float32 convolution and, on sublinear2.hip / sublinear3.hip, with their split
formula as well; `ffn1_0`: blocks.0.x_ffn1 from the traced `linear`.  The route is asserted (`subsample` present or absent; the convolution's form through the data).
The second test walks the routes (Tiny, EfficientConformerCTC-Small with fuse_subsample 0 / 1 / 2 / 3, Medium with and without sub3_auto, Large with the fused kernel
and with conv.hip + GEMM, the two-layer subsampler of ConformerCTC-Small / -Large; rectangular and ragged), the frame-tile edges (1, 2, 31, 32, 33, 127, 128, 129,
257 output frames at both parities of the mel length; a 1-frame and a 3-frame utterance next to a 700-frame one) and the inputs (synth.silence_floor_mel on
`trained` weights, whose calibrated BatchNorm folds to large taps and biases).  Its first run found every route inside every bound.

What the first runs of the block stages found (measured before the fixes; all inside the un-rounded 0.02 / 0.003 tests): (1) `trained` profile, block 0 (stream mean 160,
deviation 1): 8 % of the Q / K / V outputs and 2.4 % of the GLU outputs not the correctly rounded number, 2.1 - 2.6 x the share bound - the chains' LayerNorm
variance summed the pad columns' (0 - mean)^2 and subtracted pad * mean^2 afterwards (chain.hip ln_stats; fixed by masking the pad pieces).  (2) `trained`
profile, EfficientConformerCTC-Small: the matrix-pipe depthwise kernel up to 1.84 x the element-wise 2^-8 |r| + 2e-5 (bf16 hi + lo tap pairs on folded taps of
12 - 800 in L2 norm; blocks with |taps|_2 > 6 in some channel now run the kernel's three-plane instantiation, which the two `trained` cases of
EfficientConformerCTC-Small keep under test).  The figures after the fixes are in profiles/bf16_rounding_parity.txt."""
import numpy as np
import pytest
import torch

from efficientconformer_amd import ModelCTC, named_config, synth
from bf16_parity import _Report, check_front, check_trace, front_route
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
_L3 = [1001, 778, 97]
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
    # 167 grouped rows under a band of 21 at stage 0, 251 rows under 32 at stage 1: the third query tile starts at key block 1 (kbeg > 0 in attention2.hip); the
    # rectangular case's 97-frame utterance leaves query tiles that mix live and dead rows (whole band in the padding: uniform over all key groups)
    ("EfficientConformerCTCSmall", 1001, _L3, True, {}, {"left_context": 64, "right_context": 8}, "synthetic"),
    ("EfficientConformerCTCSmall", 1001, _L3, False, {}, {"causal": True, "left_context": 64}, "synthetic"),
    # 64-wide heads at stages 1 and 2 (Small's widths are 90 / 42 / 60): 126 rows under a band of 32 - rows of the second query tile whose first visited key
    # block holds none of their keys, NaN before NEG_BIG of attention2.hip became a power of two
    ("EfficientConformerCTCMedium", 1001, _L3, True, {}, {"left_context": 64, "right_context": 8}, "synthetic"),
]


def _id(c):
    long = ["T%d" % c[1]] if c[2] is _L3 else []          # the ids of the earlier cases stay as they were
    return "-".join([c[0], "ragged" if c[3] else "rect"] + long + ["%s=%d" % kv for kv in sorted(c[4].items())] + ["%s=%s" % kv for kv in sorted(c[5].items())] + [c[6]])


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
    check_front(got, plan, sd, mel, ln, tm, ragged, front_route(plan, opts, ragged), rep)
    rep.finish()


# ------------------------------------------------------------------ the front end's routes and edges
def _odd(t1):       # mel frames that give t1 output frames with the last patch's third column behind the end / inside
    return 2 * t1 - 1


def _even(t1):
    return 2 * t1


_EDGE_T1 = (257, 129, 128, 127, 33, 32, 31, 2, 1)
_EDGE_A = [_even(t) if i % 2 == 0 else _odd(t) for i, t in enumerate(_EDGE_T1)]          # 514, 257, 256, 253, 66, 63, 62, 3, 1
_EDGE_B = [_odd(t) if i % 2 == 0 else _even(t) for i, t in enumerate(_EDGE_T1)]          # 513, 258, 255, 254, 65, 64, 61, 4, 2
_SHORT = [1400, 5, 1]                                                                    # 700 frames next to a 3-frame and a 1-frame utterance
_M4 = [520, 401, 263, 97]
_SM, _MD, _LG = "EfficientConformerCTCSmall", "EfficientConformerCTCMedium", "EfficientConformerCTCLarge"
# name, mel frames, lengths, ragged, options, weight profile, mel ("mel": synth.make_mel, "floor": synth.silence_floor_mel)
FRONT_CASES = (
    # every route, rectangular and ragged, at a width it ships on (Tiny: 24 channels, a partly filled 32-channel block)
    [("Tiny", 1201, _T12, rg, o, "synthetic", "mel") for rg in (False, True) for o in ({}, {"fuse_subsample": 3}, {"fuse_subsample": 1}, {"fuse_subsample": 0})]
    + [(_SM, 700, _L4, rg, {"fuse_subsample": f}, "synthetic", "mel") for rg in (False, True) for f in (0, 1, 2, 3)]
    + [(_MD, 520, _M4, rg, o, "synthetic", "mel") for rg in (False, True) for o in ({}, {"sub3_auto": 0})]
    + [(_LG, 520, _M4, rg, o, "synthetic", "mel") for rg in (False, True) for o in ({}, {"fuse_subsample": 0})]
    + [(n, 520, _M4, rg, {}, "synthetic", "mel") for rg in (False, True) for n in ("ConformerCTCSmall", "ConformerCTCLarge")]
    # frame-tile edges: 1, 2, 31, 32, 33, 127, 128, 129 and 257 output frames per utterance, both parities of the mel length at every one
    + [(_SM, max(e), e, True, {"fuse_subsample": f}, "synthetic", "mel") for e in (_EDGE_A, _EDGE_B) for f in (0, 2, 3)]
    + [("Tiny", max(e), e, True, {}, "synthetic", "mel") for e in (_EDGE_A, _EDGE_B)]
    + [(_LG, max(e), e, True, o, "synthetic", "mel") for e in (_EDGE_A, _EDGE_B) for o in ({}, {"fuse_subsample": 0})]
    + [("ConformerCTCSmall", max(e), e, True, {}, "synthetic", "mel") for e in (_EDGE_A, _EDGE_B)]
    + [(_SM, tm, [tm, tm - 7, 5], False, {"fuse_subsample": f}, "synthetic", "mel") for tm in (63, 65, 66, 257, 513) for f in (1, 2)]
    + [(n, 1400, _SHORT, True, o, "synthetic", "mel") for n, o in (("Tiny", {}), (_SM, {}), (_SM, {"fuse_subsample": 3}), (_SM, {"fuse_subsample": 0}), (_LG, {}),
                                                                 ("ConformerCTCSmall", {}))]
    # inputs: silent runs at the log floor and loud frames; `trained` weights (calibrated BatchNorm: large folded taps and biases)
    + [(_SM, 700, _L4, rg, {"fuse_subsample": f}, "trained", "floor") for rg in (False, True) for f in (0, 1, 2, 3)]
    + [("Tiny", 700, _L4, True, {}, "trained", "floor"), (_MD, 520, _M4, False, {}, "trained", "floor"), (_LG, 520, _M4, True, {}, "trained", "floor"),
       (_LG, 520, _M4, True, {"fuse_subsample": 0}, "trained", "floor"), ("ConformerCTCSmall", 520, _M4, False, {}, "trained", "floor"),
       ("ConformerCTCSmall", 520, _M4, True, {}, "trained", "floor"), (_SM, 700, _L4, False, {}, "synthetic", "floor")]
)


def _fid(c):
    return "-".join([c[0], "ragged" if c[3] else "rect", "T%d" % c[1], "L%d" % len(c[2])] + ["%s=%d" % kv for kv in sorted(c[4].items())] + [c[5], c[6]])


@pytest.mark.parametrize("case", FRONT_CASES, ids=_fid)
def test_front_end_routes_and_edges_vs_the_rounding_aware_reference(case):
    """The front end (every route of run_subsample_linear and of forward_core's ragged branch, asserted) and block 0's first FFN against
    ref_bf16.front_* / ffn (tests/bf16_parity.py check_front); on Tiny's twelve-utterance batch, where it is cheap, the block stages as well."""
    name, tm, lens, ragged, opts, profile, kind = case
    torch.set_num_threads(16)
    m, sd = _model(name, profile, {})
    enc, plan = m.encoder, m.encoder.plan
    for k, v in opts.items():
        enc.set_option(k, v)
    enc.ragged = ragged
    mel, ln = (synth.make_mel if kind == "mel" else synth.silence_floor_mel)(len(lens), plan.n_mels, tm, lens, seed=5021 + tm)
    out, out_len, got = enc.trace_forward_mel(torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda(), arena_bytes=1 << 29)
    if name == "Tiny" and len(lens) == len(_T12):          # the block stages' share statistics need the rows of the twelve-utterance batch (see _T12)
        rep = check_trace(got, out_len.cpu().tolist(), plan, sd, ln, tm, ragged, 1, _fid(case))
    else:
        rep = _Report(_fid(case))
    check_front(got, plan, sd, mel, ln, tm, ragged, front_route(plan, opts, ragged), rep)
    rep.finish()
