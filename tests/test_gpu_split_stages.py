"""-m gpu: every split-mode kernel (precision = "split") against its float64 reference, stage by stage, teacher forced.

One forward through ``trace_forward_mel`` per case.  With option ``trace_fused = 1`` the trace keeps the fused kernels an untraced forward runs
(sxf_sublin_kernel, sxc_a_kernel, sxc_b_kernel) and records what they write to memory - with split_chain = 0 beside it, the feed-forward modules alone on the
FFN-only form of sxc_a_kernel between per-module kernels; without it - and with split_chain = split_sublin = split_ffn = 0 - the per-module kernels (split.hip sx_gemm_kernel, LayerNorm, sxf_glu_kernel, the fp32 convolutions) run.  Every stage is recomputed on the CPU FROM THE GPU'S OWN
TRACED INPUT of that stage (tests/split_parity.py), in float64 - ref_bf16's stage functions with every rounding off: the split mode's contract is "no rounding
anywhere" - and, as the noise model, by oracle/ref_split.py's split_runs: torch's float32 run, the kernels' float32 LayerNorm / sigmoid / exp formulas with the
hardware functions moved by 0, +-1, +-2 ulps, and the emulated fp16 operand pairs (h toward zero, l to nearest, a_h w_h + a_h w_l + a_l w_h in float32).

Bounds: rel(gpu, r64).max <= 4 x the worst noise run, .mean <= 8 x the mean of the noise runs, neither below sqrt(K) 2^-23 of the magnitude; element-wise on
the out-projection, conv_res / pointwise-2 (per-module route) and the front Linear: 2 K 2^-23 (|a| |w|^T + |x| + |b|) + the split term of ref_split.split_term;
attention, element-wise: its sum_j p_ij |v_j| analogue (tests/split_parity.py).  The noise is computed here from the reference, never from the kernel.
The route is asserted from the trace: ``x_conv`` / ``subsample`` absent on the fused route and present on the per-module one, ``out`` absent exactly where a
head is merged into chain A's tail.  Chunk-padding rows of q / k / v / att_o are never written and are ignored.  Each case prints statistic / bound per stage
(profiles/split_parity.txt: the first passing run; DESIGN.md section 2d: what is and is not seen)."""
import pytest
import torch

from efficientconformer_amd import ModelCTC, named_config, synth
from bf16_parity import _Report
from split_parity import check_split_front, check_split_trace, split_route
from test_gpu_bf16_rounding import _EDGE_A, _EDGE_B, _SHORT

pytestmark = pytest.mark.gpu

PER_MODULE = {"split_chain": 0, "split_sublin": 0, "split_ffn": 0}
FUSED = {"trace_fused": 1}
FFN_ONLY = {"trace_fused": 1, "split_chain": 0}      # every FFN as the FFN-only form of sxc_a_kernel (in place: FFN1; to another buffer, with the block norm: FFN2)
_SM, _T4 = "EfficientConformerCTCSmall", [333, 250, 97, 12]
# name, mel frames, lengths, ragged, options, encoder_params overrides, weight profile, mel kind, block stages too
CASES = (
    [("Tiny", 333, _T4, rg, o, {}, "synthetic", "mel", True) for rg in (False, True) for o in (FUSED, PER_MODULE)]
    + [(_SM, 420, [420, 333, 201], rg, FUSED, {}, "synthetic", "mel", True) for rg in (False, True)]
    + [("Tiny", 333, _T4, rg, FFN_ONLY, {}, "synthetic", "mel", True) for rg in (False, True)]               # widths 24 / 32 / 48, a last workgroup with clamped rows
    + [(_SM, 420, [420, 333, 201], rg, FFN_ONLY, {}, "synthetic", "mel", True) for rg in (False, True)]      # widths 120 / 168 / 240
    + [("EfficientConformerCTCMedium", 300, [300, 177], True, FUSED, {}, "synthetic", "mel", True),          # chains at 180 / 256, per-module kernels at 360; head width 135
       ("ConformerCTCSmall", 260, [260, 121], False, FUSED, {}, "synthetic", "mel", True),                  # width 176, two-layer subsampler, kernel 31
       ("EfficientConformerTransducerSmall", 300, [300, 222], True, FUSED, {}, "synthetic", "mel", True),   # widths 100 / 140 / 200
       ("EfficientConformerCTCLarge", 300, [300, 121], False, FUSED, {}, "synthetic", "mel", True)]         # per-module kernels at 360 / 512 / 720
    + [(n, max(e), e, True, FUSED, {}, "synthetic", "mel", True) for n in (_SM, "Tiny") for e in (_EDGE_A, _EDGE_B)]
    + [(_SM, 1400, _SHORT, True, FUSED, {}, "synthetic", "mel", True),
       (_SM, 420, [420, 333, 201], False, FUSED, {"causal": True}, "synthetic", "mel", True),
       (_SM, 420, [420, 333, 201], True, FUSED, {"left_context": 64, "right_context": 8}, "synthetic", "mel", True),
       # 167 / 251 grouped rows under bands of 21 / 32: sxf_attention_kernel skips key blocks from the left (jt_lo > 0); rectangular: tiles of live and dead rows
       (_SM, 1001, [1001, 778, 97], True, FUSED, {"left_context": 64, "right_context": 8}, "synthetic", "mel", True),
       (_SM, 1001, [1001, 778, 97], False, FUSED, {"causal": True, "left_context": 64}, "synthetic", "mel", True)]
    + [(_SM, 420, [420, 333, 201], rg, FUSED, {}, "trained", "mel", True) for rg in (False, True)]
    + [(_SM, 420, [420, 333, 201], rg, o, {}, "trained", "floor", False) for rg in (False, True) for o in (FUSED, PER_MODULE)]
)


def _id(c):
    return "-".join([c[0], "ragged" if c[3] else "rect", "T%d" % c[1], "L%d" % len(c[2])] + ["%s=%d" % kv for kv in sorted(c[4].items())]
                    + ["%s=%s" % kv for kv in sorted(c[5].items())] + [c[6], c[7]])


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
    m.encoder.precision = "split"
    osd = {k[len("encoder."):] if k.startswith("encoder.") else k: v for k, v in sd.items()}
    return m.cuda(), osd


def _traced(case):
    name, tm, lens, ragged, opts, extra, profile, kind, _ = case
    torch.set_num_threads(16)
    m, sd = _model(name, profile, extra)
    enc = m.encoder
    for k, v in opts.items():
        enc.set_option(k, v)
    enc.ragged = ragged
    mel, ln = (synth.make_mel if kind == "mel" else synth.silence_floor_mel)(len(lens), enc.plan.n_mels, tm, lens, seed=5021 + tm)
    args = (torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda())
    out, out_len, got = enc.trace_forward_mel(*args, arena_bytes=1 << 29)
    return enc, sd, mel, ln, args, out, out_len, got


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_split_stage_vs_the_float64_reference(case):
    name, tm, lens, ragged, opts, extra, profile, kind, blocks = case
    enc, sd, mel, ln, _, out, out_len, got = _traced(case)
    plan = enc.plan
    route = split_route(plan, opts)
    if blocks:
        rep = check_split_trace(got, out_len.cpu().tolist(), plan, sd, ln, tm, ragged, route, _id(case))
    else:
        rep = _Report(_id(case))
    check_split_front(got, plan, sd, mel, ln, tm, ragged, route, rep)
    rep.finish()


@pytest.mark.parametrize("ragged", [False, True])
def test_a_traced_fused_forward_is_the_untraced_forward_bit_for_bit(ragged):
    """trace_fused = 1 changes nothing but the copies into the trace arena: the output equals the untraced forward's bit for bit (and, with the option
    back at 0, a trace selects the per-module kernels again: ``x_conv`` is back in the trace)."""
    case = (_SM, 420, [420, 333, 201], ragged, FUSED, {}, "synthetic", "mel", True)
    enc, sd, mel, ln, args, out, out_len, got = _traced(case)
    plain, plain_len, _ = enc.forward_mel(*args)
    assert torch.equal(out_len, plain_len) and torch.equal(out, plain)
    assert "blocks.0.x_conv" not in got and "subsample" not in got and "blocks.0.glu" in got and "blocks.0.e" in got
    enc.set_option("trace_fused", 0)
    _, _, got0 = enc.trace_forward_mel(*args, arena_bytes=1 << 29)
    assert "blocks.0.x_conv" in got0 and "subsample" in got0 and "blocks.0.glu" in got0 and "blocks.0.e" in got0


@pytest.mark.parametrize("ragged", [False, True], ids=["rect", "ragged"])
@pytest.mark.parametrize("name,tm,lens", [("Tiny", 333, _T4), (_SM, 420, [420, 333, 201])], ids=["Tiny", _SM])
def test_the_ffn_only_form_equals_the_chain_head_bit_for_bit(name, tm, lens, ragged):
    """Block 0's first FFN as chain A's head form (trace_fused = 1) and as the FFN-only form of the same kernel (split_chain = 0 beside it): the same inlined
    functions on the same ``linear`` rows and the same image, so ``blocks.0.x_ffn1`` is bit-identical.  ``linear`` first: a mismatch then points at the kernel."""
    enc, sd, mel, ln, args, out, out_len, head = _traced((name, tm, lens, ragged, FUSED, {}, "synthetic", "mel", True))
    enc.set_option("split_chain", 0)
    _, _, alone = enc.trace_forward_mel(*args, arena_bytes=1 << 29)
    assert "blocks.0.x_conv" not in head and "blocks.0.x_conv" in alone                # the routes: chains | per-module kernels around the FFN-only form
    assert torch.equal(head["linear"], alone["linear"])
    assert torch.equal(head["blocks.0.x_ffn1"], alone["blocks.0.x_ffn1"])
