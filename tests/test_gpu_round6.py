"""-m gpu tests added in round 6: the round-5 kernels against the ORACLE per stage at production widths,
the matrix-pipe depthwise convolution alone against the oracle's depthwise stage, short utterances of the plain Conformer configurations."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from efficientconformer_amd import ModelCTC, _lib, named_config, synth
from oracle import ref_encoder as R

pytestmark = pytest.mark.gpu


def _model(name, seed):
    cfg = named_config(name)
    m = ModelCTC.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, seed, cfg["tokenizer_params"]["vocab_size"], prefix="encoder.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    osd = {k[len("encoder."):] if k.startswith("encoder.") else k: v for k, v in sd.items()}
    return m.cuda(), osd


def _rel(got, ref):
    d = (got.double() - ref.double()).abs()
    scale = max(float(ref.abs().max()), 1.0)
    return float(d.max()) / scale, float(d.mean()) / scale


# ------------------------------------------------------------------ per-stage oracle traces at production widths
# Small: D = 120 / 168 / 240 -> chain_kernel<8,4,2>, chain_kernel<12,8,3>, chain3_kernel<16> (chain A), chain2_kernel<16> (chain B), dwconv_mfma_kernel<15> at
# 120 / 168 / 240 channels, relpos_attention2_kernel<96> (stage 0, d = 90) / <64> (d = 42, 60).  Medium: D = 180 / 256 / 360 -> <12,8,3>, chain3 / chain2 at the
# full width 256, the per-GEMM row-stationary kernels at 360, attention head widths 135 / 64 / 90.  Until round 5 these kernels saw the oracle only through the
# LayerNorm-ed encoder output of 15 blocks (0.06 max) or through each other (bit-identity with the older kernel).
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name,tm,lens", [("EfficientConformerCTCSmall", 700, [700, 561, 330]), ("EfficientConformerCTCMedium", 520, [520, 401, 263])])
def test_every_traced_stage_of_the_production_widths_vs_oracle(name, tm, lens, ragged):
    """The residual stream after FFN1 (= the output of chain A: pointwise-2 + residual + FFN2 + block LayerNorm + the next block's FFN1) and after the attention
    module (= chain B's out-projection + residual on top of the attention kernel's output) of EVERY block, the subsampling + Linear output and the encoder
    output against the oracle's trace, with the Tiny test's relative bounds (tests/test_gpu_encoder.py: 0.02 max / 0.003 mean of the tensor's magnitude).
    Rectangular batches: the oracle on the collated batch (pad frames live).  Ragged batches: the oracle on every utterance ALONE, rows mapped through the
    group-padded row space (an utterance's rows start at the sum of the previous utterances' frames rounded up to the block's attention group size).
    A mis-indexed pad column, a wrong chunk order or a head-span slip in one block shows up at that block, not 15 LayerNorms later."""
    m, sd = _model(name, 7)
    plan = m.encoder.plan
    mel, ln = synth.make_mel(len(lens), 80, tm, lens, seed=4321 + tm)
    m.encoder.ragged = ragged
    out, out_len, got = m.encoder.trace_forward_mel(torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda())
    assert "blocks.0.x_conv" not in got, "the fused chains are expected on this path (x_conv only exists in registers)"
    worst = {}
    if not ragged:
        trace = {}
        with torch.no_grad():
            ref, ref_len = R.encoder_from_mel(torch.from_numpy(mel), torch.from_numpy(ln), sd, plan, trace)
        assert out_len.cpu().tolist() == ref_len.tolist()
        worst["linear"] = _rel(got["linear"], trace["linear"].reshape(-1, trace["linear"].shape[-1]))
        for k in range(len(plan.blocks)):
            for tag in ("x_ffn1", "x_mhsa"):
                r = trace["blocks.%d.%s" % (k, tag)]
                worst["blocks.%d.%s" % (k, tag)] = _rel(got["blocks.%d.%s" % (k, tag)], r.reshape(-1, r.shape[-1]))
        worst["out"] = _rel(out.cpu(), ref)
    else:
        offs = {k: 0 for k in range(len(plan.blocks))}
        for b, l in enumerate(lens):
            trace = {}
            with torch.no_grad():
                ref, ref_len = R.encoder_from_mel(torch.from_numpy(mel[b:b + 1, :, :l]), torch.tensor([l]), sd, plan, trace)
            tb = int(ref_len[0])
            assert int(out_len[b]) == tb
            worst["out.%d" % b] = _rel(out[b, :tb].cpu(), ref[0])
            assert float(out[b, tb:].abs().sum()) == 0.0
            for k, bp in enumerate(plan.blocks):
                for tag in ("x_ffn1", "x_mhsa"):
                    r = trace["blocks.%d.%s" % (k, tag)][0]
                    g = got["blocks.%d.%s" % (k, tag)][offs[k]: offs[k] + r.shape[0]]
                    key = "blocks.%d.%s" % (k, tag)
                    w = _rel(g, r)
                    worst[key] = max(worst.get(key, (0.0, 0.0)), w)
                if k == 0:
                    r = trace["linear"][0]
                    worst["linear"] = max(worst.get("linear", (0.0, 0.0)), _rel(got["linear"][offs[0]: offs[0] + r.shape[0]], r))
                t_in = trace["blocks.%d.x_ffn1" % k].shape[1]
                offs[k] += (t_in + bp.group_size - 1) // bp.group_size * bp.group_size
    top = sorted(worst.items(), key=lambda kv: -kv[1][0])[:4]
    print("%s ragged=%s worst stages (max, mean relative): %s" % (name, ragged, [(k, "%.4f" % a, "%.5f" % b) for k, (a, b) in top]))
    for k, (mx, mean) in worst.items():
        assert mx < 0.02 and mean < 0.003, (k, mx, mean, top)


# ------------------------------------------------------------------ the matrix-pipe depthwise convolution alone against the oracle's depthwise stage
def _bf16_round(x: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


@pytest.mark.parametrize("ksize,channels,frames", [(15, 120, 257), (15, 168, 131), (15, 240, 66), (15, 256, 300), (31, 176, 140), (31, 512, 70), (7, 40, 50)])
@pytest.mark.parametrize("causal", [0, 1])
def test_depthwise_conv_kernels_alone_vs_the_oracle_depthwise_stage(ksize, channels, frames, causal):
    """dwconv_mfma_kernel (stride 1) and dwconv_kernel on the SAME bf16-exact inputs against the oracle's depthwise stage (oracle/ref_encoder.py conv_module:
    zero pre-padding, F.conv1d with groups = channels, BatchNorm(eval), Swish; reference modules.py:516-518, layers.py:97-101) evaluated in float64.
    The kernels fold the BatchNorm into the taps in fp32 and store bf16: the result must be the float64 value rounded to bf16, give or take one bf16 ulp where
    the fp32 sum (the matrix-pipe kernel: taps as bf16 hi + lo halves, 2^-17 of a tap) lands on the other side of a rounding boundary - i.e. the error against the
    UN-rounded float64 value stays below one bf16 ulp (2^-8 relative) plus 2e-5 absolute - the tap split's 2^-17 times the sum of |tap x| (~3), which is what is
    left of the relative accuracy where the 15 / 31 products cancel to a pre-activation near zero - and at least 95 % of the outputs are the correctly rounded value.  Round 5 tested the
    matrix-pipe kernel against the VALU kernel only (0.04 on the encoder output); a wrong tap, a shifted frame or a mis-padded channel tile fails this at once."""
    dlib = _lib.load_debug()
    rng = np.random.default_rng(100 * ksize + channels + causal)
    batch, ld = 3, (channels + 7) // 8 * 8
    g = np.zeros((batch, frames, ld), dtype=np.float32)
    g[:, :, :channels] = _bf16_round(rng.standard_normal((batch, frames, channels)) * 1.5)
    w = (rng.standard_normal((channels, 1, ksize)) / np.sqrt(ksize)).astype(np.float32)           # Conv1d(De, De, k, groups = De).weight
    cb = (0.02 * rng.standard_normal(channels)).astype(np.float32)
    gamma = (1.0 + 0.1 * rng.standard_normal(channels)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(channels)).astype(np.float32)
    mean = (0.2 * rng.standard_normal(channels)).astype(np.float32)
    var = rng.uniform(0.5, 1.5, channels).astype(np.float32)
    # oracle arithmetic in float64 on the same numbers
    h = torch.from_numpy(g[:, :, :channels]).double().transpose(1, 2)
    half = (ksize - 1) // 2
    h = F.pad(h, (ksize - 1, 0) if causal else (half, half))
    h = F.conv1d(h, torch.from_numpy(w).double(), torch.from_numpy(cb).double(), groups=channels)
    h = F.batch_norm(h, torch.from_numpy(mean).double(), torch.from_numpy(var).double(), torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(),
                     False, 0.0, R.BN_EPS)
    want = (h * torch.sigmoid(h)).transpose(1, 2).numpy()                                       # (B, T, C) float64
    # what finalize hands the kernels: BatchNorm folded into the taps / bias in fp32 (pack.hip; SURVEY.md 8a closed form)
    sc = (gamma / np.sqrt(var + np.float32(1e-5))).astype(np.float32)
    w_kc = np.ascontiguousarray((w[:, 0, :] * sc[:, None]).T.astype(np.float32))                 # [k][C]
    bias = (cb * sc + beta - mean * sc).astype(np.float32)
    gd = torch.from_numpy(g).to(torch.bfloat16).cuda()
    for use_mfma in (1, 0):
        out = torch.zeros(batch, frames, ld, dtype=torch.bfloat16, device="cuda")
        _lib.check(dlib.effconf_debug_dwconv(gd.data_ptr(), batch, frames, channels, ld, w_kc.ctypes.data_as(ctypes.c_void_p), bias.ctypes.data_as(ctypes.c_void_p),
                                             ksize, 1, use_mfma, causal, out.data_ptr(), None), "debug_dwconv", dlib)
        torch.cuda.synchronize()
        got = out.float().cpu().numpy()[:, :, :channels].astype(np.float64)
        ulp = np.abs(want) * 2.0 ** -8 + 2e-5
        err = np.abs(got - want)
        exact = float((got == _bf16_round(want).astype(np.float64)).mean())
        assert float((err / ulp).max()) < 1.0, (use_mfma, float((err / ulp).max()), np.unravel_index(np.argmax(err / ulp), err.shape))
        assert exact > 0.95, (use_mfma, exact)


# ------------------------------------------------------------------ short utterances of the plain Conformer configurations
@pytest.mark.parametrize("name", ["ConformerCTCSmall", "ConformerCTCLarge"])
def test_short_utterances_of_the_plain_conformer_configs_vs_oracle(name):
    """Utterances of 5 - 13 encoder frames (0.2 - 0.5 s) of the plain Conformer configurations (kernel size 31, two-layer subsampler, no grouping): few frames,
    LayerNorm-ed outputs, nothing averages the bf16 rounding over time - profiles/r5_35_dw_accuracy.txt measured mean |err| 0.0107 - 0.0109 (max 0.054) here, ON /
    over the 0.010 mean the other tests state.  The tolerance of this length class, stated where it is tested: max 0.08 / mean 0.014,
    ragged (every utterance alone) and rectangular (the collated batch); the label-exact mode on the same utterances stays at fp32 noise."""
    m, sd = _model(name, 3)
    plan = m.encoder.plan
    frames = [52, 44, 37, 30, 24, 20]                       # mel frames -> 13, 11, 10, 8, 6, 5 encoder frames after the 4x subsampler
    mel, ln = synth.make_mel(len(frames), 80, max(frames), frames, seed=77)
    mel_d, ln_d = torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda()
    with torch.no_grad():
        ref, ref_len = R.encoder_from_mel(torch.from_numpy(mel), torch.from_numpy(ln), sd, plan)
    out, out_len, _ = m.encoder.forward_mel(mel_d, ln_d)
    assert out_len.cpu().tolist() == ref_len.tolist()
    d = (out.cpu() - ref).abs()
    print("%s rectangular: max %.4f mean %.5f" % (name, float(d.max()), float(d.mean())))
    assert float(d.max()) < 0.08 and float(d.mean()) < 0.014
    m.encoder.ragged = True
    rag, rag_len, _ = m.encoder.forward_mel(mel_d, ln_d)
    worst_max, means = 0.0, []
    for b, l in enumerate(frames):
        with torch.no_grad():
            alone, alone_len = R.encoder_from_mel(torch.from_numpy(mel[b:b + 1, :, :l]), torch.tensor([l]), sd, plan)
        tb = int(alone_len[0])
        assert int(rag_len[b]) == tb
        e = (rag[b, :tb].cpu() - alone[0]).abs()
        worst_max = max(worst_max, float(e.max())); means.append(float(e.mean()))
    print("%s ragged: worst max %.4f, per-utterance mean %s" % (name, worst_max, ["%.4f" % v for v in means]))
    assert worst_max < 0.08 and max(means) < 0.014


# ------------------------------------------------------------------ the label-exact split mode on the fused kernels (csrc/sxf.hip): ragged, causal, streaming
import os

from test_gpu_round3 import _STREAM, _ragged_vs_alone, _stream_model

SPLIT_MAX, SPLIT_MEAN = 2e-4, 2e-5            # the label-exact modes' stated bound against the oracle / the reference goldens (measured ~5e-6 / 1e-6)


@pytest.mark.parametrize("gname", _STREAM)
def test_split_mode_streaming_and_causal_vs_reference_goldens(golden_dir, gname):
    """`causal` (causal relative tables attentions.py:506-529, 1243-1247; causal depthwise pre-padding layers.py:97-101) and finite
    left / right contexts (attentions.py:1377-1403) in the split mode, against the REFERENCE run with those settings (tools/make_goldens.py --only-streaming):
    encoder output within 2e-4 at every frame - pad frames included, whose fully masked rows follow the reference's uniform softmax - and the per-frame argmax
    identical wherever the reference's top-2 margin exceeds 1e-3.  Until round 5 the exact modes refused `causal` (test_exact_mode_rejects_streaming_contexts)."""
    g = np.load(os.path.join(golden_dir, gname))
    m, sd, small = _stream_model(gname, g)
    m.encoder.precision = "split"
    lens = g["mel_len"].tolist()
    mel, ln = synth.make_mel(len(lens), 80, max(lens), lens, seed=int(g["mel_seed"]))
    out, out_len, _ = m.encoder.forward_mel(torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda())
    assert out_len.cpu().tolist() == g["out_len"].tolist()
    ref = torch.from_numpy(g["out_rows"] if small else g["out"])
    got = out.cpu()[:, ::4] if small else out.cpu()
    d = (got - ref).abs()
    print("%s split: max %.2e mean %.2e" % (gname, float(d.max()), float(d.mean())))
    assert float(d.max()) < SPLIT_MAX and float(d.mean()) < SPLIT_MEAN
    if small:
        logits, _, _ = m._head(out, out_len, want_logits=True)
        am = logits.argmax(-1).cpu().numpy()
        valid = np.arange(am.shape[1])[None, :] < g["out_len"][:, None]
        safe = (g["margin"] > 1e-3) & valid
        assert safe.sum() > 20 and np.array_equal(am[safe], g["argmax"][safe])


@pytest.mark.parametrize("name,extra,nsub", [("Tiny", {}, 1), ("Tiny", {}, 3), ("Tiny", dict(causal=True), 2), ("Tiny", dict(left_context=20, right_context=4), 2),
                                             ("Tiny", dict(causal=True, left_context=6), 1), ("EfficientConformerCTCSmall", {}, 2), ("ConformerCTCSmall", {}, 2),
                                             ("EfficientConformerCTCMedium", {}, 1), ("EfficientConformerCTCSmall", dict(causal=True), 1)])
def test_split_mode_ragged_batch_equals_utterances_alone_and_the_oracle(name, extra, nsub):
    """ragged batches in the split mode.  Every utterance of a ragged forward is, bit for bit, the split-mode encoder's output for that
    utterance ALONE (B = 1, rectangular), and within 2e-4 / 2e-5 of the oracle run on it alone; one and several row ranges; grouped stages with T % 3 = 0, 1, 2;
    the two-layer subsampler (ConformerCTCSmall); head widths 18 .. 135 (Medium stage 0: the V^T-aliasing instance of the attention kernel); causal and
    finite contexts.  Reference: encoders.py:97-142 on a batch of one."""
    cfg = named_config(name)
    cfg["encoder_params"] = dict(cfg["encoder_params"], **extra)
    m = ModelCTC.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, 7, cfg["tokenizer_params"]["vocab_size"], prefix="encoder.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    osd = {k[len("encoder."):] if k.startswith("encoder.") else k: v for k, v in sd.items()}
    m.encoder.precision = "split"
    if name == "Tiny":
        lens = np.array([48000, 47840, 41000, 37000, 30160, 22000, 12000, 9000, 3000, 640, 300], dtype=np.int64)     # down to 2 mel frames
    else:
        lens = np.array([70000, 52345, 33000, 20000, 8000], dtype=np.int64)
    audio = torch.from_numpy(synth.make_audio(lens, seed=4))
    _ragged_vs_alone(m.cuda(), osd, audio, lens, nsub, tol=(SPLIT_MAX, SPLIT_MEAN))


# ------------------------------------------------------------------ split-precision row-local chains (csrc/sxf_chain.hip)
@pytest.mark.parametrize("name,tm,lens", [("Tiny", 333, [333, 250, 97, 12]), ("EfficientConformerCTCSmall", 420, [420, 333, 201]),
                                          ("EfficientConformerCTCMedium", 300, [300, 177]), ("ConformerCTCSmall", 260, [260, 121]),
                                          ("ConformerCTCMedium", 180, [180, 77]), ("EfficientConformerTransducerSmall", 300, [300, 222]),
                                          ("ConformerTransducerSmall", 200, [200, 133, 61])])
@pytest.mark.parametrize("ragged", [False, True])
def test_split_chains_vs_per_module_kernels_and_the_oracle(name, tm, lens, ragged):
    """sxf_chain.hip: out-proj + residual + LayerNorm + pointwise-1 + GLU as one kernel, pointwise-2 + residual + FFN2 + block LayerNorm + the next block's FFN1 +
    attention pre-norm + Q | K | V as another (blocks.py:119-137, modules.py:385-395, 511-522, attentions.py:651-653, 716).  The split mode with the chains (the
    default) against (i) the same mode on the per-module kernels (`split_chain = 0`: LayerNorm, split GEMM, GLU kernels and the FFN-only form of chain A - a
    different summation order, so a few 1e-6, not bit equality; that leg shares the FFN body with the chains, so also with `split_ffn = 0` beside it: LayerNorm +
    split GEMMs, code the chains share nothing with, to the same bound) and (ii) the oracle within the split mode's stated 2e-4 / 2e-5; rectangular batches with pad frames (the Q / K / V and
    attention-output row remap) and ragged ones; every width a shipped configuration <= 256 has (24 .. 256: 100 / 140 / 200, 120 / 168 / 240, 144, 176, 180 / 256)
    incl. the stage transitions (D != De) and both subsampler forms."""
    m, sd = _model(name, 11)
    plan = m.encoder.plan
    m.encoder.precision = "split"
    mel, ln = synth.make_mel(len(lens), 80, tm, lens, seed=99 + tm)
    mel_d, ln_d = torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda()
    m.encoder.ragged = ragged
    out, out_len, _ = m.encoder.forward_mel(mel_d, ln_d)
    m.encoder.set_option("split_chain", 0)
    base, base_len, _ = m.encoder.forward_mel(mel_d, ln_d)
    m.encoder.set_option("split_ffn", 0)
    gemms, gemms_len, _ = m.encoder.forward_mel(mel_d, ln_d)
    m.encoder.set_option("split_ffn", 1)
    m.encoder.set_option("split_chain", 1)
    assert torch.equal(out_len, base_len) and torch.equal(out_len, gemms_len)
    d = (out - base).abs()
    print("%s ragged=%s chains vs per-module kernels: max %.2e mean %.2e" % (name, ragged, float(d.max()), float(d.mean())))
    assert float(d.max()) < 1e-4 and float(d.mean()) < 1e-5
    d = (out - gemms).abs()
    print("%s ragged=%s chains vs LayerNorm + split GEMMs: max %.2e mean %.2e" % (name, ragged, float(d.max()), float(d.mean())))
    assert float(d.max()) < 1e-4 and float(d.mean()) < 1e-5
    if ragged:
        for b, l in enumerate(lens):
            with torch.no_grad():
                ref, ref_len = R.encoder_from_mel(torch.from_numpy(mel[b:b + 1, :, :l]), torch.tensor([l]), sd, plan)
            tb = int(ref_len[0])
            assert int(out_len[b]) == tb
            e = (out[b, :tb].cpu() - ref[0]).abs()
            assert float(e.max()) < SPLIT_MAX and float(e.mean()) < SPLIT_MEAN, (b, float(e.max()), float(e.mean()))
    else:
        with torch.no_grad():
            ref, ref_len = R.encoder_from_mel(torch.from_numpy(mel), torch.from_numpy(ln), sd, plan)
        assert out_len.cpu().tolist() == ref_len.tolist()
        e = (out.cpu() - ref).abs()
        print("%s rectangular vs oracle: max %.2e mean %.2e" % (name, float(e.max()), float(e.mean())))
        assert float(e.max()) < SPLIT_MAX and float(e.mean()) < SPLIT_MEAN


# ------------------------------------------------------------------ a forward reads no workspace byte it did not write
@pytest.mark.parametrize("precision,chain", [("bf16", 1), ("split", 1), ("split", 0), ("fp32", 1)])
@pytest.mark.parametrize("name,tm,lens", [("Tiny", 100, [100, 77, 52]), ("Tiny", 333, [333, 250, 97, 12]), ("EfficientConformerCTCSmall", 420, [420, 333, 201]),
                                          ("ConformerCTCSmall", 260, [260, 180, 33])])
def test_forward_on_a_poisoned_fresh_workspace_is_bit_identical(monkeypatch, name, tm, lens, precision, chain):
    """The caller owns the workspace and may hand over ANY bytes (a recycled allocation of another dtype holds NaN / Inf patterns with probability ~1/32 per
    half word).  EFFCONF_POISON_WORKSPACE (_native.py `workspace`) fills every fresh workspace with a byte: 255 = NaN patterns in fp32 / bf16 / fp16.  A kernel
    that reads a byte nobody wrote - and scales it by a zero weight or a zero mask instead of selecting - turns that into a NaN in a VALID output: found on the
    split GEMM's A-tile tail at K < 32 (the last row read the bytes behind the buffer and multiplied them by 0), fixed by a select.  Every mode, rectangular and
    ragged, the traced (per-module) forward too: output bit-identical to the forward on a zero-filled workspace, and finite."""
    outs = {}
    for fill in ("0", "255"):
        monkeypatch.setenv("EFFCONF_POISON_WORKSPACE", fill)
        m, _ = _model(name, 7)                                   # a new handle: fresh workspaces, filled with `fill`
        enc = m.encoder
        enc.precision = precision
        if precision == "split":
            enc.set_option("split_chain", chain)
        mel, ln = synth.make_mel(len(lens), 80, tm, lens, seed=77 + tm)
        mel_d, ln_d = torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda()
        for ragged in ([False, True] if precision != "fp32" else [False]):       # the fp32 mode takes rectangular batches only
            enc.ragged = ragged
            o, ol, _ = enc.forward_mel(mel_d, ln_d, x_len_host=ln if ragged else None)
            outs[(fill, ragged)] = (o.clone(), ol.clone())
            enc._ws.clear()                                      # the next forward allocates (and fills) again
    for (fill, ragged), (o, ol) in outs.items():
        assert bool(torch.isfinite(o).all()), (fill, ragged)
        if fill == "255":
            z, zl = outs[("0", ragged)]
            assert torch.equal(ol, zl) and torch.equal(o, z), (ragged, float((o - z).abs().max()))


# ------------------------------------------------------------------ split-precision front end as one kernel (csrc/sxf_sub.hip)
@pytest.mark.parametrize("name,tm,lens", [("Tiny", 333, [333, 250, 97, 12, 3]), ("EfficientConformerCTCSmall", 700, [700, 433, 258, 57]),
                                          ("EfficientConformerCTCMedium", 300, [300, 177]), ("EfficientConformerCTCLarge", 260, [260, 121]),
                                          ("EfficientConformerTransducerSmall", 300, [300, 222, 9])])
@pytest.mark.parametrize("ragged", [False, True])
def test_split_front_end_kernel_vs_conv_gemm_kernels_and_the_oracle(name, tm, lens, ragged):
    """sxf_sub.hip: Conv2d(1, C, 3, stride 2) + BatchNorm + Swish + flatten + Linear as ONE kernel whose (frames, C F') activation never leaves the registers
    (modules.py:232-249, encoders.py:113-116), ragged batches on the frames that exist.  Against (i) the same mode on the per-module front end
    (`split_sublin = 0`: fp32 VALU convolution, split GEMM, row gather - another summation order: a few 1e-6) and (ii) the oracle within the split mode's stated
    bound; rectangular batches (pad frames live) and ragged ones (every utterance against the oracle on it ALONE: the convolution's zero padding starts behind
    its own last mel frame; the group-padding rows behind it are zeros); every instance (1 / 4 / 6 / 12 output tiles: D0 = 24, 100 / 120, 180, 360) and channel
    counts that are not a multiple of 32 (24, 100, 120, 180, 360); utterances shorter than one tile and a tile count > 1 (700 frames -> 350 rows)."""
    m, sd = _model(name, 13)
    plan = m.encoder.plan
    m.encoder.precision = "split"
    mel, ln = synth.make_mel(len(lens), 80, tm, lens, seed=5 + tm)
    mel_d, ln_d = torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda()
    m.encoder.ragged = ragged
    out, out_len, _ = m.encoder.forward_mel(mel_d, ln_d)
    m.encoder.set_option("split_sublin", 0)
    base, base_len, _ = m.encoder.forward_mel(mel_d, ln_d)
    m.encoder.set_option("split_sublin", 1)
    assert torch.equal(out_len, base_len)
    d = (out - base).abs()
    print("%s ragged=%s fused front end vs conv + GEMM kernels: max %.2e mean %.2e" % (name, ragged, float(d.max()), float(d.mean())))
    assert float(d.max()) < 1e-4 and float(d.mean()) < 1e-5
    if ragged:
        for b, l in enumerate(lens):
            with torch.no_grad():
                ref, ref_len = R.encoder_from_mel(torch.from_numpy(mel[b:b + 1, :, :l]), torch.tensor([l]), sd, plan)
            tb = int(ref_len[0])
            assert int(out_len[b]) == tb
            e = (out[b, :tb].cpu() - ref[0]).abs()
            assert float(e.max()) < SPLIT_MAX and float(e.mean()) < SPLIT_MEAN, (b, float(e.max()), float(e.mean()))
    else:
        with torch.no_grad():
            ref, ref_len = R.encoder_from_mel(torch.from_numpy(mel), torch.from_numpy(ln), sd, plan)
        assert out_len.cpu().tolist() == ref_len.tolist()
        e = (out.cpu() - ref).abs()
        print("%s rectangular vs oracle: max %.2e mean %.2e" % (name, float(e.max()), float(e.mean())))
        assert float(e.max()) < SPLIT_MAX and float(e.mean()) < SPLIT_MEAN


# ------------------------------------------------------------------ bf16 front end chunked over (output frequency, 32 channels) (csrc/sublinear3.hip)
@pytest.mark.parametrize("name,fuse,tm,lens", [("EfficientConformerCTCSmall", 3, 700, [700, 433, 258, 57]), ("EfficientConformerCTCMedium", 2, 420, [420, 333, 9]),
                                               ("EfficientConformerCTCLarge", 2, 300, [300, 121]), ("EfficientConformerTransducerSmall", 3, 300, [300, 222, 9])])
def test_chunked_bf16_front_end_vs_oracle_linear_stage_and_ragged_equals_alone(name, fuse, tm, lens):
    """sublinear3.hip (Conv2d 3 x 3 stride 2 + BatchNorm + Swish + flatten + Linear as one bf16 kernel, any channel count: the default for front ends wider than 128
    channels / columns - Medium's 180, Large's 360 - and option fuse_subsample = 3 elsewhere; modules.py:232-249, encoders.py:113-116): (i) its output - the traced
    "linear" stage of a rectangular batch - against the oracle's at the Tiny test's relative bounds (0.02 max / 0.003 mean of the tensor's magnitude; the conv in split
    bf16, the Swish-ed activation rounded to bf16 once, fp32 accumulation), pad frames live; (ii) encoder output within the bf16 path's stated tolerance; (iii) a
    ragged batch bit-identical to every utterance alone (the convolution's zero padding starts behind the utterance's own last mel frame; tiles and group-padding
    rows behind a short utterance's end; 700 frames -> 3 row tiles)."""
    m, sd = _model(name, 17)
    enc, plan = m.encoder, m.encoder.plan
    enc.set_option("fuse_subsample", fuse)
    mel, ln = synth.make_mel(len(lens), 80, tm, lens, seed=31 + tm)
    mel_d, ln_d = torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda()
    trace = {}
    with torch.no_grad():
        ref, ref_len = R.encoder_from_mel(torch.from_numpy(mel), torch.from_numpy(ln), sd, plan, trace)
    out, out_len, got = enc.trace_forward_mel(mel_d, ln_d)
    assert "subsample" not in got, "the fused front end is expected on this path (the activation only exists in registers)"
    assert out_len.cpu().tolist() == ref_len.tolist()
    mx, mean = _rel(got["linear"], trace["linear"].reshape(-1, trace["linear"].shape[-1]))
    print("%s linear stage vs oracle: max %.4f mean %.5f (relative)" % (name, mx, mean))
    assert mx < 0.02 and mean < 0.003
    e = (out.cpu() - ref).abs()
    assert float(e.max()) < 0.06 and float(e.mean()) < 0.010
    enc.ragged = True
    rag, rag_len, _ = enc.forward_mel(mel_d, ln_d, x_len_host=ln)
    enc.ragged = False
    for b, l in enumerate(lens):
        alone, alone_len, _ = enc.forward_mel(mel_d[b:b + 1, :, :l].contiguous(), ln_d[b:b + 1].contiguous())
        tb = int(alone_len[0])
        assert int(rag_len[b]) == tb and torch.equal(rag[b, :tb], alone[0, :tb]), (b, float((rag[b, :tb] - alone[0, :tb]).abs().max()))
        assert not bool(rag[b, tb:].any())


# ------------------------------------------------------------------ the bench's configuration reproduces itself
@pytest.mark.parametrize("precision,iters", [("bf16", 300), ("split", 60)])
def test_ragged_forward_on_three_streams_reproduces_itself_bit_for_bit(precision, iters):
    """EfficientConformerCTCSmall, B = 256 LibriSpeech-shaped utterances sorted by length, ragged, 3 row ranges on 3 streams (bench.py's configuration): every forward
    equals the first one bit for bit.  With the weight-ring waits of rounds 3 - 6 (global stores counted into the allowed vmcnt although a
    store can retire before an older LDS-DMA; removed) 23 % of these forwards carried one or two utterances - the last of a row range - perturbed by ~1e-2
    (profiles/r6_108_ring_wait_fix.txt); no parity test could see that, a repetition test does."""
    m, _ = _model("EfficientConformerCTCSmall", 5)
    enc = m.encoder
    enc.precision = precision
    B = 256
    lens = synth.libri_lengths(B, seed=1234)[:B]
    lens = lens[np.argsort(-lens, kind="stable")].copy()
    audio = torch.from_numpy(synth.make_audio(lens, seed=7)).cuda()
    ln = torch.from_numpy(lens).cuda()
    enc.ragged, enc.sub_batches = True, 3
    ref, ref_len, _ = enc(audio, ln, x_len_host=lens)
    assert bool(torch.isfinite(ref).all())
    bad = []
    for it in range(iters):
        got, got_len, _ = enc(audio, ln, x_len_host=lens)
        torch.cuda.synchronize()
        if not (torch.equal(got, ref) and torch.equal(got_len, ref_len)):
            d = got != ref
            bad.append((it, d.flatten(1).any(1).nonzero().flatten().tolist()[:4], float((got - ref).abs().max())))
    assert not bad, (len(bad), bad[:5])
