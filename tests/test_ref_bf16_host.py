"""CPU tests of the rounding-aware reference of the bf16 path (oracle/ref_bf16.py): it is the oracle plus roundings and nothing else, its
roundings are a plausible model of a path that passes the un-rounded oracle tests, and the bound tests/test_gpu_bf16_rounding.py holds the
kernels to sees the faults it was built for."""
import numpy as np
import pytest
import torch

from efficientconformer_amd import ModelCTC, named_config, synth
from bf16_parity import check_trace
from oracle import ref_bf16 as Q
from oracle import ref_encoder as R

F64, F32 = torch.float64, torch.float32
BF16_MAX, BF16_MEAN = 0.02, 0.003          # the un-rounded oracle bound of tests/test_gpu_weight_stats.py, test_gpu_round6.py, test_gpu_encoder.py


def _setup(name, tm, lens, profile="synthetic"):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cfg = named_config(name)
    plan = ModelCTC.from_config(cfg).encoder.plan
    vocab = cfg["tokenizer_params"]["vocab_size"]
    sd = synth.make_state_dict(plan, 7, vocab) if profile == "synthetic" else synth.make_stressed_state_dict(plan, 7, profile, vocab)
    mel, ln = synth.make_mel(len(lens), plan.n_mels, tm, lens, seed=5021 + tm)
    return plan, sd, torch.from_numpy(mel), torch.from_numpy(ln)


def _lens_after_subsampling(plan, ln):
    for _ in range(plan.sub_layers):
        ln = torch.div(ln - 1, 2, rounding_mode="floor") + 1
    return ln


@pytest.mark.parametrize("name,tm,lens", [("Tiny", 333, [333, 250, 97, 12]), ("EfficientConformerCTCSmall", 300, [300, 211, 97])])
def test_stages_without_roundings_chained_are_the_float64_oracle(name, tm, lens):
    """Every q replaced by the identity: the stage functions of ref_bf16 chained reproduce ref_encoder.encoder_from_mel(dtype = float64) to float64
    rounding, on the output and on every traced residual-stream point - the new reference is the old one plus roundings, nothing else."""
    plan, sd, mel, ln = _setup(name, tm, lens)
    want = {}
    with torch.no_grad():
        ref, _ = R.encoder_from_mel(mel, ln, sd, plan, want, dtype=F64)
        got = {}
        out = Q.encoder_from_linear(want["linear"], _lens_after_subsampling(plan, ln), sd, plan, F64, rnd=Q.ident, trace=got)
    assert Q.rel(out, ref)[0] < 1e-11, Q.rel(out, ref)
    for k in range(len(plan.blocks)):
        for tag in ("x_ffn1", "x_mhsa", "x_conv", "out"):
            key = "blocks.%d.%s" % (k, tag)
            assert Q.rel(got[key], want[key])[0] < 1e-11, (key, Q.rel(got[key], want[key]))


@pytest.mark.parametrize("folded", [True, False])
@pytest.mark.parametrize("name,tm,lens", [("Tiny", 333, [333, 250, 97, 12]), ("EfficientConformerCTCSmall", 300, [300, 211, 97])])
def test_stages_with_roundings_chained_stay_inside_the_unrounded_oracle_bound(name, tm, lens, folded):
    """Roundings on, chained over the whole encoder (no teacher forcing): inside 0.02 max / 0.003 mean of the magnitude against the plain float64
    oracle at every residual-stream point and at the output - the rounding points are a plausible model of a path that passes today's tests."""
    plan, sd, mel, ln = _setup(name, tm, lens)
    want, got = {}, {}
    with torch.no_grad():
        ref, _ = R.encoder_from_mel(mel, ln, sd, plan, want, dtype=F64)
        out = Q.encoder_from_linear(want["linear"], _lens_after_subsampling(plan, ln), sd, plan, F64, folded=folded, trace=got)
    worst = [Q.rel(out, ref)] + [Q.rel(got["blocks.%d.%s" % (k, t)], want["blocks.%d.%s" % (k, t)]) for k in range(len(plan.blocks)) for t in ("x_ffn1", "x_mhsa")]
    mx, mean = max(w[0] for w in worst), max(w[1] for w in worst)
    print("%s folded=%s: rounded chain vs float64 oracle, worst point max %.4f mean %.5f" % (name, folded, mx, mean))
    assert mx < BF16_MAX and mean < BF16_MEAN, (mx, mean)


def _flat_trace(tr, plan):
    """The (B, rows, columns) trace of encoder_from_linear as the rectangular debug trace of the bf16 path lays it out: (B * rows, columns),
    bf16-stored entries as bf16 numbers, x_conv / out only where the kernels' trace has them (never on the fused route; out: last block)."""
    got = {}
    last = len(plan.blocks) - 1
    for key, v in tr.items():
        tag = key.rsplit(".", 1)[1]
        if tag == "x_conv" or (tag == "out" and not key.startswith("blocks.%d." % last)):
            continue
        got[key] = v.float().reshape(-1, v.shape[-1]).clone()
    return got


@pytest.mark.parametrize("name,tm,lens", [("Tiny", 333, [333, 250, 97, 12]), ("EfficientConformerCTCSmall", 300, [300, 211, 97])])
def test_trace_checker_accepts_the_float32_reference_and_rejects_one_wrong_stage(name, tm, lens):
    """The checker the GPU test runs (tests/bf16_parity.py check_trace), fed a trace made on the CPU by the float32-arithmetic reference: every stage of every
    block inside its bound.  The same trace with ONE stage of one block faulted (depthwise taps one frame late; a K-slot swap in W2 of FFN2) -
    the later stages computed consistently from the faulted values, as a kernel bug would leave them - fails at that block and stage and at no other."""
    plan, sd, mel, ln = _setup(name, tm, lens)
    with torch.no_grad():
        want = {}
        R.encoder_from_mel(mel, ln, sd, plan, want)
        lens1 = _lens_after_subsampling(plan, ln)
        out_len = lens1.clone()
        for bp in plan.blocks:
            if bp.conv_stride > 1:
                out_len = torch.div(out_len - 1, bp.conv_stride, rounding_mode="floor") + 1
        tr = {}
        Q.encoder_from_linear(want["linear"], lens1, sd, plan, F32, trace=tr)
        rep = check_trace(_flat_trace(tr, plan), out_len.tolist(), plan, sd, ln.tolist(), tm, False, 1, name + " float32 reference")
        rep.finish()
        kb = len(plan.blocks) // 2
        for stage, kw, seen in ((("depthwise", dict(shift=1), "dw")), ("chain_a", dict(fault=_kswap), "chainA")):
            tr = {}
            Q.encoder_from_linear(want["linear"], lens1, sd, plan, F32, trace=tr, faults={(kb, stage): kw})
            rep = check_trace(_flat_trace(tr, plan), out_len.tolist(), plan, sd, ln.tolist(), tm, False, 1, name + " fault " + stage)
            assert rep.fails and all(f.startswith("block %d %s " % (kb, seen)) for f in rep.fails), rep.fails[:4]


# ------------------------------------------------------------------ sensitivity: what the bound of the GPU test sees
def _kswap(name, v):        # two hidden units of one 16-group meet each other's W2 column (a K-permutation slip)
    if name == "product":
        h, w2, _ = v
        w = w2.clone()
        w[:, [5, 9]] = w2[:, [9, 5]]
        return h @ w.T


def _stale_slab(name, v):   # the last 64 rows read one 32-hidden-unit slab of W2 from the previous chunk (the weight-ring race's signature)
    if name == "product":
        h, w2, _ = v
        w = w2.clone()
        w[:, 64:96] = w2[:, 32:64]
        out = h @ w2.T
        out[-64:] = h[-64:] @ w.T
        return out


def _trunc(name, v):        # bf16 by truncation instead of round-to-nearest on the hidden activations
    if name == "hidden":
        return (v.float().view(torch.int32) & -65536).view(torch.float32).to(v.dtype)


def _half_after(name, v):   # control: 1/2 applied after instead of before the rounding of W2 - exact, must not differ
    if name == "product":
        h, _, raw = v
        return h @ (0.5 * Q.q(raw)).T


def _padvar(sd, k):         # block LayerNorm's variance over the padded width without the pad-column correction
    def hook(name, x):
        if name == "ln_out":
            d = x.shape[-1]
            dp = (d + 31) // 32 * 32
            mu = x.mean(-1, keepdim=True)
            var = (((x - mu) ** 2).sum(-1, keepdim=True) + (dp - d) * mu * mu) / d
            g, b = (torch.from_numpy(np.asarray(sd["blocks.%d.norm.%s" % (k, n)])).to(x.dtype) for n in ("weight", "bias"))
            return (x - mu) * torch.rsqrt(var + R.LN_EPS) * g + b
    return hook


def _over(r):
    return max(v for s, v in r.items() if not s.startswith(("noise", "single")))


# Faults the bound cannot see somewhere: (stage, fault, block) -> listed with the measured ratio instead of asserted.  The dropped pad term changes
# the variance by (DP - D) mean^2 / D, so what it does depends on the row means of the block's stream, not on the width alone: on these weights and
# inputs it is 0.73 x the bound in block 1 (D = 120 padded to 128) and 0.40 x in block 6 (168 -> 192), but 34 x in block 4 (168) and 2.7 x in block 12
# (240 -> 256).
UNDETECTABLE = {("chainA", "variance pad term dropped", 1), ("chainA", "variance pad term dropped", 6)}


def test_the_bound_sees_every_injected_fault_and_passes_reference_and_controls():
    """EfficientConformerCTC-Small, one block per stage width (D = 120, 168, 240) and the strided transition block 4: every stage's inputs from a
    float32-reference trace (the stand-in for the GPU's), each injected fault applied to the float32-arithmetic reference of ONE stage, the
    result put through the statistics of the GPU test (ref_bf16.stage_ratios and its element-wise conditions) with the bound computed from the
    un-faulted references.  Every fault exceeds the bound (ratio > 1) except where UNDETECTABLE lists it, with its measured ratio printed;
    the un-faulted float32 reference and the exact control stay inside (ratio <= 1).  qv built from the un-rounded Q + v is a control WITH
    effect: it removes a rounding the kernel has.  Measured: the bound does NOT see it - 0.20 - 0.23 of the max bound, 0.12 of the mean bound, 0.12 - 0.24 of
    the share bound, 0.50 of the envelope, the same as the un-faulted reference; its ratios are printed, and it is asserted only to stay inside the envelope."""
    plan, sd, mel, ln = _setup("EfficientConformerCTCSmall", 420, [420, 333, 97])
    rows = []
    with torch.no_grad():
        want, tr = {}, {}
        R.encoder_from_mel(mel, ln, sd, plan, want)
        lens = _lens_after_subsampling(plan, ln)
        Q.encoder_from_linear(want["linear"], lens, sd, plan, F32, trace=tr)
        nb = len(plan.blocks)
        for k, bp in enumerate(plan.blocks):
            if k in (1, 4, 6, 12):
                p, D, De = "blocks.%d." % k, bp.dim_model, bp.dim_expand
                flat = lambda z: z.reshape(-1, z.shape[-1])
                # ---- chain A
                xm, dw = tr[p + "x_mhsa"], flat(tr[p + "dw"])
                nbp = plan.blocks[k + 1] if k + 1 < nb else None
                res = [flat(Q.conv_res(xm, sd, bp, dt)) for dt in (F64, F32)]
                r64 = Q.chain_a(res[0], dw, sd, bp, nbp, F64, True)["x_ffn1"]
                r32 = [d["x_ffn1"] for d in Q.f32_runs(lambda: Q.chain_a(res[1], dw, sd, bp, nbp, F32, True))]
                kch = max(bp.dim_ffn2, nbp.dim_ffn1)
                for nme, hook in (("none (float32 reference)", None), ("control: 1/2 after rounding W2", _half_after), ("K-slot swap in a 16-group of W2", _kswap),
                                  ("stale 32-unit W2 slab, last 64 rows", _stale_slab), ("hidden truncated to bf16", _trunc), ("variance pad term dropped", _padvar(sd, k))):
                    f = Q.chain_a(res[1], dw, sd, bp, nbp, F32, True, fault=hook)["x_ffn1"]
                    rows.append(("chainA", k, nme, De, _over(Q.stage_ratios(f, r64, r32, kch, False))))
                # ---- depthwise
                g = tr[p + "glu"]
                d64, d32 = Q.depthwise(g, sd, bp, F64), Q.f32_runs(lambda: Q.depthwise(g, sd, bp, F32))
                for nme, sh in (("none (float32 reference)", 0), ("taps one frame late", 1)):
                    f = Q.q(Q.depthwise(g, sd, bp, F32, shift=sh))
                    r = Q.stage_ratios(f, d64, d32, bp.kernel_size, True, share_factor=0.0)
                    r["ulp"] = float(((f.double() - d64).abs() / (2.0 ** -8 * d64.abs() + 2e-5)).max())
                    r["miss"] = (1.0 - float((f.double() == Q.q(d64)).double().mean())) / 0.05
                    rows.append(("dw", k, nme, De, _over(r)))
                # ---- positional rows and attention
                t = tr[p + "x_ffn1"].shape[1]
                tp = tr[p + "qu"].shape[1]
                e64, e32 = Q.pos_e(tp, sd, bp, F64), Q.pos_e(tp, sd, bp, F32)
                for nme, sh in (("none (float32 reference)", 0), ("positional rows shifted by one", 1)):
                    f = Q.q(Q.pos_e(tp, sd, bp, F32, shift=sh))
                    rows.append(("pos", k, nme, D, _over(Q.stage_ratios(f, e64, e32, D, True))))
                ops = (tr[p + "qu"], tr[p + "k"], tr[p + "v"])
                e = tr[p + "e"]
                o64, env = Q.attention(*ops, e, lens, t, sd, bp, F64)
                o32, _ = Q.attention(*ops, e, lens, t, sd, bp, F32, round_p=True)
                kmax = max(bp.dim_head, tp // bp.group_size)
                for nme, kw, e_in in (("none (float32 reference, P rounded)", dict(round_p=True), e), ("positional rows shifted by one", {}, Q.q(Q.pos_e(tp, sd, bp, F32, shift=1))),
                                      ("key mask off by one group", dict(key_shift=1), e), ("control with effect: qv from un-rounded Q + v", dict(exact_qv=True), e)):
                    f = Q.q(Q.attention(*ops, e_in, lens, t, sd, bp, F32, **kw)[0])
                    r = Q.stage_ratios(f, o64, o32, kmax, True, share_factor=2.0)
                    envr = float(((f.double() - o64).abs() / (2.0 ** -7 * env + 2e-5)).max())
                    if kw.get("exact_qv"):
                        rows.append(("attention", k, nme + " [envelope only]", D, envr))
                        print("attention D %d, qv without its rounding: ratios to the bound %s" % (D, {s: "%.3g" % v for s, v in r.items()}))
                        continue
                    r["envelope"] = envr
                    rows.append(("attention", k, nme, D, _over(r)))
            if bp.conv_stride > 1:
                lens = torch.div(lens - 1, bp.conv_stride, rounding_mode="floor") + 1
    bad = []
    for stage, blk, nme, width, ratio in rows:
        inside = nme.startswith("none") or nme.startswith("control")
        listed = (stage, nme, blk) in UNDETECTABLE
        print("%-9s block %2d width %3d  %-48s ratio to the bound %10.3g  %s" % (stage, blk, width, nme, ratio, "must stay inside" if inside else ("NOT DETECTABLE here (listed)" if listed else "must exceed")))
        if inside and not ratio <= 1.0:
            bad.append((stage, blk, nme, width, ratio))
        if not inside and not listed and not ratio > 1.0:
            bad.append((stage, blk, nme, width, ratio))
    assert not bad, bad


# ------------------------------------------------------------------ the front end (ref_bf16.front_*) and block 0's first FFN
from bf16_parity import _Report, check_front, chain_route          # noqa: E402


@pytest.mark.parametrize("name,tm,lens", [("Tiny", 333, [333, 250, 97, 12]), ("EfficientConformerCTCSmall", 201, [201, 120, 3]),
                                          ("ConformerCTCSmall", 150, [150, 97, 6])])
def test_front_end_without_roundings_is_the_float64_oracle(name, tm, lens):
    """rnd = ident, float64: front_end is ref_encoder's subsampler + Linear, and front_end + encoder_from_linear is ref_encoder.encoder_from_mel, to
    float64 rounding, on one-layer and two-layer subsamplers.  Rectangular: the whole batch.  With lengths: the contract pads at the utterance's own
    length, so every utterance's own frames equal the oracle run on that utterance alone, cut to its length."""
    plan, sd, mel, ln = _setup(name, tm, lens)
    with torch.no_grad():
        want = {}
        ref, _ = R.encoder_from_mel(mel, ln, sd, plan, want, dtype=F64)
        x = Q.front_end(mel, None, sd, plan, F64, rnd=Q.ident)
        assert Q.rel(x, want["linear"])[0] < 1e-12, Q.rel(x, want["linear"])
        out = Q.encoder_from_linear(x, _lens_after_subsampling(plan, ln), sd, plan, F64, rnd=Q.ident)
        assert Q.rel(out, ref)[0] < 1e-11, Q.rel(out, ref)
        xl = Q.front_end(mel, ln, sd, plan, F64, rnd=Q.ident)
        for b, n in enumerate(ln.tolist()):
            alone = {}
            ref_b, _ = R.encoder_from_mel(mel[b:b + 1, :, :n], None, sd, plan, alone, dtype=F64)
            t1 = alone["linear"].shape[1]
            assert t1 == int(_lens_after_subsampling(plan, ln)[b])
            assert Q.rel(xl[b:b + 1, :t1], alone["linear"])[0] < 1e-12, (b, Q.rel(xl[b:b + 1, :t1], alone["linear"]))
            out_b = Q.encoder_from_linear(xl[b:b + 1, :t1], None, sd, plan, F64, rnd=Q.ident)
            assert Q.rel(out_b, ref_b)[0] < 1e-11, (b, Q.rel(out_b, ref_b))


def _trunc16(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def _standin(mel, mlen, sd, plan, form, fold, fault=None, traced=False):
    """A CPU stand-in of a correct front-end kernel + chain head in float32 arithmetic with the kernels' summation orders, not the noise runs': the
    convolution tap by tap on the accumulator that starts at the bias (conv.hip) or, ``form = "split"``, three products per tap slot with the bias in
    slot 9 (sublinear2.hip / sublinear3.hip); the Linear one output frequency after the other (the fused kernels' K order).  ``fault``: one of the
    injected faults of FRONT_FAULTS.  Returns the trace check_front reads (rectangular layout; ``subsample`` if ``traced``)."""
    assert plan.sub_layers == 1
    mel = mel.float()
    B, F, tm = mel.shape
    if fault == "patch one mel frame late":
        mel = torch.cat([mel[:, :, 1:], torch.zeros(B, F, 1)], 2)
    x = Q.mask_time(mel, None if fault == "time padding at the batch's last frame" else mlen)
    w, sc, bias = Q.bn_fold2d(sd, 0, F32, eps=0.0 if fault == "BatchNorm folded without eps" else R.BN_EPS)
    w9 = (w * sc[:, None, None, None]).reshape(-1, 9)
    if fault == "folded bias missing from tap slot 9":
        bias = torch.zeros_like(bias)
    C, F1, T1 = w9.shape[0], F // 2, (tm - 1) // 2 + 1
    xp = torch.nn.functional.pad(x, (1, 2, 1, 2))
    tap = lambda i, j: xp[:, i: i + 2 * F1: 2, j: j + 2 * T1: 2][:, None]                   # (B, 1, F1, T1)
    if form == "fp32":
        acc = bias[None, :, None, None].expand(B, C, F1, T1).clone()
        for j in range(9):
            acc = torch.addcmul(acc, w9[None, :, j, None, None], tap(j // 3, j % 3))
    else:
        whi, wlo = Q.split_hi_lo(torch.cat([w9, bias[:, None]], 1))
        if fault == "lo tap plane dropped":
            whi, wlo = Q.q(torch.cat([w9, bias[:, None]], 1)), torch.zeros_like(wlo)
        acc = torch.zeros(B, C, F1, T1)
        for j in reversed(range(10)):
            p = tap(j // 3, j % 3) if j < 9 else torch.ones(B, 1, F1, T1)
            phi, plo = Q.split_hi_lo(p)
            cw = lambda v: v[None, :, j, None, None]
            acc = acc + (cw(whi) * phi + (cw(whi) * plo + cw(wlo) * phi))
    act = Q.swish(acc)
    act = _trunc16(act) if fault == "activation truncated to bf16" else Q.q(act)
    wq = Q.q(torch.from_numpy(np.asarray(sd["linear.weight"])).float()).reshape(-1, C, F1).clone()        # (D0, C, F1)
    if fault == "K-slot swap in one 16-group":
        wq[:, [5, 9], 3] = wq[:, [9, 5], 3].clone()
    if fault == "stale 32-channel weight chunk":
        c0 = 32 if C > 32 else 0
        wq[:, c0: c0 + 32, 7] = wq[:, c0: c0 + 32, 6].clone()
    rows = act.permute(0, 3, 1, 2).reshape(B * T1, C, F1)
    if fault == "(c, f) order transposed in one channel block":
        cb = min(C, 32)
        rows = rows.clone()
        rows[:, :cb] = rows[:, :cb].clone().reshape(-1, F1, cb).transpose(1, 2)
    y = torch.from_numpy(np.asarray(sd["linear.bias"])).float()[None, :].expand(B * T1, -1).clone()
    for f in range(F1):
        y = y + rows[:, :, f] @ wq[:, :, f].T
    got = {"linear": y}
    if traced:
        got["subsample"] = rows.reshape(B * T1, C * F1)
    with Q.hardware_like(1):
        got["blocks.0.x_ffn1"] = Q.ffn(y, sd, "blocks.0.feed_forward_module1", F32, fold != (fault == "FFN1 on the wrong LayerNorm route"))
    return got


def _ragged_layout(got, lens1, t1, g):
    """The rectangular stand-in trace as the ragged row space lays it out: every utterance's own frames, then rows up to the group size (``subsample``: zeros; else a copy of a live row: finite)."""
    out = {}
    for k, v in got.items():
        v = v.reshape(len(lens1), t1, -1)
        pad = lambda b: torch.zeros_like(v[b, :1]) if k == "subsample" else v[b, :1]
        out[k] = torch.cat([torch.cat([v[b, :n], pad(b).expand((n + g - 1) // g * g - n, -1)]) for b, n in enumerate(lens1)])
    return out


FRONT_FAULTS = ("K-slot swap in one 16-group", "stale 32-channel weight chunk", "(c, f) order transposed in one channel block", "lo tap plane dropped",
                "folded bias missing from tap slot 9", "activation truncated to bf16", "patch one mel frame late", "time padding at the batch's last frame",
                "BatchNorm folded without eps", "FFN1 on the wrong LayerNorm route")
# (fault, convolution form, weight profile) the bound does not see, with the measured ratio printed by the test and recorded in DESIGN.md section 2b.
# The eps changes a folded tap by 1e-5 / (2 var): 5e-6 of it on the synthetic weights (var ~ 1).  The split convolution's own dropped lo lo term is up to
# 2^-14 = 6e-5 of a product, so on the routes whose noise model holds the split runs the fault is below the noise itself (0.24 - 0.25 x the bound, the
# correct stand-in's own figure; no margin over the fp32 runs separates them either: the fault is at 40 - 62 x their mean noise, the correct split
# stand-in at 48 - 76 x).  On the `trained` profile (calibrated BatchNorm, small variances) it is 1.7 x the bound, on the fp32 routes 2.2 - 11 x.
FRONT_UNSEEN = {("BatchNorm folded without eps", "split", "synthetic")}


def _front_over(rep):
    return max([v for (s, st), (v, _) in rep.worst.items() if not st.startswith(("noise", "single"))] + [0.0])


@pytest.mark.parametrize("profile", ["synthetic", "trained"])
@pytest.mark.parametrize("name,tm,lens", [("Tiny", 259, [259, 130, 5, 1]), ("EfficientConformerCTCSmall", 259, [259, 130, 5])])
def test_check_front_passes_stand_ins_and_sees_the_injected_faults(name, tm, lens, profile):
    """check_front (the checker of the GPU test) on CPU stand-ins of the three kinds of route - separate kernels with the activation traced, fused with the
    float32 convolution, fused with the split convolution - rectangular and ragged: the correct stand-ins pass, the route assertion tells the two
    convolution forms apart, and every injected fault of FRONT_FAULTS fails the checker on every route it applies to, except what FRONT_UNSEEN lists
    (reported with its ratio, not asserted)."""
    plan, sd, mel, ln = _setup(name, tm, lens, profile)
    if profile == "trained":
        mel = torch.from_numpy(synth.silence_floor_mel(len(lens), plan.n_mels, tm, lens, seed=5021 + tm)[0])
    b0 = plan.blocks[0]
    fold = chain_route(1, b0.dim_model)
    lens1, t1 = [(int(v) - 1) // 2 + 1 for v in ln], (tm - 1) // 2 + 1
    routes = [("separate", "fp32", True, False), ("fused fp32", "fp32", False, False), ("fused split", "split", False, False), ("ragged split", "split", False, True),
              ("ragged fp32", "fp32", False, True), ("ragged separate", "fp32", True, True)]
    bad = []
    with torch.no_grad():
        for tag, form, traced, ragged in routes:
            route = {"conv": form, "subsample": traced, "fuse_chain": 1}

            def run(fault):
                got = _standin(mel, ln if ragged else None, sd, plan, form, fold, fault, traced)
                if ragged:
                    got = _ragged_layout(got, lens1, t1, b0.group_size)
                rep = _Report("%s %s %s" % (name, profile, tag))
                check_front(got, plan, sd, mel, ln.tolist(), tm, ragged, route, rep)
                return rep, _front_over(rep)
            rep, over = run(None)
            rep.finish()
            print("%-28s %-9s %-13s %-46s ratio to the bound %10.3g  must stay inside; conv form fit / misfit %s" % (
                name, profile, tag, "none (stand-in)", over, getattr(rep, "form", None)))
            for fault in FRONT_FAULTS:
                if (fault == "lo tap plane dropped" and form != "split") or (fault == "time padding at the batch's last frame" and not ragged):
                    continue
                rep, over = run(fault)
                listed = (fault, form, profile) in FRONT_UNSEEN
                print("%-28s %-9s %-13s %-46s ratio to the bound %10.3g  %s" % (name, profile, tag, fault, over, "NOT DETECTABLE here (listed)" if listed else "must exceed"))
                if not listed and not (rep.fails or over > 1.0):
                    bad.append((tag, fault, over))
    assert not bad, bad


@pytest.mark.parametrize("ragged", [False, True])
def test_check_front_on_a_two_layer_reference_trace_and_two_faults(ragged):
    """ConformerCTC-Small's two-layer subsampler: a trace made by the float32-arithmetic reference on the kernels' own float32 formulas, laid out as the
    kernels lay it out (layer-1 image rows (b, f, t) channel-last and zero behind an utterance's own frames, layer-2 rows in (f2, c) order, both
    rectangular; ``linear`` gathered into the ragged row space) passes every stage - conv, conv2, linear, ffn1_0; layer 2 left in the reference's
    (c, f2) order, and layer-2 weights that missed their bf16 rounding, fail."""
    name, tm, lens = "ConformerCTCSmall", 150, [150, 97, 6]
    plan, sd, mel, ln = _setup(name, tm, lens)
    b0, B = plan.blocks[0], len(lens)
    half = lambda v: (v - 1) // 2 + 1
    lens2, t2 = [half(half(v)) for v in lens], half(half(tm))
    c1 = plan.sub_filters[1]

    def trace(fault):
        with torch.no_grad(), Q.hardware_like(1):
            mlen = ln if ragged else None
            a1 = Q.q(Q.front_conv(mel, mlen, sd, plan, F32))
            if ragged:
                a1 = Q.mask_time(a1, torch.tensor([half(v) for v in lens]))
            a2 = Q.q(Q.front_conv2(a1, sd, plan, F32, rnd=Q.ident if fault == "weights" else Q.q))
            got = {"subsample1": a1.permute(0, 2, 3, 1).reshape(-1, a1.shape[1])}
            k = a2.shape[1] * a2.shape[2]
            got["subsample"] = (a2.permute(0, 3, 1, 2) if fault == "order" else a2.permute(0, 3, 2, 1)).reshape(B * t2, k)
            x = Q.front_linear(Q.feature_rows(a2), sd, plan, F32)
            rest = {"linear": x.reshape(B * t2, -1), "blocks.0.x_ffn1": Q.ffn(x, sd, "blocks.0.feed_forward_module1", F32, True).reshape(B * t2, -1)}
            got.update(_ragged_layout(rest, lens2, t2, b0.group_size) if ragged else rest)
        return got
    route = {"conv": "fp32", "subsample": True, "fuse_chain": 1}
    for fault in (None, "order", "weights"):
        rep = _Report("%s two-layer %s fault %s" % (name, "ragged" if ragged else "rect", fault))
        with torch.no_grad():
            check_front(trace(fault), plan, sd, mel, ln.tolist(), tm, ragged, route, rep)
        print("two-layer %s fault %-8s ratio to the bound %.3g" % ("ragged" if ragged else "rect", fault, _front_over(rep)))
        if fault is None:
            rep.finish()
        else:
            # (the mis-ordered activation also disagrees with the ``linear`` this trace computed from the right one; conv and ffn1_0 stay inside)
            assert any(f.startswith("block 0 conv2 ") for f in rep.fails) and all(f.startswith(("block 0 conv2 ", "block 0 linear ")) for f in rep.fails), rep.fails[:3]
