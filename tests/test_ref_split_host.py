"""CPU tests of the split mode's stage contract (oracle/ref_split.py, tests/split_parity.py): the reference is the float64 oracle, the emulated operand pairs
sit inside the derived element-wise term, CPU stand-ins of a correct kernel pass every stage bound the GPU test applies, and the bounds see the faults they were
built for - with, for every fault, what today's end-to-end 2e-4 / 2e-5 (tests/test_gpu_round6.py SPLIT_MAX / SPLIT_MEAN) makes of it.

The reference: with every rounding off the chained stages of ref_bf16 are ref_encoder.encoder_from_mel(dtype = float64) - tests/test_ref_bf16_host.py
test_stages_without_roundings_chained_are_the_float64_oracle and test_front_end_without_roundings_is_the_float64_oracle; no stage function was added for the
split mode, so nothing new is to be shown there beyond the kernel-shaped forms (``rnd = keep``: the folded LayerNorm) being the same mathematics (first test)."""
import numpy as np
import pytest
import torch

from efficientconformer_amd import ModelCTC, named_config, synth
from bf16_parity import _Report, _Space
from split_parity import check_split_front, check_split_trace
from oracle import ref_bf16 as Q
from oracle import ref_split as S
from oracle.ref_split import CHAIN_KINDS, Emu, keep

F64, F32 = torch.float64, torch.float32
SPLIT_MAX, SPLIT_MEAN = 2e-4, 2e-5          # the end-to-end bound of tests/test_gpu_round6.py (absolute, against the oracle's encoder output)
ROUTE = {"chain": True, "ffn": True, "sublin": True}


def _setup(name, tm, lens, profile="synthetic"):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cfg = named_config(name)
    plan = ModelCTC.from_config(cfg).encoder.plan
    vocab = cfg["tokenizer_params"]["vocab_size"]
    sd = synth.make_state_dict(plan, 7, vocab) if profile == "synthetic" else synth.make_stressed_state_dict(plan, 7, profile, vocab)
    mel, ln = synth.make_mel(len(lens), plan.n_mels, tm, lens, seed=5021 + tm)
    return plan, sd, torch.from_numpy(mel), torch.from_numpy(ln)


def _lens1(plan, ln):
    for _ in range(plan.sub_layers):
        ln = torch.div(ln - 1, 2, rounding_mode="floor") + 1
    return ln


def _out_len(plan, lens1):
    out = lens1.clone()
    for bp in plan.blocks:
        if bp.conv_stride > 1:
            out = torch.div(out - 1, bp.conv_stride, rounding_mode="floor") + 1
    return out


def _merged(plan, k):
    return k + 1 < len(plan.blocks) and plan.blocks[k + 1].dim_model == plan.blocks[k].dim_expand


def _split_trace(plan, sd, lin, lens1, dtype, faults=None):
    """encoder_from_linear's (B, rows, columns) trace as the rectangular split-mode trace of the fused route lays it out (tests/split_parity.py)."""
    tr = {}
    out = Q.encoder_from_linear(lin, lens1, sd, plan, dtype, rnd=keep, folded=True, trace=tr, faults=faults)
    got = {"linear": lin.float().reshape(-1, lin.shape[-1])}
    for key, v in tr.items():
        blk, tag = key.rsplit(".", 1)
        k = int(blk.split(".")[1])
        bp = plan.blocks[k]
        if tag == "x_conv" or (tag == "out" and _merged(plan, k)):
            continue
        if tag == "x_mhsa" and bp.transition:      # the trace entry conv_res: the same evaluation (and summation order) the chained stand-in used
            got[blk + ".conv_res"] = Q.conv_res(v, sd, bp, dtype, keep).float().reshape(-1, bp.dim_expand)
        if tag == "qu":
            u = torch.from_numpy(np.asarray(sd[blk + ".multi_head_self_attention_module.mhsa.u"])).to(v.dtype)
            tag, v = "q", v - u
        if tag == "att_o":
            t = v.shape[1]
            v = torch.nn.functional.pad(v, (0, 0, 0, (t + bp.group_size - 1) // bp.group_size * bp.group_size - t))
        got[blk + "." + tag] = v.float().reshape(-1, v.shape[-1]).clone()
    return got, out


def _stand_in_trace(plan, sd, mel, ln, faults=None, ulps=1, **emu):
    """A correct split kernel on the CPU: float32, the kernels' LayerNorm / sigmoid / exp formulas at an ulp shift no noise run uses, the operand pairs of
    ref_split.Emu contracted in chunks of 32 (another summation order than any noise run).  Rectangular batch, fused route."""
    with torch.no_grad(), Q.hardware_like(ulps), Q.product_like(Emu(CHAIN_KINDS | {"linear"}, chunk=32, **emu)), S.split_front():
        lin = Q.front_end(mel, None, sd, plan, F32, keep, "split")
        return _split_trace(plan, sd, lin, _lens1(plan, ln), F32, faults)


def test_the_kernel_shaped_forms_are_the_same_mathematics():
    """rnd = keep, float64, no emulation: the folded-LayerNorm forms the noise model evaluates equal the plain forms (rnd = ident) to float64 rounding."""
    plan, sd, mel, ln = _setup("Tiny", 333, [333, 250, 97, 12])
    with torch.no_grad():
        lin = Q.front_end(mel, None, sd, plan, F64, Q.ident)
        a = Q.encoder_from_linear(lin, _lens1(plan, ln), sd, plan, F64, rnd=Q.ident)
        b = Q.encoder_from_linear(Q.front_end(mel, None, sd, plan, F64, keep), _lens1(plan, ln), sd, plan, F64, rnd=keep, folded=True)
    assert Q.rel(b, a)[0] < 1e-6, Q.rel(b, a)          # the folds themselves are float32 (bn_fold2d, W * gamma): 1e-7 of a weight


@pytest.mark.parametrize("kind,scale", [("ffn2", S.SA), ("out", S.SR), ("res", S.LO_SCALE)])
def test_the_emulated_pairs_sit_inside_the_derived_element_wise_term(kind, scale):
    """ref_split.split_term against the emulation with exact (float64) accumulation: inside it everywhere, and above 1 / 50 of it somewhere (the convention of
    tests/test_mel_ref_host.py: a bound fifty times what it bounds checks nothing).  Operands over ten binades, some below the l plane's underflow."""
    g = torch.Generator().manual_seed(11)
    a = torch.randn(257, 200, generator=g) * torch.exp2(torch.randint(-12, 2, (257, 200), generator=g).float())
    w = torch.randn(96, 200, generator=g) * torch.exp2(torch.randint(-14, -1, (96, 200), generator=g).float())
    got = Emu(CHAIN_KINDS)(a.double(), w.double(), kind)
    err = (got - a.double() @ w.double().T).abs()
    term = S.split_term(a.abs(), w.abs(), scale, S.SW if kind != "res" else S.LO_SCALE)
    r = float((err / term).max())
    print("split term, %s operands: worst emulation error / term %.3f" % (kind, r))
    assert 1.0 / 50.0 < r <= 1.0, r


def _ratios(rep):
    return {key: v for key, (v, _) in rep.worst.items() if not key[1].startswith(("noise", "single"))}


@pytest.mark.parametrize("name,tm,lens,profile", [("Tiny", 333, [333, 250, 97, 12], "synthetic"), ("Tiny", 333, [333, 250, 97, 12], "trained"),
                                                  ("EfficientConformerCTCSmall", 300, [300, 211, 97], "synthetic"),
                                                  ("EfficientConformerCTCSmall", 300, [300, 211, 97], "trained")])
def test_cpu_stand_ins_of_a_correct_kernel_pass_every_stage_bound(name, tm, lens, profile):
    plan, sd, mel, ln = _setup(name, tm, lens, profile)
    got, _ = _stand_in_trace(plan, sd, mel, ln)
    with torch.no_grad():
        rep = check_split_trace(got, _out_len(plan, _lens1(plan, ln)).tolist(), plan, sd, ln.tolist(), tm, False, ROUTE, "%s %s stand-in" % (name, profile))
        check_split_front(got, plan, sd, mel, ln.tolist(), tm, False, ROUTE, rep)
    rep.finish()


# ------------------------------------------------------------------ sensitivity: what the stage bounds see, and what the end-to-end bound makes of the same fault
class _At:
    """An Emu hook armed for the n-th product of one kind (products run in encoder order: the second product of block k's FFN2 is "ffn2" number 2 k + 1,
    block 0's FFN1 being number 0; its first product "ffn1" number 2 k + 1 likewise; Q of block k is "qkv" number 3 k)."""

    def __init__(self, kind, nth, fn):
        self.kind, self.nth, self.fn, self.seen = kind, nth, fn, 0

    def __call__(self, kind, val):
        if kind != self.kind:
            return val
        self.seen += 1
        return self.fn(val) if self.seen - 1 == self.nth else val


def _drop_act_low(p):        # the low plane of one 32-unit hidden chunk never reaches the matrix pipe (a_l w_h of that chunk dropped)
    p["al"][..., 32:64] = 0.0


def _drop_weight_low(p):     # the same on the weight side (a_h w_l of that chunk dropped)
    p["wl"][:, 32:64] = 0.0


def _stale_chunk(p):         # the last 64 rows meet the PREVIOUS 32-unit weight chunk in the second chunk's place (a weight-ring race's signature)
    for n in ("ah", "al"):
        rows = p[n].reshape(-1, p[n].shape[-1])[-64:]
        rows[:, 0:32] += rows[:, 32:64]
        rows[:, 32:64] = 0.0


def _kswap(p):               # two K slots of one 16-block of the weight image swapped: positions 3 and 9 (features 3 and 5 of "position 8 kh + e holds feature 8 (e >> 2) + 4 kh + (e & 3)")
    for n in ("wh", "wl"):
        p[n][:, [3, 5]] = p[n][:, [5, 3]]


def _no_bias(sd, k):         # the bias column D of FFN2's folded pre-norm image missing: b1 + W1 beta never added
    pf = "blocks.%d.feed_forward_module2.layers." % k
    w1, b1, beta = (torch.from_numpy(np.asarray(sd[pf + n])).double() for n in ("1.weight", "1.bias", "0.bias"))
    bias = (b1 + w1 @ beta).float()
    return lambda out: out - bias


def _exp_uncorrected(x):     # sx_expf without its first-order correction: exp2 of the ROUNDED product x log2(e)
    if x.dtype == F32:
        return torch.exp2(x * 1.44269502162933349609375)
    return torch.exp(x)


def _over(rep):
    r = _ratios(rep)
    key = max(r, key=r.get)
    return r[key], "%s %s" % key


def test_the_stage_bounds_see_the_injected_faults_and_the_end_to_end_bound_does_not(monkeypatch):
    """EfficientConformerCTCSmall, 300 mel frames, lengths [300, 211, 97], fused route, faults in block 7 (D = 168).  Every fault is injected into a stand-in
    whose later stages are computed consistently from the faulted values, as a kernel bug would leave them; the checker of the GPU test runs on block 7 (and on
    the front end for the last fault) and the worst statistic / bound is asserted above 1.  Control: the same faulted forward's encoder output against the
    float64 oracle, as today's end-to-end test measures it (max / mean |delta| against 2e-4 / 2e-5).  Not seen, by construction of the bounds (printed, asserted
    BELOW 1 so that a change of this shows): a low plane that keeps 8 of its 11 bits; the softmax's exp without the first-order correction (|x| 2^-24 of a
    probability: at the float32 runs' own level - and the split kernels' softmax does not use sx_expf at all, it feeds log2-unit scores to v_exp_f32)."""
    name, tm, lens, kb = "EfficientConformerCTCSmall", 300, [300, 211, 97], 7
    plan, sd, mel, ln = _setup(name, tm, lens)
    lens1 = _lens1(plan, ln)
    out_len = _out_len(plan, lens1).tolist()
    with torch.no_grad():
        oracle = Q.encoder_from_linear(Q.front_end(mel, None, sd, plan, F64, Q.ident), lens1, sd, plan, F64, rnd=Q.ident)

    def run(label, faults=None, **emu):
        got, out = _stand_in_trace(plan, sd, mel, ln, faults=faults, **emu)
        with torch.no_grad():
            rep = check_split_trace(got, out_len, plan, sd, ln.tolist(), tm, False, ROUTE, label, only=(kb,))
        d = (out.double() - oracle).abs()
        ratio, where = _over(rep)
        e2e = max(float(d.max()) / SPLIT_MAX, float(d.mean()) / SPLIT_MEAN)
        print("%-58s stage bound %8.3g x (%s)   end to end max %.2e mean %.2e = %.2f x today's bound" % (label, ratio, where, float(d.max()), float(d.mean()), e2e))
        return ratio, e2e

    base, e0 = run("no fault")
    assert base <= 1.0 and e0 < 0.1
    ffn2 = 2 * kb + 1
    seen = [
        ("FFN2: low plane of one hidden chunk dropped, activation", dict(fault=_At("ffn2", ffn2, _drop_act_low))),
        ("FFN2: low plane of one hidden chunk dropped, weight", dict(fault=_At("ffn2", ffn2, _drop_weight_low))),
        ("FFN2: stale 32-unit weight chunk on the last 64 rows", dict(fault=_At("ffn2", ffn2, _stale_chunk))),
        ("FFN2: two K slots swapped in one 16-block of W1's image", dict(fault=_At("ffn1", ffn2, _kswap))),
        ("FFN2: bias column D of the folded pre-norm image missing", dict(post=_At("ffn1", ffn2, _no_bias(sd, kb)))),
        ("every pair: l keeps 5 of its 11 bits", dict(lo_bits=5)),
        ("depthwise taps one frame late", dict(faults={(kb, "depthwise"): dict(shift=1)})),
        ("positional rows shifted by one", dict(faults={(kb, "pos_e"): dict(shift=1)})),
        ("key mask off by one group", dict(faults={(kb, "attention"): dict(key_shift=1)})),
    ]
    hidden = []
    for label, kw in seen:
        faults = kw.pop("faults", None)
        ratio, e2e = run(label, faults, **kw)
        assert ratio > 1.0, (label, ratio)
        if e2e < 1.0:
            hidden.append(label)
    print("passed by today's end-to-end bound: %d of %d faults: %s" % (len(hidden), len(seen), "; ".join(hidden)))
    # what the stage contract adds: the precision faults - a lost or shortened low plane - pass today's end-to-end bound (the measurements that motivated this file)
    assert [lb for lb in hidden if "low plane" in lb or "keeps 5" in lb] == [seen[0][0], seen[1][0], seen[5][0]], hidden
    r8, _ = run("every pair: l keeps 8 of its 11 bits (NOT seen)", lo_bits=8)
    monkeypatch.setattr(Q, "_exp", _exp_uncorrected)
    rx, _ = run("softmax exp without the first-order correction (NOT seen)")
    assert r8 <= 1.0 and rx <= 1.0, (r8, rx)


def test_the_front_bound_sees_a_ragged_utterance_padded_at_the_batch_end():
    """A ragged batch whose short utterances see the batch's frames behind their own end (time padding taken at the batch's last frame, not at the utterance's):
    the last output frame of every odd-length utterance is wrong.  Tiny and EfficientConformerCTCSmall, fused front end; the correct stand-in passes."""
    for name in ("Tiny", "EfficientConformerCTCSmall"):
        plan, sd, mel, ln = _setup(name, 333, [333, 251, 97, 13])
        lens1 = _lens1(plan, ln).tolist()
        b0 = plan.blocks[0]
        sp = _Space(True, lens1, max(lens1), b0.group_size)
        for fault in (False, True):
            with torch.no_grad(), Q.hardware_like(1), Q.product_like(Emu(CHAIN_KINDS | {"linear"}, chunk=32)), S.split_front():
                lin = Q.front_end(mel, None if fault else ln, sd, plan, F32, keep, "split")
                rows = torch.zeros(sp.rows, b0.dim_model)
                for b, n in enumerate(sp.live):
                    rows[sp.x0[b]: sp.x0[b] + n] = lin[b, :n]
                got = {"linear": rows, "blocks.0.x_ffn1": Q.ffn(rows, sd, "blocks.0.feed_forward_module1", F32, True, keep)}
            rep = _Report("%s ragged front, %s" % (name, "padded at the batch end" if fault else "correct"))
            with torch.no_grad():
                check_split_front(got, plan, sd, mel, ln.tolist(), 333, True, ROUTE, rep)
            ratio, where = _over(rep)
            print("%s: worst statistic / bound %.3g (%s)" % (rep.label, ratio, where))
            assert (ratio > 1.0) == fault, (name, fault, ratio)
