"""Self-conditioned CTC on the GPU: csrc/interctc.hip alone through effconf_interctc against the rounding-aware stage of tests/interctc_ref.py, the Tiny InterCTC
encoder against the reference's goldens (bf16 path, split and fp32 modes; rectangular and ragged batches; row ranges; the trace), and the InterCTC model's
decoders.  Bounds: oracle.ref_bf16.stage_ratios <= 1 per stage (the project's 4 x / 8 x noise bound), the Tiny bounds of tests/test_gpu_encoder.py end to end,
2e-4 in the label-exact modes (tests/test_gpu_exact_and_sweep.py)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import interctc_ref as IR
from efficientconformer_amd import ConformerEncoderInterCTC, InterCTC, _lib, named_config, synth
from efficientconformer_amd.config import build_plan
from oracle import ref_bf16 as RB
from oracle import ref_encoder as R

pytestmark = pytest.mark.gpu

# (De, V) of the kernel-alone tests -> (dim_model stages, heads per stage, listed block): small encoders without strides whose listed block has that output width
STEP_CONFIGS = {32: ([24], [4]), 29: ([48], [4]), 256: ([120, 168, 240, 360], [4, 4, 4, 4]), 1000: ([256, 720], [4, 8])}
STEP_SHAPES = [(24, 32), (48, 29), (120, 256), (168, 256), (240, 256), (256, 1000), (360, 256), (720, 1000)]
# one row, one below / at / one above the wave's 32-row tile and the 64- and 128-row workgroups (two waves or a pair of column halves per tile: 64; four
# waves: 128), and two 128-row workgroups plus one row
ROWS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]


def _step_params(vocab):
    dims, heads = STEP_CONFIGS[vocab]
    n = len(dims)
    return dict(named_config("Tiny")["encoder_params"], dim_model=list(dims), num_heads=list(heads), num_blocks=n, expand_blocks=list(range(1, n)),
                strided_blocks=[], att_group_size=1, conv_stride=1, subsampling_filters=[8], interctc_blocks=list(range(n)), vocab_size=vocab)


@functools.lru_cache(maxsize=None)
def _step_encoder(vocab, recipe):
    """(encoder on the GPU with its handle packed, state dict) of the kernel-alone tests."""
    enc = ConformerEncoderInterCTC(_step_params(vocab))
    sd = synth.make_state_dict(enc.plan, 7)
    if recipe == "peaky":
        sd = IR.peaky(sd, enc.plan.interctc_blocks)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    enc = enc.cuda()
    enc._ensure_packed()
    return enc, sd


@functools.lru_cache(maxsize=None)
def _step_reference(de, vocab, recipe):
    """257 rows, their float64 reference and float32 noise runs (computed once; the step is row-local, so the first n rows are the n-row launch's reference)."""
    enc, sd = _step_encoder(vocab, recipe)
    k = [b.dim_expand for b in enc.plan.blocks].index(de)
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(de * 4099 + vocab)).standard_normal((max(ROWS), de)).astype(np.float32))
    r64, r32 = IR.stage_refs(x, sd, k)
    return k, x, r64, r32


def _launch(enc, k, x, y=None, probs=True, ws_fill=None):
    """effconf_interctc on the rows x (device) -> (y, probs or None)."""
    lib = _lib.load()
    rows, de = x.shape
    v = enc.plan.interctc_vocab
    y = torch.full_like(x, float("nan")) if y is None else y
    p = torch.full((rows, v), float("nan"), dtype=torch.float32, device=x.device) if probs else None
    ws = torch.empty(max(rows * v * 4, 256), dtype=torch.uint8, device=x.device)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    with torch.cuda.device(x.device):
        _lib.check(lib.effconf_interctc(enc._handle, k, x.data_ptr(), rows, y.data_ptr(), p.data_ptr() if probs else None, ws.data_ptr(), ws.numel(),
                                        torch.cuda.current_stream(x.device).cuda_stream), "interctc")
    torch.cuda.synchronize()
    return y, p


def _check_stage(tag, y, p, r64, r32, n, de, v):
    ry = RB.stage_ratios(y.cpu(), r64[0][:n], [r[0][:n] for r in r32], k_len=v, bf16_out=False)
    rp = RB.stage_ratios(p.cpu(), r64[1][:n], [r[1][:n] for r in r32], k_len=de, bf16_out=False)
    print("%s rows %d: y %.3f / %.3f  probs %.3f / %.3f" % (tag, n, ry["max"], ry["mean"], rp["max"], rp["mean"]))
    assert torch.isfinite(y).all() and torch.isfinite(p).all(), tag
    assert ry["max"] <= 1.0 and ry["mean"] <= 1.0, (tag, n, ry, RB.worst_element(y.cpu(), r64[0][:n]))
    assert rp["max"] <= 1.0 and rp["mean"] <= 1.0, (tag, n, rp, RB.worst_element(p.cpu(), r64[1][:n]))


@pytest.mark.parametrize("recipe", IR.RECIPES)
@pytest.mark.parametrize("de,vocab", STEP_SHAPES)
def test_step_kernel_alone(de, vocab, recipe):
    enc, _ = _step_encoder(vocab, recipe)
    k, x, r64, r32 = _step_reference(de, vocab, recipe)
    xd = x.cuda()
    tag = "(%d, %d) %s" % (de, vocab, recipe)
    got = {}
    for n in ROWS:
        y, p = _launch(enc, k, xd[:n].contiguous())
        _check_stage(tag, y, p, r64, r32, n, de, vocab)
        assert abs(float(p.sum(-1).mean()) - 1.0) < 1e-5
        got[n] = (y, p)
    y257, p257 = got[257]
    # the first 33 rows of a 257-row launch are the 33-row launch: a row does not depend on which other rows share the launch
    assert torch.equal(y257[:33], got[33][0]) and torch.equal(p257[:33], got[33][1])
    # y aliased to x
    xa = xd.clone()
    ya, pa = _launch(enc, k, xa, y=xa)
    assert ya.data_ptr() == xa.data_ptr() and torch.equal(ya, y257) and torch.equal(pa, p257)
    # without the probability output: the same y (and the input rows are not touched)
    yn, _ = _launch(enc, k, xd, probs=False)
    assert torch.equal(yn, y257) and torch.equal(xd.cpu(), x)


@pytest.mark.parametrize("de,vocab", [(48, 29), (256, 1000), (720, 1000)])
def test_padded_vocabulary_reads_nothing_it_should_not(de, vocab, monkeypatch):
    """V = 29 (3 padded columns of 32) and V = 1000 (24): with 0xFF (NaN) bytes in the workspace and in guard regions around every parameter buffer
    (EFFCONF_POISON_GUARDS) the outputs are finite and bit-identical to the clean run - padded columns are excluded by selection, nothing is read past a
    weight image or past x + rows * De."""
    enc, sd = _step_encoder(vocab, "peaky")
    k, x, r64, r32 = _step_reference(de, vocab, "peaky")
    n = 97
    xd = x[:n].contiguous().cuda()
    y0, p0 = _launch(enc, k, xd)
    monkeypatch.setenv("EFFCONF_POISON_GUARDS", "16")
    poisoned = ConformerEncoderInterCTC(_step_params(vocab))
    poisoned.load_state_dict({key: torch.from_numpy(val) for key, val in sd.items()}, strict=True)
    poisoned = poisoned.cuda()
    poisoned._ensure_packed()
    # the rows at the very end of their allocation: a read past x + rows * De lands in whatever follows
    y1, p1 = _launch(poisoned, k, xd, ws_fill=0xFF)
    assert torch.isfinite(y1).all() and torch.isfinite(p1).all()
    assert torch.equal(y1, y0) and torch.equal(p1, p0)
    assert float(p1.min()) >= 0.0 and abs(float(p1.sum(-1).max()) - 1.0) < 1e-5


# ------------------------------------------------------------------ the Tiny encoder against the reference's goldens
@functools.lru_cache(maxsize=None)
def _tiny_model(recipe):
    cfg = dict(named_config("Tiny"), model_type="InterCTC")
    cfg["encoder_params"] = dict(cfg["encoder_params"], interctc_blocks=list(IR.TINY_BLOCKS))
    m = InterCTC.from_config(cfg)
    sd = IR.tiny_state_dict(recipe, prefix="encoder.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda(), IR.tiny_state_dict(recipe)


@functools.lru_cache(maxsize=None)
def _tiny_oracle(recipe, tm):
    lens = dict(IR.BATCHES)[tm]
    mel, ln = IR.tiny_mel(tm, lens)
    trace = {}
    with torch.no_grad():
        out, out_len, probs = IR.encoder_from_mel(torch.from_numpy(mel), torch.from_numpy(ln), IR.tiny_state_dict(recipe), build_plan(IR.tiny_params(), interctc=True),
                                                  trace=trace)
    return mel, ln, out, out_len, probs, trace


def _err(got, ref):
    d = (got.double() - ref.double()).abs()
    return float(d.max()), float(d.mean())


def _reset(m):
    m.encoder.precision = "bf16"
    m.encoder.ragged = False
    m.encoder.sub_batches = 1


@pytest.mark.parametrize("tm", [47, 100])
@pytest.mark.parametrize("recipe", IR.RECIPES)
def test_tiny_encoder_vs_reference_golden(recipe, tm):
    m, sd = _tiny_model(recipe)
    _reset(m)
    g = IR.load_golden(recipe, tm)
    mel, ln, ref, ref_len, ref_probs, otrace = _tiny_oracle(recipe, tm)
    mel_d, ln_d = torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda()
    out, out_len, att, probs = m.encoder.forward_mel(mel_d, ln_d, return_interctc=True)
    assert out_len.cpu().tolist() == g["out_len"].tolist() and len(att) == 6 and len(probs) == 3
    mx, mean = _err(out.cpu(), torch.from_numpy(g["out"]))
    print("%s T%d: out err max %.4f mean %.5f" % (recipe, tm, mx, mean))
    assert mx < 0.08 and mean < 0.01
    # the opt-in list is empty by default, and the side output does not change the rows
    out2, _, _, none = m.encoder.forward_mel(mel_d, ln_d)
    assert none == [] and torch.equal(out2, out)
    # a traced forward equals the untraced one bit for bit; every step's output within the per-block bounds of tests/test_gpu_encoder.py
    tout, _, trace = m.encoder.trace_forward_mel(mel_d, ln_d)
    assert torch.equal(tout, out)
    for i, k in enumerate(IR.TINY_BLOCKS):
        want = otrace["blocks.%d.x_interctc" % k]
        got = trace["blocks.%d.x_interctc" % k]
        d = (got.double() - want.reshape(-1, want.shape[-1]).double()).abs()
        scale = max(float(want.abs().max()), 1.0)
        assert float(d.max()) / scale < 0.02 and float(d.mean()) / scale < 0.003, (k, float(d.max()) / scale, float(d.mean()) / scale)
        # the probabilities (returned and traced: the same numbers) and the step's output within the stage bound on the step's own traced input
        x_in = trace["blocks.%d.out" % k]
        assert tuple(probs[i].shape) == tuple(g["probs_%d" % k].shape)
        p = probs[i].reshape(-1, probs[i].shape[-1])
        assert torch.equal(p.cpu(), trace["blocks.%d.interctc_p" % k])
        r64, r32 = IR.stage_refs(x_in, sd, k)
        _check_stage("%s T%d block %d" % (recipe, tm, k), got.cuda(), p, r64, r32, x_in.shape[0], x_in.shape[1], IR.TINY_VOCAB)
        assert float((p.cpu() - torch.from_numpy(g["probs_%d" % k]).reshape(-1, IR.TINY_VOCAB)).abs().max()) < 0.08


@pytest.mark.parametrize("precision", ["bf16", "split"])
def test_ragged_utterances_do_not_depend_on_their_batch(precision):
    m, sd = _tiny_model("peaky")
    _reset(m)
    enc = m.encoder
    enc.precision, enc.ragged = precision, True
    try:
        mel, ln = IR.tiny_mel(100, [100, 77, 52])
        mel_d, ln_d = torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda()
        out, out_len, _, probs = enc.forward_mel(mel_d, ln_d, x_len_host=ln, return_interctc=True)
        plain, _, _, _ = enc.forward_mel(mel_d, ln_d, x_len_host=ln)
        assert torch.equal(plain, out)
        plan = enc.plan
        for b in range(3):
            n = int(ln[b])
            one, one_len, _, p1 = enc.forward_mel(mel_d[b:b + 1, :, :n].contiguous(), ln_d[b:b + 1], x_len_host=ln[b:b + 1], return_interctc=True)
            t = int(one_len[0])
            assert int(out_len[b]) == t and torch.equal(out[b, :t], one[0, :t]) and float(out[b, t:].abs().max() if t < out.shape[1] else 0.0) == 0.0
            ts = plan.lengths_from_mel(n)[1]
            for i, k in enumerate(IR.TINY_BLOCKS):
                tk = ts[k]
                assert tuple(probs[i].shape) == (3, plan.lengths_from_mel(100)[1][k], IR.TINY_VOCAB)
                assert torch.equal(probs[i][b, :tk], p1[i][0, :tk])
                assert abs(float(probs[i][b, :tk].sum(-1).mean()) - 1.0) < 1e-5
                assert float(probs[i][b, tk:].abs().sum()) == 0.0               # zeros behind the utterance's own frames
            if precision == "split":
                # the reference on that utterance ALONE (no pad frames exist in a ragged batch)
                with torch.no_grad():
                    ref, _, _ = IR.encoder_from_mel(torch.from_numpy(mel[b:b + 1, :, :n]), torch.from_numpy(ln[b:b + 1]), sd, build_plan(IR.tiny_params(), interctc=True))
                assert _err(out[b, :t].cpu(), ref[0])[0] < 2e-4
    finally:
        _reset(m)


def test_sub_batch_streams_are_bit_identical():
    m, _ = _tiny_model("flat")
    _reset(m)
    mel, ln = IR.tiny_mel(100, [100, 77, 52])
    mel_d, ln_d = torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda()
    one = m.encoder.forward_mel(mel_d, ln_d)[0]
    try:
        for ragged in (False, True):
            m.encoder.ragged = ragged
            want = m.encoder.forward_mel(mel_d, ln_d, x_len_host=ln)[0] if ragged else one
            m.encoder.sub_batches = 2
            got = m.encoder.forward_mel(mel_d, ln_d, x_len_host=ln)[0]
            torch.cuda.synchronize()
            assert torch.equal(got, want), ragged
            m.encoder.sub_batches = 1
    finally:
        _reset(m)


def _golden_labels(g):
    offs = g["label_offsets"]
    return [g["labels"][offs[i]:offs[i + 1]].tolist() for i in range(len(offs) - 1)]


@pytest.mark.parametrize("tm", [47, 100])
@pytest.mark.parametrize("recipe", IR.RECIPES)
@pytest.mark.parametrize("precision", ["split", "fp32"])
def test_label_exact_modes_vs_reference_golden(precision, recipe, tm):
    m, sd = _tiny_model(recipe)
    _reset(m)
    g = IR.load_golden(recipe, tm)
    mel, ln = IR.tiny_mel(tm, dict(IR.BATCHES)[tm])
    mel_d, ln_d = torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda()
    try:
        m.encoder.precision = precision
        out, out_len, _, probs = m.encoder.forward_mel(mel_d, ln_d, return_interctc=True)
        assert _err(out.cpu(), torch.from_numpy(g["out"]))[0] < 2e-4
        for i, k in enumerate(IR.TINY_BLOCKS):
            assert float((probs[i].cpu() - torch.from_numpy(g["probs_%d" % k])).abs().max()) < 2e-4
        assert m.greedy_labels(mel_d, ln_d, from_mel=True) == _golden_labels(g)
        if precision == "split":
            # ragged: utterance 0 has no pad frames in the rectangular batch either - the golden's rows and labels; the others against the reference run alone
            m.encoder.ragged = True
            rout, rlen, _, _ = m.encoder.forward_mel(mel_d, ln_d, x_len_host=ln)
            t0 = int(rlen[0])
            assert _err(rout[0, :t0].cpu(), torch.from_numpy(g["out"][0, :t0]))[0] < 2e-4
            labels = m.greedy_labels(mel_d, ln_d, from_mel=True)
            assert labels[0] == _golden_labels(g)[0]
            for b in (1, 2):
                n = int(ln[b])
                with torch.no_grad():
                    ref, ref_len, _ = IR.encoder_from_mel(torch.from_numpy(mel[b:b + 1, :, :n]), torch.from_numpy(ln[b:b + 1]), sd, build_plan(IR.tiny_params(), interctc=True))
                    logits = R.ctc_logits(ref, sd)
                assert _err(rout[b, :int(rlen[b])].cpu(), ref[0])[0] < 2e-4
                top2 = logits.topk(2, dim=-1).values
                if float((top2[..., 0] - top2[..., 1]).min()) > 1e-3:          # identical wherever the oracle's own margins exceed fp32 noise
                    assert labels[b] == R.ctc_greedy(logits, ref_len)[0]
    finally:
        _reset(m)


def test_interctc_model_decoders():
    """Every decoder of ModelCTC on an InterCTC model: shapes and lengths as the plain model's tests expect them; forward returns the reference's four values."""
    m, _ = _tiny_model("flat")
    _reset(m)
    g = IR.load_golden("flat", 100)
    lens = np.array([24000, 16000, 9000], dtype=np.int64)
    audio = torch.from_numpy(synth.make_audio(lens, seed=5)).cuda()
    lens_d = torch.from_numpy(lens).cuda()
    logits, logits_len, att, probs = m.forward((audio, None, lens_d, None))
    t_out = m.encoder.plan.lengths(int(lens.max()))[2][-1]
    assert tuple(logits.shape) == (3, t_out, IR.TINY_VOCAB) and logits_len.cpu().tolist() == [m.encoder.plan.lengths(int(n))[2][-1] for n in lens]
    assert len(att) == 6 and len(probs) == 3 and tuple(probs[0].shape) == (3, m.encoder.plan.lengths(int(lens.max()))[2][1], IR.TINY_VOCAB)
    ids = m.gready_search_decoding(audio, lens_d)
    assert len(ids) == 3 and all(isinstance(i, list) for i in ids)
    beam = m.beam_search_decoding(audio, lens_d, beam_size=4)
    assert len(beam) == 3
    al = m.align(audio, lens_d, ids)
    assert len(al) == 3 and all(a.status == 0 and a.tokens == i for a, i in zip(al, ids))
    ll = m.score_labels(audio, lens_d, ids)
    assert tuple(ll.shape) == (3,) and torch.isfinite(ll).all() and all(abs(float(ll[b])) >= 0 and float(ll[b]) >= al[b].score - 1e-3 for b in range(3))
    ga = m.greedy_alignment(audio, lens_d)
    assert [a.tokens for a in ga] == ids
    # label-exact greedy on the goldens' batch: the reference's own labels
    mel, ln = IR.tiny_mel(100, [100, 77, 52])
    m.encoder.ragged = True
    try:
        exact = m.greedy_labels(torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda(), from_mel=True, label_exact="always")
    finally:
        _reset(m)
    assert exact[0] == _golden_labels(g)[0] and len(exact) == 3
