"""-m gpu tests of the kernels whose lane constants are recomputed instead of spilled (csrc/chain3.hip, chain.hip's chain B at D = 168, attention2.hip at head
width 64): only addresses changed, so every output is bit-identical to the form it is compared with - chain3.hip against chain.hip (chain_pair = 5 / 0), the
8-wave chain workgroups against the 2-wave ones (chain_small_m = 0 / default), a launch of two utterances against each utterance alone - and the attention
kernel alone stays within the bf16 output's rounding of a float64 evaluation.  Shapes: the smallest that reach a partial row tile, a second workgroup with one
valid row, one to six key blocks (both parities of the positional ring) and the masked tail path of d = 42."""
import numpy as np
import pytest
import torch

from efficientconformer_amd import ModelCTC, _lib, named_config, synth

pytestmark = pytest.mark.gpu

BF16_MAX, BF16_MEAN = 0.02, 0.003             # the kernel-level attention parity bound (tests/test_gpu_weight_stats.py)

_MODEL = {}


def _small():
    if "m" not in _MODEL:
        cfg = named_config("EfficientConformerCTCSmall")
        m = ModelCTC.from_config(cfg)
        sd = synth.make_state_dict(m.encoder.plan, 3, None, prefix="encoder.")
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        _MODEL["m"] = m.cuda()
    m = _MODEL["m"]
    m.encoder.ragged, m.encoder.sub_batches = False, 1
    m.encoder.set_option("chain_small_m", 4096)
    m.encoder.set_option("chain_pair", 5)
    return m


def _stage_rows(samples, stage):
    """rows of one utterance at stage 1 / 2 / 3 of EfficientConformerCTCSmall: mel frames, the stride-2 subsampling, then one stride-2 block per stage"""
    n = samples // 160 + 1
    for _ in range(stage):
        n = (n - 1) // 2 + 1
    return n


def _both_layouts(m, audio, ln, lens):
    outs = {}
    for ragged in (False, True):
        m.encoder.ragged = ragged
        kw = {"x_len_host": lens} if ragged else {}
        enc, el, _ = m.encoder(audio, ln, **kw)
        outs[ragged] = (enc.clone(), el.clone())
    return outs


@pytest.mark.parametrize("seconds,rows3", [((1.5,), 19), ((3.4, 3.4, 3.4), 129)])
def test_chain3_partial_tile_and_one_row_workgroup_bit_identical_to_chain_hip(seconds, rows3):
    """chain_pair = 5 (chain A of stage 3 on chain3.hip) against chain_pair = 0 (chain.hip): one utterance with fewer than 32 stage-3 rows (one partial row
    tile), and three whose 129 rows leave the second workgroup one valid row - ragged and rectangular."""
    m = _small()
    lens = np.array([int(16000 * s) for s in seconds], dtype=np.int64)
    assert sum(_stage_rows(int(n), 3) for n in lens) == rows3
    audio = torch.from_numpy(synth.make_audio(lens, seed=5)).cuda()
    ln = torch.from_numpy(lens).cuda()
    m.encoder.set_option("chain_small_m", 0)               # chain.hip's wide shapes as the reference for every launch (tests/test_gpu_round5.py)
    res = {}
    for pair in (0, 5):
        m.encoder.set_option("chain_pair", pair)
        res[pair] = _both_layouts(m, audio, ln, lens)
    for ragged in (False, True):
        a, b = res[0][ragged], res[5][ragged]
        assert int(a[1].sum()) == rows3 and torch.equal(a[1], b[1])
        assert torch.isfinite(a[0].float()).all()
        assert torch.equal(a[0], b[0]), (ragged, float((a[0].float() - b[0].float()).abs().max()))


@pytest.mark.parametrize("samples,rows2", [(130 * 160, 33), (1024 * 160, 257)])
def test_eight_wave_chains_at_33_and_257_stage2_rows_bit_identical_to_two_wave_chains(samples, rows2):
    """chain_small_m = 0 (8-wave workgroups of 256 rows: chain_kernel<12, 8, 3, *> at D = 168) against the default (2-wave workgroups): 33 rows = one
    workgroup whose second wave holds one row, 257 rows = a second workgroup with one row.  The contract of tests/test_gpu_round4.py at these sizes."""
    m = _small()
    lens = np.array([samples], dtype=np.int64)
    assert _stage_rows(samples, 2) == rows2
    audio = torch.from_numpy(synth.make_audio(lens, seed=6)).cuda()
    ln = torch.from_numpy(lens).cuda()
    res = {}
    for small in (4096, 0):
        m.encoder.set_option("chain_small_m", small)
        res[small] = _both_layouts(m, audio, ln, lens)
    for ragged in (False, True):
        a, b = res[4096][ragged], res[0][ragged]
        assert int(a[1][0]) == (rows2 - 1) // 2 + 1 and torch.equal(a[1], b[1])
        assert torch.isfinite(a[0].float()).all()
        assert torch.equal(a[0], b[0]), (ragged, float((a[0].float() - b[0].float()).abs().max()))


def _attention(lib, qu, k, v, e, dvu, dpad, lens, heads, t, dim):
    bsz = len(lens)
    def dev_bf16(z):                                               # + 512 bytes of readable slack behind the rows
        flat = torch.zeros(z.numel() + 256, dtype=torch.bfloat16, device="cuda")
        flat[:z.numel()] = z.reshape(-1).to(torch.bfloat16).cuda()
        return flat
    qud, kd, vd, ed = dev_bf16(qu), dev_bf16(k), dev_bf16(v), dev_bf16(e)
    lens_d = torch.tensor(lens, dtype=torch.int32).cuda()
    out = torch.zeros(bsz * t, dim, dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.effconf_relpos_attention(qud.data_ptr(), kd.data_ptr(), vd.data_ptr(), ed.data_ptr(), dvu.data_ptr(), dpad, lens_d.data_ptr(),
                                            bsz, heads, t, 1, dim, out.data_ptr(), dim, 1, torch.cuda.current_stream().cuda_stream), "relpos_attention")
    torch.cuda.synchronize()
    return out.view(bsz, t, dim)


@pytest.mark.parametrize("tg", [14, 64, 65, 142, 201, 321])
@pytest.mark.parametrize("d", [42, 60])
def test_head_width_64_attention_alone_vs_float64_and_each_utterance_alone(d, tg):
    """relpos_attention2_kernel<64, 4, 1, 1> through effconf_relpos_attention (H = 4, group 1: the attention of stages 2 and 3): 1, 1, 2, 3, 4 and 6 key blocks,
    two utterances of different length in one launch, against the float64 softmax of the same bf16 operands within the bf16 output's rounding
    (tests/test_gpu_weight_stats.py), and bit-identical to each utterance launched alone."""
    lib = _lib.load()
    heads, dim, t, bsz = 4, 4 * d, tg, 2
    lens = [t, max(1, t - max(3, t // 3))]
    g = torch.Generator().manual_seed(1000 * d + tg)
    qu, k, v = (torch.randn(bsz, t, dim, generator=g, dtype=torch.float64) for _ in range(3))
    dv = torch.randn(dim, generator=g, dtype=torch.float64)            # v - u
    e = torch.randn(2 * t - 1, dim, generator=g, dtype=torch.float64)
    bf = lambda z: z.to(torch.bfloat16).double()
    qu, k, v, dv, e = bf(qu), bf(k), bf(v), bf(dv), bf(e)
    split = lambda z, rows: z.reshape(z.shape[0], rows, heads, d).transpose(1, 2)
    quh, kh, qvh, vh = split(qu, t), split(k, t), split(qu + dv, t), split(v, t)
    eh = split(e.unsqueeze(0), 2 * t - 1)[0]
    i, j = torch.arange(t).unsqueeze(1), torch.arange(t).unsqueeze(0)
    rel = torch.gather(qvh @ eh.transpose(1, 2), 3, (t - 1 + j - i).expand(bsz, heads, t, t))
    s = (quh @ kh.transpose(2, 3) + rel) / d ** 0.5
    masked = (torch.arange(t).unsqueeze(0) >= torch.tensor(lens).unsqueeze(1)).double()[:, None, None, :]
    want = ((s + masked * -1e9).softmax(-1) @ vh).transpose(1, 2).reshape(bsz, t, dim)

    dpad = (d + 31) // 32 * 32
    dvu = torch.zeros(heads, dpad, dtype=torch.float32)
    for hh in range(heads):
        dvu[hh, :d] = dv[hh * d + torch.arange(d)].float()
    dvu = dvu.cuda().contiguous()
    got = _attention(lib, qu, k, v, e, dvu, dpad, lens, heads, t, dim)
    for b in range(bsz):
        n = lens[b]
        diff = (got[b, :n].double().cpu() - want[b, :n]).abs()
        scale = max(float(want[b, :n].abs().max()), 1.0)
        mx, mean = float(diff.max()) / scale, float(diff.mean()) / scale
        print("attention d %d Tg %d utterance %d (%d frames): %.2e / %.2e" % (d, tg, b, n, mx, mean))
        assert mx < BF16_MAX and mean < BF16_MEAN, (b, mx, mean)
        alone = _attention(lib, qu[b:b + 1], k[b:b + 1], v[b:b + 1], e, dvu, dpad, [n], heads, t, dim)
        assert torch.equal(alone[0, :n], got[b, :n]), (b, float((alone[0, :n].float() - got[b, :n].float()).abs().max()))


def test_forty_ragged_forwards_on_one_and_three_streams_are_bit_identical():
    """One ragged batch of six utterances, 20 forwards as one row range on one stream and 20 as three row ranges on three streams: all 40 outputs equal.  The
    ring protocol (counted waits against the weight DMAs) is what a change of instruction schedule can break; a race shows as a rare rounding-size difference."""
    m = _small()
    enc = m.encoder
    lens = np.array([int(16000 * s) for s in (8.3, 7.1, 5.2, 4.4, 3.4, 1.5)], dtype=np.int64)
    audio = torch.from_numpy(synth.make_audio(lens, seed=8)).cuda()
    ln = torch.from_numpy(lens).cuda()
    enc.ragged = True
    ref = None
    for nsub in (1, 3):
        enc.sub_batches = nsub
        for it in range(20):
            out, out_len, _ = enc(audio, ln, x_len_host=lens)
            torch.cuda.synchronize()
            if ref is None:
                ref = (out.clone(), out_len.clone())
                assert bool(torch.isfinite(ref[0].float()).all())
            assert torch.equal(out_len, ref[1]) and torch.equal(out, ref[0]), (nsub, it, float((out.float() - ref[0].float()).abs().max()))
