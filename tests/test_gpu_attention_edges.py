"""-m gpu: the attention kernels alone (attention2.hip variants 1 and 2, attention.hip) at band, causal and ragged edges, against the float64 reference.

Every case of tests/attention_cases.py goes through effconf_debug_relpos_attention (the diagnostics library: AttnParams with the band, the causal flag and the
ragged descriptors of launch_lengths_ragged, routed by attention_route) on operands with 512 bytes of NaN patterns behind qu / k / v / e - the masked tail
paths of the kernel are what keeps them out - and an output pre-filled with a sentinel.  The stored output is held to the bounds of the ``attention`` stage
of tests/bf16_parity.py check_trace, unchanged: stage_ratios(got, o64, float32 run with P rounded, max(d, Tg), bf16, share factor 2) and element-wise
2^-7 sum_j p_ij |v_j| + 2e-5; every ratio <= 1.  Every row of a rectangular case counts, dead rows included (queries whose whole band lies in the padding:
uniform average over all Tg key groups; tests/test_attention_cases_host.py proves that rule); ragged cases compare every frame and require the
group-padding rows to be zero.  Variants 2 and 0 run where a forward can run them (full context, rectangular) and are held to the same bounds.
profiles/attention_edges.txt holds the lines of the first passing run."""
import pytest
import torch

import attention_cases as A
from attention_cases import CASES, F32, F64
from efficientconformer_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = 777.0


def _dev_bf16(z):
    """bf16 copy of z on the device with 512 bytes of NaN patterns behind the last row."""
    flat = torch.full((z.numel() + 256,), float("nan"), dtype=torch.bfloat16, device="cuda")
    flat[:z.numel()] = z.reshape(-1).to(torch.bfloat16).cuda()
    return flat


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_attention_kernels_at_band_causal_and_ragged_edges_vs_float64(case):
    lib = _lib.load_debug()
    torch.set_num_threads(16)
    D, H, G, d, dpad, tp, tg = A.dims(case)
    ops = A.operands(case)
    with torch.no_grad():
        o64, env = A.reference(case, ops, F64)
        o32, _ = A.reference(case, ops, F32, round_p=True)
    live = A.live_rows(case)
    B = len(case.lens)
    qud, kd, vd, ed = (_dev_bf16(ops[n]) for n in ("qu", "k", "v", "e"))
    dvu = torch.zeros(H, dpad, dtype=torch.float32)
    for h in range(H):
        dvu[h, :d] = ops["dv"][(h * d + torch.arange(d)) % D].float()            # pack.hip dvu_table
    dvu = dvu.cuda().contiguous()
    lens_h = torch.tensor(case.lens, dtype=torch.int64)
    lens_d = lens_h.cuda()
    ws = torch.zeros(7 * B + 8, dtype=torch.int32, device="cuda")
    rows = o64.shape[0]
    outs, fails = {}, []
    for variant in case.variants:
        out = torch.full((rows, D), SENTINEL, dtype=torch.bfloat16, device="cuda")
        _lib.check(lib.effconf_debug_relpos_attention(qud.data_ptr(), kd.data_ptr(), vd.data_ptr(), ed.data_ptr(), dvu.data_ptr(), dpad, lens_d.data_ptr(), lens_h.data_ptr(),
                                                      B, H, case.frames, G, D, out.data_ptr(), D, variant, case.band[0], case.band[1], int(case.causal), int(case.ragged),
                                                      ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream().cuda_stream), "debug_relpos_attention", lib)
        torch.cuda.synchronize()
        got = out.double().cpu()
        outs[variant] = got
        assert bool(torch.isfinite(got).all()), (case.name, variant, "NaN / inf in the output: a load behind a buffer's end reached the result")
        assert not bool((got == SENTINEL).any()), (case.name, variant, "output rows left unwritten")
        if case.ragged:
            assert float(got[~live].abs().sum()) == 0.0, (case.name, "group-padding rows are not zero")
        r = A.ratios(case, got[live], o64[live], o32[live], env[live])
        print("attention_edges | %-28s | variant %d | rows %4d | %s" % (case.name, variant, int(live.sum()), "  ".join("%s %.3g" % kv for kv in sorted(r.items()))))
        for stat, v in r.items():
            if not v <= 1.0:
                err = (got - o64).abs() / (2.0 ** -7 * env + 2e-5)
                i = int(err.max(-1).values.argmax())
                fails.append("variant %d %s: %.3g x its bound (worst row %d of %d, column %d)" % (variant, stat, v, i, rows, int(err[i].argmax())))
    for variant, got in outs.items():
        if variant != case.variants[0]:
            ref = outs[case.variants[0]]
            print("attention_edges | %-28s | variant %d against variant %d: %.4f of the elements equal, largest distance %.3g of the envelope bound" % (
                case.name, variant, case.variants[0], float((got == ref).double().mean()), float(((got - ref).abs() / (2.0 ** -7 * env + 2e-5)).max())))
    assert not fails, (case.name, fails)
