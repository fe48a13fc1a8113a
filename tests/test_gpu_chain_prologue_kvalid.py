"""-m gpu tests of the chains' one-round-trip prologue (csrc/chain.hip) and of the dropped all-pad k-step (rowstat.h ks_skip_last; chain.hip, chain2.hip, chain3.hip).

Three-block encoders of the Small topology (one block per stage, strided / expanding blocks 0 and 1), so that the second and third widths of ``dims`` are the
stages of 12 and 16 k-steps:

    width   last k-step                         rule
    168     all pad (columns 176 .. 191)        dropped, 12 k-steps
    176     all pad, exactly 11 valid k-steps   dropped
    184     half valid                          kept
    192     no pad                              kept
    240     all pad, 16 k-steps                 dropped (chain2.hip / chain3.hip, and chain.hip with chain_pair = 0)
    248     half valid                          kept
    120     8 k-steps, half valid               kept

and, for the prologue, ragged batches whose 168-wide stage has M = 1, 31, 33, 255, 256, 257 rows: the last workgroup's clamped loads and masked stores with
one row, one row short of / one row into the second wave, and one row short of / exactly / one row into the second 256-row workgroup.

Every case: (a) the traced stages x_mhsa, glu, the next block's x_ffn1 and out inside the stage bounds of the rounding-aware reference
(tests/bf16_parity.py check_trace: a k-step dropped that holds a valid column leaves 8 of 184 / 248 columns out of every product - far outside them);
(b) outputs equal by value between the 2-wave chain workgroups and the 8-wave ones; (c) between one row range and three; (d) every utterance of the ragged
batch equal to the utterance run alone.  Dropping additions of +-0 can turn an accumulator that is exactly -0.0 into +0.0: torch.equal compares values."""
import numpy as np
import pytest
import torch

from efficientconformer_amd import synth
from bf16_parity import check_trace
from test_gpu_bf16_rounding import _model

pytestmark = pytest.mark.gpu

_MODELS = {}
# the stages the chains write: x_ffn1 / out (chain A), x_mhsa (chain B's first GEMM), glu (chain B).  The other stages of check_trace run kernels that did not
# change, and their share-of-correctly-rounded-outputs statistics need thousands of rows (tests/test_gpu_bf16_rounding.py: with the float32 runs expecting less
# than one flipped tie per tensor a single one is "inf x its bound") - they are printed, not asserted, at these row counts
_STAGES = ("chainA", "outproj", "glu")


def _encoder(dims):
    if dims not in _MODELS:
        extra = {"dim_model": list(dims), "num_blocks": 3, "strided_blocks": [0, 1], "expand_blocks": [0, 1], "subsampling_filters": [dims[0]]}
        _MODELS[dims] = _model("EfficientConformerCTCSmall", "synthetic", extra)
    m, sd = _MODELS[dims]
    enc = m.encoder
    assert [b.dim_model for b in enc.plan.blocks] == list(dims)
    enc.ragged, enc.sub_batches = False, 1
    enc.set_option("chain_small_m", 4096)
    enc.set_option("chain_pair", 5)
    return enc, sd


def _frames(rows):
    """mel frames of an utterance with ``rows`` rows at the second stage (the stride-2 subsampling, then the stride-2 block 0)"""
    return 4 * rows - 3


def _run(enc, mel, ln, lens, ragged, nsub=1):
    enc.ragged, enc.sub_batches = ragged, nsub
    out, out_len, _ = enc.forward_mel(mel, ln, x_len_host=lens if ragged else None)
    torch.cuda.synchronize()
    return out.clone(), out_len.clone()


def _same(a, b, what):
    assert torch.equal(a[1], b[1]), what
    for u, n in enumerate(a[1].tolist()):
        x, y = a[0][u, :n], b[0][u, :n]
        assert torch.equal(x, y), (what, u, float((x.float() - y.float()).abs().max()))


def _check(dims, lens, ragged, label):
    torch.set_num_threads(16)
    enc, sd = _encoder(dims)
    plan = enc.plan
    lens = np.asarray(lens, dtype=np.int64)
    tm = int(lens.max())
    mel, ln = synth.make_mel(len(lens), plan.n_mels, tm, [int(v) for v in lens], seed=811 + tm)
    mel_d, ln_d = torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda()

    # (a) every stage against the rounding-aware reference, teacher forced
    enc.ragged = ragged
    out, out_len, got = enc.trace_forward_mel(mel_d, ln_d, arena_bytes=1 << 28)
    assert bool(torch.isfinite(out.float()).all())
    rep = check_trace(got, out_len.cpu().tolist(), plan, sd, ln, tm, ragged, 1, label)
    try:
        rep.finish()                                              # prints the worst statistic / bound ratio of every stage
    except AssertionError:
        pass
    mine = [f for f in rep.fails if f.split()[2] in _STAGES]
    assert not mine, "%d statistics over their bound, first: %s" % (len(mine), " || ".join(mine[:6]))

    # (b) 2-wave chain workgroups against the 8-wave ones (chain3.hip / chain2.hip at the last stage either way), both layouts
    res = {}
    for small in (1 << 30, 0):
        enc.set_option("chain_small_m", small)
        res[small] = [_run(enc, mel_d, ln_d, lens, r) for r in (False, True)]
    for r in (0, 1):
        _same(res[1 << 30][r], res[0][r], "2-wave against 8-wave workgroups, ragged %d" % r)
    # ... and chain.hip's own instance of the widest stage (chain_pair = 0) against chain3.hip / chain2.hip
    enc.set_option("chain_pair", 0)
    _same(_run(enc, mel_d, ln_d, lens, True), res[0][1], "chain.hip against chain3.hip / chain2.hip")
    enc.set_option("chain_pair", 5)
    enc.set_option("chain_small_m", 4096)

    # (c) one row range against three
    one = _run(enc, mel_d, ln_d, lens, True, 1)
    _same(_run(enc, mel_d, ln_d, lens, True, 3), one, "three row ranges against one")
    _same(one, res[0][1], "default shapes against 8-wave workgroups")

    # (d) every utterance alone
    for u, n in enumerate(lens.tolist()):
        m1, l1 = torch.from_numpy(np.ascontiguousarray(mel[u:u + 1, :, :n])).cuda(), torch.from_numpy(ln[u:u + 1].copy()).cuda()
        alone = _run(enc, m1, l1, lens[u:u + 1], True, 1)
        k = int(one[1][u])
        assert int(alone[1][0]) == k
        assert torch.equal(alone[0][0, :k], one[0][u, :k]), ("utterance alone", u, float((alone[0][0, :k].float() - one[0][u, :k].float()).abs().max()))


@pytest.mark.parametrize("dims,ragged", [((120, 168, 240), False), ((120, 176, 248), True), ((120, 184, 240), True), ((120, 192, 248), False)],
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else ("ragged" if v else "rect"))
def test_widths_that_decide_the_valid_k_step_rule(dims, ragged):
    _check(dims, [300, 233, 121, 40], ragged, "kvalid %s" % (dims,))


@pytest.mark.parametrize("rows", [(1,), (20, 11), (32, 1), (200, 55), (129, 127), (256, 1)], ids=lambda r: "M=%d" % sum(r))
def test_row_counts_that_decide_the_prologue_at_width_168(rows):
    assert sum(rows) in (1, 31, 33, 255, 256, 257)
    _check((120, 168, 240), [_frames(r) for r in rows], True, "prologue M = %d" % sum(rows))
