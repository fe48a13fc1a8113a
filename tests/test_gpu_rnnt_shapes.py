"""The RNN-T decoder kernels (csrc/rnnt.hip: per-utterance and cluster greedy kernels, rnnt_beam.hip, rnnt_lattice.hip) against float64 references at
widths every other decoder test leaves alone: H != J in both orders, widths that are no multiple of 16 or 64, every count of 16-blocks of k at
which decode_common.h's mat-vecs change their loads in flight (1, 3, odd and large, 20, 8 n), vocabularies below, at and just above a 16-row tile,
cluster workgroups with idle waves, empty and cut vocabulary slices and partial linear_decoder tiles.  tests/rnnt_shapes.py holds the cases, the
references and the margin rule; tests/test_rnnt_shapes_host.py keeps the references alone inside what is excused here and shows that the token
check sees a pitch taken from the wrong width, a dropped block of k, a masked tail tile and a dropped vocabulary slice.

Greedy: every route effconf_rnnt_greedy_route reports for the case is forced in turn (per utterance, 8 x 8 x 2, 16 x 16 x 1; both workgroup -> XCD
mappings), the route is asserted, and the tokens are held to the float64 decode under the margin rule: identity wherever the reference's smallest
top-2 margin is at least 32 x the case's float32 logit noise.  Measured (profiles/rnnt_shapes.txt): no utterance of any case is excused, and every
route gives the float64 tokens on all 20 utterances.
Beam search: tokens, capped rows and scores (1e-4 |ref|, the bound of tests/test_gpu_rnnt_beam.py) against rnnt_beam_ref.beam_decode in float64,
beam_eval_batch 1 and 16 bit-identical.  Measured: scores within 3.3e-7 |ref|.
Lattice planes: the assertions of tests/test_gpu_rnnt_align.py::test_lattice_planes_match_the_float64_oracle; bound 8 x the float32 noise of the
reference's own formula on the case (torch float32 against float64, computed at run time, never from the kernel).  The case's own noise is the
yardstick at every size, V = 5 included: measured, the kernel is within 0.9 .. 2.0 x that noise (4.6e-7 .. 9.9e-7; kernel 5.0e-7 .. 2.0e-6)."""
import numpy as np
import pytest
import torch

import rnnt_shapes as S
from efficientconformer_amd import _lib

pytestmark = pytest.mark.gpu

ROUTE_NAMES = {0: "per-utterance", 1: "8x8x2", 2: "16x16x1"}


def _route(m, batch):
    return _lib.load().effconf_rnnt_greedy_route(m._rnnt, batch)


def _greedy(m, f, lens):
    tokens, token_len = m.decode_encoded(f, lens)
    tokens, token_len = tokens.cpu(), token_len.cpu()
    assert all(int(tokens[i, int(token_len[i]):].abs().sum()) == 0 for i in range(tokens.shape[0]))      # zero-filled tails
    return [tokens[i, :int(token_len[i])].tolist() for i in range(tokens.shape[0])]


# ---------------------------------------------------------------------------------------------------------------- greedy
@pytest.mark.parametrize("dims", list(S.GREEDY_CASES))
def test_every_greedy_route_gives_the_float64_tokens(dims):
    m = S.native_decoder(dims, S.GREEDY_CASES[dims])
    f, lens = S.greedy_inputs(dims)
    fd, ld = torch.from_numpy(f).cuda(), torch.from_numpy(lens).cuda()
    tr = S.greedy_trace(dims)
    batch = f.shape[0]
    has_a, has_b = S.GREEDY_CLUSTERS[dims]
    runs = {}
    try:
        m.set_decode_option("cluster_decode", 0)
        assert _route(m, batch) == 0
        runs["per-utterance"] = _greedy(m, fd, ld)
        m.set_decode_option("cluster_decode", 1)
        for shape in (0, 1):
            m.set_decode_option("cluster_shape", shape)
            route = _route(m, batch)
            assert route == (2 if shape == 1 and has_b else 1 if has_a else 0), (dims, shape, route)
            if route == 0 or (shape == 1 and route != 2):
                continue                                           # nothing new to force
            for by_slice in (0, 1):
                m.set_decode_option("cluster_by_slice", by_slice)
                assert _route(m, batch) == route
                runs["%s by %s" % (ROUTE_NAMES[route], "slice" if by_slice else "cluster")] = _greedy(m, fd, ld)
    finally:
        m.set_decode_option("cluster_by_slice", 1)
        m.set_decode_option("cluster_shape", -1)
        m.set_decode_option("cluster_decode", -1)
    assert len(runs) == 1 + 2 * (has_a + has_b)
    bound = S.MARGIN_FACTOR * tr.noise
    for what, got in runs.items():
        wrong = [b for b in range(batch) if got[b] != tr.tokens[b]]
        print("%s %s: %d tokens, utterances off the float64 tokens %s; logit noise %.3g, margin bound %.3g, smallest margin %.3g"
              % (dims, what, sum(len(t) for t in got), wrong, tr.noise, bound, tr.smallest))
    excused = None
    for what, got in runs.items():
        excused = S.check_greedy(tr, got, (dims, what))
    print("%s: excused %s of %d" % (dims, excused, batch))
    strict = [b for b in range(batch) if b not in excused]
    base = runs["per-utterance"]
    for what, got in runs.items():                                 # the routes against each other
        assert [got[b] for b in strict] == [base[b] for b in strict], (dims, what)


# ---------------------------------------------------------------------------------------------------------------- beam search
def _beam(m, f, lens, beam):
    tokens, token_len, score, status = m.decode_encoded_beam(f, lens, beam)
    tokens, token_len, score, status = tokens.cpu(), token_len.cpu(), score.cpu().numpy(), status.cpu().numpy()
    assert all(int(tokens[i, int(token_len[i]):].abs().sum()) == 0 for i in range(tokens.shape[0]))
    return [tokens[i, :int(token_len[i])].tolist() for i in range(tokens.shape[0])], score, status


@pytest.mark.parametrize("beam", S.BEAMS)
@pytest.mark.parametrize("dims", list(S.BEAM_CASES))
def test_beam_search_gives_the_float64_tokens_scores_and_caps(dims, beam):
    m = S.native_decoder(dims, S.BEAM_CASES[dims])
    f, lens = S.beam_inputs(dims)
    fd, ld = torch.from_numpy(f).cuda(), torch.from_numpy(lens).cuda()
    ref = S.beam_oracle(dims, beam)
    try:
        m.set_decode_option("beam_eval_batch", 1)
        one = _beam(m, fd, ld, beam)
        m.set_decode_option("beam_eval_batch", 16)
        toks, score, status = _beam(m, fd, ld, beam)
    finally:
        m.set_decode_option("beam_eval_batch", 16)
    assert one[0] == toks and one[1].tobytes() == score.tobytes() and (one[2] == status).all()
    capped = [i for i, r in enumerate(ref) if r["capped"]]
    rscore = np.array([r["score"] for r in ref])
    live = [i for i in range(len(ref)) if i not in capped]
    dev = max([abs(float(score[i]) - rscore[i]) / abs(rscore[i]) for i in live if rscore[i] != 0] + [0.0])
    print("%s beam %d: %d tokens, capped %s (oracle %s), score vs float64 %.3g relative (bound 1e-4)"
          % (dims, beam, sum(len(t) for t in toks), [i for i in range(len(status)) if status[i] == 1], capped, dev))
    assert [i for i in range(len(status)) if status[i] == 1] == capped and all(status[i] == 0 for i in live)
    assert toks == [r["tokens"] for r in ref]
    assert all(abs(float(score[i]) - rscore[i]) <= 1e-4 * abs(rscore[i]) for i in live), (score, rscore)


# ---------------------------------------------------------------------------------------------------------------- lattice planes
@pytest.mark.parametrize("tmp", S.TEMPERATURES)
@pytest.mark.parametrize("dims", S.LATTICE_CASES)
def test_lattice_planes_match_the_float64_oracle(dims, tmp):
    m = S.native_decoder(dims)
    f, f_len, targets = S.lattice_inputs(dims)
    noise = S.lattice_noise(dims)
    bound = 8 * noise
    m.tmp = tmp
    try:
        lpb, lpl, st = m.lattice(torch.from_numpy(f).cuda(), torch.from_numpy(f_len).cuda(), targets)
    finally:
        m.tmp = 1.0
    lpb, lpl, st = lpb.cpu().numpy(), lpl.cpu().numpy(), st.cpu().numpy()
    umax = max(len(y) for y in targets)
    assert lpb.shape == lpl.shape == (f.shape[0], f.shape[1], umax + 1) and (st == 0).all()
    worst = 0.0
    for i, (ob, ol) in enumerate(S.lattice_oracle(dims, tmp)):
        n, u = int(f_len[i]), len(targets[i])
        assert not lpb[i, n:].any() and not lpb[i, :, u + 1:].any() and not lpl[i, n:].any() and not lpl[i, :, u + 1:].any(), i
        assert np.isneginf(lpl[i, :n, u]).all(), i
        assert np.isfinite(lpb[i, :n, :u + 1]).all() and np.isfinite(lpl[i, :n, :u]).all(), i
        worst = max(worst, float(np.abs(lpb[i, :n, :u + 1] - ob).max()), float(np.abs(lpl[i, :n, :u] - ol[:, :u]).max()) if u else 0.0)
    print("%s tmp %g: kernel vs float64 %.3g, float32 noise %.3g, bound %.3g" % (dims, tmp, worst, noise, bound))
    assert worst <= bound, (worst, bound)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_unsupported_widths_are_refused_by_message():
    m = S.native_decoder((20, 36, 44, 37), S.GREEDY_CASES[(20, 36, 44, 37)])           # H % 16 != 0: the greedy decode alone is native
    f, lens = S.greedy_inputs((20, 36, 44, 37))
    fd, ld = torch.from_numpy(f).cuda(), torch.from_numpy(lens).cuda()
    with pytest.raises(_lib.EffconfError, match="beam search: decoder and joint widths must be multiples of 16"):
        m.decode_encoded_beam(fd, ld, 4)
    with pytest.raises(_lib.EffconfError, match="rnnt lattice: decoder and joint widths must be multiples of 16"):
        m.lattice(fd, ld, [[1]] * f.shape[0])
    big = S.native_decoder((24, 816, 64, 33))                     # the prediction network's 3 x 16 x H floats: 153 KB, over the lattice's 150 KB (H = 784, 800: inside)
    fb = torch.zeros(2, 3, 24).cuda()
    with pytest.raises(_lib.EffconfError, match="rnnt lattice: decoder / joint widths exceed the LDS of one workgroup"):
        big.lattice(fb, None, [[1], [2]])
    wide = S.native_decoder((24, 64, 64, 1500))                   # 188 vocabulary entries per workgroup of 8: 8 x 8 x 2 is refused, 16 x 16 x 1 runs
    try:
        wide.set_decode_option("cluster_decode", 1)
        assert _route(wide, 20) == 0
        wide.set_decode_option("cluster_shape", 1)
        assert _route(wide, 20) == 2
    finally:
        wide.set_decode_option("cluster_shape", -1)
        wide.set_decode_option("cluster_decode", -1)
