"""The cases of tests/test_gpu_rnnt_shapes.py on the CPU (tests/rnnt_shapes.py): the float64 references alone stay inside what the GPU tests may
excuse, and the margin rule sees the faults it is there for.

Faults (rnnt_shapes.standin_greedy, torch float32): linear_decoder's output read at pitch H instead of J, the last 16-block of k dropped from
W_hh, the vocabulary's tail tile masked, one vocabulary slice's argmax candidates dropped.  Each breaks the token check on at least one case.
The first is invisible wherever H = J - here (200, 320, 320, 1000), and both shapes every decoder test ran before these cases."""
import numpy as np
import pytest
import torch

import rnnt_shapes as S
from oracle.ref_transducer import greedy_decode


@pytest.mark.parametrize("dims", list(S.GREEDY_CASES))
def test_greedy_reference_stays_inside_the_excuse_cap(dims):
    tr = S.greedy_trace(dims)
    f, lens = S.greedy_inputs(dims)
    assert lens.min() == 0 and sorted(lens)[1] == 1 and lens.max() == S.GREEDY_T
    # the trace is the oracle's float64 decode
    assert tr.tokens == greedy_decode(S.weights(dims, S.GREEDY_CASES[dims]), torch.from_numpy(f), lens, S.MAX_CONSEC, dtype=torch.float64)
    assert sum(len(t) for t in tr.tokens) >= 20
    assert 0 < tr.noise < 1e-4, tr.noise                      # float32 against float64 on logits of a few units
    excused = S.check_greedy(tr, tr.tokens, "float64")
    print("%s: noise %.3g, margin bound %.3g, smallest margin %.3g, excused %s" % (dims, tr.noise, S.MARGIN_FACTOR * tr.noise, tr.smallest, excused))
    # the same program in float32, free running, and the stand-in without a fault
    assert S.check_greedy(tr, S.greedy_float32(dims), "float32") == excused
    assert S.check_greedy(tr, S.standin_greedy(dims), "stand-in") == excused


@pytest.mark.parametrize("fault", S.FAULTS)
def test_the_token_check_sees_the_fault(fault):
    seen = []
    for dims in S.GREEDY_CASES:
        try:
            S.check_greedy(S.greedy_trace(dims), S.standin_greedy(dims, fault), fault)
        except AssertionError:
            seen.append(dims)
    print(fault, "seen at", seen)
    assert seen, fault
    if fault == "gd_pitch":
        assert (200, 320, 320, 1000) not in seen and all(d[1] != d[2] for d in seen)         # H = J hides a pitch taken from the wrong one
        assert set(seen) == {d for d in S.GREEDY_CASES if d[1] != d[2]}
    if fault == "vocab_tail":
        assert all(d[3] % 16 for d in seen)


@pytest.mark.parametrize("dims", list(S.BEAM_CASES))
def test_beam_reference_in_float32_gives_the_float64_tokens(dims):
    f, lens = S.beam_inputs(dims)
    assert lens.min() == 0 and sorted(lens)[1] == 1
    for beam in S.BEAMS:
        r64, r32 = S.beam_oracle(dims, beam), S.beam_oracle(dims, beam, False)
        differ = [i for i in range(len(r64)) if r64[i]["tokens"] != r32[i]["tokens"] or r64[i]["capped"] != r32[i]["capped"]]
        print("%s beam %d: capped %s, tokens %d, float32 differs at %s" % (dims, beam, [i for i, r in enumerate(r64) if r["capped"]],
                                                                             sum(len(r["tokens"]) for r in r64), differ))
        assert not differ, (dims, beam, differ)                # the GPU test asks for identity on every row: no near tie may sit in these seeds
        for a, b in zip(r64, r32):
            assert abs(a["score"] - b["score"]) <= 1e-4 * abs(a["score"])
    assert any(not r["capped"] and r["tokens"] for beam in S.BEAMS for r in S.beam_oracle(dims, beam))


def test_every_case_is_taken_or_refused_before_any_launch():
    """The workspace queries and the route entry need no finalize: every beam and lattice case is taken, the widths outside are refused by message."""
    import ctypes as C

    from efficientconformer_amd import _lib
    lib = _lib.load()

    def handle(dims):
        h = lib.effconf_rnnt_create(C.byref(_lib.EcRnntConfig(*dims, 1, S.MAX_CONSEC, 0, 0)))
        assert h
        return h

    for dims in S.BEAM_CASES:
        h = handle(dims)
        assert all(lib.effconf_rnnt_beam_workspace_bytes(h, S.BEAM_BATCH, S.BEAM_T, beam, 16 * beam, 16 * S.BEAM_T) > 0 for beam in S.BEAMS), dims
        lib.effconf_rnnt_destroy(h)
    for dims in S.LATTICE_CASES + [(24, 800, 64, 33)]:            # 3 x 16 x 800 floats: exactly the lattice's 150 KB
        h = handle(dims)
        assert lib.effconf_rnnt_lattice_workspace_bytes(h, S.LATTICE_BATCH, S.LATTICE_T, 14) > 0, dims
        lib.effconf_rnnt_destroy(h)
    h = handle((24, 816, 64, 33))
    assert lib.effconf_rnnt_lattice_workspace_bytes(h, 2, 3, 1) == 0 and b"exceed the LDS of one workgroup" in lib.effconf_last_error()
    lib.effconf_rnnt_destroy(h)
    h = handle((20, 36, 44, 37))
    assert lib.effconf_rnnt_lattice_workspace_bytes(h, 2, 3, 1) == 0 and b"rnnt lattice: decoder and joint widths must be multiples of 16" in lib.effconf_last_error()
    assert lib.effconf_rnnt_beam_workspace_bytes(h, 2, 3, 4, 64, 48) == 0 and b"beam search: decoder and joint widths must be multiples of 16" in lib.effconf_last_error()
    lib.effconf_rnnt_destroy(h)
    for dims, (has_a, has_b) in S.GREEDY_CLUSTERS.items():       # the routes the GPU test forces exist
        h = handle(dims)
        assert lib.effconf_rnnt_set_option(h, b"cluster_decode", 1) == 0
        assert lib.effconf_rnnt_greedy_route(h, S.GREEDY_BATCH) == (1 if has_a else 0), dims
        assert lib.effconf_rnnt_set_option(h, b"cluster_shape", 1) == 0
        assert lib.effconf_rnnt_greedy_route(h, S.GREEDY_BATCH) == (2 if has_b else 1 if has_a else 0), dims
        lib.effconf_rnnt_destroy(h)


@pytest.mark.parametrize("dims", S.LATTICE_CASES)
def test_lattice_cases_hold_their_edges(dims):
    f, lens, targets = S.lattice_inputs(dims)
    assert f.shape == (S.LATTICE_BATCH, S.LATTICE_T, dims[0]) and len(targets) == 17
    assert targets[1] == [] and len(targets[3]) > lens[3] and len(targets[2]) > lens[2] == 1
    assert all(1 <= c < dims[3] for y in targets for c in y)
    own = S.lattice_noise(dims)
    print("%s: own float32 noise %.3g" % (dims, own))
    assert 0 < own < 1e-4
    for tmp in S.TEMPERATURES:
        for i, (lpb, lpl) in enumerate(S.lattice_oracle(dims, tmp)):
            n, u = int(lens[i]), len(targets[i])
            assert lpb.shape == lpl.shape == (n, u + 1) and np.isfinite(lpb).all() and np.isfinite(lpl[:, :u]).all() and np.isneginf(lpl[:, u]).all()
