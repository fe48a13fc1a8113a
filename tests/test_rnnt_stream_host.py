"""The streaming RNN-T greedy decode on the CPU (tests/rnnt_stream_ref.py): the specification with the explicit carried state (h, c, gd, primed) gives, for the
cases and push patterns of tests/test_gpu_rnnt_stream.py and in float32 and float64, exactly the tokens of the oracle's whole-utterance greedy_decode; LSTM
steps = tokens + 1 (0 for a stream without a frame); the boundary invariant and the per-push token bound are asserted inside the helper at every push.  The
inputs reach every condition the GPU test must have seen, and each fault a GPU implementation could have - a decoder step re-run at the start of every push,
h / c zeroed at a push, gd not carried (a neighbour's stale one read), the start token not consumed on a fresh stream - changes the tokens of at least one
utterance of the smallest case (which patterns show it is printed); emission frames that are not offset by the frames already consumed leave the tokens alone by
construction and change the emission frames instead.  Then the C ABI: the five entries are declared, bound and exported, their host-side refusals name the
reason, the state size is the documented layout, and Transducer.open_stream on a non-causal configuration is refused."""
import ctypes as C
import os
import re

import pytest
import torch

import rnnt_shapes as S
import rnnt_stream_ref as R
from efficientconformer_amd import Transducer, _lib, named_config
from oracle.ref_transducer import greedy_decode

ENTRIES = ("effconf_rnnt_stream_state_bytes", "effconf_rnnt_stream_init", "effconf_rnnt_stream_reset", "effconf_rnnt_stream_workspace_bytes",
           "effconf_rnnt_greedy_resume")
# float32 oracle at bias 1.2: tokens, forced decisions, utterances with a token on a full push's last frame and blank-only pushes under the patterns 3 / 4 / 5
TABLE = {(20, 36, 44, 37): (298, 59, (11, 12, 7), (7, 6, 4)),
         (12, 20, 28, 9): (229, 45, (10, 7, 5), (14, 13, 9)),
         (200, 320, 320, 1000): (529, 104, (16, 12, 10), (2, 1, 0))}


_WHOLE = {}


def _whole(case, dtype):
    if (case, dtype) not in _WHOLE:
        dims, bias = case
        f, lens = R.inputs(dims)
        _WHOLE[case, dtype] = greedy_decode(R.weights(dims, bias), torch.from_numpy(f), lens, S.MAX_CONSEC, dtype=dtype)
    return _WHOLE[case, dtype]


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64), ids=("float32", "float64"))
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_chunked_decode_gives_the_whole_utterance_tokens(case, dtype):
    dims, bias = case
    _, lens = R.inputs(dims)
    assert lens.min() == 0 and sorted(lens)[1] == 1 and any(int(n) % R.KF for n in lens)
    whole = _whole(case, dtype)
    first = None
    for pattern in R.PATTERNS:
        out, rounds_listed = R.reference(case, pattern, dtype)
        assert out["tokens"] == whole, (case, pattern)
        for b, n in enumerate(lens):
            assert out["steps"][b] == (len(whole[b]) + 1 if n else 0), (case, pattern, b)
            assert out["primed"][b] == bool(n)
            fr = out["frames"][b]
            assert fr == sorted(fr) and all(0 <= t < n for t in fr) and len(fr) == len(whole[b])
        # a primed stream runs no decoder step before its first token: a blank-only resumed push has none
        assert all(r["steps"] == r["tokens"] + (0 if r["primed"] else 1) for r in out["records"] if r["frames"])
        # the final state and the emission frames do not depend on the pattern
        sig = (out["frames"], [t.tolist() for b, t in enumerate(out["h"]) if lens[b]], [t.tolist() for b, t in enumerate(out["gd"]) if lens[b]])
        first = first or sig
        assert sig == first, (case, pattern)
    print("%s %s: %d tokens" % (R.case_id(case), dtype, sum(len(t) for t in whole)))


@pytest.mark.parametrize("dims", list(TABLE), ids=lambda d: "x".join(map(str, d)))
def test_the_inputs_are_the_ones_the_cases_were_chosen_for(dims):
    """The float32 counts the cases were chosen by: a change of the seeds, the lengths or the patterns shows here."""
    case = (dims, 1.2)
    tokens, forced, last_frame, blank_only = TABLE[dims]
    whole = _whole(case, torch.float32)
    assert sum(len(t) for t in whole) == tokens
    got_last, got_blank = [], []
    for pattern in ("3", "4", "5"):
        out, _ = R.reference(case, pattern)
        recs = [r for r in out["records"] if r["frames"]]
        got_last.append(len({r["stream"] for r in recs if r["last_frame_tokens"] and r["frames"] == int(pattern)}))      # on a full push's last frame
        got_blank.append(sum(1 for r in recs if r["tokens"] == 0))
    # forced decisions: a frame that holds max_consec tokens ends in one
    out, _ = R.reference(case, "12")
    got_forced = sum(1 for fr in out["frames"] for t in set(fr) if fr.count(t) == S.MAX_CONSEC)
    print(dims, sum(len(t) for t in whole), got_forced, got_last, got_blank)
    assert (got_forced, tuple(got_last), tuple(got_blank)) == (forced, last_frame, blank_only)


def test_the_cases_reach_every_condition():
    seen = set()
    for case in R.CASES:
        _, lens = R.inputs(case[0])
        for pattern in R.PATTERNS:
            out, rounds_listed = R.reference(case, pattern)
            seen |= R.conditions(out["records"], lens, rounds_listed)
    assert seen == set(R.CONDITIONS), set(R.CONDITIONS) - seen


@pytest.mark.parametrize("fault", R.FAULTS)
def test_the_token_check_sees_the_fault(fault):
    case = R.SMALLEST
    whole = _whole(case, torch.float32)
    changed, moved = set(), set()
    for pattern in R.PATTERNS:
        good, _ = R.reference(case, pattern)
        bad, _ = R.reference(case, pattern, torch.float32, fault)
        ch = [b for b in range(len(whole)) if bad["tokens"][b] != whole[b]]
        mv = [b for b in range(len(whole)) if bad["frames"][b] != good["frames"][b]]
        print("%s under pattern %s: tokens of %s, frames of %s" % (fault, pattern, ch, mv))
        changed |= set(ch)
        moved |= set(mv)
        if pattern == "12":       # one push for a whole utterance resumes nothing: only the fresh-stream fault can show
            assert bool(ch) == (fault == "start_not_consumed"), (fault, ch)
    if fault == "frames_not_offset":
        assert not changed and moved, fault
    else:
        assert changed, fault


def test_the_step_count_sees_a_start_token_that_is_not_consumed():
    """The milder form of that fault - gd rebuilt from the zero state instead of read as it lies - moves the first logits by what the LSTM's biases (< 0.06 here)
    make of a zero input, too little to change a token of these cases: it is the step count that shows it."""
    dims, bias = R.SMALLEST
    f, lens = R.inputs(dims)
    sd = {k: torch.from_numpy(v) for k, v in R.weights(dims, bias).items()}
    wd, bd = sd["joint_network.linear_decoder.weight"], sd["joint_network.linear_decoder.bias"]
    assert max(float(sd["decoder.rnn.bias_ih_l0"].abs().max()), float(sd["decoder.rnn.bias_hh_l0"].abs().max())) < 0.06
    out = R.chunked_greedy(sd, f, R.all_pushes("3", lens), fault="start_not_consumed", fresh_gd=wd @ torch.zeros(dims[1]) + bd)
    assert [out["steps"][b] for b in range(len(lens))] == [len(out["tokens"][b]) for b in range(len(lens))]


# ------------------------------------------------------------------ the C ABI
def test_stream_entries_are_declared_bound_and_exported():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "effconf.h")).read()
    declared = set(re.findall(r"\b(effconf_rnnt_\w+)\s*\(", hdr))
    assert set(ENTRIES) <= declared
    assert set(ENTRIES) <= set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert len(_lib.SIGNATURES["effconf_rnnt_greedy_resume"][1]) == 16


def test_sizes_and_refusals_before_any_launch():
    lib = _lib.load()
    up = lambda x: (x + 255) // 256 * 256
    for (de, h, j, v), _ in R.CASES:
        r = lib.effconf_rnnt_create(C.byref(_lib.EcRnntConfig(de, h, j, v, 1, S.MAX_CONSEC, 0, 0)))
        assert r
        for streams in (1, 20, 65):
            # i32 primed[streams], then per stream h[H], c[H], gd[J]; every region on 256 bytes, one slack for the base's alignment
            assert lib.effconf_rnnt_stream_state_bytes(r, streams) == up(4 * streams) + streams * up(4 * (2 * h + j)) + 256
        assert lib.effconf_rnnt_stream_state_bytes(r, 0) == 0 and b"max_streams" in lib.effconf_last_error()
        assert lib.effconf_rnnt_stream_workspace_bytes(r, 3, 5) == 3 * 5 * j * 4 + 256
        assert lib.effconf_rnnt_stream_workspace_bytes(r, 0, 5) == 256
        assert lib.effconf_rnnt_stream_workspace_bytes(r, -1, 5) == 0 and lib.effconf_rnnt_stream_workspace_bytes(r, 3, 0) == 0
        assert b"t_new" in lib.effconf_last_error()
        # the decoder workspace of the whole-utterance decode is what it was
        assert lib.effconf_rnnt_workspace_bytes(r, 3, 5) >= 3 * 5 * j * 4
        # a handle that is not finalized is refused before anything is touched (null pointers everywhere)
        assert lib.effconf_rnnt_greedy_resume(r, None, 4, None, None, None, 2, 3, None, None, None, None, 15, None, 0, None) != 0
        assert b"not finalized" in lib.effconf_last_error()
        assert lib.effconf_rnnt_stream_init(r, None, 0, 4, None) != 0
        assert lib.effconf_rnnt_stream_reset(r, None, 4, 4, None) != 0
        lib.effconf_rnnt_destroy(r)


def test_open_stream_on_a_non_causal_configuration_is_refused():
    m = Transducer.from_config(named_config("TinyTransducer"))
    with pytest.raises(_lib.EffconfError, match="causal"):
        m.open_stream(2)
    cfg = named_config("TinyTransducer")
    cfg["encoder_params"] = dict(cfg["encoder_params"], causal=True)
    m = Transducer.from_config(cfg)
    m.encoder.precision = "split"
    with pytest.raises(_lib.EffconfError, match="bf16"):
        m.open_stream(2)
    # the decoder alone has no CPU path either
    with pytest.raises(RuntimeError, match="HIP device"):
        Transducer.from_config(cfg).open_decode_stream(2)


def test_both_greedy_kernels_keep_four_waves_and_no_scratch():
    """The resumed kernel beside the whole-utterance one it shares its body with (tests/test_kernel_resources_host.py holds the latter and the other decoders)."""
    import test_kernel_resources_host as K
    if K._hipcc() is None:
        pytest.skip("hipcc not found")
    res = K._REMARKS.get("rnnt.hip") or K._compile("rnnt.hip")
    for kernel in ("rnnt_greedy_kernel", "rnnt_greedy_resume_kernel"):
        assert kernel in res, (kernel, sorted(res))
        got = res[kernel]
        print("%s: %d VGPRs, %d waves/SIMD, %d scratch bytes/lane" % (kernel, got["vgpr"], got["occupancy"], got["scratch"]))
        assert got["occupancy"] == 4 and got["scratch"] == 0 and got["vgpr"] <= 128, got
