"""CPU: the streaming session's state machine and arithmetic, without a GPU.

tests/stream_ref.py - a float64 chunked encoder with an explicit K / V cache and conv state, written from the oracle's stage functions - equals the oracle's
whole-utterance causal forward on every valid row to 1e-12 for every push pattern; the oracle itself is prefix invariant at aligned rows for causal plans and
is not without ``causal`` (the reason for the refusal); each injected fault of the state machine moves the result by more than the GPU test's bound
(tests/test_gpu_stream.py: 0.09 max / 0.012 mean), so that bound sees them; the alignment, the emission rule and the cache capacities follow a hand-written
table; the collapse carry; the refusals; the C ABI's declarations."""
import os
import re

import numpy as np
import pytest
import torch

import stream_ref
from efficientconformer_amd import ConformerEncoder, ConformerEncoderInterCTC, _lib, build_plan, named_config, streaming as S, synth
from oracle import ref_encoder as R

F64 = torch.float64
STREAM_MAX, STREAM_MEAN = 0.09, 0.012
PATTERNS = ("24", "48", "irregular", "all")


def _tiny(**extra):
    cfg = named_config("Tiny")
    params = dict(cfg["encoder_params"], **extra)
    plan = build_plan(params)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(plan, 7, cfg["tokenizer_params"]["vocab_size"]).items()}
    return plan, sd


_CACHE = {}


def _whole(extra, T):
    """(plan, sd, mel (n_mels, T), the oracle's float64 whole-utterance output rows): computed once per case, never modified."""
    key = (tuple(sorted(extra.items())), T)
    if key not in _CACHE:
        plan, sd = _tiny(**extra)
        mel, _ = synth.make_mel(1, plan.n_mels, T, [T], seed=4421)
        mel = torch.from_numpy(mel)[0].to(F64)
        torch.set_num_threads(8)
        with torch.no_grad():
            out, n = R.encoder_from_mel(mel[None], torch.tensor([T]), sd, plan, dtype=F64)
        _CACHE[key] = (plan, sd, mel, out[0, :int(n[0])])
    return _CACHE[key]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("T", (47, 100))
@pytest.mark.parametrize("extra", (dict(causal=True), dict(causal=True, left_context=12)), ids=("causal", "causal-l12"))
def test_chunked_float64_encoder_equals_the_oracle(extra, T, pattern):
    plan, sd, mel, whole = _whole(extra, T)
    with torch.no_grad():
        got = stream_ref.run(sd, plan, mel, stream_ref.pushes_of(pattern, T))
    assert got.shape == whole.shape, (got.shape, whole.shape)
    assert float((got - whole).abs().max()) <= 1e-12


@pytest.mark.parametrize("extra", (dict(causal=True), dict(causal=True, left_context=12)), ids=("causal", "causal-l12"))
def test_oracle_is_prefix_invariant_at_aligned_rows_for_causal_plans(extra):
    plan, sd, mel, whole = _whole(extra, 100)
    for cut, rows in ((25, 3), (49, 6), (73, 9), (97, 12)):       # prefix cut -> the output rows of its complete subsampled rows, counted at a multiple of 12 (3 output rows per 24 frames)
        with torch.no_grad():
            out, _ = R.encoder_from_mel(mel[None, :, :cut], torch.tensor([cut]), sd, plan, dtype=F64)
        assert float((out[0, :rows] - whole[:rows]).abs().max()) <= 1e-12, cut


def test_oracle_is_not_prefix_invariant_without_causal():
    """left_context = 7, right_context = 0 WITHOUT causal: the symmetric depthwise padding looks ahead - the reason streaming refuses such plans."""
    plan, sd, mel, whole = _whole(dict(left_context=7, right_context=0), 100)
    with torch.no_grad():
        out, _ = R.encoder_from_mel(mel[None, :, :49], torch.tensor([49]), sd, plan, dtype=F64)
    assert float((out[0, :6] - whole[:6]).abs().max()) > 1e-2


@pytest.mark.parametrize("fault", stream_ref.FAULTS)
def test_injected_faults_move_the_result_by_more_than_the_gpu_bound(fault):
    plan, sd, mel, whole = _whole(dict(causal=True, left_context=12), 100)
    with torch.no_grad():
        got = stream_ref.run(sd, plan, mel, stream_ref.pushes_of("24", 100), fault=fault, fault_chunk=2)
    if got.shape != whole.shape:
        return                                   # the fault changes the number of rows: out_len catches it
    d = (got - whole).abs()
    print("fault %-40s moves the output by max %.3f mean %.4f" % (fault, float(d.max()), float(d.mean())))
    assert float(d.max()) > STREAM_MAX or float(d.mean()) > STREAM_MEAN, (fault, float(d.max()), float(d.mean()))


# ------------------------------------------------------------------ arithmetic
def test_stream_align_is_12_rows_for_tiny_and_every_efficient_configuration():
    from efficientconformer_amd.config import _NAMED
    names = ["Tiny"] + [n for n in _NAMED if n.startswith("EfficientConformer")]
    assert len(names) > 3
    for name in names:
        plan = build_plan(dict(named_config(name)["encoder_params"], causal=True))
        assert S.stream_align(plan) == 12, name


def test_emission_rule_follows_the_hand_written_table():
    #        frames  done  final -> rows
    table = [(0, 0, False, 0), (23, 0, False, 0), (24, 0, False, 12), (25, 0, False, 12), (47, 0, False, 12), (48, 0, False, 24), (48, 12, False, 12),
             (57, 12, False, 12), (71, 24, False, 0), (72, 24, False, 12), (7, 0, True, 4), (8, 0, True, 4), (9, 0, True, 5), (47, 12, True, 12), (100, 48, True, 2),
             (24, 12, True, 0), (25, 12, True, 1), (0, 0, True, 0), (1, 0, True, 1)]
    for frames, done, final, rows in table:
        assert S.rows_to_encode(frames, done, 12, final) == rows, (frames, done, final)
    # rows leaving the encoder: T -> (T - 1) // 2 + 1 behind each of Tiny's two strided blocks
    plan = build_plan(dict(named_config("Tiny")["encoder_params"], causal=True))
    assert [S.block_rows(plan, r)[-1] for r in (12, 24, 5, 2, 1)] == [3, 6, 2, 1, 1]


def test_cache_capacities_follow_the_band_of_the_whole_utterance_forward():
    plan = build_plan(dict(named_config("Tiny")["encoder_params"], causal=True, left_context=12))
    caps = S.cache_capacities(plan)
    ms, want = 1, []
    for bp in plan.blocks:
        want.append(12 // (ms * bp.group_size))
        ms *= bp.conv_stride
    assert caps == want
    # left_context 12 at mask strides 1 / 2 / 4 with G = 3 / 1 / 1: bands 4 / 6 / 3
    by_stage = {(bp.mask_stride, bp.group_size): c for bp, c in zip(plan.blocks, caps)}
    assert by_stage[(1, 3)] == 4 and by_stage[(2, 1)] == 6 and by_stage[(4, 1)] == 3
    # an unlimited context: what max_frames brings to the block, in grouped rows
    plan = build_plan(dict(named_config("Tiny")["encoder_params"], causal=True, left_context=1 << 30))
    assert S.cache_capacities(plan) == [bp.max_pos // bp.group_size for bp in plan.blocks]      # no sequence is longer than max_pos_encoding
    caps = S.cache_capacities(plan, max_frames=100)          # 50 rows -> 17 groups of 3; 25 rows; 13 rows
    by_stage = {(bp.mask_stride, bp.group_size): c for bp, c in zip(plan.blocks, caps)}
    assert by_stage[(1, 3)] == 17 and by_stage[(2, 1)] == 25 and by_stage[(4, 1)] == 13


def test_collapse_carry():
    assert S.ctc_collapse_carry([5, 5, 0, 5], 0) == ([5, 5], 5)
    # a label repeated across a push boundary is emitted once
    a, c = S.ctc_collapse_carry([0, 3, 3], 0)
    b, c = S.ctc_collapse_carry([3, 3, 4], c)
    assert a + b == [3, 4] and c == 4
    # a repeat separated by a blank in the earlier push is emitted twice
    a, c = S.ctc_collapse_carry([3, 0], 0)
    b, c = S.ctc_collapse_carry([3], c)
    assert a + b == [3, 3]
    # an empty push in between keeps the carry
    a, c = S.ctc_collapse_carry([7], 0)
    e, c = S.ctc_collapse_carry([], c)
    b, c = S.ctc_collapse_carry([7, 2], c)
    assert a + e + b == [7, 2]
    # the head's collapsed labels + the first / last frame's label give the same as the frame labels
    rng = np.random.RandomState(3)
    for _ in range(200):
        frames = rng.randint(0, 3, size=rng.randint(1, 9)).tolist()
        carry = int(rng.randint(0, 3))
        collapsed, _ = S.ctc_collapse_carry(frames, 0)
        assert S.merge_collapsed(collapsed, frames[0], frames[-1], carry) == S.ctc_collapse_carry(frames, carry), (frames, carry)


# ------------------------------------------------------------------ refusals (before any device work)
def test_refusals_name_the_reason():
    tiny = named_config("Tiny")["encoder_params"]
    enc = ConformerEncoder(dict(tiny))
    with pytest.raises(_lib.EffconfError, match="causal"):
        enc.open_stream(1)
    enc = ConformerEncoder(dict(tiny, left_context=7, right_context=0))
    with pytest.raises(_lib.EffconfError, match="causal"):
        enc.open_stream(1)
    for precision in ("split", "fp32"):
        enc = ConformerEncoder(dict(tiny, causal=True))
        enc.precision = precision
        with pytest.raises(_lib.EffconfError, match="bf16"):
            enc.open_stream(1)
    enc = ConformerEncoder(dict(tiny, causal=True))
    enc.sub_batches = 2
    with pytest.raises(_lib.EffconfError, match="sub_batches"):
        enc.open_stream(1)
    ic = named_config("EfficientConformerInterCTCSmall") if "EfficientConformerInterCTCSmall" in __import__("efficientconformer_amd.config", fromlist=["_NAMED"])._NAMED else None
    params = dict(ic["encoder_params"] if ic else tiny, causal=True)
    if not ic:
        params.update(interctc_blocks=[1], vocab_size=32)
    enc = ConformerEncoderInterCTC(params)
    with pytest.raises(_lib.EffconfError, match="InterCTC"):
        enc.open_stream(1)
    conformer = build_plan(dict(named_config("ConformerCTCSmall")["encoder_params"], causal=True))
    assert "two-layer" in S.stream_refusal(conformer)


def test_stream_entries_are_declared_bound_and_exported():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "effconf.h")).read()
    declared = set(re.findall(r"\b(effconf_stream_\w+)\s*\(", hdr))
    want = {"effconf_stream_align", "effconf_stream_state_bytes", "effconf_stream_create", "effconf_stream_destroy", "effconf_stream_reset",
            "effconf_stream_workspace_bytes", "effconf_stream_push_mel", "effconf_stream_attention", "effconf_stream_dwconv"}
    assert want <= declared
    assert want <= set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in want:
        assert hasattr(lib, name), name
    assert lib.effconf_abi_version() == 3
