"""CTC forced alignment and transcript scoring, host side: the float64 oracle (tests/ctc_align_ref.py) against torch's ctc_loss and
against brute force over every alignment, the degenerate cases, ``frame_seconds`` and the Python / C surface (no GPU needed)."""
import inspect
import itertools
import os

import numpy as np
import pytest
import torch

from ctc_align_ref import brute_force, check_path, ctc_log_prob, forward, logp64, path_logp, status_of, viterbi
from efficientconformer_amd import named_config


def _case(rng, v, t, u, scale, repeats=False):
    lp = logp64((rng.standard_normal((t, v)) * scale).astype(np.float32))
    y = rng.integers(1, v, u).tolist()
    if repeats and u > 1:
        for i in rng.integers(1, u, max(1, u // 3)):
            y[i] = y[i - 1]
    return lp, y


def test_forward_equals_ctc_loss_in_float64():
    rng = np.random.default_rng(21)
    n = 0
    for v in (2, 3, 32, 256, 1000):
        for scale in (1.0, 3.0):
            for _ in range(6):
                t = int(rng.integers(1, 400))
                u = int(rng.integers(0, max(1, min(t // 2, 120)) + 1))
                lp, y = _case(rng, v, t, u, scale, repeats=bool(rng.integers(0, 2)))
                length = int(rng.integers(max(1, t // 2), t + 1))
                if status_of(length, y, v) != 0:
                    continue
                got, want = forward(lp, length, y), ctc_log_prob(lp, length, y)
                assert abs(got - want) <= 1e-9 * (1 + abs(want)), (v, t, u, got, want)
                n += 1
    assert n >= 50


def _best_alignment(lp, y):
    """Brute force over all V^T alignments: the best log-probability among those that collapse to y."""
    t, v = lp.shape
    best = -np.inf
    for path in itertools.product(range(v), repeat=t):
        lab, prev = [], 0
        for c in path:
            if c != 0 and c != prev:
                lab.append(c)
            prev = c
        if lab == list(y):
            best = max(best, float(sum(lp[i, c] for i, c in enumerate(path))))
    return best


@pytest.mark.parametrize("v,t", [(2, 6), (3, 4), (3, 6)])
def test_viterbi_and_forward_equal_brute_force(v, t):
    rng = np.random.default_rng(100 * v + t)
    lp = logp64((rng.standard_normal((t, v)) * 2).astype(np.float32))
    total = brute_force(lp)
    targets = [(), (1,), (1, 1), (1, 1, 1)] + ([(1, 2), (2, 1, 2), (2, 2, 1), (1, 2, 2, 1)] if v == 3 else [])
    for y in targets:
        res = viterbi(lp, t, y)
        if status_of(t, y, v) != 0:
            assert y not in total and np.isneginf(forward(lp, t, y)) and np.isneginf(res["score"])
            continue
        assert abs(forward(lp, t, y) - total[y]) <= 1e-9 * (1 + abs(total[y])), y
        want = _best_alignment(lp, y)
        assert abs(res["score"] - want) <= 1e-9 * (1 + abs(want)), (y, res["score"], want)
        assert check_path(res["frame_token"], y) is None
        assert abs(path_logp(lp, res["frame_token"], y) - res["score"]) <= 1e-9 * (1 + abs(want))


def test_ties_take_the_smaller_step():
    lp = np.log(np.full((4, 3), 1.0 / 3.0))              # every path has the same probability
    res = viterbi(lp, 4, [1, 2])
    # from the end: S - 1 (the last blank) wins the end tie and is kept for as long as it can be reached; state 4 at frame 2 needs 1 -> 3 -> 4
    assert res["states"].tolist() == [1, 3, 4, 4] and res["margin"] == 0.0
    assert viterbi(lp, 4, [1])["states"].tolist() == [1, 2, 2, 2]


def test_degenerate_cases():
    rng = np.random.default_rng(5)
    lp = logp64(rng.standard_normal((5, 4)).astype(np.float32))
    assert forward(lp, 0, []) == 0.0 and viterbi(lp, 0, [])["score"] == 0.0
    assert np.isneginf(forward(lp, 0, [1])) and status_of(0, [1], 4) == 1
    assert forward(lp, 5, []) == pytest.approx(float(lp[:, 0].sum()), abs=1e-12)
    res = viterbi(lp, 5, [])
    assert res["score"] == pytest.approx(float(lp[:, 0].sum()), abs=1e-12) and (res["frame_token"] == -1).all()
    # U + repeats frames are needed: [2, 2, 3] needs 4
    assert status_of(3, [2, 2, 3], 4) == 1 and np.isneginf(forward(lp, 3, [2, 2, 3])) and np.isneginf(viterbi(lp, 3, [2, 2, 3])["score"])
    assert status_of(4, [2, 2, 3], 4) == 0
    res = viterbi(lp, 4, [2, 2, 3])
    assert res["frame_token"].tolist() == [0, -1, 1, 2] and forward(lp, 4, [2, 2, 3]) == pytest.approx(res["score"], abs=1e-12)
    assert status_of(5, [0], 4) == 2 and status_of(5, [4], 4) == 2 and status_of(5, [3], 4) == 0
    assert check_path([0, 0, -1, 1], [1, 2]) is None
    assert check_path([0, 1, 1, 1], [1, 1]) is not None          # equal neighbours need a blank between them
    assert check_path([-1, -1, 0, -1], [1, 2]) is not None        # token 1 never emitted
    assert check_path([1, 1, 1, 1], [1, 2]) is not None           # starts in state 3
    assert check_path([0, -1, 0, 1], [1, 2]) is not None          # a token split by a blank


def test_frame_seconds_of_the_named_configs():
    from efficientconformer_amd import ConformerEncoder
    want = {"EfficientConformerCTCSmall": 0.08, "EfficientConformerCTCMedium": 0.08, "EfficientConformerCTCLarge": 0.08,
            "ConformerCTCSmall": 0.04, "ConformerCTCMedium": 0.04, "ConformerCTCLarge": 0.04}
    for name, sec in want.items():
        enc = ConformerEncoder(named_config(name)["encoder_params"])
        assert enc.frame_seconds == pytest.approx(sec, rel=1e-12), name
        # consistent with the frame count of the plan: 100 s of audio
        n = 100 * enc.plan.sample_rate
        assert abs(enc.plan.lengths(n)[2][-1] * enc.frame_seconds - 100.0) <= 2 * enc.frame_seconds, name


def test_ctc_align_surface():
    from efficientconformer_amd import Alignment, ModelCTC
    assert list(inspect.signature(ModelCTC.align_logits).parameters)[:5] == ["self", "logits", "logits_len", "targets", "target_len"]
    for fn in (ModelCTC.align, ModelCTC.score_labels):
        assert list(inspect.signature(fn).parameters) == ["self", "x", "x_len", "y", "y_len", "from_mel"]
    assert list(inspect.signature(ModelCTC.greedy_alignment).parameters) == ["self", "x", "x_len", "from_mel"]
    assert Alignment._fields == ("tokens", "start_frame", "end_frame", "start_time", "end_time", "token_logp", "score", "log_likelihood",
                                 "status")


def test_ctc_align_workspace_bytes_rejects_and_grows():
    from efficientconformer_amd import _lib
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "effconf.h")) as fh:
        hdr = fh.read()
    for fn in ("effconf_ctc_align_workspace_bytes", "effconf_ctc_align"):
        assert fn in hdr and fn in _lib.SIGNATURES
    assert lib.effconf_abi_version() == 3
    ok = lib.effconf_ctc_align_workspace_bytes(4, 50, 256, 20)
    assert ok > 0
    for args in [(4, 50, 1, 20), (4, 50, 1025, 20), (4, 50, 256, -1), (4, 50, 256, 2048), (-1, 50, 256, 20), (4, -1, 256, 20)]:
        assert lib.effconf_ctc_align_workspace_bytes(*args) == 0, args
    assert lib.effconf_ctc_align_workspace_bytes(8, 50, 256, 20) > ok
    assert lib.effconf_ctc_align_workspace_bytes(4, 100, 256, 20) > ok
    assert lib.effconf_ctc_align_workspace_bytes(4, 50, 256, 40) > ok
    assert lib.effconf_ctc_align_workspace_bytes(0, 0, 2, 0) > 0 and lib.effconf_ctc_align_workspace_bytes(1, 1, 1024, 2047) > 0
    assert 0 < lib.effconf_ctc_align_workspace_bytes(256, 200, 256, 200) < 256 * 1024 ** 2
    # arguments are checked before any launch: no device pointer is touched
    none = [None] * 7
    assert lib.effconf_ctc_align(None, None, 1, 1, 1025, None, None, 4, 1.0, *none, None, 0, None) != 0
    assert lib.effconf_ctc_align(None, None, 1, 1, 256, None, None, 2048, 1.0, *none, None, 0, None) != 0
    assert lib.effconf_ctc_align(None, None, 1, 1, 256, None, None, 4, 0.0, *none, None, 0, None) != 0
    assert lib.effconf_ctc_align(None, None, 1, 1, 256, None, None, 4, float("inf"), *none, None, 0, None) != 0
    assert lib.effconf_ctc_align(None, None, 1, 1, 256, None, None, 4, 1.0, *none, None, 0, None) != 0


def test_ctc_align_bad_arguments_raise_before_the_gpu():
    from efficientconformer_amd import ModelCTC, _lib
    m = ModelCTC.from_config(named_config("Tiny"))
    logits = torch.zeros(2, 5, 32)
    with pytest.raises(_lib.EffconfError):
        m.align_logits(torch.zeros(2, 5), None, [[1], [2]])
    with pytest.raises(_lib.EffconfError):
        m.align_logits(torch.zeros(2, 5, 1), None, [[1], [2]])
    with pytest.raises(_lib.EffconfError):
        m.align_logits(torch.zeros(2, 5, 1025), None, [[1], [2]])
    with pytest.raises(_lib.EffconfError):
        m.align(torch.zeros(2, 1600).cpu(), None, ["a", "b"])      # strings without a tokenizer
    m.tmp = 0.0
    with pytest.raises(_lib.EffconfError):
        m.align_logits(logits, None, [[1], [2]])
    m.tmp = 1.0
    with pytest.raises(RuntimeError):                            # a CPU tensor: no fallback
        m.align_logits(logits, None, [[1], [2]])
    with pytest.raises(RuntimeError):
        m.score_labels(torch.zeros(2, 1600), None, [[1], [2]])
