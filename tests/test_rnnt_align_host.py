"""RNN-T lattice scoring and forced alignment, host side: the float64 oracle (tests/rnnt_align_ref.py) against brute force over every
monotone path, against the reference's own lattice (tests/golden/rnnt_lattice_*.npz: its RnnDecoder and JointNetwork run as
Transducer.forward runs them, reduced with log_softmax), the seeds of the GPU tests, and the Python / C surface (no GPU needed).

Golden planes.  The reference computes in float32, the oracle in float64: they differ by the reference's own rounding noise.  Measured
(max over the finite cells, |lp| up to 8.9): 4.2e-7 on TinyTransducer, 1.6e-6 on EfficientConformerTransducerMedium.  The float32 CPU
evaluation of the oracle's own formula deviates from float64 by 4.5e-7 / 1.8e-6 on the same lattices (rnnt_align_cases.float32_noise, the
yardstick of the GPU test); the bound here is 8 x that noise, the project's stage convention, i.e. 1.4e-5."""
import inspect
import os

import numpy as np
import pytest
import torch

import rnnt_align_cases as cases
from rnnt_align_ref import all_paths, brute_force, check_path, forward, path_logp, status_of, viterbi
from efficientconformer_amd import named_config

MARGIN = 1e-3


@pytest.mark.parametrize("t", [1, 2, 3, 4])
@pytest.mark.parametrize("u", [0, 1, 2, 3])
def test_forward_and_viterbi_equal_brute_force(t, u):
    rng = np.random.default_rng(100 * t + u)
    assert len(all_paths(t, u)) == {0: 1, 1: t, 2: t * (t + 1) // 2, 3: t * (t + 1) * (t + 2) // 6}[u]
    for _ in range(8):
        lpb, lpl = cases.random_planes(rng, t, u)
        want = brute_force(lpb, lpl, t, u)
        got = forward(lpb, lpl, t, u)
        assert abs(got - want["log_likelihood"]) <= 1e-9 * (1 + abs(got)), (t, u)
        res = viterbi(lpb, lpl, t, u)
        assert abs(res["score"] - want["score"]) <= 1e-9 * (1 + abs(res["score"])), (t, u)
        assert check_path(res["token_frame"], t, u) is None
        assert abs(path_logp(lpb, lpl, res["token_frame"], t) - res["score"]) <= 1e-9 * (1 + abs(res["score"]))
        assert res["token_frame"].tolist() in want["best"]
        assert res["score"] <= got + 1e-12
        if len(all_paths(t, u)) == 1:
            assert res["margin"] == np.inf


def test_ties_take_the_blank_move():
    """Uniform planes: every path has the same probability.  Traced back from (T - 1, U), equality takes the time move for as long as a
    frame is left: every token is emitted at frame 0."""
    lpb, lpl = np.full((4, 3), np.log(0.25)), np.full((4, 3), np.log(0.25))
    lpl[:, 2] = -np.inf
    res = viterbi(lpb, lpl)
    assert res["token_frame"].tolist() == [0, 0] and res["margin"] == 0.0
    assert res["score"] == pytest.approx(6 * np.log(0.25), abs=1e-12)
    assert forward(lpb, lpl) == pytest.approx(np.log(10) + 6 * np.log(0.25), abs=1e-12)       # C(5, 2) paths


def test_degenerate_cases():
    rng = np.random.default_rng(5)
    lpb, lpl = (p.astype(np.float64) for p in cases.random_planes(rng, 5, 3))
    assert forward(lpb, lpl, 0, 0) == 0.0 and viterbi(lpb, lpl, 0, 0)["score"] == 0.0
    assert np.isneginf(forward(lpb, lpl, 0, 2)) and np.isneginf(viterbi(lpb, lpl, 0, 2)["score"])
    assert forward(lpb, lpl, 5, 0) == pytest.approx(float(lpb[:, 0].sum()), abs=1e-12)
    assert viterbi(lpb, lpl, 5, 0)["score"] == pytest.approx(float(lpb[:, 0].sum()), abs=1e-12)
    one = viterbi(lpb, lpl, 1, 3)                                # one frame: the labels, then the blank
    assert one["token_frame"].tolist() == [0, 0, 0] and one["score"] == pytest.approx(float(lpl[0, :3].sum() + lpb[0, 3]), abs=1e-12)
    assert forward(lpb, lpl, 1, 3) == pytest.approx(one["score"], abs=1e-12)
    assert status_of(5, [3, 1], 4) == 0 and status_of(5, [0], 4) == 2 and status_of(5, [4], 4) == 2 and status_of(0, [1], 4) == 1
    assert status_of(0, [], 4) == 0 and status_of(5, [1, 2, 3], 4, u_max=2) == 2
    assert check_path([0, 0, 3], 4, 3) is None and check_path([], 0, 0) is None
    assert check_path([1, 0], 4, 2) is not None and check_path([0, 4], 4, 2) is not None and check_path([0], 4, 2) is not None
    assert check_path([0], 0, 1) is not None


@pytest.mark.parametrize("case,name", [("tiny", "TinyTransducer"), ("medium", "EfficientConformerTransducerMedium")])
def test_oracle_planes_equal_the_reference_lattice(case, name):
    g = np.load(os.path.join(cases.GOLDEN, "rnnt_lattice_%s.npz" % name))
    _, f, f_len, targets = cases.lattice_case(case)
    bound = 8 * cases.float32_noise()
    assert 1e-6 < bound < 1e-4
    worst = 0.0
    for i, (lpb, lpl) in enumerate(cases.oracle_planes(case, 1.0)):
        n, u = int(f_len[i]), len(targets[i])
        assert lpb.shape == (n, u + 1) and np.isneginf(lpl[:, u]).all() and np.isfinite(lpl[:, :u]).all()
        gb, gl = g["lp_blank"][i], g["lp_label"][i]
        assert not gb[n:].any() and not gb[:, u + 1:].any() and not gl[n:].any() and not gl[:, u + 1:].any()       # 0 outside the rectangle
        assert np.isneginf(gl[:n, u]).all()
        worst = max(worst, np.abs(gb[:n, :u + 1] - lpb).max(), np.abs(gl[:n, :u] - lpl[:, :u]).max() if u else 0.0)
        # the reference's loss on its own planes: forward in float64 on the fp32 planes agrees with forward on the oracle's
        assert abs(forward(gb[:n, :u + 1], gl[:n, :u + 1]) - forward(lpb, lpl)) <= bound * (n + u)
    print("%s: golden vs float64 oracle %.3g (bound %.3g)" % (name, worst, bound))
    assert worst <= bound, (worst, bound)


def _excused(planes):
    return sum(viterbi(b, l)["margin"] < MARGIN for b, l in planes)


def test_the_seeds_of_the_gpu_tests_leave_few_near_ties():
    """Path identity is asserted on the GPU wherever the oracle's margin is at least 1e-3; at most 1 case in 8 of a test may fall below."""
    for n in cases.DP_U:
        planes = cases.dp_case("u", n)
        assert 8 * _excused(planes) <= len(planes), ("u", n)
    for n in cases.DP_T:
        planes = cases.dp_case("t", n)
        assert 8 * _excused(planes) <= len(planes), ("t", n)
    planes = cases.dp_case("ragged")
    assert 8 * _excused(planes) <= len(planes)
    for case in ("tiny", "medium", "tiny17"):
        for tmp in cases.TEMPERATURES:
            planes = cases.oracle_planes(case, tmp)
            assert 8 * _excused(planes) <= len(planes), (case, tmp)


def test_rnnt_align_surface():
    from efficientconformer_amd import Transducer, TransducerAlignment
    assert list(inspect.signature(Transducer.lattice).parameters) == ["self", "f", "f_len", "y", "y_len"]
    assert list(inspect.signature(Transducer.align_lattice).parameters)[:6] == ["self", "lp_blank", "lp_label", "f_len", "y_len", "scores_only"]
    for fn in (Transducer.align, Transducer.score_labels):
        assert list(inspect.signature(fn).parameters) == ["self", "x", "x_len", "y", "y_len", "from_mel"]
    assert TransducerAlignment._fields == ("tokens", "frame", "time", "token_logp", "score", "log_likelihood", "status")
    m = Transducer.from_config(named_config("TinyTransducer"))
    with pytest.raises(NotImplementedError) as e:
        m.forward(None)
    assert "lattice()" in str(e.value)


def test_rnnt_align_workspace_bytes_rejects_and_grows():
    from efficientconformer_amd import _lib
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "effconf.h")) as fh:
        hdr = fh.read()
    for fn in ("effconf_rnnt_lattice_workspace_bytes", "effconf_rnnt_lattice", "effconf_rnnt_align_workspace_bytes", "effconf_rnnt_align"):
        assert fn in hdr and fn in _lib.SIGNATURES
    ok = lib.effconf_rnnt_align_workspace_bytes(4, 50, 20)
    assert ok > 0
    for args in [(4, 50, -1), (4, 50, 1024), (-1, 50, 20), (4, -1, 20), (1 << 15, 1 << 10, 63)]:      # the last: 2^31 cells
        assert lib.effconf_rnnt_align_workspace_bytes(*args) == 0, args
        assert b"rnnt align" in lib.effconf_last_error()
    assert lib.effconf_rnnt_align_workspace_bytes(8, 50, 20) > ok
    assert lib.effconf_rnnt_align_workspace_bytes(4, 100, 20) > ok
    assert lib.effconf_rnnt_align_workspace_bytes(4, 50, 40) > ok
    assert lib.effconf_rnnt_align_workspace_bytes(0, 0, 0) > 0 and lib.effconf_rnnt_align_workspace_bytes(1, 1, 1023) > 0
    assert 0 < lib.effconf_rnnt_align_workspace_bytes(256, 200, 100) < 16 * 1024 ** 2
    # arguments are checked before any launch: no device pointer is touched
    assert lib.effconf_rnnt_align(None, None, None, None, 1, 1, 1024, None, None, None, None, None, None, 0, None) != 0
    assert lib.effconf_rnnt_align(None, None, None, None, 1, 1, 4, None, None, None, None, None, None, 0, None) != 0
    assert b"null argument" in lib.effconf_last_error()
    assert lib.effconf_rnnt_align(None, None, None, None, 0, 1, 4, None, None, None, None, None, None, 0, None) == 0      # batch 0: a no-op
    # the lattice: a null / unfinalized handle is refused by both entry points
    assert lib.effconf_rnnt_lattice_workspace_bytes(None, 1, 1, 1) == 0
    assert lib.effconf_rnnt_lattice(None, None, None, 1, 1, None, None, 1, 1.0, None, None, None, None, 0, None) != 0


def test_rnnt_align_bad_arguments_raise_before_the_gpu():
    from efficientconformer_amd import Transducer, _lib
    m = Transducer.from_config(named_config("TinyTransducer"))
    with pytest.raises(_lib.EffconfError):
        m.align(torch.zeros(2, 1600), None, ["a", "b"])             # strings without a tokenizer
    with pytest.raises(_lib.EffconfError):
        m.lattice(torch.zeros(2, 5), None, [[1], [2]])
    with pytest.raises(RuntimeError):                               # a CPU tensor: no fallback
        m.lattice(torch.zeros(2, 5, 48), None, [[1], [2]])
    with pytest.raises(RuntimeError):
        m.score_labels(torch.zeros(2, 1600), None, [[1], [2]])
    with pytest.raises(_lib.EffconfError):
        m.align_lattice(torch.zeros(2, 5, 3), torch.zeros(2, 5, 4), None, [2, 2])
    with pytest.raises(_lib.EffconfError):
        m.align_lattice(torch.zeros(2, 5, 1025), torch.zeros(2, 5, 1025), None, [2, 2])      # more than 1023 tokens
    with pytest.raises(RuntimeError):
        m.align_lattice(torch.zeros(2, 5, 3), torch.zeros(2, 5, 3), None, [2, 2])
