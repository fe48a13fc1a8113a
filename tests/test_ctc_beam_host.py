"""CTC prefix beam search, host side: the float64 oracle (tests/ctc_beam_ref.py) against brute force and torch's ctc_loss, its
top-(2 beam + 1) shortcut against full evaluation, and the Python / C surface (no GPU needed)."""
import inspect
import os

import numpy as np
import pytest
import torch

from ctc_beam_ref import all_labellings, beam_search, brute_force, ctc_log_prob, logp64
from efficientconformer_amd import named_config

SHIPPED_CTC = ["EfficientConformerCTCSmall", "EfficientConformerCTCMedium", "EfficientConformerCTCLarge",
               "ConformerCTCSmall", "ConformerCTCMedium", "ConformerCTCLarge"]


def _lp(rng, t, v, scale=2.0):
    return logp64((rng.standard_normal((t, v)) * scale).astype(np.float32))


@pytest.mark.parametrize("t", [1, 2, 3])
def test_oracle_equals_brute_force_when_nothing_is_pruned(t):
    """V = 3, T <= 3: at most 15 prefixes, so beam 16 keeps every candidate.  The finite entries are exactly the labellings that
    some alignment produces, with their total log-probabilities; the -inf entries are the unreachable labellings."""
    rng = np.random.default_rng(100 + t)
    for _ in range(5):
        lp = _lp(rng, t, 3)
        res = beam_search(lp, t, 16)
        want = brute_force(lp)
        got = {p: s for p, s in zip(res["prefixes"], res["score"])}
        assert len(got) == len(res["prefixes"])                          # no duplicates
        finite = {p: s for p, s in got.items() if np.isfinite(s)}
        assert set(finite) == set(want)
        for p, s in finite.items():
            assert abs(s - want[p]) <= 1e-9, (p, s, want[p])
        unreachable = set(got) - set(finite)
        assert unreachable == set(got) & (set(all_labellings(3, t)) - set(want))


def test_oracle_against_ctc_loss():
    """The best score is -ctc_loss (float64) of its tokens when nothing is pruned and never above it when something is."""
    rng = np.random.default_rng(7)
    for t in (2, 3):
        lp = _lp(rng, t, 3)
        res = beam_search(lp, t, 16)
        for p, s in zip(res["prefixes"], res["score"]):
            if np.isfinite(s):
                assert abs(s - ctc_log_prob(lp, t, p)) <= 1e-9
    for t, v, beam in [(12, 5, 2), (20, 8, 4), (30, 16, 3)]:
        lp = _lp(rng, t, v)
        res = beam_search(lp, t, beam)
        assert res["score"][0] <= ctc_log_prob(lp, t, res["prefixes"][0]) + 1e-9


def test_shortcut_equals_full_evaluation():
    """Only the frame's 2 beam + 1 most probable tokens can give a plain extension that survives: the shortcut keeps the same beams."""
    rng = np.random.default_rng(11)
    for i in range(60):
        t, v, beam = int(rng.integers(3, 14)), int(rng.integers(3, 24)), int(rng.integers(1, 6))
        lp = _lp(rng, t, v, scale=float(rng.choice([0.5, 2.0, 5.0])))
        full = beam_search(lp, t, beam, trace=True)
        short = beam_search(lp, t, beam, shortcut=True, trace=True)
        assert [[p for p, _, _ in fr] for fr in full["beams"]] == [[p for p, _, _ in fr] for fr in short["beams"]], (t, v, beam)
        assert np.array_equal(full["score"], short["score"])


def test_ctc_configs_carry_beam_size_and_tmp():
    from efficientconformer_amd import ModelCTC
    for name in SHIPPED_CTC:
        cfg = named_config(name)
        assert cfg["decoding_params"]["beam_size"] == 16 and cfg["decoding_params"]["tmp"] == 1
        m = ModelCTC.from_config(name)
        assert (m.beam_size, m.tmp) == (16, 1.0)


def test_ctc_decoding_params_defaults_and_overrides():
    from efficientconformer_amd import ModelCTC
    cfg = named_config("Tiny")
    del cfg["decoding_params"]                                   # Model.__init__ defaults (model.py:60-61)
    m = ModelCTC.from_config(cfg)
    assert (m.beam_size, m.tmp) == (1, 1.0)
    cfg["decoding_params"] = {"beam_size": 4, "tmp": 2.5, "ngram_path": "lm.arpa", "ngram_alpha": 0.5}
    m = ModelCTC.from_config(cfg)
    assert (m.beam_size, m.tmp) == (4, 2.5)


def test_ctc_beam_search_decoding_has_reference_signature():
    from efficientconformer_amd import ModelCTC
    sig = inspect.signature(ModelCTC.beam_search_decoding)
    assert list(sig.parameters) == ["self", "x", "x_len", "beam_size"]
    assert sig.parameters["beam_size"].default is None
    assert list(inspect.signature(ModelCTC.decode_logits_beam).parameters) == ["self", "logits", "logits_len", "beam_size"]
    assert list(inspect.signature(ModelCTC.beam_labels).parameters) == ["self", "x", "x_len", "beam_size", "from_mel"]


def test_ctc_beam_workspace_bytes_rejects_and_grows():
    from efficientconformer_amd import _lib
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "effconf.h")) as fh:
        hdr = fh.read()
    for fn in ("effconf_ctc_beam_workspace_bytes", "effconf_ctc_beam"):
        assert fn in hdr and fn in _lib.SIGNATURES
    ok = lib.effconf_ctc_beam_workspace_bytes(4, 50, 256, 16)
    assert ok > 0
    for args in [(4, 50, 256, 0), (4, 50, 256, 33), (4, 50, 1, 16), (4, 50, 1025, 16), (-1, 50, 256, 16), (4, -1, 256, 16)]:
        assert lib.effconf_ctc_beam_workspace_bytes(*args) == 0, args
    assert lib.effconf_ctc_beam_workspace_bytes(8, 50, 256, 16) > ok
    assert lib.effconf_ctc_beam_workspace_bytes(4, 100, 256, 16) > ok
    assert 0 < lib.effconf_ctc_beam_workspace_bytes(256, 200, 256, 16) < 256 * 1024 ** 2
    # arguments are checked before any launch: no device pointer is touched
    assert lib.effconf_ctc_beam(None, None, 1, 1, 256, 33, 1.0, None, None, None, None, 0, None) != 0
    assert lib.effconf_ctc_beam(None, None, 1, 1, 256, 4, 0.0, None, None, None, None, 0, None) != 0
    assert lib.effconf_ctc_beam(None, None, 1, 1, 256, 4, 1.0, None, None, None, None, 0, None) != 0


def test_ctc_beam_bad_arguments_raise_before_the_gpu():
    from efficientconformer_amd import ModelCTC, _lib
    cfg = named_config("Tiny")
    m = ModelCTC.from_config(cfg)
    logits = torch.zeros(2, 5, 32)
    for beam in (0, 33):
        with pytest.raises(_lib.EffconfError):
            m.decode_logits_beam(logits, None, beam)
        with pytest.raises(_lib.EffconfError):
            m.beam_search_decoding(torch.zeros(2, 1600), torch.tensor([1600, 1600]), beam)
    with pytest.raises(_lib.EffconfError):
        m.decode_logits_beam(torch.zeros(2, 5, 1), None, 4)
    with pytest.raises(_lib.EffconfError):
        m.decode_logits_beam(torch.zeros(2, 5, 1025), None, 4)
    m.tmp = 0.0
    with pytest.raises(_lib.EffconfError):
        m.decode_logits_beam(logits, None, 4)
    m.tmp = 1.0
    with pytest.raises(RuntimeError):                            # a CPU tensor: no fallback
        m.decode_logits_beam(logits, None, 4)
