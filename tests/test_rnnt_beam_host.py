"""RNN-T beam search, host side: the float64 restatement of the algorithm (tests/rnnt_beam_ref.py) against the reference's own
beam_search_decoding (tools/make_goldens.py --only-rnnt-beam -> tests/golden/rnnt_beam_*.npz), and the Python surface."""
import inspect
import os

import numpy as np
import pytest
import torch

from efficientconformer_amd import named_config, synth
from rnnt_beam_ref import beam_decode

SHIPPED_TRANSDUCERS = ["EfficientConformerTransducerSmall", "EfficientConformerTransducerMedium", "EfficientConformerTransducerLarge",
                       "ConformerTransducerSmall", "ConformerTransducerMedium", "ConformerTransducerLarge"]


def _fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "rnnt_%s.npz" % name))
    bg = np.load(os.path.join(golden_dir, "rnnt_beam_%s.npz" % name))
    cfg = named_config(name)
    sd = synth.make_transducer_state_dict(g["f"].shape[-1], cfg["decoder_params"], cfg["joint_params"], int(bg["weight_seed"]),
                                          blank_bias=float(bg["blank_bias"]))
    return torch.from_numpy(g["f"]), torch.from_numpy(g["f_len"]), sd, bg


def _want(bg, beam, n):
    offs = bg["offsets_b%d" % beam]
    return [bg["tokens_b%d" % beam][offs[i]:offs[i + 1]].tolist() for i in range(n)]


@pytest.mark.parametrize("name", ["TinyTransducer", "EfficientConformerTransducerMedium"])
def test_beam_oracle_matches_reference_goldens(golden_dir, name):
    """The float64 oracle reproduces the reference's fp32 beam search on every row and beam: the fixtures hold no decision that fp32
    rounding could flip, so token identity with them is a fair requirement for the fp32 kernel."""
    f, f_len, sd, bg = _fixture(golden_dir, name)
    assert float(bg["blank_bias"]) == np.float32(1.2)
    for beam in bg["beams"].tolist():
        res = beam_decode(sd, f, f_len, beam)
        assert [r["tokens"] for r in res] == _want(bg, beam, f.shape[0]), (name, beam)
        assert not any(r["capped"] for r in res)
        for r, n in zip(res, f_len.tolist()):
            assert len(r["expansions"]) == n and all(e >= beam for e in r["expansions"])


def test_beam_oracle_cap_flags_non_terminating_rows(golden_dir):
    """Blank bias 0 on Tiny: on rows 0, 1 and 3 blank never reaches the top 16 of the popped hypotheses in some frame and the reference
    would expand forever; under the default cap (16 * beam expansions per frame) the oracle flags exactly those rows and decodes row 2.
    Beam 1 at blank bias 1.2 does not terminate either (the reference's own beam 1 loops on every row of this fixture)."""
    g = np.load(os.path.join(golden_dir, "rnnt_TinyTransducer.npz"))
    cfg = named_config("TinyTransducer")
    f, f_len = torch.from_numpy(g["f"]), torch.from_numpy(g["f_len"])
    sd = synth.make_transducer_state_dict(f.shape[-1], cfg["decoder_params"], cfg["joint_params"], int(g["weight_seed"]), blank_bias=0.0)
    res = beam_decode(sd, f, f_len, 16, max_expansions=256)
    assert [r["capped"] for r in res] == [True, True, False, True]
    assert all(r["tokens"] == [] and r["expansions"][-1] == 256 for r in res if r["capped"])
    assert len(res[2]["tokens"]) > 0 and max(res[2]["expansions"]) < 256
    sd = synth.make_transducer_state_dict(f.shape[-1], cfg["decoder_params"], cfg["joint_params"], int(g["weight_seed"]), blank_bias=1.2)
    assert all(r["capped"] for r in beam_decode(sd, f, f_len, 1, max_expansions=1000))


def test_transducer_reads_beam_size_and_tmp_from_configs():
    from efficientconformer_amd import Transducer
    for name in SHIPPED_TRANSDUCERS:
        cfg = named_config(name)
        assert cfg["decoding_params"]["beam_size"] == 16 and cfg["decoding_params"]["tmp"] == 1
    m = Transducer.from_config("TinyTransducer")
    assert (m.beam_size, m.tmp) == (16, 1.0)
    cfg = named_config("TinyTransducer")
    cfg["decoding_params"] = {"beam_size": 4, "tmp": 2.5}
    m = Transducer.from_config(cfg)
    assert (m.beam_size, m.tmp) == (4, 2.5)
    del cfg["decoding_params"]                                   # Model.__init__ defaults (model.py:60-61)
    m = Transducer.from_config(cfg)
    assert (m.beam_size, m.tmp) == (1, 1.0)


def test_beam_search_decoding_has_reference_signature():
    from efficientconformer_amd import Transducer
    sig = inspect.signature(Transducer.beam_search_decoding)
    assert list(sig.parameters) == ["self", "x", "x_len", "beam_size"]
    assert sig.parameters["beam_size"].default is None
    sig = inspect.signature(Transducer.decode_encoded_beam)
    assert list(sig.parameters) == ["self", "f", "f_len", "beam_size", "max_expansions_per_frame", "max_tokens"]


def test_beam_abi_declared_and_rejects_bad_arguments():
    """The two entry points are in include/effconf.h and _lib.SIGNATURES; unsupported beams are refused before any launch."""
    import ctypes as C

    from efficientconformer_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "effconf.h")) as fh:
        hdr = fh.read()
    for fn in ("effconf_rnnt_beam_workspace_bytes", "effconf_rnnt_beam"):
        assert fn in hdr and fn in _lib.SIGNATURES
    lib = _lib.load()
    cfg = _lib.EcRnntConfig(48, 32, 32, 40, 1, 5, 0, 0)
    h = lib.effconf_rnnt_create(C.byref(cfg))
    try:
        assert lib.effconf_rnnt_beam_workspace_bytes(h, 4, 13, 16, 256, 208) > 0
        assert lib.effconf_rnnt_beam_workspace_bytes(h, 4, 13, 17, 256, 208) == 0          # beam > 16
        assert lib.effconf_rnnt_beam_workspace_bytes(h, 4, 13, 0, 256, 208) == 0
        assert lib.effconf_rnnt_beam_workspace_bytes(h, 4, 13, 4, 0, 208) == 0             # no expansion allowed
        assert lib.effconf_rnnt_set_option(h, b"beam_eval_batch", 1) == 0
        assert lib.effconf_rnnt_set_option(h, b"beam_eval_batch", 17) != 0
        # not finalized: rejected before any launch
        assert lib.effconf_rnnt_beam(h, None, None, 1, 1, 4, 1.0, 64, None, None, None, None, 64, None, 0, None) != 0
    finally:
        lib.effconf_rnnt_destroy(h)
    cfg = _lib.EcRnntConfig(48, 40, 40, 40, 1, 5, 0, 0)          # widths not multiples of 16
    h = lib.effconf_rnnt_create(C.byref(cfg))
    try:
        assert lib.effconf_rnnt_beam_workspace_bytes(h, 4, 13, 4, 64, 64) == 0
        assert b"multiples of 16" in lib.effconf_last_error()
    finally:
        lib.effconf_rnnt_destroy(h)


def test_beam_workspace_for_256_utterances():
    """Batch 256, T = 250, beam 16, default limits (16 * beam expansions per frame, 16 * T tokens), Transducer-Medium widths."""
    import ctypes as C

    from efficientconformer_amd import _lib
    lib = _lib.load()
    cfg = _lib.EcRnntConfig(360, 640, 640, 1000, 1, 5, 0, 0)
    h = lib.effconf_rnnt_create(C.byref(cfg))
    try:
        n = lib.effconf_rnnt_beam_workspace_bytes(h, 256, 250, 16, 256, 4000)
        assert 0 < n < 2 * 1024 ** 3, n
    finally:
        lib.effconf_rnnt_destroy(h)
