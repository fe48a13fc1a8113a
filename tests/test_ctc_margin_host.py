"""Margin-gated label-exact decoding, host side (no GPU): the row selection rule, the C / ctypes surface of effconf_ctc_greedy_margin, the Python signatures
and the refusals that need no device."""
import inspect
import os
import re

import pytest
import torch

from efficientconformer_amd import ModelCTC, _lib, named_config, select_rerun
from efficientconformer_amd import model_ctc as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


def test_select_rerun_takes_what_is_not_known_to_reach_the_band():
    mm = torch.tensor([0.5, 0.25, NAN, INF, 0.2499, 0.0, 0.25])
    assert select_rerun(mm, 0.25).tolist() == [2, 4, 5]                  # a margin equal to the band is kept, NaN is taken, +inf never
    assert select_rerun(mm, 0.0).tolist() == [2]                         # band 0: nothing but NaN
    assert select_rerun(mm, INF).tolist() == [0, 1, 2, 4, 5, 6]          # band inf: everything that has frames
    assert select_rerun(torch.tensor([INF, INF]), INF).tolist() == []
    assert select_rerun(torch.tensor([-0.0, 0.0]), 0.0).tolist() == []
    empty = select_rerun(torch.empty(0), 0.3)
    assert empty.shape == (0,) and empty.dtype == torch.int64
    got = select_rerun(torch.tensor([1.0, 0.1, 0.3]), 0.3)
    assert got.dtype == torch.int64 and got.tolist() == [1]
    mm0 = mm.clone()
    select_rerun(mm, 0.25)
    assert torch.equal(mm.nan_to_num(7.0), mm0.nan_to_num(7.0))            # pure: the input is untouched


def test_margin_entry_is_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "effconf.h")) as fh:
        hdr = fh.read()
    decl = re.search(r"int effconf_ctc_greedy_margin\(([^;]*)\);", hdr)
    assert decl, "include/effconf.h does not declare effconf_ctc_greedy_margin"
    names = [a.split()[-1].lstrip("*") for a in decl.group(1).replace("\n", " ").split(",")]
    assert names == ["enc", "enc_out", "enc_is_bf16", "out_len", "batch", "t_out", "labels", "label_len", "logits", "frame_margin", "min_margin", "min_frame",
                     "workspace", "workspace_bytes", "stream"]
    assert len(_lib.SIGNATURES["effconf_ctc_greedy_margin"][1]) == len(names)
    lib = _lib.load()
    assert hasattr(lib, "effconf_ctc_greedy_margin")
    assert lib.effconf_abi_version() == 3                                  # additive: the ABI version stays


def test_margin_entry_refuses_an_unfinalized_handle():
    import ctypes as C
    lib = _lib.load()
    cfg, _keep = ModelCTC.from_config(named_config("Tiny")).encoder._make_config()
    h = lib.effconf_encoder_create(C.byref(cfg))
    assert h, lib.effconf_last_error()
    try:
        assert lib.effconf_ctc_greedy_margin(h, None, 0, None, 2, 8, None, None, None, None, None, None, None, 0, None) != 0
        assert lib.effconf_last_error() == b"encoder not finalized"
        assert lib.effconf_ctc_greedy_margin(None, None, 0, None, 2, 8, None, None, None, None, None, None, None, 0, None) != 0
    finally:
        lib.effconf_encoder_destroy(h)


def test_python_surface_and_refusals_before_the_gpu():
    assert list(inspect.signature(ModelCTC.head_margins).parameters) == ["self", "enc", "enc_len", "want_logits"]
    assert list(inspect.signature(ModelCTC.greedy_exact).parameters) == ["self", "x", "x_len", "band", "from_mel", "x_len_host"]
    p = inspect.signature(ModelCTC.greedy_labels).parameters
    assert list(p) == ["self", "x", "x_len", "from_mel", "label_exact", "band"]
    assert p["label_exact"].kind is inspect.Parameter.KEYWORD_ONLY and p["label_exact"].default is None and p["band"].default is None
    assert inspect.signature(ModelCTC.gready_search_decoding).parameters["label_exact"].default is None
    assert MC.HeadMargins._fields == ("labels", "label_len", "frame_margin", "min_margin", "min_frame", "logits")
    m = ModelCTC.from_config(named_config("Tiny"))
    assert m.label_exact_band == MC.LABEL_EXACT_BAND and 0 < MC.LABEL_EXACT_BAND < INF
    cfg = dict(named_config("Tiny"), decoding_params={"label_exact_band": 0.75})
    assert ModelCTC.from_config(cfg).label_exact_band == 0.75
    x, n = torch.zeros(2, 1600), torch.tensor([1600, 800])
    with pytest.raises(RuntimeError):                                      # a CPU tensor: no fallback
        m.greedy_exact(x, n)
    with pytest.raises(RuntimeError):
        m.head_margins(torch.zeros(2, 5, 48), None)
    with pytest.raises(ValueError):
        m.greedy_labels(x, n, label_exact="sometimes")
