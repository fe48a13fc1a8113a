"""RNN-T beam search with neural-LM fusion, host side (no GPU): the float64 oracle (tests/rnnt_beam_lm_ref.py) against the reference's own fused
beam_search_decoding (tests/golden/rnnt_beam_lm_TinyTransducer.npz, its fp32 run), the conditions the fixture must meet for the GPU tests to mean something,
the float32 / float64 agreement the production-width GPU case relies on, and the argument rules of the Python wrapper."""
import numpy as np
import pytest
import torch

import lm_ref
import rnnt_beam_lm_cases as cases
from rnnt_beam_lm_ref import lm_step_torch

BEAMS = (4, 16)


def _fixture_params():
    g = cases.golden()
    return float(g["blank_bias"]), float(g["lm_weight"]), float(g["lm_tmp"])


def test_golden_is_the_fixture_the_tests_assume():
    g = cases.golden()
    assert _fixture_params() == (2.0, 0.3, 1.0) and g["beams"].tolist() == list(BEAMS)
    cases.tiny_lm()                                                   # asserts the stored LM seed and bias are lm_TinyLM.npz's
    assert len(g["offsets_b4"]) == len(g["offsets_b16"]) == cases.encoded(cases.TINY)[0].shape[0] + 1


@pytest.mark.parametrize("beam", BEAMS)
def test_float64_oracle_reproduces_the_reference_fused_search(beam):
    bb, w, lm_tmp = _fixture_params()
    ref = cases.oracle(cases.TINY, beam, bb, w, 1.0, lm_tmp)
    assert [r["tokens"] for r in ref] == cases.golden_tokens(beam)


@pytest.mark.parametrize("beam", BEAMS)
def test_fixture_terminates_and_the_lm_changes_the_answer(beam):
    """Conditions on the fixture: every utterance terminates under the default cap 16 * beam, and the fused tokens differ from the plain search's for at least
    two of the four utterances - otherwise the GPU tests would pass on a search that ignores the LM."""
    bb, w, lm_tmp = _fixture_params()
    for tmp, ltmp in ((1.0, lm_tmp), (1.3, 2.0)):
        fused = cases.oracle(cases.TINY, beam, bb, w, tmp, ltmp, 16 * beam)
        plain = cases.oracle(cases.TINY, beam, bb, 0.0, tmp, 1.0, 16 * beam)
        assert not any(r["capped"] for r in fused) and not any(r["capped"] for r in plain)
        differ = [i for i in range(len(fused)) if fused[i]["tokens"] != plain[i]["tokens"]]
        assert len(differ) >= 2, (beam, tmp, ltmp, differ)
        assert all(r["lm_steps"] > 0 for r in fused)


def test_cap_fixture_caps_rows_0_and_1():
    """Blank bias 1.2, beam 4, weight 0.3: the LM's token-0 probability lands on blank; rows 0 and 1 do not fill B within 64 expansions of a frame."""
    ref = cases.oracle(cases.TINY, 4, 1.2, 0.3, max_expansions=64)
    assert [r["capped"] for r in ref] == [True, True, False, False]
    assert all(len(r["tokens"]) > 0 for r in ref[2:])


def test_float32_twin_of_the_lm_step_is_the_float64_oracle():
    """rnnt_beam_lm_ref's float32 path restates lm_ref.step; in float64 the restatement equals it to rounding."""
    params, sd = cases.tiny_lm()
    t64 = {k: torch.from_numpy(v).double() for k, v in sd.items()}
    state = None
    want_state = None
    for tok in (0, 7, 39, 1):
        got, state = lm_step_torch(t64, params["num_layers"], tok, state)
        want, want_state = lm_ref.step(sd, [tok], want_state)
        assert np.allclose(got.numpy(), want[0], rtol=0, atol=1e-12)
        assert np.allclose(state[0].numpy(), want_state[0][:, 0], rtol=0, atol=1e-12) and np.allclose(state[1].numpy(), want_state[1][:, 0], rtol=0, atol=1e-12)


def test_production_width_case_is_decided_the_same_in_float32_and_float64():
    """The GPU test at Medium's widths demands the float64 oracle's tokens on every utterance: legitimate only where the oracle program evaluated in float32
    gives those tokens too (seed and weight of the synthetic LM were chosen for that; no row is excluded)."""
    f64 = cases.oracle(cases.MEDIUM, 16, 1.2, cases.MEDIUM_LM_WEIGHT, max_expansions=256)
    f32 = cases.oracle(cases.MEDIUM, 16, 1.2, cases.MEDIUM_LM_WEIGHT, max_expansions=256, dtype=torch.float32)
    plain = cases.oracle(cases.MEDIUM, 16, 1.2, 0.0, max_expansions=256)
    assert not any(r["capped"] for r in f64)
    assert [r["tokens"] for r in f32] == [r["tokens"] for r in f64]
    assert all(a["tokens"] != b["tokens"] for a, b in zip(f64, plain))


def test_wrapper_argument_rules():
    """No LM, or weight 0: the plain entry (nothing to fuse).  A negative or non-finite weight with an LM raises ValueError before anything else happens."""
    from efficientconformer_amd import LanguageModel, Transducer, named_config
    cfg = named_config(cases.TINY)
    m = Transducer.from_config(dict(cfg, decoding_params={"beam_size": 4, "tmp": 1, "lm_weight": 0.25, "lm_tmp": 2}))
    assert m.lm is None and m.lm_weight == 0.25 and m.lm_tmp == 2.0
    assert Transducer.from_config(cfg).lm_weight == 0 and Transducer.from_config(cfg).lm_tmp == 1
    lm = LanguageModel(dict(cases.tiny_lm()[0]))
    assert m._fusion(None, None, None) == (None, 0.0, 2.0)             # no LM attached
    assert m._fusion(lm, 0, None)[0] is None and m._fusion(lm, 0.0, 1.0)[0] is None
    assert m._fusion(lm, None, None) == (lm, 0.25, 2.0) and m._fusion(lm, 0.5, 1.5) == (lm, 0.5, 1.5)
    m.lm = lm
    assert m._fusion(None, None, None) == (lm, 0.25, 2.0) and m._fusion(None, 0, None)[0] is None
    f = torch.zeros(1, 3, m.encoder.plan.dim_out)
    for bad in (-0.3, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            m.decode_encoded_beam_lm(f, None, 4, lm_weight=bad)
        with pytest.raises(ValueError):
            m.beam_tokens(f, None, 4, lm_weight=bad)
    with pytest.raises(ValueError):
        m.decode_encoded_beam_lm(f, None, 4, lm_tmp=0.0)
    m.lm = None
    with pytest.raises(RuntimeError, match="HIP device only"):        # nothing to fuse: the plain path, which has no CPU fallback either
        m.decode_encoded_beam_lm(f, None, 4, lm_weight=-0.3)
    assert m.last_beam_rounds() is None
