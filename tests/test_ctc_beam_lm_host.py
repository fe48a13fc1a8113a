"""CTC prefix beam search with neural-LM fusion, host side (no GPU): the float64 oracle (tests/ctc_beam_lm_ref.py) against closed forms, the conditions the
fixtures of tests/ctc_beam_lm_cases.py must meet for the GPU tests to mean something, the C entry's refusals and the argument rules of the Python wrapper."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_beam_lm_cases as cases
import ctc_beam_lm_ref as ref
import ctc_beam_ref
import lm_ref
from efficientconformer_amd import LanguageModel, ModelCTC, _lib, named_config, synth

NAMES = [c.name for c in cases.CASES]


def test_exact_totals_when_nothing_is_pruned():
    """V = 3, T = 4, beam 32 >= the 31 reachable labellings: every prefix's total is ctc_log_prob + w * sum(token_logprobs) + bonus * len."""
    v, t, w, bonus, lm_tmp = 3, 4, 0.7, 0.25, 1.5
    rng = np.random.default_rng(5)
    lp = ctc_beam_ref.logp64((rng.standard_normal((t, v)) * 1.5).astype(np.float32))
    sd = synth.make_lm_state_dict(dict(arch="RNN", vocab_size=v, dim_model=32, num_layers=2), 11, bias=np.array([0.0, 1.0, -1.0], dtype=np.float32))
    out = ref.beam_search(lp, t, 32, ref.LmRows(sd, lm_tmp), w, bonus)
    assert sorted(out["prefixes"]) == sorted(ctc_beam_ref.all_labellings(v, t)) and len(out["prefixes"]) == 31
    for p, tot, am, lm in zip(out["prefixes"], out["total"], out["score"], out["lm"]):
        y = np.array([list(p) + [0] * (t - len(p))], dtype=np.int64)
        want_lm = float(lm_ref.token_logprobs(sd, y, [len(p)], lm_tmp)[1][0])
        want_am = ctc_beam_ref.ctc_log_prob(lp, t, p)
        assert abs(lm - want_lm) <= 1e-10, p
        if np.isneginf(want_am):                     # repeats without room for the blanks between them
            assert np.isneginf(am) and np.isneginf(tot), p
            continue
        assert abs(am - want_am) <= 1e-9 * (1 + abs(want_am)), p
        assert abs(tot - (want_am + w * want_lm + bonus * len(p))) <= 1e-9 * (1 + abs(tot)), p
    assert all(a >= b for a, b in zip(out["total"][:-1], out["total"][1:]))


@pytest.mark.parametrize("name", ["v32_b4_cols16", "v257_b4_cols32", "v2_b4_short"])
def test_weight_zero_is_the_plain_search(name):
    c = cases.BY_NAME[name]
    for r, got in zip(cases.logits(name)[0], cases.oracle(name, weight=0.0)):
        want = ctc_beam_ref.beam_search(ctc_beam_ref.logp64(r, c.tmp) if r.shape[0] else np.zeros((0, c.v)), r.shape[0], c.beam)
        assert got["prefixes"] == want["prefixes"]
        assert np.array_equal(got["score"], want["score"]) and np.array_equal(got["total"], want["score"]) and not got["lm"].any()


@pytest.mark.parametrize("name", NAMES)
def test_shortcut_is_full_evaluation(name):
    """Exact pruning with an LM: a member's `beam` best plain tokens by lp + w * row, per member, lose nothing."""
    for full, short in zip(cases.oracle(name), cases.oracle(name, shortcut=True)):
        assert short["prefixes"] == full["prefixes"]
        assert np.array_equal(short["total"], full["total"]) and np.array_equal(short["pb"], full["pb"]) and np.array_equal(short["pnb"], full["pnb"])


@pytest.mark.parametrize("name", NAMES)
def test_fixture_decisions_are_clear_and_float32_rows_decide_the_same(name):
    """What the GPU tests assume of every (seed, V, beam, weight) they use: no decision on totals closer than 1e-3, and the oracle on float32 LM rows
    (torch's own LSTM) keeps every rank's tokens."""
    f64, f32 = cases.oracle(name), cases.oracle(name, float32_rows=True)
    for i, (a, b) in enumerate(zip(f64, f32)):
        assert a["gap"] >= 1e-3, (name, i, a["gap"])
        assert a["prefixes"] == b["prefixes"], (name, i)


@pytest.mark.parametrize("name", NAMES)
def test_the_lm_changes_the_answer(name):
    """Otherwise the GPU tests would pass on a search that ignores the LM: the best tokens of at least two utterances of every case differ from the plain
    search's."""
    fused, plain = cases.oracle(name), cases.oracle(name, weight=0.0)
    differ = [i for i in range(len(fused)) if fused[i]["prefixes"][0] != plain[i]["prefixes"][0]]
    assert len(differ) >= 2, (name, differ)


def test_fusion_is_not_rescoring():
    """The fused best differs from the best of the rescored LM-blind n-best: the search itself uses the LM."""
    differ = 0
    for name in ("v32_b4_cols16", "v1000_b16_cols48"):
        c = cases.BY_NAME[name]
        for r, fused in zip(cases.logits(name)[0], cases.oracle(name)):
            differ += ref.rescored_best(ctc_beam_ref.logp64(r, c.tmp), r.shape[0], c.beam, cases.rows64(name), c.weight, c.bonus) != fused["prefixes"][0]
    assert differ >= 1


def test_fixtures_reenter_prefixes_and_reuse_lm_slots():
    reentry = [(n, i) for n in NAMES for i, r in enumerate(cases.oracle(n)) if r["reentries"] > 0]
    reuse = [(n, i) for n in NAMES for i, r in enumerate(cases.oracle(n)) if 1 + r["entered"] > 2 * cases.BY_NAME[n].beam + 1]
    assert reentry and reuse, (reentry, reuse)
    assert any(n == "v1024_b32_cols64" for n, _ in reentry) and any(n == "v1024_b32_cols64" for n, _ in reuse)      # also at the largest beam


# ---------------------------------------------------------------------------------------------------------------- the C surface
@pytest.fixture(scope="module")
def lm_handle():
    lib = _lib.load()
    cfg = _lib.EcLmConfig(32, 32, 1)
    h = lib.effconf_lm_create(C.byref(cfg))
    assert h
    yield lib, h
    lib.effconf_lm_destroy(h)


def _call(lib, h, batch=1, t=4, v=32, beam=4, tmp=1.0, w=0.5, lm_tmp=1.0, bonus=0.0):
    rounds = C.c_int32(-1)
    rc = lib.effconf_ctc_beam_lm(h, None, None, batch, t, v, beam, tmp, w, lm_tmp, bonus, None, None, None, None, None, C.byref(rounds), None, 0, None)
    return rc, (lib.effconf_last_error() or b"").decode()


def test_entry_refuses_what_the_header_says(lm_handle):
    lib, h = lm_handle
    inf, nan = float("inf"), float("nan")
    for kw, word in (({"w": 0.0}, "lm_weight"), ({"w": -0.5}, "lm_weight"), ({"w": nan}, "lm_weight"), ({"w": inf}, "lm_weight"),
                     ({"lm_tmp": 0.0}, "lm_tmp"), ({"lm_tmp": -1.0}, "lm_tmp"), ({"lm_tmp": nan}, "lm_tmp"),
                     ({"bonus": inf}, "length_bonus"), ({"bonus": nan}, "length_bonus"),
                     ({"tmp": 0.0}, "temperature"),
                     ({"v": 33}, "vocab_size"),
                     ({"beam": 0}, "beam"), ({"beam": 33}, "beam"), ({"v": 1}, "vocab"), ({"v": 1025}, "vocab"), ({"batch": -1}, "shape"), ({"t": -1}, "shape"),
                     ({"t": 1 << 22, "beam": 4}, "beam * t_out"),
                     ({"batch": (1 << 19) + 1, "beam": 4}, "2^21"),
                     ({}, "not finalized")):
        rc, msg = _call(lib, h, **kw)
        assert rc != 0 and word in msg, (kw, rc, msg)
    rc, msg = _call(lib, None)
    assert rc != 0 and "lm handle" in msg
    # the size query answers 0 for the same shapes, and needs no finalized handle for the good ones
    size = lib.effconf_ctc_beam_lm_workspace_bytes
    assert size(h, 1, 4, 32, 4) > 0
    for args in ((None, 1, 4, 32, 4), (h, 1, 4, 33, 4), (h, 1, 4, 32, 33), (h, 1, 4, 32, 0), (h, -1, 4, 32, 4), (h, (1 << 19) + 1, 4, 32, 4)):
        assert size(*args) == 0, args


def test_workspace_grows_with_batch_frames_and_beam(lm_handle):
    lib, h = lm_handle
    size = lib.effconf_ctc_beam_lm_workspace_bytes
    base = size(h, 3, 50, 32, 4)
    assert base > lib.effconf_ctc_beam_workspace_bytes(3, 50, 32, 4)
    for b in range(0, 40):
        assert size(h, b + 1, 50, 32, 4) > size(h, b, 50, 32, 4)
    for t in range(0, 70):
        assert size(h, 3, t + 1, 32, 4) >= size(h, 3, t, 32, 4)
    assert size(h, 3, 70, 32, 4) > size(h, 3, 0, 32, 4)
    for beam in range(1, 32):
        assert size(h, 3, 50, 32, beam + 1) > size(h, 3, 50, 32, beam)


# ---------------------------------------------------------------------------------------------------------------- the Python wrapper
def test_wrapper_argument_rules():
    cfg = named_config("Tiny")
    m = ModelCTC.from_config(dict(cfg, decoding_params={"beam_size": 4, "tmp": 1, "lm_weight": 0.25, "lm_tmp": 2}))
    v = cfg["tokenizer_params"]["vocab_size"]
    lm = LanguageModel(dict(arch="RNN", vocab_size=v, dim_model=32, num_layers=1))
    assert m._fusion(None, None, None, 0.0) == (None, 0.0, 2.0, 0.0)                 # no LM attached
    assert m._fusion(lm, 0, None, 0.0)[0] is None
    assert m._fusion(lm, None, None, 0.5) == (lm, 0.25, 2.0, 0.5) and m._fusion(lm, 0.5, 1.5, -0.1) == (lm, 0.5, 1.5, -0.1)
    logits = torch.zeros(1, 3, v)
    x, x_len = torch.zeros(1, 1600), torch.tensor([1600])
    for bad in (-0.3, float("nan"), float("inf")):                                   # a weight that is not >= 0 and finite, with an LM
        with pytest.raises(ValueError):
            m.decode_logits_beam_lm(logits, None, 4, lm=lm, lm_weight=bad)
        with pytest.raises(ValueError):
            m.beam_labels_fused(x, x_len, 4, lm=lm, lm_weight=bad)
    with pytest.raises(ValueError):
        m.decode_logits_beam_lm(logits, None, 4, lm=lm, lm_tmp=0.0)
    for lm_, w_ in ((None, None), (lm, 0.0)):                                        # nothing to fuse: a bonus has no total to go to
        with pytest.raises(ValueError):
            m.decode_logits_beam_lm(logits, None, 4, lm=lm_, lm_weight=w_, length_bonus=0.3)
        with pytest.raises(ValueError):
            m.beam_labels_fused(x, x_len, 4, lm=lm_, lm_weight=w_, length_bonus=0.3)
    with pytest.raises(ValueError):
        m.decode_logits_beam_lm(logits, None, 4, lm=lm, length_bonus=float("nan"))
    with pytest.raises(RuntimeError, match="HIP device only"):                       # nothing to fuse, bonus 0: the plain path, which has no CPU fallback
        m.decode_logits_beam_lm(logits, None, 4, lm_weight=-0.3)
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.decode_logits_beam_lm(logits, None, 4, lm=lm)
    assert m.last_beam_rounds() is None
