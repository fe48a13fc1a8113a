"""RNN-T beam search with neural-LM shallow fusion on the GPU (effconf_rnnt_beam_lm, reference transducer.py:188-327 with its LM term): token identity
with the reference's own fused beam_search_decoding (tests/golden/rnnt_beam_lm_TinyTransducer.npz), scores against the float64 oracle
(tests/rnnt_beam_lm_ref.py), independence of the evaluation batch, of the rows sharing a call and of the chunking, the caps, edge cases, the routing of
``Transducer.lm`` / ``lm_weight`` and the mel -> tokens pipeline.

Shapes: Tiny - f (4, 13, 48), lengths 13 / 10 / 7 / 2, H = J = 32, V = 40 (V % 16 != 0: the clamped vocabulary tile), TinyLM 32 x 2 layers (the
[W_ih | W_hh] path).  Batches of 1, 2 and 3 utterances are 16 / 32 / 48 LM columns: lm_lstm_step_kernel<1>, <2> and <4>."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from efficientconformer_amd import _lib, named_config, synth
import rnnt_beam_lm_cases as cases
from rnnt_beam_lm_ref import beam_decode_lm

pytestmark = pytest.mark.gpu

W, BB = 0.3, 2.0                      # the golden's lm_weight and blank bias (asserted against the file in the host test)


@functools.lru_cache(maxsize=None)
def _model(name=cases.TINY, blank_bias=BB):
    from efficientconformer_amd import Transducer
    cfg = named_config(name)
    m = Transducer.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, cases.encoded(name)[2], None, prefix="encoder.")
    sd.update(cases.transducer_sd(name, blank_bias))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda()


def _make_lm(params, sd):
    from efficientconformer_amd import LanguageModel
    lm = LanguageModel(dict(params))
    lm.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return lm


@functools.lru_cache(maxsize=None)
def _lm(name=cases.TINY):
    return _make_lm(*(cases.tiny_lm() if name == cases.TINY else cases.medium_lm())).cuda()


def _decode(m, f, f_len, beam, **kw):
    tokens, token_len, score, status = m.decode_encoded_beam_lm(f.cuda(), None if f_len is None else f_len.cuda(), beam, **kw)
    tokens, token_len, score, status = tokens.cpu(), token_len.cpu(), score.cpu(), status.cpu()
    toks = [tokens[i, :int(token_len[i])].tolist() for i in range(tokens.shape[0])]
    assert all(int(tokens[i, int(token_len[i]):].abs().sum()) == 0 for i in range(tokens.shape[0]))     # zero-filled tails
    return toks, score.numpy(), status.numpy()


def _fused(f, f_len, beam, m=None, **kw):
    kw.setdefault("lm_weight", W)
    return _decode(m or _model(), f, f_len, beam, lm=_lm(), **kw)


def _same(a, b):
    return a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and (a[2] == b[2]).all()


@contextlib.contextmanager
def _encoder_returns(m, f, f_len):
    """``m.encoder(x, x_len)`` returns the stored encoder outputs (the pattern of test_gpu_rnnt_beam.py's cap test)."""
    enc = m.__dict__.get("encoder")
    object.__setattr__(m, "encoder", lambda x, x_len: (f.cuda(), f_len.cuda(), None))
    try:
        yield
    finally:
        del m.__dict__["encoder"]
        if enc is not None:
            m.__dict__["encoder"] = enc


@pytest.mark.parametrize("beam", [4, 16])
def test_fused_beam_is_token_identical_to_reference(beam):
    f, f_len, _ = cases.encoded(cases.TINY)
    toks, score, status = _fused(f, f_len, beam)
    assert toks == cases.golden_tokens(beam)
    assert (status == 0).all()
    ref = np.array([r["score"] for r in cases.oracle(cases.TINY, beam, BB, W)])
    print("score", score, "oracle", ref)
    assert np.all(np.abs(score - ref) <= 1e-4 * np.abs(ref)), (beam, score, ref)


@pytest.mark.parametrize("beam", [4, 16])
def test_fused_beam_with_both_temperatures_matches_oracle(beam):
    f, f_len, _ = cases.encoded(cases.TINY)
    m = _model()
    ref = cases.oracle(cases.TINY, beam, BB, W, 1.3, 2.0)
    try:
        m.tmp = 1.3
        toks, score, status = _fused(f, f_len, beam, lm_tmp=2.0)
    finally:
        m.tmp = 1.0
    assert toks == [r["tokens"] for r in ref] and (status == 0).all()
    want = np.array([r["score"] for r in ref])
    print("score", score, "oracle", want)
    assert np.all(np.abs(score - want) <= 1e-4 * np.abs(want)), (score, want)


def test_fused_eval_batch_1_and_16_are_bit_identical():
    f, f_len, _ = cases.encoded(cases.TINY)
    m = _model()
    try:
        m.set_decode_option("beam_eval_batch", 1)
        one = _fused(f, f_len, 16)
        st1, r1 = m.last_beam_stats(), m.last_beam_rounds()
        m.set_decode_option("beam_eval_batch", 16)
        six = _fused(f, f_len, 16)
        st16, r16 = m.last_beam_stats(), m.last_beam_rounds()
    finally:
        m.set_decode_option("beam_eval_batch", 16)
    assert _same(one, six)
    assert (st1[:, 2] == st16[:, 2]).all()                          # the same expansions ...
    assert (st1[:, 0] == st1[:, 1]).all() and (st16[:, 0] < st1[:, 0]).all()        # ... in fewer evaluation batches
    assert (st16[:, 3] == f_len.numpy()).all()
    print("rounds", r1, r16)
    assert len(r1) == len(r16) == 1 and r16[0] < r1[0]              # and fewer LM steps
    ref = cases.oracle(cases.TINY, 16, BB, W)
    assert (st16[:, 2] == [sum(r["expansions"]) for r in ref]).all()


def test_fused_rows_do_not_depend_on_the_batch(monkeypatch):
    """Each row alone (16 LM columns), pairs (32), triples (48), a 24-row ragged batch with repeated rows, its reverse: identical tokens and bitwise equal
    scores; a repeated run is bitwise equal; chunks under a small byte cap equal the unchunked call."""
    from efficientconformer_amd import transducer
    f, f_len, _ = cases.encoded(cases.TINY)
    m = _model()
    n = f.shape[0]
    src = [i % n for i in range(24)]
    lens = torch.tensor([max(1, int(f_len[s]) - (i // n) % 3) for i, s in enumerate(src)], dtype=torch.int64)
    fb = f[src].contiguous()
    batch = _fused(fb, lens, 4)
    assert len(m.last_beam_rounds()) == 1
    assert batch[0][:n] == cases.golden_tokens(4)
    for width in (1, 2, 3):
        parts = [_fused(fb[i:i + width], lens[i:i + width], 4) for i in range(0, 24, width)]
        assert batch[0] == [t for p in parts for t in p[0]], width
        assert batch[1].tobytes() == np.concatenate([p[1] for p in parts]).tobytes(), width
        assert (np.concatenate([p[2] for p in parts]) == 0).all()
    rev = _fused(fb.flip(0), lens.flip(0), 4)
    assert rev[0][::-1] == batch[0] and rev[1][::-1].tobytes() == batch[1].tobytes()
    assert _same(_fused(fb, lens, 4), batch)
    one = _lib.load().effconf_rnnt_beam_lm_workspace_bytes(m._rnnt, _lm()._handle, 1, fb.shape[1], 4, 64, 16 * fb.shape[1])
    monkeypatch.setattr(transducer, "BEAM_LM_WORKSPACE_CAP", 5 * one)
    chunked = _fused(fb, lens, 4)
    assert len(m.last_beam_rounds()) > 1 and m.last_beam_stats().shape == (24, 4)
    assert _same(chunked, batch)


def test_fused_edge_cases():
    f, f_len, _ = cases.encoded(cases.TINY)
    m, lm = _model(), _lm()
    lens = torch.tensor([0, 1, int(f_len[2]), int(f_len[3])], dtype=torch.int64)
    toks, score, status = _fused(f, lens, 4)
    assert toks[0] == [] and status[0] == 0 and score[0] == 0
    want = beam_decode_lm(cases.transducer_sd(cases.TINY, BB), cases.tiny_lm()[1], f, lens, 4, W, max_expansions=64)
    assert toks == [r["tokens"] for r in want] and (status == 0).all() and len(toks[1]) > 0
    # no frames at all: nothing to search, one launch, no LM step
    toks, score, status = _fused(f[:2], torch.zeros(2, dtype=torch.int64), 4)
    assert toks == [[], []] and (status == 0).all() and (score == 0).all() and m.last_beam_rounds() == [1]
    # x_len = None: every frame
    assert _same(_fused(f, None, 4), _fused(f, torch.full((f.shape[0],), f.shape[1], dtype=torch.int64), 4))
    with pytest.raises(_lib.EffconfError):
        m.decode_encoded_beam_lm(f.cuda(), f_len.cuda(), 17, lm=lm, lm_weight=W)
    # an LM of another vocabulary: refused by the size query, before anything is launched
    params, _ = cases.tiny_lm()
    p41 = dict(params, vocab_size=41)
    lm41 = _make_lm(p41, synth.make_lm_state_dict(p41, 3)).cuda()
    with pytest.raises(_lib.EffconfError, match="vocab_size"):
        m.decode_encoded_beam_lm(f.cuda(), f_len.cuda(), 4, lm=lm41, lm_weight=W)
    # an LM on the CPU: no CPU path
    with pytest.raises(RuntimeError):
        m.decode_encoded_beam_lm(f.cuda(), f_len.cuda(), 4, lm=_make_lm(*cases.tiny_lm()), lm_weight=W)
    # a handle that was never finalized (the raw C call); a weight or temperature the entry refuses
    lib = _lib.load()
    raw = lib.effconf_lm_create(C.byref(_lib.EcLmConfig(40, 32, 2)))
    try:
        b, t, _ = f.shape
        fd, ld = f.cuda().contiguous(), f_len.cuda()
        nbytes = lib.effconf_rnnt_beam_lm_workspace_bytes(m._rnnt, raw, b, t, 4, 64, 16 * t)
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        outs = [torch.zeros(b, 16 * t, dtype=torch.int32, device="cuda"), torch.zeros(b, dtype=torch.int32, device="cuda"),
                torch.zeros(b, device="cuda"), torch.zeros(b, dtype=torch.int32, device="cuda")]

        def call(handle, weight, lm_tmp):
            return lib.effconf_rnnt_beam_lm(m._rnnt, handle, fd.data_ptr(), ld.data_ptr(), b, t, 4, 1.0, weight, lm_tmp, 64, outs[0].data_ptr(), outs[1].data_ptr(),
                                            outs[2].data_ptr(), outs[3].data_ptr(), 16 * t, None, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        assert call(raw, W, 1.0) != 0 and b"not finalized" in lib.effconf_last_error()
        for weight, lm_tmp in ((0.0, 1.0), (-0.1, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (W, 0.0), (W, float("inf"))):
            assert call(lm._handle, weight, lm_tmp) != 0, (weight, lm_tmp)
        assert call(lm._handle, W, 1.0) == 0
        torch.cuda.synchronize()
    finally:
        lib.effconf_lm_destroy(raw)


def test_fused_expansion_cap_flags_exactly_the_non_terminating_rows():
    """Blank bias 1.2, beam 4, weight 0.3: the LM's token-0 probability lands on blank and rows 0 and 1 never fill B (the reference's behaviour).  Under the default cap
    (16 * beam = 64 expansions per frame) the search flags exactly the rows the oracle flags and decodes the rest."""
    f, f_len, _ = cases.encoded(cases.TINY)
    m = _model(cases.TINY, 1.2)
    ref = cases.oracle(cases.TINY, 4, 1.2, W, max_expansions=64)
    flagged = [i for i, r in enumerate(ref) if r["capped"]]
    assert flagged == [0, 1]
    toks, score, status = _fused(f, f_len, 4, m=m)
    assert [i for i in range(len(status)) if status[i] == 1] == flagged
    assert all(status[i] == 0 and toks[i] == ref[i]["tokens"] for i in range(len(ref)) if i not in flagged)
    assert all(toks[i] == [] and score[i] == 0 for i in flagged)
    m.lm, m.lm_weight = _lm(), W
    try:
        with _encoder_returns(m, f, f_len):
            with pytest.raises(_lib.EffconfError) as e:
                m.beam_search_decoding(torch.zeros(f.shape[0], 1), f_len, beam_size=4)
        assert str(flagged) in str(e.value) and "expansion cap" in str(e.value)
    finally:
        m.lm, m.lm_weight = None, 0.0
    # the token cap: status 2, no tokens
    toks, _, status = _fused(f, f_len, 4, max_tokens=3)
    assert (status == 2).all() and all(t == [] for t in toks)


def test_fused_workspace_contents_do_not_matter():
    """A workspace filled with 0xFF gives the bits of a fresh one (the raw C call)."""
    f, f_len, _ = cases.encoded(cases.TINY)
    m, lm = _model(), _lm()
    want = _fused(f, f_len, 16)
    lib = _lib.load()
    fd, ld = f.cuda().contiguous(), f_len.cuda()
    b, t, _ = f.shape
    max_tok = 16 * t
    nbytes = lib.effconf_rnnt_beam_lm_workspace_bytes(m._rnnt, lm._handle, b, t, 16, 256, max_tok)
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device="cuda")
    tokens = torch.full((b, max_tok), -1, dtype=torch.int32, device="cuda")
    token_len = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    score = torch.full((b,), float("nan"), device="cuda")
    status = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    rounds = C.c_int32(-1)
    _lib.check(lib.effconf_rnnt_beam_lm(m._rnnt, lm._handle, fd.data_ptr(), ld.data_ptr(), b, t, 16, 1.0, W, 1.0, 256, tokens.data_ptr(), token_len.data_ptr(),
                                        score.data_ptr(), status.data_ptr(), max_tok, C.byref(rounds), ws.data_ptr(), nbytes,
                                        torch.cuda.current_stream().cuda_stream), "rnnt_beam_lm")
    torch.cuda.synchronize()
    got = [tokens.cpu()[i, :int(token_len[i])].tolist() for i in range(b)]
    assert got == want[0] and score.cpu().numpy().tobytes() == want[1].tobytes() and (status.cpu() == 0).all()
    assert int(tokens.cpu()[0, int(token_len[0]):].abs().sum()) == 0
    assert rounds.value == m.last_beam_rounds()[0] > 1


def test_attached_lm_and_weight_route_the_search():
    """``model.lm`` attached with lm_weight 0: the plain search, to the bit.  Attached with weight 0.3: beam_search_decoding is the fused search."""
    f, f_len, _ = cases.encoded(cases.TINY)
    m = _model()
    plain = _decode(m, f, f_len, 4)
    assert m.last_beam_rounds() is None
    m.lm = _lm()
    try:
        assert m.lm_weight == 0
        assert _same(_decode(m, f, f_len, 4), plain) and m.last_beam_rounds() is None
        m.lm_weight = W
        attached = _decode(m, f, f_len, 4)
        assert _same(attached, _fused(f, f_len, 4)) and attached[0] != plain[0]
        with _encoder_returns(m, f, f_len):
            x = torch.zeros(f.shape[0], 1)
            got = m.beam_search_decoding(x, f_len, beam_size=4)
            m.lm_weight = 0.0
            assert got == m.beam_tokens(x, f_len, 4, lm=_lm(), lm_weight=W) == cases.golden_tokens(4)
            assert m.beam_search_decoding(x, f_len, beam_size=4) == plain[0]
    finally:
        m.lm, m.lm_weight = None, 0.0
    with pytest.raises(ValueError):
        m.decode_encoded_beam_lm(f.cuda(), f_len.cuda(), 4, lm=_lm(), lm_weight=-0.3)


def test_fused_full_pipeline_from_mel_matches_oracle():
    """mel -> native encoder -> beam_tokens(from_mel=True, lm=...) == the oracle's fused search of the same encoder output."""
    m = _model()
    mel, ln = synth.make_mel(3, 80, 100, [100, 61, 20], seed=17)
    mel, ln = torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda()
    got = m.beam_tokens(mel, ln, beam_size=4, from_mel=True, lm=_lm(), lm_weight=W)
    f, f_len, _ = m.encoder.forward_mel(mel, ln)
    want = beam_decode_lm(cases.transducer_sd(cases.TINY, BB), cases.tiny_lm()[1], f.float().cpu(), f_len.cpu(), 4, W, max_expansions=64)
    assert not any(r["capped"] for r in want)
    assert got == [r["tokens"] for r in want]


def test_fused_beam_at_production_widths():
    """EfficientConformerTransducerMedium's decoder and joint (width 640, vocabulary 1000) at beam 16, on the first half of the stored frames, with a synthetic
    LM of the transducer's vocabulary, 48 x 3 layers: tokens identical to the float64 oracle on every utterance (the host test asserts that the oracle's
    float32 evaluation agrees with float64 for this seed and weight)."""
    f, f_len, _ = cases.encoded(cases.MEDIUM)
    m = _model(cases.MEDIUM, 1.2)
    ref = cases.oracle(cases.MEDIUM, 16, 1.2, cases.MEDIUM_LM_WEIGHT, max_expansions=256)
    assert not any(r["capped"] for r in ref)
    toks, score, status = _decode(m, f, f_len, 16, lm=_lm(cases.MEDIUM), lm_weight=cases.MEDIUM_LM_WEIGHT)
    assert toks == [r["tokens"] for r in ref] and (status == 0).all()
    want = np.array([r["score"] for r in ref])
    print("score", score, "oracle", want)
    assert np.all(np.abs(score - want) <= 1e-4 * np.abs(want)), (score, want)
