"""RNN-T beam search on the GPU (effconf_rnnt_beam, reference transducer.py:188-327 without LM / n-gram terms): token identity with
the reference's own beam_search_decoding (tests/golden/rnnt_beam_*.npz), scores against the float64 oracle (tests/rnnt_beam_ref.py),
independence of the evaluation batch and of the rows sharing a launch, the caps, edge cases and the mel -> tokens pipeline."""
import functools
import os

import numpy as np
import pytest
import torch

from efficientconformer_amd import named_config, synth
from rnnt_beam_ref import beam_decode

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _transducer(name, seed, blank_bias):
    from efficientconformer_amd import Transducer
    cfg = named_config(name)
    m = Transducer.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, seed, None, prefix="encoder.")
    tsd = synth.make_transducer_state_dict(m.encoder.plan.dim_out, cfg["decoder_params"], cfg["joint_params"], seed, blank_bias=blank_bias)
    sd.update(tsd)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda(), tsd


@functools.lru_cache(maxsize=None)
def _fixture(name, blank_bias=1.2):
    g = np.load(os.path.join(GOLDEN, "rnnt_%s.npz" % name))
    m, tsd = _transducer(name, int(g["weight_seed"]), blank_bias)
    return m, tsd, torch.from_numpy(g["f"]), torch.from_numpy(g["f_len"])


@functools.lru_cache(maxsize=None)
def _oracle(name, beam, blank_bias=1.2, max_expansions=None):
    _, tsd, f, f_len = _fixture(name, blank_bias)
    return beam_decode(tsd, f, f_len, beam, max_expansions=max_expansions)


def _decode(m, f, f_len, beam, **kw):
    tokens, token_len, score, status = m.decode_encoded_beam(f.cuda(), None if f_len is None else f_len.cuda(), beam, **kw)
    tokens, token_len, score, status = tokens.cpu(), token_len.cpu(), score.cpu(), status.cpu()
    toks = [tokens[i, :int(token_len[i])].tolist() for i in range(tokens.shape[0])]
    assert all(int(tokens[i, int(token_len[i]):].abs().sum()) == 0 for i in range(tokens.shape[0]))     # zero-filled tails
    return toks, score.numpy(), status.numpy()


@pytest.mark.parametrize("name", ["TinyTransducer", "EfficientConformerTransducerMedium"])
def test_beam_is_token_identical_to_reference(name):
    bg = np.load(os.path.join(GOLDEN, "rnnt_beam_%s.npz" % name))
    m, _, f, f_len = _fixture(name)
    for beam in bg["beams"].tolist():
        toks, score, status = _decode(m, f, f_len, beam)
        offs = bg["offsets_b%d" % beam]
        want = [bg["tokens_b%d" % beam][offs[i]:offs[i + 1]].tolist() for i in range(f.shape[0])]
        assert toks == want, (name, beam)
        assert (status == 0).all()
        ref = np.array([r["score"] for r in _oracle(name, beam)])
        assert np.all(np.abs(score - ref) <= 1e-4 * np.abs(ref)), (name, beam, score, ref)


@pytest.mark.parametrize("name", ["TinyTransducer", "EfficientConformerTransducerMedium"])
def test_beam_eval_batch_1_and_16_are_bit_identical(name):
    m, _, f, f_len = _fixture(name)
    try:
        m.set_decode_option("beam_eval_batch", 1)
        one = _decode(m, f, f_len, 16)
        st1 = m.last_beam_stats()
        m.set_decode_option("beam_eval_batch", 16)
        six = _decode(m, f, f_len, 16)
        st16 = m.last_beam_stats()
    finally:
        m.set_decode_option("beam_eval_batch", 16)
    assert one[0] == six[0]
    assert one[1].tobytes() == six[1].tobytes() and (one[2] == six[2]).all()
    assert (st1[:, 2] == st16[:, 2]).all()                          # the same expansions, in fewer weight passes
    assert (st1[:, 0] == st1[:, 1]).all() and (st16[:, 0] < st1[:, 0]).all()
    assert (st16[:, 3] == f_len.numpy()).all()


def test_beam_rows_do_not_depend_on_the_batch():
    """Each row alone, inside a 24-row ragged batch with repeated rows, and in reversed order: identical tokens and scores;
    a repeated run is bitwise equal."""
    m, _, f, f_len = _fixture("TinyTransducer")
    n = f.shape[0]
    src = [i % n for i in range(24)]
    lens = torch.tensor([max(1, int(f_len[s]) - (i // n) % 3) for i, s in enumerate(src)], dtype=torch.int64)
    fb = f[src].contiguous()
    batch = _decode(m, fb, lens, 4)
    alone = [_decode(m, fb[i:i + 1], lens[i:i + 1], 4) for i in range(24)]
    assert batch[0] == [a[0][0] for a in alone]
    assert batch[1].tobytes() == np.concatenate([a[1] for a in alone]).tobytes()
    rev = _decode(m, fb.flip(0), lens.flip(0), 4)
    assert rev[0][::-1] == batch[0] and rev[1][::-1].tobytes() == batch[1].tobytes()
    again = _decode(m, fb, lens, 4)
    assert again[0] == batch[0] and again[1].tobytes() == batch[1].tobytes()


def test_beam_edge_cases():
    m, tsd, f, f_len = _fixture("TinyTransducer")
    lens = torch.tensor([0, 1, int(f_len[2]), int(f_len[3])], dtype=torch.int64)
    toks, score, status = _decode(m, f, lens, 4)
    assert toks[0] == [] and status[0] == 0 and score[0] == 0
    want = beam_decode(tsd, f, lens, 4)
    assert toks == [r["tokens"] for r in want] and (status == 0).all()
    # x_len = None: every frame
    assert _decode(m, f, None, 4)[0] == _decode(m, f, torch.full((f.shape[0],), f.shape[1], dtype=torch.int64), 4)[0]
    # beam 1: at blank bias 1.2 no row terminates (the oracle's and the reference's beam 1 expand forever): every row capped;
    # at blank bias 2 the oracle's tokens and scores
    assert (_decode(m, f, f_len, 1)[2] == 1).all() and all(r["capped"] for r in _oracle("TinyTransducer", 1, 1.2, 16))
    m2 = _fixture("TinyTransducer", 2.0)[0]
    toks, score, status = _decode(m2, f, f_len, 1)
    ref = _oracle("TinyTransducer", 1, 2.0)
    assert toks == [r["tokens"] for r in ref] and (status == 0).all() and sum(len(t) for t in toks) > 0
    assert np.allclose(score, [r["score"] for r in ref], rtol=1e-4, atol=0)
    with pytest.raises(Exception):
        m.decode_encoded_beam(f.cuda(), f_len.cuda(), 17)


def test_beam_expansion_cap_flags_exactly_the_non_terminating_rows():
    """Blank bias 0: some rows never see blank in the top of the popped hypothesis (the reference loops forever).  Under the
    default cap (16 * beam expansions per frame) the kernel flags exactly the rows the oracle flags and decodes the rest."""
    m, tsd, f, f_len = _fixture("TinyTransducer", 0.0)
    ref = _oracle("TinyTransducer", 16, 0.0, 256)
    flagged = [i for i, r in enumerate(ref) if r["capped"]]
    assert flagged, "fixture no longer exercises the cap"
    assert 0 < len(flagged) < len(ref)
    toks, score, status = _decode(m, f, f_len, 16)
    assert [i for i in range(len(status)) if status[i] == 1] == flagged
    assert all(status[i] == 0 and toks[i] == ref[i]["tokens"] for i in range(len(ref)) if i not in flagged)
    assert all(toks[i] == [] for i in flagged)
    enc = m.__dict__.get("encoder")
    object.__setattr__(m, "encoder", lambda x, x_len: (f.cuda(), f_len.cuda(), None))
    try:
        with pytest.raises(Exception) as e:
            m.beam_search_decoding(torch.zeros(f.shape[0], 1), f_len, beam_size=16)
        assert str(flagged) in str(e.value) and "expansion cap" in str(e.value)
    finally:
        del m.__dict__["encoder"]
        if enc is not None:
            m.__dict__["encoder"] = enc
    # the token cap: status 2, no tokens
    toks, _, status = _decode(_fixture("TinyTransducer")[0], f, f_len, 4, max_tokens=3)
    assert (status == 2).all() and all(t == [] for t in toks)


def test_beam_workspace_contents_do_not_matter():
    """A workspace filled with 0xFF gives the same result as a fresh one."""
    from efficientconformer_amd import _lib
    m, _, f, f_len = _fixture("TinyTransducer")
    want = _decode(m, f, f_len, 16)
    lib = _lib.load()
    fd, ld = f.cuda().contiguous(), f_len.cuda()
    b, t, _ = f.shape
    max_tok = 16 * t
    nbytes = lib.effconf_rnnt_beam_workspace_bytes(m._rnnt, b, t, 16, 256, max_tok)
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device="cuda")
    tokens = torch.full((b, max_tok), -1, dtype=torch.int32, device="cuda")
    token_len = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    score = torch.full((b,), float("nan"), device="cuda")
    status = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.effconf_rnnt_beam(m._rnnt, fd.data_ptr(), ld.data_ptr(), b, t, 16, 1.0, 256, tokens.data_ptr(), token_len.data_ptr(),
                                     score.data_ptr(), status.data_ptr(), max_tok, ws.data_ptr(), nbytes,
                                     torch.cuda.current_stream().cuda_stream), "rnnt_beam")
    torch.cuda.synchronize()
    got = [tokens.cpu()[i, :int(token_len[i])].tolist() for i in range(b)]
    assert got == want[0] and score.cpu().numpy().tobytes() == want[1].tobytes() and (status.cpu() == 0).all()
    assert int(tokens.cpu()[0, int(token_len[0]):].abs().sum()) == 0


def test_beam_full_pipeline_from_mel_matches_oracle():
    """mel -> native encoder -> beam_tokens(from_mel=True) == the oracle's beam search of the same encoder output."""
    m, tsd = _transducer("TinyTransducer", 7, 1.2)
    mel, ln = synth.make_mel(3, 80, 100, [100, 61, 20], seed=17)
    mel, ln = torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda()
    got = m.beam_tokens(mel, ln, beam_size=4, from_mel=True)
    f, f_len, _ = m.encoder.forward_mel(mel, ln)
    want = beam_decode(tsd, f.float().cpu(), f_len.cpu(), 4)
    assert got == [r["tokens"] for r in want]
