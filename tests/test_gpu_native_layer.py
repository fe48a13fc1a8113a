"""Every decode entry point of the Python wrappers on a poisoned fresh workspace (EFFCONF_POISON_WORKSPACE, efficientconformer_amd/_native.py
``workspace``): the greedy CTC head, the margin head, the per-range hooks, the CTC beam search, RNN-T greedy (per-utterance and cluster kernels) and the
RNN-T beam search allocate through the one hook, so "no kernel reads workspace nobody wrote" holds for them as it does for the encoder
(tests/test_gpu_round6.py), the alignments and the LM.  Outputs are bit-identical to the run with the variable unset for the fills 0 (zeros),
127 (huge finite values) and 255 (NaN patterns; for the CTC beam search 255 is the hash table's own empty key, so 0 and 127 are the fills that tell)."""
import functools

import pytest
import torch

from efficientconformer_amd import ModelCTC, Transducer, named_config, synth

pytestmark = pytest.mark.gpu

POISON = "EFFCONF_POISON_WORKSPACE"
LENS = [97, 64, 33]                # mel frames: three utterances, two of them padded
CLUSTER_BATCH = 19                 # tests/test_gpu_encoder.py::test_rnnt_cluster_decode_equals_per_utterance_decode: two clusters of 8, one partly filled


@functools.lru_cache(maxsize=None)
def _mel(n_mels):
    mel, ln = synth.make_mel(len(LENS), n_mels, max(LENS), LENS, seed=97)
    return torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda()


@functools.lru_cache(maxsize=None)
def _ctc():
    """-> (model, enc, enc_len, logits): the Tiny CTC model, its encoder output for the batch and the head's logits (inputs of the entries, computed once)."""
    cfg = named_config("Tiny")
    m = ModelCTC.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, 7, cfg["tokenizer_params"]["vocab_size"], prefix="encoder.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda()
    enc, enc_len, _ = m.encoder.forward_mel(*_mel(m.encoder.plan.n_mels))
    return m, enc, enc_len, m._head(enc, enc_len, want_logits=True)[0]


@functools.lru_cache(maxsize=None)
def _rnnt():
    """-> (model, f, f_len, f19, f19_len): TinyTransducer, its encoder output for the batch, and the same rows repeated to the cluster test's batch with
    lengths that shrink from copy to copy (down to utterances without frames)."""
    cfg = named_config("TinyTransducer")
    m = Transducer.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, 7, None, prefix="encoder.")
    sd.update(synth.make_transducer_state_dict(m.encoder.plan.dim_out, cfg["decoder_params"], cfg["joint_params"], 7, blank_bias=1.2))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda()
    f, f_len, _ = m.encoder.forward_mel(*_mel(m.encoder.plan.n_mels))
    rows = [i % len(LENS) for i in range(CLUSTER_BATCH)]
    host = f_len.cpu()
    f19_len = torch.tensor([max(0, int(host[r]) - 3 * (i // len(LENS))) for i, r in enumerate(rows)]).cuda()
    return m, f, f_len, f[rows].contiguous(), f19_len


def _greedy_rnnt(cluster):
    m, _, _, f19, f19_len = _rnnt()
    m.set_decode_option("cluster_decode", cluster)
    try:
        return m.decode_encoded(f19, f19_len)
    finally:
        m.set_decode_option("cluster_decode", -1)


def _encode_greedy():
    m = _ctc()[0]
    m.encoder.sub_batches = 2                          # two row ranges: the head runs in the per-range hook, one of them on a side stream
    m.encoder._ws.clear()                              # the encoder's own workspaces are fresh (and filled) as well
    try:
        return m.encode_greedy(*_mel(m.encoder.plan.n_mels), from_mel=True)
    finally:
        m.encoder.sub_batches = 1


def _encode_margins():
    m = _ctc()[0]
    m.encoder.sub_batches = 2                          # the margin head per row range: its frame margins live in the workspace
    try:
        return m._encode_margins(*_mel(m.encoder.plan.n_mels), True, None)
    finally:
        m.encoder.sub_batches = 1


ENTRIES = {
    "head_fp32_rows": lambda: _ctc()[0]._head(_ctc()[1], _ctc()[2], want_logits=True),
    "head_bf16_rows": lambda: _ctc()[0]._head(_ctc()[1].bfloat16(), _ctc()[2], want_logits=True),
    "head_margins": lambda: _ctc()[0].head_margins(_ctc()[1], _ctc()[2], want_logits=True),
    "encode_greedy_2_ranges": _encode_greedy,
    "encode_margins_2_ranges": _encode_margins,
    "decode_logits_beam_4": lambda: _ctc()[0].decode_logits_beam(_ctc()[3], _ctc()[2], 4),
    "decode_encoded_default": lambda: _greedy_rnnt(-1),
    "decode_encoded_cluster_0": lambda: _greedy_rnnt(0),
    "decode_encoded_cluster_1": lambda: _greedy_rnnt(1),
    "decode_encoded_beam_4": lambda: _rnnt()[0].decode_encoded_beam(_rnnt()[1], _rnnt()[2], 4),
}


def _run(entry):
    out = ENTRIES[entry]()
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out if t is not None)


@functools.lru_cache(maxsize=None)
def _unpoisoned(entry):
    return _run(entry)


@pytest.mark.parametrize("fill", ["0", "127", "255"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_decode_entry_on_a_poisoned_workspace_is_bit_identical(monkeypatch, entry, fill):
    monkeypatch.delenv(POISON, raising=False)
    want = _unpoisoned(entry)                          # inputs and reference with the variable unset, once per entry
    monkeypatch.setenv(POISON, fill)
    got = _run(entry)
    assert len(got) == len(want) and len(want) >= 2
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (entry, fill, k)
        assert torch.equal(g, w), (entry, fill, k, int((g != w).sum()))
        if g.dtype.is_floating_point:
            assert not bool(torch.isnan(g).any()), (entry, fill, k)
