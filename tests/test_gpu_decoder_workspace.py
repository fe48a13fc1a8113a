"""A decoder entry stays inside the workspace size it reports, wherever the caller's pointer sits: the C entries take any pointer and align it up once
(csrc/decode_layout.h, WsPlan), and `*_workspace_bytes` reserves exactly that one alignment.

Each entry runs through ctypes on ONE torch allocation of workspace_bytes + 16 + 4096 bytes: it is handed `ptr + 16` (torch allocations are 256-aligned, so
the entry spends 240 bytes of its slack) and `workspace_bytes`; the 4096 bytes behind that hold a pattern.  The pattern must be intact, and every output must
equal the run on an aligned pointer.  The guard bytes belong to the test's own allocation: nothing can fault whatever the outcome.

The greedy entry is the one whose size and carve were two formulas (the carve aligned a second time behind the linear_encoder region); it runs the cluster
decode here: (De, H, J, V) = (48, 64, 64, 40), B = 19, T = 13, cluster_decode = 1.  The beam, lattice and LM entries follow on the same model."""
import functools

import numpy as np
import pytest
import torch

from efficientconformer_amd import LanguageModel, Transducer, _lib, named_config, synth

pytestmark = pytest.mark.gpu

GUARD = 4096
B, T, H, J, V = 19, 13, 64, 64, 40


@functools.lru_cache(maxsize=None)
def _transducer():
    import copy
    cfg = copy.deepcopy(named_config("TinyTransducer"))
    cfg["decoder_params"].update(dim_model=H, vocab_size=V)
    cfg["joint_params"].update(dim_model=J)
    if "tokenizer_params" in cfg:
        cfg["tokenizer_params"]["vocab_size"] = V
    m = Transducer.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, 11, None, prefix="encoder.")
    sd.update(synth.make_transducer_state_dict(m.encoder.plan.dim_out, cfg["decoder_params"], cfg["joint_params"], 11, blank_bias=1.2))
    m.load_state_dict({k: torch.from_numpy(a) for k, a in sd.items()})
    m = m.cuda()
    m._ensure_rnnt()
    g = np.random.Generator(np.random.PCG64(77))
    f = torch.from_numpy(g.standard_normal((B, T, m.encoder.plan.dim_out)).astype(np.float32)).cuda()
    f_len = torch.from_numpy(np.array([13, 0, 7, 13, 1, 12, 5] + list(g.integers(0, T + 1, B - 7)), dtype=np.int64)).cuda()
    return m, f, f_len


def _both(nbytes, call):
    """call(workspace pointer, workspace bytes) -> output tensors; on a guarded, misaligned workspace and on an aligned one."""
    assert nbytes > 0
    pattern = (torch.arange(GUARD, device="cuda") % 251).to(torch.uint8)
    buf = torch.full((nbytes + 16 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    buf[-GUARD:] = pattern
    got = call(buf.data_ptr() + 16, nbytes)
    torch.cuda.synchronize()
    assert torch.equal(buf[-GUARD:], pattern), "the entry wrote behind the workspace size it reported"
    aligned = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    want = call(aligned.data_ptr(), nbytes)
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    return got


def _stream():
    return torch.cuda.current_stream().cuda_stream


def test_greedy_cluster_decode_stays_inside_its_workspace():
    m, f, f_len = _transducer()
    lib = _lib.load()
    max_tok = int(lib.effconf_rnnt_max_tokens(m._rnnt, T))
    m.set_decode_option("cluster_decode", 1)
    try:
        def call(ws, nbytes):
            tokens = torch.full((B, max_tok), -1, dtype=torch.int32, device="cuda")
            token_len = torch.full((B,), -1, dtype=torch.int32, device="cuda")
            _lib.check(lib.effconf_rnnt_greedy(m._rnnt, f.data_ptr(), f_len.data_ptr(), B, T, tokens.data_ptr(), token_len.data_ptr(), max_tok, ws, nbytes, _stream()),
                       "rnnt_greedy")
            return tokens, token_len
        tokens, token_len = _both(int(lib.effconf_rnnt_workspace_bytes(m._rnnt, B, T)), call)
    finally:
        m.set_decode_option("cluster_decode", -1)
    assert int(token_len.min()) >= 0 and int(token_len.sum()) > 0
    ref_tokens, ref_len = m.decode_encoded(f, f_len)                 # the default route at this batch, on torch's aligned workspace
    assert torch.equal(tokens, ref_tokens) and torch.equal(token_len, ref_len)


def test_beam_stays_inside_its_workspace():
    m, f, f_len = _transducer()
    lib = _lib.load()
    beam, max_exp, max_tok = 4, 64, 16 * T

    def call(ws, nbytes):
        tokens = torch.full((B, max_tok), -1, dtype=torch.int32, device="cuda")
        outs = [torch.full((B,), -1, dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.int32)]
        _lib.check(lib.effconf_rnnt_beam(m._rnnt, f.data_ptr(), f_len.data_ptr(), B, T, beam, 1.0, max_exp, tokens.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                         outs[2].data_ptr(), max_tok, ws, nbytes, _stream()), "rnnt_beam")
        return [tokens] + outs
    _, token_len, _, status = _both(int(lib.effconf_rnnt_beam_workspace_bytes(m._rnnt, B, T, beam, max_exp, max_tok)), call)
    assert int((status == 0).sum()) > 0 and int(token_len.sum()) > 0


def test_lattice_stays_inside_its_workspace():
    m, f, f_len = _transducer()
    lib = _lib.load()
    u = 5
    g = np.random.Generator(np.random.PCG64(78))
    y = torch.from_numpy(g.integers(1, V, (B, u)).astype(np.int32)).cuda()
    y_len = torch.from_numpy((np.arange(B) % (u + 1)).astype(np.int64)).cuda()

    def call(ws, nbytes):
        planes = [torch.full((B, T, u + 1), 7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
        status = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        _lib.check(lib.effconf_rnnt_lattice(m._rnnt, f.data_ptr(), f_len.data_ptr(), B, T, y.data_ptr(), y_len.data_ptr(), u, 1.0, planes[0].data_ptr(),
                                            planes[1].data_ptr(), status.data_ptr(), ws, nbytes, _stream()), "rnnt_lattice")
        return planes + [status]
    lpb, _, status = _both(int(lib.effconf_rnnt_lattice_workspace_bytes(m._rnnt, B, T, u)), call)
    assert int((status == 0).sum()) > 0 and float(lpb.min()) < 0


def test_lm_score_stays_inside_its_workspace():
    params = dict(arch="RNN", vocab_size=V, dim_model=64, num_layers=2)
    lm = LanguageModel(params)
    lm.load_state_dict({k: torch.from_numpy(a) for k, a in synth.make_lm_state_dict(params, 5).items()})
    lm = lm.cuda()
    lm._ensure()
    lib = _lib.load()
    n, u = 17, 6
    g = np.random.Generator(np.random.PCG64(79))
    y = torch.from_numpy(g.integers(1, V, (n, u)).astype(np.int32)).cuda()
    y_len = torch.from_numpy((np.arange(n) % (u + 1)).astype(np.int64)).cuda()

    def call(ws, nbytes):
        token_logp = torch.full((n, u), 7.0, dtype=torch.float32, device="cuda")
        score = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
        status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        _lib.check(lib.effconf_lm_score(lm._handle, y.data_ptr(), y_len.data_ptr(), n, u, 1.0, token_logp.data_ptr(), score.data_ptr(), status.data_ptr(), ws, nbytes,
                                        _stream()), "lm_score")
        return token_logp, score, status
    _, score, status = _both(int(lib.effconf_lm_workspace_bytes(lm._handle, n, u)), call)
    assert int(status.abs().sum()) == 0 and float(score.min()) < 0
