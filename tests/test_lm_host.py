"""LSTM language model, CPU side (no GPU): the float64 oracle (tests/lm_ref.py) against the reference's own float64 run stored in
tests/golden/lm_*.npz and against torch.nn.LSTM in float64; the state-dict surface against the reference's LanguageModel for configs/LM-RNN.json;
what the C surface refuses; the selection rule of ModelCTC.rescore_nbest on hand-made scores."""
import ctypes as C

import numpy as np
import pytest
import torch

import lm_ref
from lm_cases import fixture, torch_lm
from efficientconformer_amd import LanguageModel, _lib, select_nbest, synth

LM_RNN = dict(arch="RNN", num_layers=3, vocab_size=1000, dim_model=4096)       # configs/LM-RNN.json lm_params


@pytest.mark.parametrize("name", ["TinyLM", "LM257"])
def test_oracle_equals_the_reference_float64_run_and_torch_float64(name):
    g, params, sd = fixture(name)
    y, lens = g["tokens"], g["token_len"]
    got = lm_ref.forward_logits(sd, y, lens)
    assert got.shape == g["logits_f64"].shape and g["logits_f64"].dtype == np.float64
    assert np.abs(got - g["logits_f64"]).max() <= 1e-10
    assert set(lens.tolist()) >= {0, 1, 2, y.shape[1]}
    run = torch_lm(params, sd, torch.float64)
    x = np.concatenate([np.zeros((y.shape[0], 1), dtype=np.int64), y], axis=1)
    full = run(x)[0].numpy()
    for i, n in enumerate(lens):                     # positions of the sequence itself: what follows a pad token is not the reference's output
        assert np.abs(full[i, :n + 1] - g["logits_f64"][i, :n + 1]).max() <= 1e-10
        assert np.abs(got[i, :n + 1] - full[i, :n + 1]).max() <= 1e-10
    # the decode walk: 5 steps from zero state
    state, tstate = None, None
    for k in range(g["walk_tokens"].shape[0]):
        lg, state = lm_ref.step(sd, g["walk_tokens"][k], state)
        tl, tstate = run(g["walk_tokens"][k][:, None], tstate)
        assert np.abs(lg - g["walk_logits_f64"][k]).max() <= 1e-10
        assert np.abs(lg - tl[:, 0].numpy()).max() <= 1e-10
    assert np.abs(state[0] - g["walk_h_f64"]).max() <= 1e-10 and np.abs(state[1] - g["walk_c_f64"]).max() <= 1e-10
    # per-token log-probabilities are the log_softmax of these logits at the next token
    lp, score, status = lm_ref.token_logprobs(sd, y, lens, tmp=2.0)
    want = lm_ref.log_softmax(g["logits_f64"] / 2.0)
    for i, n in enumerate(lens):
        assert status[i] == 0
        assert np.abs(lp[i, :n] - np.array([want[i, k, y[i, k]] for k in range(n)])).max(initial=0.0) <= 1e-10
        assert (lp[i, n:] == 0).all() and abs(score[i] - lp[i, :n].sum()) <= 1e-10
    assert score[list(lens).index(0)] == 0


def test_state_dict_surface_is_the_reference_language_model():
    g, _, _ = fixture("TinyLM")
    keys = bytes(g["lmrnn_keys"]).decode().split("\n")
    shapes = [tuple(int(v) for v in row if v) for row in g["lmrnn_shapes"]]
    with torch.device("meta"):
        m = LanguageModel(LM_RNN, dict(vocab_size=1000))
    sd = m.state_dict()
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert sorted(synth.make_lm_state_dict(dict(LM_RNN, dim_model=16, vocab_size=5), 0)) == sorted(keys)
    cfg = LanguageModel.from_config({"lm_params": dict(LM_RNN, dim_model=16, vocab_size=5), "decoding_params": {"lm_tmp": 2}})
    assert cfg.lm_tmp == 2.0 and cfg.chunk_size() % 64 == 0
    with torch.device("meta"):
        assert LanguageModel(LM_RNN).chunk_size() * 12 * 3 * 4096 <= 1 << 30


def _create(v, h, layers):
    lib = _lib.load()
    cfg = _lib.EcLmConfig(v, h, layers)
    return lib, lib.effconf_lm_create(C.byref(cfg))


def test_the_c_surface_refuses_without_a_gpu():
    for v, h, layers, word in ((40, 40, 2, "multiple of 16"), (40, 32, 5, "num_layers"), (40, 32, 0, "num_layers"), (40, 8192, 2, "dim_model"),
                               (1, 32, 2, "vocab_size")):
        lib, handle = _create(v, h, layers)
        assert not handle
        assert word in lib.effconf_last_error().decode()
    with pytest.raises(NotImplementedError):
        LanguageModel(dict(LM_RNN, arch="Transformer"))
    with pytest.raises(Exception):
        LanguageModel(dict(LM_RNN, arch="GRU"))
    lib, handle = _create(40, 32, 2)
    assert handle
    try:
        sd = synth.make_lm_state_dict(dict(vocab_size=40, dim_model=32, num_layers=2), 0)
        for key, arr in sd.items():
            if key == "decoder.rnn.weight_hh_l1":
                continue
            shape = (C.c_int64 * arr.ndim)(*arr.shape)
            assert lib.effconf_lm_load_tensor(handle, key.encode(), arr.ctypes.data_as(C.c_void_p), shape, arr.ndim) == 0
        assert lib.effconf_lm_finalize(handle) != 0
        assert "missing tensor decoder.rnn.weight_hh_l1" in lib.effconf_last_error().decode()
        bad = np.zeros((4 * 32, 16), dtype=np.float32)
        shape = (C.c_int64 * 2)(*bad.shape)
        assert lib.effconf_lm_load_tensor(handle, b"decoder.rnn.weight_hh_l1", bad.ctypes.data_as(C.c_void_p), shape, 2) == 0
        assert lib.effconf_lm_finalize(handle) != 0
        assert "bad shape for decoder.rnn.weight_hh_l1" in lib.effconf_last_error().decode()
        assert lib.effconf_lm_workspace_bytes(handle, 33, 40) == 256 + 256 + 2 * 3 * 64 * 32 * 4
        assert lib.effconf_lm_workspace_bytes(handle, 0, 0) > 0
        for n, u in ((-1, 4), (4, -1), (4, 4097), (1 << 20, 2048), ((1 << 21) + 1, 1)):
            assert lib.effconf_lm_workspace_bytes(handle, n, u) == 0
            assert lib.effconf_last_error()
        assert "2^21" in lib.effconf_last_error().decode()
        assert lib.effconf_lm_workspace_bytes(None, 4, 4) == 0
        ws = C.create_string_buffer(16)
        assert lib.effconf_lm_score(handle, None, None, 1, 1, 1.0, None, None, None, ws, 16, None) != 0      # not finalized
        assert "not finalized" in lib.effconf_last_error().decode()
    finally:
        lib.effconf_lm_destroy(handle)


def test_no_cpu_fallback():
    m = LanguageModel(dict(arch="RNN", vocab_size=40, dim_model=32, num_layers=2))
    with pytest.raises(RuntimeError):
        m.score([[1, 2, 3]])
    with pytest.raises(RuntimeError):
        m.decode(torch.zeros(1, 1, dtype=torch.long), None)


def test_selection_rule_of_rescore_nbest():
    inf = float("inf")
    am = torch.tensor([[-1.0, -2.0, -3.0, -inf],       # the LM moves the winner to rank 1
                       [-1.0, -2.0, -3.0, -inf],       # the LM cannot bring back a rank without a hypothesis
                       [-1.0, -1.5, -2.0, -2.5],       # a tie of ranks 1 and 3: the lower rank
                       [-inf, -inf, -inf, -inf],       # nothing to choose from: rank 0
                       [-1.0, -2.0, -3.0, -4.0]])      # lm_weight * lm_score of -inf on rank 0
    lm = torch.tensor([[-9.0, -4.0, -8.0, 0.0],
                       [-9.0, -9.0, -9.0, 50.0],
                       [-4.0, -2.0, -4.0, 0.0],
                       [0.0, 0.0, 0.0, 0.0],
                       [-inf, -3.0, -0.5, -1.0]])
    ln = torch.tensor([[3, 2, 3, 0], [1, 1, 1, 0], [2, 2, 2, 2], [0, 0, 0, 0], [1, 2, 3, 4]], dtype=torch.int32)
    best, total = select_nbest(am, lm, ln, 0.5)
    assert best.tolist() == [1, 0, 1, 0, 2]
    assert best.dtype == torch.int64 and total.dtype == torch.float32
    want = am + 0.5 * lm
    assert torch.equal(total[:3], want[:3]) and total[2, 1] == total[2, 3] == -2.5
    # lm_weight = 0: the acoustic ranking, whatever the LM says (also -inf)
    best0, total0 = select_nbest(am, lm, ln, 0.0)
    assert best0.tolist() == [0, 0, 0, 0, 0] and torch.equal(total0, am)
    # the length bonus: fp32 am + bonus * len
    bestb, totalb = select_nbest(am, lm, ln, 0.0, length_bonus=1.25)
    assert torch.equal(totalb, am + 1.25 * ln.float()) and bestb.tolist() == [0, 0, 0, 0, 3]
    # fp32 arithmetic in the stated order
    a = torch.tensor([[-10.123456, -10.123457]])
    l = torch.tensor([[-3.3333333, -3.3333330]])
    _, t = select_nbest(a, l, torch.tensor([[1, 1]]), 0.3, length_bonus=0.1)
    assert torch.equal(t, (a + 0.3 * l) + 0.1 * torch.tensor([[1.0, 1.0]]))


def test_the_fixture_bias_makes_rescoring_move_some_winners_and_keep_others():
    """The rescoring fixture on the CPU: the float64 beam search (tests/ctc_beam_ref.py) of the Tiny CTC goldens' logits at beam 16, rescored by
    the float64 LM with TinyLM's stored fc bias at the stored lm_weight, picks the stored ranks - some are rank 0, some are not - and every
    decision is wider than 0.05 (float32 noise is 1e-6), which is what lets the GPU test assert both counts."""
    import os

    import ctc_beam_ref
    from lm_cases import GOLDEN
    g, params, sd = fixture("TinyLM")
    w = float(g["rescore_lm_weight"])
    best = []
    for tm in (100, 47):
        gold = np.load(os.path.join(GOLDEN, "tiny_T%d.npz" % tm))
        for i in range(gold["logits"].shape[0]):
            r = ctc_beam_ref.beam_search(ctc_beam_ref.logp32(gold["logits"][i]), int(gold["out_len"][i]), 16)
            y = np.zeros((len(r["prefixes"]), max(max(len(p) for p in r["prefixes"]), 1)), dtype=np.int64)
            for k, p in enumerate(r["prefixes"]):
                y[k, :len(p)] = p
            _, lms, _ = lm_ref.token_logprobs(sd, y, [len(p) for p in r["prefixes"]])
            total = np.where(np.isfinite(r["score"]), r["score"] + w * lms, -np.inf)
            order = np.argsort(-total, kind="stable")
            assert total[order[0]] - total[order[1]] > 0.05
            best.append(int(order[0]))
    assert best == g["rescore_best_rank"].tolist()
    assert sum(b != 0 for b in best) >= 2 and sum(b == 0 for b in best) >= 2
