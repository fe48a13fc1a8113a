"""Shared by the language-model tests: the fixtures of tests/golden/lm_*.npz with their synthetic weights, torch's own LSTM LM on these weights
(float64: a second oracle; float32: the reference arithmetic whose distance to float64 is the noise the GPU results are held to), and that
noise for a set of sequences."""
import os

import numpy as np
import torch

from efficientconformer_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture(name):
    g = np.load(os.path.join(GOLDEN, "lm_%s.npz" % name))
    params = dict(arch="RNN", vocab_size=int(g["vocab_size"]), dim_model=int(g["dim_model"]), num_layers=int(g["num_layers"]))
    sd = synth.make_lm_state_dict(params, int(g["weight_seed"]), bias=g["fc_bias_extra"] if "fc_bias_extra" in g.files else None)
    return g, params, sd


def torch_lm(params, sd, dtype):
    """torch's own Embedding + nn.LSTM + Linear with these weights -> f(tokens (N, U + 1), state) = (logits, (h, c))."""
    emb = torch.nn.Embedding(params["vocab_size"], params["dim_model"])
    rnn = torch.nn.LSTM(params["dim_model"], params["dim_model"], params["num_layers"], batch_first=True)
    fc = torch.nn.Linear(params["dim_model"], params["vocab_size"])
    t = {k: torch.from_numpy(v) for k, v in sd.items()}
    emb.load_state_dict({"weight": t["decoder.embedding.weight"]})
    rnn.load_state_dict({k[len("decoder.rnn."):]: v for k, v in t.items() if k.startswith("decoder.rnn.")})
    fc.load_state_dict({"weight": t["fc.weight"], "bias": t["fc.bias"]})
    emb, rnn, fc = emb.to(dtype).eval(), rnn.to(dtype).eval(), fc.to(dtype).eval()

    def run(x, state=None):
        with torch.no_grad():
            y, state = rnn(emb(torch.as_tensor(x).long()), state)
            return fc(y), state
    return run


def float32_logprobs(params, sd, y, tmp):
    """log_softmax(logits / tmp) gathered at y, (N, U), by torch in float32: nn.LSTM + Linear + log_softmax on the CPU."""
    y = np.asarray(y, dtype=np.int64)
    x = np.concatenate([np.zeros((y.shape[0], 1), dtype=np.int64), y], axis=1)[:, :max(y.shape[1], 1)]
    lp = torch.log_softmax(torch_lm(params, sd, torch.float32)(x)[0] / tmp, dim=-1)
    return lp.gather(2, torch.from_numpy(y[:, :, None]))[:, :, 0].double().numpy() if y.shape[1] else np.zeros(y.shape)


def float32_noise(params, sd, y, lens, tmp, want):
    """The largest |float32 - float64| per-token log-probability over the valid positions of a case; `want` = lm_ref.token_logprobs(...)[0]."""
    got = float32_logprobs(params, sd, y, tmp)
    valid = np.arange(y.shape[1])[None, :] < np.asarray(lens)[:, None]
    return float(np.abs(got - want)[valid].max(initial=0.0))
