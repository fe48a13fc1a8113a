"""Float64 numpy oracle of the LSTM language model (reference models/lm.py: Embedding + L-layer nn.LSTM + fc): logits of ``forward``, the
``decode`` step, per-token log-probabilities and sequence scores.  Gate order i, f, g, o; b_ih + b_hh; zero initial state; the input of a
sequence y is x = [0, y_0 .. y_{U-1}] and token_logp[u] = log_softmax(fc(h_u) / tmp)[y_u]."""
from typing import Dict, Optional, Tuple

import numpy as np


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def num_layers(sd: Dict[str, np.ndarray]) -> int:
    n = 0
    while "decoder.rnn.weight_ih_l%d" % n in sd:
        n += 1
    return n


def step(sd: Dict[str, np.ndarray], tokens, state: Optional[Tuple[np.ndarray, np.ndarray]] = None):
    """One token per sequence: tokens (N,), state (h, c) each (L, N, H) or None -> (logits (N, V) float64, (h', c'))."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    L, H = num_layers(sd), w["fc.weight"].shape[1]
    tokens = np.asarray(tokens, dtype=np.int64)
    n = tokens.shape[0]
    h, c = (np.zeros((L, n, H)), np.zeros((L, n, H))) if state is None else (np.array(state[0], dtype=np.float64), np.array(state[1], dtype=np.float64))
    x = w["decoder.embedding.weight"][tokens]
    for l in range(L):
        g = (x @ w["decoder.rnn.weight_ih_l%d" % l].T + w["decoder.rnn.bias_ih_l%d" % l]
             + h[l] @ w["decoder.rnn.weight_hh_l%d" % l].T + w["decoder.rnn.bias_hh_l%d" % l])
        i, f, gg, o = _sig(g[:, :H]), _sig(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sig(g[:, 3 * H:])
        c[l] = f * c[l] + i * gg
        h[l] = o * np.tanh(c[l])
        x = h[l]
    return x @ w["fc.weight"].T + w["fc.bias"], (h, c)


def forward_logits(sd: Dict[str, np.ndarray], y: np.ndarray, y_len=None) -> np.ndarray:
    """``LanguageModel.forward``: y (N, U) ids -> logits (N, U + 1, V) float64 of the inputs [0, y_0 .. y_{U-1}]; rows at or beyond y_len + 1 are
    fc's bias (the padded LSTM output is zero there)."""
    y = np.asarray(y, dtype=np.int64)
    n, u = y.shape
    x = np.concatenate([np.zeros((n, 1), dtype=np.int64), y], axis=1)
    out = np.zeros((n, u + 1, sd["fc.weight"].shape[0]))
    state = None
    for k in range(u + 1):
        out[:, k], state = step(sd, np.clip(x[:, k], 0, sd["fc.weight"].shape[0] - 1), state)
    if y_len is not None:
        for i, m in enumerate(np.asarray(y_len)):
            out[i, int(m) + 1:] = np.asarray(sd["fc.bias"], dtype=np.float64)
    return out


def log_softmax(z: np.ndarray) -> np.ndarray:
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def token_logprobs(sd: Dict[str, np.ndarray], y: np.ndarray, y_len=None, tmp: float = 1.0):
    """(token_logp (N, U) float64 - 0 at or beyond the length, -inf rows for status 2 -, score (N,), status (N,))."""
    y = np.asarray(y, dtype=np.int64)
    n, u = y.shape
    v = sd["fc.weight"].shape[0]
    lens = np.full(n, u, dtype=np.int64) if y_len is None else np.asarray(y_len, dtype=np.int64)
    status = np.zeros(n, dtype=np.int32)
    for i in range(n):
        if lens[i] < 0 or lens[i] > u or np.any((y[i, :max(lens[i], 0)] < 1) | (y[i, :max(lens[i], 0)] >= v)):
            status[i] = 2
    lp = log_softmax(forward_logits(sd, np.where((y >= 1) & (y < v), y, 0))[:, :u] / tmp)
    out = np.zeros((n, u))
    for i in range(n):
        if status[i]:
            out[i] = -np.inf
            continue
        for k in range(int(lens[i])):
            out[i, k] = lp[i, k, y[i, k]]
    score = np.where(status == 0, np.where(np.isfinite(out), out, 0.0).sum(axis=1), -np.inf)
    return out, score, status
