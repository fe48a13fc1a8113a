"""Float64 oracle of the RNN-T lattice, its forward recursion and its Viterbi alignment (test helper, not a test module).

Lattice of T frames and a transcript y of U tokens (blank 0): cell (t, u), t < T, u <= U, holds
    lp_blank[t, u] = log_softmax(logits(t, u) / tmp)[0]        the move to (t + 1, u)
    lp_label[t, u] = log_softmax(logits(t, u) / tmp)[y[u]]     the move to (t, u + 1); -inf at u = U
    logits(t, u)   = linear_joint(tanh(linear_encoder(f[t]) + linear_decoder(g_u))),  g_u = the LSTM's output after [0, y_1 .. y_u]
(reference models/transducer.py:88-107, decoders.py:52-67, joint_networks.py:80-104).  A path starts in (0, 0), takes T blank moves and U
label moves and leaves the lattice by the blank of (T - 1, U).  ``forward`` sums the paths, ``viterbi`` takes the best one; at equal values
the blank (time) move wins: the label move is taken only when strictly greater.  A path is written as token_frame[u] = the frame at which
token u is emitted (non-decreasing).
"""
from __future__ import annotations

import itertools
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

NEG = -np.inf


def _w(sd, key, dtype):
    v = sd[key]
    v = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))
    return v.to(dtype)


def prediction_outputs(sd: Dict, y: Sequence[int], dtype=torch.float64) -> torch.Tensor:
    """(U + 1, H): the prediction network's output after [0], [0, y_1], .. (Embedding -> 1-layer LSTM, torch gate order i, f, g, o)."""
    emb, wih, whh = _w(sd, "decoder.embedding.weight", dtype), _w(sd, "decoder.rnn.weight_ih_l0", dtype), _w(sd, "decoder.rnn.weight_hh_l0", dtype)
    bias = _w(sd, "decoder.rnn.bias_ih_l0", dtype) + _w(sd, "decoder.rnn.bias_hh_l0", dtype)
    hd = whh.shape[1]
    h, c = torch.zeros(hd, dtype=dtype), torch.zeros(hd, dtype=dtype)
    out = []
    for tok in [0] + [int(v) for v in y]:
        g = wih @ emb[tok] + whh @ h + bias
        i, f, gg, o = torch.sigmoid(g[:hd]), torch.sigmoid(g[hd:2 * hd]), torch.tanh(g[2 * hd:3 * hd]), torch.sigmoid(g[3 * hd:])
        c = f * c + i * gg
        h = o * torch.tanh(c)
        out.append(h)
    return torch.stack(out)


def lattice_planes(sd: Dict, f, length: Optional[int], y: Sequence[int], tmp: float = 1.0, dtype=torch.float64):
    """-> (lp_blank, lp_label), numpy (T, U + 1) of `dtype`, for one utterance: f (frames, Denc), the first `length` frames, transcript y."""
    f = f if isinstance(f, torch.Tensor) else torch.from_numpy(np.asarray(f))
    n = f.shape[0] if length is None else max(0, min(int(length), f.shape[0]))
    y = [int(v) for v in y]
    u = len(y)
    with torch.no_grad():
        g = prediction_outputs(sd, y, dtype)
        fe = f[:n].to(dtype) @ _w(sd, "joint_network.linear_encoder.weight", dtype).T + _w(sd, "joint_network.linear_encoder.bias", dtype)
        gd = g @ _w(sd, "joint_network.linear_decoder.weight", dtype).T + _w(sd, "joint_network.linear_decoder.bias", dtype)
        z = torch.tanh(fe[:, None, :] + gd[None, :, :])
        logits = z @ _w(sd, "joint_network.linear_joint.weight", dtype).T + _w(sd, "joint_network.linear_joint.bias", dtype)
        lp = torch.log_softmax(logits / tmp, dim=-1)
        lpb = lp[:, :, 0].clone()
        lpl = torch.full((n, u + 1), NEG, dtype=dtype)
        if u:
            idx = torch.tensor(y, dtype=torch.int64)[None, :, None].expand(n, u, 1)
            lpl[:, :u] = lp[:, :u].gather(2, idx)[:, :, 0]
    return lpb.numpy(), lpl.numpy()


def status_of(length: int, y: Sequence[int], vocab: int, u_max: Optional[int] = None) -> int:
    """0 ok, 2 a token outside 1 .. vocab - 1 (or more tokens than u_max), 1 tokens but no frames."""
    y = [int(c) for c in y]
    if any(c < 1 or c >= vocab for c in y) or (u_max is not None and len(y) > u_max):
        return 2
    return 1 if length <= 0 and y else 0


def _dims(lpb, length, u):
    lpb = np.asarray(lpb, dtype=np.float64)
    n = lpb.shape[0] if length is None else max(0, min(int(length), lpb.shape[0]))
    u = lpb.shape[1] - 1 if u is None else int(u)
    return n, u


def forward(lpb, lpl, length: Optional[int] = None, u: Optional[int] = None) -> float:
    """log P(y | x) of the planes' first `length` frames and first u + 1 columns, float64 (0 for the empty lattice without tokens, -inf for
    tokens without frames)."""
    n, u = _dims(lpb, length, u)
    if n == 0:
        return 0.0 if u == 0 else NEG
    lpb, lpl = np.asarray(lpb, dtype=np.float64), np.asarray(lpl, dtype=np.float64)
    a = np.full(u + 1, NEG)                           # row t of alpha
    for t in range(n):
        for k in range(u + 1):
            if t == 0 and k == 0:
                a[k] = 0.0
                continue
            p = a[k] + lpb[t - 1, k] if t > 0 else NEG              # a still holds row t - 1 at k
            q = a[k - 1] + lpl[t, k - 1] if k > 0 else NEG          # and row t at k - 1
            a[k] = np.logaddexp(p, q)
    return float(a[u] + lpb[n - 1, u])


def viterbi(lpb, lpl, length: Optional[int] = None, u: Optional[int] = None) -> Dict:
    """-> score (float64, every blank included), token_frame (u,) the frame token k is emitted at, margin: the smallest difference between the
    chosen and the other finite predecessor along the path (inf: nothing to decide)."""
    n, u = _dims(lpb, length, u)
    if n == 0:
        return {"score": 0.0 if u == 0 else NEG, "token_frame": np.full(u, -1, dtype=np.int64), "margin": np.inf}
    lpb, lpl = np.asarray(lpb, dtype=np.float64), np.asarray(lpl, dtype=np.float64)
    v = np.full((n, u + 1), NEG)
    lab = np.zeros((n, u + 1), dtype=bool)
    gap = np.full((n, u + 1), np.inf)
    for t in range(n):
        for k in range(u + 1):
            if t == 0 and k == 0:
                v[t, k] = 0.0
                continue
            p = v[t - 1, k] + lpb[t - 1, k] if t > 0 else NEG
            q = v[t, k - 1] + lpl[t, k - 1] if k > 0 else NEG
            lab[t, k] = q > p                                       # strict: equality takes the blank (time) move
            v[t, k] = q if lab[t, k] else p
            if np.isfinite(p) and np.isfinite(q):
                gap[t, k] = abs(p - q)
    frames = np.zeros(u, dtype=np.int64)
    t, k, margin = n - 1, u, np.inf
    while t > 0 or k > 0:
        margin = min(margin, float(gap[t, k]))
        if lab[t, k]:
            k -= 1
            frames[k] = t
        else:
            t -= 1
    return {"score": float(v[n - 1, u] + lpb[n - 1, u]), "token_frame": frames, "margin": float(margin)}


def check_path(token_frame, length: int, u: int) -> Optional[str]:
    """None when token_frame is a path of the (length, u) lattice, else what is wrong with it."""
    fr = [int(c) for c in token_frame]
    if len(fr) != u:
        return "%d frames for %d tokens" % (len(fr), u)
    if u and length <= 0:
        return "no frames"
    for k, c in enumerate(fr):
        if c < 0 or c >= length:
            return "token %d: frame %d of %d" % (k, c, length)
        if k and c < fr[k - 1]:
            return "token %d: frame %d after frame %d" % (k, c, fr[k - 1])
    return None


def path_logp(lpb, lpl, token_frame, length: int) -> float:
    """The float64 log-probability of the path token_frame: its label moves and the blank of every frame (taken in the column reached there)."""
    lpb, lpl = np.asarray(lpb, dtype=np.float64), np.asarray(lpl, dtype=np.float64)
    fr = [int(c) for c in token_frame]
    total = sum(lpl[c, k] for k, c in enumerate(fr))
    k = 0
    for t in range(length):
        while k < len(fr) and fr[k] <= t:
            k += 1
        total += lpb[t, k]
    return float(total)


def all_paths(length: int, u: int) -> List[List[int]]:
    """Every monotone path of the (length, u) lattice as token_frame lists (brute force: small lattices only)."""
    return [list(c) for c in itertools.combinations_with_replacement(range(length), u)]


def brute_force(lpb, lpl, length: int, u: int) -> Dict:
    """log-sum and maximum over all_paths: log_likelihood, score, and the paths within 1e-12 of the best."""
    if length == 0:
        return {"log_likelihood": 0.0 if u == 0 else NEG, "score": 0.0 if u == 0 else NEG, "best": [[-1] * u]}
    paths = all_paths(length, u)
    vals = np.array([path_logp(lpb, lpl, p, length) for p in paths])
    m = vals.max()
    return {"log_likelihood": float(m + np.log(np.exp(vals - m).sum())), "score": float(m),
            "best": [p for p, v in zip(paths, vals) if v >= m - 1e-12]}
