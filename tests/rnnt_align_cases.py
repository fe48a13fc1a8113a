"""The inputs of the RNN-T lattice / alignment tests (test helper, not a test module): shared by tests/test_gpu_rnnt_align.py, which runs
them on the GPU, and tests/test_rnnt_align_host.py, which holds the oracle to the reference's golden planes on the same lattices and checks
that the seeds below leave the oracle's own near-ties within the share the GPU tests may excuse.  Everything here runs on the CPU."""
import functools
import os

import numpy as np
import torch

from efficientconformer_amd import named_config, synth
from rnnt_align_ref import lattice_planes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLANK_BIAS = 1.2
TEMPERATURES = (1.0, 2.0)


# ---------------------------------------------------------------------------------------------------------------- lattices of a model
@functools.lru_cache(maxsize=None)
def weights(name):
    """The prediction / joint network weights of the goldens: {key: numpy fp32}, and the config."""
    cfg = named_config(name)
    g = np.load(os.path.join(GOLDEN, "rnnt_%s.npz" % name))
    tsd = synth.make_transducer_state_dict(g["f"].shape[-1], cfg["decoder_params"], cfg["joint_params"], int(g["weight_seed"]), blank_bias=BLANK_BIAS)
    return tsd, cfg


@functools.lru_cache(maxsize=None)
def lattice_case(case):
    """-> (model name, f (B, T, Denc) fp32, f_len (B,), targets: list of id lists).
    "tiny":   TinyTransducer (Denc 48, H = J = 32: two 16-blocks of k; V = 40: a partial third vocabulary tile), the golden's encoder
              outputs with 13 / 10 / 7 / 2 frames and 5 / 0 / 9 / 3 tokens: no tokens at all, and more tokens than frames.
    "medium": EfficientConformerTransducerMedium (J = 640, V = 1000: 62.5 tiles), 126 / 80 frames, 17 / 30 tokens: 4748 cells, no multiple
              of the 32-cell tile; utterance 1 starts inside a tile.
    "tiny17": 17 TinyTransducer utterances: a second, partly filled group of 16 prediction-network columns."""
    name = "EfficientConformerTransducerMedium" if case == "medium" else "TinyTransducer"
    g = np.load(os.path.join(GOLDEN, "rnnt_%s.npz" % name))
    f, f_len = g["f"], g["f_len"].astype(np.int64)
    if case in ("tiny", "medium"):
        lg = np.load(os.path.join(GOLDEN, "rnnt_lattice_%s.npz" % name))
        assert lg["f_len"].tolist() == f_len.tolist()
        targets = [lg["targets"][i, :int(n)].tolist() for i, n in enumerate(lg["target_len"])]
        return name, f, f_len, targets
    rng = np.random.default_rng(1717)
    vocab = weights(name)[1]["decoder_params"]["vocab_size"]
    src = [i % f.shape[0] for i in range(17)]
    lens = np.array([max(1, int(f_len[s]) - (i // 4) % 3) for i, s in enumerate(src)], dtype=np.int64)
    targets = [rng.integers(1, vocab, int(rng.integers(0, 12))).tolist() for _ in src]
    return name, np.ascontiguousarray(f[src]), lens, targets


@functools.lru_cache(maxsize=None)
def oracle_planes(case, tmp, double=True):
    """Per utterance (lp_blank, lp_label) of the oracle's formula in float64, or - double = False - the SAME formula in float32 on the CPU."""
    name, f, f_len, targets = lattice_case(case)
    tsd = weights(name)[0]
    dtype = torch.float64 if double else torch.float32
    return [lattice_planes(tsd, f[i], int(f_len[i]), y, tmp, dtype) for i, y in enumerate(targets)]


def _dev(a, b):
    fin = np.isfinite(b)
    assert np.array_equal(fin, np.isfinite(a))
    return float(np.abs(a[fin].astype(np.float64) - b[fin]).max()) if fin.any() else 0.0


@functools.lru_cache(maxsize=None)
def float32_noise():
    """The largest deviation of the float32 CPU evaluation from float64 over every cell of the three lattice cases at both temperatures."""
    worst = 0.0
    for case in ("tiny", "medium", "tiny17"):
        for tmp in TEMPERATURES:
            for (b32, l32), (b64, l64) in zip(oracle_planes(case, tmp, False), oracle_planes(case, tmp, True)):
                worst = max(worst, _dev(b32, b64), _dev(l32, l64))
    return worst


# ---------------------------------------------------------------------------------------------------------------- planes for the dynamic programs
def random_planes(rng, t, u, scale=3.0):
    """Planes of a (t, u) lattice: per cell the log-probabilities of blank and of the label out of a random 3-way softmax (blank, label,
    everything else); lp_label is -inf in column u."""
    x = rng.standard_normal((t, u + 1, 3)) * scale
    lp = x - np.log(np.exp(x).sum(axis=-1, keepdims=True))
    lpb, lpl = lp[:, :, 0].astype(np.float32), lp[:, :, 1].astype(np.float32)
    lpl[:, u] = -np.inf
    return lpb, lpl


DP_SEEDS = {"u": 4100, "t": 4200, "ragged": 4300}
DP_U = (0, 1, 63, 64, 255, 256, 1023)      # columns = threads: one wave up to 63, two from 64, four up to 255, five from 256, sixteen at 1023
DP_T = (1, 2, 400)                         # one frame (label moves only), two, and thirteen back-pointer words per column


def dp_case(kind, n=None):
    """-> list of (lp_blank, lp_label) float32 planes, each (T, U + 1).  "u": four lattices of 3 frames and n tokens; "t": four of n frames
    and 20 tokens; "ragged": one batch that mixes the shapes of both."""
    if kind == "u":
        rng = np.random.default_rng(DP_SEEDS["u"] + n)
        return [random_planes(rng, 3, n) for _ in range(4)]
    if kind == "t":
        rng = np.random.default_rng(DP_SEEDS["t"] + n)
        return [random_planes(rng, n, 20) for _ in range(4)]
    rng = np.random.default_rng(DP_SEEDS["ragged"])
    shapes = [(3, 0), (3, 64), (1, 20), (400, 20), (3, 255), (2, 20), (57, 33), (3, 256), (1, 0), (90, 130), (3, 1), (12, 63)]
    return [random_planes(rng, t, u) for t, u in shapes]


def pad_planes(planes, tpad=None, upad=None, fill=0.0):
    """-> lp_blank, lp_label (B, T, U + 1) fp32 padded with `fill`, f_len, y_len."""
    t = max([p[0].shape[0] for p in planes] + [1]) if tpad is None else tpad
    e = max(p[0].shape[1] for p in planes) if upad is None else upad + 1
    lpb = np.full((len(planes), t, e), fill, dtype=np.float32)
    lpl = np.full((len(planes), t, e), fill, dtype=np.float32)
    for i, (b, l) in enumerate(planes):
        lpb[i, :b.shape[0], :b.shape[1]] = b
        lpl[i, :l.shape[0], :l.shape[1]] = l
    return lpb, lpl, np.array([p[0].shape[0] for p in planes], dtype=np.int64), np.array([p[0].shape[1] - 1 for p in planes], dtype=np.int64)
