"""Shared by the fused CTC beam search tests (host and GPU): the fixtures - peaked (CTC-like) logits, small synthetic LMs - and their float64 oracle
results (tests/ctc_beam_lm_ref.py), computed once per process.  Not a test module.

The logits follow tests/test_gpu_ctc_beam.py's ``_peaked`` recipe with a softer peak (the LM has to be able to move a decision); the LMs are
``synth.make_lm_state_dict`` with a seeded unigram bias (random weights alone give nearly flat rows).  Seeds were picked on the CPU with the oracle so
that every decision gap on totals is at least 1e-3 and the float32-row oracle decides as the float64 one: tests/test_ctc_beam_lm_host.py asserts both
for every case below, the GPU tests then demand the oracle's tokens at every rank."""
import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np

import ctc_beam_lm_ref as ref
from ctc_beam_ref import logp64
from efficientconformer_amd import synth


class Case(NamedTuple):
    name: str
    v: int
    beam: int
    h: int
    layers: int
    lens: Tuple[int, ...]          # frames per utterance; the batch is padded to the longest
    seed: int
    weight: float
    tmp: float = 1.0
    lm_tmp: float = 1.0
    bonus: float = 0.0
    useeds: Optional[Tuple[int, ...]] = None     # a logits seed per utterance where one seed for the batch was not found


# request columns per LM step = batch * beam: 16, 32 and 48+ pick lm_lstm_step_kernel<1>, <2> and <4>
CASES = [
    Case("v32_b4_cols16", 32, 4, 32, 1, (64, 41, 20, 33), 5, 0.6),
    Case("v257_b4_cols32", 257, 4, 48, 3, (37, 20, 64, 25, 31, 52, 22, 45), 2, 0.6),
    Case("v1000_b16_cols48", 1000, 16, 32, 1, (30, 24, 20), 10, 0.6),
    Case("v1024_b32_cols64", 1024, 32, 32, 1, (22, 20), 1, 0.6, useeds=(10, 13)),
    Case("v2_b4_short", 2, 4, 32, 1, (0, 1, 2, 20), 7, 0.6),
    Case("v32_b16_tmps", 32, 16, 48, 3, (28, 20, 35, 24), 8, 0.6, 1.3, 2.0),
    Case("v257_b1_bonus", 257, 1, 32, 1, (20, 33, 26, 21, 40, 22, 30, 25, 27, 23, 36, 24, 29, 31, 34, 28), 2, 0.6, 1.0, 1.0, 0.4),
]
BY_NAME = {c.name: c for c in CASES}
PEAK = 4.0


def peaked(seed, v, t):
    """tests/test_gpu_ctc_beam.py's recipe at a given length, peak PEAK instead of 9."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((t, v)) * 1.5).astype(np.float32)
    if t:
        spike = rng.random(t) < 0.35
        tok = rng.integers(1, v, t)
        x[np.arange(t), 0] += np.where(spike, 0.0, PEAK).astype(np.float32)
        x[np.arange(t), tok] += np.where(spike, PEAK, 0.0).astype(np.float32)
    return x


def lm_params(c: Case):
    return dict(arch="RNN", vocab_size=c.v, dim_model=c.h, num_layers=c.layers)


@functools.lru_cache(maxsize=None)
def lm_weights(name):
    c = BY_NAME[name]
    bias = (np.random.default_rng(7000 + c.seed).standard_normal(c.v) * 2.0).astype(np.float32)
    return synth.make_lm_state_dict(lm_params(c), 300 + c.seed, bias=bias)


@functools.lru_cache(maxsize=None)
def logits(name):
    """(rows: list of (t_i, V) float32, padded (B, T, V) float32 with zeros behind the lengths, lens int64)"""
    c = BY_NAME[name]
    rows = [peaked(c.useeds[i] if c.useeds else 1000 * c.seed + 17 * i + c.v, c.v, t) for i, t in enumerate(c.lens)]
    t = max(max(c.lens), 1)
    pad = np.zeros((len(rows), t, c.v), dtype=np.float32)
    for i, r in enumerate(rows):
        pad[i, :r.shape[0]] = r
    return rows, pad, np.array(c.lens, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def rows64(name):
    c = BY_NAME[name]
    return ref.LmRows({k: np.asarray(v, dtype=np.float64) for k, v in lm_weights(name).items()}, c.lm_tmp)


@functools.lru_cache(maxsize=None)
def rows32(name):
    return ref.LmRows(lm_weights(name), BY_NAME[name].lm_tmp, float32=True)


@functools.lru_cache(maxsize=None)
def oracle(name, shortcut=False, float32_rows=False, weight=None, trace=False):
    """The oracle's result for every utterance of the case (full evaluation unless `shortcut`); weight None: the case's."""
    c = BY_NAME[name]
    w = c.weight if weight is None else weight
    rows = rows32(name) if float32_rows else rows64(name)
    return [ref.beam_search(logp64(r, c.tmp) if r.shape[0] else np.zeros((0, c.v)), r.shape[0], c.beam, rows, w, c.bonus if w else 0.0,
                            shortcut=shortcut, trace=trace) for r in logits(name)[0]]
