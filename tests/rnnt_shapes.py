"""The RNN-T decoders at unequal widths and tile edges (test helper, not a test module): the case tables of tests/test_gpu_rnnt_shapes.py and
tests/test_rnnt_shapes_host.py, a native decoder of any (Denc, H, J, V) without an encoder run, the float64 references of the cases, the margin
rule that decides where token identity with float64 may be asked of float32 arithmetic, and a float32 stand-in of the decode that takes the
faults the tests must see.  Everything but ``native_decoder`` runs on the CPU.

A case is (Denc, H, J, V): encoder width, prediction-network width (dim_decoder), joint width, vocabulary.  The weights are
synth.make_transducer_state_dict's, the encoder outputs seeded standard-normal (B, T, Denc).

The margin rule.  The float64 reference takes every decision as argmax of its logits.  The case's logit noise is max |float32 - float64| over
every logit of every decision of the reference, the float32 evaluation following the reference's tokens (so both see the same history).  An
utterance must give the reference's tokens when the smallest top-2 margin of its decisions is at least MARGIN_FACTOR x that noise; decisions
forced by max_consec_dec_step have no margin.  Otherwise the utterance is excused, and must still agree on the tokens emitted before its first
under-margin decision.  At most 1 utterance in 8 of a case may be excused (tests/test_rnnt_shapes_host.py keeps the reference alone inside
that cap for the seeds and biases below)."""
import copy
import functools
from typing import NamedTuple

import numpy as np
import torch

from efficientconformer_amd import named_config, synth
from oracle.ref_transducer import greedy_decode, joint_logits, lstm_step
from rnnt_align_ref import lattice_planes
from rnnt_beam_ref import beam_decode

SEED = 11
MAX_CONSEC = 5
MARGIN_FACTOR = 32
TEMPERATURES = (1.0, 2.0)

# ---- greedy: batch 20 (the last cluster partly filled under 8 and under 16 utterances per cluster), 12 frames, ragged lengths with 0 and 1
GREEDY_BATCH, GREEDY_T = 20, 12
GREEDY_CASES = {
    (20, 36, 44, 37): 1.2,        # per-utterance only (not % 16): matvec unroll remainder, sgemm K % 16 != 0, N % 64 != 0
    (48, 64, 128, 41): 1.2,       # 8 x 8 x 2: HU = 8, two gate tiles across two gates each, six idle waves, VU = 6, workgroup 7 empty; 16 x 16 x 1: HU = 4, workgroups 14, 15 empty
    (24, 832, 64, 1017): 1.2,     # 8 x 8 x 2: 26 gate tiles (4 and 3 per wave), VU = 128 with the last slice cut at V; 16 x 16 x 1: 13 tiles (2 and 1); H > J
    (40, 128, 320, 1000): 1.2,    # JU = 40 (a partial linear_decoder tile), 20 16-blocks of k on the joint; H < J
    (200, 320, 320, 1000): 1.2,   # the shipped Small decoder
    (12, 20, 28, 9): 1.2,         # per-utterance only: the linear_encoder GEMM with K = 12 < 16 (one clamped, masked k-step)
}
# what effconf_rnnt_greedy_route allows per case: (8 x 8 x 2, 16 x 16 x 1)
GREEDY_CLUSTERS = {(20, 36, 44, 37): (False, False), (12, 20, 28, 9): (False, False), (48, 64, 128, 41): (True, True), (24, 832, 64, 1017): (True, True),
                   (40, 128, 320, 1000): (True, True), (200, 320, 320, 1000): (True, True)}

# ---- beam search: 6 utterances, 8 frames
BEAM_BATCH, BEAM_T = 6, 8
BEAMS = (1, 4, 16)
BEAM_CASES = {
    (20, 16, 48, 17): 1.2,        # one and three 16-blocks of k: one block of loads in flight
    (40, 128, 320, 1000): 1.2,    # 8 blocks in flight on linear_decoder, 4 on the joint; J > H
    (24, 320, 64, 33): 1.2,       # the reverse; H > J
}

# ---- lattice planes: 17 utterances (a second, partly filled group of 16 prediction-network columns), 12 frames
LATTICE_BATCH, LATTICE_T = 17, 12
LATTICE_CASES = [(20, 16, 48, 5), (36, 48, 16, 16), (36, 48, 16, 17), (48, 80, 112, 273), (24, 784, 64, 33), (200, 320, 320, 1000)]


def _sd(dims, blank_bias):
    de, h, j, v = dims
    return synth.make_transducer_state_dict(de, {"dim_model": h, "vocab_size": v, "num_layers": 1}, {"dim_model": j, "joint_mode": "sum", "act": "tanh"},
                                            SEED, blank_bias=blank_bias)


@functools.lru_cache(maxsize=None)
def weights(dims, blank_bias=1.2):
    """{key: numpy fp32} of the prediction and joint networks of a case."""
    return _sd(dims, blank_bias)


def _as(sd, dtype):
    return {k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def frames(de, batch, t, seed=SEED):
    """Encoder outputs (batch, t, de) fp32, standard normal."""
    return np.random.default_rng(seed).standard_normal((batch, t, de)).astype(np.float32)


def ragged(batch, t, seed=SEED):
    """Lengths in 2 .. t, the first and the last utterance full, utterance 1 without frames, utterance 2 with one."""
    lens = np.random.default_rng(seed + 1).integers(2, t + 1, batch).astype(np.int64)
    lens[0] = lens[-1] = t
    lens[1], lens[2] = 0, 1
    return lens


@functools.lru_cache(maxsize=None)
def native_decoder(dims, blank_bias=1.2):
    """A Transducer whose prediction / joint networks have the widths of the case, on the GPU; its encoder (TinyTransducer's) never runs."""
    from efficientconformer_amd import Transducer
    from efficientconformer_amd.transducer import JointNetwork
    de, h, j, v = dims
    cfg = copy.deepcopy(named_config("TinyTransducer"))
    cfg["decoder_params"].update(dim_model=h, vocab_size=v, max_consec_dec_step=MAX_CONSEC)
    cfg["joint_params"].update(dim_model=j)
    m = Transducer.from_config(cfg)
    m.joint_network = JointNetwork(de, h, v, cfg["joint_params"])
    m._cfg = (de, h, j, v, 1)
    missing = m.load_state_dict({k: torch.from_numpy(t) for k, t in weights(dims, blank_bias).items()}, strict=False)
    assert not missing.unexpected_keys and all(k.startswith("encoder.") for k in missing.missing_keys)
    return m.cuda()


# ---------------------------------------------------------------------------------------------------------------- greedy: reference and margin rule
class GreedyTrace(NamedTuple):
    tokens: list        # per utterance: the float64 reference's tokens
    decisions: list     # per utterance: [(top-2 margin in float64, None when forced by max_consec; tokens emitted before the decision)]
    noise: float        # max |float32 - float64| over every logit of every decision
    smallest: float     # the smallest margin of the case


def greedy_inputs(dims):
    return frames(dims[0], GREEDY_BATCH, GREEDY_T), ragged(GREEDY_BATCH, GREEDY_T)


@functools.lru_cache(maxsize=None)
def greedy_trace(dims, blank_bias=None):
    bias = GREEDY_CASES[dims] if blank_bias is None else blank_bias
    f, lens = greedy_inputs(dims)
    sd = weights(dims, bias)
    s64, s32 = _as(sd, torch.float64), _as(sd, torch.float32)
    f32 = torch.from_numpy(f)
    f64 = f32.double()
    h = dims[1]
    tokens, decisions, noise, smallest = [], [], 0.0, float("inf")
    with torch.no_grad():
        for b in range(f.shape[0]):
            y, dec = [0], []
            h64, c64, h32, c32 = torch.zeros(h, dtype=torch.float64), torch.zeros(h, dtype=torch.float64), torch.zeros(h), torch.zeros(h)
            step, consec, n = 0, 0, int(lens[b])
            while step < n:
                h64, c64 = lstm_step(s64, y[-1], h64, c64)
                h32, c32 = lstm_step(s32, y[-1], h32, c32)
                while step < n:
                    l64, l32 = joint_logits(s64, f64[b, step], h64), joint_logits(s32, f32[b, step], h32)
                    noise = max(noise, float((l32.double() - l64).abs().max()))
                    pred = int(l64.argmax())
                    forced = consec == MAX_CONSEC
                    top = l64.topk(2).values
                    margin = None if forced else float(top[0] - top[1])
                    dec.append((margin, len(y) - 1))
                    if margin is not None:
                        smallest = min(smallest, margin)
                    if pred == 0 or forced:
                        consec = 0
                        step += 1
                    else:
                        consec += 1
                        y.append(pred)
                        break
            tokens.append(y[1:])
            decisions.append(dec)
    return GreedyTrace(tokens, decisions, noise, smallest)


def first_under_margin(trace, b):
    """None when utterance b must give the reference's tokens, else the number of tokens it must still share with them."""
    bound = MARGIN_FACTOR * trace.noise
    for margin, ntok in trace.decisions[b]:
        if margin is not None and margin < bound:
            return ntok
    return None


def check_greedy(trace, got, what=""):
    """The margin rule on the token lists `got` -> the excused utterances.  Raises AssertionError where it is broken."""
    assert len(got) == len(trace.tokens), what
    excused = []
    for b, ref in enumerate(trace.tokens):
        k = first_under_margin(trace, b)
        if k is None:
            assert list(got[b]) == ref, (what, b, list(got[b]), ref)
        else:
            excused.append(b)
            assert list(got[b][:k]) == ref[:k], (what, b, k, list(got[b]), ref)
    assert 8 * len(excused) <= len(trace.tokens), (what, excused)
    return excused


FAULTS = ("gd_pitch", "whh_last_block", "vocab_tail", "vocab_slice")


def standin_greedy(dims, fault=None, blank_bias=None):
    """The greedy decode in torch float32 the way the cluster kernels lay it out - linear_decoder(h) of utterance b in slot b % 8 of a [8][J] buffer, the
    vocabulary in 8 slices - with one fault:
      gd_pitch        the slot is read at pitch H instead of J
      whh_last_block  the last 16-block of k is dropped from W_hh
      vocab_tail      the vocabulary entries of the tail tile (n >= 16 floor(V / 16)) are masked
      vocab_slice     the argmax candidates of slice 1 of 8 are dropped"""
    assert fault is None or fault in FAULTS
    de, h, j, v = dims
    f, lens = greedy_inputs(dims)
    sd = _as(weights(dims, GREEDY_CASES[dims] if blank_bias is None else blank_bias), torch.float32)
    if fault == "whh_last_block":
        sd["decoder.rnn.weight_hh_l0"][:, h - 16:] = 0
    wd, bd = sd["joint_network.linear_decoder.weight"], sd["joint_network.linear_decoder.bias"]
    we, be = sd["joint_network.linear_encoder.weight"], sd["joint_network.linear_encoder.bias"]
    wj, bj = sd["joint_network.linear_joint.weight"], sd["joint_network.linear_joint.bias"]
    pitch = h if fault == "gd_pitch" else j
    buf = torch.zeros(8 * max(h, j) + j)
    vu = (v + 7) // 8
    out = []
    f = torch.from_numpy(f)
    with torch.no_grad():
        for b in range(f.shape[0]):
            y, slot = [0], b % 8
            hh, cc = torch.zeros(h), torch.zeros(h)
            step, consec, n = 0, 0, int(lens[b])
            while step < n:
                hh, cc = lstm_step(sd, y[-1], hh, cc)
                buf[slot * j:slot * j + j] = wd @ hh + bd
                while step < n:
                    logits = wj @ torch.tanh(we @ f[b, step] + be + buf[slot * pitch:slot * pitch + j]) + bj
                    if fault == "vocab_tail":
                        logits[16 * (v // 16):] = -np.inf
                    if fault == "vocab_slice":
                        logits[vu:2 * vu] = -np.inf
                    pred = int(logits.argmax())
                    if pred == 0 or consec == MAX_CONSEC:
                        consec = 0
                        step += 1
                    else:
                        consec += 1
                        y.append(pred)
                        break
            out.append(y[1:])
    return out


def greedy_float32(dims, blank_bias=None):
    """The oracle's own program in float32 (free running)."""
    f, lens = greedy_inputs(dims)
    return greedy_decode(_as(weights(dims, GREEDY_CASES[dims] if blank_bias is None else blank_bias), torch.float32), torch.from_numpy(f), lens, MAX_CONSEC)


# ---------------------------------------------------------------------------------------------------------------- beam search
def beam_inputs(dims):
    return frames(dims[0], BEAM_BATCH, BEAM_T, SEED + 2), ragged(BEAM_BATCH, BEAM_T, SEED + 2)


@functools.lru_cache(maxsize=None)
def beam_oracle(dims, beam, double=True):
    """rnnt_beam_ref.beam_decode of the case under the kernel's default cap of 16 x beam expansions per frame."""
    f, lens = beam_inputs(dims)
    return beam_decode(weights(dims, BEAM_CASES[dims]), torch.from_numpy(f), lens, beam, max_expansions=16 * beam,
                       dtype=torch.float64 if double else torch.float32)


# ---------------------------------------------------------------------------------------------------------------- lattice planes
@functools.lru_cache(maxsize=None)
def lattice_inputs(dims):
    """-> f, f_len (lengths 1 .. 12), targets: utterance 1 has no tokens, utterance 2 one frame and four tokens, utterance 3 more tokens (14) than frames."""
    v = dims[3]
    rng = np.random.default_rng(SEED + 3)
    lens = ragged(LATTICE_BATCH, LATTICE_T, SEED + 3)
    lens[1] = 5
    lens[3] = 9
    targets = [rng.integers(1, v, int(rng.integers(0, 12))).tolist() for _ in range(LATTICE_BATCH)]
    targets[1] = []
    targets[2] = rng.integers(1, v, 4).tolist()
    targets[3] = rng.integers(1, v, 14).tolist()
    return frames(dims[0], LATTICE_BATCH, LATTICE_T, SEED + 3), lens, targets


@functools.lru_cache(maxsize=None)
def lattice_oracle(dims, tmp, double=True):
    f, lens, targets = lattice_inputs(dims)
    dtype = torch.float64 if double else torch.float32
    return [lattice_planes(weights(dims), f[i], int(lens[i]), y, tmp, dtype) for i, y in enumerate(targets)]


def _dev(a, b):
    fin = np.isfinite(b)
    assert np.array_equal(fin, np.isfinite(a))
    return float(np.abs(a[fin].astype(np.float64) - b[fin]).max()) if fin.any() else 0.0


@functools.lru_cache(maxsize=None)
def lattice_noise(dims):
    """The case's own float32 noise: the largest deviation of the reference's float32 evaluation from float64 over every cell at both temperatures."""
    worst = 0.0
    for tmp in TEMPERATURES:
        for (b32, l32), (b64, l64) in zip(lattice_oracle(dims, tmp, False), lattice_oracle(dims, tmp, True)):
            worst = max(worst, _dev(b32, b64), _dev(l32, l64))
    return worst


