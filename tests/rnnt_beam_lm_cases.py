"""Shared by the tests of the RNN-T beam search with neural-LM fusion: the fixtures (stored encoder outputs of tests/golden/rnnt_*.npz, key-seeded
transducer and LM weights), the golden tokens of the reference's own fused search and the float64 oracle's results, each computed once."""
import functools
import os

import numpy as np
import torch

from efficientconformer_amd import named_config, synth
from lm_cases import fixture as lm_fixture
from rnnt_beam_lm_ref import beam_decode_lm
from rnnt_beam_ref import beam_decode

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = "TinyTransducer"
MEDIUM = "EfficientConformerTransducerMedium"
# The production-width case: the first half of the frames of Medium's stored encoder outputs (63 and 40 frames: the float64 oracle stays at a few seconds; blank
# bias 1.2, beam 16) with a synthetic LM of the transducer's vocabulary, 48 x 3 layers.
# Seed and weight were chosen on the CPU so that the float32 evaluation of the oracle program gives the float64 tokens on every utterance
# (tests/test_rnnt_beam_lm_host.py asserts it).
MEDIUM_LM_SEED = 21
MEDIUM_LM_WEIGHT = 0.3


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLDEN, "rnnt_beam_lm_%s.npz" % TINY))


def golden_tokens(beam):
    g = golden()
    offs = g["offsets_b%d" % beam]
    return [g["tokens_b%d" % beam][offs[i]:offs[i + 1]].tolist() for i in range(len(offs) - 1)]


@functools.lru_cache(maxsize=None)
def encoded(name):
    """(f (B, T, Denc), f_len (B,), weight seed) of tests/golden/rnnt_<name>.npz; Medium: the first half of every utterance's frames."""
    g = np.load(os.path.join(GOLDEN, "rnnt_%s.npz" % name))
    f, f_len = torch.from_numpy(g["f"]), torch.from_numpy(g["f_len"])
    if name == MEDIUM:
        f_len = f_len // 2
        f = f[:, :int(f_len.max())].contiguous()
    return f, f_len, int(g["weight_seed"])


@functools.lru_cache(maxsize=None)
def transducer_sd(name, blank_bias):
    cfg = named_config(name)
    f, _, seed = encoded(name)
    return synth.make_transducer_state_dict(f.shape[-1], cfg["decoder_params"], cfg["joint_params"], seed, blank_bias=blank_bias)


@functools.lru_cache(maxsize=None)
def tiny_lm():
    """(params, state dict) of TinyLM as the golden was made with: lm_TinyLM.npz's weight seed and fc bias (the golden stores both again)."""
    g, params, sd = lm_fixture("TinyLM")
    gb = golden()
    assert int(gb["lm_weight_seed"]) == int(g["weight_seed"]) and np.array_equal(gb["fc_bias_extra"], g["fc_bias_extra"])
    return params, sd


@functools.lru_cache(maxsize=None)
def medium_lm():
    params = dict(arch="RNN", vocab_size=named_config(MEDIUM)["decoder_params"]["vocab_size"], dim_model=48, num_layers=3)
    return params, synth.make_lm_state_dict(params, MEDIUM_LM_SEED)


@functools.lru_cache(maxsize=None)
def oracle(name, beam, blank_bias, lm_weight, tmp=1.0, lm_tmp=1.0, max_expansions=None, dtype=torch.float64):
    """The fused float64 oracle (lm_weight > 0) or the plain one (lm_weight == 0) on the stored encoder outputs."""
    f, f_len, _ = encoded(name)
    sd = transducer_sd(name, blank_bias)
    if lm_weight == 0:
        return beam_decode(sd, f, f_len, beam, tmp=tmp, max_expansions=max_expansions, dtype=dtype)
    lm_sd = (tiny_lm() if name == TINY else medium_lm())[1]
    return beam_decode_lm(sd, lm_sd, f, f_len, beam, lm_weight, tmp=tmp, lm_tmp=lm_tmp, max_expansions=max_expansions, dtype=dtype)
