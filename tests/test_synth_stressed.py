"""CPU: the stressed parameter generator (synth.make_stressed_state_dict) - deterministic, leaves make_state_dict alone, and puts its values
exactly where its profiles say relative to the fused split images' limit (|w| < 65000 / 1024 after folding, csrc/pack.h kSplitImgMax)."""
import zlib

import numpy as np
import pytest

from efficientconformer_amd import ModelCTC, named_config, synth

LIMIT = 65000.0 / 1024.0


def _plan(name):
    return ModelCTC.from_config(named_config(name)).encoder.plan


def _over(plan, sd):
    return {k: float(np.abs(v).max()) for k, v in synth.split_image_values(plan, sd).items() if np.abs(v).max() >= LIMIT}


# crc32 over (key, float32 bytes) of make_state_dict(Tiny, seed 7, vocab 65), keys sorted: the value the committed goldens were made with
TINY_SEED7_DIGEST = 0xD6E80261


def test_make_state_dict_is_unchanged():
    """The goldens and the benchmark depend on make_state_dict byte for byte: a digest of Tiny's seed-7 weights against a committed constant."""
    sd = synth.make_state_dict(_plan("Tiny"), 7, 65)
    h = 0
    for k in sorted(sd):
        h = zlib.crc32(np.ascontiguousarray(sd[k]).tobytes(), zlib.crc32(k.encode(), h))
    assert h == TINY_SEED7_DIGEST, hex(h)


@pytest.mark.parametrize("profile", synth.STRESS_PROFILES)
def test_stressed_generator_is_deterministic(profile):
    plan = _plan("Tiny")
    a = synth.make_stressed_state_dict(plan, 7, profile, 65, prefix="encoder.")
    b = synth.make_stressed_state_dict(plan, 7, profile, 65, prefix="encoder.")
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert "fc.weight" in a and "encoder.linear.weight" in a
    c = synth.make_stressed_state_dict(plan, 8, profile, 65, prefix="encoder.")
    assert not np.array_equal(a["encoder.linear.weight"], c["encoder.linear.weight"])


@pytest.mark.parametrize("name", ["Tiny", "EfficientConformerCTCSmall", "EfficientConformerCTCMedium", "ConformerCTCSmall"])
def test_boundary_crosses_exactly_the_intended_limits(name):
    """Folded in numpy as pack.hip folds them (bn_fold, gamma W, b1 + W beta): the subsampler tap x BN scale and BN shift (one-layer subsampler),
    block 0's gamma W1 / bias column (FFN1) and pointwise-1 at ~100; nothing else at or beyond the limit; the below-limit values present in the last
    block (FFN2 bias column and pointwise-1 at 60, gamma W1 at 40)."""
    plan = _plan(name)
    sd = synth.make_stressed_state_dict(plan, 7, "boundary")
    over = _over(plan, sd)
    want = {"blocks.0.ffn1.w1", "blocks.0.ffn1.bias", "blocks.0.pw1.w"} | ({"sub.taps", "sub.shift"} if plan.sub_layers == 1 else set())
    assert set(over) == want, over
    assert all(abs(v - 100.0) < 1e-3 for v in over.values()), over
    vals = synth.split_image_values(plan, sd)
    last = "blocks.%d" % plan.blocks[-1].index
    for key, v in ((".ffn2.bias", 60.0), (".pw1.w", 60.0), (".ffn2.w1", 40.0)):
        assert abs(float(np.abs(vals[last + key]).max()) - v) < 1e-3, key
    assert not _over(plan, synth.make_state_dict(plan, 7))


@pytest.mark.parametrize("name", ["Tiny", "EfficientConformerCTCSmall", "EfficientConformerCTCMedium", "ConformerCTCSmall"])
def test_trained_stays_inside_the_weight_side_envelopes(name):
    """Every folded value of every fused image below the limit (with margin), and the profile's statistics where its docstring puts them:
    LN gains in [0.05, 5], calibrated BatchNorm (running stats differ from the synthetic ones, near-dead channels with small running_var)."""
    plan = _plan(name)
    sd = synth.make_stressed_state_dict(plan, 7, "trained")
    vals = synth.split_image_values(plan, sd)
    worst = max(float(np.abs(v).max()) for v in vals.values())
    assert worst < 0.5 * LIMIT, worst
    g = sd["blocks.0.feed_forward_module1.layers.0.weight"]
    assert g.min() >= 0.05 and g.max() <= 5.0 and g.max() > 1.5
    rv = sd["blocks.0.convolution_module.layers.5.running_var"]
    assert rv.min() < 1e-2 * np.median(rv)                     # near-dead channels
    sv = sd["subsampling_module.layers.0.1.running_mean"]
    assert float(np.abs(sv).mean()) > 1.0                      # the mel mean absorbed by the calibrated subsampler statistics
    assert abs(float(sd["linear.bias"].mean())) > 100.0        # common offset on the residual stream


def test_silence_floor_mel():
    mel, lens = synth.silence_floor_mel(3, 80, 200, [200, 150, 60], seed=3)
    base, _ = synth.make_mel(3, 80, 200, [200, 150, 60], seed=3)
    floor = np.float32(np.log(1e-9))
    for b, n in enumerate(lens):
        cols = np.all(mel[b, :, :n] == floor, axis=0)
        assert cols.sum() >= 5
        loud = mel[b, :, :n].min(axis=0) > 6.0                   # 12 + N(0, 1) in every bin
        assert loud.any()
        changed = np.any(mel[b] != base[b], axis=0)
        assert np.all(cols[changed[:n]] | loud[changed[:n]]) and not changed[n:].any()   # only whole frames, only floor / loud ones
