"""Self-conditioned CTC encoders on the CPU: the plan, the state-dict surface, the composed oracle against the reference's goldens, the packing dry run and the
routes of an InterCTC handle, and the teeth of the stage checker the GPU tests (tests/test_gpu_interctc.py) hold csrc/interctc.hip to."""
import ctypes as C
import hashlib
import importlib.util
import os
import zlib

import numpy as np
import pytest
import torch

import interctc_ref as IR
from efficientconformer_amd import ConformerEncoder, ConformerEncoderInterCTC, InterCTC, ModelCTC, _lib, model_from_config, named_config, synth
from efficientconformer_amd import params as P
from efficientconformer_amd.config import _NAMED, build_plan
from oracle import ref_bf16 as RB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("pack_digest", os.path.join(ROOT, "tools", "pack_digest.py"))
pack_digest = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pack_digest)

# (number of specs, sha256[:16] of "key shape kind" lines) of param_specs, and the crc of make_state_dict(plan, 7, 32), of the named configurations - computed
# on the commit before the InterCTC encoders existed: the goldens and the bench depend on these staying what they were
SPEC_PINS = {'ConformerCTCLarge': (754, '79bc9b637e48254a'), 'ConformerCTCMedium': (754, '3e1e9cd693c3c0ac'), 'ConformerCTCSmall': (672, '864ee6dbc6d0fb35'),
             'ConformerTransducerLarge': (713, '7fb85386d32cfada'), 'ConformerTransducerMedium': (672, '07926d9dde34ecb0'),
             'ConformerTransducerSmall': (672, '879083ea2fd184ba'), 'EfficientConformerCTCLarge': (669, '6d90c3b15f25e206'),
             'EfficientConformerCTCMedium': (669, 'f81ebc18fee33458'), 'EfficientConformerCTCSmall': (628, '3c44ef3cd62afe60'),
             'EfficientConformerTransducerLarge': (628, '21894b99d95210ec'), 'EfficientConformerTransducerMedium': (628, 'd01655e197df6188'),
             'EfficientConformerTransducerSmall': (628, 'b83df3943bc3519a'), 'SmallAligned': (628, 'd6620f1c723d213f'), 'Tiny': (259, 'b689807c83b139f9'),
             'TinyTransducer': (259, 'b689807c83b139f9')}
SD_PINS = {'Tiny': 1915953845, 'EfficientConformerCTCSmall': 3676334158}


def _spec_hash(specs):
    return len(specs), hashlib.sha256("\n".join("%s %s %s" % (k, tuple(s), kind) for k, s, kind in specs).encode()).hexdigest()[:16]


# ------------------------------------------------------------------ plan, keys, Python surface
def test_plan_validation():
    base = IR.tiny_params()
    plan = build_plan(base, interctc=True)
    assert plan.interctc_blocks == [1, 3, 5] and plan.interctc_vocab == 32
    assert build_plan(dict(base, interctc_blocks=[5, 1]), interctc=True).interctc_blocks == [1, 5]
    plain = build_plan(base)                                   # the plain encoder ignores both keys, as the reference's does
    assert plain.interctc_blocks == [] and plain.interctc_vocab == 0
    for bad, word in ((dict(base, interctc_blocks=[1, 6]), "outside"), (dict(base, interctc_blocks=[-1]), "outside"), (dict(base, interctc_blocks=[1, 1]), "twice"),
                      (dict(base, interctc_blocks=[1.0]), "ints"), (dict(base, interctc_blocks=[True]), "ints"), (dict(base, vocab_size=1), ">= 2"),
                      (dict(base, vocab_size="32"), ">= 2")):
        with pytest.raises(Exception) as err:
            build_plan(bad, interctc=True)
        assert word in str(err.value), (bad["interctc_blocks"], bad["vocab_size"], err.value)
    for missing in ("interctc_blocks", "vocab_size"):
        with pytest.raises(Exception) as err:
            build_plan({k: v for k, v in base.items() if k != missing}, interctc=True)
        assert missing in str(err.value)


@pytest.mark.parametrize("name", sorted(SPEC_PINS))
def test_param_specs_without_interctc_are_unchanged(name):
    enc = named_config(name)["encoder_params"]
    specs = P.param_specs(build_plan(enc))
    assert _spec_hash(specs) == SPEC_PINS[name]
    assert not any(k.startswith(("linear_expand_", "linear_proj_")) for k, _, _ in specs)
    # ... also with the keys present (the plain class ignores them), and as the head of the InterCTC plan's list
    with_keys = dict(enc, interctc_blocks=[0], vocab_size=40)
    assert P.param_specs(build_plan(with_keys)) == specs
    ic = P.param_specs(build_plan(with_keys, interctc=True))
    de = build_plan(enc).blocks[0].dim_expand
    assert ic[:len(specs)] == specs
    assert ic[len(specs):] == [("linear_expand_0.weight", (40, de), P.W), ("linear_expand_0.bias", (40,), P.B),
                               ("linear_proj_0.weight", (de, 40), P.W), ("linear_proj_0.bias", (de,), P.B)]


def test_named_configs_are_all_pinned():
    assert sorted(_NAMED) == sorted(SPEC_PINS)


@pytest.mark.parametrize("name", sorted(SD_PINS))
def test_make_state_dict_without_interctc_is_unchanged(name):
    sd = synth.make_state_dict(build_plan(named_config(name)["encoder_params"]), 7, 32)
    c = 0
    for k in sd:
        c = zlib.crc32(np.ascontiguousarray(sd[k]).tobytes(), zlib.crc32(k.encode(), c))
    assert c == SD_PINS[name]


def test_state_dict_keys_equal_the_reference_modules():
    enc = ConformerEncoderInterCTC(IR.tiny_params())
    g = IR.load_golden("flat", 47)
    want = bytes(g["state_dict_keys"]).decode().split("\n")
    assert sorted(enc.state_dict().keys()) == want
    sd = IR.tiny_state_dict("flat")
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if not k.startswith("fc.")}, strict=True)
    assert tuple(enc.linear_expand_3.weight.shape) == (32, 48) and tuple(enc.linear_proj_1.weight.shape) == (32, 32)
    # the plain class neither grows the modules nor accepts the keys
    plain = ConformerEncoder(IR.tiny_params())
    assert not any(k.startswith("linear_expand_") for k in plain.state_dict())
    with pytest.raises(RuntimeError):
        plain.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if not k.startswith("fc.")}, strict=True)


def test_model_type_dispatch():
    cfg = dict(named_config("Tiny"), model_type="InterCTC")
    cfg["encoder_params"] = dict(cfg["encoder_params"], interctc_blocks=[1, 3, 5])
    for m in (model_from_config(cfg), ModelCTC.from_config(cfg), InterCTC.from_config(cfg)):
        assert type(m) is InterCTC and type(m.encoder) is ConformerEncoderInterCTC
        assert m.encoder.plan.interctc_vocab == cfg["tokenizer_params"]["vocab_size"]              # model_ctc.py:189
        assert "encoder.linear_proj_5.bias" in m.state_dict() and "fc.weight" in m.state_dict()
    assert "vocab_size" not in cfg["encoder_params"]                                             # the caller's dict is left alone
    assert type(model_from_config(named_config("Tiny"))) is ModelCTC
    assert type(ModelCTC.from_config(named_config("Tiny")).encoder) is ConformerEncoder


# ------------------------------------------------------------------ the composed oracle against the reference's goldens
@pytest.mark.parametrize("tm", [47, 100])
@pytest.mark.parametrize("recipe", IR.RECIPES)
def test_composed_oracle_reproduces_the_goldens(recipe, tm):
    """float32-oracle-vs-golden scale of the existing goldens; measured 1.5e-6 (out) and 3e-6 (probabilities)."""
    g = IR.load_golden(recipe, tm)
    lens = dict(IR.BATCHES)[tm]
    mel, ln = IR.tiny_mel(tm, lens)
    plan = build_plan(IR.tiny_params(), interctc=True)
    with torch.no_grad():
        out, out_len, probs = IR.encoder_from_mel(torch.from_numpy(mel), torch.from_numpy(ln), IR.tiny_state_dict(recipe), plan)
    assert out_len.tolist() == g["out_len"].tolist()
    e_out = float((out - torch.from_numpy(g["out"])).abs().max())
    e_p = max(float((p - torch.from_numpy(g["probs_%d" % k])).abs().max()) for k, p in zip(IR.TINY_BLOCKS, probs))
    print("%s T%d: out %.2e probs %.2e" % (recipe, tm, e_out, e_p))
    assert e_out <= 5e-6 and e_p <= 1e-5
    if recipe == "peaky":
        assert max(float(p.max()) for p in probs) > 0.9999 and min(float(p.min()) for p in probs) < 1e-17


# ------------------------------------------------------------------ packing dry run and routes
def _tiny_handle(lib, precision="bf16", blocks=IR.TINY_BLOCKS, vocab=IR.TINY_VOCAB, drop=()):
    plan = build_plan(IR.tiny_params(blocks, vocab), interctc=True)
    sd = {k: v for k, v in synth.make_state_dict(plan, 7, 32).items() if k not in drop}
    h = pack_digest.create(lib, plan, 32, precision, sd)
    ids = (C.c_int32 * len(blocks))(*blocks)
    _lib.check(lib.effconf_encoder_set_interctc(h, ids, len(blocks), vocab), "set_interctc", lib)
    return h


def _routes_text(lib, h, ragged=False):
    buf = C.create_string_buffer(256 * 64)
    assert lib.effconf_debug_routes(h, int(ragged), buf, len(buf)) == 0, lib.effconf_last_error()
    return buf.value.decode()


@pytest.mark.parametrize("precision", ["bf16", "split"])
def test_pack_dry_run(precision):
    lib = _lib.load_debug()
    plain_plan, _, plain_sd = pack_digest.state_dict("Tiny")
    hp = pack_digest.create(lib, plain_plan, 32, precision, synth.make_state_dict(plain_plan, 7, 32))
    h = _tiny_handle(lib, precision)
    hm = _tiny_handle(lib, precision, drop=("linear_proj_3.weight",))
    try:
        rc, digest, buffers, nbytes = pack_digest.dry_run(lib, h)
        assert rc == 0, lib.effconf_last_error()
        rcp, dp, bp, nbp = pack_digest.dry_run(lib, hp)
        assert rcp == 0
        assert buffers > bp and nbytes > nbp and digest != dp           # the images of the three steps are part of the dry run
        assert pack_digest.dry_run(lib, h) == (rc, digest, buffers, nbytes)
        assert pack_digest.dry_run(lib, hm)[0] != 0
        assert "linear_proj_3.weight" in lib.effconf_last_error().decode()
    finally:
        for x in (h, hm, hp):
            lib.effconf_encoder_destroy(x)


def test_set_interctc_argument_errors():
    lib = _lib.load_debug()
    plan, _, sd = pack_digest.state_dict("Tiny")
    h = pack_digest.create(lib, plan, 32, "bf16", sd)
    try:
        for blocks, vocab, word in (([1, 6], 32, "outside"), ([1, 1], 32, "twice"), ([1], 1, "vocab_size")):
            assert lib.effconf_encoder_set_interctc(h, (C.c_int32 * len(blocks))(*blocks), len(blocks), vocab) != 0
            assert word in lib.effconf_last_error().decode()
        assert pack_digest.dry_run(lib, h)[0] == 0                      # refused calls left the handle as it was
    finally:
        lib.effconf_encoder_destroy(h)


def test_envelope_is_refused_at_finalize():
    """V = 1025 and De = 772 are outside the fused kernel's envelope: the packing (= finalize) fails with a message, no fallback."""
    lib = _lib.load_debug()
    h = _tiny_handle(lib, vocab=1025)
    try:
        assert pack_digest.dry_run(lib, h)[0] != 0
        msg = lib.effconf_last_error().decode()
        assert "1025" in msg and "1024" in msg and "block 1" in msg, msg
    finally:
        lib.effconf_encoder_destroy(h)
    wide = dict(named_config("Tiny")["encoder_params"], dim_model=[772, 772, 772], num_heads=193, att_group_size=1, num_blocks=1, expand_blocks=[],
                strided_blocks=[], interctc_blocks=[0], vocab_size=32)
    plan = build_plan(wide, interctc=True)
    h = pack_digest.create(lib, plan, 32, "bf16", synth.make_state_dict(plan, 7, 32))
    try:
        _lib.check(lib.effconf_encoder_set_interctc(h, (C.c_int32 * 1)(0), 1, 32), "set_interctc", lib)
        assert pack_digest.dry_run(lib, h)[0] != 0
        msg = lib.effconf_last_error().decode()
        assert "772" in msg and "768" in msg, msg
    finally:
        lib.effconf_encoder_destroy(h)


@pytest.mark.parametrize("precision", ["bf16", "split"])
def test_routes_of_an_interctc_handle(precision):
    lib = _lib.load_debug()
    plan, _, sd = pack_digest.state_dict("Tiny")
    hp = pack_digest.create(lib, plan, 32, precision, sd)
    h = _tiny_handle(lib, precision)
    try:
        plain, text = _routes_text(lib, hp), _routes_text(lib, h)
        assert "interctc" not in plain
        # a handle whose steps are taken away again prints what the plain handle prints
        _lib.check(lib.effconf_encoder_set_interctc(h, None, 0, 0), "set_interctc", lib)
        assert _routes_text(lib, h) == plain
    finally:
        lib.effconf_encoder_destroy(h)
        lib.effconf_encoder_destroy(hp)
    lines = text.splitlines()
    ic = [ln for ln in lines if ln.startswith("interctc ")]
    assert ic == ["interctc 1 De=32 V=32 route=fused", "interctc 3 De=48 V=32 route=fused", "interctc 5 De=48 V=32 route=fused"]
    fields = lambda prefix, k: dict(w.split("=") for w in next(ln for ln in lines if ln.startswith("%s %d " % (prefix, k))).split()[2:] if "=" in w)
    pfields = lambda prefix, k: dict(w.split("=") for w in next(ln for ln in plain.splitlines() if ln.startswith("%s %d " % (prefix, k))).split()[2:] if "=" in w)
    assert pfields("block", 2)["head"] == "prev_tail" or pfields("block", 1)["tail"] != "full"      # Tiny's transitions change the width: no full tail there anyway
    for k in (1, 3):
        assert fields("block", k)["tail"] == "tail"
    for k in (2, 4):
        assert fields("block", k)["head"] != "prev_tail"
    # blocks without a step keep their routes
    for k in (0,):
        assert fields("block", k) == pfields("block", k)
    if precision == "split":
        for kind in ("untraced", "traced", "maps"):
            for k in (1, 3, 5):
                assert fields("split %s block" % kind, k)["tail"] != "full"
            for k in (2, 4):
                assert fields("split %s block" % kind, k)["head"] != "prev_tail"


def test_a_step_between_equal_widths_splits_a_full_tail():
    """Tiny's listed blocks 1 and 3 are transitions (their tails never carried a head).  Block 4 -> 5 is 48 -> 48: listing block 4 turns its `full` tail into `tail`
    and block 5's `prev_tail` head into a chain of its own - the rule of routes.h, where it changes something."""
    lib = _lib.load_debug()
    plan, _, sd = pack_digest.state_dict("Tiny")
    hp = pack_digest.create(lib, plan, 32, "bf16", sd)
    h = _tiny_handle(lib, blocks=[4])
    try:
        plain, text = _routes_text(lib, hp).splitlines(), _routes_text(lib, h).splitlines()
    finally:
        lib.effconf_encoder_destroy(h)
        lib.effconf_encoder_destroy(hp)
    get = lambda lines, k: dict(w.split("=") for w in lines[1 + k].split()[2:])
    assert get(plain, 4)["tail"] == "full" and get(plain, 5)["head"] == "prev_tail"
    assert get(text, 4)["tail"] == "tail" and get(text, 5)["head"] == "chain"
    assert text[-1] == "interctc 4 De=48 V=32 route=fused"
    assert [get(text, k) for k in (0, 1, 2, 3)] == [get(plain, k) for k in (0, 1, 2, 3)]


# ------------------------------------------------------------------ the stage checker has teeth
SHAPES = [(24, 32), (120, 256), (240, 256), (256, 1000), (720, 1000)]


def _ratios(got, r64, r32, de, v):
    y = RB.stage_ratios(got[0], r64[0], [r[0] for r in r32], k_len=v, bf16_out=False)
    p = RB.stage_ratios(got[1], r64[1], [r[1] for r in r32], k_len=de, bf16_out=False)
    return max(y["max"], y["mean"]), max(p["max"], p["mean"])


@pytest.mark.parametrize("recipe", IR.RECIPES)
@pytest.mark.parametrize("de,v", SHAPES)
def test_stage_checker_accepts_and_rejects(de, v, recipe):
    """The bound the GPU tests hold the kernel to (oracle.ref_bf16.stage_ratios <= 1 against the float64 stage with p un-rounded, noise = float32 with q(p) at two
    summation orders) accepts legitimate float32 evaluations of the contract and rejects wrong kernels.  Measured: accepted ones at 0.08 - 0.25 of the bound,
    a missing bp at 8 - 1000 x, bf16 logits on the peaky recipe at 3.2 - 3.4 x."""
    torch.manual_seed(de * 1009 + v)
    sd = IR.stage_weights(de, v, 0, 7, recipe)
    x = torch.randn(96, de)
    r64, r32 = IR.stage_refs(x, sd, 0)
    perm = (torch.randperm(de), torch.randperm(v))
    other_order = IR.interctc_stage(x, sd, 0, torch.float32, True, order=perm)
    kernel_like = IR.interctc_stage(x, sd, 0, torch.float32, True, order=perm, round_exp=True)
    no_bp = IR.interctc_stage(x, sd, 0, torch.float32, True, drop_bp=True)
    figures = {"other_order": _ratios(other_order, r64, r32, de, v), "round_exp": _ratios(kernel_like, r64, r32, de, v), "no_bp": _ratios(no_bp, r64, r32, de, v)}
    print(de, v, recipe, {k: "%.3g / %.3g" % f for k, f in figures.items()})
    assert max(figures["other_order"]) <= 1.0 and max(figures["round_exp"]) <= 1.0
    assert figures["no_bp"][0] > 1.0
    if recipe == "peaky" and (de, v) in ((24, 32), (240, 256), (256, 1000)):
        rl = _ratios(IR.interctc_stage(x, sd, 0, torch.float32, True, round_logits=True), r64, r32, de, v)
        print(de, v, "round_logits %.3g / %.3g" % rl)
        assert max(rl) > 1.0
