"""The bf16 schedule's route decisions (csrc/routes.h) read on the CPU: `effconf_debug_routes` (include/effconf_debug.h) packs a scratch copy of the handle in
dry mode and prints what `front_route`, `block_routes` and `attention_route` - the functions the forward itself reads - return under the handle's options.
Held against two independent statements of the rules: tests/bf16_parity.py (`front_route`, `chain_route`: the hand-written mirror the GPU trace tests use) over
the option grid tests/test_gpu_bf16_rounding.py walks, and a table of the three EfficientConformerCTC sizes under default options written out by hand from
forward_core as it stood before the routes had a file of their own.  ConformerCTCLarge is left out as in tests/test_pack_host.py (its dry run takes seconds)."""
import ctypes as C
import functools
import importlib.util
import itertools
import os

import pytest

from bf16_parity import chain_route, front_route
from efficientconformer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("pack_digest", os.path.join(ROOT, "tools", "pack_digest.py"))
pack_digest = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pack_digest)

_SM, _MD, _LG = "EfficientConformerCTCSmall", "EfficientConformerCTCMedium", "EfficientConformerCTCLarge"
GRID_MODELS = ["Tiny", _SM, _MD, _LG, "ConformerCTCSmall"]


@functools.lru_cache(maxsize=1)
def _weights(name):
    return pack_digest.state_dict(name)


def _routes(lib, h, ragged):
    """(front-end fields, [per-block fields]) of one effconf_debug_routes call: every line's key=value words as a dict (the front end's route under "route")."""
    buf = C.create_string_buffer(256 * 20)
    assert lib.effconf_debug_routes(h, int(ragged), buf, len(buf)) == 0, lib.effconf_last_error()
    lines = buf.value.decode().splitlines()
    words = lines[0].split()
    assert words[0] == "front"
    front = dict([("route", words[1])] + [w.split("=") for w in words[2:]])
    blocks = []
    for k, ln in enumerate(lines[1:]):
        words = ln.split()
        assert words[:2] == ["block", str(k)]
        blocks.append(dict(w.split("=") for w in words[2:]))
    return front, blocks


@pytest.mark.parametrize("ragged", [False, True], ids=["rect", "ragged"])
@pytest.mark.parametrize("name", GRID_MODELS)
def test_option_grid_agrees_with_the_hand_written_mirror(name, ragged):
    """fuse_subsample 0 .. 3 x sub3_auto x fuse_chain, on a rectangular and on a ragged batch: the printed front-end route is the one bf16_parity.front_route expects, the workspace
    scratch is what that route needs, and the chain columns follow bf16_parity.chain_route (D for the head and chain B, De for the tail)."""
    lib = _lib.load_debug()
    plan, vocab, sd = _weights(name)
    h = pack_digest.create(lib, plan, vocab, "bf16", sd)
    try:
        for fuse, auto, chain in itertools.product((0, 1, 2, 3), (0, 1), (0, 1)):
            opts = {"fuse_subsample": fuse, "sub3_auto": auto, "fuse_chain": chain}
            for k, v in opts.items():
                _lib.check(lib.effconf_encoder_set_option(h, k.encode(), v), "set_option(%s)" % k, lib)
            front, blocks = _routes(lib, h, ragged)
            want = front_route(plan, opts, ragged)
            if plan.sub_layers == 2:
                allowed = {"two_layer"}
            elif want["conv"] == "split":
                allowed = {"chunked", "row_stationary"}            # the two matrix-pipe fused routes
            else:
                allowed = {"conv_gemm"} if want["subsample"] else {"tiled_fused"}
            where = (name, opts, "ragged" if ragged else "rect", front)
            assert front["route"] in allowed, where
            unfused = front["route"] in ("two_layer", "conv_gemm")
            assert front["sub"] == str(int(unfused or not ragged)), where              # rectangular batches keep the reservation whatever the route
            assert front["sub1"] == str(int(front["route"] == "two_layer")) and front["xrect"] == str(int(ragged and front["route"] == "two_layer")), where
            assert len(blocks) == len(plan.blocks)
            for k, (b, r) in enumerate(zip(plan.blocks, blocks)):
                assert (int(r["D"]), int(r["De"])) == (b.dim_model, b.dim_expand)
                assert (r["head"] != "modules") == chain_route(chain, b.dim_model), (where, k, r)
                assert (r["b"] == "chain") == chain_route(chain, b.dim_model), (where, k, r)
                assert (r["tail"] != "modules") == chain_route(chain, b.dim_expand), (where, k, r)
                assert (r["head"] == "prev_tail") == (k > 0 and blocks[k - 1]["tail"] == "full"), (where, k, r)
    finally:
        lib.effconf_encoder_destroy(h)


# Default options, read off forward_core before routes.h existed.  One entry per run of equal blocks: (blocks, head, b, tail, attention, modules) with `modules`
# the per-module kernels of the parts that are not chains ("-": none).
#   chains: every width <= 256 (chain_supported, chain_max_dim = 256); block 0 starts with CHAIN_A_HEAD, every later head ran in the previous tail where the
#   width carries on and chain_full_supported(De, pair ? 256 : chain_full_max = 192): 120 / 168 / 180 by chain_full_max, 240 / 256 by the chain3.hip pair;
#   the last block and a block in front of a width without chains end in CHAIN_A_TAIL / modules.
#   modules: K <= 384 fits the row-stationary kernels (fused FFN, LayerNorm in the prologue of Q/K/V and pointwise-1) unless prefer_tiled - Medium's widest stage is
#   360, so tiled_auto sends it to LayerNorm + tiled GEMMs; Large's widest is 720, so its 360 stage stays row-stationary and 512 / 720 are beyond the kernels.
#   Block 4 of Large expands 360 -> 512: its D-wide modules are row-stationary, conv_res (512 resident columns), pointwise-2 and FFN2 are tiled.
#   attention: attention2.hip's 2-wave variant everywhere (attention_v2 = 1; padded head widths 96 / 64 / 64, 160 / 64 / 96, 160 / 64 / 96).
_RS = dict(ffn1="fused", qkv="ln_rs", outp="rs", pw1="ln_rs", pw2="rs", ffn2="ln_fused")
_TILED = dict(ffn1="tiled", qkv="ln+tiled", outp="tiled", pw1="ln+tiled", pw2="tiled", ffn2="ln+tiled")
_NONE = dict(ffn1="-", qkv="-", outp="-", pw1="-", pw2="-", ffn2="-")
DEFAULT_TABLE = {
    _SM: [(1, "chain", "chain", "full", "attention2/1", _NONE), (13, "prev_tail", "chain", "full", "attention2/1", _NONE),
          (1, "prev_tail", "chain", "tail", "attention2/1", _NONE)],
    _MD: [(1, "chain", "chain", "full", "attention2/1", _NONE), (9, "prev_tail", "chain", "full", "attention2/1", _NONE),
          (1, "prev_tail", "chain", "modules", "attention2/1", dict(_NONE, pw2="tiled", ffn2="ln+tiled")),          # 256 -> 360: the De-wide part on the tiled kernels
          (5, "modules", "modules", "modules", "attention2/1", _TILED)],
    _LG: [(4, "modules", "modules", "modules", "attention2/1", _RS),
          (1, "modules", "modules", "modules", "attention2/1", dict(_RS, pw2="tiled", ffn2="ln+tiled")),            # 360 -> 512
          (11, "modules", "modules", "modules", "attention2/1", _TILED)],
}
DEFAULT_FRONT = {_SM: "row_stationary", _MD: "chunked", _LG: "chunked"}       # sublinear2.hip up to 128 channels / columns, sublinear3.hip above (sub3_auto)


@pytest.mark.parametrize("name", sorted(DEFAULT_TABLE))
def test_default_routes_of_the_three_sizes_are_the_hand_written_table(name):
    lib = _lib.load_debug()
    plan, vocab, sd = _weights(name)
    h = pack_digest.create(lib, plan, vocab, "bf16", sd)
    try:
        want = [dict(mods, head=head, b=b, tail=tail, attention=att) for n, head, b, tail, att, mods in DEFAULT_TABLE[name] for _ in range(n)]
        for ragged in (False, True):
            front, blocks = _routes(lib, h, ragged)
            assert front["route"] == DEFAULT_FRONT[name]
            assert len(blocks) == len(want)
            for k, (r, w) in enumerate(zip(blocks, want)):
                assert {f: r[f] for f in w} == w, (name, k, r)
    finally:
        lib.effconf_encoder_destroy(h)


def test_refusals_and_attention_variants_are_reported():
    """attention_v2 = 0 keeps attention.hip for rectangular batches only (ragged batches need attention2.hip); a null handle and a short buffer are refused."""
    lib = _lib.load_debug()
    plan, vocab, sd = _weights("Tiny")
    h = pack_digest.create(lib, plan, vocab, "bf16", sd)
    try:
        _lib.check(lib.effconf_encoder_set_option(h, b"attention_v2", 0), "set_option", lib)
        assert {r["attention"] for r in _routes(lib, h, False)[1]} == {"attention"}
        assert {r["attention"] for r in _routes(lib, h, True)[1]} == {"attention2/1"}
        _lib.check(lib.effconf_encoder_set_option(h, b"attention_v2", 2), "set_option", lib)
        assert {r["attention"] for r in _routes(lib, h, False)[1]} == {"attention2/2"}
        buf = C.create_string_buffer(16)
        assert lib.effconf_debug_routes(h, 0, buf, len(buf)) != 0 and lib.effconf_debug_routes(None, 0, buf, len(buf)) != 0
        assert lib.effconf_encoder_forward_mel(h, None, None, 2, 64, None, None, None, 0, None) != 0 and lib.effconf_last_error() == b"encoder not finalized"
    finally:
        lib.effconf_encoder_destroy(h)
