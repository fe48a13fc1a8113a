"""The route decisions of the bf16 schedule and of the label-exact split schedule (csrc/routes.h) read on the CPU: `effconf_debug_routes` (include/effconf_debug.h) packs a scratch copy of the handle in
dry mode and prints what `front_route`, `block_routes` and `attention_route` - the functions the forward itself reads - return under the handle's options.
Held against two independent statements of the rules: tests/bf16_parity.py (`front_route`, `chain_route`: the hand-written mirror the GPU trace tests use) over
the option grid tests/test_gpu_bf16_rounding.py walks, and a table of the three EfficientConformerCTC sizes under default options written out by hand from
forward_core as it stood before the routes had a file of their own.  The split schedule's lines (handles packed for "split"; `exact_forward_routes`,
`exact_block_routes`) are held against tests/split_parity.py (`split_route`, `SXC_WIDTHS`: the mirror the GPU stage tests choose their references by) over
split_chain x split_ffn x split_sublin x trace_fused x traced / untraced, and against a default table written by hand.  ConformerCTCLarge is left out as in tests/test_pack_host.py (its dry run takes seconds)."""
import ctypes as C
import functools
import importlib.util
import itertools
import os

import pytest

from bf16_parity import chain_route, front_route
from oracle.ref_split import CHAIN_KINDS, FFN_KINDS
from split_parity import SXC_WIDTHS, _kinds, split_route
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


# ------------------------------------------------------------------ the label-exact split schedule
def _split_routes(lib, h):
    """{kind: (forward fields, [per-block fields])} of the "split <kind> ..." lines effconf_debug_routes prints behind the bf16 ones; kind = untraced | traced | maps."""
    buf = C.create_string_buffer(1024 * 24)
    assert lib.effconf_debug_routes(h, 0, buf, len(buf)) == 0, lib.effconf_last_error()
    out = {}
    for ln in buf.value.decode().splitlines():
        words = ln.split()
        if words[0] != "split":
            continue
        fwd, blocks = out.setdefault(words[1], ({}, []))
        if words[2] == "block":
            assert words[3] == str(len(blocks))
            blocks.append(dict(w.split("=") for w in words[4:]))
        else:
            fwd.update(w.split("=") for w in words[2:])
    return out


SPLIT_MODELS = ["Tiny", _SM, _MD, _LG, "EfficientConformerTransducerSmall"]


@pytest.mark.parametrize("name", SPLIT_MODELS)
def test_split_option_grid_agrees_with_the_hand_written_mirror(name):
    """split_chain x split_ffn x split_sublin x trace_fused, traced and untraced (an untraced forward runs what a traced one runs under trace_fused = 1): the
    printed routes are split_parity.split_route's - the front end, and per block `_kinds` of the D-wide and the De-wide part - and the chain and FFN columns are
    on exactly where the width is in SXC_WIDTHS.  A bf16 handle prints no split line."""
    lib = _lib.load_debug()
    plan, vocab, sd = _weights(name)
    hb = pack_digest.create(lib, plan, vocab, "bf16", sd)
    try:
        assert _split_routes(lib, hb) == {}
    finally:
        lib.effconf_encoder_destroy(hb)
    h = pack_digest.create(lib, plan, vocab, "split", sd)
    try:
        for chain, ffn, sublin, tfused in itertools.product((0, 1), repeat=4):
            opts = {"split_chain": chain, "split_ffn": ffn, "split_sublin": sublin, "trace_fused": tfused}
            for k, v in opts.items():
                _lib.check(lib.effconf_encoder_set_option(h, k.encode(), v), "set_option(%s)" % k, lib)
            got = _split_routes(lib, h)
            assert sorted(got) == ["maps", "traced", "untraced"]
            assert got["maps"][0]["family"] == "modules" and all(r["head"] == r["b"] == r["tail"] == "modules" and r["attention"] != "sxf" for r in got["maps"][1])
            for kind in ("untraced", "traced"):
                want = split_route(plan, opts if kind == "traced" else dict(opts, trace_fused=1))
                fwd, blocks = got[kind]
                where = (name, opts, kind)
                assert fwd["family"] == "fused" and fwd["causal"] == "ok", where
                assert (fwd["front"] == "sublin") == want["sublin"], where
                assert len(blocks) == len(plan.blocks)
                for k, (b, r) in enumerate(zip(plan.blocks, blocks)):
                    D, De = b.dim_model, b.dim_expand
                    assert (int(r["D"]), int(r["De"])) == (D, De) and r["attention"] == "sxf"
                    kin, kout = _kinds(want, D)[0], _kinds(want, De)[0]
                    merged_in = k > 0 and blocks[k - 1]["tail"] == "full"
                    assert (r["head"] != "modules") == (kin is CHAIN_KINDS) and (r["b"] == "chain") == (kin is CHAIN_KINDS), (where, k, r)
                    assert (r["head"] == "prev_tail") == merged_in, (where, k, r)
                    assert r["ffn1"] == ("-" if kin is CHAIN_KINDS else ("fused" if kin is FFN_KINDS else "ln+gemms")), (where, k, r)
                    assert (r["tail"] != "modules") == (kout is CHAIN_KINDS), (where, k, r)
                    assert r["ffn2"] == ("-" if kout is CHAIN_KINDS else ("fused" if kout is FFN_KINDS else "ln+gemms")), (where, k, r)
                    nxt = plan.blocks[k + 1] if k + 1 < len(plan.blocks) else None
                    assert (r["tail"] == "full") == (kout is CHAIN_KINDS and nxt is not None and nxt.dim_model == De), (where, k, r)
                    # the columns are on exactly at the widths of the list
                    assert (r["b"] == "chain") == (bool(want["chain"]) and D in SXC_WIDTHS) and (r["tail"] != "modules") == (bool(want["chain"]) and De in SXC_WIDTHS), (where, k, r)
                    assert (r["ffn1"] == "fused") == (want["ffn"] and not want["chain"] and D in SXC_WIDTHS), (where, k, r)
                    assert (r["ffn2"] == "fused") == (want["ffn"] and not want["chain"] and De in SXC_WIDTHS), (where, k, r)
    finally:
        lib.effconf_encoder_destroy(h)


# Default options, untraced, written out from forward_exact as it stood with its predicates inline: (blocks, head, ffn1, b, tail, ffn2).  Chains at every width of
# SXC_WIDTHS; block 0 starts with chain A's head form, every later head runs in the previous block's chain A where the width carries on, the last block ends in the
# tail form.  Medium's block 10 expands 256 -> 360: its head ran in block 9's chain A, chain B at 256, and at 360 neither a chain nor an FFN image exists -
# pointwise-2, LayerNorm + two split GEMMs, LayerNorm; blocks 11 - 15 (360) are per-module throughout.
SPLIT_DEFAULT_TABLE = {
    _SM: [(1, "chain", "-", "chain", "full", "-"), (13, "prev_tail", "-", "chain", "full", "-"), (1, "prev_tail", "-", "chain", "tail", "-")],
    _MD: [(1, "chain", "-", "chain", "full", "-"), (9, "prev_tail", "-", "chain", "full", "-"), (1, "prev_tail", "-", "chain", "modules", "ln+gemms"),
          (5, "modules", "ln+gemms", "modules", "modules", "ln+gemms")],
}


@pytest.mark.parametrize("name", sorted(SPLIT_DEFAULT_TABLE))
def test_default_split_routes_are_the_hand_written_table(name):
    lib = _lib.load_debug()
    plan, vocab, sd = _weights(name)
    h = pack_digest.create(lib, plan, vocab, "split", sd)
    try:
        fwd, blocks = _split_routes(lib, h)["untraced"]
        assert fwd == dict(family="fused", front="sublin", causal="ok")
        want = [dict(head=head, ffn1=f1, b=b, tail=tail, ffn2=f2, attention="sxf") for n, head, f1, b, tail, f2 in SPLIT_DEFAULT_TABLE[name] for _ in range(n)]
        assert len(blocks) == len(want)
        for k, (r, w) in enumerate(zip(blocks, want)):
            assert {f: r[f] for f in w} == w, (name, k, r)
        # a traced forward without trace_fused: per-module kernels around the FFN-only form wherever the width has an image
        _, traced = _split_routes(lib, h)["traced"]
        for b, r in zip(plan.blocks, traced):
            assert (r["head"], r["b"], r["tail"]) == ("modules",) * 3
            assert (r["ffn1"], r["ffn2"]) == tuple("fused" if d in SXC_WIDTHS else "ln+gemms" for d in (b.dim_model, b.dim_expand)), r
    finally:
        lib.effconf_encoder_destroy(h)
