"""CPU: the case table of tests/attention_cases.py is what tests/test_gpu_attention_edges.py takes it for.

* Dead rows: the float64 reference sets the scores of a query whose every key is masked to 0 (uniform softmax over all Tg key groups).  Proved against
  relpos_scores run in float32 on the same operands, where -1e9 + s IS -1e9 for |s| < 32 - the precondition, asserted on every case.
* Coverage: which conditions of relpos_attention2_kernel each case reaches, recomputed from the launch arithmetic; the union over the table is asserted,
  so that an edit of the table cannot silently drop a path.
* Sensitivity: a stand-in for a correct kernel (the float32 reference on the kernels' exp formula, P rounded, output rounded to bf16) stays inside every
  bound; the same stand-in with one fault - a key block dropped, the band one position off, one positional row off after a skipped block, the causal table
  read from its middle, dead rows averaged over nkv groups, a ragged E offset omitted - exceeds some bound, each at the smallest case that has the path.
* The entry's refusals, by message: no launch is needed for them, so they run on the host."""
import ctypes as C

import pytest
import torch

import attention_cases as A
from attention_cases import BY_NAME, CASES, F32, F64, FAULTS, UNL
from efficientconformer_amd import _lib
from oracle import ref_bf16 as Q

_OPS = {}


def _ops(case):
    if case.name not in _OPS:
        _OPS[case.name] = A.operands(case)
    return _OPS[case.name]


def test_the_table_is_what_the_issue_lists():
    assert 36 <= len(CASES) <= 44 and len(BY_NAME) == len(CASES)
    assert {c.inst for c in CASES} == {A.I32, A.I42, A.I64, A.I90, A.I96, A.I128, A.I135, A.I160, A.I192}
    assert {A.dims(c)[6] for c in CASES if len(c.lens) == 3} >= {63, 64, 65, 97, 129, 160, 191, 192, 193}
    assert {c.band for c in CASES if not c.causal} >= {(UNL, UNL), (0, 0), (1, 0), (0, 1), (15, 16), (21, 2), (63, 0), (64, 64), (65, 1), (100, UNL), (UNL, 3)}
    assert {c.band for c in CASES if c.causal} == {(UNL, 0), (6, 0), (64, 0)}
    for c in CASES:
        D, H, G, d, dpad, tp, tg = A.dims(c)
        assert c.why and (G == 1 or c.frames % G), c.name
        assert max(c.lens) == c.frames and (not c.ragged or c.variants == (1,)), c.name
        if 2 in c.variants or 0 in c.variants:                     # attention_route: streaming and ragged batches run variant 1
            assert c.band == (UNL, UNL) and not c.causal and not c.ragged, c.name
        assert (2 not in c.variants or dpad in (32, 64, 96, 128)) and (0 not in c.variants or dpad in (96, 192)), c.name
    assert any(len(c.lens) == 11 and len(set(c.lens)) == 11 and c.ragged for c in CASES) and any(0 in c.lens for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_dead_rows_are_the_float32_reference_and_logits_stay_below_32(case):
    ops = _ops(case)
    with torch.no_grad():
        sc = []
        o64, _ = A.reference(case, ops, F64, scores=sc)
        top = max(float(s[s > Q.DEAD_ROW].abs().max()) for s in sc if bool((s > Q.DEAD_ROW).any()))
        # the precondition of the dead-row rule: float32(s - 1e9) == -1e9 exactly (the spacing of float32 numbers at 1e9 is 64)
        assert top < 32.0, (case.name, top)
        assert 4.0 < top < 12.0, (case.name, top)                   # "max |logit| about 8": the rescale threshold is another test's business
        o32, _ = A.reference(case, ops, F32, dead_rows="keep")      # relpos_scores and the softmax in float32, nothing special-cased
        o64k, _ = A.reference(case, ops, F64, dead_rows="keep")     # float64 WITHOUT the rule: s - 1e9 keeps s
    dead = torch.cat([torch.cat([(s[0, 0].amax(-1) < Q.DEAD_ROW)[:, None].expand(-1, case.inst[2]).reshape(-1)[:t],
                                 torch.zeros(r - t if case.ragged else 0, dtype=torch.bool)]) for s, (_, r, _, t) in zip(sc, A.layout(case))])
    assert dead.shape[0] == o64.shape[0]
    err = (o32.double() - o64).abs().max(-1).values
    assert float(err.max()) < 2e-5, (case.name, float(err.max()))          # float32 arithmetic on outputs of magnitude <= 4
    if bool(dead.any()):
        # the rule is needed: without it float64 gives those rows another (non-uniform) average
        assert float((o64k - o64).abs()[dead].max()) > 1e-2, case.name
        assert float((o64k - o64).abs()[~dead].max() if bool((~dead).any()) else 0.0) == 0.0
    expect_dead = any(n == 0 for n in case.lens) or (not case.ragged and case.band[0] < A.dims(case)[6] - 5)
    assert bool(dead.any()) == expect_dead, (case.name, int(dead.sum()))


WANTED = {"kbeg>=64", "kbeg>=128", "blocks=1", "blocks=2", "blocks=3", "blocks=4", "sets=1,odd", "sets=1,even", "sets=2,odd", "sets=2,even",
          "short block under a band", "short block at the key-padding edge", "dead tile with live rows", "dead tile", "dead tile without a dead row", "ragged_d tail K/V", "ragged_d tail E",
          "causal rnew from kbeg>0", "ragged E offset with causal", "ragged E offset with kbeg>0"}


def test_the_table_reaches_every_kernel_condition():
    per_case = {c.name: A.reached(c) for c in CASES}
    union = set().union(*per_case.values())
    for cond in sorted(WANTED):
        print("%-36s %s" % (cond, ", ".join(n for n, s in per_case.items() if cond in s)))
    assert union >= WANTED, sorted(WANTED - union)
    # the conditions the stage tests never reached are reached by more than one instance, on both staging forms
    for cond in ("kbeg>=64", "kbeg>=128", "dead tile with live rows", "short block under a band"):
        insts = {BY_NAME[n].inst for n, s in per_case.items() if cond in s}
        assert len(insts) >= 3, (cond, insts)
    # spot checks of the arithmetic itself against attention2.hip read by hand
    t = [x for x in A.tiles(BY_NAME["band21-2-d96-tg193"]) if x.b == 0]
    assert [(x.i0, x.kbeg, x.nkeys, x.blocks) for x in t] == [(0, 0, 66, 2), (64, 0, 130, 3), (128, 64, 193, 3), (192, 0, 193, 4)]
    t = [x for x in A.tiles(BY_NAME["band21-2-d96-tg193"]) if x.b == 2]                  # 5 frames, 2 key groups: rows >= 23 dead
    assert [(x.dead, x.live_in_dead, x.kbeg, x.nkeys) for x in t] == [(True, True, 0, 193), (True, False, 0, 193), (True, False, 0, 193), (True, False, 0, 193)]


FAULT_CASE = {FAULTS[0]: "band65-1-d160-tg129", FAULTS[1]: "band1-0-d128-tg65", FAULTS[2]: "band1-0-d64-tg191", FAULTS[3]: "causal-d128-tg129",
              FAULTS[4]: "band1-0-d128-tg65", FAULTS[5]: "ragged-full-d32-tg129"}


@pytest.mark.parametrize("fault", FAULTS)
def test_the_statistics_see_the_fault(fault):
    case = BY_NAME[FAULT_CASE[fault]]
    ops = _ops(case)
    live = A.live_rows(case)
    with torch.no_grad():
        o64, env = A.reference(case, ops, F64)
        o32, _ = A.reference(case, ops, F32, round_p=True)
        with Q.hardware_like(1):
            good = Q.q(A.reference(case, ops, F32, round_p=True)[0])
            bad = Q.q(A.reference(case, ops, F32, round_p=True, fault=fault)[0])
    rg = A.ratios(case, good[live], o64[live], o32[live], env[live])
    rb = A.ratios(case, bad[live], o64[live], o32[live], env[live])
    print("%s | %s | unfaulted %s | faulted %s" % (case.name, fault, {k: "%.3g" % v for k, v in rg.items()}, {k: "%.3g" % v for k, v in rb.items()}))
    assert max(rg.values()) <= 1.0, (fault, rg)
    assert max(rb.values()) > 1.0, (fault, rb)


def _refusal(**kw):
    lib = _lib.load_debug()
    a = dict(batch=2, heads=4, frames=130, group=1, dim=128, variant=1, band_l=UNL, band_r=UNL, causal=0, ragged=0)
    a.update(kw)
    buf = (C.c_int64 * 64)()
    lens = (C.c_int64 * a["batch"])(*([a["frames"]] * a["batch"]))
    p = C.addressof(buf)
    dpad = (a["group"] * a["dim"] // a["heads"] + 31) // 32 * 32
    rc = lib.effconf_debug_relpos_attention(p, p, p, p, p, dpad, p, C.addressof(lens), a["batch"], a["heads"], a["frames"], a["group"], a["dim"], p, a["dim"], a["variant"],
                                            a["band_l"], a["band_r"], a["causal"], a["ragged"], p, 0, None)
    assert rc != 0, a
    return lib.effconf_last_error().decode()


def test_the_entry_refuses_what_the_forward_refuses_by_the_same_text():
    streaming = "streaming contexts / causal attention run on attention2.hip (padded head width <= 160, option attention_v2 != 0)"
    ragged = "ragged batches need attention2.hip (padded head width <= 160)"
    assert _refusal(variant=0, band_l=21, band_r=2) == streaming
    assert _refusal(variant=0, band_r=0, causal=1) == streaming
    assert _refusal(variant=1, heads=3, group=3, dim=192, band_l=21) == streaming        # dpad 192
    assert _refusal(variant=1, heads=3, group=3, dim=192, ragged=1) == ragged
    other = "another kernel than the variant asked for"      # a forward would not refuse these: it runs variant 1 (or attention.hip) whatever the option says
    assert other in _refusal(variant=0, ragged=1) and other in _refusal(variant=2, band_l=21) and other in _refusal(variant=2, ragged=1)
    assert other in _refusal(variant=2, heads=3, group=3, dim=192)
    assert "band_r must be 0" in _refusal(causal=1, band_r=3)
    assert "band_l / band_r" in _refusal(band_l=-1)
    assert "workspace too small" in _refusal()                                           # everything else accepted: stops at the workspace size, before any launch
