"""Test helper (no tests here): the case table of the attention kernels' edge logic, its operands, its float64 reference and - in a few lines of
Python - the launch arithmetic of relpos_attention2_kernel (attention2.hip), so that the table can say on the CPU which kernel conditions each case reaches.
tests/test_gpu_attention_edges.py runs every case through effconf_debug_relpos_attention; tests/test_attention_cases_host.py proves the reference's
dead-row rule, asserts the coverage union and shows that the statistics see one wrong key block, band row or table row.

Operands: seeded float64 qu = Q + u, k, v (rows of D columns), dv = v - u (D,) and e (2 Tp - G rows; causal: Tp), scaled so that the largest |logit| is
about 8 and then rounded to bf16.  Chunk-padding rows by the contract: qu = u (a non-zero row), k = v = 0.  Rectangular batches hold B x Tp rows (every
frame of the rectangle is a query; keys behind lens[b] are masked); ragged batches hold every utterance's own frames padded to the group size, and e is
built for the longest one - utterance b reads its LAST 2 Tp_b - G (causal: Tp_b) rows.

Reference: oracle/ref_bf16.py attention_operands - oracle/ref_encoder.py relpos_scores with the band in FRAMES (left = band_l * G, right = band_r * G,
mask_stride 1) - per utterance, float64 and, as the noise model, float32 with P rounded to bf16.  Bounds: those of tests/bf16_parity.py check_trace for the
``attention`` stage, unchanged (ratios)."""
from collections import namedtuple

import torch

from oracle import ref_bf16 as Q

F64, F32 = torch.float64, torch.float32
UNL = 1 << 30            # an unlimited context (AttnParams: >= Tg)
BI = BJ = 64             # queries per workgroup / keys per block of relpos_attention2_kernel (variant 1)

# (D, H, G): head width d = G D / H, padded to 32
I32, I42, I64, I90, I96 = (128, 4, 1), (56, 4, 3), (256, 4, 1), (120, 4, 3), (128, 4, 3)
I128, I135, I160, I192 = (256, 2, 1), (180, 4, 3), (320, 2, 1), (192, 3, 3)

Case = namedtuple("Case", "name inst frames lens band causal ragged variants why")


def _c(name, inst, frames, lens, band=(UNL, UNL), causal=False, ragged=False, variants=(1,), why=""):
    return Case(name, inst, frames, tuple(lens), band, causal, ragged, variants, why)


# Lengths of the rectangular cases: [T, a length whose key count nkv lies 1 or 33 past a 64-key edge, 5 frames]; the 5-frame utterance has 2 - 5 key groups,
# so under every finite band_l its query tiles mix live and dead rows.  G = 3: T is no multiple of 3 everywhere (a chunk-padding group row exists).
CASES = [
    # ---- full context, rectangular: every instance once; variants 2 and 0 where they exist
    _c("full-d32-tg63", I32, 63, [63, 40, 5], variants=(1, 2), why="one key block, one query tile with idle waves; two staging sets, odd block count"),
    _c("full-d42-tg65", I42, 194, [194, 100, 5], variants=(1, 2), why="nkv = 65: a 1-key second block (short); d % 8 != 0 on dpad 64, one staging set"),
    _c("full-d64-tg129", I64, 129, [129, 97, 5], variants=(1, 2), why="three blocks, the last with 1 key; nkv = 97: 33 keys in the last block (full block)"),
    _c("full-d90-tg192", I90, 575, [575, 482, 5], variants=(0, 1, 2), why="Tg = 192, d = 90: the K / V block and the E batch that END at the last row take the masked tail path; nkv = 161"),
    _c("full-d96-tg97", I96, 290, [290, 194, 5], variants=(0, 1, 2), why="last block 33 keys (full) next to nkv = 65 (short)"),
    _c("full-d128-tg160-empty", I128, 160, [160, 129, 0], variants=(1, 2), why="last block 32 keys (short); an EMPTY utterance: every row dead, uniform over all 160 groups"),
    _c("full-d135-tg64", I135, 191, [191, 100, 5], why="launch2<160>: exactly one full block, d % 8 != 0: tail path in the only block"),
    _c("full-d160-tg193", I160, 193, [193, 161, 5], why="launch2<160> at d = 160: four blocks (even count, two staging sets), the last with 1 key"),
    _c("full-d192-tg65", I192, 194, [194, 120, 5], variants=(0,), why="dpad 192 runs on attention.hip only"),
    # ---- finite bands, rectangular
    _c("band0-0-d32-tg193", I32, 193, [193, 129, 5], (0, 0), why="the diagonal alone: kbeg = i0 at every tile (64, 128, 192), one visited block per tile"),
    _c("band1-0-d64-tg191", I64, 191, [191, 161, 5], (1, 0), why="kbeg = (i0 - 1) & ~63: two visited blocks from a non-zero start, one staging set"),
    _c("band0-1-d42-tg129", I42, 386, [386, 290, 5], (0, 1), why="right context 1: nkeys = i0 + 65, a 1-key short block under a band; d = 42"),
    _c("band15-16-d90-tg160", I90, 479, [479, 385, 5], (15, 16), why="both sides inside one block; nkeys = min(i0 + 80, nkv); d = 90 tails from kbeg = 64"),
    _c("band21-2-d96-tg193", I96, 578, [578, 482, 5], (21, 2), why="the streaming plan's band at stage 0 (left 64, right 8 frames, G = 3): the third tile starts at key block 1; the one-row fourth tile counts as dead (its absent rows lie behind the band) and visits every block"),
    _c("band63-0-d128-tg193", I128, 193, [193, 129, 5], (63, 0), why="band_l = 63: kbeg = (i0 - 63) & ~63 = i0 - 64, the largest band that still skips a block per tile; the one-row fourth tile starts at key block 2"),
    _c("band64-64-d135-tg193", I135, 578, [578, 385, 5], (64, 64), why="a band of exactly one block to either side: three visited blocks, launch2<160>, d = 135; fourth tile from key block 2"),
    _c("band65-1-d160-tg129", I160, 129, [129, 97, 5], (65, 1), why="band_l one past a block: kbeg falls back one more block"),
    _c("band100-unl-d64-tg193", I64, 193, [193, 161, 5], (100, UNL), why="left band only: kbeg > 0 with every key to the right visible (nkeys = nkv)"),
    _c("bandunl-3-d32-tg160", I32, 160, [160, 97, 5], (UNL, 3), why="right band only: kbeg = 0, nkeys = i0 + 67 (short last block under a band); no dead rows"),
    _c("band21-2-d90-tg193", I90, 577, [577, 290, 5], (21, 2), why="d = 90 with kbeg = 128: positional rows taken from a non-zero start on the tail-masked width"),
    _c("band15-16-d135-tg160", I135, 478, [478, 385, 5], (15, 16), why="launch2<160> under a band, two staging sets from kbeg = 64 and 128"),
    _c("band64-64-d42-tg192", I42, 575, [575, 482, 5], (64, 64), why="d = 42, Tg = 192: the K / V block that ends at row Tg - 1 under a band"),
    _c("band0-0-d160-tg97", I160, 97, [97, 65, 5], (0, 0), why="diagonal at d = 160; second tile: kbeg = 64, 33 keys (full block)"),
    _c("band1-0-d128-tg65", I128, 65, [65, 40, 5], (1, 0), why="second tile of one live row: keys 63 and 64 in two blocks"),
    # ---- causal tables (e holds Tp rows; band_r = 0), rectangular
    _c("causal-d64-tg192", I64, 192, [192, 129, 5], (UNL, 0), causal=True, why="causal, unlimited left: 1 .. 3 blocks per tile; the diagonal block reads the table's last rows"),
    _c("causal6-d90-tg129", I90, 386, [386, 290, 5], (6, 0), causal=True, why="causal with left context 6 (Small's stage-0 band is 21): d = 90, erows = Tg on the tail path"),
    _c("causal64-d32-tg193", I32, 193, [193, 161, 5], (64, 0), causal=True, why="causal, band_l = 64: kbeg = i0 - 64, two blocks per tile"),
    _c("causal6-d135-tg97", I135, 290, [290, 194, 5], (6, 0), causal=True, why="causal on launch2<160>"),
    _c("causal64-d96-tg160", I96, 479, [479, 385, 5], (64, 0), causal=True, why="causal at d = 96, one staging set, kbeg = 64 at the third tile"),
    _c("causal-d128-tg129", I128, 129, [129, 97, 5], (UNL, 0), causal=True, why="causal at d = 128; third tile holds one live row"),
    # ---- ragged batches (variant 1): [T, about 0.6 T, G - 1 or 1 frames]
    _c("ragged-full-d32-tg129", I32, 129, [129, 77, 1], ragged=True, why="ragged: a 1-frame utterance; the E offset (tgmax - Tg) rows for two shorter utterances"),
    _c("ragged-full-d42-tg97", I42, 290, [290, 175, 2], ragged=True, why="ragged at d = 42: an utterance of G - 1 frames (one group, mostly padding)"),
    _c("ragged-full-d90-tg192", I90, 575, [575, 346, 2], ragged=True, why="ragged, Tg = 192 and 116: tail paths at the utterance's OWN last row"),
    _c("ragged-full-d135-tg65", I135, 194, [194, 116, 1], ragged=True, why="ragged on launch2<160>"),
    _c("ragged-b11-d64", I64, 90, [41, 90, 20, 83, 33, 77, 26, 70, 64, 57, 49], ragged=True, why="B = 11, eleven lengths: rag_wg in the permuted utterance order (0, 8 | 1, 9 | 2, 10 | 3 | ..) with one or two tiles each"),
    _c("ragged-band21-2-d96-tg193", I96, 578, [578, 524, 2], (21, 2), ragged=True, why="the new stage case's shape on the kernel alone: ragged under (21, 2); the second utterance (Tg = 175, longer than 0.6 T for this) starts its third tile at key block 1 with a non-zero E offset"),
    _c("ragged-band21-2-d64-tg191", I64, 191, [191, 115, 1], (21, 2), ragged=True, why="ragged under a band with G = 1"),
    _c("ragged-causal-d90-tg160", I90, 479, [479, 290, 2], (UNL, 0), causal=True, ragged=True, why="ragged with causal tables: the offset (tgmax - Tg) rows into a Tg-row table"),
    _c("ragged-causal64-d128-tg193", I128, 193, [193, 116, 1], (64, 0), causal=True, ragged=True, why="ragged, causal and a left band at once"),
    _c("ragged-band64-64-d160-tg129", I160, 129, [129, 77, 1], (64, 64), ragged=True, why="ragged on launch2<160> under a band"),
    _c("ragged-causal6-d42-tg129", I42, 386, [386, 230, 1], (6, 0), causal=True, ragged=True, why="ragged, causal, d = 42"),
]
BY_NAME = {c.name: c for c in CASES}


def _up(n, g):
    return (n + g - 1) // g * g


def dims(case):
    """D, H, G, d, dpad, Tp, Tg of the launch (ragged: of the longest utterance)."""
    D, H, G = case.inst
    d = G * D // H
    tp = _up(case.frames, G)
    return D, H, G, d, _up(d, 32), tp, tp // G


def layout(case):
    """Per utterance: (first row in the Q / K / V row space, rows there, first output row, frames that are queries)."""
    G, T = case.inst[2], case.frames
    out, q0, o0 = [], 0, 0
    for n in case.lens:
        tp, t = (_up(n, G), n) if case.ragged else (_up(T, G), T)
        out.append((q0, tp, o0, t))
        q0 += tp
        o0 += tp if case.ragged else T
    return out


def operands(case, seed=None):
    """{"qu", "k", "v": (rows, D); "e": (erows, D); "dv": (D,); "u": (D,)}: float64 tensors holding bf16 numbers (dv: a bf16 number as well)."""
    D, H, G, d, dpad, tp, tg = dims(case)
    g = torch.Generator().manual_seed(CASES.index(case) + 9100 if seed is None else seed)
    rows = sum(r for _, r, _, _ in layout(case))
    qu, k, v = (torch.randn(rows, D, generator=g, dtype=F64) for _ in range(3))
    u = torch.randn(D, generator=g, dtype=F64)
    dv = torch.randn(D, generator=g, dtype=F64)
    e = torch.randn(tp if case.causal else 2 * tp - G, D, generator=g, dtype=F64)
    for q0, r, _, t in layout(case):
        qu[q0 + t: q0 + r] = u
        k[q0 + t: q0 + r] = 0.0
        v[q0 + t: q0 + r] = 0.0
    # scale to max |logit| about 8 on the longest utterance's unmasked scores (qu, k, e, dv scale alike: the scores by the square)
    q0, r, _, t = layout(case)[max(range(len(case.lens)), key=lambda b: case.lens[b]) if case.ragged else 0]
    s = Q.R.relpos_scores(qu[None, q0: q0 + r], qu[None, q0: q0 + r] + dv, k[None, q0: q0 + r], _table(case, e, r), None, r, H, G, causal=case.causal,
                          **({"right": 0} if case.causal else {}))
    a = (8.0 / float(s[s > -1e8].abs().max())) ** 0.5
    bf = lambda z: (z * a).to(torch.bfloat16).double()
    return {"qu": bf(qu), "k": bf(k), "v": v.to(torch.bfloat16).double(), "e": bf(e), "dv": bf(dv), "u": bf(u)}


def _table(case, e, tp_b, omit_offset=False):
    """The rows of ``e`` (built for the longest utterance) that an utterance of tp_b padded frames reads: its LAST 2 tp_b - G (causal: tp_b) rows."""
    D, H, G, d, dpad, tp, tg = dims(case)
    off = 0 if omit_offset else tp - tp_b
    return e[off: off + tp_b] if case.causal else e[off: off + 2 * tp_b - G]


def _ctx(case):
    G = case.inst[2]
    l, r = case.band
    ctx = {}
    if case.causal:
        ctx["causal"] = True
    if l < UNL:
        ctx["left"] = l * G
    if r < UNL:
        ctx["right"] = r * G
    return ctx


def reference(case, ops, dtype, round_p=False, fault=None, dead_rows="auto", scores=None):
    """(o, env): the attention output before its bf16 store and the envelope sum_j p_ij |v_j|, in the OUTPUT's row order (rectangular: B x T rows; ragged:
    every utterance's tp_b rows, the group-padding rows zero).  ``fault``: one of FAULTS (tests only); ``scores``: a list that receives every utterance's
    masked scores (1, H, Tg, Tg) as relpos_scores returns them."""
    D, H, G, d, dpad, tp, tg = dims(case)
    o, env = [], []
    for b, (q0, r, _, t) in enumerate(layout(case)):
        sl = slice(q0, q0 + r)
        n = case.lens[b]
        e_b = _table(case, ops["e"], r, omit_offset=(fault == "ragged E offset omitted"))
        edit = _fault_edit(case, fault, b, r // G, n, e_b) if fault else None
        if scores is not None:
            edit = lambda s, again: (scores.append(s), s)[1]
        a, en = Q.attention_operands(ops["qu"][None, sl], ops["k"][None, sl], ops["v"][None, sl], e_b, ops["dv"], torch.tensor([n]), t, H, G, dtype,
                                     round_p=round_p, ctx=_ctx(case), edit_scores=edit, dead_rows=dead_rows)
        if case.ragged and r > t:
            a, en = (torch.cat([z, torch.zeros(1, r - t, D, dtype=z.dtype)], 1) for z in (a, en))
        o.append(a[0])
        env.append(en[0])
    return torch.cat(o), torch.cat(env)


def ratios(case, got, o64, o32, env):
    """statistic / bound of one output (rows as ``reference`` orders them) exactly as tests/bf16_parity.py check_trace holds the ``attention`` stage: stage_ratios
    with share factor 2 against the float32 run(s) with P rounded, and the element-wise envelope 2^-7 env + 2e-5.  Only the statistics that count
    (``max``, ``mean``, ``share``, ``envelope``); every one must be <= 1."""
    D, H, G, d, dpad, tp, tg = dims(case)
    r = Q.stage_ratios(got, o64, o32, max(d, tg), True, share_factor=2.0)
    out = {k: v for k, v in r.items() if not k.startswith(("noise", "single"))}
    out["envelope"] = float(((got.double() - o64).abs() / (2.0 ** -7 * env + 2e-5)).max())
    return out


def live_rows(case):
    """Mask over the output rows: False on the group-padding rows of a ragged batch (kept zero by the kernel), True on every row that is compared."""
    m = []
    for q0, r, _, t in layout(case):
        m += [True] * t + ([False] * (r - t) if case.ragged else [])
    return torch.tensor(m)


# ------------------------------------------------------------------ the launch arithmetic of relpos_attention2_kernel (attention2.hip), variant 1
Tile = namedtuple("Tile", "b i0 tg nkv kbeg nkeys blocks nrows nlive dead live_in_dead short kv_tail e_tail kv_tail_d e_tail_d sets")


def tiles(case):
    """One entry per workgroup and head-independent: what the kernel computes from AttnParams before its key loop."""
    D, H, G, d, dpad, tp, tg_max = dims(case)
    ragged_d = d % 8 != 0
    sets = 1 if dpad in (64, 96) else 2                     # launch_relpos_attention2: ATT2_CASE(64, 1), ATT2_CASE(96, 1); 32 / 128 / 160: two sets
    out = []
    for b, n in enumerate(case.lens):
        tg = _up(n, G) // G if case.ragged else tg_max
        nkv = min((n + G - 1) // G, tg)
        band_l, band_r = min(case.band[0], tg), min(case.band[1], tg)
        banded = band_l < tg or band_r < tg
        erows = tg if case.causal else 2 * tg - 1
        for i0 in range(0, tg, BI):
            dead = nkv < 1 or i0 + BI - 1 - band_l >= nkv
            kbeg, nkeys = 0, nkv
            if dead:
                nkeys = tg
            elif banded:
                kbeg = max(i0 - band_l, 0) & ~(BJ - 1)
                nkeys = min(i0 + BI + band_r, nkv)
            blocks = list(range(kbeg, nkeys, BJ))
            rows = range(i0, min(i0 + BI, tg))
            live = [i for i in rows if not (nkv < 1 or i - band_l >= nkv)]
            r0 = tg - 1 - i0 - (BI - 1) + kbeg
            kv_tail = [not (jn + BJ <= tg - (1 if ragged_d else 0)) for jn in blocks]
            rnew = [r0 + (jn - kbeg) + BI - 1 for jn in blocks if jn > kbeg]
            e_tail = [not (r >= 0 and r + 63 < erows - (1 if ragged_d else 0)) for r in rnew]
            out.append(Tile(b, i0, tg, nkv, kbeg, nkeys, len(blocks), len(rows), len(live), dead, dead and bool(live) and len(live) < len(rows), (not dead) and bool(blocks) and nkeys - blocks[-1] <= 32,
                            any(kv_tail), any(e_tail), ragged_d and any(jn + BJ == tg for jn in blocks), ragged_d and any(r >= 0 and r + 63 == erows - 1 for r in rnew), sets))
    return out


def reached(case):
    """The conditions of the coverage union (tests/test_attention_cases_host.py) that a variant-1 launch of this case takes."""
    ts = tiles(case) if 1 in case.variants else []
    banded = case.band[0] < UNL or case.band[1] < UNL
    got = set()
    for t in ts:
        if t.kbeg >= 64:
            got.add("kbeg>=64")
        if t.kbeg >= 128:
            got.add("kbeg>=128")
        if 1 <= t.blocks <= 4:
            got.add("blocks=%d" % t.blocks)
            got.add("sets=%d,%s" % (t.sets, "odd" if t.blocks & 1 else "even"))
        if t.short and banded:
            got.add("short block under a band")
        if t.short and t.nkeys == t.nkv:
            got.add("short block at the key-padding edge")
        if t.live_in_dead:
            got.add("dead tile with live rows")
        if t.dead and t.nrows and not t.nlive:
            got.add("dead tile")
        if t.dead and t.nlive == t.nrows:
            got.add("dead tile without a dead row")
        if t.kv_tail_d:
            got.add("ragged_d tail K/V")
        if t.e_tail_d:
            got.add("ragged_d tail E")
        if case.causal and t.kbeg > 0 and t.blocks > 1:
            got.add("causal rnew from kbeg>0")
        if case.ragged and case.causal and t.tg < dims(case)[6]:
            got.add("ragged E offset with causal")
        if case.ragged and t.tg < dims(case)[6] and t.kbeg > 0:
            got.add("ragged E offset with kbeg>0")
    return got


# ------------------------------------------------------------------ faults injected through the reference (tests/test_attention_cases_host.py)
FAULTS = ("one key block dropped from the left of a banded tile", "band shifted by one position", "positional row off by one after a skipped block",
          "causal table indexed as if it had 2 Tg - 1 rows", "dead rows averaged over nkv groups", "ragged E offset omitted")


def _fault_edit(case, fault, b, tg, n, e_b):
    """edit_scores hook of ref_bf16.attention_operands for utterance b (tg groups, n valid frames, table e_b)."""
    D, H, G, d, dpad, tp, tg_max = dims(case)
    mine = [t for t in tiles(case) if t.b == b]

    def edit(s, again):
        s = s.clone()
        if fault == FAULTS[0]:          # the first visited block of the first tile that starts right of key 0 is never read: its keys are masked for the tile's rows
            t = next((t for t in mine if not t.dead and t.i0 >= BI), None)
            if t is not None:
                s[:, :, t.i0: t.i0 + BI, t.kbeg: t.kbeg + BJ] = -1e9
        elif fault == FAULTS[1]:        # keys j - i in [-band_l - 1, band_r - 1]
            l, r = case.band
            s = again(**dict(({"left": (l + 1) * G} if l < UNL else {}), **({"right": (r - 1) * G} if r < UNL else {})))
        elif fault == FAULTS[2]:        # tiles with kbeg > 0: the rows staged after the first block (rnew) come from one table row further on
            alt = again(torch.cat([e_b[G:], e_b[-G:]]))
            for t in mine:
                if t.kbeg > 0 and t.blocks > 1:
                    s[:, :, t.i0: t.i0 + BI, t.kbeg + BJ:] = torch.where(s[:, :, t.i0: t.i0 + BI, t.kbeg + BJ:] > Q.DEAD_ROW, alt[:, :, t.i0: t.i0 + BI, t.kbeg + BJ:],
                                                                          s[:, :, t.i0: t.i0 + BI, t.kbeg + BJ:])
        elif fault == FAULTS[3]:        # distance 0 looked up at the MIDDLE row of the table, (erows - 1) / 2, as in a table of both signs: erows = Tg here
            idx = (torch.arange(tg) - (tg - 1) + (tg - 1) // 2).clamp(0, tg - 1)
            s = again(e_b.reshape(tg, G, D)[idx].reshape(tg * G, D))
        elif fault == FAULTS[4]:
            nkv = min((n + G - 1) // G, tg)
            dead = s.amax(-1, keepdim=True) < Q.DEAD_ROW
            keys = (torch.arange(tg) < max(nkv, 1)).to(s.dtype)
            s = torch.where(dead, (1.0 - keys) * -1e30, s)
        return s
    return None if fault == FAULTS[5] else edit
