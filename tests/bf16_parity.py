"""Test helper (no tests here): one traced forward of the bf16 path against oracle/ref_bf16.py, stage by stage - the row maps of rectangular and
ragged batches, the report of statistic / bound ratios and the checker both tests/test_gpu_bf16_rounding.py (GPU traces) and
tests/test_ref_bf16_host.py (traces made on the CPU) run."""
import numpy as np
import torch

from oracle.ref_bf16 import (attention, chain_a, conv_res, depthwise, f32_runs, glu, out_proj, pos_e, q, qkv, rel, stage_ratios, worst_element)

F64, F32 = torch.float64, torch.float32


def _up(n, g):
    return (n + g - 1) // g * g


class _Space:
    """Row map of one block's input (k < nb) or of the encoder output (k = nb): utterance b's frames t < live[b] are the rows x0[b] + t of the
    residual stream and q0[b] + t of the Q / K / V buffers, which hold tp[b] rows per utterance.  Rectangular: every frame of the rectangle is
    live (pad frames are computed like any other).  Ragged: the utterance's own frames; the rows up to the group size are padding."""

    def __init__(self, ragged, lens, t_rect, g):
        self.lens = [int(v) for v in lens]
        if ragged:
            self.live = list(self.lens)
            self.tp = [_up(v, g) for v in self.live]
            self.x0 = [0] + list(np.cumsum(self.tp)[:-1])
            self.q0 = list(self.x0)
            self.rows = int(sum(self.tp))
        else:
            self.live = [t_rect] * len(self.lens)
            self.tp = [_up(t_rect, g)] * len(self.lens)
            self.x0 = [b * t_rect for b in range(len(self.lens))]
            self.q0 = [b * self.tp[0] for b in range(len(self.lens))]
            self.rows = t_rect * len(self.lens)
        self.qrows = int(sum(self.tp))
        self.xidx = torch.cat([torch.arange(a, a + n) for a, n in zip(self.x0, self.live)])
        self.qidx = torch.cat([torch.arange(a, a + n) for a, n in zip(self.q0, self.live)])
        self.qpad = torch.cat([torch.arange(a + n, a + p) for a, n, p in zip(self.q0, self.live, self.tp)])

    def utt(self, flat, b, padded=False):
        return flat[self.q0[b]: self.q0[b] + self.tp[b]] if padded else flat[self.x0[b]: self.x0[b] + self.live[b]]


class _Report:
    def __init__(self, label):
        self.label, self.worst, self.fails = label, {}, []

    def add(self, stage, k, ratios, detail):
        for stat, v in ratios.items():
            key = (stage, stat)
            if v > self.worst.get(key, (-1.0, 0))[0]:
                self.worst[key] = (v, k)
            if not stat.startswith(("noise", "single")) and not v <= 1.0:
                self.fails.append("block %d %s %s: %.3g x its bound; %s" % (k, stage, stat, v, detail()))

    def elementwise(self, stage, k, name, err, bound, got, ref):
        r = float((err / bound).max())
        self.add(stage, k, {name: r}, lambda: worst_element(got, ref, bound))

    def finish(self):
        for stage in sorted({s for s, _ in self.worst}):
            print("%s | %-8s | %s" % (self.label, stage, "  ".join("%s %.3g (block %d)" % (st, v, k) for (s, st), (v, k) in sorted(self.worst.items()) if s == stage)))
        assert not self.fails, "%d statistics over their bound, first: %s" % (len(self.fails), " || ".join(self.fails[:6]))


def _misses(x: torch.Tensor, r64: torch.Tensor) -> str:
    m = x.double() != q(r64).double()
    return "%d of %d elements off q(r64) in %d rows" % (int(m.sum()), m.numel(), int(m.reshape(-1, m.shape[-1]).any(-1).sum()))


def check_trace(got, out_len, plan, sd, ln, tm, ragged, fuse, label):
    """Every stage of every block of one traced forward (``got``: trace name -> float tensor of (rows, columns)) against the reference computed
    from the trace's own inputs of that stage.  Returns the _Report (``finish`` prints the worst ratios and asserts).  ``fuse``: the fused chains
    are on (option fuse_chain), so the widths they support take the folded-LayerNorm route."""
    nb, B = len(plan.blocks), len(ln)
    chained = lambda width: bool(fuse) and width % 4 == 0 and 16 <= width <= 256          # encoder.hip: chain_max_dim = 256; chain.hip chain_supported
    rep = _Report(label)

    # lengths and the row map of every block's input (and of the output)
    cur = [int(v) for v in ln]
    t_rect = tm
    for _ in range(plan.sub_layers):
        cur = [(v - 1) // 2 + 1 for v in cur]
        t_rect = (t_rect - 1) // 2 + 1
    spaces = []
    for bp in plan.blocks:
        spaces.append(_Space(ragged, cur, t_rect, bp.group_size))
        if bp.conv_stride > 1:
            cur = [(v - 1) // bp.conv_stride + 1 for v in cur]
            t_rect = (t_rect - 1) // bp.conv_stride + 1
    spaces.append(_Space(ragged, cur, t_rect, 1))
    assert [int(v) for v in out_len] == cur

    for k, bp in enumerate(plan.blocks):
        p = "blocks.%d." % k
        si, so = spaces[k], spaces[k + 1]
        D, De = bp.dim_model, bp.dim_expand
        fin, fout = chained(D), chained(De)
        # the route the reference's ``folded`` flags assume: x_conv leaves the registers only on the per-module route
        assert ((p + "x_conv") in got) == (not fout), (k, "chain A tail expected" if fout else "per-module route expected")
        x_ffn1, x_mhsa, att_o, g_glu, g_dw = (got[p + n] for n in ("x_ffn1", "x_mhsa", "att_o", "glu", "dw"))
        qu, kk, vv, ee = (got[p + n] for n in ("qu", "k", "v", "e"))
        # every excluded row is a group-padding row, and there are as many as the lengths imply
        assert x_ffn1.shape[0] == si.rows and qu.shape[0] == si.qrows and g_dw.shape[0] == so.rows and g_glu.shape[0] == si.rows, (k, x_ffn1.shape, qu.shape, g_dw.shape)
        assert si.rows - len(si.xidx) == (sum(_up(v, bp.group_size) - v for v in si.lens) if ragged else 0)

        # ---- Q / K / V: chain A head part / rs_gemm QKV, pad-row kernels
        xin = x_ffn1[si.xidx]
        r64, r32 = qkv(xin, sd, bp, F64, fin), f32_runs(lambda: qkv(xin, sd, bp, F32, fin))
        for i, (nme, g) in enumerate(zip(("qu", "k", "v"), (qu, kk, vv))):
            gv, a, b = g[si.qidx], r64[i], [r[i] for r in r32]
            rep.add("qkv", k, stage_ratios(gv, a, b, D, True), lambda: "%s gpu %s, float32 runs %s; %s" % (nme, _misses(gv, a), [_misses(q(r), a).split(" of")[0] for r in b], worst_element(gv, a)))
        # the route behind ``fin`` (chain A head / chain B with the LayerNorm folded at pack time, or the per-module kernels) leaves no trace entry of its
        # own: it is asserted through the data - the other route's reference (other weight and operand roundings) must fit the GPU's numbers worse
        other = qkv(xin, sd, bp, F64, not fin)[0]
        fit, misfit = rel(qu[si.qidx], r64[0])[1], rel(qu[si.qidx], other)[1]
        assert fit < misfit, (k, "Q/K/V: expected the %s route" % ("folded-LayerNorm (chain)" if fin else "per-module"), fit, misfit)
        if len(si.qpad):
            u = q(torch.from_numpy(np.asarray(sd["blocks.%d.multi_head_self_attention_module.mhsa.u" % k])).float())
            assert torch.equal(qu[si.qpad], u.expand(len(si.qpad), -1)) and float(kk[si.qpad].abs().sum()) == 0.0 and float(vv[si.qpad].abs().sum()) == 0.0, (k, "chunk-padding rows")

        # ---- positional rows E (gemm.hip on the table of encoder.hip build_pos_table); the table's own float32 angles are part of the noise model
        tpmax = max(si.tp)
        assert ee.shape[0] == (tpmax if plan.causal else 2 * tpmax - bp.group_size), (k, ee.shape)
        e64, e32 = pos_e(tpmax, sd, bp, F64, plan.causal), pos_e(tpmax, sd, bp, F32, plan.causal)
        rep.add("pos", k, stage_ratios(ee, e64, e32, D, True), lambda: worst_element(ee, e64))

        # ---- attention: every utterance on its own operands
        o64, o32, env, og = [], [], [], []
        for b in range(B):
            tb, tpb = si.live[b], si.tp[b]
            e_b = ee[tpmax - tpb:] if plan.causal else ee[tpmax - tpb: tpmax - tpb + 2 * tpb - bp.group_size]
            ops = [si.utt(z, b, True)[None] for z in (qu, kk, vv)]
            lb = torch.tensor([si.lens[b]])
            a, en = attention(*ops, e_b, lb, tb, sd, bp, F64, plan=plan)
            c, _ = attention(*ops, e_b, lb, tb, sd, bp, F32, round_p=True, plan=plan)
            o64.append(a[0]); o32.append(c[0]); env.append(en[0]); og.append(si.utt(att_o, b))
        o64, o32, env, og = (torch.cat(z) for z in (o64, o32, env, og))
        kmax = max(bp.dim_head, tpmax // bp.group_size)
        rep.add("attention", k, stage_ratios(og, o64, o32, kmax, True, share_factor=2.0), lambda: worst_element(og, o64))
        rep.elementwise("attention", k, "envelope", (og.double() - o64).abs(), 2.0 ** -7 * env + 2e-5, og, o64)

        # ---- out-projection: chain B's first GEMM / rs_gemm
        ao = att_o[si.xidx]
        r64, r32 = out_proj(xin, ao, sd, bp, F64), out_proj(xin, ao, sd, bp, F32)
        gm = x_mhsa[si.xidx]
        rep.add("outproj", k, stage_ratios(gm, r64, r32, D, False), lambda: worst_element(gm, r64))
        wo = "blocks.%d.multi_head_self_attention_module.mhsa.output_layer." % k
        w_, b_ = q(torch.from_numpy(np.asarray(sd[wo + "weight"])).double()), torch.from_numpy(np.asarray(sd[wo + "bias"])).double()
        cls = 2.0 * D * 2.0 ** -23 * (ao.double().abs() @ w_.abs().T + xin.double().abs() + b_.abs())
        rep.elementwise("outproj", k, "summation", (gm.double() - r64).abs(), cls + 1e-30, gm, r64)

        # ---- GLU: chain B / chain2 second half, rs_gemm GLU epilogue
        r64, r32 = glu(gm, sd, bp, F64, fin), f32_runs(lambda: glu(gm, sd, bp, F32, fin))
        gg = g_glu[si.xidx]
        fit, misfit = rel(gg, r64)[1], rel(gg, glu(gm, sd, bp, F64, not fin))[1]
        assert fit < misfit, (k, "GLU: expected the %s route" % ("folded-LayerNorm (chain B)" if fin else "per-module"), fit, misfit)
        rep.add("glu", k, stage_ratios(gg, r64, r32, D, True), lambda: "gpu %s, float32 runs %s; %s" % (_misses(gg, r64), [_misses(q(r), r64).split(" of")[0] for r in r32], worst_element(gg, r64)))

        # ---- depthwise convolution (dwconv_mfma_kernel / dwconv_kernel) and the residual branch around the module, per utterance
        d64, d32, dg, res64, res32 = [], [], [], [], []
        for b in range(B):
            gb = si.utt(g_glu, b)[None]
            d64.append(depthwise(gb, sd, bp, F64, plan.causal)[0]); d32.append([r[0] for r in f32_runs(lambda: depthwise(gb, sd, bp, F32, plan.causal))])
            dg.append(so.utt(g_dw, b))
            xb = si.utt(x_mhsa, b)[None]
            res64.append(conv_res(xb, sd, bp, F64)[0]); res32.append(conv_res(xb, sd, bp, F32)[0])
        d64, dg, res64, res32 = (torch.cat(z) for z in (d64, dg, res64, res32))
        d32 = [torch.cat([u[i] for u in d32]) for i in range(len(d32[0]))]
        assert d64.shape[0] == len(so.xidx)
        rep.add("dw", k, stage_ratios(dg, d64, d32, bp.kernel_size, True, share_factor=0.0), lambda: worst_element(dg, d64))
        rep.elementwise("dw", k, "ulp", (dg.double() - d64).abs(), 2.0 ** -8 * d64.abs() + 2e-5, dg, d64)
        miss = 1.0 - float((dg.double() == q(d64)).double().mean())
        rep.add("dw", k, {"miss/0.05": miss / 0.05}, lambda: "share of correctly rounded outputs %.4f" % (1.0 - miss))

        # ---- chain A: pointwise-2 + residual, FFN2, block LayerNorm, the next block's FFN1 (chain.hip tail / full / head, chain3.hip, rsgemm.hip FFN)
        nbp = plan.blocks[k + 1] if k + 1 < nb else None
        fnext = chained(nbp.dim_model) if nbp is not None else None
        dwv = g_dw[so.xidx]
        a64 = chain_a(res64, dwv, sd, bp, nbp, F64, fout, fnext)
        a32 = f32_runs(lambda: chain_a(res32, dwv, sd, bp, nbp, F32, fout, fnext))
        kch = max(bp.dim_ffn2, nbp.dim_ffn1 if nbp is not None else 0)
        targets = [("x_ffn1", "blocks.%d.x_ffn1" % (k + 1))] if nbp is not None else [("out", p + "out")]
        if not fout:
            targets += [("x_conv", p + "x_conv")] + ([("out", p + "out")] if nbp is not None else [])
        for tag, key in targets:
            gt = got[key]
            assert gt.shape[0] == so.rows, (key, gt.shape, so.rows)
            gt = gt[so.xidx]
            rep.add("chainA", k, stage_ratios(gt, a64[tag], [r[tag] for r in a32], kch, False), lambda gt=gt, tag=tag: tag + " " + worst_element(gt, a64[tag]))
    return rep
