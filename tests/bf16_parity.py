"""Test helper (no tests here): one traced forward of the bf16 path against oracle/ref_bf16.py, stage by stage - the row maps of rectangular and
ragged batches, the report of statistic / bound ratios and the checker both tests/test_gpu_bf16_rounding.py (GPU traces) and
tests/test_ref_bf16_host.py (traces made on the CPU) run."""
import numpy as np
import torch

from oracle import ref_bf16 as Q
from oracle.ref_bf16 import (attention, chain_a, conv_res, depthwise, f32_runs, ffn, glu, out_proj, pos_e, q, qkv, rel, stage_ratios, worst_element)

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


def chain_route(fuse, width):
    """The fused chains serve this stage width (encoder_state.h: chain_max_dim = 256; chain.hip chain_supported) and are on (option fuse_chain)."""
    return bool(fuse) and width % 4 == 0 and 16 <= width <= 256


def front_route(plan, opts, ragged):
    """What run_subsample_linear / the ragged branch of forward_core (forward_bf16.hip) choose for this configuration and these options:
    {"conv": "fp32" | "split" - the convolution's form, "subsample": the activation is in the trace (separate kernels write it), "fuse_chain": the option}."""
    fuse, auto = opts.get("fuse_subsample", 2), opts.get("sub3_auto", 1)
    C0, D0, F = plan.sub_filters[0], plan.blocks[0].dim_model, plan.n_mels
    route = {"fuse_chain": opts.get("fuse_chain", 1)}
    if plan.sub_layers == 2:                                                  # conv2.hip + gemm.hip; the ragged form runs on the rectangle and gathers
        return dict(route, conv="fp32", subsample=True)
    sub3 = D0 % 4 == 0 and D0 <= 384 and (fuse == 3 or (fuse == 2 and auto and (C0 > 128 or D0 > 128)))          # use_sublinear3, sub_chunked_tiles
    sub2 = fuse >= 2 and F == 80 and D0 % 4 == 0 and ((C0 <= 128 and D0 <= 128) or (C0 <= 192 and D0 <= 192))      # sublinear2_groups
    if sub3 or sub2:
        return dict(route, conv="split", subsample=False)
    sub1 = fuse >= 1 and F == 80 and D0 <= 256 and not ragged                 # sublinear_fused_supported; ragged batches: conv.hip writes the ragged rows
    return dict(route, conv="fp32", subsample=not sub1)


def _bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """The distance between neighbouring bf16 numbers at |x| (8 significant bits; never below the smallest normal's)."""
    _, e = torch.frexp(x.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 8)


def check_front(got, plan, sd, mel, ln, tm, ragged, route, rep):
    """The front end and block 0's first FFN of one traced forward against oracle/ref_bf16.py, into the _Report ``rep`` (block number 0).
    mel (B, n_mels, tm) float32 as the GPU got it, ``ln`` the mel lengths; ``route``: what front_route expects - asserted.
    Where separate kernels write the activation (``subsample`` in the trace), every stage from its own traced input: ``conv`` - layer 1 from the mel
    (K = 9; the two-layer subsampler's layer-1 image is the trace entry ``subsample1``) - and ``conv2`` - layer 2 from that image (K = 9 C) - with
    stage_ratios (bf16 output: the share of correctly rounded outputs included) and the element-wise bound one bf16 ulp of r64 +
    2 K 2^-23 (sum |w| |p| + |b|) 1.1 (float32 summation through the Swish, whose slope is at most 1.1); ``linear`` from the traced activation with the
    out-projection's element-wise summation bound.  Fused routes: one stage mel -> ``linear`` (stage ``front``).  Then ``ffn1_0``: blocks.0.x_ffn1 from the
    traced ``linear``.  Rectangular batches count every frame of the rectangle; ragged batches every utterance's own frames, the reference padding the time
    axis at the utterance's own length.  Excluded: the group-padding rows of the ragged row space (counted against the lengths; finite in ``linear``, zero in
    ``subsample``) and, in the two-layer subsampler's rectangular images of a ragged batch, the frames behind an utterance's own (layer 1: asserted zero)."""
    mel = torch.as_tensor(mel).float()
    B = len(ln)
    lens0 = [int(v) for v in ln]
    lens1, t1 = lens0, tm
    half = lambda v: (v - 1) // 2 + 1
    for _ in range(plan.sub_layers):
        lens1, t1 = [half(v) for v in lens1], half(t1)
    b0 = plan.blocks[0]
    sp = _Space(ragged, lens1, t1, b0.group_size)
    D0 = b0.dim_model
    K = plan.sub_filters[plan.sub_layers - 1] * (plan.n_mels >> plan.sub_layers)
    mlen = torch.as_tensor(lens0) if ragged else None
    lin = got["linear"]
    assert lin.shape == (sp.rows, D0), (lin.shape, sp.rows, D0)
    npad = sp.rows - len(sp.xidx)
    assert npad == (sum(_up(v, b0.group_size) - v for v in lens1) if ragged else 0)
    pad_rows = torch.ones(sp.rows, dtype=torch.bool)
    pad_rows[sp.xidx] = False
    assert int(pad_rows.sum()) == npad and bool(torch.isfinite(lin[pad_rows]).all()), "group-padding rows of ``linear``: count / not finite"
    assert ("subsample" in got) == bool(route["subsample"]), ("subsample", "expected in the trace" if route["subsample"] else "expected to stay in registers", route)
    assert ("subsample1" in got) == (plan.sub_layers == 2), "the two-layer subsampler's layer-1 image"

    def own(x, live=None):      # (B, T, columns) -> the valid frames' rows, utterance after utterance
        live = sp.live if live is None else live
        return torch.cat([x[b, :live[b]] for b in range(B)])

    def conv_stage(stage, gv, fn, kc, wabs, babs, xabs, rows):
        """One convolution with a bf16 output: gv the GPU's rows, fn(dtype) the reference's rows before the rounding; |w|, |b|, |input| and the map image -> rows for the bound."""
        c64, c32 = fn(F64), f32_runs(lambda: fn(F32))
        rep.add(stage, 0, stage_ratios(gv, c64, c32, kc, True), lambda: "gpu %s, float32 runs %s; %s" % (_misses(gv, c64), [_misses(q(r), c64).split(" of")[0] for r in c32], worst_element(gv, c64)))
        bound = _bf16_ulp(c64) + 2.0 * kc * 2.0 ** -23 * 1.1 * rows(torch.nn.functional.conv2d(xabs, wabs, babs, stride=2, padding=1))
        rep.elementwise(stage, 0, "ulp+sum", (gv.double() - c64).abs(), bound, gv, c64)

    gl = lin[sp.xidx]
    if route["subsample"]:
        sub = got["subsample"]
        w, sc, bias = Q.bn_fold2d(sd, 0, F32)
        w9 = (w * sc[:, None, None, None]).double()
        mel_own = Q.mask_time(mel, mlen)
        if plan.sub_layers == 1:
            assert sub.shape == (sp.rows, K), (sub.shape, sp.rows, K)          # the Linear's rows: rectangular, or the ragged row space (conv.hip writes it)
            assert float(sub[pad_rows].abs().sum()) == 0.0, "group-padding rows of ``subsample`` are not zero"
            sub = sub[sp.xidx]
            rows = lambda x: own(Q.feature_rows(x))
            conv_stage("conv", sub, lambda dt: rows(Q.front_conv(mel, mlen, sd, plan, dt)), 9, w9.abs(), bias.double().abs(), mel_own.double().abs().unsqueeze(1), rows)
        else:
            c0, c1, f1 = plan.sub_filters[0], plan.sub_filters[1], plan.n_mels // 2
            tl1, live1 = half(tm), ([half(v) for v in lens0] if ragged else [half(tm)] * B)
            t1r = half(tl1)                                                    # both images are rectangular, ragged batch or not (forward_core gathers the Linear's rows)
            img = got["subsample1"]
            assert img.shape == (B * f1 * tl1, c0) and sub.shape == (B * t1r, K), (img.shape, sub.shape)
            img = img.reshape(B, f1, tl1, c0).permute(0, 3, 1, 2)              # conv2.hip subsample_conv_cl_kernel: rows (b, f, t), channel-last
            assert float(Q.mask_time(img, live1).sub(img).abs().sum()) == 0.0, "layer-1 image behind an utterance's own frames is not zero"
            rows = lambda x: own(Q.feature_rows(x), live1)
            conv_stage("conv", rows(img), lambda dt: rows(Q.front_conv(mel, mlen, sd, plan, dt)), 9, w9.abs(), bias.double().abs(), mel_own.double().abs().unsqueeze(1), rows)
            sub = sub.reshape(B, t1r, K // c1, c1).transpose(2, 3).reshape(B, t1r, K)        # conv2_igemm_kernel writes (f2, c); the reference's order is c * F2 + f2
            sub = own(sub)
            w2, sc2, bias2 = Q.bn_fold2d(sd, 1, F32)
            rows = lambda x: own(Q.feature_rows(x))
            conv_stage("conv2", sub, lambda dt: rows(Q.front_conv2(img, sd, plan, dt)), 9 * c0, q(w2 * sc2[:, None, None, None]).double().abs(), bias2.double().abs(), img.double().abs(), rows)
        l64, l32 = Q.front_linear(sub, sd, plan, F64), Q.front_linear(sub, sd, plan, F32)
        rep.add("linear", 0, stage_ratios(gl, l64, l32, K, False), lambda: worst_element(gl, l64))
        w_, b_ = q(torch.from_numpy(np.asarray(sd["linear.weight"])).double()), torch.from_numpy(np.asarray(sd["linear.bias"])).double()
        cls = 2.0 * K * 2.0 ** -23 * (sub.double().abs() @ w_.abs().T + b_.abs())
        rep.elementwise("linear", 0, "summation", (gl.double() - l64).abs(), cls + 1e-30, gl, l64)
    else:
        fe = lambda dt, cv: own(Q.front_end(mel, mlen, sd, plan, dt, conv=cv))
        r64 = fe(F64, "fp32")
        runs = {"fp32": f32_runs(lambda: fe(F32, "fp32"))}
        if route["conv"] == "split":
            runs["split"] = f32_runs(lambda: fe(F32, "split"))
        pool = [r for v in runs.values() for r in v]
        rep.add("front", 0, stage_ratios(gl, r64, pool, K, False), lambda: worst_element(gl, r64))
        if plan.sub_layers == 1:
            # the convolution's form leaves no trace entry: asserted through the data - the other form's float32 run must fit the GPU's numbers worse
            if "split" not in runs:
                runs["split"] = [fe(F32, "split")]
            other = "fp32" if route["conv"] == "split" else "split"
            fit, misfit = rel(gl, runs[route["conv"]][0])[1], rel(gl, runs[other][0])[1]
            rep.form = (fit, misfit)
            if not fit < misfit:
                rep.fails.append("block 0 front route: expected the %s convolution, mean distance to its float32 run %.3g, to the other form's %.3g" % (route["conv"], fit, misfit))

    # ---- block 0's first FFN: the chain head (chain.hip) / rs_gemm FFN on the front end's output
    fold = chain_route(route["fuse_chain"], D0)
    x1 = got["blocks.0.x_ffn1"]
    assert x1.shape[0] == sp.rows, (x1.shape, sp.rows)
    g1 = x1[sp.xidx]
    pf = "blocks.0.feed_forward_module1"
    f64, f32 = ffn(gl, sd, pf, F64, fold), f32_runs(lambda: ffn(gl, sd, pf, F32, fold))
    rep.add("ffn1_0", 0, stage_ratios(g1, f64, f32, b0.dim_ffn1, False), lambda: worst_element(g1, f64))
    return rep


def check_trace(got, out_len, plan, sd, ln, tm, ragged, fuse, label):
    """Every stage of every block of one traced forward (``got``: trace name -> float tensor of (rows, columns)) against the reference computed
    from the trace's own inputs of that stage.  Returns the _Report (``finish`` prints the worst ratios and asserts).  ``fuse``: the fused chains
    are on (option fuse_chain), so the widths they support take the folded-LayerNorm route."""
    nb, B = len(plan.blocks), len(ln)
    chained = lambda width: chain_route(fuse, width)
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

        # ---- positional rows E (gemm.hip on the table of pack.hip build_pos_table); the table's own float32 angles are part of the noise model
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
