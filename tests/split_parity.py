"""Test helper (no tests here): one traced forward of the split mode (precision = "split") against its float64 reference, stage by stage, teacher forced -
the checker both tests/test_gpu_split_stages.py (GPU traces, option trace_fused = 1 or the per-module route) and tests/test_ref_split_host.py (traces of
CPU stand-ins) run.  The reference is oracle/ref_bf16.py's stage functions with rnd = ident; the noise is oracle/ref_split.py's split_runs.  Row maps and
the report are tests/bf16_parity.py's.

Bounds (the project's factors, nothing else): rel(got, r64).max <= 4 x the worst noise run's, .mean <= 8 x the mean of the noise runs', neither below
sqrt(K) 2^-23 of the magnitude (ref_bf16.stage_ratios, float32 outputs).  Element-wise, on the out-projection, conv_res, the per-module pointwise-2 and the front Linear:
|got - r64| <= 2 K 2^-23 (|a| |w|^T + |x| + |b|) + ref_split.split_term(|a|, |w|, scale).  Attention, element-wise, with env_i = sum_j p_ij |v_j|: a score
error of at most ds_i in every score of row i moves every p_ij by a factor within exp(+-2 ds_i), so |got - r64| <= (2 ds_i + c_v) env_i with
ds_i = (2 (d + 1) 2^-23 + 2^-20 + 2^-22) max_j (|q + u| |k_j| + |q + v| |e_ij|) / sqrt(d) (float32 summation of the d + 1 products, the split term, the two
roundings of the scale multiply) and c_v = 2 Tg 2^-23 + 2^-20 + 8 2^-23 (P V summation, its split term, exp / sum / reciprocal).

Trace layout of the split mode (forward_exact.hip forward_exact, fused kernel family): ``q`` is Q + b WITHOUT u (the attention kernel adds u), q / k / v / att_o live in the
projections' row space (rectangular: b Tp + t; ragged: the group-padded stream rows) whose chunk-padding rows are never written and are ignored here;
``e`` is the float32 positional projection; ``conv_res`` exists on transition blocks, ``x_conv`` on the per-module route only, ``out`` wherever no head is merged into chain A's tail."""
import numpy as np
import torch

from bf16_parity import _Report, _Space
from oracle import ref_bf16 as Q
from oracle import ref_encoder as R
from oracle import ref_split as S
from oracle.ref_bf16 import ident, stage_ratios, worst_element
from oracle.ref_split import CHAIN_KINDS, FFN_KINDS, NO_KINDS, keep, split_runs, split_term

F64, F32 = torch.float64, torch.float32
SXC_WIDTHS = (24, 32, 48, 100, 120, 140, 144, 168, 176, 180, 200, 240, 256)      # sxf_chain.hip SXC_WIDTHS (held to it on the CPU: tests/test_routes_host.py)
EPS = 2.0 ** -23


def split_route(plan, opts):
    """What forward_exact (fused kernel family) chooses for these options: {"chain": the row-local chains (split_chain and split_ffn), "ffn": the FFN-only form of sxc_a_kernel where no chain runs,
    "sublin": sxf_sub.hip}.  A traced forward takes this route only with trace_fused = 1; otherwise chain = sublin = False."""
    fused = bool(opts.get("trace_fused", 0))
    ffn = bool(opts.get("split_ffn", 1))
    return {"chain": fused and bool(opts.get("split_chain", 1)) and ffn, "ffn": ffn,
            "sublin": fused and bool(opts.get("split_sublin", 1)) and plan.sub_layers == 1}


def _kinds(route, width):
    """(the products on the same-scale kernels, LayerNorm folded into the image) of a row-local stage at this width."""
    if width in SXC_WIDTHS and route["chain"]:
        return CHAIN_KINDS, True
    if width in SXC_WIDTHS and route["ffn"]:
        return FFN_KINDS, True          # the FFN-only form folds its LayerNorm; every other product: LayerNorm kernel + split.hip
    return NO_KINDS, False


def _t(sd, key):
    return torch.from_numpy(np.asarray(sd[key]))


def _lin_bound(a, w, x, b, k, sa, sw=S.SW):
    cls = 2.0 * k * EPS * (a.double().abs() @ w.double().abs().T + (x.double().abs() if x is not None else 0.0) + b.double().abs())
    return cls + split_term(a.abs(), w.abs(), sa, sw) + 1e-30


def check_split_front(got, plan, sd, mel, ln, tm, ragged, route, rep):
    """mel -> ``linear`` and block 0's first FFN.  sxf_sub.hip (route["sublin"]): one stage, ``subsample`` asserted absent.  Per-module route: ``subsample`` asserted
    present - the convolution(s) from the mel (fp32 VALU kernels: float32 noise) and the Linear from the traced activation, with the element-wise bound."""
    mel = torch.as_tensor(mel).float()
    B = len(ln)
    lens0 = [int(v) for v in ln]
    half = lambda v: (v - 1) // 2 + 1
    lens1, t1 = lens0, tm
    for _ in range(plan.sub_layers):
        lens1, t1 = [half(v) for v in lens1], half(t1)
    b0 = plan.blocks[0]
    sp = _Space(ragged, lens1, t1, b0.group_size)
    D0 = b0.dim_model
    K = plan.sub_filters[plan.sub_layers - 1] * (plan.n_mels >> plan.sub_layers)
    mlen = torch.as_tensor(lens0) if ragged else None
    lin = got["linear"]
    assert lin.shape == (sp.rows, D0), (lin.shape, sp.rows, D0)
    assert ("subsample" in got) == (not route["sublin"]), ("subsample", "expected to stay in registers" if route["sublin"] else "expected in the trace")
    own = lambda x: torch.cat([x[b, :sp.live[b]] for b in range(B)])
    gl = lin[sp.xidx]
    if route["sublin"]:
        fe = lambda dt, rnd, conv="fp32": own(Q.front_end(mel, mlen, sd, plan, dt, rnd, conv))
        r64 = fe(F64, ident)
        rep.add("front", 0, stage_ratios(gl, r64, split_runs(fe, frozenset(("linear",)), front=True), K, False), lambda: worst_element(gl, r64))
    else:
        sub = got["subsample"]
        assert sub.shape == (B * t1, K), (sub.shape, B, t1, K)          # the rectangular image, ragged batch or not
        sub = own(sub.reshape(B, t1, K))

        def conv(dt, rnd):
            tr = {}
            Q.front_end(mel, mlen, sd, plan, dt, rnd, trace=tr)
            return own(tr["subsample"])
        c64 = conv(F64, ident)
        rep.add("conv", 0, stage_ratios(sub, c64, split_runs(conv, NO_KINDS), 9 * (plan.sub_filters[0] if plan.sub_layers == 2 else 1), False), lambda: worst_element(sub, c64))
        fl = lambda dt, rnd: Q.front_linear(sub, sd, plan, dt, rnd)
        l64 = fl(F64, ident)
        rep.add("linear", 0, stage_ratios(gl, l64, split_runs(fl, NO_KINDS), K, False), lambda: worst_element(gl, l64))
        rep.elementwise("linear", 0, "summation", (gl.double() - l64).abs(), _lin_bound(sub, _t(sd, "linear.weight"), None, _t(sd, "linear.bias"), K, S.LO_SCALE, S.LO_SCALE), gl, l64)
    kinds, fold = _kinds(route, D0)
    g1 = got["blocks.0.x_ffn1"][sp.xidx]
    f1 = lambda dt, rnd: Q.ffn(gl, sd, "blocks.0.feed_forward_module1", dt, fold, rnd)
    f64 = f1(F64, ident)
    rep.add("ffn1", 0, stage_ratios(g1, f64, split_runs(f1, kinds), b0.dim_ffn1, False), lambda: worst_element(g1, f64))
    return rep


def check_split_trace(got, out_len, plan, sd, ln, tm, ragged, route, label, only=None):
    """Every stage of every block of one traced split forward (``got``: trace name -> float tensor (rows, columns)) against the float64 reference computed
    from the trace's own inputs of that stage.  Returns the _Report (``finish`` prints the worst statistic / bound of every stage and asserts).  ``only``: these blocks."""
    nb, B = len(plan.blocks), len(ln)
    rep = _Report(label)
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
        if only is not None and k not in only:
            continue
        p = "blocks.%d." % k
        pm = p + "multi_head_self_attention_module.mhsa."
        si, so = spaces[k], spaces[k + 1]
        D, De = bp.dim_model, bp.dim_expand
        kin = _kinds(route, D)[0]
        kout, fout = _kinds(route, De)
        chain_in, chain_out = kin is CHAIN_KINDS, kout is CHAIN_KINDS
        nbp = plan.blocks[k + 1] if k + 1 < nb else None
        merged = chain_out and nbp is not None and _kinds(route, nbp.dim_model)[0] is CHAIN_KINDS and nbp.dim_model == De
        # ---- the route, from the trace: x_conv leaves the registers only on the per-module route; ``out`` is absent exactly where the next block's head is merged
        assert ((p + "x_conv") in got) == (not chain_out), (k, "chain A tail expected" if chain_out else "per-module route expected")
        assert ((p + "out") in got) == (not merged), (k, "merged tail + head expected" if merged else "a block output expected in the trace")
        x_ffn1, x_mhsa, att_o, g_glu, g_dw, ee = (got[p + n] for n in ("x_ffn1", "x_mhsa", "att_o", "glu", "dw", "e"))
        qq, kk, vv = (got[p + n] for n in ("q", "k", "v"))
        assert x_ffn1.shape == (si.rows, D) and qq.shape == (si.qrows, D) and att_o.shape == (si.qrows, D) and g_dw.shape == (so.rows, De) and g_glu.shape == (si.rows, De), \
            (k, x_ffn1.shape, qq.shape, att_o.shape, g_dw.shape, g_glu.shape)
        u = _t(sd, pm + "u")

        # ---- Q / K / V (chain A head | LayerNorm + split.hip); the trace's q is without u
        xin = x_ffn1[si.xidx]
        fq = lambda dt, rnd: Q.qkv(xin, sd, bp, dt, chain_in, rnd)
        r64 = fq(F64, ident)
        runs = split_runs(fq, kin)
        for i, (nme, g) in enumerate(zip(("q", "k", "v"), (qq, kk, vv))):
            gv = g[si.qidx].double() + (u.double() if i == 0 else 0.0)
            rep.add("qkv", k, stage_ratios(gv, r64[i], [r[i] for r in runs], D, False), lambda gv=gv, i=i, nme=nme: nme + " " + worst_element(gv, r64[i]))

        # ---- positional projection (split.hip on the float32 sinusoid table of pack.hip build_pos_table)
        tpmax = max(si.tp)
        assert ee.shape == ((tpmax if plan.causal else 2 * tpmax - bp.group_size), D), (k, ee.shape)
        fe = lambda dt, rnd: Q.pos_e(tpmax, sd, bp, dt, plan.causal, rnd)
        e64 = fe(F64, ident)
        rep.add("pos", k, stage_ratios(ee, e64, split_runs(fe, NO_KINDS), D, False), lambda: worst_element(ee, e64))

        # ---- attention, every utterance on its own operands (pad rows by the contract: q + u = u, k = v = 0)
        o64, oruns, env, smax, og = [], [], [], [], []
        d = bp.group_size * D // bp.num_heads
        for b in range(B):
            tb, tpb = si.live[b], si.tp[b]
            e_b = ee[tpmax - tpb:] if plan.causal else ee[tpmax - tpb: tpmax - tpb + 2 * tpb - bp.group_size]
            qb, kb, vb = (z[si.q0[b]: si.q0[b] + tb][None] for z in (qq, kk, vv))
            lb = torch.tensor([si.lens[b]])

            def fa(dt, rnd, env_out=None):
                pair = (lambda z, sc: S.pair22(z, sc)) if rnd is keep else (lambda z, sc: z)
                ops = Q.pad_rows(pair(qb.to(dt) + u.to(dt), S.SQK), pair(kb.to(dt), S.SQK), pair(vb.to(dt), S.SV_), sd, bp, ident)
                o, en = Q.attention(*ops, pair(e_b.to(dt), S.SQK), lb, tb, sd, bp, dt, ident, plan=plan)
                if env_out is not None:
                    env_out.append(en[0])
                    a_ = [z.abs() for z in ops]
                    dvu = (_t(sd, pm + "v").double() - u.double()).abs()
                    sm = R.relpos_scores(a_[0], a_[0] + dvu, a_[1], e_b.double().abs(), None, tpb, bp.num_heads, bp.group_size, causal=plan.causal).amax(-1)      # (1, H, Tg)
                    sm = sm[..., None].expand(1, bp.num_heads, tpb // bp.group_size, d).transpose(1, 2).reshape(1, tpb, D)[0, :tb]
                    smax.append(sm)
                return o[0]
            o64.append(fa(F64, ident, env))
            oruns.append(split_runs(fa, NO_KINDS))
            og.append(att_o[si.q0[b]: si.q0[b] + tb])
        o64, env, smax, og = (torch.cat(z) for z in (o64, env, smax, og))
        oruns = [torch.cat([r[i] for r in oruns]) for i in range(len(oruns[0]))]
        tg = tpmax // bp.group_size
        rep.add("attention", k, stage_ratios(og, o64, oruns, max(d, tg), False), lambda: worst_element(og, o64))
        ds = (2.0 * (d + 1) * EPS + 2.0 ** -20 + 2.0 ** -22) * smax
        rep.elementwise("attention", k, "envelope", (og.double() - o64).abs(), (2.0 * ds + 2.0 * tg * EPS + 2.0 ** -20 + 8.0 * EPS) * env + 1e-30, og, o64)

        # ---- out-projection (chain B | split.hip with the residual epilogue)
        ao = att_o[si.qidx]
        fo = lambda dt, rnd: Q.out_proj(xin, ao, sd, bp, dt, rnd)
        r64 = fo(F64, ident)
        gm = x_mhsa[si.xidx]
        rep.add("outproj", k, stage_ratios(gm, r64, split_runs(fo, kin), D, False), lambda: worst_element(gm, r64))
        wo = pm + "output_layer."
        rep.elementwise("outproj", k, "summation", (gm.double() - r64).abs(),
                        _lin_bound(ao, _t(sd, wo + "weight"), xin, _t(sd, wo + "bias"), D, S.SR if chain_in else S.LO_SCALE, S.SW if chain_in else S.LO_SCALE), gm, r64)

        # ---- GLU (chain B | LayerNorm + split.hip + sxf_glu_kernel)
        fg = lambda dt, rnd: Q.glu(gm, sd, bp, dt, chain_in, rnd)
        r64 = fg(F64, ident)
        gg = g_glu[si.xidx]
        rep.add("glu", k, stage_ratios(gg, r64, split_runs(fg, kin), D, False), lambda: worst_element(gg, r64))

        # ---- depthwise convolution (sxf_dwconv_kernel, fp32) and the residual branch, per utterance
        d64, druns, dg, xm_utts = [], [], [], []
        for b in range(B):
            gb = si.utt(g_glu, b)[None]
            fd = lambda dt, rnd: Q.depthwise(gb, sd, bp, dt, plan.causal, rnd)[0]
            d64.append(fd(F64, ident)); druns.append(split_runs(fd, NO_KINDS)); dg.append(so.utt(g_dw, b))
            xm_utts.append(si.utt(x_mhsa, b)[None])
        d64, dg = torch.cat(d64), torch.cat(dg)
        druns = [torch.cat([r[i] for r in druns]) for i in range(len(druns[0]))]
        assert d64.shape[0] == len(so.xidx)
        rep.add("dw", k, stage_ratios(dg, d64, druns, bp.kernel_size, False), lambda: worst_element(dg, d64))

        # ---- conv_res of transition blocks (split.hip on the decimated rows): its own trace entry, element-wise bound included; elsewhere the rows themselves
        xs = torch.cat([xb[0, ::bp.conv_stride] for xb in xm_utts])
        if bp.transition:
            fr = lambda dt, rnd: torch.cat([Q.conv_res(xb, sd, bp, dt, rnd)[0] for xb in xm_utts])
            r64 = fr(F64, ident)
            res = got[p + "conv_res"]
            assert res.shape == (so.rows, De), (k, res.shape)
            res = res[so.xidx]
            rep.add("conv_res", k, stage_ratios(res, r64, split_runs(fr, NO_KINDS), D, False), lambda: worst_element(res, r64))
            m = "blocks.%d.conv_res.1." % k
            rep.elementwise("conv_res", k, "summation", (res.double() - r64).abs(), _lin_bound(xs, _t(sd, m + "weight")[:, :, 0], None, _t(sd, m + "bias"), D, S.LO_SCALE, S.LO_SCALE), res, r64)
        else:
            assert (p + "conv_res") not in got
            res = xs
        # ---- chain A from the traced residual rows and dw: x_conv (per-module route), out (no merged head), the next block's x_ffn1 (merged head)
        dwv = g_dw[so.xidx]
        kch = max(bp.dim_ffn2, nbp.dim_ffn1 if (nbp is not None and merged) else 0)
        fold_next = _kinds(route, nbp.dim_model)[1] if nbp is not None else None
        fc = lambda dt, rnd: Q.chain_a(res, dwv, sd, bp, nbp if merged else None, dt, fout, fold_next, rnd)
        a64 = fc(F64, ident)
        aruns = split_runs(fc, kout)
        targets = [("x_ffn1", "blocks.%d.x_ffn1" % (k + 1))] if merged else [("out", p + "out")]
        if not chain_out:
            targets = [("x_conv", p + "x_conv")] + targets
        for tag, key in targets:
            gt = got[key]
            assert gt.shape == (so.rows, De), (key, gt.shape, so.rows)
            gt = gt[so.xidx]
            rep.add("chainA", k, stage_ratios(gt, a64[tag], [r[tag] for r in aruns], De if tag == "x_conv" else kch, False), lambda gt=gt, tag=tag: tag + " " + worst_element(gt, a64[tag]))
        if not chain_out:       # x_conv = res + dw Wp2^T + b on split.hip: element-wise
            gt = got[p + "x_conv"][so.xidx]
            c = p + "convolution_module.layers.7."
            rep.elementwise("pw2", k, "summation", (gt.double() - a64["x_conv"]).abs(), _lin_bound(dwv, _t(sd, c + "weight")[:, :, 0], res, _t(sd, c + "bias"), De, S.LO_SCALE, S.LO_SCALE), gt, a64["x_conv"])
        if not merged and nbp is not None:      # the next block's head is its own launch on the traced block output
            sn = spaces[k + 1]
            xo = got[p + "out"][so.xidx]
            kn, fn_ = _kinds(route, nbp.dim_model)
            f1 = lambda dt, rnd: Q.ffn(xo, sd, "blocks.%d.feed_forward_module1" % (k + 1), dt, fn_, rnd)
            f64 = f1(F64, ident)
            g1 = got["blocks.%d.x_ffn1" % (k + 1)][sn.xidx]
            rep.add("ffn1", k + 1, stage_ratios(g1, f64, split_runs(f1, kn), nbp.dim_ffn1, False), lambda g1=g1, f64=f64: worst_element(g1, f64))
    return rep
