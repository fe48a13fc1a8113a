// Which kernel every step of a forward runs - the bf16 schedule, and in its last section the label-exact split schedule: pure functions of the handle after packing (options and "image exists" pointers) and of the two batch
// properties that matter (ragged, streaming).  The ONE place that decides: forward_bf16.hip's schedule and per-module entries, its workspace layout,
// pack.hip's "which images to build" and forward_exact.hip's schedule read these and hold no predicate of their own.  Host only, no HIP call; nothing here is cached on the handle - a forward
// computes its routes on entry (a handful of integer compares per block), so an option set between two forwards needs no invalidation.
#pragma once
#include "encoder_state.h"

#include <algorithm>
#include <string>

// Widths 257 .. 384 (EfficientConformer Large stage 1, Medium stage 3) fit the row-stationary kernels, but at 24 k-steps those run one
// wave per SIMD and stream every weight per 32-row tile: 60 - 200 TFLOP/s (profiles/r2_03_large_kernel_stats.txt).  `wide_gemm` 2 / 3
// sends these layers to LayerNorm + the tiled GEMMs instead, and so does `tiled_auto` for configurations whose widest stage lies there (tiled_auto_on).
// Never chosen by row count: it was -3 % kernel time on Large and wall-neutral, and it made a forward's bits depend on how the batch is split into row ranges
// (the two paths round differently; tools/robustness_sweep.py) - the gemm.hip / gemm256.hip choice does not (bit-identical kernels).
inline bool prefer_tiled(const EcEncoder* e, int K) {
    const bool on = e->wide_gemm == 2 || e->wide_gemm == 3 || (e->wide_gemm == 0 && (e->tiled_auto == 2 || (e->tiled_auto && e->tiled_auto_on)));
    return on && K > e->tiled_min_k && K % 8 == 0;
}

// Option tiled_auto's outcome for a configuration (EcEncoder::tiled_auto_on, set by finalize): its widest stage lies in (tiled_min_k, 384].  A property of
// the configuration, never of the batch: one path per handle
inline bool tiled_auto_rule(const EcEncoder* e) {
    int dmax = 0;
    for (const EcBlock& b : e->blocks) dmax = std::max(dmax, std::max(b.dim_model, b.dim_expand));
    return dmax > e->tiled_min_k && dmax <= 384;
}

// ------------------------------------------------------------------ front end: Conv2dSubsampling + transpose + Linear
enum FrontRoute {
    FRONT_TWO_LAYER,   // conv.hip layer 1 + conv2.hip implicit GEMM + tiled Linear (the plain Conformer configurations); ragged: on the rectangle, then a row gather
    FRONT_CHUNKED,     // sublinear3.hip: workgroup = (utterance, 128 frames); any channel count, widths up to 384
    FRONT_ROW_STAT,    // sublinear2.hip: F = 80, channels and width <= 192; indexes ragged rows itself
    FRONT_TILED_FUSED, // sublinear.hip: F = 80, width <= 256; rectangular batches only
    FRONT_CONV_GEMM    // conv.hip + tiled Linear: the conv writes ragged rows itself.  The only one-layer route whose "subsample" activation exists (debug trace)
};
// Precedence (option fuse_subsample; every test of an image = "packed for this shape"):
//   two subsampling layers                                                    -> two-layer, whatever the option says
//   3, or 2 with sub3_auto on a front end wider than 128 channels / columns   -> chunked, where its image exists (widths <= 384, multiples of 4)
//   2 or 3                                                                    -> row-stationary, where its image exists (3 on a width the chunked kernel does not build lands here)
//   1, 2 or 3 on a rectangular batch                                          -> tiled-fused, where its image exists
//   everything else (0; 1 on a ragged batch; no fused kernel for the shape)   -> conv + GEMM
// A debug trace changes nothing: "subsample" is recorded where a route writes it.
inline FrontRoute front_route(const EcEncoder* e, bool ragged) {
    if (e->cfg.sub_layers == 2) return FRONT_TWO_LAYER;
    const bool wide = e->cfg.sub_filters[0] > 128 || e->blocks[0].dim_model > 128;
    if (e->sub3.wimg && (e->fuse_subsample == 3 || (e->fuse_subsample == 2 && e->sub3_auto && wide))) return FRONT_CHUNKED;
    if (e->fuse_subsample >= 2 && e->lin_rs) return FRONT_ROW_STAT;
    if (!ragged && e->fuse_subsample && e->lin_fused) return FRONT_TILED_FUSED;
    return FRONT_CONV_GEMM;
}

// Scratch of the front end in bytes (0 = not needed), for `batch` utterances of `t1` frames after the subsampling at a mel pitch of `tm` frames:
//   sub   bf16 output rows of the subsampler, C x F columns: the two unfused routes.  Ragged: every utterance's frames rounded up to the first block's group
//         size.  Rectangular batches reserve it whatever the route (their workspace size predates the fused routes and is kept)
//   sub1  the two-layer subsampler's channel-last layer-1 image [B][F/2][frames after layer 1][Cp]
//   xrect ragged two-layer route: the rectangular Linear output before the gather (the ragged conv + GEMM route writes ragged rows directly)
struct FrontScratch { size_t sub = 0, sub1 = 0, xrect = 0; };
inline FrontScratch front_scratch(const EcEncoder* e, bool ragged, size_t batch, size_t tm, size_t t1) {
    const EcConfig& c = e->cfg;
    const FrontRoute r = front_route(e, ragged);
    FrontScratch n;
    if (!ragged || r == FRONT_TWO_LAYER || r == FRONT_CONV_GEMM) {
        const size_t rows = batch * (t1 + (ragged ? e->blocks[0].group_size - 1 : 0));
        n.sub = rows * c.sub_filters[c.sub_layers - 1] * (c.n_mels >> c.sub_layers) * 2;
    }
    if (r == FRONT_TWO_LAYER) {
        n.sub1 = batch * (c.n_mels / 2) * ((tm - 1) / 2 + 1) * ec_round_up(c.sub_filters[0], 64) * 2;
        if (ragged) n.xrect = batch * t1 * e->blocks[0].dim_model * 4;
    }
    return n;
}

// ------------------------------------------------------------------ row-local work of a block
// A single GEMM of K inputs on rsgemm.hip (true) or on the tiled kernels (false).  resident_n > 0: a residual / fp32 epilogue, which keeps the whole output
// row of resident_n columns in registers
inline bool gemm_row_stat(const EcEncoder* e, int K, int resident_n = 0) {
    return (resident_n ? rs_gemm_resident_supported(K, resident_n) : rs_gemm_supported(K)) && !prefer_tiled(e, K);
}
// A feed-forward module of width D in a forward: the fused kernel of rsgemm.hip, or two tiled GEMMs
inline bool ffn_fused(const EcEncoder* e, int D) { return ffn_fused_supported(D) && !prefer_tiled(e, D); }
// effconf_ffn, NOT the forward's rule: the fused kernel (pre-norm in its prologue) wherever the width allows, also where ffn_fused sends a forward to the tiled GEMMs
inline bool ffn_fused_module(int D) { return ffn_fused_supported(D); }

// Chain launches of width D that go to chain2.hip / chain3.hip (launch_chain's rule)
inline bool chain_pair_on(const EcEncoder* e, int D) { return e->chain_pair && chain3_supported(D); }
// Block k's tail chain and block k + 1's head as ONE kernel (CHAIN_A_FULL), as far as shapes and chain-packed weights decide: chain.hip up to width
// chain_full_max, the chain3.hip instance (pair: padded width 256) whatever chain_full_max says
inline bool chain_full_fits(const EcEncoder* e, size_t k, bool pair) {
    const int De = e->blocks[k].dim_expand;
    return k + 1 < e->blocks.size() && e->bw[k].chain_out && chain_tail_supported(De) && e->bw[k + 1].chain_in && e->blocks[k + 1].dim_model == De &&
           chain_full_supported(De, pair ? 256 : e->chain_full_max);
}

enum HeadRoute { HEAD_PREV_TAIL, HEAD_CHAIN, HEAD_MODULES };   // FFN1 + Q/K/V: inside the previous block's tail chain / CHAIN_A_HEAD / per-module kernels
enum TailRoute { TAIL_FULL, TAIL_ONLY, TAIL_MODULES };         // pointwise-2 + FFN2 + block norm: with the next block's head (CHAIN_A_FULL) / CHAIN_A_TAIL / per-module kernels
struct BlockRoutes {
    HeadRoute head;
    bool ffn1_fused;   // HEAD_MODULES: FFN1 on the fused kernel, else two tiled GEMMs (its pre-norm is a LayerNorm launch either way)
    bool qkv_rs;       // HEAD_MODULES: Q/K/V row-stationary with the LayerNorm in its prologue, else LayerNorm + tiled
    bool chain_b;      // out-projection + LayerNorm + pointwise-1 / GLU as CHAIN_B, else per-module kernels:
    bool outp_rs;      //   out-projection row-stationary, else tiled
    bool pw1_rs;       //   pointwise-1 row-stationary with the LayerNorm in its prologue, else LayerNorm + tiled
    bool dw_mfma;      // depthwise convolution on the matrix pipe where the block has a tap table (option dwconv_mfma)
    bool res_rs;       // conv_res (expanding blocks) row-stationary, else tiled
    TailRoute tail;
    bool pw2_rs;       // TAIL_MODULES (and effconf_conv_module): pointwise-2 row-stationary, else tiled
    bool ffn2_fused;   // TAIL_MODULES: FFN2 on the fused kernel with the LayerNorm in its prologue, else LayerNorm + two tiled GEMMs
};

// ------------------------------------------------------------------ self-conditioned CTC step after block k (effconf_encoder_set_interctc)
// The step rewrites the block's output rows before the next block reads them, so a block followed by one never takes the next block's head along (TAIL_FULL ->
// TAIL_ONLY below, in both schedules), and its block-final LayerNorm must not pre-compute the next block's FFN1 operand from the pre-step rows (interctc_after)
inline bool interctc_after(const EcEncoder* e, size_t k) { return e->ic_index(k) >= 0; }
// bf16 schedule: the fused kernel of interctc.hip, or no kernel (finalize refuses the handle with interctc_refusal's text).  A function of the configuration only,
// never of the row count - as prefer_tiled above
enum InterCtcRoute { IC_FUSED, IC_REFUSED };
inline InterCtcRoute interctc_route(const EcEncoder* e, size_t k) { return interctc_supported(e->blocks[k].dim_expand, e->ic_vocab) ? IC_FUSED : IC_REFUSED; }
inline std::string interctc_refusal(const EcEncoder* e, size_t k) {
    return "InterCTC step after block " + std::to_string(k) + " (dim_expand " + std::to_string(e->blocks[k].dim_expand) + ", vocab_size " + std::to_string(e->ic_vocab) +
           "): the fused kernel takes dim_expand % 4 == 0, dim_expand <= 768 and 2 <= vocab_size <= 1024";
}

inline TailRoute tail_route(const EcEncoder* e, size_t k) {
    const int De = e->blocks[k].dim_expand;
    if (!(e->fuse_chain && e->bw[k].chain_out && chain_tail_supported(De) && De <= e->chain_max_dim)) return TAIL_MODULES;
    // cc_full: pack.hip built the constant block (chain_full_fits under ITS pair rule); k + 1's width = De <= chain_max_dim
    return e->bw[k].cc_full && chain_full_fits(e, k, chain_pair_on(e, De)) && !interctc_after(e, k) ? TAIL_FULL : TAIL_ONLY;
}

inline BlockRoutes block_routes(const EcEncoder* e, size_t k) {
    const EcBlock& b = e->blocks[k];
    const int D = b.dim_model, De = b.dim_expand;
    const bool chain_d = e->fuse_chain && e->bw[k].chain_in && D <= e->chain_max_dim;      // the D-wide chains: weights packed, option on, width in range
    BlockRoutes r;
    r.head = k > 0 && tail_route(e, k - 1) == TAIL_FULL ? HEAD_PREV_TAIL : (chain_d && chain_head_supported(D) ? HEAD_CHAIN : HEAD_MODULES);
    r.ffn1_fused = ffn_fused(e, D);
    r.qkv_rs = gemm_row_stat(e, D);
    r.chain_b = chain_d;
    r.outp_rs = gemm_row_stat(e, D, D);
    r.pw1_rs = gemm_row_stat(e, D);
    r.dw_mfma = e->dwconv_mfma == 2 || (e->dwconv_mfma == 1 && b.kernel_size == 15);
    r.res_rs = gemm_row_stat(e, D, De);
    r.tail = tail_route(e, k);
    r.pw2_rs = gemm_row_stat(e, De, De);
    r.ffn2_fused = ffn_fused(e, De);
    return r;
}

// ------------------------------------------------------------------ attention
// waves 0: attention.hip; 1 / 2: that variant of attention2.hip (padded head width dpad <= 160); refusal: no kernel takes this forward - the error text
struct AttentionRoute { int waves; const char* refusal; };
inline AttentionRoute attention_route(const EcEncoder* e, int dpad, bool ragged, bool streaming) {
    const bool v2 = relpos_attention2_supported(dpad);
    if (streaming && !(v2 && e->attention_v2))
        return {0, "streaming contexts / causal attention run on attention2.hip (padded head width <= 160, option attention_v2 != 0)"};
    if (ragged && !v2) return {0, "ragged batches need attention2.hip (padded head width <= 160)"};
    if (ragged || streaming) return {1, nullptr};
    return {v2 ? e->attention_v2 : 0, nullptr};
}

// ------------------------------------------------------------------ label-exact split schedule (forward_exact.hip; fp32 mode = its per-module family)
// Split mode with every block on widths the fused kernels take (sxf.hip attention at the head width, 16-byte rows): the sxf_* family can run at all.
// encoder.hip's ragged and streaming entries refuse a label-exact forward without it
inline bool split_fused_ok(const EcEncoder* e) {
    if (!e->exact_split) return false;
    for (const EcBlock& b : e->blocks)
        if (!sxf_attention_supported(b.group_size * b.dim_model / b.num_heads) || b.dim_model % 4 || b.dim_expand % 4) return false;
    return true;
}

// Per forward.  traced: a debug trace is recorded (it wants the intermediate states the fused kernels keep in registers, unless option trace_fused keeps the
// forward as it runs untraced); maps: attention maps were requested (a by-product of the scores in memory: per-module attention only)
struct ExactForwardRoutes {
    bool fused;            // kernel family: sxf*.hip (ragged batches, causal kernels, the E cache) | per-module exact.hip / split.hip
    bool sublin;           // Conv2dSubsampling + Linear as sxf_sub.hip, else conv kernel(s) + GEMM [+ row gather]
    bool ffn;              // a stand-alone FeedForwardModule as the FFN-only form of sxc_a_kernel where its image exists (option split_ffn), else LayerNorm + two GEMMs
    bool chains;           // the row-local chains of sxf_chain.hip where their images exist (options split_chain and split_ffn: the chains contain the modules)
    const char* refusal;   // no kernel takes this forward: the error text
};
inline ExactForwardRoutes exact_forward_routes(const EcEncoder* e, bool traced, bool maps) {
    const bool tr_modules = traced && !e->trace_fused;
    ExactForwardRoutes f;
    f.fused = split_fused_ok(e) && !maps;
    f.sublin = f.fused && e->split_sublin && e->xsub.wimg && e->cfg.sub_layers == 1 && !tr_modules;
    f.ffn = f.fused && e->split_ffn;
    f.chains = f.ffn && e->split_chain && !tr_modules;
    // finite left / right contexts: the band mask is part of every label-exact attention kernel; `causal` (causal relative tables, causal depthwise
    // padding: attentions.py:506, 1243-1247; layers.py:97-101) exists in the fused family only
    f.refusal = !f.fused && e->cfg.causal ? "the label-exact modes have no causal kernels (causal relative tables / depthwise pre-padding): bf16 path only" : nullptr;
    return f;
}

// Per block, the row-local work as in BlockRoutes.  rows_carry: block k + 1 reads exactly the rows block k writes (Min[k + 1] == Mout[k]) - a shape fact the
// caller knows; without it a tail cannot take the next head along
struct ExactBlockRoutes {
    HeadRoute head;        // FFN1 + Q/K/V: in the previous block's chain A / chain A's head form / per-module kernels
    bool ffn1_fused;       // HEAD_MODULES: FFN1 on the FFN-only form, else LayerNorm + two GEMMs
    bool chain_b;          // out-projection + LayerNorm + pointwise-1 / GLU as sxc_b_kernel, else per-module kernels
    TailRoute tail;        // pointwise-2 + FFN2 + block norm: chain A with the next block's head / chain A's tail form / per-module kernels
    bool ffn2_fused;       // TAIL_MODULES: FFN2 + block norm on the FFN-only form, else LayerNorm + two GEMMs + LayerNorm
};
inline TailRoute exact_tail_route(const EcEncoder* e, const ExactForwardRoutes& f, size_t k, bool rows_carry) {
    if (!(f.chains && e->bw[k].xc_out)) return TAIL_MODULES;
    return k + 1 < e->blocks.size() && e->bw[k + 1].xc_in && e->blocks[k + 1].dim_model == e->blocks[k].dim_expand && rows_carry && !interctc_after(e, k) ? TAIL_FULL : TAIL_ONLY;
}
inline ExactBlockRoutes exact_block_routes(const EcEncoder* e, const ExactForwardRoutes& f, size_t k, bool rows_carry_in, bool rows_carry_out) {
    const BlockW& W = e->bw[k];
    const bool chain_d = f.chains && W.xc_in;
    ExactBlockRoutes r;
    r.head = k > 0 && exact_tail_route(e, f, k - 1, rows_carry_in) == TAIL_FULL ? HEAD_PREV_TAIL : (chain_d ? HEAD_CHAIN : HEAD_MODULES);
    r.ffn1_fused = f.ffn && W.xc_f[0];
    r.chain_b = chain_d;
    r.tail = exact_tail_route(e, f, k, rows_carry_out);
    r.ffn2_fused = f.ffn && W.xc_f[1];
    return r;
}

// Per-module attention of head width d on batch_heads = B H (score tiles ride in a 16-bit grid dimension): split.hip's sx_attention, else exact.hip's ex_attention
inline bool exact_attention_split(const EcEncoder* e, int d, long long batch_heads) { return e->exact_split && sx_attention_supported(d) && batch_heads <= 65535; }
