// The label-exact forward schedule: fp32 activations everywhere, every product either on the fp32 matrix pipe (exact_fp32 = 1, exact.hip) or on the fp16
// matrix pipe with split operand pairs (exact_fp32 = 2, split.hip / sxf*.hip).  One schedule, two kernel families (forward_exact).
#include "forward_common.h"
#include "routes.h"

// rows come from the Shapes totals: B * T for rectangular batches, the sums over the utterances for ragged ones (s.Tm = the input's row pitch there)
XWorkspace make_xworkspace(const EcEncoder* e, const Shapes& s) {
    XWorkspace w;
    size_t off = 0;
    auto take = [&](size_t floats) { size_t o = off; off += al(floats * 4); return o; };
    const size_t B = s.B;
    size_t mx = 0, mh = 0, mq = 0, me = 0, mp = 0, mg = 0, mc = 0, mkp = 0, mvp = 0, mep = 0, mxs = 0;
    for (size_t k = 0; k < e->blocks.size(); ++k) {
        const EcBlock& b = e->blocks[k];
        const size_t T = s.Tin[k], D = b.dim_model, De = b.dim_expand;
        const size_t Mi = (size_t)s.Min[k], Mo = (size_t)s.Mout[k], Mqk = (size_t)s.Mq[k];
        const size_t Tp = ec_round_up((int)T, b.group_size);
        mx = std::max(mx, std::max(Mi * D, Mo * De));
        mh = std::max(mh, std::max(Mi * D, Mo * De) * b.ff_ratio);
        mq = std::max(mq, Mqk * D);
        me = std::max(me, (2 * Tp - b.group_size) * D);
        {   // operand images of the fused split attention (kernels.h: SxfAttnParams), in floats
            const size_t dh = b.group_size * D / b.num_heads, pk = sxf_attention_pk((int)dh), vx = sxf_attention_vx((int)dh), Tg = Tp / b.group_size;
            mkp = std::max(mkp, (Mqk / b.group_size + 64) * b.num_heads * 2 * pk / 2);
            mvp = std::max(mvp, B * b.num_heads * 2 * vx * (size_t)ec_round_up((int)Tg, 64) / 2);
            mep = std::max(mep, 2 * Tg * b.num_heads * 2 * pk / 2);
        }
        mp = std::max(mp, Mi * 2 * De);
        mg = std::max(mg, Mi * De);
        mc = std::max(mc, Mo * De);
        if (D != De) mxs = std::max(mxs, Mo * D);
        if (e->ic_index(k) >= 0) mh = std::max(mh, Mo * (size_t)e->ic_vocab);      // the (rows, V) logits / probabilities of an InterCTC step live in the FFN's hidden plane
    }
    const int L = e->cfg.sub_layers;
    size_t T1r = s.Tm; for (int i = 0; i < L; ++i) T1r = (T1r - 1) / 2 + 1;          // rows per utterance of the rectangular front end (ragged: at the input's pitch)
    const size_t F1 = (e->cfg.n_mels - 1) / 2 + 1, Tl1 = (s.Tm - 1) / 2 + 1;
    w.conv1 = take(L == 2 ? B * e->cfg.sub_filters[0] * F1 * Tl1 : 0);
    int F = e->cfg.n_mels; for (int i = 0; i < L; ++i) F = (F - 1) / 2 + 1;
    w.sub = take(B * T1r * (size_t)e->cfg.sub_filters[L - 1] * F);
    w.x0 = take(mx); w.x1 = take(mx); w.a = take(mx); w.h = take(mh);
    w.q = take(mq); w.k = take(mq); w.v = take(mq); w.e = take(me); w.o = take(mq);
    w.p1 = take(mp); w.g = take(mg); w.c = take(mc);
    w.lens = take((e->blocks.size() + 1) * B);
    w.qkv_stride = (w.k - w.q) / 4;                 // floats between the Q, K and V buffers (the stacked projection writes all three)
    if (e->exact_split) {                           // split.hip: (B, H, Tg, Tg) attention scores of one block (rectangular batches with attention maps)
        size_t ms = 0;
        if (!s.ragged)
            for (size_t k = 0; k < e->blocks.size(); ++k) {
                const EcBlock& b = e->blocks[k];
                const int Tg = ec_round_up(s.Tin[k], b.group_size) / b.group_size;
                ms = std::max(ms, sx_attention_scores_bytes(s.B, b.num_heads, Tg) / 4);
            }
        w.scores = take(ms);
        w.kp = take(mkp); w.vp = take(mvp); w.ep = take(mep); w.xs = take(mxs);
        for (size_t k = 0; k < e->blocks.size(); ++k) {
            const EcBlock& b = e->blocks[k];
            const size_t dh = b.group_size * b.dim_model / b.num_heads, pk = sxf_attention_pk((int)dh), Tg = ec_round_up(s.Tin[k], b.group_size) / b.group_size;
            w.ep_blk.push_back(take(2 * Tg * b.num_heads * 2 * pk / 2));
        }
        if (s.ragged) {
            const size_t nbk = e->blocks.size();
            w.xrect = take(B * T1r * e->blocks[0].dim_model);
            w.mel_len = take(B);
            w.row_off = take((nbk + 1) * (B + 1));
            w.wg_off = take(nbk * (B + 1));
            w.tile_off = take(nbk * (B + 1));
        }
    }
    w.total = off;
    return w;
}

namespace {

const float* xget(EcEncoder* e, const std::string& k) {
    auto it = e->xw.find(k);
    return it == e->xw.end() ? nullptr : it->second;
}

// C = epi(A W^T + bias) with the weights of state-dict module `prefix` ([N][K]); everything a call does not name in GemmOpt is the plain product on M contiguous rows
struct Rows { int rows = 0, pitch = 0, stride = 0; };      // row m -> (m / rows) * pitch + (m % rows) * stride (C rows: stride 1); rows = 0: the identity
struct GemmOpt {
    Rows a, c;                                                  // kernels.h: ExGemmParams a_rows / a_pitch / a_stride, c_rows / c_pitch
    int epi = 0; const float* R = nullptr; float alpha = 1.f;   // 0 plain, 1 Swish, 2 residual: C = R + alpha * (acc + bias) (R may alias C)
    int cols = 0; size_t stride = 0;                            // cols > 0: column n -> buffer C + (n / cols) * stride, column n % cols
    int cls = PC_GEMM_OTHER;                                    // profile class
};

int xgemm(EcEncoder* e, hipStream_t st, const float* A, int lda, int M, const std::string& prefix, int N, int K, float* C, int ldc, const GemmOpt& o = GemmOpt{}) {
    ExGemmParams p{};
    p.A = A; p.lda = lda; p.a_rows = o.a.rows; p.a_pitch = o.a.pitch; p.a_stride = o.a.stride;
    p.W = xget(e, prefix + ".weight"); p.ldw = K; p.bias = xget(e, prefix + ".bias");
    if (!p.bias) return fail("exact mode: missing " + prefix);
    p.M = M; p.N = N; p.K = K; p.C = C; p.ldc = ldc; p.c_rows = o.c.rows; p.c_pitch = o.c.pitch;
    p.split_cols = o.cols; p.split_stride = o.stride;
    p.R = o.R; p.ldr = ldc; p.alpha = o.alpha; p.epi = o.epi;
    // flop: the algorithmic 2 M N K (the split kernels issue three MFMAs per product)
    PROF(o.cls, 2.0 * M * (double)N * K, 4.0 * ((double)M * K + (double)N * K + (double)M * N));
    if (e->exact_split) {
        auto it = e->xsplit.find(prefix);
        if (it != e->xsplit.end()) {
            SxGemmParams q{};
            q.g = p; q.Whi = it->second.hi; q.Wlo = it->second.lo; q.ldh = it->second.ldh;
            const int rc = launch_sx_gemm(q, st);
            // -2 = a shape the split kernel does not take (N, lda or ldc not a multiple of 4, rows * lda >= 2^32 elements, more than 65535 column tiles):
            // the fp32-MFMA kernel handles those, and its weights are uploaded in split mode too (advisor, round 4)
            if (rc != -2 || !p.W) return rc;
        }
    }
    if (!p.W) return fail("exact mode: missing " + prefix);
    return launch_ex_gemm(p, st);
}

// x += alpha * (A W^T + bias); o: A's row map, the profile class
int xresid(EcEncoder* e, hipStream_t st, const float* A, int lda, int M, const std::string& prefix, int N, int K, float* x, float alpha, GemmOpt o = GemmOpt{}) {
    o.epi = 2; o.R = x; o.alpha = alpha;
    return xgemm(e, st, A, lda, M, prefix, N, K, x, N, o);
}

int xlayernorm(EcEncoder* e, hipStream_t st, const float* in, int rows, int dim, const LNp& ln, float* dst) {
    PROF(PC_LAYERNORM, 0, (double)rows * dim * 8);
    return launch_layernorm(in, rows, dim, ln.g, ln.b, dst, nullptr, 0, nullptr, nullptr, st);
}

// x += 1/2 FFN(LN(x)) as LayerNorm + two GEMMs (modules.py:385-392); a / hb: scratch rows of width dim / dim * ratio
int xffn(EcEncoder* e, hipStream_t st, float* x, int rows, int dim, int ratio, const LNp& ln, const std::string& module, float* a, float* hb) {
    GemmOpt ffn; ffn.cls = PC_GEMM_FFN;
    GemmOpt swish = ffn; swish.epi = 1;
    EC_TRY(xlayernorm(e, st, x, rows, dim, ln, a));
    EC_TRY(xgemm(e, st, a, dim, rows, module + ".layers.1", dim * ratio, dim, hb, dim * ratio, swish));
    return xresid(e, st, hb, dim * ratio, rows, module + ".layers.4", dim, dim * ratio, x, 0.5f, ffn);
}

// One FeedForwardModule outside a chain: xo = x + 1/2 FFN(LN(x)), then xo = ln_out(xo) where ln_out is given (blocks.py:122, 132-135).  fused: the FFN-only form of
// sxc_a_kernel on the module's chain image, else LayerNorm + two GEMMs (in place on x) [+ LayerNorm]
int xffn_module(EcEncoder* e, hipStream_t st, bool fused, size_t k, int which, float* x, float* xo, int rows, const LNp* ln_out, float* a, float* hb) {
    const EcBlock& b = e->blocks[k];
    const BlockW& W = e->bw[k];
    const int dim = which ? b.dim_expand : b.dim_model;
    if (fused) {
        SxcAParams cp{};
        cp.xres = x; cp.y = xo; cp.M = rows; cp.D = dim; cp.w_f2 = W.xc_f[which]; cp.nch_f2 = W.xf_nch[which]; cp.b_f2 = W.xf_b2[which];
        if (ln_out) { cp.ln_g = ln_out->g; cp.ln_b = ln_out->b; }
        PROF(PC_GEMM_FFN, 4.0 * rows * (double)dim * dim * b.ff_ratio, (double)rows * dim * 8 + 16.0 * dim * dim * b.ff_ratio);
        return launch_sxc_a(cp, st);
    }
    EC_TRY(xffn(e, st, x, rows, dim, b.ff_ratio, which ? W.ln_ffn2 : W.ln_ffn1, "blocks." + std::to_string(k) + (which ? ".feed_forward_module2" : ".feed_forward_module1"), a, hb));
    return ln_out ? xlayernorm(e, st, x, rows, dim, *ln_out, xo) : 0;
}

}  // namespace

// ------------------------------------------------------------------ the label-exact forward.  Reference: encoders.py:97-142, blocks.py:119-137,
// attentions.py:506-529, 549-718, 1243-1247, layers.py:97-101.  One schedule on one of two kernel families:
//   fused (split mode with every width built, no attention maps requested): sxf*.hip - ONE attention kernel per block that keeps the scores on the CU; the front
//     end, the feed-forward modules and the row-local work around attention as fused kernels where their images exist; ragged batches - every utterance at its own
//     length in the concatenated, group-padded row space of the bf16 path (the row-local GEMMs / LayerNorms see M rows; attention, depthwise conv and the conv_res
//     decimation index utterances through the descriptors of lengths_ragged_kernel); causal relative tables / causal depthwise padding; the E cache;
//   per-module (fp32 mode; split mode with a head width sxf.hip does not take or with attention maps, which are a by-product of the scores in memory): exact.hip /
//     split.hip - LayerNorm, GEMMs, GLU, depthwise conv as kernels of their own, attention with the scores in memory, chunk-padding rows of Q / K / V zero filled
//     by a memset.  Rectangular batches only (the ragged entry refuses), no causal kernels, and the smaller debug trace it always had.
int forward_exact(EcEncoder* e, const float* mel, const int64_t* in_len, int from_audio, const Shapes& s, const XWorkspace& w,
                  char* ws, float* out, int64_t* out_len, hipStream_t st, int out_frames) {
    const EcConfig& c = e->cfg;
    const int B = s.B, nb = (int)e->blocks.size();
    const bool rg = s.ragged;
    // every kernel choice of this forward (routes.h), decided here; the schedule below only reads them
    const ExactForwardRoutes fr = exact_forward_routes(e, e->trace_arena != nullptr, !e->att_out.empty());
    if (fr.refusal) return fail(fr.refusal);
    const bool fused = fr.fused;
    std::vector<ExactBlockRoutes> routes(nb);
    for (int k = 0; k < nb; ++k) routes[k] = exact_block_routes(e, fr, k, k > 0 && s.Min[k] == s.Mout[k - 1], k + 1 < nb && s.Min[k + 1] == s.Mout[k]);
    // The E image of the fused family is cached like the bf16 path's E; the tag is never equal to a bf16 forward's on the same workspace.  A debug trace wants
    // the projections recorded, and the per-module family lays its own buffers over the workspace: both drop whatever cache is there and leave none
    // (fp32 -> bf16 -> fp32 -> bf16 on one workspace otherwise ends with attention reading fp32 activations as E)
    const size_t e_layout = w.ep_blk.empty() ? 0 : w.ep_blk[0] ^ ((size_t)1 << 62) ^ ((size_t)c.causal << 61);
    const ECache ec = e_cache_begin(e, st, ws, s, e_layout, fused && !e->trace_arena);
    BatchRows br;
    EC_TRY(begin_forward(e, st, s, w, ws, mel, in_len, from_audio, out_len, &br));
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    // every entry of this schedule's trace: fp32 rows, dense.  The per-module family records mel, subsample, linear and per block x_ffn1, x_mhsa, x_conv, out
    // only (ftrace = the rest): the arena silently drops what does not fit, so more entries could push `out` off its end
    auto trace = [&](int k, const char* what, const float* ptr, int64_t rows, int cols) { trace_block(e, st, k, what, ptr, rows, cols, cols, 0); };
    auto ftrace = [&](int k, const char* what, const float* ptr, int64_t rows, int cols) { if (fused) trace(k, what, ptr, rows, cols); };
    // ---- Conv2dSubsampling (modules.py:232-249) + transpose + Linear (encoders.py:113-116).  Ragged: on the rectangular image at the input's pitch with every
    //      utterance's frames behind its own end read / written as zeros (the zero padding it sees when run alone), then the valid rows are gathered
    float* sub = F32(w.sub);
    float* x = F32(w.x0);
    float* xalt = F32(w.x1);
    const int C0 = c.sub_filters[0], D0 = e->blocks[0].dim_model;
    int T1r = s.Tm; for (int i = 0; i < c.sub_layers; ++i) T1r = (T1r - 1) / 2 + 1;
    // one-layer subsampler: convolution + Swish + Linear as ONE kernel on the frames that exist (sxf_sub.hip) - the (frames, C F') activation stays in registers.
    // A debug trace wants that activation ("subsample"): per-module kernels then, unless option trace_fused keeps the forward as it runs untraced
    if (fr.sublin) {
        const double Mr = (double)s.Min[0], Ks = (double)C0 * e->xsub.fo;
        PROF(PC_SUBCONV, 2.0 * Mr * Ks * (9.0 + D0), (double)B * c.n_mels * s.Tm * 4 + Mr * D0 * 4);
        EC_TRY(launch_sxf_sublin(sub_chunk_params(e, e->xsub, mel, s, rg ? &br : nullptr, x), st));
    } else {
        int Fl = (c.n_mels - 1) / 2 + 1, Cl = C0;
        {
            PROF(PC_SUBCONV, 0, (double)B * c.n_mels * s.Tm * 4);
            if (c.sub_layers == 1) {
                EC_TRY(launch_ex_conv2d(mel, B, 1, c.n_mels, s.Tm, xget(e, "subsampling_module.layers.0.0.weight"), e->xsub_scale[0], e->xsub_shift[0], C0, sub, 1, st, br.mel_len));
            } else {
                float* img = F32(w.conv1);
                const int F1 = Fl, Tl1 = (s.Tm - 1) / 2 + 1, C1 = c.sub_filters[1];
                EC_TRY(launch_ex_conv2d(mel, B, 1, c.n_mels, s.Tm, xget(e, "subsampling_module.layers.0.0.weight"), e->xsub_scale[0], e->xsub_shift[0], C0, img, 0, st, br.mel_len));
                EC_TRY(launch_ex_conv2d(img, B, C0, F1, Tl1, xget(e, "subsampling_module.layers.1.0.weight"), e->xsub_scale[1], e->xsub_shift[1], C1, sub, 1, st));
                Fl = (F1 - 1) / 2 + 1; Cl = C1;
            }
        }
        // the rectangular image: rows (b, t) at the batch's pitch (ragged: zeros read behind an utterance's own mel frames; the valid rows are gathered)
        const int Ksub = Cl * Fl, Tsub = rg ? T1r : s.T1;
        trace_add(e, st, "subsample", sub, (int64_t)B * Tsub, Ksub, Ksub, 0);
        EC_TRY(xgemm(e, st, sub, Ksub, B * Tsub, "linear", D0, Ksub, rg ? F32(w.xrect) : x, D0));
        if (rg) { PROF(PC_MISC, 0, (double)s.Min[0] * D0 * 8); EC_TRY(launch_gather_rows(F32(w.xrect), D0, T1r, br.rows_at(0), x, st)); }
    }
    trace_add(e, st, "linear", x, s.Min[0], D0, D0, 0);
    float *a = F32(w.a), *hb = F32(w.h), *q = F32(w.q), *kk = F32(w.k), *v = F32(w.v), *eb = F32(w.e), *o = F32(w.o), *p1 = F32(w.p1), *g = F32(w.g),
          *cbuf = F32(w.c), *xs = F32(w.xs);
    uint16_t *kpk = reinterpret_cast<uint16_t*>(ws + w.kp), *vpk = reinterpret_cast<uint16_t*>(ws + w.vp);
    int mask_stride = 1;                       // product of the strides of the blocks before block k
    // the row-local work between attention and the depthwise convolution as two kernels per block, and a feed-forward module outside them as one (sxf_chain.hip);
    // a debug trace wants the intermediate states, which the chains never write: per-module kernels then (option trace_fused: the chains stay, and the trace
    // holds what they write to memory)
    for (int k = 0; k < nb; ++k) {
        const ExactBlockRoutes& rt = routes[k];
        const EcBlock& b = e->blocks[k];
        const BlockW& W = e->bw[k];
        const int T = s.Tin[k], To = s.Tout[k], D = b.dim_model, De = b.dim_expand;          // ragged: the LONGEST utterance's frames
        const int M = (int)s.Min[k], Mo = (int)s.Mout[k];
        const int G = b.group_size, H = b.num_heads, Tp = ec_round_up(T, G), Tg = Tp / G, d = G * D / H;
        const std::string p = "blocks." + std::to_string(k);
        const std::string m = p + ".multi_head_self_attention_module", cm = p + ".convolution_module.layers";
        // Rows of Q / K / V: rectangular (b, t) -> b Tp + t, ragged: the identity (the residual stream keeps every utterance group-padded)
        const int qr = rg ? 0 : T, qp = rg ? 0 : Tp;
        const bool head_done = rt.tail == TAIL_FULL;      // the next block's FFN1 + Q / K / V projections run at the end of this block's chain A
        if (rt.head == HEAD_PREV_TAIL) {
            trace(k, "x_ffn1", x, M, D);      // nothing to run: x is the stream after FFN1, Q / K / V are written
        } else if (rt.head == HEAD_CHAIN) {
            SxcAParams cp{};
            cp.head = 1; cp.y = x; cp.M = M; cp.D = D; cp.w_f1 = W.xc_f[0]; cp.nch_f1 = W.xf_nch[0]; cp.b_f1 = W.xf_b2[0]; cp.w_qkv = W.xc_qkv;
            cp.q = q; cp.qkv_stride = w.qkv_stride; cp.q_rows = qr; cp.q_pitch = qp; cp.qkv_bytes = (2 * w.qkv_stride + (size_t)s.Mq[k] * D) * 4;
            PROF(PC_GEMM_FFN, M * (double)D * D * (4.0 * b.ff_ratio + 6.0), (double)M * D * 24 + D * (double)D * (16.0 * b.ff_ratio + 12.0));
            EC_TRY(launch_sxc_a(cp, st));
            trace(k, "x_ffn1", x, M, D);
        } else {
            // ---- x += 1/2 FFN1(LN(x))   (blocks.py:122; modules.py:385-392)
            EC_TRY(xffn_module(e, st, rt.ffn1_fused, k, 0, x, x, M, nullptr, a, hb));
            trace(k, "x_ffn1", x, M, D);
            // ---- x += MHSA(LN(x))   (blocks.py:125-126; attentions.py:549-718).  Chunk-padding rows of Q / K / V (attentions.py:107-138, 671) are never written:
            //      the fused attention kernel substitutes them, the per-module ones read the zeros of a memset
            EC_TRY(xlayernorm(e, st, x, M, D, W.ln_att, a));
            if (!fused && Tp != T) {
                if (hipMemsetAsync(q, 0, (size_t)B * Tp * D * 4, st) != hipSuccess || hipMemsetAsync(kk, 0, (size_t)B * Tp * D * 4, st) != hipSuccess ||
                    hipMemsetAsync(v, 0, (size_t)B * Tp * D * 4, st) != hipSuccess) return fail("memset failed");
            }
            GemmOpt proj; proj.c = Rows{qr, qp};
            if (e->exact_split && e->xsplit.count(m + ".mhsa.qkv_layer")) {      // one stacked projection: column n -> buffer n / D (q | k | v), column n % D
                GemmOpt stacked = proj; stacked.cols = D; stacked.stride = w.qkv_stride;
                EC_TRY(xgemm(e, st, a, D, M, m + ".mhsa.qkv_layer", 3 * D, D, q, D, stacked));
            } else {
                EC_TRY(xgemm(e, st, a, D, M, m + ".mhsa.query_layer", D, D, q, D, proj));
                EC_TRY(xgemm(e, st, a, D, M, m + ".mhsa.key_layer", D, D, kk, D, proj));
                EC_TRY(xgemm(e, st, a, D, M, m + ".mhsa.value_layer", D, D, v, D, proj));
            }
        }
        // rows (b, t) -> b Tp + t of the projections (chunk-padding rows: whatever the workspace held)
        ftrace(k, "q", q, s.Mq[k], D); ftrace(k, "k", kk, s.Mq[k], D); ftrace(k, "v", v, s.Mq[k], D);
        if (Tp > b.max_pos) return fail("sequence longer than max_pos_encoding");
        // relative tables: R[m] = sinusoid(Tp - 1 - G/2 - m), m < 2 Tp - G; causal: R[m] = sinusoid(Tp - 1 - m), m < Tp (attentions.py:1243-1251, 1296-1309)
        const float* tab = e->xtab[std::make_pair(b.max_pos, D)];
        const int erows = c.causal ? Tp : 2 * Tp - G;
        uint16_t* epk = fused ? reinterpret_cast<uint16_t*>(ws + w.ep_blk[k]) : nullptr;
        if (!ec.hit) {
            EC_TRY(xgemm(e, st, tab + (size_t)(b.max_pos - Tp + (c.causal ? 0 : G / 2)) * D, D, erows, m + ".mhsa.pos_layer", D, D, eb, D));
            ftrace(k, "e", eb, erows, D);      // the fp32 projection, before sxf_pack_e
            if (fused) { PROF(PC_MISC, 0, (double)erows * D * 8); EC_TRY(launch_sxf_pack_e(eb, W.u, W.v, erows / G, H, G, D, d, epk, st)); }
        }
        const Band bd = band(c, mask_stride, G);
        if (fused) {
            SxfAttnParams ap{};
            ap.q = q; ap.k = kk; ap.v = v; ap.kp = kpk; ap.vp = vpk; ap.ep = epk; ap.vpitch = ec_round_up(Tg, 64); ap.u = W.u; ap.lens = br.lens_at(k);
            ap.off = rg ? br.off_at(k) : nullptr;
            ap.B = B; ap.H = H; ap.G = G; ap.D = D; ap.d = d; ap.T = T; ap.Tp = Tp; ap.Tg = Tg; ap.out = o; ap.causal = c.causal;
            ap.band_l = bd.l; ap.band_r = bd.r;
            { PROF(PC_MISC, 0, (double)s.Mq[k] * D * 16); EC_TRY(launch_sxf_pack_kv(ap, st)); }
            PROF(PC_ATTENTION, 2.0 * H * (rg ? s.tg2[k] : (double)B * Tg * Tg) * d * 3.0, (double)s.Mq[k] * D * 4 * 4);
            EC_TRY(launch_sxf_attention(ap, st));
        } else {
            ExAttnParams ap{};
            ap.q = q; ap.k = kk; ap.v = v; ap.e = eb; ap.u = W.u; ap.vb = W.v; ap.lens = br.lens_at(k);
            ap.B = B; ap.H = H; ap.T = T; ap.Tp = Tp; ap.G = G; ap.D = D; ap.d = d; ap.Tg = Tg; ap.out = o; ap.variant = e->exact_attention;
            ap.att = (int)e->att_out.size() == nb ? e->att_out[k] : nullptr;
            ap.band_l = bd.l; ap.band_r = bd.r;
            PROF(PC_ATTENTION, 2.0 * B * H * (double)Tg * Tg * d * 3.0, (double)M * D * 4 * 5);
            if (exact_attention_split(e, d, (long long)B * H)) EC_TRY(launch_sx_attention(ap, F32(w.scores), st));
            else EC_TRY(launch_ex_attention(ap, st));
        }
        ftrace(k, "att_o", o, s.Mq[k], D);
        if (rt.chain_b) {     // x += O Wo^T + bo;  g = GLU(LN(x) Wp1^T + bp1)
            SxcBParams cp{};
            cp.o = o; cp.o_rows = qr; cp.o_pitch = qp; cp.x = x; cp.g = g; cp.M = M; cp.D = D; cp.De = De;
            cp.w_o = W.xc_wo; cp.b_o = W.xc_bo; cp.w_p1 = W.xc_p1; cp.nch_p1 = W.xc_nch_p1;
            PROF(PC_GEMM_OTHER, 2.0 * M * D * ((double)D + 2.0 * De), (double)M * (D * 12.0 + De * 4.0) + 4.0 * D * ((double)D + 2.0 * De));
            EC_TRY(launch_sxc_b(cp, st));
            trace(k, "x_mhsa", x, M, D);
        } else {
            GemmOpt orows; orows.a = Rows{qr, qp, 1};
            EC_TRY(xresid(e, st, o, D, M, m + ".mhsa.output_layer", D, D, x, 1.0f, orows));
            trace(k, "x_mhsa", x, M, D);
            // ---- x = conv_res(x) + ConvModule(x)   (blocks.py:129; modules.py:511-522)
            EC_TRY(xlayernorm(e, st, x, M, D, W.ln_conv, a));
            EC_TRY(xgemm(e, st, a, D, M, cm + ".2", 2 * De, D, p1, 2 * De));
            if (fused) { PROF(PC_MISC, 0, (double)M * De * 12); EC_TRY(launch_sxf_glu(p1, M, De, g, st)); }
            else EC_TRY(launch_ex_glu(p1, M, De, g, st));
        }
        ftrace(k, "glu", g, M, De);
        const RaggedConv rc = rg ? br.conv_at(k, Mo, false) : RaggedConv{};
        if (fused) {
            const int tcap = rg ? ec_round_up(To, k + 1 < nb ? e->blocks[k + 1].group_size : 1) : To;
            PROF(PC_DWCONV, 2.0 * Mo * (double)De * b.kernel_size, (double)M * De * 4 + (double)Mo * De * 4);
            EC_TRY(launch_sxf_dwconv(g, B, T, To, De, W.dw_w, W.dw_b, b.kernel_size, b.conv_stride, cbuf, st, rg ? &rc : nullptr, c.causal, tcap));
        } else {
            EC_TRY(launch_ex_dwconv(g, B, T, To, De, W.dw_w, W.dw_b, b.kernel_size, b.conv_stride, cbuf, st));
        }
        ftrace(k, "dw", cbuf, Mo, De);
        mask_stride *= b.conv_stride;
        if (D != De) {      // 1x1 strided conv on frames 0, s, 2s, ...  (blocks.py:106-110)
            if (rg) {
                { PROF(PC_MISC, 0, (double)Mo * D * 8); EC_TRY(launch_sxf_decimate(x, D, b.conv_stride, rc, xs, st)); }
                EC_TRY(xgemm(e, st, xs, D, Mo, p + ".conv_res.1", De, D, xalt, De));
            } else {
                GemmOpt strided; strided.a = Rows{To, T, b.conv_stride};
                EC_TRY(xgemm(e, st, x, D, Mo, p + ".conv_res.1", De, D, xalt, De, strided));
            }
            std::swap(x, xalt);
            ftrace(k, "conv_res", x, Mo, De);      // the residual rows chain A's tail / pointwise-2 adds to
        } else if (b.conv_stride > 1) {
            return fail("strided block without expansion is not native (no shipped config uses it)");
        }
        const bool to_out = k == nb - 1 && !rg;       // ragged: the last block's rows stay in the workspace; emit_ragged pads them into `out`
        float* xo = to_out ? out : xalt;
        if (rt.tail != TAIL_MODULES) {      // x = xres + C Wp2^T + bp2;  x += 1/2 FFN2(LN(x));  xo = LN(x);  [next block: xo += 1/2 FFN1(LN(xo)); Q | K | V]
            SxcAParams cp{};
            cp.tail = 1; cp.c = cbuf; cp.xres = x; cp.y = xo; cp.M = Mo; cp.D = De;
            cp.w_p2 = W.xc_p2; cp.b_p2 = W.xc_bp2; cp.w_f2 = W.xc_f[1]; cp.nch_f2 = W.xf_nch[1]; cp.b_f2 = W.xf_b2[1]; cp.ln_g = W.ln_out.g; cp.ln_b = W.ln_out.b;
            double fl = Mo * (double)De * De * (2.0 + 4.0 * b.ff_ratio), by = (double)Mo * De * 16 + De * (double)De * (4.0 + 16.0 * b.ff_ratio);
            if (head_done) {
                const EcBlock& bn = e->blocks[k + 1];
                const BlockW& Wn = e->bw[k + 1];
                const int Tn = s.Tin[k + 1];
                cp.head = 1; cp.w_f1 = Wn.xc_f[0]; cp.nch_f1 = Wn.xf_nch[0]; cp.b_f1 = Wn.xf_b2[0]; cp.w_qkv = Wn.xc_qkv;
                cp.q = q; cp.qkv_stride = w.qkv_stride; cp.q_rows = rg ? 0 : Tn; cp.q_pitch = rg ? 0 : ec_round_up(Tn, bn.group_size); cp.qkv_bytes = (2 * w.qkv_stride + (size_t)s.Mq[k + 1] * De) * 4;
                fl += Mo * (double)De * De * (4.0 * bn.ff_ratio + 6.0); by += (double)Mo * De * 20 + De * (double)De * (16.0 * bn.ff_ratio + 12.0);
            }
            PROF(PC_GEMM_FFN, fl, by);
            EC_TRY(launch_sxc_a(cp, st));
        } else {
            EC_TRY(xresid(e, st, cbuf, De, Mo, cm + ".7", De, De, x, 1.0f));
            trace(k, "x_conv", x, Mo, De);
            // ---- x += 1/2 FFN2(LN(x)); x = LN(x)   (blocks.py:132-135)
            EC_TRY(xffn_module(e, st, rt.ffn2_fused, k, 1, x, xo, Mo, &W.ln_out, a, hb));
        }
        if (!to_out) std::swap(x, xalt);
        if (!head_done) trace(k, "out", xo, Mo, De);      // a merged head has already made xo the next block's x_ffn1
        // ---- self-conditioned CTC (encoders.py:209-213): p = softmax(linear_expand_k(x)) in the reference's order, x += linear_proj_k(p) - three launches, the
        //      logits in memory (routes.h: a listed block's tail never carries the next head, so xo holds the block's output here)
        if (const int ic = e->ic_index(k); ic >= 0) {
            const int V = e->ic_vocab;
            const std::string ks = std::to_string(k);
            EC_TRY(xgemm(e, st, xo, De, Mo, "linear_expand_" + ks, V, De, hb, V));
            { PROF(PC_MISC, 0, (double)Mo * V * 12); EC_TRY(launch_row_softmax(hb, Mo, V, st)); }
            EC_TRY(xresid(e, st, hb, V, Mo, "linear_proj_" + ks, De, V, xo, 1.0f));
            trace(k, "x_interctc", xo, Mo, De);
            ftrace(k, "interctc_p", hb, Mo, V);
            if (float* user = e->ic_out.size() == e->ic_blocks.size() ? e->ic_out[ic] : nullptr) {
                PROF(PC_MISC, 0, (double)Mo * V * 8);
                if (rg) { const RaggedRows rl = br.rows_at(k + 1); EC_TRY(launch_emit_rows(hb, V, rl.off, rl.len, B, s.Tout[k], user, st)); }
                else if (hipMemcpyAsync(user, hb, (size_t)Mo * V * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail("copy failed");
            }
        }
    }
    e_cache_end(e, ws, s, ec);
    if (rg) EC_TRY(emit_ragged(e, st, br, x, out_frames, out));
    return 0;
}
