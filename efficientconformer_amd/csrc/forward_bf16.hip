// The bf16 forward schedule: bf16 activations between kernels, an fp32 residual stream, fused row-local chains where the stage width allows.  Follows
// ConformerEncoder.forward (reference models/encoders.py:97-142) and ConformerBlock.forward (models/blocks.py:119-137); see DESIGN.md for the kernel map.
// Also the per-module entries of the C ABI, which exist only on this file's helpers.
#include "forward_common.h"
#include "routes.h"
#include "stream.h"

#include <cmath>

Workspace make_workspace(const EcEncoder* e, const Shapes& s, bool from_audio) {
    Workspace w;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += al(bytes); return o; };
    const size_t B = s.B;
    size_t mx = 0, ma = 0, mh = 0, mq = 0, me = 0, mg = 0, mc = 0;
    std::vector<size_t> esz;
    for (size_t k = 0; k < e->blocks.size(); ++k) {
        const EcBlock& b = e->blocks[k];
        const size_t T = s.Tin[k], D = b.dim_model, De = b.dim_expand;
        const size_t Tp = ec_round_up((int)T, b.group_size), Tg = Tp / b.group_size;
        const size_t d = (size_t)b.group_size * D / b.num_heads, dpad = ec_round_up((int)d, 32);
        const size_t Mi = (size_t)s.Min[k], Mo = (size_t)s.Mout[k], Mqk = (size_t)s.Mq[k];     // rows in, rows out, Q / K / V rows
        mx = std::max(mx, std::max(Mi * D, Mo * De) * 4);
        ma = std::max(ma, std::max(Mi * ld8(D), Mo * ld8(De)) * 2);
        mh = std::max(mh, std::max(Mi * D, Mo * De) * b.ff_ratio * 2);
        mq = std::max(mq, Mqk * D * 2 + 512);     // Q / K / V: Mq rows x D  + slack: 16-byte chunk loads may run past a row's head span
        me = std::max(me, (size_t)b.num_heads * (2 * Tg - 1) * dpad * 2);
        esz.push_back((size_t)b.num_heads * (2 * Tg - 1) * dpad * 2 + 512);
        mg = std::max(mg, Mi * ld8(De) * 2);
        mc = std::max(mc, Mo * ld8(De) * 2);
    }
    w.mel = take(from_audio ? B * e->cfg.n_mels * s.Tm * 4 : 0);
    size_t T1r = (size_t)s.T1;         // frames per utterance after the subsampling at the input's row pitch (ragged: s.Tm is that pitch, s.T1 the longest utterance's)
    if (s.ragged) { T1r = (size_t)s.Tm; for (int i = 0; i < e->cfg.sub_layers; ++i) T1r = (T1r - 1) / 2 + 1; }
    const FrontScratch fs = front_scratch(e, s.ragged, B, (size_t)s.Tm, T1r);
    w.sub = take(fs.sub); w.xrect = take(fs.xrect); w.sub1 = take(fs.sub1);
    w.x0 = take(mx); w.x1 = take(mx);
    w.a = take(ma); w.hbuf = take(mh);
    w.qu = take(mq); w.kh = take(mq); w.vt = take(mq); w.eh = take(me);
    w.o = take(ma); w.gbuf = take(mg); w.cbuf = take(mc); w.xs = take(ma);
    w.lens = take((e->blocks.size() + 1) * B * 4);
    if (s.ragged) {
        const size_t nbk = e->blocks.size();
        w.mel_len = take(B * 4);
        w.row_off = take((nbk + 1) * (B + 1) * 4);
        w.wg_off = take(nbk * (B + 1) * 4);
        w.tile_off = take(nbk * (B + 1) * 4);
    }
    for (size_t k = 0; k < esz.size(); ++k) w.eh_blk.push_back(take(esz[k]));
    size_t mic = 0;                    // InterCTC handles only (every other configuration: zero bytes, the layout as it was)
    for (int k : e->ic_blocks) mic = std::max(mic, (size_t)s.Mout[k] * e->ic_vocab * 4);
    w.icp = take(mic);
    w.preds = take(0);
    w.total = off;
    return w;
}

namespace {

int run_gemm(EcEncoder* e, int cls, hipStream_t st, const bf16_t* A, int lda, int M, const PackedLinear& L, int epi, void* C, int ldc,
             const float* R = nullptr, int ldr = 0, float alpha = 1.f) {
    const double out_b = (epi == EPI_F32) ? 4.0 : (epi == EPI_RESID_F32 ? 8.0 : 2.0);
    PROF(cls, 2.0 * M * (double)L.N * L.K, (double)M * L.K * 2 + (double)L.N * L.K * 2 + (double)M * L.N * out_b);
    GemmParams p{};
    p.A = A; p.lda = lda; p.W = L.w; p.ldw = L.ldw; p.bias = L.bias;
    p.M = M; p.N = L.N; p.K = L.K; p.C = C; p.ldc = ldc; p.R = R; p.ldr = ldr; p.alpha = alpha;
    p.wide = e->wide_gemm;
    return launch_gemm(p, epi, st);
}

inline int F1c(const EcBlock& b) { return ec_round_up(b.dim_model * b.ff_ratio, 32); }

// POST half of a chain A: the block's FFN1 and stacked Q/K/V projection (both pre-norms folded into the weights at pack time)
void fill_chain_head(ChainParams& cp, const BlockW& W, int D, int Fp, int T, int Tp, const GemmParams& q) {
    cp.D = D;
    cp.f[1] = ChainFfn{W.c_f1a.w, W.c_f1a.ldw, W.c_f1b, W.ffn1_b.ldw, Fp, W.c_f1b_cm};
    cp.g1 = ChainGemm{W.c_qkv.w, W.c_qkv.ldw, W.c_qkv_chunks};
    cp.qu = q.qu; cp.kh = q.kh; cp.vt = q.vt; cp.u = W.u; cp.v = W.v; cp.T = T; cp.Tp = Tp;
}

// x += 1/2 FFN(a): the fused row-stationary kernel (routes.h: ffn_fused; ln != null: the pre-norm is computed in its prologue and `a` is not read), else
// two tiled GEMMs on `a`
int run_ffn(EcEncoder* e, hipStream_t st, bool fused, const bf16_t* a, int M, int D, const PackedLinear& L1, const PackedLinear& L2,
            const bf16_t* w2p, float* x, bf16_t* hbuf, const LNp* ln = nullptr) {
    const int F = L1.N;
    if (fused) {
        PROF(PC_GEMM_FFN, 4.0 * M * (double)D * F, (double)M * D * 10 + 4.0 * D * F);
        FfnParams p{};
        p.A = a; p.lda = ld8(D); p.X = x; p.ldx = D; p.Y = x; p.ldy = D;
        p.W1 = L1.w; p.ldw1 = L1.ldw; p.b1 = L1.bias; p.W2 = w2p; p.ldw2 = L2.ldw; p.b2 = L2.bias;
        p.M = M; p.D = D; p.Fp = ec_round_up(F, 32); p.alpha = 0.5f;
        if (ln) { p.ln_g = ln->g; p.ln_b = ln->b; }
        return launch_ffn_fused(p, st);
    }
    int rc = run_gemm(e, PC_GEMM_FFN, st, a, ld8(D), M, L1, EPI_SWISH_BF16, hbuf, F);
    if (rc) return rc;
    return run_gemm(e, PC_GEMM_FFN, st, hbuf, F, M, L2, EPI_RESID_F32, x, D, x, D, 0.5f);
}

// One GEMM on the row-stationary kernel (rs: routes.h gemm_row_stat) or the tiled one.  lnX / ln: the operand is LayerNorm(lnX) - computed in the
// row-stationary kernel's prologue, or by a LayerNorm launch into A in front of the tiled kernel
int run_rs_or_tiled(EcEncoder* e, bool rs, int cls, hipStream_t st, const bf16_t* A, int lda, int M, const PackedLinear& L, int rs_epi,
                    int tiled_epi, void* C, int ldc, const float* R = nullptr, int ldr = 0, float alpha = 1.f,
                    const float* lnX = nullptr, const LNp* ln = nullptr) {
    if (!rs) {
        if (lnX && ln) { PROF(PC_LAYERNORM, 0, (double)M * L.K * 6); EC_TRY(launch_layernorm(lnX, M, L.K, ln->g, ln->b, nullptr, const_cast<bf16_t*>(A), lda, nullptr, nullptr, st)); }
        return run_gemm(e, cls, st, A, lda, M, L, tiled_epi, C, ldc, R, ldr, alpha);
    }
    const double out_b = (tiled_epi == EPI_F32) ? 4.0 : (tiled_epi == EPI_RESID_F32 ? 8.0 : 2.0);
    PROF(cls, 2.0 * M * (double)L.N * L.K, (double)M * L.K * 2 + (double)L.N * L.K * 2 + (double)M * L.N * out_b);
    GemmParams p{};
    p.A = A; p.lda = lda; p.W = L.w; p.ldw = L.ldw; p.bias = L.bias;
    p.M = M; p.N = L.N; p.K = L.K; p.C = C; p.ldc = ldc; p.R = R; p.ldr = ldr; p.alpha = alpha;
    if (lnX && ln) { p.X = lnX; p.ldx = L.K; p.ln_g = ln->g; p.ln_b = ln->b; }
    return launch_rs_gemm(p, rs_epi, st);
}

// Conv2dSubsampling (modules.py:232-249) + transpose + Linear (encoders.py:113-116): mel (B, n_mels, s.Tm) -> x fp32 (s.Min[0] rows, D0).  The one list of the bf16
// schedule's front-end routes, for rectangular batches (rg = null: rows (b, t), B * T1) and ragged ones (rg: the batch's descriptors; x = the ragged row space).
// sub / act1: bf16 scratch of the unfused variants (the subsampler's output rows / the two-layer subsampler's layer-1 image); xrect: ragged two-layer route only.
// The route: routes.h front_route
int run_subsample_linear(EcEncoder* e, hipStream_t st, const float* mel, const Shapes& s, const BatchRows* rg, bf16_t* sub, bf16_t* act1, float* xrect, float* x) {
    const EcConfig& c = e->cfg;
    const int B = s.B, Tm = s.Tm, C0 = c.sub_filters[0], F2 = c.n_mels / 2, Ksub = C0 * F2, N = e->lin.N;
    const RaggedRows r0 = rg ? rg->rows_at(0) : RaggedRows{};
    const int* mel_len = rg ? rg->mel_len : nullptr;
    const double Mr = (double)s.Min[0];                            // rows of x
    const int Tl1 = (Tm - 1) / 2 + 1;                              // frames after one layer, at the input's pitch
    const FrontRoute route = front_route(e, rg != nullptr);
    if (route == FRONT_TWO_LAYER) {
        // two-layer subsampler (the plain Conformer configurations).  Ragged: both convolutions and the Linear on the RECTANGULAR image at the input's pitch - layer 1
        // zero-fills every utterance's image behind its own last frame, so layer 2 sees the zero padding of the utterance run alone - then the valid rows are gathered
        // into the ragged row space
        const int T2 = (Tl1 - 1) / 2 + 1, F1 = c.n_mels / 2, F2q = c.n_mels / 4, C1 = c.sub_filters[1];
        { PROF(PC_SUBCONV, 2.0 * 9 * B * Tl1 * (double)C0 * F1, (double)B * c.n_mels * Tm * 4 + (double)B * Tl1 * F1 * e->sub2_cp * 2);
          EC_TRY(launch_subsample_conv_cl(mel, B, c.n_mels, Tm, Tl1, e->sub_w9, e->sub_b, C0, e->sub2_cp, act1, st, mel_len)); }
        trace_add(e, st, "subsample1", act1, (int64_t)B * F1 * Tl1, C0, e->sub2_cp, 1);       // layer-1 image, rows (b, f, t), channel-last
        { PROF(PC_GEMM_OTHER, 2.0 * 9 * (double)B * F2q * T2 * C0 * C1, (double)B * Tl1 * F1 * e->sub2_cp * 2 + (double)B * T2 * F2q * C1 * 2);
          EC_TRY(launch_conv2_igemm(act1, B, F1, Tl1, e->sub2_cp, e->sub2_w, 9 * e->sub2_cp, e->sub2_b, C1, F2q, T2, sub, st)); }
        trace_add(e, st, "subsample", sub, (int64_t)B * T2, F2q * C1, F2q * C1, 1);           // the RECTANGULAR image's rows (b, t)
        EC_TRY(run_gemm(e, PC_GEMM_OTHER, st, sub, F2q * C1, B * T2, e->lin, EPI_F32, rg ? xrect : x, N));
        if (rg) { PROF(PC_MISC, 0, Mr * N * 8); EC_TRY(launch_gather_rows(xrect, N, T2, r0, x, st)); }
    } else if (route == FRONT_CHUNKED) {                           // sublinear3.hip: workgroup = (utterance, 128 frames)
        PROF(PC_SUBCONV, 2.0 * 9 * Mr * Ksub + 2.0 * Mr * Ksub * N, (double)B * c.n_mels * Tm * 4 + Mr * N * 4);
        EC_TRY(launch_sublinear3(sub_chunk_params(e, e->sub3, mel, s, rg, x), st));
    } else if (route == FRONT_ROW_STAT) {                          // sublinear2.hip indexes the ragged rows itself
        PROF(PC_SUBCONV, 2.0 * 9 * Mr * Ksub + 2.0 * Mr * Ksub * N, (double)B * c.n_mels * Tm * 4 + Mr * N * 4);
        EC_ABL(rg ? 32 : 0, EC_TRY(launch_sublinear2(mel, B, c.n_mels, Tm, s.T1, e->conv_tab, e->lin_rs, e->lin.bias, C0, N, x, N, st, rg ? &r0 : nullptr, mel_len)));
    } else if (route == FRONT_TILED_FUSED) {                       // sublinear.hip: rectangular batches only
        PROF(PC_SUBCONV, 2.0 * 9 * Mr * Ksub + 2.0 * Mr * Ksub * N, (double)B * c.n_mels * Tm * 4 + Mr * N * 4);
        EC_TRY(launch_sublinear_fused(mel, B, c.n_mels, Tm, s.T1, e->sub_w9, e->sub_b, C0, e->lin_fused, e->lin_fused_ld, e->lin.bias, N, x, N, st));
    } else {
        // FRONT_CONV_GEMM (wide front ends: Large with sub3_auto = 0).  Ragged: the conv (zero padding at every utterance's own last mel frame) writes the RAGGED rows
        // itself (tiles behind an utterance's own end exit; group-padding rows = zeros) and the Linear runs on those rows only.  Group-padding rows of x = the Linear's
        // bias (finite; no kernel mixes them into valid rows).  Tcover >= every utterance's frames rounded up to the group size
        const int Tcover = rg ? Tl1 + e->blocks[0].group_size - 1 : s.T1;
        { PROF(PC_SUBCONV, 2.0 * 9 * Mr * Ksub, (double)B * c.n_mels * Tm * 4 + Mr * Ksub * 2);
          EC_TRY(launch_subsample_conv(mel, B, c.n_mels, Tm, Tcover, e->sub_w9, e->sub_b, C0, sub, Ksub, st, mel_len, rg ? &r0 : nullptr)); }
        trace_add(e, st, "subsample", sub, s.Min[0], Ksub, Ksub, 1);
        EC_TRY(run_gemm(e, PC_GEMM_OTHER, st, sub, Ksub, (int)s.Min[0], e->lin, EPI_F32, x, N));
    }
    return 0;
}

// the launch options every chain carries
ChainParams chain_params(const EcEncoder* e) { ChainParams cp{}; cp.small_m = e->chain_small_m; cp.pair = e->chain_pair; return cp; }

// Self-conditioned CTC step i (of listed block k) on the product kernel: y = x + softmax(x We^T + be) Wp^T + bp on `rows` dense fp32 rows (y may alias x), the
// normalised probabilities to probs (rows, V) where given
int run_interctc(EcEncoder* e, hipStream_t st, int i, const float* x, int rows, float* y, float* probs) {
    const EcEncoder::InterCtcW& W = e->ic_w[i];
    const int De = e->blocks[e->ic_blocks[i]].dim_expand, V = e->ic_vocab;
    InterCtcParams p{};
    p.X = x; p.ldx = De; p.Y = y; p.ldy = De;
    p.W1 = W.expand.w; p.ldw1 = W.expand.ldw; p.b1 = W.expand.bias; p.W2 = W.proj; p.ldw2 = W.proj_ld; p.b2 = W.proj_b;
    p.M = rows; p.D = De; p.V = V; p.Vp = ec_round_up(V, 32); p.probs = probs;
    PROF(PC_GEMM_OTHER, 4.0 * rows * (double)De * V * (probs ? 1.5 : 1.0), (double)rows * De * 8 + 4.0 * De * V + (probs ? (double)rows * V * 4 : 0.0));
    EC_TRY(launch_interctc(p, st));
    return 0;
}

}  // namespace

// Ragged batches (s.ragged): every utterance runs at its own length in one concatenated row space (kernels.h: RaggedRows) - the row-local
// kernels (chains, GEMMs, LayerNorms) just see M rows; the frame-mixing ones (subsampling, attention, depthwise conv, conv_res decimation)
// index utterances through the descriptor arrays lengths_ragged_kernel leaves in the workspace.  out: (B, out_frames, D_last), zero filled
// behind every utterance's own last frame.
int forward_core(EcEncoder* e, const float* mel, const int64_t* in_len, int from_audio, const Shapes& s, const Workspace& w,
                 char* ws, float* out, int64_t* out_len, hipStream_t st, int out_frames, const StreamRound* sr) {
    const EcConfig& c = e->cfg;
    const int B = s.B, nb = (int)e->blocks.size();
    const bool rg = s.ragged;
    BatchRows br;
    EC_TRY(begin_forward(e, st, s, w, ws, mel, in_len, from_audio, out_len, &br));
    const int* mel_len = br.mel_len;

    // ---- Conv2dSubsampling (modules.py:232-249) + transpose + Linear (encoders.py:113-116)
    float* x = reinterpret_cast<float*>(ws + w.x0);
    float* xalt = reinterpret_cast<float*>(ws + w.x1);
    if (sr) {
        // a streaming round (stream.h): the rectangular front end over the streams' mel windows, then chunk row i = window row i + 1 into the ragged row space
        const Shapes win = make_shapes(e, B, sr->mel_pitch);
        EC_TRY(run_subsample_linear(e, st, sr->mel, win, nullptr, sr->sub, sr->sub1, nullptr, sr->xrect));
        { PROF(PC_MISC, 0, (double)s.Min[0] * e->lin.N * 8); EC_TRY(launch_gather_rows(sr->xrect + e->lin.N, e->lin.N, win.T1, br.rows_at(0), x, st)); }
    } else
    EC_TRY(run_subsample_linear(e, st, mel, s, rg ? &br : nullptr, reinterpret_cast<bf16_t*>(ws + w.sub), reinterpret_cast<bf16_t*>(ws + w.sub1),
                                reinterpret_cast<float*>(ws + w.xrect), x));
    trace_add(e, st, "linear", x, s.Min[0], e->lin.N, e->lin.N, 0);

    bf16_t* a = reinterpret_cast<bf16_t*>(ws + w.a);
    bf16_t* hbuf = reinterpret_cast<bf16_t*>(ws + w.hbuf);
    bf16_t* o = reinterpret_cast<bf16_t*>(ws + w.o);
    bf16_t* gbuf = reinterpret_cast<bf16_t*>(ws + w.gbuf);
    bf16_t* cbuf = reinterpret_cast<bf16_t*>(ws + w.cbuf);
    bf16_t* xs = reinterpret_cast<bf16_t*>(ws + w.xs);
    bool have_a = false;
    std::vector<BlockRoutes> routes;           // decided here, once per forward (routes.h); the loop below only reads them
    for (int k = 0; k < nb; ++k) routes.push_back(block_routes(e, k));
    const ECache ec = sr ? ECache{} : e_cache_begin(e, st, ws, s, w.eh_blk[0], true);      // a streaming round reads the session's tables
    const bool e_cached = sr || ec.hit;

    // The self-conditioned CTC step after block k (encoders.py:209-213), in place on the block's output rows (group-padding rows of a ragged batch are just rows).
    // Probabilities: written only where somebody reads them - the caller's buffer (rectangular batches: rows (b, t) ARE (B, T_k, V); ragged ones go through the
    // workspace and are padded per utterance) or a debug trace
    auto interctc_step = [&](int k, float* rows, int Mo) -> int {
        const int i = e->ic_index(k);
        if (i < 0) return 0;
        const int V = e->ic_vocab, De = e->blocks[k].dim_expand;
        float* user = e->ic_out.size() == e->ic_blocks.size() ? e->ic_out[i] : nullptr;
        float* scratch = reinterpret_cast<float*>(ws + w.icp);
        float* probs = user && !rg ? user : (user || e->trace_arena ? scratch : nullptr);
        EC_TRY(run_interctc(e, st, i, rows, Mo, rows, probs));
        trace_block(e, st, k, "x_interctc", rows, Mo, De, De, 0);
        if (probs) trace_block(e, st, k, "interctc_p", probs, Mo, V, V, 0);
        if (user && rg) {
            const RaggedRows rl = br.rows_at(k + 1);
            PROF(PC_MISC, 0, (double)Mo * V * 4 + (double)B * s.Tout[k] * V * 4);
            EC_TRY(launch_emit_rows(scratch, V, rl.off, rl.len, B, s.Tout[k], user, st));
        }
        return 0;
    };

    const int wide_gemm = e->wide_gemm;        // GemmParams::wide of the tiled Q/K/V GEMM (launch_gemm only)
    int mask_stride = 1;                       // product of the strides of the blocks before block k
    for (int k = 0; k < nb; ++k) {
        const EcBlock& b = e->blocks[k];
        const BlockW& W = e->bw[k];
        const BlockRoutes& r = routes[k];
        const int T = s.Tin[k], To = s.Tout[k], D = b.dim_model, De = b.dim_expand;      // ragged: the LONGEST utterance's frames
        const int M = (int)s.Min[k], Mo = (int)s.Mout[k];
        const int G = b.group_size, H = b.num_heads;
        const int Tp = ec_round_up(T, G), Tg = Tp / G, Tgp = ec_round_up(Tg, 8);
        const int d = G * D / H, dpad = ec_round_up(d, 32);
        // Q/K/V/E layout: plain row-major [B*Tp][D] (16-byte row stores from the GEMM, head split = pointer arithmetic in
        // the attention kernel).  An odd grouped head width (d = 135: Medium / Large stage 0) makes the head spans only 2-byte
        // aligned; gfx950 global loads are alignment-free, so the attention kernel reads them as they are.
        // rows (b, t) -> Q / K / V rows b * Tp + t; a ragged batch keeps every utterance's rows group-padded in the residual stream itself,
        // so the map is the identity: ONE "utterance" of M rows
        const int qT = rg ? M : T, qTp = rg ? M : Tp;
        GemmParams p{};
        p.A = a; p.lda = ld8(D); p.W = W.qkv.w; p.ldw = W.qkv.ldw; p.bias = W.qkv.bias;
        p.M = M; p.N = 3 * D; p.K = D;
        p.T = qT; p.Tp = qTp; p.D = D;
        p.qu = reinterpret_cast<bf16_t*>(ws + w.qu);
        p.kh = reinterpret_cast<bf16_t*>(ws + w.kh); p.vt = reinterpret_cast<bf16_t*>(ws + w.vt);
        p.u = W.u; p.v = W.v; p.wide = wide_gemm;
        if (r.head == HEAD_PREV_TAIL) {
            // FFN1 and the Q/K/V projection of this block already ran inside the previous block's tail chain
        } else if (r.head == HEAD_CHAIN) {
            ChainParams cp = chain_params(e);
            fill_chain_head(cp, W, D, F1c(b), qT, qTp, p);
            cp.M = M; cp.X = x; cp.ldx = D; cp.Y = x; cp.ldy = D; cp.consts = W.cc_head;
            PROF(PC_GEMM_FFN, 2.0 * M * (double)D * (2.0 * D * b.ff_ratio + 3.0 * D), (double)M * D * 16 + 22.0 * D * D);
            EC_ABL(2, EC_TRY(launch_chain(cp, CHAIN_A_HEAD, st)));
        } else {
            // ---- x += 1/2 FFN1(x)   (blocks.py:122; modules.py:385-392)
            { PROF(PC_LAYERNORM, 0, (double)M * D * 6); if (!have_a) EC_TRY(launch_layernorm(x, M, D, W.ln_ffn1.g, W.ln_ffn1.b, nullptr, a, ld8(D), nullptr, nullptr, st)); }
            EC_TRY(run_ffn(e, st, r.ffn1_fused, a, M, D, W.ffn1_a, W.ffn1_b, W.ffn1_bp, x, hbuf));
            // ---- Q/K/V of LN(x)   (modules.py:472-488; attentions.py:651-686): row-stationary = the pre-norm in the kernel's prologue
            if (!r.qkv_rs) { PROF(PC_LAYERNORM, 0, (double)M * D * 6); EC_TRY(launch_layernorm(x, M, D, W.ln_att.g, W.ln_att.b, nullptr, a, ld8(D), nullptr, nullptr, st)); }
            { PROF(PC_GEMM_OTHER, 2.0 * M * 3.0 * D * D, (double)M * D * 2 + 3.0 * D * D * 2 + (double)M * D * 8);
              if (r.qkv_rs) {
                  p.W = W.qkv_nat.w; p.ldw = W.qkv_nat.ldw; p.bias = W.qkv_nat.bias;          // rows permuted inside every 32-row chunk
                  p.X = x; p.ldx = D; p.ln_g = W.ln_att.g; p.ln_b = W.ln_att.b;
                  EC_TRY(launch_rs_gemm(p, 4, st));
              } else {
                  EC_TRY(launch_gemm(p, EPI_QKV_NAT, st));
              } }
        }
        trace_block(e, st, k, "x_ffn1", x, M, D, D, 0);

        // ---- x += MHSA(LN(x))   (blocks.py:125-126; attentions.py:549-718)
        {
            { PROF(PC_MISC, 0, 0);
              if (rg) EC_ABL(64, EC_TRY(launch_attn_pad_rows_ragged(p.qu, p.kh, p.vt, W.u, D, G, br.rows_at(k), st)));
              else EC_TRY(launch_attn_pad_rows_nat(p, B, st)); }
            // positional embeddings E = pos_layer(R) (attentions.py:588 / 678): input independent, tiny (2Tp-G rows)
            GemmParams pe{};
            // relative tables: R[m] = sinusoid(Tp - 1 - G/2 - m), m < 2 Tp - G; causal: R[m] = sinusoid(Tp - 1 - m), m < Tp (attentions.py:1243-1251, 1296-1309)
            const int erows = c.causal ? Tp : 2 * Tp - G;
            pe.A = W.pos_table + (size_t)(b.max_pos - Tp + (c.causal ? 0 : G / 2)) * ld8(D); pe.lda = ld8(D);
            pe.W = W.pos.w; pe.ldw = W.pos.ldw; pe.bias = W.pos.bias;
            pe.M = erows; pe.N = D; pe.K = D;
            bf16_t* eh = reinterpret_cast<bf16_t*>(ws + w.eh_blk[k]);
            pe.C = eh; pe.ldc = D;
            if (!sr && Tp > b.max_pos) return fail("sequence longer than max_pos_encoding");
            if (!e_cached) { PROF(PC_GEMM_OTHER, 2.0 * erows * (double)D * D, (double)erows * D * 4 + (double)D * D * 2);
                             EC_TRY(launch_gemm(pe, EPI_BF16, st)); }
            if (e->trace_arena) {    // the attention kernel's operands: rows b Tp + t (ragged: the group-padded row space), pad rows filled; E rows m < erows
                const int64_t qrows = rg ? (int64_t)M : (int64_t)B * Tp;
                trace_block(e, st, k, "qu", p.qu, qrows, D, D, 1);
                trace_block(e, st, k, "k", p.kh, qrows, D, D, 1);
                trace_block(e, st, k, "v", p.vt, qrows, D, D, 1);
                trace_block(e, st, k, "e", eh, erows, D, D, 1);
            }
            AttnParams ap{};
            ap.qu = p.qu; ap.kh = p.kh; ap.vt = p.vt; ap.eh = eh;
            ap.dvu = W.dvu; ap.dvu_ld = W.dvu_ld;
            ap.lens = br.lens_at(k);
            ap.B = B; ap.H = H; ap.T = T; ap.G = G; ap.D = D; ap.d = d; ap.dpad = dpad; ap.Tg = Tg; ap.Tgp = Tgp;
            ap.q_bstride = (long long)Tp * D; ap.q_hstride = d; ap.q_rowstride = G * D; ap.e_hstride = d; ap.e_rowstride = G * D;
            ap.out = o; ap.ldo = ld8(D); ap.scale = 1.0f / std::sqrt((float)d);
            const Band bd = band(c, mask_stride, G);
            ap.band_l = bd.l; ap.band_r = bd.r;
            ap.causal = c.causal;
            const bool streaming = c.causal || ap.band_l < Tg || ap.band_r < Tg;
            const AttentionRoute ar = sr ? AttentionRoute{} : attention_route(e, dpad, rg, streaming);
            if (ar.refusal) return fail(ar.refusal);
            if (rg) {
                ap.rag_off = br.off_at(k); ap.rag_wg = br.wg_off + (size_t)k * (B + 1); ap.rag_nwg = s.wgs[k]; ap.rag_tgmax = Tg;
            }
            if (sr) {
                // the chunk's queries against the stream's ring + the chunk's own keys, then the chunk's K / V rows join the ring
                const StreamRound::Block& sb = sr->blk[k];
                StreamAttnParams sp{};
                sp.qu = p.qu; sp.k = p.kh; sp.v = p.vt; sp.e = sb.e; sp.n_dist = sb.n_dist; sp.dvu = W.dvu; sp.dvu_ld = W.dvu_ld;
                sp.kc = sb.kc; sp.vc = sb.vc; sp.cap = sb.cap;
                sp.row_off = br.off_at(k); sp.rows = br.lens_at(k); sp.cached = sb.cached; sp.pos = sb.pos; sp.slot = sr->slot;
                sp.B = B; sp.H = H; sp.G = G; sp.D = D; sp.d = d; sp.dpad = dpad; sp.max_rows = T; sp.band_l = bd.l;
                sp.out = o; sp.ldo = ld8(D); sp.scale = ap.scale;
                { PROF(PC_ATTENTION, 2.0 * H * (double)M / G * (sb.cap + (double)Tg) * d * 3.0, (double)B * sb.cap * G * D * 4 + (double)M * D * 2 * 5);
                  EC_TRY(launch_stream_attention(sp, st)); }
                { PROF(PC_MISC, 0, (double)M * D * 8); EC_TRY(launch_stream_kv_append(sp, st)); }
            } else
            { PROF(PC_ATTENTION, 2.0 * H * (rg ? s.tg2[k] : (double)B * Tg * Tg) * d * 3.0, (double)M * D * 2 * 5);
              if (ar.waves) EC_ABL(rg || streaming ? 1 : 0, EC_TRY(launch_relpos_attention2(ap, ar.waves, st)));
              else EC_TRY(launch_relpos_attention(ap, st)); }
            if (!sr && (int)e->att_out.size() == nb && e->att_out[k]) {       // opt-in: the reference's att_w of this block (encoders.py:129)
                // ragged batches: (B, H, Tg of the LONGEST utterance, same) per block, an utterance's own Tg x Tg block = its map run alone, zeros elsewhere
                EC_TRY(launch_attention_probs(ap, e->att_out[k], st));
            }
            trace_block(e, st, k, "att_o", o, M, D, ld8(D), 1);
            if (r.chain_b) {
                ChainParams cp = chain_params(e);
                cp.M = M; cp.D = D; cp.X = x; cp.ldx = D; cp.Y = x; cp.ldy = D; cp.A = o; cp.lda = ld8(D);
                cp.g0 = ChainGemm{W.c_outp.w, W.c_outp.ldw, 0};
                cp.g1 = ChainGemm{W.c_pw1.w, W.c_pw1.ldw, W.c_pw1_chunks};
                cp.glu = gbuf; cp.ldg = ld8(De); cp.Ng = De; cp.T = qT; cp.Tp = qTp; cp.consts = W.cc_b;
                PROF(PC_GEMM_OTHER, 2.0 * M * (double)D * (D + 2.0 * De), (double)M * D * 10 + (double)M * De * 2 + 2.0 * D * (D + 2.0 * De));
                EC_ABL(4, EC_TRY(launch_chain(cp, CHAIN_B, st)));
            } else {
                EC_TRY(run_rs_or_tiled(e, r.outp_rs, PC_GEMM_OTHER, st, o, ld8(D), M, W.outp, 0, EPI_RESID_F32, x, D, x, D, 1.0f));
            }
            trace_block(e, st, k, "x_mhsa", x, M, D, D, 0);
        }

        // ---- x = conv_res(x) + ConvModule(x)   (blocks.py:129; modules.py:511-522)
        if (!r.chain_b) EC_TRY(run_rs_or_tiled(e, r.pw1_rs, PC_GEMM_OTHER, st, a, ld8(D), M, W.pw1, 2, EPI_GLU_BF16, gbuf, ld8(De), nullptr, 0, 1.f, x, &W.ln_conv));
        trace_block(e, st, k, "glu", gbuf, M, De, ld8(De), 1);
        const RaggedConv rc = rg ? br.conv_at(k, Mo, true) : RaggedConv{};
        if (sr) {
            // the k - 1 rows in front of the chunk come from the stream's state, which then takes the chunk's last rows
            StreamDwParams dp{};
            dp.g = gbuf; dp.ld = ld8(De); dp.C = De; dp.w_kc = W.dw_w; dp.bias = W.dw_b; dp.ksize = b.kernel_size; dp.stride = b.conv_stride;
            dp.state = sr->blk[k].conv; dp.in_off = rc.in_off; dp.rows = rc.in_len; dp.hist = sr->blk[k].hist; dp.out_off = rc.out_off; dp.out_end = rc.out_off + 1;
            dp.slot = sr->slot; dp.B = B; dp.max_rows = T; dp.out = cbuf;
            PROF(PC_DWCONV, 2.0 * Mo * (double)De * b.kernel_size, (double)M * De * 2 + (double)Mo * De * 2);
            EC_TRY(launch_stream_dwconv(dp, st));
            EC_TRY(launch_stream_dwconv_state(dp, st));
        } else
        { PROF(PC_DWCONV, 2.0 * Mo * (double)De * b.kernel_size, (double)M * De * 2 + (double)Mo * De * 2); EC_ABL(8, EC_TRY(launch_dwconv(gbuf, B, T, To, De, ld8(De), W.dw_w, W.dw_b, b.kernel_size, b.conv_stride, cbuf, st, rg ? &rc : nullptr, c.causal, r.dw_mfma ? W.dw_a : nullptr, W.dw_a3))); }
        mask_stride *= b.conv_stride;
        trace_block(e, st, k, "dw", cbuf, Mo, De, ld8(De), 1);
        if (D != De) {   // 1x1 strided conv on frames 0, s, 2s, ...  (blocks.py:106-110)
            { PROF(PC_MISC, 0, (double)Mo * D * 6); EC_ABL(64, EC_TRY(launch_cast_rows(x, D, T, b.conv_stride, To, B, xs, ld8(D), st, rg ? &rc : nullptr))); }
            EC_TRY(run_rs_or_tiled(e, r.res_rs, PC_GEMM_OTHER, st, xs, ld8(D), Mo, W.res, 1, EPI_F32, xalt, De));
            std::swap(x, xalt);
        } else if (b.conv_stride > 1) {
            return fail("strided block without expansion is not native (no shipped config uses it)");
        }
        const bool last = (k == nb - 1);
        float* xo = (last && !rg) ? out : x;        // ragged: the last block writes its rows in place; emit_rows pads them into `out` below
        if (r.tail != TAIL_MODULES) {
            const bool next_head = r.tail == TAIL_FULL;
            ChainParams cp = chain_params(e);
            cp.M = Mo; cp.D = De; cp.X = x; cp.ldx = De; cp.Y = xo; cp.ldy = De; cp.A = cbuf; cp.lda = ld8(De);
            cp.g0 = ChainGemm{W.c_pw2.w, W.c_pw2.ldw, 0};
            cp.f[0] = ChainFfn{W.c_f2a.w, W.c_f2a.ldw, W.c_f2b, W.ffn2_b.ldw, ec_round_up(De * b.ff_ratio, 32), W.c_f2b_cm};
            double fl = 2.0 * Mo * (double)De * (De + 2.0 * De * b.ff_ratio), by = (double)Mo * De * 10 + 2.0 * De * De * (1 + 2.0 * b.ff_ratio);
            if (next_head) {
                const EcBlock& nbk = e->blocks[k + 1];
                const int Gn = nbk.group_size;
                const int Tn = rg ? Mo : s.Tin[k + 1], Tpn = rg ? Mo : ec_round_up(Tn, Gn);
                GemmParams pn{};
                pn.qu = reinterpret_cast<bf16_t*>(ws + w.qu);
                pn.kh = reinterpret_cast<bf16_t*>(ws + w.kh); pn.vt = reinterpret_cast<bf16_t*>(ws + w.vt);
                fill_chain_head(cp, e->bw[k + 1], De, F1c(nbk), Tn, Tpn, pn);
                fl += 2.0 * Mo * (double)De * (2.0 * De * nbk.ff_ratio + 3.0 * De); by += (double)Mo * De * 8 + 2.0 * De * De * (3 + 2.0 * nbk.ff_ratio);
            }
            cp.consts = next_head ? W.cc_full : W.cc_tail;
            { PROF(PC_GEMM_FFN, fl, by); EC_ABL(2, EC_TRY(launch_chain(cp, next_head ? CHAIN_A_FULL : CHAIN_A_TAIL, st))); }
            have_a = false;
            if (last || interctc_after(e, k)) { trace_block(e, st, k, "out", xo, Mo, De, De, 0); }      // (a step's input is part of its trace)
            EC_TRY(interctc_step(k, xo, Mo));
            continue;
        }
        EC_TRY(run_rs_or_tiled(e, r.pw2_rs, PC_GEMM_OTHER, st, cbuf, ld8(De), Mo, W.pw2, 0, EPI_RESID_F32, x, De, x, De, 1.0f));
        trace_block(e, st, k, "x_conv", x, Mo, De, De, 0);

        // ---- x += 1/2 FFN2(x); x = LN(x)   (blocks.py:132-135)
        if (!r.ffn2_fused) { PROF(PC_LAYERNORM, 0, (double)Mo * De * 6); EC_TRY(launch_layernorm(x, Mo, De, W.ln_ffn2.g, W.ln_ffn2.b, nullptr, a, ld8(De), nullptr, nullptr, st)); }
        EC_TRY(run_ffn(e, st, r.ffn2_fused, a, Mo, De, W.ffn2_a, W.ffn2_b, W.ffn2_bp, x, hbuf, r.ffn2_fused ? &W.ln_ffn2 : nullptr));
        // block-final norm fused with the next block's FFN1 pre-norm (both read the same rows) - unless an InterCTC step rewrites those rows first
        const bool next_a = !last && !interctc_after(e, k);
        { PROF(PC_LAYERNORM, 0, (double)Mo * De * 10); EC_TRY(launch_layernorm(x, Mo, De, W.ln_out.g, W.ln_out.b, xo, next_a ? a : nullptr, ld8(De),
                                next_a ? e->bw[k + 1].ln_ffn1.g : nullptr, next_a ? e->bw[k + 1].ln_ffn1.b : nullptr, st)); }
        have_a = next_a;
        trace_block(e, st, k, "out", xo, Mo, De, De, 0);
        EC_TRY(interctc_step(k, xo, Mo));
    }
    if (!sr) e_cache_end(e, ws, s, ec);
    if (rg) EC_TRY(emit_ragged(e, st, br, x, out_frames, out));
    return 0;
}

// =================================================================== C ABI: one module on the product kernels
extern "C" {

int effconf_relpos_attention(const uint16_t* qu, const uint16_t* k, const uint16_t* v, const uint16_t* e, const float* dvu, int32_t dvu_ld,
                             const int32_t* lens, int32_t batch, int32_t heads, int32_t frames, int32_t group, int32_t dim, uint16_t* out,
                             int32_t ld_out, int32_t variant, void* stream) {
    if (!qu || !k || !v || !e || !dvu || !lens || !out) return fail("null argument");
    if (batch <= 0 || heads <= 0 || frames <= 0 || group <= 0 || !(group & 1) || dim <= 0 || (group * dim) % heads) return fail("bad attention shape");
    AttnParams ap{};
    const int Tp = ec_round_up(frames, group), Tg = Tp / group, d = group * dim / heads, dpad = ec_round_up(d, 32);
    if (dpad > 192 || dvu_ld < dpad || ld_out < dim) return fail("unsupported head width / leading dimension");
    ap.qu = qu; ap.kh = k; ap.vt = v; ap.eh = e; ap.dvu = dvu; ap.dvu_ld = dvu_ld; ap.lens = lens;
    ap.B = batch; ap.H = heads; ap.T = frames; ap.G = group; ap.D = dim; ap.d = d; ap.dpad = dpad; ap.Tg = Tg; ap.Tgp = ec_round_up(Tg, 8);
    ap.q_bstride = (long long)Tp * dim; ap.q_hstride = d; ap.q_rowstride = group * dim; ap.e_hstride = d; ap.e_rowstride = group * dim;
    ap.out = out; ap.ldo = ld_out; ap.scale = 1.0f / std::sqrt((float)d);
    ap.band_l = ap.band_r = 1 << 30;          // full context, rectangular; bands, causal tables and ragged batches: effconf_debug_relpos_attention (tests/test_gpu_attention_edges.py)
    if (variant == 0) { EC_TRY(launch_relpos_attention(ap, (hipStream_t)stream)); return 0; }
    if ((variant != 1 && variant != 2) || !relpos_attention2_supported(dpad)) return fail("attention variant not available for this head width");
    EC_TRY(launch_relpos_attention2(ap, variant, (hipStream_t)stream));
    return 0;
}

// ---- per-kernel entry points: one module of a block on the product kernels, unit-testable against the reference's
// per-module outputs (tests/golden/tiny_*.npz: trace/blocks.N.ffn1 | conv | out, trace/linear)
size_t effconf_module_workspace_bytes(const EcEncoder* e, int32_t batch, int32_t frames) {
    if (!e || batch <= 0 || frames <= 0) return 0;
    size_t mx = 0;
    for (const EcBlock& b : e->blocks) {
        const size_t D = (size_t)std::max(b.dim_model, b.dim_expand);
        mx = std::max(mx, D * ((size_t)b.ff_ratio + 4) * 2 + 64);
    }
    const size_t rows = (size_t)batch * frames;
    // effconf_subsample's scratch: frames = mel frames here; its rows counted after ONE layer (an upper bound for the two-layer subsampler, kept)
    const FrontScratch fs = front_scratch(e, false, (size_t)batch, (size_t)frames, (size_t)(frames - 1) / 2 + 1);
    return std::max(al(rows * mx) + 4 * 256, al(fs.sub) + al(fs.sub1) + 256);
}

int effconf_ffn(EcEncoder* e, int32_t block, int32_t which, const float* x, int32_t rows, float* y, void* workspace, size_t workspace_bytes,
                void* stream) {
    if (!e || !e->finalized) return fail("encoder not finalized");
    if (block < 0 || block >= (int)e->blocks.size() || (which != 1 && which != 2) || !x || !y || rows <= 0 || !workspace) return fail("bad argument");
    const EcBlock& b = e->blocks[block];
    const BlockW& W = e->bw[block];
    const int D = which == 1 ? b.dim_model : b.dim_expand, F = D * b.ff_ratio;
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(workspace);
    const size_t a_bytes = al((size_t)rows * ld8(D) * 2), h_bytes = al((size_t)rows * F * 2);
    if (workspace_bytes < a_bytes + h_bytes) return fail("workspace too small");
    bf16_t* a = reinterpret_cast<bf16_t*>(ws);
    bf16_t* hbuf = reinterpret_cast<bf16_t*>(ws + a_bytes);
    if (y != x && hipMemcpyAsync(y, x, (size_t)rows * D * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail("copy failed");
    const LNp& ln = which == 1 ? W.ln_ffn1 : W.ln_ffn2;
    const PackedLinear &L1 = which == 1 ? W.ffn1_a : W.ffn2_a, &L2 = which == 1 ? W.ffn1_b : W.ffn2_b;
    const bf16_t* w2p = which == 1 ? W.ffn1_bp : W.ffn2_bp;
    const bool fused = ffn_fused_module(D);      // not the forward's ffn_fused: this entry keeps the fused kernel where tiled_auto / wide_gemm send a forward to the tiled GEMMs
    if (!fused) EC_TRY(launch_layernorm(y, rows, D, ln.g, ln.b, nullptr, a, ld8(D), nullptr, nullptr, st));
    return run_ffn(e, st, fused, a, rows, D, L1, L2, w2p, y, hbuf, fused ? &ln : nullptr);       // fused: pre-norm in the kernel's prologue
}

int effconf_interctc(EcEncoder* e, int32_t block, const float* x, int32_t rows, float* y, float* probs, void* workspace, size_t workspace_bytes,
                     void* stream) {
    (void)workspace; (void)workspace_bytes;          // the fused kernel keeps the logits on the CU: no scratch
    if (!e || !e->finalized) return fail("encoder not finalized");
    if (block < 0 || block >= (int)e->blocks.size() || !x || !y || rows <= 0) return fail("bad argument");
    const int i = e->ic_index(block);
    if (i < 0) return fail("effconf_interctc: block " + std::to_string(block) + " has no InterCTC step (effconf_encoder_set_interctc)");
    return run_interctc(e, (hipStream_t)stream, i, x, rows, y, probs);
}

int effconf_conv_module(EcEncoder* e, int32_t block, const float* x, int32_t batch, int32_t frames, float* y, void* workspace,
                        size_t workspace_bytes, void* stream) {
    if (!e || !e->finalized) return fail("encoder not finalized");
    if (block < 0 || block >= (int)e->blocks.size() || !x || !y || batch <= 0 || frames <= 0 || !workspace) return fail("bad argument");
    const EcBlock& b = e->blocks[block];
    const BlockW& W = e->bw[block];
    const int D = b.dim_model, De = b.dim_expand, T = frames, To = (T - 1) / b.conv_stride + 1, M = batch * T, Mo = batch * To;
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(workspace);
    const size_t a_bytes = al((size_t)M * ld8(D) * 2), g_bytes = al((size_t)M * ld8(De) * 2), c_bytes = al((size_t)Mo * ld8(De) * 2);
    if (workspace_bytes < a_bytes + g_bytes + c_bytes) return fail("workspace too small");
    bf16_t* a = reinterpret_cast<bf16_t*>(ws);
    bf16_t* gbuf = reinterpret_cast<bf16_t*>(ws + a_bytes);
    bf16_t* cbuf = reinterpret_cast<bf16_t*>(ws + a_bytes + g_bytes);
    const BlockRoutes r = block_routes(e, block);
    // LayerNorm -> pointwise-1 + GLU (modules.py:511-514)
    EC_TRY(run_rs_or_tiled(e, r.pw1_rs, PC_GEMM_OTHER, st, a, ld8(D), M, W.pw1, 2, EPI_GLU_BF16, gbuf, ld8(De), nullptr, 0, 1.f, x, &W.ln_conv));
    // depthwise conv + BatchNorm + Swish (modules.py:516-518), pointwise-2 (modules.py:519)
    EC_TRY(launch_dwconv(gbuf, batch, T, To, De, ld8(De), W.dw_w, W.dw_b, b.kernel_size, b.conv_stride, cbuf, st, nullptr, e->cfg.causal, r.dw_mfma ? W.dw_a : nullptr, W.dw_a3));
    return run_rs_or_tiled(e, r.pw2_rs, PC_GEMM_OTHER, st, cbuf, ld8(De), Mo, W.pw2, 1, EPI_F32, y, De);
}

int effconf_subsample(EcEncoder* e, const float* mel, int32_t batch, int32_t n_frames, float* y, void* workspace, size_t workspace_bytes,
                      void* stream) {
    if (!e || !e->finalized) return fail("encoder not finalized");
    if (!mel || !y || batch <= 0 || n_frames <= 0 || !workspace) return fail("bad argument");
    const Shapes s = make_shapes(e, batch, n_frames);
    const FrontScratch fs = front_scratch(e, false, (size_t)batch, (size_t)n_frames, (size_t)s.T1);
    const size_t sub_bytes = al(fs.sub);
    if (workspace_bytes < sub_bytes + al(fs.sub1)) return fail("workspace too small");
    char* ws = reinterpret_cast<char*>(workspace);
    return run_subsample_linear(e, (hipStream_t)stream, mel, s, nullptr, reinterpret_cast<bf16_t*>(ws), reinterpret_cast<bf16_t*>(ws + sub_bytes), nullptr, y);
}

int effconf_layernorm_residual(EcEncoder* e, int32_t block, int32_t which, const float* x, const float* r, float alpha, int32_t rows, float* y,
                               void* stream) {
    if (!e || !e->finalized) return fail("encoder not finalized");
    if (block < 0 || block >= (int)e->blocks.size() || which < 0 || which > 4 || !x || !y || rows <= 0) return fail("bad argument");
    const EcBlock& b = e->blocks[block];
    const BlockW& W = e->bw[block];
    const LNp* ln[5] = {&W.ln_ffn1, &W.ln_att, &W.ln_conv, &W.ln_ffn2, &W.ln_out};
    const int D = which >= 3 ? b.dim_expand : b.dim_model;
    EC_TRY(launch_layernorm_residual(x, r, alpha, rows, D, ln[which]->g, ln[which]->b, y, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
