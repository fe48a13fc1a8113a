// Weight packing (pack.h).  First half: the image builders, pure host arithmetic.  Second half: the steps of effconf_encoder_finalize - each finds its
// tensors among the loaded host tensors, calls a builder, uploads the result and stores the pointer; `upload` (encoder_state.h) is their only way to a device.
#include "pack.h"
#include "routes.h"

#include <algorithm>

namespace pack {

struct Linear { Img w; std::vector<float> bias; int N = 0, K = 0, ldw = 0; };      // pack_linear's result: [round_up(N, 128)][ldw] bf16 + padded bias
struct MelHost { std::vector<float> window, fb_weight; std::vector<float2> twiddle; std::vector<int> fb_start, fb_count, fb_offset; };

std::vector<const float*> row_ptrs(const float* w, int N, int K) {       // the rows of a row-major [N][K] matrix
    std::vector<const float*> rows(N);
    for (int n = 0; n < N; ++n) rows[n] = w + (size_t)n * K;
    return rows;
}
std::vector<float> padded(const std::vector<float>& v, int n, float scale = 1.f) {
    std::vector<float> o(n, 0.f);
    for (size_t i = 0; i < v.size() && (int)i < n; ++i) o[i] = scale * v[i];
    return o;
}

// [N][K] fp32 (row-major, possibly a gather of rows given by `rows`; null = zero row) -> padded bf16 + padded bias
// kperm: K index in accumulator order (acc16): the B fragments of chain.hip are LayerNorm-ed accumulator registers in MFMA C order
// ln_g / ln_b: a LayerNorm in front of this linear layer folded in: W diag(gamma), b + W beta (fp32, before the bf16 rounding); without ln_g: W * scale
// min_ldw: row pitch floor in elements.  The whole-row kernels of rsgemm.hip (RS_F32 / RS_RESID) pick their k-step class from
// max(K, N) and DMA that many columns of every weight row: an expanding layer (K < N) must be packed at least N wide, or the last
// row's DMA runs past the buffer (found with EFFCONF_POISON_GUARDS: conv_res 180 -> 256 of EfficientConformer Medium)
Linear pack_linear(const std::vector<const float*>& rows, const std::vector<float>& bias, int K, bool kperm = false, const float* ln_g = nullptr, const float* ln_b = nullptr, int min_ldw = 0,
                   float scale = 1.0f) {
    Linear L;
    const int N = (int)rows.size(), Np = ec_round_up(N, 128), Kp = ec_round_up(K > min_ldw ? K : min_ldw, 64);
    L.w.assign((size_t)Np * Kp, 0);
    L.bias.assign(Np, 0.f);
    for (int n = 0; n < N && n < (int)bias.size(); ++n) L.bias[n] = bias[n];
    for (int n = 0; n < N; ++n) {
        if (!rows[n]) continue;
        for (int k = 0; k < Kp; ++k) {
            const int src = kperm ? acc16(k) : k;
            if (src < K) L.w[(size_t)n * Kp + k] = bf16_rn(rows[n][src] * (ln_g ? ln_g[src] : scale));
        }
        if (ln_b) {
            double acc = 0.0;
            for (int k = 0; k < K; ++k) acc += (double)rows[n][k] * ln_b[k];
            L.bias[n] += (float)acc;
        }
    }
    L.N = N; L.K = K; L.ldw = Kp;
    return L;
}

// second FFN weight [D][F] (* scale) with the hidden (K) index in accumulator order, so that the first GEMM's accumulator registers are directly the second GEMM's B fragments
Img pack_ffn2_permuted(const float* w, int D, int F, float scale) {
    return pack_linear(row_ptrs(w, D, F), {}, F, true, nullptr, nullptr, 0, scale).w;
}

// The same weight chunk-major for chain2.hip: slab c (hidden units 32c .. 32c + 31 of all DP output rows, 64 B per row) is contiguous and already in
// the LDS image's slot order (piece pc of row n at slot 4n + ((pc + (n >> 2)) & 3), rowstat.h dma_w2_off), so a wave-DMA reads 1 KiB of consecutive
// bytes (row-major: sixteen 64-byte half lines per wave-DMA, the other half of every line belonging to the next slab)
Img pack_ffn2_chunkmajor(const float* w, int D, int F, float scale, int DP) {
    const int nch = ec_round_up(F, 32) / 32;
    Img out((size_t)nch * DP * 32, 0);
    for (int c = 0; c < nch; ++c)
        for (int n = 0; n < D; ++n)
            for (int pc = 0; pc < 4; ++pc) {
                const int slot = 4 * n + ((pc + (n >> 2)) & 3);
                for (int i = 0; i < 8; ++i) {
                    const int src = acc16(32 * c + 8 * pc + i);
                    if (src < F) out[((size_t)c * DP * 4 + slot) * 8 + i] = bf16_rn(scale * w[(size_t)n * F + src]);
                }
            }
    return out;
}

void conv_bn_fold(const float* w, const float* b, const std::vector<float>& sc, const std::vector<float>& sh, int C, int taps, std::vector<double>* wf, std::vector<float>* bf) {
    if (wf) wf->resize((size_t)C * taps);
    bf->resize(C);
    for (int ch = 0; ch < C; ++ch) {
        for (int j = 0; j < taps; ++j) (*wf)[(size_t)ch * taps + j] = (double)w[(size_t)ch * taps + j] * sc[ch];      // 24 x 24 bits: exact
        (*bf)[ch] = b[ch] * sc[ch] + sh[ch];
    }
}

// Relative sinusoid table, fp32 operation order of the reference (attentions.py:1219-1226 / 1275-1284): angle = pos / 10000^(2i/D) in fp32, row r <-> position
// max_pos-1-r, even cols sin, odd cols cos.  bf16 [rows][ld8(D)] for the bf16 path, fp32 [rows][D] for the fp32 / split modes, both from the same angles.
void build_pos_table(int max_pos, int D, Img* bf16_ld8, std::vector<float>* f32) {
    const int rows = 2 * max_pos - 1, ld = ld8(D);
    if (bf16_ld8) bf16_ld8->assign((size_t)rows * ld, 0);
    if (f32) f32->assign((size_t)rows * D, 0.f);
    std::vector<float> denom(D / 2);
    for (int i = 0; i < D / 2; ++i) denom[i] = std::pow(10000.0f, (2.0f * (float)i) / (float)D);
    for (int r = 0; r < rows; ++r) {
        const float pos = (float)(max_pos - 1 - r);
        for (int i = 0; i < D / 2; ++i) {
            const float a = pos / denom[i], s = std::sin(a), c = std::cos(a);
            if (bf16_ld8) { (*bf16_ld8)[(size_t)r * ld + 2 * i] = bf16_rn(s); (*bf16_ld8)[(size_t)r * ld + 2 * i + 1] = bf16_rn(c); }
            if (f32) { (*f32)[(size_t)r * D + 2 * i] = s; (*f32)[(size_t)r * D + 2 * i + 1] = c; }
        }
    }
}

// Q | K | V stacked into one weight (row pointers) + bias, each projection [D][D] + [D] padded to `pitch` rows (null rows, zero bias)
void stack_qkv(const HostTensor* const w[3], const HostTensor* const b[3], int D, int pitch, std::vector<const float*>* rows, std::vector<float>* bias) {
    for (int i = 0; i < 3; ++i)
        for (int r = 0; r < pitch; ++r) { rows->push_back(r < D ? w[i]->data.data() + (size_t)r * D : nullptr); bias->push_back(r < D ? b[i]->data[r] : 0.f); }
}

// pointwise-1 (2De, D, 1): GLU halves interleaved in blocks of 32 output channels (a | b)
void glu_interleave(const float* w, const float* b, int De, int D, std::vector<const float*>* rows, std::vector<float>* bias) {
    const int nblk = ec_cdiv(De, 32);
    rows->assign(nblk * 64, nullptr); bias->assign(nblk * 64, 0.f);
    for (int j = 0; j < De; ++j) {
        const int at = j / 32 * 64 + j % 32;
        (*rows)[at] = w + (size_t)j * D;             (*bias)[at] = b[j];
        (*rows)[at + 32] = w + (size_t)(De + j) * D; (*bias)[at + 32] = b[De + j];
    }
}

// two-layer subsampler, layer 2: folded (C1, C, 3, 3) conv -> implicit-GEMM weight [round_up(C1, 128)][9 * Cp], K order (tap, c_in), Cp = round_up(C, 64)
Img sub2_conv_image(const std::vector<double>& wf, int C1, int C) {
    const int Cp = ec_round_up(C, 64);
    Img wp((size_t)ec_round_up(C1, 128) * 9 * Cp, 0);
    for (int n = 0; n < C1; ++n)
        for (int ci = 0; ci < C; ++ci)
            for (int tap = 0; tap < 9; ++tap) wp[(size_t)n * 9 * Cp + (size_t)tap * Cp + ci] = bf16_rn((float)wf[((size_t)n * C + ci) * 9 + tap]);
    return wp;
}

// two-layer subsampler: the Linear's [N][C1 * F2] weight with its K axis in (f2, c) order (reference feature index c*F2 + f2, modules.py:247)
std::vector<float> linear_f2c(const float* lw, int N, int C1, int F2) {
    const int K = C1 * F2;
    std::vector<float> perm((size_t)N * K);
    for (int n = 0; n < N; ++n)
        for (int f2 = 0; f2 < F2; ++f2)
            for (int ch = 0; ch < C1; ++ch) perm[(size_t)n * K + (size_t)f2 * C1 + ch] = lw[(size_t)n * K + (size_t)ch * F2 + f2];
    return perm;
}

// sublinear.hip: K' = (fc*Cp + ch)*8 + e  <->  reference feature ch*(F/2) + 8*fc + e; row pitch (F2 / 8) * round_up(C, 8) * 8
Img sublinear_image(const float* lw, int N, int C, int F2) {
    const int Cp = ec_round_up(C, 8), Kp = (F2 / 8) * Cp * 8;
    Img wf((size_t)ec_round_up(N, 128) * Kp, 0);
    for (int n = 0; n < N; ++n)
        for (int fc = 0; fc < F2 / 8; ++fc)
            for (int ch = 0; ch < C; ++ch)
                for (int ee = 0; ee < 8; ++ee) wf[(size_t)n * Kp + ((size_t)fc * Cp + ch) * 8 + ee] = bf16_rn(lw[(size_t)n * (C * F2) + ch * F2 + fc * 8 + ee]);
    return wf;
}

// sublinear2.hip: per output frequency f a slab [32 NT rows n][32 CG columns]: natural column = channel c (reference feature c*(F/2) + f, modules.py:247) in
// accumulator order - the Swish-ed accumulator registers of the conv MFMA are the B fragments directly (chain.hip's register hand-off); conv taps [32 CG][16]
void sublinear2_images(const float* lw, const std::vector<double>& taps, const std::vector<float>& tbias, int N, int C, int F2, int CGr, Img* w, std::vector<float>* tab) {
    const int Cp = 32 * CGr, rows = 32 * CGr;
    w->assign((size_t)F2 * rows * Cp, 0);
    for (int f = 0; f < F2; ++f)
        for (int n = 0; n < N; ++n)
            for (int k = 0; k < Cp; ++k)
                if (acc16(k) < C) (*w)[((size_t)f * rows + n) * Cp + k] = bf16_rn(lw[(size_t)n * (C * F2) + (size_t)acc16(k) * F2 + f]);
    tab->assign((size_t)Cp * 16, 0.f);
    for (int ch = 0; ch < C; ++ch) {
        for (int j = 0; j < 9; ++j) (*tab)[(size_t)ch * 16 + j] = (float)taps[ch * 9 + j];
        (*tab)[(size_t)ch * 16 + 9] = tbias[ch];
    }
}

// The chunked front-end images of sublinear3.hip (bf16: taps truncated hi + lo, weight one plane) and sxf_sub.hip (fp16 same-scale pairs, weight two planes):
// conv taps [ncb][hi | lo][32 channels][16] (taps 0 - 8 folded, 9 the folded bias) and the Linear's weight in chunks of (output frequency, 32 channels)
// [chunk][w_planes][DP2 rows][32 k], k in accumulator order (register 8 s + e of lane half kh holds channel 32 cb + acc16(pos)); false: an element was refused
bool front_chunks(const std::vector<double>& taps, const std::vector<float>& tbias, const float* lw, const float* lb, int C, int F, int N, int nt,
                  PairEnc tap_enc, PairEnc w_enc, int w_planes, Img* cimg, Img* wimg, std::vector<float>* bias) {
    const int ncb = (C + 31) / 32, DP2 = 32 * nt;
    cimg->assign((size_t)ncb * 2 * 32 * 16, 0); wimg->assign((size_t)F * ncb * w_planes * DP2 * 32, 0);
    bool ok = true;
    for (int ch = 0; ch < C; ++ch) {
        uint16_t* at = cimg->data() + (size_t)(ch / 32) * 2 * 32 * 16 + (size_t)(ch % 32) * 16;
        for (int j = 0; j < 9; ++j) ok &= tap_enc(taps[ch * 9 + j], at + j, at + 32 * 16 + j);
        ok &= tap_enc(tbias[ch], at + 9, at + 32 * 16 + 9);
    }
    for (int f = 0; f < F; ++f)
        for (int cb = 0; cb < ncb; ++cb) {
            uint16_t* base = wimg->data() + (size_t)(f * ncb + cb) * w_planes * DP2 * 32;
            for (int n = 0; n < N; ++n)
                for (int pos = 0; pos < 32; ++pos) {
                    const int ch = 32 * cb + acc16(pos);
                    if (ch < C) ok &= w_enc(lw[(size_t)n * C * F + (size_t)ch * F + f], base + (size_t)n * 32 + pos, w_planes == 2 ? base + (size_t)DP2 * 32 + (size_t)n * 32 + pos : nullptr);
                }
        }
    bias->assign(DP2, 0.f);
    for (int n = 0; n < N; ++n) (*bias)[n] = lb[n];
    return ok;
}

// (v - u) per head column [H][ld]: head column x of head h is feature (h*d + x) % D of the un-grouped row (group = view, attentions.py:677-686)
std::vector<float> dvu_table(const float* u, const float* v, int H, int d, int D, int ld) {
    std::vector<float> t((size_t)H * ld, 0.f);
    for (int h = 0; h < H; ++h)
        for (int x = 0; x < d; ++x) { const int n = (h * d + x) % D; t[(size_t)h * ld + x] = v[n] - u[n]; }
    return t;
}

// Constant block of a fused chain (chain_const_layout; one LDS-DMA per workgroup instead of a dozen small strided copies): pre / post = the block whose
// tail / head the chain runs (chain B: pre = its block), from the host copies their packing left in BlockW
std::vector<float> chain_const_block(int kind, int dim, const BlockW* pre, const BlockW* post, const EcBlock* pb, const EcBlock* qb) {
    ChainParams cp{};
    cp.D = dim;
    const bool isb = kind == CHAIN_B;
    if (pre && !isb) cp.f[0].Fp = ec_round_up(pb->dim_expand * pb->ff_ratio, 32);
    if (post) cp.f[1].Fp = ec_round_up(qb->dim_model * qb->ff_ratio, 32);
    cp.g1.nchunks = isb ? pre->c_pw1_chunks : (post ? post->c_qkv_chunks : 0);
    int nf[8];
    const int nfl = chain_const_layout(cp, kind, nf);
    const int DP = chain_padded_width(dim);
    std::vector<float> blk(nfl, 0.f);
    auto put = [&](int off, const std::vector<float>& src, int n) { for (int i = 0; i < n && i < (int)src.size(); ++i) blk[off + i] = src[i]; };
    if (isb) {
        put(nf[0], pre->c_outp.hbias, dim);
        put(nf[6], pre->c_pw1.hbias, 64 * cp.g1.nchunks);
    } else {
        if (pre) {
            put(nf[0], pre->c_pw2.hbias, dim);
            put(nf[1], pre->h_ln_out_g, dim); put(nf[1] + DP, pre->h_ln_out_b, dim);
            put(nf[2], pre->c_f2a.hbias, cp.f[0].Fp); put(nf[3], pre->h_f2b2, dim);
        }
        if (post) {
            put(nf[4], post->c_f1a.hbias, cp.f[1].Fp); put(nf[5], post->h_f1b2, dim);
            put(nf[6], post->c_qkv.hbias, 64 * cp.g1.nchunks);
            put(nf[7], post->h_u, dim); put(nf[7] + DP, post->h_v, dim);
        }
    }
    return blk;
}

// CTC head: fc.weight [V][D] transposed to [D][V] fp32, and as split-bf16 MFMA B fragments W = hi + lo: fragment (k-step s, column v, k-half h) = W[v][16 s + 8 h .. + 7],
// V padded to whole 256-column passes of ctc_argmax_bf16x3_kernel (4 waves x 64): every wave's fragment loads stay inside the image
void ctc_head_images(const float* w, int V, int D, std::vector<float>* wt, Img* hi, Img* lo) {
    const int Kp = ec_round_up(D, 16), Vp = ec_round_up(V, 256);
    wt->resize((size_t)D * V);
    hi->assign((size_t)(Kp / 16) * Vp * 16, 0); lo->assign(hi->size(), 0);
    for (int v = 0; v < V; ++v)
        for (int k = 0; k < D; ++k) {
            (*wt)[(size_t)k * V + v] = w[(size_t)v * D + k];
            const size_t idx = (((size_t)(k / 16) * Vp + v) * 2 + (k % 16) / 8) * 8 + k % 8;
            bf16_pair_round(w[(size_t)v * D + k], &(*hi)[idx], &(*lo)[idx]);
        }
}

MelHost build_mel_tables(const EcConfig& c) {
    MelHost t;
    // Hann(win_length, periodic) centred in n_fft (torch.stft pads the window on both sides)
    t.window.assign(c.n_fft, 0.f);
    const int off = (c.n_fft - c.win_length) / 2;
    for (int n = 0; n < c.win_length; ++n) t.window[off + n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / c.win_length));
    t.twiddle.resize(c.n_fft / 2);
    for (int k = 0; k < c.n_fft / 2; ++k) {
        const double a = -2.0 * M_PI * k / c.n_fft;
        t.twiddle[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    // HTK triangular filterbank, f in [0, 8000], no area normalisation (torchaudio melscale_fbanks, modules.py:82)
    const int nf = c.n_fft / 2 + 1, nm = c.n_mels;
    const double fmin = 0.0, fmax = 8000.0;
    auto hz2mel = [](double f) { return 2595.0 * std::log10(1.0 + f / 700.0); };
    auto mel2hz = [](double m) { return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0); };
    std::vector<double> fpts(nm + 2);
    for (int i = 0; i < nm + 2; ++i) fpts[i] = mel2hz(hz2mel(fmin) + (hz2mel(fmax) - hz2mel(fmin)) * i / (nm + 1));
    t.fb_start.resize(nm); t.fb_count.resize(nm); t.fb_offset.resize(nm);
    for (int m = 0; m < nm; ++m) {
        int s0 = -1, cnt = 0;
        std::vector<float> row;
        for (int k = 0; k < nf; ++k) {
            const double f = (double)(c.sample_rate / 2) * k / (nf - 1);
            const double down = (f - fpts[m]) / (fpts[m + 1] - fpts[m]);
            const double up = (fpts[m + 2] - f) / (fpts[m + 2] - fpts[m + 1]);
            const double w = std::max(0.0, std::min(down, up));
            if (w > 0.0) {
                if (s0 < 0) s0 = k;
                row.resize(k - s0 + 1, 0.f);
                row[k - s0] = (float)w;
                cnt = k - s0 + 1;
            }
        }
        t.fb_start[m] = s0 < 0 ? 0 : s0; t.fb_count[m] = cnt; t.fb_offset[m] = (int)t.fb_weight.size();
        t.fb_weight.insert(t.fb_weight.end(), row.begin(), row.begin() + cnt);
    }
    return t;
}

// Per-module split images of one 2-D weight (nn.Linear [N][K], 1x1 Conv1d [N][K][1]): h and l planes (f16_pair_2048), K padded with zeros to whole 32-wide
// k-tiles and stored k-tile major (kernels.h: SxGemmParams); false + the first refused element's index
bool split_pair_image(const std::vector<const float*>& rows, int K, Img* hi, Img* lo, int* bad_n, int* bad_k) {
    const int N = (int)rows.size(), ldh = ec_round_up(K, 32);
    hi->assign((size_t)N * ldh, 0); lo->assign(hi->size(), 0);
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k) {
            const size_t at = ((size_t)(k / 32) * N + n) * 32 + k % 32;
            if (!f16_pair_2048(rows[n][k], &(*hi)[at], &(*lo)[at])) { *bad_n = n; *bad_k = k; return false; }
        }
    return true;
}

// F1 chunks (sxf_chain.hip), chunk c at base + c * stride: 32 output rows (of `rows`, 32 per chunk; null = padding) x DP1 columns, h plane then l plane
// (f16_pair_s10); gamma folded into the weights, W beta + bias in column K; columns in accumulator order (the operand is a converted accumulator tile).
// false: an element was refused
bool f1_chunk(Img& img, size_t base, size_t stride, int DP1, int K, const std::vector<const float*>& rows, const std::vector<float>& bias, const float* g, const float* beta) {
    bool ok = true;
    for (size_t r = 0; r < rows.size(); ++r) {
        if (!rows[r]) continue;
        uint16_t* at = &img[base + r / 32 * stride + r % 32 * DP1];
        auto put = [&](int col, double v) { ok &= f16_pair_s10(v, at + col, at + 32 * DP1 + col); };
        double bsum = bias[r];
        for (int col = 0; col < DP1; ++col) {
            const int f = acc16(col);
            if (f >= K) continue;
            const double wv = rows[r][f];
            if (beta) bsum += wv * beta[f];
            put(col, g ? wv * g[f] : wv);
        }
        for (int col = 0; col < DP1; ++col)
            if (acc16(col) == K) put(col, bsum);
    }
    return ok;
}

// F2 chunks, chunk c < nch at base + c * stride: DP2 output rows (N of W [N][K]) x 32 input positions (inputs 32 c .. in accumulator order), h plane then l plane
bool f2_chunk(Img& img, size_t base, size_t stride, int DP2, int nch, const float* Wm, int N, int K, double scale) {
    bool ok = true;
    for (int c = 0; c < nch; ++c)
        for (int n = 0; n < N; ++n)
            for (int pos = 0; pos < 32; ++pos) {
                uint16_t* at = &img[base + c * stride + (size_t)n * 32 + pos];
                if (32 * c + acc16(pos) < K) ok &= f16_pair_s10(scale * Wm[(size_t)n * K + 32 * c + acc16(pos)], at, at + 32 * DP2);
            }
    return ok;
}

// One FeedForwardModule at width D as per 32 hidden units an F1 chunk (pre-norm folded) + an F2 chunk (W2 / 2): xc_f (sxf_chain.hip; kernels.h: SxcAParams
// w_f1 / w_f2).  Empty: a folded value the image cannot hold
Img ffn_image(const float* g, const float* beta, const float* w1, const float* b1, const float* w2, int D, int F) {
    int ks, nt; sxc_shape(D, &ks, &nt);
    const int DP1 = 16 * ks, DP2 = 32 * nt, nch = (F + 31) / 32;
    const size_t per = (size_t)64 * (DP1 + DP2);
    std::vector<const float*> rows(32 * nch, nullptr); std::vector<float> bias(32 * nch, 0.f);
    for (int h = 0; h < F; ++h) { rows[h] = w1 + (size_t)h * D; bias[h] = b1[h]; }
    Img img((size_t)nch * per, 0);
    if (!f1_chunk(img, 0, per, DP1, D, rows, bias, g, beta) || !f2_chunk(img, (size_t)64 * DP1, per, DP2, nch, w2, D, F, 0.5)) img.clear();
    return img;
}

}  // namespace pack

std::string mel_config_error(const EcConfig& c) {      // win_length > n_fft would write the window in front of its vector, hop_length <= 0 divides by zero in every frame count
    if (c.n_fft != 512) return "n_fft = " + std::to_string(c.n_fft) + ": only n_fft = 512 is native";
    if (c.win_length <= 0 || c.win_length > c.n_fft) return "win_length = " + std::to_string(c.win_length) + ": must be in 1..n_fft (" + std::to_string(c.n_fft) + ")";
    if (c.hop_length <= 0) return "hop_length = " + std::to_string(c.hop_length) + ": must be >= 1";
    if (c.n_mels < 1 || c.n_mels > 128) return "n_mels = " + std::to_string(c.n_mels) + ": must be in 1..128";
    if (c.sample_rate < 2) return "sample_rate = " + std::to_string(c.sample_rate) + ": must be >= 2";
    return "";
}

// =================================================================== the steps of effconf_encoder_finalize
namespace {
using namespace pack;

const float* fdata(const HostTensor* t) { return t->data.data(); }
bool sized(const HostTensor* t, int64_t n) { return t && (int64_t)t->data.size() == n; }

bool put_linear(EcEncoder* e, const Linear& L, PackedLinear* out) {
    out->w = upload(e, L.w); out->bias = upload(e, L.bias);
    out->hbias = L.bias; out->N = L.N; out->K = L.K; out->ldw = L.ldw;
    return out->w && out->bias;
}

bool pack_named_linear(EcEncoder* e, const std::string& prefix, int N, int K, PackedLinear* out, std::string* err, bool kperm = false,
                       const std::string& fold_ln = "", int min_ldw = 0) {
    const HostTensor *w = find(e, prefix + ".weight"), *b = find(e, prefix + ".bias");
    if (!w || !b) { *err = "missing tensor " + prefix + ".weight/.bias"; return false; }
    if (!sized(w, (int64_t)N * K) || (int)b->data.size() != N) { *err = "shape mismatch for " + prefix; return false; }
    const HostTensor *lg = fold_ln.empty() ? nullptr : find(e, fold_ln + ".weight"), *lb = fold_ln.empty() ? nullptr : find(e, fold_ln + ".bias");
    if (!fold_ln.empty() && (!sized(lg, K) || !sized(lb, K))) { *err = "missing LayerNorm " + fold_ln; return false; }
    return put_linear(e, pack_linear(row_ptrs(fdata(w), N, K), b->data, K, kperm, lg ? fdata(lg) : nullptr, lb ? fdata(lb) : nullptr, min_ldw), out);
}

// a Linear given by rows / bias as the tiled / row-stationary kernels read it and, where the chains are built for width K, in chain order with LayerNorm `ln` folded in
bool put_linear_and_chain(EcEncoder* e, const std::vector<const float*>& rows, const std::vector<float>& bias, int K, const std::string& ln, PackedLinear* plain, PackedLinear* chain) {
    if (!put_linear(e, pack_linear(rows, bias, K), plain)) return false;
    if (!chain_supported(K)) return true;
    const HostTensor *lg = find(e, ln + ".weight"), *lb = find(e, ln + ".bias");
    return lg && lb && put_linear(e, pack_linear(rows, bias, K, true, fdata(lg), fdata(lb)), chain);
}

bool get_ln(EcEncoder* e, const std::string& prefix, int D, LNp* out, std::string* err) {
    const HostTensor *g = find(e, prefix + ".weight"), *b = find(e, prefix + ".bias");
    if (!sized(g, D) || !sized(b, D)) { *err = "missing/mis-shaped LayerNorm " + prefix; return false; }
    out->g = upload(e, g->data); out->b = upload(e, b->data);
    return out->g && out->b;
}

// BatchNorm(eval) fold: y = (x - mean) / sqrt(var + 1e-5) * gamma + beta  -> per-channel scale / shift
bool bn_fold(const EcEncoder* e, const std::string& prefix, int C, std::vector<float>* scale, std::vector<float>* shift, std::string* err) {
    const HostTensor *g = find(e, prefix + ".weight"), *b = find(e, prefix + ".bias");
    const HostTensor *m = find(e, prefix + ".running_mean"), *v = find(e, prefix + ".running_var");
    if (!g || !b || !m || !v || (int)g->data.size() != C) { *err = "missing/mis-shaped BatchNorm " + prefix; return false; }
    scale->resize(C); shift->resize(C);
    for (int c = 0; c < C; ++c) {
        const float s = g->data[c] / std::sqrt(v->data[c] + 1e-5f);
        (*scale)[c] = s;
        (*shift)[c] = b->data[c] - m->data[c] * s;
    }
    return true;
}

// layer-0 subsampling conv (C,1,3,3) + BatchNorm2d fold: taps [C][9] and bias [C] (the bf16 front ends and the fused split front end)
bool fold_front_conv(const EcEncoder* e, std::vector<double>* taps, std::vector<float>* tbias, std::string* err) {
    const int C = e->cfg.sub_filters[0];
    const HostTensor *w = find(e, "subsampling_module.layers.0.0.weight"), *b = find(e, "subsampling_module.layers.0.0.bias");
    std::vector<float> sc, sh;
    if (!b || !sized(w, C * 9)) { *err = "missing subsampling conv weights"; return false; }
    if (!bn_fold(e, "subsampling_module.layers.0.1", C, &sc, &sh, err)) return false;
    conv_bn_fold(fdata(w), fdata(b), sc, sh, C, 9, taps, tbias);
    return true;
}

// the three attention projections of block `m` (prefix up to "mhsa."), each [D][D] + [D]
bool find_qkv(const EcEncoder* e, const std::string& m, int D, const HostTensor* w[3], const HostTensor* b[3], std::string* missing = nullptr) {
    const char* names[3] = {"query_layer", "key_layer", "value_layer"};
    for (int i = 0; i < 3; ++i) {
        w[i] = find(e, m + names[i] + ".weight"); b[i] = find(e, m + names[i] + ".bias");
        if (!sized(w[i], D * D) || !sized(b[i], D)) { if (missing) *missing = m + names[i]; return false; }
    }
    return true;
}

int pack_front_end(EcEncoder* e) {
    const EcConfig& c = e->cfg;
    const int C = c.sub_filters[0], N = e->blocks[0].dim_model;
    std::string err;
    std::vector<double> taps; std::vector<float> tbias;
    if (!fold_front_conv(e, &taps, &tbias, &err)) return fail(err);
    e->sub_w9 = upload(e, std::vector<float>(taps.begin(), taps.end())); e->sub_b = upload(e, tbias);
    if (c.sub_layers == 1) {
        if (!pack_named_linear(e, "linear", N, C * (c.n_mels / 2), &e->lin, &err)) return fail(err);
    } else {
        const int C1 = c.sub_filters[1], F2 = c.n_mels / 4, K = C1 * F2;
        const HostTensor *w2 = find(e, "subsampling_module.layers.1.0.weight"), *b2 = find(e, "subsampling_module.layers.1.0.bias");
        std::vector<float> sc2, sh2, bf;
        std::vector<double> wf;
        if (!b2 || !sized(w2, (int64_t)C1 * C * 9)) return fail("missing subsampling layer-2 conv weights");
        if (!bn_fold(e, "subsampling_module.layers.1.1", C1, &sc2, &sh2, &err)) return fail(err);
        conv_bn_fold(fdata(w2), fdata(b2), sc2, sh2, C1, C * 9, &wf, &bf);
        e->sub2_w = upload(e, sub2_conv_image(wf, C1, C)); e->sub2_b = upload(e, padded(bf, ec_round_up(C1, 128))); e->sub2_cp = ec_round_up(C, 64);
        const HostTensor *lw = find(e, "linear.weight"), *lb = find(e, "linear.bias");
        if (!lb || !sized(lw, (int64_t)N * K)) return fail("missing / mis-shaped linear.weight");
        const std::vector<float> perm = linear_f2c(fdata(lw), N, C1, F2);
        if (!put_linear(e, pack_linear(row_ptrs(perm.data(), N, K), lb->data, K), &e->lin)) return fail("upload failed");
    }
    e->lin_rs = nullptr; e->conv_tab = nullptr;
    if (c.sub_layers != 1) return 0;
    const int F2 = c.n_mels / 2;
    const HostTensor *lw = find(e, "linear.weight"), *lb = find(e, "linear.bias");
    if (sublinear_fused_supported(c.n_mels, N)) { e->lin_fused = upload(e, sublinear_image(fdata(lw), N, C, F2)); e->lin_fused_ld = (F2 / 8) * ec_round_up(C, 8) * 8; }
    if (const int CGr = sublinear2_groups(c.n_mels, C, N)) {
        Img wr; std::vector<float> tab;
        sublinear2_images(fdata(lw), taps, tbias, N, C, F2, CGr, &wr, &tab);
        e->lin_rs = upload(e, wr); e->conv_tab = upload(e, tab);
    }
    // sublinear3.hip: any channel count / width up to 384
    e->sub3 = SubChunkImg{};
    if (const int nt3 = sub_chunked_tiles(N)) {
        Img cimg, wimg; std::vector<float> bp;
        front_chunks(taps, tbias, fdata(lw), fdata(lb), C, F2, N, nt3, bf16_pair_trunc, bf16_single, 1, &cimg, &wimg, &bp);
        e->sub3 = SubChunkImg{upload(e, cimg), upload(e, wimg), upload(e, bp), (C + 31) / 32, F2};
    }
    return 0;
}

int pack_block(EcEncoder* e, size_t k, std::map<std::pair<int, int>, const bf16_t*>* tables) {
    const EcBlock& b = e->blocks[k];
    BlockW& W = e->bw[k];
    const int D = b.dim_model, De = b.dim_expand, F1 = D * b.ff_ratio, F2 = De * b.ff_ratio;
    const std::string p = "blocks." + std::to_string(k), ff1 = p + ".feed_forward_module1.layers", ff2 = p + ".feed_forward_module2.layers";
    std::string err;
    bool ok = get_ln(e, ff1 + ".0", D, &W.ln_ffn1, &err) && pack_named_linear(e, ff1 + ".1", F1, D, &W.ffn1_a, &err) && pack_named_linear(e, ff1 + ".4", D, F1, &W.ffn1_b, &err) &&
              get_ln(e, ff2 + ".0", De, &W.ln_ffn2, &err) && pack_named_linear(e, ff2 + ".1", F2, De, &W.ffn2_a, &err) && pack_named_linear(e, ff2 + ".4", De, F2, &W.ffn2_b, &err) &&
              get_ln(e, p + ".norm", De, &W.ln_out, &err);
    if (!ok) return fail(err);
    const float *w1b = fdata(find(e, ff1 + ".4.weight")), *w2b = fdata(find(e, ff2 + ".4.weight"));      // [D][F1], [De][F2]: checked by pack_named_linear above
    W.ffn1_bp = upload(e, pack_ffn2_permuted(w1b, D, F1, 1.0f));
    W.ffn2_bp = upload(e, pack_ffn2_permuted(w2b, De, F2, 1.0f));
    if (!W.ffn1_bp || !W.ffn2_bp) return fail("upload failed");
    const std::string m = p + ".multi_head_self_attention_module";
    if (!get_ln(e, m + ".norm", D, &W.ln_att, &err)) return fail(err);
    {
        const HostTensor *wq[3], *bq[3];
        if (!find_qkv(e, m + ".mhsa.", D, wq, bq, &err)) return fail("missing " + err);
        std::vector<const float*> rows; std::vector<float> bias;
        stack_qkv(wq, bq, D, D, &rows, &bias);
        if (!put_linear(e, pack_linear(rows, bias, D), &W.qkv)) return fail("upload failed");
        // natural-layout variant for the row-stationary kernel: rows in accumulator order inside every chunk of 32, so that a lane's
        // accumulators are row-contiguous runs of 8 columns
        const int np = ec_round_up(3 * D, 32);
        std::vector<const float*> prow(np, nullptr); std::vector<float> pbias(np, 0.f);
        for (int n = 0; n < np; ++n)
            if (acc16(n) < 3 * D) { prow[n] = rows[acc16(n)]; pbias[n] = bias[acc16(n)]; }
        if (!put_linear_and_chain(e, prow, pbias, D, m + ".norm", &W.qkv_nat, &W.c_qkv)) return fail("upload failed");      // chain: attention pre-norm folded in
        W.qkv_nat.N = 3 * D; W.c_qkv_chunks = chain_supported(D) ? ec_cdiv(3 * D, 64) : 0;
    }
    // fused row-local chains (chain.hip): the D-wide part of the block - FFN1, attention output projection (pointwise-1 below) - and the De-wide part - pointwise-2, FFN2
    for (int part = 0; part < 2; ++part) {
        const int Dw = part ? De : D, F = part ? F2 : F1;
        if (!chain_supported(Dw)) continue;
        const std::string& ff = part ? ff2 : ff1;
        const HostTensor* b2 = find(e, ff + ".4.bias");
        if (!b2 || !pack_named_linear(e, ff + ".1", F, Dw, part ? &W.c_f2a : &W.c_f1a, &err, true, ff + ".0") ||
            !pack_named_linear(e, part ? p + ".convolution_module.layers.7" : m + ".mhsa.output_layer", Dw, Dw, part ? &W.c_pw2 : &W.c_outp, &err, true)) return fail("chain packing failed: " + err);
        const bf16_t* wb = upload(e, pack_ffn2_permuted(part ? w2b : w1b, Dw, F, 0.5f));
        const bf16_t* wcm = chain3_supported(Dw) ? upload(e, pack_ffn2_chunkmajor(part ? w2b : w1b, Dw, F, 0.5f, chain_padded_width(Dw))) : nullptr;
        const std::vector<float> hb = padded(b2->data, (int)b2->data.size(), 0.5f);
        const float* hbd = upload(e, hb);
        (part ? W.c_f2b : W.c_f1b) = wb; (part ? W.c_f2b_cm : W.c_f1b_cm) = wcm; (part ? W.c_f2b2 : W.c_f1b2) = hbd; (part ? W.h_f2b2 : W.h_f1b2) = hb;
        if (part) {
            const HostTensor *og = find(e, p + ".norm.weight"), *ob = find(e, p + ".norm.bias");
            if (!og || !ob) return fail("missing " + p + ".norm");
            W.h_ln_out_g = og->data; W.h_ln_out_b = ob->data;
        }
        if (!wb || !hbd || (chain3_supported(Dw) && !wcm)) return fail("upload failed");
        (part ? W.chain_out : W.chain_in) = true;
    }
    if (!pack_named_linear(e, m + ".mhsa.pos_layer", D, D, &W.pos, &err)) return fail(err);
    if (!pack_named_linear(e, m + ".mhsa.output_layer", D, D, &W.outp, &err)) return fail(err);
    const HostTensor *u = find(e, m + ".mhsa.u"), *v = find(e, m + ".mhsa.v");
    if (!u || !v || (int)u->data.size() != D) return fail("missing " + m + ".mhsa.u/v");
    W.u = upload(e, u->data); W.v = upload(e, v->data);
    W.h_u = u->data; W.h_v = v->data;
    W.dvu_ld = ec_round_up(b.group_size * D / b.num_heads, 32);
    W.dvu = upload(e, dvu_table(fdata(u), fdata(v), b.num_heads, b.group_size * D / b.num_heads, D, W.dvu_ld));
    auto key = std::make_pair(b.max_pos, D);
    if (!tables->count(key)) { Img t; build_pos_table(b.max_pos, D, &t, nullptr); (*tables)[key] = upload(e, t); }
    W.pos_table = (*tables)[key];
    // ---- convolution module
    const std::string cm = p + ".convolution_module.layers";
    if (!get_ln(e, cm + ".0", D, &W.ln_conv, &err)) return fail(err);
    {
        const HostTensor *w = find(e, cm + ".2.weight"), *bb = find(e, cm + ".2.bias");
        if (!bb || !sized(w, 2 * De * D)) return fail("missing " + cm + ".2");
        std::vector<const float*> rows; std::vector<float> bias;
        glu_interleave(fdata(w), fdata(bb), De, D, &rows, &bias);
        if (!put_linear_and_chain(e, rows, bias, D, cm + ".0", &W.pw1, &W.c_pw1)) return fail("upload failed");             // chain: conv-module pre-norm folded in
        W.c_pw1_chunks = chain_supported(D) ? ec_cdiv(De, 32) : 0;
    }
    {   // depthwise (De, 1, k) + BatchNorm1d fold -> [k][De] fp32
        const int ks = b.kernel_size;
        const HostTensor *w = find(e, cm + ".4.weight"), *bb = find(e, cm + ".4.bias");
        std::vector<float> sc, sh, bz, wk((size_t)ks * De);
        std::vector<double> wf;
        if (!bb || !sized(w, De * ks)) return fail("missing " + cm + ".4");
        if (!bn_fold(e, cm + ".5", De, &sc, &sh, &err)) return fail(err);
        conv_bn_fold(fdata(w), fdata(bb), sc, sh, De, ks, &wf, &bz);
        // The matrix-pipe kernel holds every folded tap as a bf16 hi + lo pair: 2^-18 of the tap is lost, sigma = 2^-18 / sqrt(3) * |taps|_2 * rms(x) on the
        // pre-activation.  The stage's contract (oracle/ref_bf16.py, tests/test_gpu_bf16_rounding.py) leaves 2e-5 absolute on the output, 4e-5 on the
        // pre-activation where Swish has slope 1/2; five sigma inside that at rms(GLU) = 0.6 means |taps|_2 <= 6 per channel.  Initialised and synthetic
        // weights sit at 1.5 - 2.4; BatchNorm statistics of a trained-like profile fold to 12 - 800: those blocks get a third tap plane (one more MFMA per
        // tap group on the same kernel; taps exact to 2^-27)
        float tap_norm = 0.f;
        for (int ch = 0; ch < De; ++ch) {
            double n2 = 0.0;
            for (int j = 0; j < ks; ++j) { const float t = (float)wf[(size_t)ch * ks + j]; wk[(size_t)j * De + ch] = t; n2 += (double)t * t; }
            tap_norm = std::max(tap_norm, (float)std::sqrt(n2));
        }
        W.dw_w = upload(e, wk); W.dw_b = upload(e, bz);
        if (dwconv_mfma_supported(ks, b.conv_stride)) {
            Img ta((size_t)De * 4 * dwconv_mfma_groups(ks) * 8);
            pack_dwconv_mfma(wk.data(), ks, De, ta.data());
            if (tap_norm > kDwMfmaTwoPlaneNorm) {
                Img t3((size_t)De * 4 * dwconv_mfma_groups(ks) * 4);
                pack_dwconv_mfma3(wk.data(), ks, De, t3.data());
                W.dw_a3 = upload(e, t3);
                if (!W.dw_a3) return fail("upload failed");
            }
            W.dw_a = upload(e, ta);
            if (!W.dw_a) return fail("upload failed");
        }
    }
    if (!pack_named_linear(e, cm + ".7", De, De, &W.pw2, &err)) return fail(err);
    if (D != De && !pack_named_linear(e, p + ".conv_res.1", De, D, &W.res, &err, false, "", De)) return fail(err);
    return 0;
}

int pack_blocks(EcEncoder* e) {
    e->bw.assign(e->blocks.size(), BlockW());
    std::map<std::pair<int, int>, const bf16_t*> tables;
    std::vector<int> strides, gs, hs;
    for (size_t k = 0; k < e->blocks.size(); ++k) {
        if (int rc = pack_block(e, k, &tables)) return rc;
        strides.push_back(e->blocks[k].conv_stride); gs.push_back(e->blocks[k].group_size); hs.push_back(e->blocks[k].num_heads);
    }
    e->block_stride = upload(e, strides); e->block_group = upload(e, gs); e->block_heads = upload(e, hs);
    return 0;
}

int pack_chain_consts(EcEncoder* e) {
    for (size_t k = 0; k < e->blocks.size(); ++k) {
        BlockW& W = e->bw[k];
        const EcBlock& b = e->blocks[k];
        const int D = b.dim_model, De = b.dim_expand;
        if (W.chain_in) {
            W.cc_b = upload(e, chain_const_block(CHAIN_B, D, &W, nullptr, &b, nullptr));
            if (chain_head_supported(D)) W.cc_head = upload(e, chain_const_block(CHAIN_A_HEAD, D, nullptr, &W, nullptr, &b));
        }
        if (W.chain_out && chain_tail_supported(De)) {
            W.cc_tail = upload(e, chain_const_block(CHAIN_A_TAIL, De, &W, nullptr, &b, nullptr));
            // The forward's rule (routes.h tail_route) with "the width has a chain3.hip instance" for its chain_pair_on: with chain_pair = 0 set before finalize
            // and chain_full_max < De the block is built and no forward reads it (kept: the option may be set back without a second finalize)
            if (chain_full_fits(e, k, chain3_supported(De)))
                W.cc_full = upload(e, chain_const_block(CHAIN_A_FULL, De, &W, &e->bw[k + 1], &b, &e->blocks[k + 1]));
        }
    }
    return 0;
}

// Self-conditioned CTC: per listed block k the two images of interctc.hip (kernels.h: InterCtcParams) - linear_expand_k [V][De] as a plain packed Linear whose
// rows are at least as wide as the kernel instance reads them, linear_proj_k [De][V] padded to that instance's row count with its K (vocabulary) index in
// accumulator order - and the fp32 biases.  The label-exact modes find the same tensors by prefix (pack_fp32_tensors, pack_split_modules)
int pack_interctc(EcEncoder* e) {
    e->ic_w.assign(e->ic_blocks.size(), EcEncoder::InterCtcW());
    const int V = e->ic_vocab;
    for (size_t i = 0; i < e->ic_blocks.size(); ++i) {
        const size_t k = (size_t)e->ic_blocks[i];
        const int De = e->blocks[k].dim_expand;
        if (interctc_route(e, k) == IC_REFUSED) return fail(interctc_refusal(e, k));
        const std::string ex = "linear_expand_" + std::to_string(k), pr = "linear_proj_" + std::to_string(k);
        const HostTensor *we = find(e, ex + ".weight"), *be = find(e, ex + ".bias"), *wp = find(e, pr + ".weight"), *bp = find(e, pr + ".bias");
        if (!we) return fail("missing tensor " + ex + ".weight");
        if (!be) return fail("missing tensor " + ex + ".bias");
        if (!wp) return fail("missing tensor " + pr + ".weight");
        if (!bp) return fail("missing tensor " + pr + ".bias");
        if (!sized(we, (int64_t)V * De) || !sized(be, V)) return fail("shape mismatch for " + ex);
        if (!sized(wp, (int64_t)V * De) || !sized(bp, De)) return fail("shape mismatch for " + pr);
        const int cols = 16 * interctc_ks_class(De);          // columns of We / rows of Wp the kernel instance of this width streams
        EcEncoder::InterCtcW& W = e->ic_w[i];
        if (!put_linear(e, pack_linear(row_ptrs(fdata(we), V, De), be->data, De, false, nullptr, nullptr, cols), &W.expand)) return fail("upload failed");
        std::vector<const float*> rows(cols, nullptr);
        for (int n = 0; n < De; ++n) rows[n] = fdata(wp) + (size_t)n * V;
        const Linear L = pack_linear(rows, {}, V, true);
        W.proj = upload(e, L.w); W.proj_ld = L.ldw; W.proj_b = upload(e, padded(bp->data, cols));
        if (!W.proj || !W.proj_b) return fail("upload failed");
    }
    return 0;
}

int pack_ctc_head(EcEncoder* e) {
    const HostTensor *w = find(e, "fc.weight"), *b = find(e, "fc.bias");
    const int D = e->blocks.back().dim_expand, V = e->cfg.vocab_size;
    if (V <= 0 || !w || !b) return 0;
    if ((int)w->data.size() != V * D) return fail("fc.weight shape mismatch");
    std::vector<float> wt; Img hi, lo;
    ctc_head_images(fdata(w), V, D, &wt, &hi, &lo);
    e->fc_wt = upload(e, wt); e->fc_b = upload(e, b->data); e->fc_hi = upload(e, hi); e->fc_lo = upload(e, lo);
    return 0;
}

int pack_mel_tables(EcEncoder* e) {
    const std::string err = mel_config_error(e->cfg);
    if (!err.empty()) return fail(err);
    const MelHost t = build_mel_tables(e->cfg);
    e->mel.window = upload(e, t.window); e->mel.twiddle = upload(e, t.twiddle);
    e->mel.fb_start = upload(e, t.fb_start); e->mel.fb_count = upload(e, t.fb_count); e->mel.fb_offset = upload(e, t.fb_offset);
    e->mel.fb_nnz = (int)t.fb_weight.size(); e->mel.fb_weight = upload(e, t.fb_weight);
    return e->mel.window && e->mel.twiddle && e->mel.fb_weight ? 0 : fail("");
}

// fp32-operand mode: the reference-layout fp32 tensors themselves, BatchNorm scale / shift (+ scaled conv bias) of the subsampling convs
int pack_fp32_tensors(EcEncoder* e) {
    std::string err;
    for (auto& kv : e->host) e->xw[kv.first] = upload(e, kv.second.data);
    for (int l = 0; l < e->cfg.sub_layers; ++l) {
        const std::string sp = "subsampling_module.layers." + std::to_string(l);
        const int C = e->cfg.sub_filters[l];
        const HostTensor* cbias = find(e, sp + ".0.bias");
        std::vector<float> sc, sh, shift;
        if (!sized(cbias, C) || !bn_fold(e, sp + ".1", C, &sc, &sh, &err)) return fail("exact mode: " + err);
        conv_bn_fold(nullptr, fdata(cbias), sc, sh, C, 0, nullptr, &shift);
        e->xsub_scale[l] = upload(e, sc); e->xsub_shift[l] = upload(e, shift);
    }
    return 0;
}

int pack_fp32_tables(EcEncoder* e) {       // fp32 sinusoid tables
    for (const EcBlock& b : e->blocks) {
        auto key = std::make_pair(b.max_pos, b.dim_model);
        if (e->xtab.count(key)) continue;
        std::vector<float> t;
        build_pos_table(b.max_pos, b.dim_model, nullptr, &t);
        e->xtab[key] = upload(e, t);
    }
    return 0;
}

// split mode, per-module kernels (split.hip): every 2-D weight as two fp16 images; the three attention projections of a block additionally stacked (q | k | v).
// The first tensor with an element the images cannot hold fails finalize
int pack_split_modules(EcEncoder* e) {
    std::string range_err;
    auto add_split = [&](const std::string& prefix, const std::vector<const float*>& rows, int K) {
        Img hi, lo; int n = 0, k = 0;
        if (split_pair_image(rows, K, &hi, &lo, &n, &k))
            e->xsplit[prefix] = EcEncoder::SplitW{upload(e, hi), upload(e, lo), ec_round_up(K, 32)};
        else if (range_err.empty())
            range_err = "split mode: " + prefix + ".weight[" + std::to_string(n) + "][" + std::to_string(k) + "] = " + std::to_string(rows[n][k]) + " is outside the split images' range |w| < 65000";
    };
    for (auto& kv : e->host) {
        const std::string& key = kv.first;
        const HostTensor& t = kv.second;
        if (key.size() < 8 || key.compare(key.size() - 7, 7, ".weight") != 0) continue;
        const bool lin = t.shape.size() == 2, pw = t.shape.size() == 3 && t.shape[2] == 1 && key.find("subsampling") == std::string::npos;
        if (!lin && !pw) continue;
        const int N = (int)t.shape[0], K = (int)t.shape[1];
        if (K % 4 || key == "fc.weight") continue;
        add_split(key.substr(0, key.size() - 7), row_ptrs(t.data.data(), N, K), K);
    }
    for (size_t k = 0; k < e->blocks.size(); ++k) {
        const std::string m = "blocks." + std::to_string(k) + ".multi_head_self_attention_module.mhsa.";
        const int D = e->blocks[k].dim_model;
        const HostTensor *wq[3], *bq[3];
        if (!find_qkv(e, m, D, wq, bq)) continue;
        std::vector<const float*> rows; std::vector<float> bias;
        stack_qkv(wq, bq, D, D, &rows, &bias);
        add_split(m + "qkv_layer", rows, D);
        e->xw[m + "qkv_layer.bias"] = upload(e, bias);
    }
    return range_err.empty() ? 0 : fail(range_err);
}

// split mode: images of the fused front end (sxf_sub.hip; kernels.h: SubChunkParams) - one-layer subsampler only; a folded value the image cannot hold: no fused
// front end (per-module kernels)
int pack_split_front_end(EcEncoder* e) {
    const EcConfig& c = e->cfg;
    if (c.sub_layers != 1) return 0;
    const int Co = c.sub_filters[0], Fo = (c.n_mels - 1) / 2 + 1, N = e->blocks[0].dim_model, nt = sub_chunked_tiles(N);
    const HostTensor *lw = find(e, "linear.weight"), *lb = find(e, "linear.bias");
    std::vector<double> taps; std::vector<float> tbias, bp; std::string err;
    Img cimg, wimg;
    if (!nt || !sized(lw, (int64_t)N * Co * Fo) || !sized(lb, N) || !fold_front_conv(e, &taps, &tbias, &err)) return 0;
    if (!front_chunks(taps, tbias, fdata(lw), fdata(lb), Co, Fo, N, nt, f16_pair_s10, f16_pair_s10, 2, &cimg, &wimg, &bp)) return 0;
    e->xsub = SubChunkImg{upload(e, cimg), upload(e, wimg), upload(e, bp), (Co + 31) / 32, Fo};
    return 0;
}

// One FeedForwardModule for sxf_chain.hip: its image xc_f[which], b2 / 2 and the chunk count.  Nothing is set where the width is not built, a tensor is missing
// or mis-shaped, or a folded value is beyond the image's range: that FFN runs as LayerNorm + two split GEMMs, and no chain of its side is built
void pack_split_ffn(EcEncoder* e, size_t k, int which) {
    const int D = which ? e->blocks[k].dim_expand : e->blocks[k].dim_model, F = D * e->blocks[k].ff_ratio;
    const std::string pf = "blocks." + std::to_string(k) + (which ? ".feed_forward_module2.layers." : ".feed_forward_module1.layers.");
    const HostTensor *g = find(e, pf + "0.weight"), *bt = find(e, pf + "0.bias"), *w1 = find(e, pf + "1.weight"), *b1 = find(e, pf + "1.bias"), *w2 = find(e, pf + "4.weight"), *b2 = find(e, pf + "4.bias");
    if (!sxc_supported(D) || !sized(g, D) || !sized(bt, D) || !sized(w1, (int64_t)F * D) || !sized(b1, F) || !sized(w2, (int64_t)F * D) || !sized(b2, D)) return;
    const Img img = ffn_image(fdata(g), fdata(bt), fdata(w1), fdata(b1), fdata(w2), D, F);
    if (img.empty()) return;
    int ks, nt; sxc_shape(D, &ks, &nt);
    BlockW& W = e->bw[k];
    W.xf_b2[which] = upload(e, padded(b2->data, 32 * nt, 0.5f)); W.xf_nch[which] = (F + 31) / 32; W.xc_f[which] = upload(e, img);
}

// split mode: weight images of the split chains (sxf_chain.hip; kernels.h: SxcBParams / SxcAParams), all in accumulator order - every operand of a product is a
// converted accumulator tile: out-proj / pointwise-2 (F2 chunks), pointwise-1 with GLU row pairs / Q | K | V (F1 chunks, pre-norm folded), the two FFN modules.
// A part with a folded value its images cannot hold is not built; xc_in / xc_out: every image of that side exists.  An FFN image stands on its own - the module
// runs as the chain kernel's FFN-only form where its siblings were refused
int pack_split_chains(EcEncoder* e) {
    for (size_t k = 0; k < e->blocks.size(); ++k) {
        const EcBlock& b = e->blocks[k];
        BlockW& W = e->bw[k];
        const int D = b.dim_model, De = b.dim_expand;
        const std::string pb = "blocks." + std::to_string(k), mh = pb + ".multi_head_self_attention_module.", cm = pb + ".convolution_module.layers.";
        pack_split_ffn(e, k, 0); pack_split_ffn(e, k, 1);
        const HostTensor *wo = find(e, mh + "mhsa.output_layer.weight"), *bo = find(e, mh + "mhsa.output_layer.bias"), *lg = find(e, cm + "0.weight"), *lb = find(e, cm + "0.bias"),
                         *w1 = find(e, cm + "2.weight"), *b1 = find(e, cm + "2.bias"), *ag = find(e, mh + "norm.weight"), *ab = find(e, mh + "norm.bias"), *wq[3], *bq[3];
        if (sxc_supported(D) && sized(wo, D * D) && sized(bo, D) && sized(lg, D) && sized(lb, D) && sized(w1, (int64_t)2 * De * D) && sized(b1, 2 * De) &&
            sized(ag, D) && sized(ab, D) && find_qkv(e, mh + "mhsa.", D, wq, bq)) {
            int ks, nt; sxc_shape(D, &ks, &nt);
            const int DP1 = 16 * ks, DP2 = 32 * nt, nte = (De + 31) / 32;
            Img io((size_t)nt * 64 * DP2, 0), ip((size_t)2 * nte * 64 * DP1, 0), iq((size_t)3 * nt * 64 * DP1, 0);
            std::vector<const float*> prow, qrow; std::vector<float> pbias, qbias;
            glu_interleave(fdata(w1), fdata(b1), De, D, &prow, &pbias);          // chunk 2 j: value rows 32 j .., chunk 2 j + 1: their gate rows De + 32 j ..
            stack_qkv(wq, bq, D, 32 * nt, &qrow, &qbias);
            if (f2_chunk(io, 0, (size_t)64 * DP2, DP2, nt, fdata(wo), D, D, 1.0) && f1_chunk(ip, 0, (size_t)64 * DP1, DP1, D, prow, pbias, fdata(lg), fdata(lb)) &&
                f1_chunk(iq, 0, (size_t)64 * DP1, DP1, D, qrow, qbias, fdata(ag), fdata(ab))) {
                W.xc_wo = upload(e, io); W.xc_bo = upload(e, padded(bo->data, DP2)); W.xc_p1 = upload(e, ip); W.xc_nch_p1 = 2 * nte; W.xc_qkv = upload(e, iq);
                W.xc_in = W.xc_f[0] != nullptr;
            }
        }
        if (sxc_supported(De)) {
            int ks, nt; sxc_shape(De, &ks, &nt);
            const int DP2 = 32 * nt;
            const HostTensor *w2 = find(e, cm + "7.weight"), *b2 = find(e, cm + "7.bias");
            Img i2((size_t)nt * 64 * DP2, 0);
            if (sized(w2, (int64_t)De * De) && sized(b2, De) && f2_chunk(i2, 0, (size_t)64 * DP2, DP2, nt, fdata(w2), De, De, 1.0)) {
                W.xc_p2 = upload(e, i2); W.xc_bp2 = upload(e, padded(b2->data, DP2));
                W.xc_out = W.xc_f[1] != nullptr;
            }
        }
    }
    return 0;
}

}  // namespace

int pack_encoder(EcEncoder* e) {
    int rc;
    if ((rc = pack_front_end(e)) || (rc = pack_blocks(e)) || (rc = pack_chain_consts(e)) || (rc = pack_interctc(e)) || (rc = pack_ctc_head(e)) || (rc = pack_mel_tables(e))) return rc;
    e->xw.clear(); e->xtab.clear();
    if (!e->exact_pack) return 0;
    if ((rc = pack_fp32_tensors(e))) return rc;
    e->xsplit.clear();
    e->xsub = SubChunkImg{};
    if (e->exact_split && ((rc = pack_split_front_end(e)) || (rc = pack_split_modules(e)) || (rc = pack_split_chains(e)))) return rc;
    return pack_fp32_tables(e);
}
