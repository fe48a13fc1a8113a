// bf16 MFMA GEMM with fused epilogues for the Conformer encoder (gfx950).
//
//   C[m, n] = sum_k A[m, k] * W[n, k] + bias[n]
//
// Replaces every nn.Linear / pointwise Conv1d on the hot path of the reference
// (models/layers.py:57-67, 122-136; call sites modules.py:378-382, 502-508, attentions.py:57-60, 471;
// encoders.py:116) together with the element-wise op that follows it (Swish, GLU, residual add,
// +u of attentions.py:674-686; the head split is index arithmetic in the attention kernels).
//
// Tiling: 128 x BN x 64 block tile, 4 waves (2x2), each wave 64 x BN/2 built from
// v_mfma_f32_32x32x16_bf16; register-staged global->LDS double buffer with one barrier per k-tile;
// LDS rows padded by 16 B (row stride 144 B = 9 x 16 B slots, conflict-free for ds_read_b128).
// M is large (B*T), N and K are small/odd multiples of 4: A tail chunks are masked in registers,
// weights are zero-padded once at pack time.
#include "gemm_epilogue.h"

namespace {

constexpr int BM = 128;
constexpr int BK = 64;
constexpr int LROW = BK * 2 + 16;   // bytes per LDS row

struct GemmDev {
    GemmParams p;
    FastDiv32 fD;         // EPI_QKV_NAT: stacked Q | K | V column -> tensor
    bool staged;          // the output leaves through the LDS-staged 16-byte-piece epilogue (gemm_staged_ok)
};

template <int BN, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_kernel(const GemmDev gd) {
    const GemmParams& p = gd.p;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sA = smem;                       // [2][BM][LROW]
    char* sB = smem + 2 * BM * LROW;       // [2][BN][LROW]
    constexpr int NB = BN / 32;            // B chunks per thread
    constexpr int NF = BN / 64;            // 32-col fragments per wave

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int n_tiles = (p.N + BN - 1) / BN;
    const int m_tiles = (p.M + BM - 1) / BM;
    const int id = xcd_remap(blockIdx.x, m_tiles * n_tiles);
    const int tm = id / n_tiles, tn = id - tm * n_tiles;
    const int m0 = tm * BM, n0 = tn * BN;

    // ---- staging addresses (constant over the k loop)
    const int srow = tid >> 3, kc = tid & 7;
    const bf16_t* a_ptr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int m = m0 + srow + 32 * i;
        m = m < p.M ? m : p.M - 1;
        size_t src = m;
        if (p.a_rows > 0) {
            int b = m / p.a_rows, r = m - b * p.a_rows;
            src = (size_t)b * p.a_pitch + (size_t)r * p.a_stride;
        }
        a_ptr[i] = p.A + src * p.lda;
    }
    const bf16_t* b_ptr[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) b_ptr[i] = p.W + (size_t)(n0 + srow + 32 * i) * p.ldw + kc * 8;

    f32x16 acc[2][NF];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < NF; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    const int nk = (p.K + BK - 1) / BK;
    const int frag_off = (lane & 31) * LROW + (lane >> 5) * 16;
    // Two register staging sets: the global loads of k-tile kt+2 are issued at the top of iteration kt and published (written to
    // LDS) at the bottom of iteration kt+1, so they have a whole iteration to arrive.  (One set - issue at the top, publish at the
    // bottom of the SAME iteration - left only one 16-MFMA compute phase to cover the L2 / HBM latency.)
    struct Stage { uint4 ra[4], rb[NB]; int valid, tail; };
    Stage s0, s1;
#pragma unroll
    for (int i = 0; i < 4; ++i) { s0.ra[i] = make_uint4(0, 0, 0, 0); s1.ra[i] = s0.ra[i]; }
#pragma unroll
    for (int i = 0; i < NB; ++i) { s0.rb[i] = make_uint4(0, 0, 0, 0); s1.rb[i] = s0.rb[i]; }
    s0.valid = s1.valid = 0;
    s0.tail = s1.tail = 1;
    auto load_tile = [&](Stage& st, int t) __attribute__((always_inline)) {
        const int k = t * BK + kc * 8;
        const int valid = p.K - k;
        const int kcl = k < p.lda - 8 ? k : p.lda - 8;          // unconditional, clamped (in-bounds) loads; masked below
        const int tb = t < nk ? t : nk - 1;                     // weight tiles past the end: harmless re-read, never published
#pragma unroll
        for (int i = 0; i < 4; ++i) st.ra[i] = *reinterpret_cast<const uint4*>(a_ptr[i] + (kcl < 0 ? 0 : kcl));
#pragma unroll
        for (int i = 0; i < NB; ++i) st.rb[i] = *reinterpret_cast<const uint4*>(b_ptr[i] + tb * BK);
        st.tail = t >= nk - 1;
        st.valid = valid;          // the K tail is masked at PUBLISH time: masking here made every iteration wait for the loads it had
                                   // just issued (s_waitcnt vmcnt right after them: one L2 round trip per k-tile, 20 % of MFMA peak)
    };
    auto publish = [&](const Stage& st, int buf) __attribute__((always_inline)) {
        char* a = sA + buf * BM * LROW;
        char* b = sB + buf * BN * LROW;
        // only the last k-tile can hold columns >= K: wave-uniform branch (the 64 mask instructions were ~15 % of a k-tile's issue slots)
        if (__builtin_amdgcn_readfirstlane(st.tail)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<uint4*>(a + (srow + 32 * i) * LROW + kc * 16) = mask_chunk(st.ra[i], st.valid);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<uint4*>(a + (srow + 32 * i) * LROW + kc * 16) = st.ra[i];
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) *reinterpret_cast<uint4*>(b + (srow + 32 * i) * LROW + kc * 16) = st.rb[i];
    };
    auto compute = [&](int buf) __attribute__((always_inline)) {
        const char* a = sA + buf * BM * LROW + (wm * 64) * LROW + frag_off;
        const char* b = sB + buf * BN * LROW + (wn * (BN / 2)) * LROW + frag_off;
#pragma unroll
        for (int kk = 0; kk < BK / 16; ++kk) {
            bf16x8 af[2], bf[NF];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) af[mi] = *reinterpret_cast<const bf16x8*>(a + mi * 32 * LROW + kk * 32);
#pragma unroll
            for (int ni = 0; ni < NF; ++ni) bf[ni] = *reinterpret_cast<const bf16x8*>(b + ni * 32 * LROW + kk * 32);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < NF; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
        }
    };
    load_tile(s0, 0);
    load_tile(s1, 1);
    publish(s0, 0);
    __syncthreads();
    for (int kt = 0; kt < nk; kt += 2) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {            // h = 0: tile kt in buffer 0, tile kt+1 waiting in s1, tile kt+2 -> s0;  h = 1: roles swapped
            const int t = kt + h;
            if (t < nk) {
                // UNCONDITIONAL (tiles past the end re-read a clamped tile and are never published): with `if (t + 2 < nk)` the
                // compiler has to cover the path without these 8 younger loads and waits vmcnt(7..0) at the publish below instead
                // of vmcnt(15..8) - i.e. for the loads just issued, which removes the second stage of the prefetch
                if (h == 0) load_tile(s0, t + 2); else load_tile(s1, t + 2);
                compute(h);
                if (t + 1 < nk) { if (h == 0) publish(s1, 1); else publish(s0, 0); }
                __syncthreads();
            }
        }
    }

    // ---- epilogue.  C layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    const int lcol = lane & 31, lrow = 4 * (lane >> 5);
    if constexpr (EPI != EPI_F32) {
        if (gd.staged) {       // gemm_epilogue.h: all 64 rows of the wave's tile staged at once
            constexpr int STAGE = 64 * EpiStage<NF, EPI>::PITCH;
            static_assert(4 * STAGE <= 2 * (BM + BN) * LROW, "staging fits the operand buffers");
            __syncthreads();                                   // every wave is done with the last k-tile
            staged_epilogue<NF, EPI, 64>(acc, p, gd.fD, smem + wave * STAGE, m0 + wm * 64, n0 + wn * (BN / 2), lane);
            return;
        }
    }
    // unstaged fallbacks (ldc, D or a pointer fails the 16-byte rules) and EPI_F32: one store per element
    if constexpr (EPI == EPI_GLU_BF16) {
        static_assert(BN == 128, "GLU needs both halves in one wave");
        const int j = (n0 + wn * 64) / 2 + lcol;           // output channel
        const float ba = p.bias[n0 + wn * 64 + lcol], bb = p.bias[n0 + wn * 64 + 32 + lcol];
        bf16_t* C = reinterpret_cast<bf16_t*>(p.C);
        if (j < p.ldc) {
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    int m = m0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + lrow;
                    if (m < p.M) C[(size_t)m * p.ldc + j] = f2bf((acc[mi][0][r] + ba) * sigmoidf_(acc[mi][1][r] + bb));
                }
        }
    } else if constexpr (EPI == EPI_QKV_NAT) {
        // natural layout: out[which][(b*Tp + t)][nn], which = n / D; rows m = (b, t)
        const int Tp = p.Tp;
        int b0 = (m0 + wm * 64) / p.T, t0 = (m0 + wm * 64) - b0 * p.T;
#pragma unroll
        for (int ni = 0; ni < NF; ++ni) {
            const int n = n0 + wn * (BN / 2) + ni * 32 + lcol;
            if (n >= p.N) continue;
            const int which = gd.fD.div(n), nn = n - which * p.D;
            const float bias = p.bias[n];
            const float bu = which == 0 ? p.u[nn] : 0.f;
            bf16_t* dst = which == 1 ? p.kh : (which == 2 ? p.vt : p.qu);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rr = mi * 32 + (r & 3) + 8 * (r >> 2) + lrow;
                    if (m0 + wm * 64 + rr >= p.M) continue;
                    int b = b0, t = t0 + rr;
                    while (t >= p.T) { t -= p.T; ++b; }
                    const size_t idx = ((size_t)b * Tp + t) * p.D + nn;
                    const float val = acc[mi][ni][r] + bias;
                    if (which == 0) p.qu[idx] = f2bf(val + bu);
                    else dst[idx] = f2bf(val);
                }
        }
    } else {
#pragma unroll
        for (int ni = 0; ni < NF; ++ni) {
            const int n = n0 + wn * (BN / 2) + ni * 32 + lcol;
            const bool f32out = (EPI == EPI_F32 || EPI == EPI_RESID_F32);
            const int nlim = f32out ? p.N : p.ldc;   // bf16 outputs also write their (zero) pad columns
            if (n >= nlim) continue;
            const float bias = p.bias[n];
            if constexpr (EPI == EPI_RESID_F32) {
                // residual epilogue: all 32 residual loads of this column tile first (unconditional, clamped rows), then the stores.
                // As one guarded load -> add -> store per element the loads were waited for one by one: 47 % of a wave's life
                // (s_memtime phases) for K = 2048.
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    float rv[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = m0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + lrow;
                        rv[r] = p.R[(size_t)(m < p.M ? m : p.M - 1) * p.ldr + n];
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(rv[r]));
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = m0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + lrow;
                        if (m < p.M) reinterpret_cast<float*>(p.C)[(size_t)m * p.ldc + n] = rv[r] + p.alpha * (acc[mi][ni][r] + bias);
                    }
                }
                continue;
            }
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + lrow;
                    if (m >= p.M) continue;
                    float val = acc[mi][ni][r] + bias;
                    if constexpr (EPI == EPI_F32) {
                        reinterpret_cast<float*>(p.C)[(size_t)m * p.ldc + n] = val;
                    } else if constexpr (EPI == EPI_RESID_F32) {
                        reinterpret_cast<float*>(p.C)[(size_t)m * p.ldc + n] = p.R[(size_t)m * p.ldr + n] + p.alpha * val;
                    } else if constexpr (EPI == EPI_SWISH_BF16) {
                        reinterpret_cast<bf16_t*>(p.C)[(size_t)m * p.ldc + n] = f2bf(swishf_(val));
                    } else {
                        reinterpret_cast<bf16_t*>(p.C)[(size_t)m * p.ldc + n] = f2bf(val);
                    }
                }
        }
    }
}

template <int BN, int EPI>
int launch_t(const GemmDev& gd, hipStream_t s) {
    const GemmParams& p = gd.p;
    const int n_tiles = (p.N + BN - 1) / BN, m_tiles = (p.M + BM - 1) / BM;
    const size_t lds = 2 * (BM + BN) * LROW;
    static LdsAttr attr;
    ensure_dynamic_lds(reinterpret_cast<const void*>(&gemm_kernel<BN, EPI>), (int)lds, attr);
    hipLaunchKernelGGL((gemm_kernel<BN, EPI>), dim3(m_tiles * n_tiles), dim3(256), lds, s, gd);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int EPI>
int launch_bn(const GemmDev& gd, hipStream_t s) {
    const int n = gd.p.N;
    // the 64-wide tile wastes less when N just exceeds a multiple of 128 by <= 64
    if constexpr (EPI != EPI_GLU_BF16) {
        if (ec_round_up(n, 64) < ec_round_up(n, 128)) return launch_t<64, EPI>(gd, s);
    }
    return launch_t<128, EPI>(gd, s);
}

}  // namespace

constexpr long GEMM256_MIN_TILES = 100;     // Large 35.4 -> 34.3 ms per step, ConformerCTC-Large 48.9 -> 47.1, Medium unchanged (profiles/r5_22_gemm256_tile_threshold.txt); 200 until round 4

int launch_gemm(const GemmParams& p, int epi, hipStream_t s) {
    if (p.M <= 0 || p.N <= 0 || p.K <= 0) return 0;
    if (p.lda % 8 || p.ldw % 64) return -2;
    if (p.wide != 1 && gemm256_supported(p, epi)) {
        // gemm256.hip when its 256 x 256 tiles fill the chip (256 CUs, one 8-wave workgroup each).  Measured on the Large layer shapes
        // (tools/gemm_bench.py, in situ with bench.py --wide-gemm): >= 200 tiles: up to 1.4x over the 128 x 128 kernel (FFN, D = 720),
        // never behind; fewer tiles, or its 256 x 128 tile at any size: behind.  `wide` 2 / 3 force a tile (kernel-level tests).
        // Round 5: the threshold was tuned on kernels running ALONE (a launch of 141 tiles leaves 45 % of the CUs idle and loses to the 128 x 128 kernel's
        // 564 workgroups); in the forward three row ranges run on three streams and the chip is saturated (throughput flat from B = 256 to 1024,
        // profiles/r5_03_*), so what a launch costs is its CU time, not its latency - and per CU the 256 x 256 LDS-DMA kernel is the efficient one.
        // `wide` >= 16 = the tile threshold itself (option wide_gemm; default GEMM256_MIN_TILES)
        const long t256 = (long)((p.M + 255) / 256) * ((p.N + 255) / 256);
        const long min_tiles = p.wide >= 16 ? p.wide : GEMM256_MIN_TILES;
        if (p.wide == 2 || ((p.wide == 0 || p.wide >= 16) && p.N >= 192 && t256 >= min_tiles)) return launch_gemm256(p, epi, 256, s);
        if (p.wide == 3) return launch_gemm256(p, epi, 128, s);
    }
    GemmDev gd;
    gd.p = p;
    gd.staged = gemm_staged_ok(p, epi);       // (EPI_F32 stays unstaged in this kernel whatever the answer)
    if (epi == EPI_QKV_NAT) gd.fD = FastDiv32(p.D);
    return gemm_epi_dispatch(epi, [&](auto e) { return launch_bn<decltype(e)::value>(gd, s); });
}
