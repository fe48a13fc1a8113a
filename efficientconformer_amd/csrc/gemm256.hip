// Wide-model bf16 MFMA GEMM (gfx950): 256 x BN x 64 block tiles with BOTH operands streamed by LDS-DMA.
//
//   C[m, n] = sum_k A[m, k] * W[n, k] + bias[n]      (same operands and epilogues as gemm.hip; launch_gemm picks this kernel)
//
// Serves the Linear / pointwise-conv layers of the widths the row-stationary kernels do not hold (D = 512, 720: EfficientConformer
// Large stages 2-3, Conformer Large; reference models/layers.py:57-67, call sites modules.py:378-382, 502-508, attentions.py:57-60).
//
//   * 8 waves as 4 (M) x 2 (N); a wave owns 64 x BN/2 of the tile: 2 x BN/64 accumulators of v_mfma_f32_32x32x16_bf16.
//   * Two LDS buffers of [256 + BN rows][128 bytes]; k-tile t+1 is written by global_load_lds_dwordx4 (no staging registers, no
//     ds_write pass) while k-tile t feeds the MFMAs: one s_waitcnt vmcnt(0) + s_barrier per k-tile.
//   * The DMA destination is lane-linear, so the bank swizzle lives on the SOURCE address: the 16-byte slot s of tile row r holds
//     the row's k-chunk s ^ ((r >> 1) & 7).  A fragment read (lane = row lr, k-chunk 2 kk + half) is conflict-free for the
//     ds_read_b128 lane groups of this chip (16 lanes: 8 even + 8 odd rows, all (row & 1, slot) pairs distinct), and every DMA
//     instruction still fetches 8 whole 128-byte row segments.
//   * K tail (K % 64 != 0, K % 8 == 0): chunks at or beyond column K are fetched from a 16-byte zero block instead of the row, so
//     neither stale workspace bytes nor the next row's data reach the MFMA (the packed weights are zero there as well).
//   * Epilogues leave through a per-wave LDS staging region as 16-byte pieces (bf16 rows, fp32 residual rows, GLU, Q+u | K | V rows),
//     32 rows at a time: the bf16 forms are gemm_epilogue.h's, shared with gemm.hip; the fp32 form is this file's own (see there).
#include "gemm_epilogue.h"
#include "rowstat.h"

namespace {

constexpr int G_BM = 256, G_BK = 64, G_NW = 8;
constexpr int G_ROWB = G_BK * 2;   // bytes per tile row

__device__ __attribute__((aligned(16))) uint32_t g_zero_chunk[4] = {0u, 0u, 0u, 0u};

struct G256Dev {
    GemmParams p;
    FastDiv32 fD;
    int n_tiles, m_tiles;
};

template <int BN, int EPI>
__global__ __launch_bounds__(G_NW * 64, 2) void gemm256_kernel(const G256Dev gd) {
    const GemmParams& p = gd.p;
    constexpr int NF = BN / 64, WCOLS = BN / 2;
    constexpr int A_BYTES = G_BM * G_ROWB, W_BYTES = BN * G_ROWB, BUF = A_BYTES + W_BYTES;
    constexpr int NA = G_BM / 8 / G_NW, NWD = BN / 8 / G_NW;     // DMA instructions (8 tile rows each) per wave and k-tile
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31, half = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int id = xcd_remap(blockIdx.x, gd.m_tiles * gd.n_tiles);
    const int tm = id / gd.n_tiles, tn = id - tm * gd.n_tiles;
    const int m0 = tm * G_BM, n0 = tn * BN;

    // ---- per-lane DMA sources: instruction j of a tile covers tile rows 8j .. 8j+7, lane -> (row 8j + lane/8, slot lane%8)
    const char* pa[NA];
    const char* pw[NWD];
    int ca[NA];                                                  // first k column (inside a k-tile) of this lane's A chunk
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const int r = 8 * (wave * NA + k) + (lane >> 3);
        const int cs = (lane & 7) ^ ((r >> 1) & 7);
        int m = m0 + r;
        m = m < p.M ? m : p.M - 1;
        size_t src = m;
        if (p.a_rows > 0) {
            const int b = m / p.a_rows, rr = m - b * p.a_rows;
            src = (size_t)b * p.a_pitch + (size_t)rr * p.a_stride;
        }
        pa[k] = reinterpret_cast<const char*>(p.A + src * p.lda + cs * 8);
        ca[k] = cs * 8;
    }
#pragma unroll
    for (int k = 0; k < NWD; ++k) {
        const int r = 8 * (wave * NWD + k) + (lane >> 3);
        const int cs = (lane & 7) ^ ((r >> 1) & 7);
        int n = n0 + r;
        n = n < p.N ? n : p.N - 1;                               // rows past N: any in-bounds row (their columns are never stored)
        pw[k] = reinterpret_cast<const char*>(p.W + (size_t)n * p.ldw + cs * 8);
    }
    const int nk = (p.K + G_BK - 1) / G_BK;
    const bool ktail = (p.K & (G_BK - 1)) != 0;
    auto issue = [&](int t, int buf) __attribute__((always_inline)) {
        char* base = smem + buf * BUF;
        const size_t kb = (size_t)t * G_ROWB;
        if (ktail && t == nk - 1) {
            const int k0 = t * G_BK;
#pragma unroll
            for (int k = 0; k < NA; ++k) {
                const char* src = (k0 + ca[k] < p.K) ? pa[k] + kb : reinterpret_cast<const char*>(g_zero_chunk);
                glds16(src, base + (wave * NA + k) * 1024);
            }
        } else {
#pragma unroll
            for (int k = 0; k < NA; ++k) glds16(pa[k] + kb, base + (wave * NA + k) * 1024);
        }
#pragma unroll
        for (int k = 0; k < NWD; ++k) glds16(pw[k] + kb, base + A_BYTES + (wave * NWD + k) * 1024);
    };

    f32x16 acc[2][NF];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < NF; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    // fragment byte offsets inside a 32-row group: row lr, k-chunk 2 kk + half at slot (2 kk + half) ^ ((lr >> 1) & 7)
    const int s0 = (half ^ ((lr >> 1) & 7)) * 16;
    int foff[G_BK / 16];
#pragma unroll
    for (int kk = 0; kk < G_BK / 16; ++kk) foff[kk] = lr * G_ROWB + ((kk * 32) ^ s0);

    auto compute = [&](int buf) __attribute__((always_inline)) {
        const char* a = smem + buf * BUF + (wm * 64) * G_ROWB;
        const char* b = smem + buf * BUF + A_BYTES + (wn * WCOLS) * G_ROWB;
#pragma unroll
        for (int kk = 0; kk < G_BK / 16; ++kk) {
            bf16x8 af[2], bf[NF];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) af[mi] = *reinterpret_cast<const bf16x8*>(a + mi * 32 * G_ROWB + foff[kk]);
#pragma unroll
            for (int ni = 0; ni < NF; ++ni) bf[ni] = *reinterpret_cast<const bf16x8*>(b + ni * 32 * G_ROWB + foff[kk]);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < NF; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
        }
    };

    issue(0, 0);
    for (int t = 0; t < nk; ++t) {
        wait_vmcnt<0>();                  // this wave's pieces of k-tile t have landed ...
        wg_barrier();                     // ... and everybody's; everybody is done reading the other buffer (k-tile t-1)
        if (t + 1 < nk) issue(t + 1, (t + 1) & 1);
        compute(t & 1);
    }
    wg_barrier();                         // the operand buffers are free: they become the staging regions below

    // ---- epilogue: 32 rows per pass.  C layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    using ST = EpiStage<NF, EPI>;
    char* wbuf = smem + wave * 32 * ST::PITCH;
    const int nw0 = n0 + wn * WCOLS;       // first column of this wave
    if constexpr (!ST::F32OUT) {
        staged_epilogue<NF, EPI, 32>(acc, p, gd.fD, wbuf, m0 + wm * 64, nw0, lane);
    } else {
        // fp32 rows (EPI_F32, EPI_RESID_F32): residual in and sum out per 16-byte piece, the residual pieces of a pass loaded AHEAD of its staging writes.
        // Kept here: through gemm_epilogue.h's fp32 form - with the loads in this place - the 256 x 256 residual launches were 2 - 8 % slower (tools/gemm_bench.py,
        // parent and new alternating, profiles/gemm_epilogue_single_source.txt); the listings differ in register allocation only and did not explain it
        const int lcol = lr, lrow = 4 * half;
        constexpr int PITCH = ST::PITCH, PPR = ST::PPR, RPI = ST::RPI, NIT = 32 / RPI;
        float bias[NF];
#pragma unroll
        for (int ni = 0; ni < NF; ++ni) { const int n = nw0 + ni * 32 + lcol; bias[ni] = p.bias[n < p.N ? n : p.N - 1]; }
        const int piece = lane % PPR, prow = lane / PPR, nb = nw0 + piece * 4;
        const int nbc = nb < p.N - 4 ? nb : p.N - 4;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            float4 rv[NIT];
            if constexpr (EPI == EPI_RESID_F32) {
#pragma unroll
                for (int it = 0; it < NIT; ++it) {               // all residual pieces first (unconditional, clamped)
                    const int m = m0 + wm * 64 + mi * 32 + it * RPI + prow;
                    rv[it] = *reinterpret_cast<const float4*>(p.R + (size_t)(m < p.M ? m : p.M - 1) * p.ldr + nbc);
                }
            }
#pragma unroll
            for (int ni = 0; ni < NF; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + lrow;
                    float val = acc[mi][ni][r] + bias[ni];
                    if constexpr (EPI == EPI_RESID_F32) val *= p.alpha;
                    *reinterpret_cast<float*>(wbuf + row * PITCH + (ni * 32 + lcol) * 4) = val;
                }
            wave_sync();
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int row = it * RPI + prow, m = m0 + wm * 64 + mi * 32 + row;
                float4 a = *reinterpret_cast<const float4*>(wbuf + row * PITCH + piece * 16);
                if constexpr (EPI == EPI_RESID_F32) a = make_float4(rv[it].x + a.x, rv[it].y + a.y, rv[it].z + a.z, rv[it].w + a.w);
                if (m < p.M && nb < p.N) *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + nb) = a;
            }
            wave_sync();
        }
    }
}

template <int BN, int EPI>
int launch256_t(G256Dev& gd, hipStream_t s) {
    const GemmParams& p = gd.p;
    gd.n_tiles = (p.N + BN - 1) / BN;
    gd.m_tiles = (p.M + G_BM - 1) / G_BM;
    constexpr int stage = G_NW * 32 * EpiStage<BN / 64, EPI_F32>::PITCH;   // the widest (fp32) staging region, whatever the epilogue
    constexpr int ring = 2 * (G_BM + BN) * G_ROWB;
    const int lds = ring > stage ? ring : stage;
    static LdsAttr attr;
    ensure_dynamic_lds(reinterpret_cast<const void*>(&gemm256_kernel<BN, EPI>), lds, attr);
    hipLaunchKernelGGL((gemm256_kernel<BN, EPI>), dim3(gd.m_tiles * gd.n_tiles), dim3(G_NW * 64), lds, s, gd);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int EPI>
int launch256_bn(G256Dev& gd, int bn, hipStream_t s) {
    return bn == 128 ? launch256_t<128, EPI>(gd, s) : launch256_t<256, EPI>(gd, s);
}

}  // namespace

// what the kernel needs beyond launch_gemm's own checks: whole 16-byte k-chunks, 16-byte-aligned operand rows, and an output that can leave staged
// (this kernel has no other epilogue)
bool gemm256_supported(const GemmParams& p, int epi) {
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    if (p.K % 8 || p.lda % 8 || p.ldw % 64 || p.ldw < ec_round_up(p.K, 64) || !al16(p.A) || !al16(p.W)) return false;
    return gemm_staged_ok(p, epi);
}

// bn: 256 or 128 columns per workgroup tile
int launch_gemm256(const GemmParams& p, int epi, int bn, hipStream_t s) {
    if (p.M <= 0 || p.N <= 0 || p.K <= 0) return 0;
    if (!gemm256_supported(p, epi) || (bn != 128 && bn != 256)) return -2;
    G256Dev gd;
    gd.p = p;
    gd.fD = FastDiv32(epi == EPI_QKV_NAT ? p.D : 1);
    return gemm_epi_dispatch(epi, [&](auto e) { return launch256_bn<decltype(e)::value>(gd, bn, s); });
}
