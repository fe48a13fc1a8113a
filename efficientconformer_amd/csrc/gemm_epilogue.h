// The LDS-staged epilogues of the tiled bf16 GEMMs (gemm.hip, gemm256.hip), said once.
//
// Both kernels give a wave a 64 x (NF * 32) tile of 2 x NF accumulators of v_mfma_f32_32x32x16_bf16 (C layout: col = lane & 31,
// row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)).  The wave writes the finished values into a private LDS region (the operand
// buffers are free by then) and leaves them as 16-byte pieces, whole row segments per store instruction.  One 2-byte global store
// per element was half of gemm.hip (s_memtime phases: 51 %).  Three forms:
//   bf16 rows  EPI_BF16, EPI_SWISH_BF16 (pad columns N .. ldc written as zeros), EPI_QKV_NAT (Q + u | K | V rows of D columns)
//   GLU        the fragment pairs (2q, 2q + 1) are (a, b) of 32 output channels: a * sigmoid(b), NF / 2 * 32 columns
//   fp32 rows  EPI_RESID_F32 (alpha * (acc + bias) staged; the residual pieces are loaded behind the staging writes and pinned in front of the
//              write-out; then per piece: residual in, sum out).  gemm.hip only: gemm256.hip keeps its own fp32 form (EPI_F32 too; the residual
//              loads ahead of the staging writes) - through this function it measured 2 - 8 % slower on the 256 x 256 residual launches.
// The kernels differ in schedule only, which the template parameter carries: ROWS = rows staged per pass (64: all at once; 32: one
// accumulator row at a time, half the region).  The workgroup barrier that frees the operand buffers stays in the kernel.
#pragma once
#include "kernels.h"

#include <type_traits>

namespace {

// staging region of one wave: [ROWS][PITCH bytes], PPR 16-byte pieces per row, RPI rows per write-out instruction
template <int NF, int EPI> struct EpiStage {
    static constexpr bool F32OUT = EPI == EPI_F32 || EPI == EPI_RESID_F32, GLU = EPI == EPI_GLU_BF16;
    static constexpr int NQ = GLU ? NF / 2 : NF;                       // staged 32-column groups
    static constexpr int ESZ = F32OUT ? 4 : 2, EPP = 16 / ESZ;         // bytes per element, elements per piece
    static constexpr int PITCH = NQ * 32 * ESZ + 16, PPR = NQ * 32 / EPP, RPI = 64 / PPR;
};

// The 16-byte rules of the staged forms: whole pieces inside the rows, 16-byte-aligned rows
inline bool gemm_staged_ok(const GemmParams& p, int epi) {
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    switch (epi) {
        case EPI_BF16: case EPI_SWISH_BF16: case EPI_GLU_BF16: return p.ldc % 8 == 0 && al16(p.C);
        case EPI_QKV_NAT: return p.D % 8 == 0 && al16(p.qu) && al16(p.kh) && al16(p.vt);      // D % 8 == 0: a piece never straddles Q | K | V
        case EPI_RESID_F32: return p.N % 4 == 0 && p.N >= 4 && p.ldc % 4 == 0 && p.ldr % 4 == 0 && al16(p.C) && al16(p.R);
        case EPI_F32: return p.N % 4 == 0 && p.N >= 4 && p.ldc % 4 == 0 && al16(p.C);
    }
    return false;
}

// f(std::integral_constant<int, EPI>) for the epilogue `epi` of the tiled kernels
template <class F> int gemm_epi_dispatch(int epi, F&& f) {
    switch (epi) {
#define EC_EPI(E) case E: return f(std::integral_constant<int, E>{});
        EC_EPI(EPI_F32) EC_EPI(EPI_BF16) EC_EPI(EPI_SWISH_BF16) EC_EPI(EPI_RESID_F32) EC_EPI(EPI_GLU_BF16) EC_EPI(EPI_QKV_NAT)
#undef EC_EPI
    }
    return -3;
}

// wbuf: this wave's staging region (ROWS * EpiStage::PITCH bytes); (m_w, n_w): first row and column of the wave's tile; fD: divider by p.D (EPI_QKV_NAT)
template <int NF, int EPI, int ROWS>
__device__ __forceinline__ void staged_epilogue(const f32x16 (&acc)[2][NF], const GemmParams& p, const FastDiv32& fD, char* wbuf, int m_w, int n_w, int lane) {
    using ST = EpiStage<NF, EPI>;
    constexpr bool F32OUT = ST::F32OUT, GLU = ST::GLU, RESID = EPI == EPI_RESID_F32;
    constexpr int NQ = ST::NQ, PITCH = ST::PITCH, PPR = ST::PPR, RPI = ST::RPI, NIT = ROWS / RPI;
    static_assert(!GLU || NF % 2 == 0, "GLU needs both halves in one wave");
    static_assert(ROWS == 32 || ROWS == 64, "one or both accumulator rows per pass");
    static_assert(EPI != EPI_F32, "EPI_F32 leaves unstaged (gemm.hip) or through gemm256.hip's own fp32 form");
    const int lcol = lane & 31, lrow = 4 * (lane >> 5);
    // per-column constants of the lane's NQ staged columns: bias (+ u for the Q columns; GLU: bias of a and of b); live: not a pad column
    float ca[NQ], cb[NQ];
    bool live[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int n = n_w + q * (GLU ? 64 : 32) + lcol, nc = n < p.N ? n : p.N - 1;
        live[q] = n < p.N;
        ca[q] = p.bias[nc];
        cb[q] = GLU ? p.bias[n + 32 < p.N ? n + 32 : p.N - 1] : 0.f;
        if constexpr (EPI == EPI_QKV_NAT) { if (fD.div(nc) == 0) ca[q] += p.u[nc]; }
    }
    char* wlane = wbuf + lrow * PITCH + lcol * ST::ESZ;                // this lane's element of accumulator row 0, column group 0
    const int piece = lane % PPR, prow = lane / PPR;
    const int m_l = m_w + prow;                                        // first output row of this lane's pieces
    const int nb = (GLU ? n_w / 2 : n_w) + piece * ST::EPP;           // first output column of this lane's piece
    const int nbc = nb < p.N - 4 ? nb : p.N - 4;
#pragma unroll
    for (int ps = 0; ps < 64 / ROWS; ++ps) {
        float4 rv[NIT];
#pragma unroll
        for (int k = 0; k < ROWS / 32; ++k) {
            const int mi = ps * (ROWS / 32) + k;
#pragma unroll
            for (int q = 0; q < NQ; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    char* dst = wlane + (k * 32 + (r & 3) + 8 * (r >> 2)) * PITCH + q * 32 * ST::ESZ;       // lane address + a constant
                    if constexpr (F32OUT) {
                        float val = acc[mi][q][r] + ca[q];
                        if constexpr (RESID) val *= p.alpha;
                        *reinterpret_cast<float*>(dst) = val;
                    } else {
                        float val;
                        if constexpr (GLU) val = (acc[mi][2 * q][r] + ca[q]) * sigmoidf_(acc[mi][2 * q + 1][r] + cb[q]);
                        else val = acc[mi][q][r] + ca[q];
                        if constexpr (EPI == EPI_SWISH_BF16) val = swishf_(val);
                        *reinterpret_cast<bf16_t*>(dst) = f2bf(live[q] ? val : 0.f);      // pad columns of the row buffers stay zero
                    }
                }
        }
        wave_sync();
        if constexpr (RESID) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {                        // all residual pieces of the pass at once (unconditional, clamped)
                const int m = m_l + ps * ROWS + it * RPI;
                rv[it] = *reinterpret_cast<const float4*>(p.R + (size_t)(m < p.M ? m : p.M - 1) * p.ldr + nbc);
            }
#pragma unroll
            for (int it = 0; it < NIT; ++it) asm volatile("" : "+v"(rv[it].x), "+v"(rv[it].y), "+v"(rv[it].z), "+v"(rv[it].w));
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int row = it * RPI + prow, m = m_l + ps * ROWS + it * RPI;
            const char* src = wbuf + row * PITCH + piece * 16;
            if constexpr (F32OUT) {
                float4 a = *reinterpret_cast<const float4*>(src);
                if constexpr (RESID) a = make_float4(rv[it].x + a.x, rv[it].y + a.y, rv[it].z + a.z, rv[it].w + a.w);
                if (m < p.M && nb < p.N) *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + nb) = a;
            } else {
                const uint4 v = *reinterpret_cast<const uint4*>(src);
                if (m >= p.M) continue;
                if constexpr (EPI == EPI_QKV_NAT) {
                    if (nb >= p.N) continue;
                    const int which = fD.div(nb), nn = nb - which * p.D;
                    const int b = m / p.T, t = m - b * p.T;
                    bf16_t* dst = which == 1 ? p.kh : (which == 2 ? p.vt : p.qu);
                    *reinterpret_cast<uint4*>(dst + ((size_t)b * p.Tp + t) * p.D + nn) = v;
                } else {
                    if (nb < p.ldc) *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(p.C) + (size_t)m * p.ldc + nb) = v;
                }
            }
        }
        if (ps + 1 < 64 / ROWS) wave_sync();                           // the region is rewritten by the next pass
    }
}

}  // namespace
