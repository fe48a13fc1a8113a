// Device pieces shared by the RNN-T decoders: rnnt.hip (greedy: per-utterance and cluster kernels) and rnnt_beam.hip (beam search).
// The prediction network's weights live in the k-major / k-permuted images effconf_rnnt_finalize builds; the fp32-MFMA mat-vec
// below keeps the k order of every dot product ascending whatever the number of state vectors (columns) it multiplies.
#pragma once
#include "kernels.h"
#include "../../include/effconf.h"

#include <map>
#include <string>
#include <vector>

namespace ecrnnt {

struct RnntDev {
    const float* gin;        // [V][4H]   W_ih emb[y] + b_ih + b_hh
    const float4* whh4;      // [H/4][4H]
    const float4* wd4;       // [H/4][J]
    const float* bd;         // [J]
    const float4* wj4;       // [J/4][V]
    const float4 *whh16, *wd16, *wj16;   // the same three in the MFMA order: [K/16][4][N] (kperm16), null if K % 16
    const float* bj;         // [V]
    int H, J, V, max_consec;
};

__device__ __forceinline__ float sigmoid_precise(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- the three mat-vec phases on the fp32 matrix pipe -----------------------------------------------------------------------------------
// A round multiplies a slice of a weight matrix with the CU = 8 (joint: CU * CKF = 16) state vectors of the cluster's utterances.  As VALU
// code that is 32 FMAs + 8 broadcast LDS reads per weight float4 and thread: the phases were issue-bound (s_memtime: 71k + 37k + 77k of a
// round's 206k cycles; the three cluster barriers 1.5k each).  v_mfma_f32_16x16x4_f32 takes 16 weight rows x 4 k (A) against 4 k x 16 state
// vectors (B): one weight float4 and one state float4 per lane feed four MFMAs (4096 MACs).  The k order of every dot product stays
// ASCENDING: lane group g = lane / 16 is k-slot g of an MFMA, so the float4 a lane loads for 16-block q must hold k = 16q + g, 16q + 4 + g,
// 16q + 8 + g, 16q + 12 + g (MFMA c of the block then covers k = 16q + 4c .. 16q + 4c + 3) - the weights get a second image in that order
// (kperm16) and the state vectors sit in LDS with k permuted the same way (kperm).
__host__ __device__ __forceinline__ int kperm(int k) { return (k & ~15) | ((k & 3) << 2) | ((k >> 2) & 3); }
constexpr int CMB = 4;          // 16-blocks of weight loads in flight per tile and lane (8 when a wave owns at most two tiles and K allows)

template <int NTL, int CMB>
__device__ __forceinline__ void mfma_rows16_t(const float4* __restrict__ W16, int N, int K16, const int (&nrow)[NTL], const float* xs_lane, f32x4 (&acc)[NTL]) {
    const int g = (threadIdx.x & 63) >> 4;
    const size_t bs = (size_t)4 * N;                    // float4s per 16-block: [g][n]
    const float4* wp[NTL];
    float4 wn[NTL][CMB];
#pragma unroll
    for (int i = 0; i < NTL; ++i) {
        wp[i] = W16 + (size_t)g * N + nrow[i];
#pragma unroll
        for (int b = 0; b < CMB; ++b) wn[i][b] = wp[i][b * bs];
    }
    for (int q0 = 0; q0 < K16; q0 += CMB) {
        float4 wv[NTL][CMB];
#pragma unroll
        for (int i = 0; i < NTL; ++i)
#pragma unroll
            for (int b = 0; b < CMB; ++b) wv[i][b] = wn[i][b];
        const int qn = q0 + CMB < K16 ? q0 + CMB : q0;                      // last pass: harmless re-load
#pragma unroll
        for (int i = 0; i < NTL; ++i)
#pragma unroll
            for (int b = 0; b < CMB; ++b) wn[i][b] = wp[i][(size_t)(qn + b) * bs];
#pragma unroll
        for (int b = 0; b < CMB; ++b) {
            const float4 x = *reinterpret_cast<const float4*>(xs_lane + 16 * (q0 + b));
#pragma unroll
            for (int i = 0; i < NTL; ++i) {
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i][b].x, x.x, acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i][b].y, x.y, acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i][b].z, x.z, acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i][b].w, x.w, acc[i], 0, 0, 0);
            }
        }
    }
}

template <int NTL>
__device__ __forceinline__ void mfma_rows16(const float4* __restrict__ W16, int N, int K16, const int (&nrow)[NTL], const float* xs_lane, f32x4 (&acc)[NTL]) {
    if (NTL <= 2 && (K16 & 7) == 0) mfma_rows16_t<NTL, 8>(W16, N, K16, nrow, xs_lane, acc);
    else mfma_rows16_t<NTL, 4>(W16, N, K16, nrow, xs_lane, acc);
}

// mfma_rows16 for any K16 (the greedy kernels' shapes need K16 % 4 == 0; one 16-block of loads in flight otherwise).  Same k order.
template <int NTL>
__device__ __forceinline__ void mfma_rows16_any(const float4* __restrict__ W16, int N, int K16, const int (&nrow)[NTL], const float* xs_lane, f32x4 (&acc)[NTL]) {
    if ((K16 & 3) == 0) mfma_rows16<NTL>(W16, N, K16, nrow, xs_lane, acc);
    else mfma_rows16_t<NTL, 1>(W16, N, K16, nrow, xs_lane, acc);
}

// W [N][K] row-major -> float4 image [K/16][4][N]: entry (q, g, n) = W[n][16q + g], W[n][16q + 4 + g], W[n][16q + 8 + g], W[n][16q + 12 + g]
// (host; rnnt.hip and lm.hip build their MFMA weight images with it at finalize)
inline std::vector<float> kperm16(const std::vector<float>& W, int N, int K) {
    std::vector<float> o((size_t)N * K);
    for (int q = 0; q < K / 16; ++q)
        for (int g = 0; g < 4; ++g)
            for (int n = 0; n < N; ++n)
                for (int e = 0; e < 4; ++e) o[(((size_t)q * 4 + g) * N + n) * 4 + e] = W[(size_t)n * K + 16 * q + 4 * e + g];
    return o;
}

// fp32 GEMM  C[m][n] = sum_k A[m][k] * B[n][k] + bias[n]   (nn.Linear semantics), K % 4 == 0 (rnnt.hip)
int launch_sgemm_nt(const float* A, int lda, const float* Bw, int ldb, const float* bias, float* C, int ldc, int M, int N, int K, hipStream_t s);

// Beam search (rnnt_beam.hip) needs the MFMA weight images: finalize uploads them whenever this holds
inline bool beam_dims_supported(const EcRnntConfig& c) { return c.dim_decoder % 16 == 0 && c.dim_joint % 16 == 0; }

}  // namespace ecrnnt

struct EcRnntHostT { std::vector<int64_t> shape; std::vector<float> data; };

struct EcRnnt {
    EcRnntConfig cfg;
    std::map<std::string, EcRnntHostT> host;
    std::vector<void*> allocs;
    ecrnnt::RnntDev dev{};
    float* we = nullptr;     // linear_encoder.weight [J][De]
    float* be = nullptr;
    float* wd = nullptr;     // linear_decoder.weight [J][H], row-major (the lattice's GEMM over all (b, u) rows)
    bool finalized = false;
    int cluster_by_slice = 1;   // cluster decode: workgroup -> XCD mapping (see rnnt_cluster_kernel)
    int cluster_mode = -1;   // -1 auto (cluster decode for batches >= 2 x the cluster's utterances), 0 per-utterance kernel, 1 force cluster
    int beam_eval_batch = 16;   // beam search: A hypotheses evaluated per pass over the weights (1 .. 16; identical results)
    int cluster_shape = 0;   // 0 <8, 8, 2> (default), 1 <16, 16, 1> where supported (measured: no faster - see the shapes' comment - and a blank costs a round of its own)
};
