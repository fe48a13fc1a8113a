// What the three forms of the fused row-local chains (chain.hip, chain2.hip, chain3.hip) have in common, said once: the device struct and the launch, the
// LayerNorm partial sums and their hand-off between the waves of a row tile, the normalised bf16 fragment, the weight-slab reader and the paired MFMA loop
// of a 64-row ring chunk.  chain2.hip / chain3.hip promise chain.hip's bits ("every accumulator sees chain.hip's operations in chain.hip's order"): the
// operations whose order that promise is about live here.  The bodies - roles, barrier structure, ring protocol, write-outs - stay with their files.
// chain.hip's register-bound instances (256 VGPRs, some with scratch) keep local code where a call, though the same arithmetic, moved their scratch or
// their loop unrolling: each such site says so; profiles/chain_common_parity.txt has the listings' comparison.
// Layout throughout: xc[t][r] <-> row (lane & 31), column 32 t + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)   (chain.hip).
#pragma once
#include "rowstat.h"

namespace {

struct ChainDev {
    ChainParams p;
    FastDiv32 fT, fD;     // rows -> (utterance, frame), stacked Q | K | V column -> tensor (the Q/K/V write-out of the chain A kernels)
    int nf[8];            // float offsets of the LDS constant arrays (see chain_const_layout)
    int nfl_kb;           // size of the constant block in KiB (LDS-DMA pieces)
    int ldr, ld2;         // row pitch (elements) shared by every row-shaped weight of the chain / by the FFN second weights
};

// ---- LayerNorm statistics: two passes over the D valid columns, eps 1e-6 (reference modules.py:377, 447; blocks.py:97) ---------------------------------
// sum of N tiles, continuing `sum` (pad columns hold exact zeros: nothing to the sum)
template <int N>
__device__ __forceinline__ float row_psum(const f32x16 (&xc)[N], float sum) {
#pragma unroll
    for (int t = 0; t < N; ++t)
#pragma unroll
        for (int r = 0; r < 16; r += 4) sum += (xc[t][r] + xc[t][r + 1]) + (xc[t][r + 2] + xc[t][r + 3]);
    return sum;
}
// squared deviations of N tiles, continuing `var`; the tiles start at column col0 of the row for this lane (32 x first tile + 4 (lane >> 5)).
// Registers r .. r + 3 of tile t are the columns col0 + 32 t + 2 r + (0..3); D % 4 == 0: such a piece is valid or pad as a whole.
// A pad piece adds nothing: summing its four (0 - mean)^2 and subtracting pad * mean^2 afterwards cancels catastrophically where
// |mean| >> std (a stream with an offset of 160 and unit deviation at D = 24: 2e5 + 24 - 2e5 in float32, rstd off by 5e-4).  The pads lie in
// the last two tiles of the row (widths 16 .. 32 -> 32, .. 64, 68 .. 128, .. 192, .. 256: at most 60 pad columns; launch_chain refuses more), and the
// row's last two tiles are among the last two of any part of it that reaches its end
template <int N>
__device__ __forceinline__ float row_pvar(const f32x16 (&xc)[N], float var, float mu, int col0, int D) {
#pragma unroll
    for (int t = 0; t < N; ++t)
#pragma unroll
        for (int r = 0; r < 16; r += 4) {
            const float a = xc[t][r] - mu, b = xc[t][r + 1] - mu, c = xc[t][r + 2] - mu, d = xc[t][r + 3] - mu;
            const float g = (a * a + b * b) + (c * c + d * d);
            var += (t < N - 2 || col0 + 32 * t + 2 * r < D) ? g : 0.f;
        }
    return var;
}
// The single-wave form is chain.hip's ln_stats.  The pair form: a row split over two waves (second == 0: the first NTH tiles, 1: the rest) in the single-wave
// summation order - the first wave sums its tiles, the second continues from that partial and finishes (the xor-32 shuffle, the division, the rsqrt), and
// hands the result back: four workgroup barriers per norm, which every other wave of the workgroup executes too.  my / pa: this wave's and the partner's
// hand-off slot (one float per lane, already offset by the lane)
template <int NTH>
__device__ __forceinline__ void pair_ln_stats(const f32x16 (&xc)[NTH], int second, int col0, int D, float* my, const float* pa, float& mean, float& rstd) {
    mean = 0.f; rstd = 0.f;
    if (second == 0) *my = row_psum<NTH>(xc, 0.f);
    wg_barrier();
    if (second == 1) { const float sum = row_psum<NTH>(xc, *pa); mean = (sum + __shfl_xor(sum, 32)) / (float)D; *my = mean; }
    wg_barrier();
    if (second == 0) { mean = *pa; *my = row_pvar<NTH>(xc, 0.f, mean, col0, D); }
    wg_barrier();
    if (second == 1) {
        float var = row_pvar<NTH>(xc, *pa, mean, col0, D);
        var += __shfl_xor(var, 32);
        rstd = rsqrtf(fmaxf(var, 0.f) / (float)D + 1e-6f);
        *my = rstd;
    }
    wg_barrier();
    if (second == 0) rstd = *pa;
    // opaque copy: keeps the compiler from carrying all (x - mean) differences of the variance pass into the normalisation (chain.hip, ln_stats)
    asm volatile("" : "+v"(mean));
}

// bf16((xc - mean) * rstd), nm = -mean * rstd, as the K-permuted B fragment of k-step s of these tiles: registers [8 (s & 1), + 8) of tile s / 2.  The
// LayerNorm's gamma / beta are folded into the next GEMM at pack time (W diag(gamma), b + W beta), so the pre-norms cost no loads; pad columns become
// -mean * rstd but meet zero weight columns
template <int N>
__device__ __forceinline__ bf16x8 norm_frag(const f32x16 (&xc)[N], int s, float rstd, float nm) {
    const int r = 8 * (s & 1);
    return as_bf16x8(make_uint4(pack_bf2(fmaf(xc[s >> 1][r + 0], rstd, nm), fmaf(xc[s >> 1][r + 1], rstd, nm)),
                                pack_bf2(fmaf(xc[s >> 1][r + 2], rstd, nm), fmaf(xc[s >> 1][r + 3], rstd, nm)),
                                pack_bf2(fmaf(xc[s >> 1][r + 4], rstd, nm), fmaf(xc[s >> 1][r + 5], rstd, nm)),
                                pack_bf2(fmaf(xc[s >> 1][r + 6], rstd, nm), fmaf(xc[s >> 1][r + 7], rstd, nm))));
}

// Reader of a [32 rows][P1 pieces of 16 bytes] weight slab of the ring (image of dma_rows32_off): the A fragment of k-step s for this lane.  A value built from
// a lane id, so that the site decides where its two lane constants are born and how long they live (a stage that makes its own from lane_now() keeps them out
// of scratch between stages)
template <int P1>
struct WFrag {
    int q0, w1row;
    __device__ __forceinline__ explicit WFrag(int lane) : q0(((lane >> 5) + (lane & 31)) % P1), w1row((lane & 31) * (P1 * 16)) {}
    __device__ __forceinline__ bf16x8 operator()(const char* slab, int s) const {
        int q = q0 + 2 * s;
        q -= q >= P1 ? P1 : 0;
        return *reinterpret_cast<const bf16x8*>(slab + w1row + q * 16);
    }
};

// ---- a 64-row ring chunk (two 32-row slabs) against the whole fragment row: pointwise-1 / GLU and the stacked Q/K/V projection ------------------------------
// bias of the two slabs of ring chunk c -> accumulators
__device__ __forceinline__ void acc_from_bias(f32x16 (&acc)[2], const float* sb, int c, int half) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(sb + 64 * c + 32 * j + 8 * q + 4 * half);
            acc[j][4 * q + 0] = v.x; acc[j][4 * q + 1] = v.y; acc[j][4 * q + 2] = v.z; acc[j][4 * q + 3] = v.w;
        }
}
template <int KS, bool KPAD>
__device__ __forceinline__ void g1_mfma(f32x16 (&acc)[2], const bf16x8 (&xf)[KS], const char* buf, const WFrag<2 * KS>& wfrag) {
    constexpr int FB = 2, HALF = CH * 2 * KS * 16;       // fragments per batch and slab; bytes of a slab
#pragma unroll
    for (int s0 = 0; s0 < KS; s0 += FB) {
        bf16x8 wa[2][FB];
#pragma unroll
        for (int i = 0; i < FB; ++i) if (kstep<KS, KPAD>(s0 + i)) { wa[0][i] = wfrag(buf, s0 + i); wa[1][i] = wfrag(buf + HALF, s0 + i); }
#pragma unroll
        for (int i = 0; i < FB; ++i) if (kstep<KS, KPAD>(s0 + i)) {
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[0][i], xf[s0 + i], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[1][i], xf[s0 + i], acc[1], 0, 0, 0);
        }
    }
}

// ---- launch side ------------------------------------------------------------------------------------------------------------------------------------------------
// Fills the device struct of a chain of `kind`.  One row pitch for g0 / g1 / W1 (all have K = D) and one for the W2 matrices: the kernels keep their DMA offsets
// in registers.  w2cm: the chain reads the chunk-major images of the second FFN weights (chain3.hip) instead of the row-major ones.  Returns the
// launch's dynamic LDS bytes (lds_fixed = ring + staging, then the constant block), or the launch's error code
inline int chain_dev_init(ChainDev& cd, const ChainParams& p, int kind, bool w2cm, int lds_fixed) {
    const bool isb = kind == CHAIN_B, pre = kind == CHAIN_A_FULL || kind == CHAIN_A_TAIL, post = kind == CHAIN_A_FULL || kind == CHAIN_A_HEAD;
    cd.p = p;
    cd.fT = FastDiv32(p.T > 0 ? p.T : 1);
    cd.fD = FastDiv32(p.D);
    int ldr = 0, ld2 = 0;
    bool ok = true;
    auto row = [&](int ld) { if (!ldr) ldr = ld; else ok = ok && ld == ldr; };
    auto w2 = [&](const ChainFfn& f) { if (w2cm) ok = ok && f.w2cm; else if (!ld2) ld2 = f.ldw2; else ok = ok && f.ldw2 == ld2; };
    if (isb || pre) row(p.g0.ldw);
    if (isb || post) row(p.g1.ldw);
    if (pre) { row(p.f[0].ldw1); w2(p.f[0]); }
    if (post) { row(p.f[1].ldw1); w2(p.f[1]); }
    if (!ok || ldr <= 0) return -6;
    cd.ldr = ldr; cd.ld2 = ld2;
    const int nfl = chain_const_layout(p, kind, cd.nf);
    cd.nfl_kb = nfl / 256;
    if (!p.consts) return -5;
    const int lds = lds_fixed + nfl * 4;
    return lds > 160 * 1024 ? -4 : lds;
}
// Launches `kernel` (cd, nullptr), or `kernel_kpad` (cd) where the launcher of the file applied ks_skip_last; raises the instance's dynamic-LDS limit first.
// One instantiation - and so one pair of LdsAttr statics - per pair of kernels
template <auto KERNEL, auto KERNEL_KPAD>
int chain_launch(bool kpad, dim3 grid, dim3 block, int lds, hipStream_t s, const ChainDev& cd) {
    static LdsAttr attr;
    ensure_dynamic_lds(reinterpret_cast<const void*>(KERNEL), lds, attr);
    if constexpr (!std::is_same_v<decltype(KERNEL_KPAD), std::nullptr_t>) {
        if (kpad) {
            static LdsAttr attr_kpad;
            ensure_dynamic_lds(reinterpret_cast<const void*>(KERNEL_KPAD), lds, attr_kpad);
            hipLaunchKernelGGL(KERNEL_KPAD, grid, block, lds, s, cd);
            return hipGetLastError() == hipSuccess ? 0 : -1;
        }
    }
    hipLaunchKernelGGL(KERNEL, grid, block, lds, s, cd, nullptr);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace
