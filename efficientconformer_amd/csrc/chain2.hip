// Column-pair form of chain B (gfx950): the out-projection + LayerNorm + pointwise-1 / GLU chain of chain.hip at padded width 256
// (D = 193 .. 256), two waves per SIMD.  Chain A at that width runs on chain3.hip.
//
// chain.hip keeps a wave's 32 residual rows in registers over the full padded width: 32 x 256 fp32 + their bf16 copy are 192 registers
// before any temporary, so the D = 240 chains run ONE wave per SIMD (4-wave, 128-row workgroups, 467 of 512 registers).  A lone wave is
// its own dependency chain, its refill DMAs blocking everything behind them, and only four waves issue the L2 -> LDS weight stream
// (5.6 B / cycle per issuing wave, profiles/r4_03_lds_fill_rate.txt).
//
// Here a workgroup is 8 waves on the same 128 rows: a PAIR of waves (w, w + 4: the two waves of one SIMD) per 32 rows.
//   * wave A (cw = 0) owns the residual columns [0, DP / 2), wave B (cw = 1) [DP / 2, DP): NT / 2 accumulator tiles each (64 registers
//     at D = 240 instead of 128); both hold the full normalised row as bf16 B fragments (xf: they exchange their halves through LDS
//     after every LayerNorm / load, 8 KiB per wave);
//   * GLU chunks alternate between the two, and the owner of chunk c writes its tile out DURING chunk c + 1 (the partner's MFMAs): the
//     HBM-bound write-out runs beside the other wave's matrix work;
//   * the two waves of a pair issue the weight ring's LDS-DMAs in turns (2 PER = KS / 2 per wave and chunk).
// Every accumulator sees the same operations on the same operands in the same order as in chain.hip (k order of the GEMMs, LayerNorm
// sums continued from wave A's partial in wave B), so the rows are BIT-IDENTICAL to chain.hip's - which is how this file is tested
// (tests/test_gpu_round5.py: option chain_pair 5 against 0).  Weights, constant blocks and parameters are chain.hip's (same packing, same
// ring chunk layout).  Reference: models/modules.py:511-514; blocks.py:126; attentions.py:716.
#include "chain_common.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>

namespace {

constexpr int NW2 = 8, NBUF2 = 3;
constexpr int S2_WIN = 32 * STG128_ROW;         // 4608: the window area; its bytes [0, 4096) also carry the xf exchanges between the waves of a pair
constexpr int S2_BYTES = S2_WIN + 512;       // + the LayerNorm hand-off slots (never touched by the window / exchange traffic: no barrier between their last read and the next private use)

template <int KS>
struct Geo2 {
    static_assert(KS % 4 == 0, "an even number of 32-column tiles per wave");
    static constexpr int NT = KS / 2, NTH = NT / 2, KSH = KS / 2;
    static constexpr int DP = 16 * KS, P1 = KS * 2;
    static constexpr int HALF = CH * P1 * 16, BUF = 2 * HALF;
    static constexpr int PER = 2 * KS / NW2;             // wave-DMAs per wave and ring chunk (2 PER in the wave's turn)
};

// PROF (tuning library only, -DEFFCONF_PHASE_PROF; EFFCONF_CHAIN2_PHASES=1): s_memtime per phase, wave A and wave B of every 8th workgroup's first pair
// KPAD: the last k-step holds pad columns only and is left out of every product over the model width (rowstat.h, ks_skip_last)
template <int KS, bool PROF, bool KPAD>
__device__ __forceinline__ void chain2_body(const ChainDev& cd, unsigned long long* prof) {
    unsigned long long ph[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, t0 = 0;
    if constexpr (PROF) t0 = __builtin_readcyclecounter();
#define C2_TICK(i) do { if constexpr (PROF) { asm volatile("" ::: "memory"); const unsigned long long t1_ = __builtin_readcyclecounter(); ph[i] += t1_ - t0; t0 = t1_; } } while (0)
    using G = Geo2<KS>;
    constexpr int NT = G::NT, NTH = G::NTH, KSH = G::KSH, P1 = G::P1, HALF = G::HALF, BUF = G::BUF, PER = G::PER;
    const ChainParams& p = cd.p;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* stg_base = smem + NBUF2 * BUF;
    float* sf = reinterpret_cast<float*>(stg_base + NW2 * S2_BYTES);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pr = wave & 3, cw = wave >> 2;                  // row tile of the workgroup; column half (waves w and w + 4 share a SIMD)
    const int lr = lane & 31, half = lane >> 5;
    const int m_base = (blockIdx.x * 4 + pr) * 32;
    char* stg = stg_base + wave * S2_BYTES;                   // this wave's staging region
    const char* stgp = stg_base + (wave ^ 4) * S2_BYTES;      // the partner's (read only)
    const int D = p.D;
    // KPAD: the dropped k-step (rowstat.h, kstep) is wave B's last own fragment: not built (zeros travel through the exchange in its place), not read back,
    // no weight fragment, no MFMA
    const bool own_pad = KPAD && cw == 1;                     // this wave's own[KSH - 1] is the dropped k-step

    // ---- chunk schedule: [g0] [g1]
    const int n_g0 = (NT + 1) / 2;
    const int n_g1 = p.g1.nchunks;
    const int total = n_g0 + n_g1;

    // the two waves of a pair take the refills in turns: ring chunk k is issued (2 PER wave-DMAs, wave-instructions pr + 4 k') by the waves with
    // cw == (k & 1), in iteration k - 2
    constexpr int NOFF = 2 * PER;
    uint32_t off_r[NOFF];
#pragma unroll
    for (int k = 0; k < NOFF; ++k) {
        const int i = pr + 4 * k;
        off_r[k] = i < KS ? dma_rows32_off<P1>(cd.ldr, i, lane) : dma_rows32_off<P1>(cd.ldr, i - KS, lane) + (uint32_t)(32 * cd.ldr) * 2u;
    }
    auto issue = [&](int c) __attribute__((always_inline)) {
        const bool first_g = c < n_g0;
        const bf16_t* gw = first_g ? p.g0.w : p.g1.w;
        const int cg = first_g ? c : c - n_g0;
        const char* w = reinterpret_cast<const char*>(gw + (size_t)(cg > 0 ? cg : 0) * 64 * cd.ldr);
        char* buf = smem + (c % NBUF2) * BUF;
#pragma unroll
        for (int k = 0; k < NOFF; ++k) glds16(w, off_r[k], buf + 1024 * (pr + 4 * k));
    };
    static_assert(HALF == 64 * KS * 16, "second half of a buffer = wave-instruction KS");
    // Ring protocol of chain.hip (plain rule): barrier k = chunk k has landed for everybody and everybody is done with chunk k - 1, whose
    // buffer takes chunk k + 2 - issued in iteration k by the waves whose turn it is
    int gc = 0;
    auto advance = [&]() __attribute__((always_inline)) -> const char* {
        // the issuer of chunk gc has nothing younger in its queue than the stores it issued since (chunk gc + 2 comes in iteration gc); a store may
        // retire before an older DMA (chain.hip, advance()), so the queue is drained rather than the stores counted
        if (cw == (gc & 1)) wait_vmcnt_dyn(0);
        C2_TICK(1);
        wg_barrier();
        C2_TICK(0);
        const char* buf = smem + (gc % NBUF2) * BUF;
        ++gc;
        return buf;
    };
    // the refill of iteration gc - 1 (chunk gc + 1): only the waves whose turn it is (cw == parity of the iteration = of the chunk)
    auto refill = [&]() __attribute__((always_inline)) {
        if (cw != ((gc - 1) & 1)) return;
        if (gc + NBUF2 - 2 < total) issue(gc + NBUF2 - 2);
        C2_TICK(11);
    };

    float* s_b0 = sf + cd.nf[0];
    float* s_g1b = sf + cd.nf[6];
    for (int i = wave; i < cd.nfl_kb; i += NW2) glds16(reinterpret_cast<const char*>(p.consts) + (size_t)i * 1024 + lane * 16, reinterpret_cast<char*>(sf) + i * 1024);
#pragma unroll
    for (int c = 0; c < NBUF2 - 1; ++c)
        if (c < total && cw == (c & 1)) issue(c);

    // ---- this wave's state: NTH residual tiles (its column half), the whole normalised row as B fragments
    f32x16 xc[NTH];
    bf16x8 xf[KS];
    const int ct0 = cw * NTH;                                // first tile / (x 2) first k-step of the wave's column half

    // own fragments -> both waves of the pair hold xf[0 .. KS): through the staging regions, 4 fragments (4 KiB) per round.  Every wave reads BOTH
    // halves back from LDS (its own from its own region): a branch on cw around the register array would be if-converted into a dynamically
    // indexed store and put xf into scratch
    const char* stgA = stg_base + pr * S2_BYTES;             // staging of the pair's wave A / wave B
    const char* stgB = stg_base + (pr + 4) * S2_BYTES;
    auto publish_xf = [&](const bf16x8 (&own)[KSH]) __attribute__((always_inline)) {
#pragma unroll
        for (int r0 = 0; r0 < KSH; r0 += 4) {
            if (r0 > 0) wg_barrier();                        // the partner has read the previous round
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (r0 + i < KSH) *reinterpret_cast<bf16x8*>(stg + i * 1024 + lane * 16) = own[r0 + i];
            wg_barrier();
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (r0 + i < KSH) {
                    xf[r0 + i] = *reinterpret_cast<const bf16x8*>(stgA + i * 1024 + lane * 16);
                    if (kstep<KS, KPAD>(KSH + r0 + i)) xf[KSH + r0 + i] = *reinterpret_cast<const bf16x8*>(stgB + i * 1024 + lane * 16);
                }
        }
        wg_barrier();                                        // the staging regions are private again
    };

    // ---- rows in: x (the wave's column half, fp32) and the bf16 operand rows (each wave its half of the k-steps, then exchanged)
    {
        const char* xb = reinterpret_cast<const char*>(p.X);
        u32x4 vx[4 * NTH] = {};
        static_for<0, NTH>([&](auto I) { constexpr int tt = decltype(I)::value; stage128_load<4 * tt>(xb, (size_t)p.ldx * 4, D * 4, m_base, p.M, 128 * (ct0 + tt), lane, vx); });
        constexpr int NWA = (KSH + 3) / 4;                   // 128-byte windows (4 k-steps) of the wave's half of the operand row
        u32x4 va[4 * NWA] = {};
        const char* ab = reinterpret_cast<const char*>(p.A);
        static_for<0, NWA>([&](auto I) { constexpr int w = decltype(I)::value; stage128_load<4 * w>(ab, (size_t)p.lda * 2, p.lda * 2, m_base, p.M, cw * KSH * 32 + 128 * w, lane, va); });
        static_for<0, NTH>([&](auto I) {
            constexpr int tt = decltype(I)::value;
            wave_sync();
            stage128_put<4 * tt>(stg, lane, vx);
            wave_sync();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int col = 32 * (ct0 + tt) + 8 * q + 4 * half;
                float4 x4 = *reinterpret_cast<const float4*>(stg + lr * STG128_ROW + (q * 8 + half * 4) * 4);
                if (col >= D) x4 = make_float4(0.f, 0.f, 0.f, 0.f);
                xc[tt][4 * q + 0] = x4.x; xc[tt][4 * q + 1] = x4.y; xc[tt][4 * q + 2] = x4.z; xc[tt][4 * q + 3] = x4.w;
            }
        });
        bf16x8 own[KSH];
        static_for<0, NWA>([&](auto I) {
            constexpr int w = decltype(I)::value;
            wave_sync();
            stage128_put<4 * w>(stg, lane, va);
            wave_sync();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (4 * w + j == KSH - 1 && own_pad) own[4 * w + j] = as_bf16x8(make_uint4(0u, 0u, 0u, 0u));
                else if (4 * w + j < KSH) {
                    const int s = cw * KSH + 4 * w + j;
                    const char* src = stg + lr * STG128_ROW + (16 * j + 4 * half) * 2;
                    uint2 lo = *reinterpret_cast<const uint2*>(src), hi = *reinterpret_cast<const uint2*>(src + 16);
                    const int c0 = 16 * s + 4 * half;
                    if (c0 >= D || m_base + lr >= p.M) lo = make_uint2(0u, 0u);
                    if (c0 + 8 >= D || m_base + lr >= p.M) hi = make_uint2(0u, 0u);
                    own[4 * w + j] = as_bf16x8(make_uint4(lo.x, lo.y, hi.x, hi.y));
                }
            }
        });
        wave_sync();
        publish_xf(own);
    }
    // constants and the first chunk visible to everybody
    wait_vmcnt<0>();
    wg_barrier();
    C2_TICK(6);

    const WFrag<P1> wfrag(lane);

    auto add_cvec2 = [&](const float* sv) __attribute__((always_inline)) {       // xc[tt][r] += sv[column]
#pragma unroll
        for (int tt = 0; tt < NTH; ++tt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 v = *reinterpret_cast<const float4*>(sv + 32 * (ct0 + tt) + 8 * q + 4 * half);
                xc[tt][4 * q + 0] += v.x; xc[tt][4 * q + 1] += v.y; xc[tt][4 * q + 2] += v.z; xc[tt][4 * q + 3] += v.w;
            }
    };
    // LayerNorm statistics in chain.hip's summation order: wave A's partial continued by wave B (pair_ln_stats)
    auto ln_stats2 = [&](float& mean, float& rstd) __attribute__((always_inline)) {
        float* my = reinterpret_cast<float*>(stg + S2_WIN) + lane;
        const float* pa = reinterpret_cast<const float*>(stgp + S2_WIN) + lane;
        pair_ln_stats<NTH>(xc, cw, 32 * ct0 + 4 * half, D, my, pa, mean, rstd);
        C2_TICK(5);
    };
    // bf16((x - mean) * rstd) of the wave's columns as K-permuted B fragments, then both halves to both waves
    auto norm_xf = [&](float mean, float rstd) __attribute__((always_inline)) {
        const float nm = -mean * rstd;
        bf16x8 own[KSH];
#pragma unroll
        for (int s = 0; s < KSH; ++s) {
            if (s == KSH - 1 && own_pad) own[s] = as_bf16x8(make_uint4(0u, 0u, 0u, 0u));
            else own[s] = norm_frag(xc, s, rstd, nm);
        }
        publish_xf(own);
        C2_TICK(5);
    };
    auto store_x2 = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int tt = 0; tt < NTH; ++tt) {
            wave_sync();
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<float4*>(stg + lr * STG128_ROW + (q * 8 + half * 4) * 4) = make_float4(xc[tt][4 * q + 0], xc[tt][4 * q + 1], xc[tt][4 * q + 2], xc[tt][4 * q + 3]);
            wave_sync();
            stage128_store(stg, reinterpret_cast<char*>(p.Y), (size_t)p.ldy * 4, D * 4, m_base, p.M, 128 * (ct0 + tt), lane);
        }
        C2_TICK(10);
    };

    // ---- stage: x += g0(A).  Ring chunk c carries the weight rows of tiles 2c and 2c + 1: wave A's tiles come first, then wave B's
    add_cvec2(s_b0);
#pragma unroll
    for (int c = 0; c < (NT + 1) / 2; ++c) {
        const char* buf = advance();
        refill();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            constexpr int FB = (KS % 8 == 0) ? 8 : 4;
            const int t = 2 * c + j;                         // compile-time after unrolling
            if (t < NT && cw == t / NTH) {
                const int tt = t % NTH;
#pragma unroll
                for (int s0 = 0; s0 < KS; s0 += FB) {
                    bf16x8 wa[FB];
#pragma unroll
                    for (int i = 0; i < FB; ++i) if (kstep<KS, KPAD>(s0 + i)) wa[i] = wfrag(buf + j * HALF, s0 + i);
#pragma unroll
                    for (int i = 0; i < FB; ++i) if (kstep<KS, KPAD>(s0 + i)) xc[tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[i], xf[s0 + i], xc[tt], 0, 0, 0);
                }
            }
        }
        if constexpr (PROF) asm volatile("s_nop 0" :: "v"(xc[0][0]), "v"(xc[NTH - 1][15]));
        C2_TICK(7);
    }

    // ---- conv-module pre-norm, pointwise-1 + GLU -> bf16 rows (modules.py:512-514).  GLU chunks alternate between the pair; the owner of chunk c
    //      writes it out during chunk c + 1
    {
        float mean, rstd;
        ln_stats2(mean, rstd);
        norm_xf(mean, rstd);
        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        auto glu_out = [&](int c) __attribute__((always_inline)) {
            wave_sync();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float o[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = acc[0][4 * q + i] * sigmoidf_(acc[1][4 * q + i]);
                *reinterpret_cast<uint2*>(stg + lr * STG128_ROW + (8 * q + 4 * half) * 2) = make_uint2(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]));
            }
            wave_sync();
            const int col = 32 * c + 8 * (lane & 3);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = 16 * i + (lane >> 2), m = m_base + row;
                const u32x4 v = *reinterpret_cast<const u32x4*>(stg + row * STG128_ROW + 16 * (lane & 3));
                if (m < p.M && col < p.Ng) *reinterpret_cast<u32x4*>(p.glu + (size_t)m * p.ldg + col) = v;
            }
        };
        const int op = gc & 1;                               // owner(c) = the waves with cw == ((c + op) & 1): the wave that refills in that iteration
        for (int c = 0; c < n_g1; ++c) {
            const char* buf = advance();
            refill();
            if (((c + op) & 1) == cw) { acc_from_bias(acc, s_g1b, c, half); g1_mfma<KS, KPAD>(acc, xf, buf, wfrag); if constexpr (PROF) asm volatile("s_nop 0" :: "v"(acc[0][0]), "v"(acc[1][15])); C2_TICK(8); }
            else if (c >= 1) { glu_out(c - 1); C2_TICK(9); }
        }
        if (n_g1 >= 1 && ((n_g1 - 1 + op) & 1) == cw) glu_out(n_g1 - 1);
    }
    // ---- residual rows out
    store_x2();
    if constexpr (PROF) {
        C2_TICK(12);
        if (lane == 0 && pr == 0 && (blockIdx.x & 7) == 0) {
            for (int i = 0; i < 13; ++i) atomicAdd(prof + 16 * cw + i, ph[i]);
            atomicAdd(prof + 16 * cw + 15, 1ull);
        }
    }
#undef C2_TICK
}

template <int KS, bool PROF = false>
__global__ __launch_bounds__(NW2 * 64, 1) void chain2_kernel(const ChainDev cd, unsigned long long* prof = nullptr) {
    chain2_body<KS, PROF, false>(cd, prof);
}
// the same chain for a width whose last k-step is all pad (D = 240)
template <int KS>
__global__ __launch_bounds__(NW2 * 64, 1) void chain2_kpad_kernel(const ChainDev cd) {
    chain2_body<KS, false, true>(cd, nullptr);
}

#ifdef EFFCONF_PHASE_PROF    // in-kernel phase profiles: a tuning build (tools/build_ablate.py) only
unsigned long long* g_chain2_prof = nullptr;
void chain2_prof_dump() {
    unsigned long long h[32];
    if (!g_chain2_prof || hipMemcpy(h, g_chain2_prof, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess || !h[15]) return;
    static const char* names[13] = {"barrier", "vmcnt wait", "-", "-", "-", "LN + exchange", "prologue", "g0 mfma", "g1 mfma", "g1 write-out", "store_x", "refill issue", "tail"};
    for (int w = 0; w < 2; ++w) {
        const unsigned long long* q = h + 16 * w;
        unsigned long long tot = 0;
        for (int i = 0; i < 13; ++i) tot += q[i];
        fprintf(stderr, "[chain2 phases] wave %c: waves %llu, cycles/wave %.0f\n", w ? 'B' : 'A', q[15], (double)tot / q[15]);
        for (int i = 0; i < 13; ++i) if (q[i]) fprintf(stderr, "[chain2 phases]   %-16s %10.0f cyc/wave  %5.1f%%\n", names[i], (double)q[i] / q[15], 100.0 * q[i] / tot);
    }
}
#endif

}  // namespace

int launch_chain2(const ChainParams& p, hipStream_t s) {
    constexpr int KS = 16;
    using G = Geo2<KS>;
    if (p.M <= 0) return 0;
    if (!chain3_supported(p.D)) return -2;                   // padded width 256
    if (p.g0.ldw <= 0) return -6;                            // (chain_dev_init skips a leading zero pitch, as chain.hip always did; this launcher never did)
    ChainDev cd;
    const int lds = chain_dev_init(cd, p, CHAIN_B, false, NBUF2 * G::BUF + NW2 * S2_BYTES);       // LDS: ring + staging + constant block
    if (lds < 0) return lds;
#ifdef EFFCONF_PHASE_PROF
    static const bool prof = getenv("EFFCONF_CHAIN2_PHASES") != nullptr;
    if (prof) {
        if (!g_chain2_prof) {
            if (hipMalloc(&g_chain2_prof, 256) != hipSuccess || hipMemset(g_chain2_prof, 0, 256) != hipSuccess) return -1;
            atexit(chain2_prof_dump);
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&chain2_kernel<KS, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        }
        hipLaunchKernelGGL((chain2_kernel<KS, true>), dim3((p.M + 127) / 128), dim3(NW2 * 64), lds, s, cd, g_chain2_prof);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
#endif
    return chain_launch<&chain2_kernel<KS, false>, &chain2_kpad_kernel<KS>>(ks_skip_last<KS>((p.D + 15) / 16), dim3((p.M + 127) / 128), dim3(NW2 * 64), lds, s, cd);
}
