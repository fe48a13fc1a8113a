// Self-conditioned CTC step (reference models/encoders.py:209-213) as one row-stationary kernel for gfx950:
//
//     z = q(x) q(We)^T + be          fp32 accumulate, q = bf16 round-to-nearest-even
//     p = softmax(z)                 fp32
//     x' = x + P~ q(Wp)^T + bp       fp32 in, fp32 out (y may alias x)
//
// D -> V -> D with a row softmax in the middle: the fused FFN's shape (rsgemm.hip), and its layout.  A wave owns 32 rows; lane l holds row (l & 31), the
// two half-lanes split every group of 16 columns.  The vocabulary streams through in chunks of 32 columns: the first product leaves a lane with 16 logits
// of ITS OWN row, so the row maximum and the row sum need one xor-32 shuffle, and - with Wp's K index permuted per 16 at pack time - the packed
// exponentials are directly the B fragments of the second product.  Online softmax over the chunks: P~ = bf16(exp(z - m)) against the running maximum m,
// the output accumulators and the running sum are rescaled by exp(m_old - m_new) when a chunk raises it, and the division by the row sum happens once, in
// the epilogue.  The (M, V) logits never exist in memory.
//
// The weight ring holds ONE operand per entry (entry 2c = the 32 rows of We of chunk c, entry 2c + 1 = the 32 K-columns of Wp of chunk c, both KS KiB), so
// that three entries fit the LDS at the widest stage (De = 720: 48 KiB each).  Widths above 256 (KS 24 / 32 / 48) split a row tile's OUTPUT columns over a
// pair of waves: both compute the logits of the tile (identical instructions on identical operands: identical statistics, no exchange), each keeps half of
// the output accumulators - 192 registers instead of 384 at De = 720.  The KS = 48 instance still carries scratch (DESIGN.md section 6h says what it costs).
//
// Padded vocabulary columns (V..Vp) get logit -inf and probability 0 by selection; nothing read from a padded weight row reaches a result.  Rows beyond M
// are clamped on load and masked on store.  MODE 1 is the opt-in probability output: two sweeps over We only (statistics, then exp(z - m) / l stored).
#include "kernels.h"
#include "rowstat.h"

#include <cmath>

namespace {

template <int KS, int NBUF, int NW>
struct IcSmem {
    static constexpr int ENT = KS * 1024;                 // one ring entry: 32 rows x KS k-steps of We, or KS * 16 rows x 32 columns of Wp
    static constexpr int RING = NBUF * ENT;
    static constexpr int STAGE = NW * STG_BYTES;
    static constexpr int BIAS = (1024 + KS * 16) * 4;     // be padded to Vp <= 1024, bp padded to KS * 16
    static constexpr bool ALIAS = RING + STAGE + BIAS > 160 * 1024;      // staging inside the last ring buffer (free in the prologue and after the loop)
    static_assert(!ALIAS || ENT >= STAGE, "staging region must fit one ring entry");
    static constexpr int TOTAL = RING + BIAS + (ALIAS ? 0 : STAGE);
};

// This lane's row as bf16 B fragments (columns 16 s + 8 half + 0..7 of row lr), fetched through the staging region like rowstat.h's fetch_row_f32 but packed
// window by window: the fp32 row (8 KS registers) never exists at once - at KS = 48 it would not fit next to the fragments.  Columns >= D are zeroed by
// selection (the clamped loads hold other columns there)
template <int KS, int W>
__device__ __forceinline__ void ic_take_window(const char* stg, int lr, int half, int D, bf16x8 (&xf)[KS]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (4 * W + j < KS) {
            const char* src = stg + lr * STG_ROW + (16 * j + 8 * half) * 4;
            const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 16);
            const int c0 = (4 * W + j) * 16 + half * 8;
            const bool va = c0 < D, vb = c0 + 4 < D;
            const uint32_t ka = va ? ~0u : 0u, kb = vb ? ~0u : 0u;          // bit masks, not branches: the packs run unconditionally
            uint4 w;
            w.x = pack_bf2(a.x, a.y) & ka; w.y = pack_bf2(a.z, a.w) & ka;
            w.z = pack_bf2(b.x, b.y) & kb; w.w = pack_bf2(b.z, b.w) & kb;
            xf[4 * W + j] = as_bf16x8(w);
        }
    }
}
template <int KS, int W0>
__device__ __forceinline__ void ic_fetch_rows(const char* X, size_t pitch, int D, int m_base, int M, char* stg, int lane, bf16x8 (&xf)[KS]) {
    constexpr int NWIN = (KS + 3) / 4;
    if constexpr (W0 < NWIN) {
        u32x4 v[16] = {};
        stage_load<0>(X, pitch, D * 4, m_base, M, 256 * W0, lane, v);
        if constexpr (W0 + 1 < NWIN) stage_load<8>(X, pitch, D * 4, m_base, M, 256 * (W0 + 1), lane, v);
        wave_sync();
        stage_put<0>(stg, lane, v);
        wave_sync();
        ic_take_window<KS, W0>(stg, lane & 31, lane >> 5, D, xf);
        if constexpr (W0 + 1 < NWIN) {
            wave_sync();
            stage_put<8>(stg, lane, v);
            wave_sync();
            ic_take_window<KS, W0 + 1>(stg, lane & 31, lane >> 5, D, xf);
        }
        ic_fetch_rows<KS, W0 + 2>(X, pitch, D, m_base, M, stg, lane, xf);
    }
}

// y = x + (acc + bp) on 64-column windows (acc already divided by the row sum): the residual tile comes in coalesced through the staging region, every lane
// updates its own elements, the tile leaves coalesced.  t0: first of the wave's NT output tiles (a multiple of 2: window t0 / 2)
template <int NT, int W>
__device__ __forceinline__ void ic_epilogue(const char* xb, char* yb, size_t xpitch, size_t ypitch, int row_bytes, int m_base, int M, char* stg, int lane,
                                            const float* sb2, int t0, const f32x16 (&acc)[NT]) {
    if constexpr (2 * W < NT) {
        const int lr = lane & 31, half = lane >> 5;
        u32x4 v[8] = {};
        stage_load<0>(xb, xpitch, row_bytes, m_base, M, 128 * t0 + 256 * W, lane, v);
        wave_sync();
        stage_put<0>(stg, lane, v);
        wave_sync();
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            if (2 * W + tt < NT) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float4* cell = reinterpret_cast<float4*>(stg + lr * STG_ROW + (tt * 32 + q * 8 + half * 4) * 4);
                    const float4 bv = *reinterpret_cast<const float4*>(sb2 + (t0 + 2 * W + tt) * 32 + q * 8 + half * 4);
                    const float4 x4 = *cell;
                    float4 o;
                    o.x = x4.x + (acc[2 * W + tt][q * 4 + 0] + bv.x);
                    o.y = x4.y + (acc[2 * W + tt][q * 4 + 1] + bv.y);
                    o.z = x4.z + (acc[2 * W + tt][q * 4 + 2] + bv.z);
                    o.w = x4.w + (acc[2 * W + tt][q * 4 + 3] + bv.w);
                    *cell = o;
                }
            }
        }
        wave_sync();
        stage_store(stg, yb, ypitch, row_bytes, m_base, M, 128 * t0 + 256 * W, lane);
        wave_sync();
        ic_epilogue<NT, W + 1>(xb, yb, xpitch, ypitch, row_bytes, m_base, M, stg, lane, sb2, t0, acc);
    }
}

// KS: k16-steps over De (De <= 16 KS); SPLIT: waves per row tile (output column parts); NW: waves; NBUF: ring depth; MODE 0: the step, 1: probabilities only
template <int KS, int SPLIT, int NW, int NBUF, int MODE>
__global__ __launch_bounds__(NW * 64) void interctc_kernel(const InterCtcParams p) {
    using SM = IcSmem<KS, NBUF, NW>;
    static_assert(KS % NW == 0 && KS % (2 * SPLIT) == 0, "uniform DMA count per wave, whole output tiles per wave");
    constexpr int PER = KS / NW;                           // DMA instructions per wave and ring entry
    constexpr int P1 = 2 * KS;                             // 16-byte pieces per We row
    constexpr int NT = KS / 2 / SPLIT;                     // 32-column output tiles of this wave
    constexpr int NTHR = NW * 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sb1 = reinterpret_cast<float*>(smem + SM::RING);
    float* sb2 = sb1 + 1024;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31, half = lane >> 5;
    const int part = wave % SPLIT;
    const int m_base = (blockIdx.x * (NW / SPLIT) + wave / SPLIT) * 32;
    const int nchunks = p.Vp / CH;
    const int nent = 2 * nchunks;
    char* stg = (SM::ALIAS ? smem + (NBUF - 1) * SM::ENT : reinterpret_cast<char*>(sb2 + KS * 16)) + wave * STG_BYTES;

    // per-lane byte offsets of this wave's DMA instructions, computed once for both entry kinds (rowstat.h)
    uint32_t doff1[PER], doff2[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        doff1[k] = dma_rows32_off<P1>(p.ldw1, wave + NW * k, lane);
        doff2[k] = dma_w2_off(p.ldw2, wave + NW * k, lane);
    }
    // MODE 0: entry e = We chunk e / 2 (even) | Wp chunk e / 2 (odd); MODE 1: We chunk e mod nchunks, two sweeps
    auto issue = [&](int e) {
        char* buf = smem + (e % NBUF) * SM::ENT;
        const bool first = MODE == 1 || !(e & 1);
        const int c = MODE == 1 ? (e < nchunks ? e : e - nchunks) : e >> 1;
        if (first) {
            const char* w1 = reinterpret_cast<const char*>(p.W1 + (size_t)c * CH * p.ldw1);
#pragma unroll
            for (int k = 0; k < PER; ++k) glds16(w1, doff1[k], buf + 64 * (wave + NW * k) * 16);
        } else {
            const char* w2 = reinterpret_cast<const char*>(p.W2 + c * CH);
#pragma unroll
            for (int k = 0; k < PER; ++k) glds16(w2, doff2[k], buf + 64 * (wave + NW * k) * 16);
        }
    };

    for (int i = tid; i < 1024; i += NTHR) sb1[i] = i < p.V ? p.b1[i] : 0.f;
    for (int i = tid; i < KS * 16; i += NTHR) sb2[i] = i < p.D ? p.b2[i] : 0.f;
#pragma unroll
    for (int e = 0; e < NBUF - 1; ++e)
        if (e < nent) issue(e);
    // this lane's row as bf16 B fragments: columns 16 s + 8 half + (0..7); columns >= De and nothing else are zeroed (clamped loads hold other columns there)
    bf16x8 xf[KS];
    ic_fetch_rows<KS, 0>(reinterpret_cast<const char*>(p.X), (size_t)p.ldx * 4, p.D, m_base, p.M, stg, lane, xf);
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float mrun = -INFINITY, lrun = 0.f;                     // running maximum of the row (both half-lanes agree), this half-lane's share of the running sum

    const int q0 = (half + lr) % P1;
    const int k2 = (half + (lr >> 2)) & 3;
    const int w2off0 = lr * 64 + k2 * 16, w2off1 = lr * 64 + (k2 ^ 2) * 16;
    constexpr int FB = (KS % 8 == 0 && KS <= 16) ? 8 : ((KS % 4 == 0) ? 4 : KS);      // fragment batches (a divisor of KS)

    // entry e: wait until it has landed (this wave's pieces), meet the other waves (theirs have too, and everybody is done with entry e - 1), refill that buffer
    auto next_entry = [&](int e) -> const char* {
        wait_chunks<PER, NBUF - 2>(nent - 1 - e);
        wg_barrier();
        if (e + NBUF - 1 < nent) issue(e + NBUF - 1);
        return smem + (e % NBUF) * SM::ENT;
    };
    // logits of chunk c from a We entry: Z^T[j][m] = sum_k We[32 c + j][k] x[m][k] + be.  Register r <-> vocabulary column 32 c + (r & 3) + 8 (r >> 2) + 4 half;
    // a padded column's logit is -inf by selection.  Returns the row maximum over the chunk (both half-lanes)
    auto logits = [&](const char* buf, int c, float (&z)[16]) -> float {
        const char* w1 = buf + lr * (P1 * 16);
        f32x16 h;
#pragma unroll
        for (int r = 0; r < 16; ++r) h[r] = 0.f;
#pragma unroll
        for (int s0 = 0; s0 < KS; s0 += FB) {
            bf16x8 wa[FB];
#pragma unroll
            for (int i = 0; i < FB; ++i) {
                int q = q0 + 2 * (s0 + i);
                q -= q >= P1 ? P1 : 0;
                wa[i] = *reinterpret_cast<const bf16x8*>(w1 + q * 16);
            }
#pragma unroll
            for (int i = 0; i < FB; ++i) h = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[i], xf[s0 + i], h, 0, 0, 0);
        }
        // be of the lane's four runs of four columns by unconditional 16-byte LDS reads (padded with zeros to 1024), then selects on register values only:
        // per-element conditional reads became sixteen exec-masked blocks, each waiting for its own LDS round trip
        const float* b1 = sb1 + c * CH + 4 * half;
        const int rem = p.V - c * CH - 4 * half;            // local column (r & 3) + 8 (r >> 2) exists iff it is < rem
        float cmax = -INFINITY;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 bv = *reinterpret_cast<const float4*>(b1 + 8 * q);
            const float b4[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float v = h[4 * q + i] + b4[i];
                z[4 * q + i] = 8 * q + i < rem ? v : -INFINITY;
                cmax = fmaxf(cmax, z[4 * q + i]);
            }
        }
        return fmaxf(cmax, __shfl_xor(cmax, 32));
    };
    // online softmax: z -> exp(z - m) against the new running maximum (0 by selection in padded columns); returns the factor exp(m_old - m_new) everything
    // accumulated so far is rescaled by (0 at chunk 0, where m_old = -inf and m_new is finite: column 0 exists)
    auto online = [&](int c, float cmax, float (&z)[16]) -> float {
        const float mnew = fmaxf(mrun, cmax);
        const float scale = __expf(mrun - mnew);
        mrun = mnew;
        const int rem = p.V - c * CH - 4 * half;
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t keep = (r & 3) + 8 * (r >> 2) < rem ? ~0u : 0u;      // a bit mask selects: whatever the exponential of a padded column is, 0 remains
            z[r] = __uint_as_float(__float_as_uint(__expf(z[r] - mnew)) & keep);
            psum += z[r];
        }
        lrun = lrun * scale + psum;
        return scale;
    };

    if constexpr (MODE == 0) {
        for (int c = 0; c < nchunks; ++c) {
            float z[16];
            const float cmax = logits(next_entry(2 * c), c, z);
            const float scale = online(c, cmax, z);
            // registers [8 s, 8 s + 8) are the B fragment of k-step s of the second product
            bf16x8 hf[2];
            hf[0] = as_bf16x8(make_uint4(pack_bf2(z[0], z[1]), pack_bf2(z[2], z[3]), pack_bf2(z[4], z[5]), pack_bf2(z[6], z[7])));
            hf[1] = as_bf16x8(make_uint4(pack_bf2(z[8], z[9]), pack_bf2(z[10], z[11]), pack_bf2(z[12], z[13]), pack_bf2(z[14], z[15])));
            // ---- Y^T[n][m] += sum_j Wp'[n][j] P~^T[j][m] on this wave's output tiles
            const char* w2 = next_entry(2 * c + 1) + part * NT * 2048;
            constexpr int TB = (NT % 4 == 0 && KS <= 16) ? 4 : ((NT % 2 == 0) ? 2 : 1);
#pragma unroll
            for (int t0 = 0; t0 < NT; t0 += TB) {
                bf16x8 wb[TB][2];
#pragma unroll
                for (int i = 0; i < TB; ++i) {
                    wb[i][0] = *reinterpret_cast<const bf16x8*>(w2 + (t0 + i) * 2048 + w2off0);
                    wb[i][1] = *reinterpret_cast<const bf16x8*>(w2 + (t0 + i) * 2048 + w2off1);
                }
                // the rescale of what the earlier chunks left in a tile sits right in front of the tile's products, batch by batch (sched_barrier: rescaling all
                // tiles in one block made the scheduler keep a second copy of the accumulators - 16 NT more registers, spills from KS = 24 on)
#pragma unroll
                for (int i = 0; i < TB; ++i) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[t0 + i][r] *= scale;
                    acc[t0 + i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wb[i][0], hf[0], acc[t0 + i], 0, 0, 0);
                    acc[t0 + i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wb[i][1], hf[1], acc[t0 + i], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    } else {
        for (int c = 0; c < nchunks; ++c) {                 // first sweep: the row statistics
            float z[16];
            const float cmax = logits(next_entry(c), c, z);
            (void)online(c, cmax, z);
        }
        // second sweep: the normalised probabilities, in the reference's order exp(z - max) / sum.  A pair of waves (SPLIT = 2) shares the chunks
        const float inv_l = 1.0f / (lrun + __shfl_xor(lrun, 32));
        const int m = m_base + lr;
        for (int c = 0; c < nchunks; ++c) {
            float z[16];
            (void)logits(next_entry(nchunks + c), c, z);
            if (m < p.M && c % SPLIT == part) {
                float* pr = p.probs + (size_t)m * p.V + c * CH;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (c * CH + j < p.V) pr[j] = __expf(z[r] - mrun) * inv_l;
                }
            }
        }
    }
    if constexpr (MODE == 0) {
        // ---- epilogue: y[m][n] = x[m][n] + acc / l + bp[n]
        const float inv = 1.0f / (lrun + __shfl_xor(lrun, 32));
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] *= inv;
        if constexpr (SM::ALIAS) wg_barrier();             // every wave is done with the ring before it becomes staging memory
        ic_epilogue<NT, 0>(reinterpret_cast<const char*>(p.X), reinterpret_cast<char*>(p.Y), (size_t)p.ldx * 4, (size_t)p.ldy * 4, p.D * 4, m_base, p.M,
                           stg, lane, sb2, part * NT, acc);
    }
}

template <int KS, int SPLIT, int NW, int NBUF, int MODE>
int launch_ic_t(const InterCtcParams& p, hipStream_t s) {
    using SM = IcSmem<KS, NBUF, NW>;
    if (p.ldw1 < KS * 16) return -6;        // every We row is read KS * 16 columns wide, Wp has KS * 16 rows: the packing must be that large (pack.hip)
    static LdsAttr attr;
    ensure_dynamic_lds(reinterpret_cast<const void*>(&interctc_kernel<KS, SPLIT, NW, NBUF, MODE>), SM::TOTAL, attr);
    const int rows_per_wg = NW / SPLIT * 32;
    hipLaunchKernelGGL((interctc_kernel<KS, SPLIT, NW, NBUF, MODE>), dim3((p.M + rows_per_wg - 1) / rows_per_wg), dim3(NW * 64), SM::TOTAL, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int MODE>
int launch_ic_mode(const InterCtcParams& p, hipStream_t s) {
    switch (interctc_ks_class(p.D)) {
        case 2: return launch_ic_t<2, 1, 2, 4, MODE>(p, s);
        case 4: return launch_ic_t<4, 1, 4, 4, MODE>(p, s);
        case 8: return launch_ic_t<8, 1, 4, 4, MODE>(p, s);
        case 12: return launch_ic_t<12, 1, 4, 4, MODE>(p, s);
        case 16: return launch_ic_t<16, 1, 4, 4, MODE>(p, s);
        case 24: return launch_ic_t<24, 2, 4, 4, MODE>(p, s);      // one wave per tile: 288 resident registers (fragments + accumulators), 620 bytes of scratch
        case 32: return launch_ic_t<32, 2, 4, 3, MODE>(p, s);
        case 48: return launch_ic_t<48, 2, 4, 3, MODE>(p, s);
    }
    return -2;
}

// exact modes: p = exp(z - max) / sum per row, in place, one wave per row (the reference's order; torch softmax)
__global__ __launch_bounds__(256) void row_softmax_kernel(float* z, int M, int V) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    float* r = z + (size_t)row * V;
    float mx = -INFINITY;
    for (int i = lane; i < V; i += 64) mx = fmaxf(mx, r[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.f;
    for (int i = lane; i < V; i += 64) { const float e = expf(r[i] - mx); r[i] = e; sum += e; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    for (int i = lane; i < V; i += 64) r[i] = r[i] / sum;
}

}  // namespace

int interctc_ks_class(int D) {
    if (D <= 0 || D % 4 || D > 768) return 0;
    const int ks = (D + 15) / 16;
    for (int c : {2, 4, 8, 12, 16, 24, 32, 48}) if (ks <= c) return c;
    return 0;
}
bool interctc_supported(int D, int V) { return interctc_ks_class(D) != 0 && V >= 2 && V <= 1024; }

int launch_interctc(const InterCtcParams& p, hipStream_t s) {
    if (p.M <= 0) return 0;
    if (!interctc_supported(p.D, p.V) || p.Vp != ec_round_up(p.V, CH) || p.ldw1 % 8 || p.ldw2 % 8 || p.ldw2 < p.Vp) return -2;
    // the probabilities first: they read the rows the step then overwrites when y aliases x
    if (p.probs) { const int rc = launch_ic_mode<1>(p, s); if (rc) return rc; }
    return p.Y ? launch_ic_mode<0>(p, s) : 0;
}

int launch_row_softmax(float* z, int M, int V, hipStream_t s) {
    if (M <= 0) return 0;
    hipLaunchKernelGGL(row_softmax_kernel, dim3((M + 3) / 4), dim3(256), 0, s, z, M, V);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
