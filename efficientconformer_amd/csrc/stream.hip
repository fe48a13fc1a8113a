// Chunked streaming inference: the two frame-mixing kernels of a causal encoder that sees its input a chunk at a time.
//
// stream_attention_kernel - a chunk brings a few grouped query rows per stream and meets hundreds of cached key rows: the opposite aspect ratio of
// attention2.hip (32 queries per wave, tiles over queries).  Here a workgroup is (stream, head, 16 queries) and its four waves SPLIT THE KEY RANGE: wave w takes
// the 32-key blocks w, w + 4, .. of the tile's visible keys [max(i0 - band_l, pos - cached), i0 + 15], keeps its own running (max, sum, accumulator) and the four
// partials merge through LDS.  Per 32-key block, v_mfma_f32_16x16x32_bf16 throughout:
//     S^T = K Qu^T       A = 16 key rows (16-byte loads straight from the ring or the chunk), B = the tile's Qu fragments (registers): lane (g, li) gets
//                        keys 4 g + r of query li - which IS the B-operand layout of the P V product (k index = key), so P never moves between lanes
//     R^T = E Qv^T       three 16-row tiles of the 47 distances a 16 x 32 tile can see; E is indexed by the distance i - j alone (stream.h), so the rows
//                        are i0 - j0 + 15 - c.  The relative-to-absolute skew is one trip through a per-wave LDS buffer: written [query][c], read at
//                        c = jj - ii + 15
//     O^T += V^T P^T     A = V^T gathered as 2-byte loads (8 keys x one column per lane), B = P (bf16), C = O^T: query li's row statistics and its
//                        accumulator columns share a lane, the rescale needs no shuffle
// The softmax is the online one in the exp2 domain; p is rounded to bf16 for the product and summed unrounded (the noise model of tests/attention_cases.py).
// Masked keys are never LOADED (their slots may hold anything, NaN included): K, V and E loads are predicated on the key's / distance's validity and 16-byte
// chunks are masked to the head span (mask_chunk), as in attention2.hip.  Every launch is one round: no spinning, nothing persistent.
//
// stream_dwconv_kernel - dwconv_kernel's tap nest (conv.hip: channel pairs, the pair's taps in registers, rows streamed once through LDS, the same FMA order)
// on 32-output tiles, the k - 1 rows in front of the chunk taken from the stream's state.
#include "stream.h"
#include "encoder_state.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int SA_NW = 4;           // waves per workgroup: they split the key range
constexpr int SA_QT = 16;          // queries per workgroup
constexpr int SA_KB = 32;          // keys per wave and iteration
constexpr int SA_SKEW = 49;        // floats per query row of the skew buffer: 47 distances + 2 (odd: rows on rotating banks)
constexpr float LOG2E = 1.44269504088896f;

__device__ __forceinline__ uint4 sa_ld16(const bf16_t* p) {    // 16-byte global load from a 2-byte aligned address (odd head widths)
    typedef uint32_t u32x4_a2 __attribute__((ext_vector_type(4), aligned(2)));
    const u32x4_a2 v = *reinterpret_cast<const u32x4_a2*>(p);
    return make_uint4(v[0], v[1], v[2], v[3]);
}

// 8 columns [col, col + 8) of a head span of d columns at `row`, zero where ok is false or the column lies behind the span
__device__ __forceinline__ bf16x8 sa_frag(const bf16_t* row, int col, int d, bool ok) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (ok && col < d) v = mask_chunk(sa_ld16(row + col), d - col);
    return as_bf16x8(v);
}

__device__ __forceinline__ uint32_t sa_add2(uint32_t w, float a, float b) {       // two bf16 + two floats -> two bf16 (RNE)
    return pack_bf2(__uint_as_float(w << 16) + a, __uint_as_float(w & 0xFFFF0000u) + b);
}

template <int DP>
struct StreamAttnSmem {
    static constexpr int SKEW_F = SA_NW * SA_QT * SA_SKEW, PART_F = SA_NW * SA_QT * DP, STAT_F = SA_NW * SA_QT * 2;
    static constexpr int TOTAL = (SKEW_F + PART_F + STAT_F) * 4;
};

template <int DP>
__global__ __launch_bounds__(SA_NW * 64) void stream_attention_kernel(const StreamAttnParams p) {
    constexpr int KS = DP / 32, CT = DP / 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* skew = reinterpret_cast<float*>(smem);
    float* part = skew + StreamAttnSmem<DP>::SKEW_F;
    float* stat = part + StreamAttnSmem<DP>::PART_F;
    const int b = blockIdx.z, h = blockIdx.y;
    const int G = p.G, D = p.D, d = p.d;
    const int n = p.rows[b];
    const int ng = (n + G - 1) / G;                         // grouped query rows of this stream's chunk
    const int q0 = blockIdx.x * SA_QT;
    if (q0 >= ng) return;                                   // uniform over the workgroup
    const int nq = min(SA_QT, ng - q0);
    const int pos = p.pos[b], cached = p.cached[b];
    const size_t row0 = (size_t)p.row_off[b];
    const int i0 = pos + q0;                                // absolute position of the tile's first query
    const int first = pos - cached;                         // oldest cached key
    const int band_l = min(p.band_l, 1 << 30);
    const int jlo = max(first, i0 - band_l), jhi = i0 + nq - 1;          // visible keys of the tile (jlo <= i0: the tile's own keys are in)
    const int nblk = (jhi - jlo) / SA_KB + 1;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, g = lane >> 4;
    const size_t GD = (size_t)G * D;
    const int sb = p.slot ? p.slot[b] : b;                  // the stream's place in the state
    const bf16_t* kc = p.kc + (size_t)sb * p.cap * GD;
    const bf16_t* vc = p.vc + (size_t)sb * p.cap * GD;
    const int hcol = h * d;

    // the tile's queries: Qu as stored, Qv = bf16(Qu + (v - u)); rows >= nq are zero (and masked below)
    bf16x8 qu[KS], qv[KS];
    {
        const bf16_t* qrow = p.qu + (row0 + (size_t)(q0 + li) * G) * D + hcol;
        const float* dv = p.dvu + (size_t)h * p.dvu_ld;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int col = 32 * ks + 8 * g;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (li < nq && col < d) v = mask_chunk(sa_ld16(qrow + col), d - col);
            qu[ks] = as_bf16x8(v);
            uint4 s = make_uint4(0u, 0u, 0u, 0u);
            if (li < nq && col < d) {                        // dvu is zero behind d (and dvu_ld >= dpad): the masked columns stay 0
                const float4 a = *reinterpret_cast<const float4*>(dv + col), c = *reinterpret_cast<const float4*>(dv + col + 4);
                s = make_uint4(sa_add2(v.x, a.x, a.y), sa_add2(v.y, a.z, a.w), sa_add2(v.z, c.x, c.y), sa_add2(v.w, c.z, c.w));
            }
            qv[ks] = as_bf16x8(s);
        }
    }
    const float scale2 = p.scale * LOG2E;
    const float NEG_INF = -__builtin_inff();
    float m = NEG_INF, l = 0.f;                              // query li's running maximum (log2 units) and this lane's share of its sum
    f32x4 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    float* sk = skew + (w * SA_QT + li) * SA_SKEW;

    for (int blk = w; blk < nblk; blk += SA_NW) {
        const int j0 = jlo + SA_KB * blk;
        // ---- S^T = K Qu^T: tile t holds keys j0 + 16 t + 4 g + r of query li
        f32x4 st[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int j = j0 + 16 * t + li;
            const bool ok = j <= jhi;
            const bf16_t* krow = j >= pos ? p.k + (row0 + (size_t)(j - pos) * G) * D + hcol : kc + (size_t)(p.cap ? j % p.cap : 0) * GD + hcol;
            st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sa_frag(krow, 32 * ks + 8 * g, d, ok), qu[ks], st[t], 0, 0, 0);
        }
        // ---- R^T = E Qv^T over the distances i0 - j0 + 15 - c, c < 48, then the skew through LDS
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int delta = i0 - j0 + 15 - (16 * t + li);
            const bool ok = delta >= 0 && delta < p.n_dist;
            const bf16_t* erow = p.e + (size_t)(ok ? p.n_dist - 1 - delta : 0) * GD + hcol;      // the causal table's own order
            f32x4 pe = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) pe = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sa_frag(erow, 32 * ks + 8 * g, d, ok), qv[ks], pe, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) { const int c = 16 * t + 4 * g + r; sk[c] = pe[r]; }
        }
        wave_sync();
        float s[2][4], bm = NEG_INF;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jj = 16 * t + 4 * g + r;
                const int dist = i0 + li - (j0 + jj);        // i - j
                const bool vis = li < nq && dist >= 0 && dist <= band_l;      // j >= first: jlo >= first
                const float rel = sk[jj - li + 15];
                s[t][r] = vis ? (st[t][r] + rel) * scale2 : NEG_INF;
                bm = fmaxf(bm, s[t][r]);
            }
        wave_sync();                                         // the next block's skew writes come after these reads
        bm = fmaxf(bm, __shfl_xor(bm, 16));
        bm = fmaxf(bm, __shfl_xor(bm, 32));
        const float mn = fmaxf(m, bm);
        float alpha = 1.f, ps = 0.f;
        float pr[2][4];
        if (mn == NEG_INF) {                                 // no visible key for this query so far
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) pr[t][r] = 0.f;
        } else {
            alpha = __builtin_amdgcn_exp2f(m - mn);          // m = -inf: 0
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) { pr[t][r] = __builtin_amdgcn_exp2f(s[t][r] - mn); ps += pr[t][r]; }
        }
        m = mn;
        l = l * alpha + ps;
        union { uint4 u; bf16x8 b; } pb;                     // P as the B operand: k slot 8 g + x <-> key 16 (x / 4) + 4 g + x % 4
        pb.u = make_uint4(pack_bf2(pr[0][0], pr[0][1]), pack_bf2(pr[0][2], pr[0][3]), pack_bf2(pr[1][0], pr[1][1]), pack_bf2(pr[1][2], pr[1][3]));
        // ---- O^T += V^T P^T: this lane's 8 keys, one column per 16-column tile
        const bf16_t* vrow[8];
        bool vok[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int j = j0 + 16 * (x >> 2) + 4 * g + (x & 3);
            vok[x] = j <= jhi;
            vrow[x] = j >= pos ? p.v + (row0 + (size_t)(j - pos) * G) * D + hcol : vc + (size_t)(p.cap ? j % p.cap : 0) * GD + hcol;
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int col = 16 * ct + li;
            uint32_t e[8];
#pragma unroll
            for (int x = 0; x < 8; ++x) e[x] = (vok[x] && col < d) ? (uint32_t)vrow[x][col] : 0u;
            const uint4 va = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[ct][r] *= alpha;
            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(va), pb.b, acc[ct], 0, 0, 0);
        }
    }
    // ---- merge the four waves' partials
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    {
        float* pw = part + (size_t)(w * SA_QT + li) * DP;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) pw[16 * ct + 4 * g + r] = acc[ct][r];
        if (g == 0) { stat[(w * SA_QT + li) * 2] = m; stat[(w * SA_QT + li) * 2 + 1] = l; }
    }
    __syncthreads();
    for (int idx = tid; idx < SA_QT * DP; idx += SA_NW * 64) {
        const int q = idx / DP, c = idx % DP;
        if (q >= nq || c >= d) continue;
        float mx = NEG_INF;
#pragma unroll
        for (int ww = 0; ww < SA_NW; ++ww) mx = fmaxf(mx, stat[(ww * SA_QT + q) * 2]);
        float den = 0.f, num = 0.f;                          // mx is finite: a live query sees its own key
#pragma unroll
        for (int ww = 0; ww < SA_NW; ++ww) {
            const float mw = stat[(ww * SA_QT + q) * 2];
            const float f = mw == NEG_INF ? 0.f : __builtin_amdgcn_exp2f(mw - mx);
            den += f * stat[(ww * SA_QT + q) * 2 + 1];
            num += f * part[(size_t)(ww * SA_QT + q) * DP + c];
        }
        const int cf = hcol + c;                             // column of the grouped row -> (frame of the group, column)
        const int frame = (q0 + q) * G + cf / D;
        p.out[(row0 + frame) * p.ldo + cf % D] = frame < n ? f2bf(num / den) : (bf16_t)0;
    }
}

// the chunk's last min(ng, cap) grouped K / V rows -> their ring slots; 4-byte copies (D is even)
__global__ __launch_bounds__(256) void stream_kv_append_kernel(const StreamAttnParams p) {
    const int b = blockIdx.y;
    const int n = p.rows[b];
    if (n <= 0 || p.cap <= 0) return;
    const int sb = p.slot ? p.slot[b] : b;
    const int ng = (n + p.G - 1) / p.G, pos = p.pos[b];
    const int t0 = max(0, ng - p.cap);
    const int words = p.G * p.D / 2;
    const size_t GD = (size_t)p.G * p.D;
    for (int t = t0 + blockIdx.x; t < ng; t += gridDim.x) {
        const size_t src = ((size_t)p.row_off[b] + (size_t)t * p.G) * p.D;
        const size_t dst = ((size_t)sb * p.cap + (size_t)((pos + t) % p.cap)) * GD;
        const uint32_t* ks = reinterpret_cast<const uint32_t*>(p.k + src);
        const uint32_t* vs = reinterpret_cast<const uint32_t*>(p.v + src);
        uint32_t* kd = reinterpret_cast<uint32_t*>(p.kc + dst);
        uint32_t* vd = reinterpret_cast<uint32_t*>(p.vc + dst);
        for (int i = threadIdx.x; i < words; i += 256) { kd[i] = ks[i]; vd[i] = vs[i]; }
    }
}

template <int DP>
int launch_sa(const StreamAttnParams& p, hipStream_t s) {
    const int tiles = ec_cdiv(ec_cdiv(p.max_rows, p.G), SA_QT);
    static LdsAttr attr;
    ensure_dynamic_lds(reinterpret_cast<const void*>(&stream_attention_kernel<DP>), StreamAttnSmem<DP>::TOTAL, attr);
    hipLaunchKernelGGL((stream_attention_kernel<DP>), dim3(tiles, p.H, p.B), dim3(SA_NW * 64), StreamAttnSmem<DP>::TOTAL, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------- depthwise convolution with a carried left halo
constexpr int SD_NT = 4;                       // outputs per thread
constexpr int SD_TT = 8 * SD_NT;               // output frames per workgroup
constexpr int SD_CC = 64;                      // channels per workgroup
constexpr int SD_PITCH = SD_CC * 2 + 16;       // bytes per LDS row

typedef float sdf2 __attribute__((ext_vector_type(2)));

template <int KSZ, int STRIDE>
__global__ __launch_bounds__(256) void stream_dwconv_kernel(const StreamDwParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int ROWS = (SD_TT - 1) * STRIDE + KSZ;
    constexpr int TROWS = (SD_NT - 1) * STRIDE + KSZ;
    const int C = p.C, ld = p.ld;
    const int ctiles = (C + SD_CC - 1) / SD_CC;
    const int ct = blockIdx.x % ctiles, tt = blockIdx.x / ctiles, b = blockIdx.y;
    const int n = p.rows[b];
    const int To = n > 0 ? (n - 1) / STRIDE + 1 : 0;
    const int to0 = tt * SD_TT;
    if (to0 >= To) return;                                                  // uniform over the workgroup
    const int hist = p.hist[b];
    const int c0 = ct * SD_CC;
    const int tin0 = to0 * STRIDE - (KSZ - 1);                              // first input row of the tile, relative to the chunk: >= -(KSZ - 1)
    const int tid = threadIdx.x;
    const int cp = tid & 31, tg = tid >> 5;
    const int c = c0 + 2 * cp;
    sdf2 w[KSZ], bz;
    {
        const unsigned ca = c < C ? c : C - 1, cb = c + 1 < C ? c + 1 : C - 1;
#pragma unroll
        for (int j = 0; j < KSZ; ++j) {
            const float wa = p.w_kc[(unsigned)(j * C) + ca], wb = p.w_kc[(unsigned)(j * C) + cb];
            w[j] = sdf2{c < C ? wa : 0.f, c + 1 < C ? wb : 0.f};
        }
        const float ba = p.bias[ca], bb = p.bias[cb];
        bz = sdf2{c < C ? ba : 0.f, c + 1 < C ? bb : 0.f};
    }
    {
        const bf16_t* gb = p.g + (size_t)p.in_off[b] * ld;
        const bf16_t* sb = p.state + (size_t)(p.slot ? p.slot[b] : b) * (KSZ - 1) * ld;
        for (int i = tid; i < ROWS * (SD_CC / 8); i += 256) {
            const int r = i >> 3, ch = (i & 7) * 8;
            const int t = tin0 + r, cq = c0 + ch;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (cq < ld && cq < C) {
                // t < 0: state row KSZ - 1 + t, valid iff it is one of the last `hist`; t >= n: behind the chunk (feeds no kept output)
                if (t < 0) { if (-t <= hist) v = *reinterpret_cast<const uint4*>(sb + (size_t)(KSZ - 1 + t) * ld + cq); }
                else if (t < n) v = *reinterpret_cast<const uint4*>(gb + (size_t)t * ld + cq);
                v = mask_chunk(v, C - cq);
            }
            *reinterpret_cast<uint4*>(smem + r * SD_PITCH + ch * 2) = v;
        }
    }
    __syncthreads();
    sdf2 acc[SD_NT];
#pragma unroll
    for (int o = 0; o < SD_NT; ++o) acc[o] = bz;
    const char* base = smem + (tg * SD_NT * STRIDE) * SD_PITCH + cp * 4;
#pragma unroll
    for (int r = 0; r < TROWS; ++r) {
        const uint32_t raw = *reinterpret_cast<const uint32_t*>(base + r * SD_PITCH);
        const sdf2 x = sdf2{__uint_as_float(raw << 16), __uint_as_float(raw & 0xFFFF0000u)};
#pragma unroll
        for (int o = 0; o < SD_NT; ++o) {
            const int tap = r - o * STRIDE;                                 // static after unrolling
            if (tap >= 0 && tap < KSZ) acc[o] = __builtin_elementwise_fma(w[tap], x, acc[o]);
        }
    }
    if (c < ld) {   // ld is even: the pair is inside the row; channels >= C have zero taps and bias, swish(0) = 0 keeps the pad columns zero
        bf16_t* ob = p.out + (size_t)p.out_off[b] * ld;
#pragma unroll
        for (int o = 0; o < SD_NT; ++o) {
            const int to = to0 + tg * SD_NT + o;
            if (to < To) *reinterpret_cast<uint32_t*>(ob + (size_t)to * ld + c) = pack_bf2(swishf_(acc[o].x), swishf_(acc[o].y));
        }
        // the rows that pad the chunk to the next block's group size (a final chunk): zeros, written by the chunk's last tile
        if (p.out_end && to0 + SD_TT >= To)
            for (int to = To + tg; p.out_off[b] + to < p.out_end[b]; to += 8) *reinterpret_cast<uint32_t*>(ob + (size_t)to * ld + c) = 0u;
    }
}

// state <- the last k - 1 rows of [state | chunk].  One thread owns a 16-byte column chunk and walks the rows upwards: a short chunk's shift reads row s + n
// before any row above s is written
__global__ __launch_bounds__(64) void stream_dwconv_state_kernel(const StreamDwParams p) {
    const int b = blockIdx.x, n = p.rows[b], K1 = p.ksize - 1, ld = p.ld;
    if (n <= 0) return;
    const bf16_t* gb = p.g + (size_t)p.in_off[b] * ld;
    bf16_t* sb = p.state + (size_t)(p.slot ? p.slot[b] : b) * K1 * ld;
    for (int cq = threadIdx.x * 8; cq < ld; cq += 64 * 8)
        for (int s = 0; s < K1; ++s) {
            const int t = s - (K1 - n);                                     // row of the chunk that lands in state row s (n >= K1: n - K1 + s)
            const uint4 v = t >= 0 ? *reinterpret_cast<const uint4*>(gb + (size_t)t * ld + cq) : *reinterpret_cast<const uint4*>(sb + (size_t)(s + n) * ld + cq);
            *reinterpret_cast<uint4*>(sb + (size_t)s * ld + cq) = v;
        }
}

template <int KSZ, int STRIDE>
int launch_sd(const StreamDwParams& p, hipStream_t s) {
    const int ctiles = ec_cdiv(p.C, SD_CC), ttiles = ec_cdiv(ec_cdiv(p.max_rows, STRIDE), SD_TT);
    constexpr int ROWS = (SD_TT - 1) * STRIDE + KSZ;
    hipLaunchKernelGGL((stream_dwconv_kernel<KSZ, STRIDE>), dim3(ctiles * ttiles, p.B), dim3(256), (size_t)ROWS * SD_PITCH, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

bool sd_args_ok(const StreamDwParams& p) { return p.ld % 8 == 0 && p.ld >= p.C && p.C > 0 && p.B > 0; }

}  // namespace

bool stream_attention_supported(int dpad) { return dpad >= 32 && dpad <= 192 && dpad % 32 == 0; }

int launch_stream_attention(const StreamAttnParams& p, hipStream_t s) {
    if (p.B <= 0 || p.max_rows <= 0) return 0;
    if (p.D % 2 || p.dvu_ld < p.dpad || p.dvu_ld % 4 || p.H * p.d != p.G * p.D || p.n_dist <= 0 || p.cap < 0) return -2;
    switch (p.dpad) {
        case 32: return launch_sa<32>(p, s);
        case 64: return launch_sa<64>(p, s);
        case 96: return launch_sa<96>(p, s);
        case 128: return launch_sa<128>(p, s);
        case 160: return launch_sa<160>(p, s);
        case 192: return launch_sa<192>(p, s);
    }
    return -3;
}

int launch_stream_kv_append(const StreamAttnParams& p, hipStream_t s) {
    if (p.B <= 0 || p.max_rows <= 0 || p.cap <= 0) return 0;
    if (p.D % 2) return -2;
    const int ng = ec_cdiv(p.max_rows, p.G);
    hipLaunchKernelGGL(stream_kv_append_kernel, dim3(std::min(std::min(ng, p.cap), 64), p.B), dim3(256), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_stream_dwconv(const StreamDwParams& p, hipStream_t s) {
    if (p.B <= 0 || p.max_rows <= 0) return 0;
    if (!sd_args_ok(p)) return -2;
    if (p.ksize == 15 && p.stride == 1) return launch_sd<15, 1>(p, s);
    if (p.ksize == 15 && p.stride == 2) return launch_sd<15, 2>(p, s);
    if (p.ksize == 31 && p.stride == 1) return launch_sd<31, 1>(p, s);
    if (p.ksize == 31 && p.stride == 2) return launch_sd<31, 2>(p, s);
    if (p.ksize == 7 && p.stride == 1) return launch_sd<7, 1>(p, s);
    if (p.ksize == 7 && p.stride == 2) return launch_sd<7, 2>(p, s);
    return -3;
}

int launch_stream_dwconv_state(const StreamDwParams& p, hipStream_t s) {
    if (p.B <= 0 || p.max_rows <= 0) return 0;
    if (!sd_args_ok(p) || p.ksize < 2) return -2;
    hipLaunchKernelGGL(stream_dwconv_state_kernel, dim3(p.B), dim3(64), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// =================================================================== C ABI: the two kernels alone on caller-provided operands and state
extern "C" {

int effconf_stream_attention(const uint16_t* qu, const uint16_t* k, const uint16_t* v, const uint16_t* e, int32_t e_rows, const float* dvu, int32_t dvu_ld,
                             uint16_t* k_cache, uint16_t* v_cache, int32_t capacity, const int32_t* row_off, const int32_t* rows, const int32_t* cached,
                             const int32_t* pos, int32_t streams, int32_t max_rows, int32_t heads, int32_t group, int32_t dim, int32_t band_left,
                             uint16_t* out, int32_t ld_out, int32_t append, void* stream) {
    if (!qu || !k || !v || !e || !dvu || !row_off || !rows || !cached || !pos || !out) return fail("null argument");
    if (streams <= 0 || max_rows < 0 || heads <= 0 || group <= 0 || !(group & 1) || dim <= 0 || dim % 2 || (group * dim) % heads || e_rows <= 0 || band_left < 0)
        return fail("bad stream attention shape");
    if (capacity < 0 || (capacity > 0 && (!k_cache || !v_cache))) return fail("stream attention: a cache of capacity > 0 needs both rings");
    StreamAttnParams p{};
    p.d = group * dim / heads; p.dpad = ec_round_up(p.d, 32);
    if (!stream_attention_supported(p.dpad) || dvu_ld < p.dpad || dvu_ld % 4 || ld_out < dim) return fail("unsupported head width / leading dimension");
    p.qu = qu; p.k = k; p.v = v; p.e = e; p.n_dist = e_rows; p.dvu = dvu; p.dvu_ld = dvu_ld;
    p.kc = k_cache; p.vc = v_cache; p.cap = capacity;
    p.row_off = row_off; p.rows = rows; p.cached = cached; p.pos = pos;
    p.B = streams; p.H = heads; p.G = group; p.D = dim; p.max_rows = max_rows; p.band_l = band_left;
    p.out = out; p.ldo = ld_out; p.scale = 1.0f / std::sqrt((float)p.d);
    EC_TRY(launch_stream_attention(p, (hipStream_t)stream));
    if (append) EC_TRY(launch_stream_kv_append(p, (hipStream_t)stream));
    return 0;
}

int effconf_stream_dwconv(const uint16_t* g, int32_t ld, int32_t channels, const float* taps, const float* bias, int32_t ksize, int32_t stride,
                          uint16_t* state, const int32_t* in_off, const int32_t* rows, const int32_t* hist, const int32_t* out_off, int32_t streams,
                          int32_t max_rows, uint16_t* out, int32_t update_state, void* stream) {
    if (!g || !taps || !bias || !state || !in_off || !rows || !hist || !out_off || !out) return fail("null argument");
    if (streams <= 0 || max_rows < 0 || channels <= 0 || ld % 8 || ld < channels) return fail("bad stream depthwise shape");
    if ((ksize != 7 && ksize != 15 && ksize != 31) || (stride != 1 && stride != 2)) return fail("stream depthwise: kernel size 7 / 15 / 31 and stride 1 / 2 only");
    StreamDwParams p{};
    p.g = g; p.ld = ld; p.C = channels; p.w_kc = taps; p.bias = bias; p.ksize = ksize; p.stride = stride; p.state = state;
    p.in_off = in_off; p.rows = rows; p.hist = hist; p.out_off = out_off; p.B = streams; p.max_rows = max_rows; p.out = out;
    EC_TRY(launch_stream_dwconv(p, (hipStream_t)stream));
    if (update_state) EC_TRY(launch_stream_dwconv_state(p, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
