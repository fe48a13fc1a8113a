// LSTM language model (gfx950): the reference's LanguageModel (models/lm.py: RnnDecoder = Embedding + L-layer LSTM, then fc) as a scorer of
// token sequences - n-best rescoring of the CTC beam search (ModelCTC.rescore_nbest) - and as its one-token decode(x, hidden) step.
//   x = [0, y_0 .. y_{U-1}];  h_u = the top layer's output after x_0 .. x_u from zero state;  lp_u = log_softmax(fc(h_u) / tmp)
//   token_logp[u] = lp_u[y_u] (u < U);  score = sum_u token_logp[u], fp32, u ascending;  U = 0: score 0
// Step-major schedule on the caller's stream: for u = 0 .. u_max - 1, one lm_lstm_step_kernel launch per layer, then one lm_head_kernel
// launch.  Memory: the (h, c) state of the N sequences and the outputs; no (N, U, 4H) or (N, U, V) tensor exists.  No kernel synchronises
// workgroups: a step's launches are ordered by the stream, every loop bound is an argument.
//   * lm_lstm_step_kernel<CT>: a GEMM with the LSTM cell as its epilogue, fp32 operands on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32).  A wave
//     owns 16 hidden units = the four gate row tiles {j0, H + j0, 2H + j0, 3H + j0} (torch gate order i, f, g, o) and CT 16-sequence column
//     tiles: one weight float4 per gate feeds 4 CT MFMAs.  Grid: (hidden tiles / 4 waves) x (column tiles / CT), so a step covers the chip
//     where one workgroup per 16 sequences (rnnt_lattice.hip's prediction network) would leave it idle.  The state lives in global memory
//     with k permuted as the weight images (kperm, rnnt_common.h): a lane's B operand of a 16-block is ONE 16-byte load, and no LDS is used (16
//     state vectors at H = 4096 are 256 KiB).  Layer 0: K = H against W_hh, the input term from the table Gin0[y] = W_ih0 emb[y] + b_ih0 + b_hh0
//     (built at finalize as effconf_rnnt_finalize builds gin).  Layers l >= 1: K = 2H against the image of [W_ih_l | W_hh_l]: first the layer
//     below's h of THIS step, then this layer's h of the previous step; k ascends within each part.  h is double buffered between steps; a
//     sequence with u >= len keeps (h, c) through a select, and a wave whose column tiles hold finished sequences only returns at once
//     (wave-uniform; nothing reads such a state again; LanguageModel sorts the sequences by length, so such tiles exist).
//   * lm_head_kernel<FULL>: fc as a GEMM over the vocabulary tiles of 32 sequences per workgroup (rnnt_joint_kernel's loop).  FULL = false: the
//     lane's running (max, sum exp) of (acc + b) / tmp and the pick of column y_u, merged in a fixed order (k-slots of a wave, then waves 0 .. 7);
//     ONE float per (sequence, position) leaves the kernel, and score[n] += it (a launch per position: u ascending).  FULL = true (the decode
//     step): the raw logits row acc + b.  V % 16 != 0: rows clamped on load, masked with -inf.
// A column of an MFMA tile depends on that column of B alone and unused columns are zero: a sequence's results are bit-identical alone, in any
// batch, in any order, under a larger u_max, with garbage behind its length and on a workspace filled with any byte (the state is cleared by a
// memset on the stream, nothing else is read before it is written).
#include "rnnt_common.h"

#include <algorithm>
#include <cmath>

int ec_fail(const char* msg);

using namespace ecrnnt;

struct EcLm {
    EcLmConfig cfg;
    std::map<std::string, EcRnntHostT> host;
    std::vector<void*> allocs;
    const float* gin0 = nullptr;          // [V][4H]
    const float4* w16[4] = {};            // layer 0: kperm16(W_hh0) [H/16][4][4H]; l >= 1: kperm16([W_ih_l | W_hh_l]) [2H/16][4][4H]
    const float* bsum[4] = {};            // l >= 1: b_ih_l + b_hh_l [4H]
    const float4* wfc16 = nullptr;        // kperm16(fc.weight) [H/16][4][V]
    const float* bfc = nullptr;           // [V]
    bool finalized = false;
};

namespace {

constexpr int ST = 256;          // threads of a step workgroup: 4 waves = 4 hidden tiles
constexpr int SW = ST / 64;
constexpr int HT = 512;          // threads of a head workgroup
constexpr int HW = HT / 64;
constexpr int HC = 32;           // sequences per head workgroup: two column tiles
constexpr int NPADQ = 64;        // the state holds the sequences rounded up to this many columns: every column tile a kernel touches exists
constexpr int MAX_H = 4096, MAX_L = 4, MAX_U = 4096;
constexpr int MAX_N = 1 << 21;   // the step grid's y extent is Np / 64 at most: 32768 < 65536

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
int npad(int n) { return (n + NPADQ - 1) / NPADQ * NPADQ; }

const char* cfg_check(const EcLmConfig& c) {
    if (c.dim_model % 16 != 0) return "lm: dim_model must be a multiple of 16";
    if (c.dim_model < 16 || c.dim_model > MAX_H) return "lm: dim_model must be in 16 .. 4096";
    if (c.num_layers < 1 || c.num_layers > MAX_L) return "lm: num_layers must be in 1 .. 4";
    if (c.vocab_size < 2) return "lm: vocab_size must be at least 2";
    return nullptr;
}

const char* shape_check(const EcLm* lm, int32_t n, int32_t u_max) {
    if (!lm) return "null handle";
    if (n < 0) return "lm: bad batch";
    if (n > MAX_N) return "lm: at most 2^21 sequences per call";
    if (u_max < 0 || u_max > MAX_U) return "lm: u_max must be in 0 .. 4096";
    if ((int64_t)n * u_max >= (1ll << 31)) return "lm: n * u_max must be below 2^31";
    return nullptr;
}

// workspace (the pointer aligned up to 256 bytes): i32 ulen[n]; then per layer l: h[l][2][Np][H] (k-permuted), c[l][Np][H]
struct LmLayout { size_t ulen, state, layer, total; };

LmLayout lm_layout(const EcLmConfig& c, int n) {
    LmLayout L{};
    L.ulen = 0;
    L.state = al256((size_t)n * 4);
    L.layer = (size_t)3 * npad(n) * c.dim_model * 4;
    L.total = L.state + (size_t)c.num_layers * L.layer + 256;
    return L;
}

struct StepArgs {
    const float4* w16;       // the layer's weight image
    const float* xa;         // layers >= 1: the layer below's h of this step [Np][H] k-permuted; layer 0: null
    const float* hp;         // this layer's h of the previous step
    float* hn;               // this layer's h of this step
    float* c;                // [Np][H], natural order, updated in place
    const float* gin;        // layer 0: Gin0 [V][4H]; else null
    const float* bias;       // layers >= 1: b_ih + b_hh [4H]
    const int* tok;          // layer 0: the token of sequence n is tok[n * tok_stride + tok_off], 0 when tok_off < 0
    const int* ulen;         // null: every sequence advances; else sequence n advances iff u < ulen[n]
    long long tok_stride; int tok_off;
    int u, N, H, V;
};

// acc[gate][c] += W[gate rows][16 K16 k's] x[k][16 columns of tile c], k ascending; wp: the lane's entry of gate 0 in 16-block 0
template <int CT>
__device__ __forceinline__ void lm_accum(const float4* __restrict__ wp, int H, size_t bs, int K16, const float* const (&xl)[CT], f32x4 (&acc)[4][CT]) {
    float4 wn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) wn[i] = wp[i * H];
    for (int q = 0; q < K16; ++q) {
        float4 wv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) wv[i] = wn[i];
        const int qn = q + 1 < K16 ? q + 1 : q;                      // last pass: a harmless re-load
#pragma unroll
        for (int i = 0; i < 4; ++i) wn[i] = wp[(size_t)qn * bs + i * H];
        float4 x[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) x[c] = *reinterpret_cast<const float4*>(xl[c] + 16 * q);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i].x, x[c].x, acc[i][c], 0, 0, 0);
                acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i].y, x[c].y, acc[i][c], 0, 0, 0);
                acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i].z, x[c].z, acc[i][c], 0, 0, 0);
                acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i].w, x[c].w, acc[i][c], 0, 0, 0);
            }
    }
}

template <int CT>
__global__ __launch_bounds__(ST) void lm_lstm_step_kernel(const StepArgs a) {
    const int H = a.H, K16 = H / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
    const int ub = blockIdx.x * SW + wave;           // hidden tile of the wave
    if (ub >= K16) return;                           // the whole wave; the kernel has no barrier
    const int col0 = blockIdx.y * CT * 16;           // first sequence of the workgroup's column tiles (< Np: the grid covers Np / 16 tiles exactly)
    const int unit0 = 16 * ub + 4 * g;               // rows 4 g + e of the tiles = hidden units unit0 + e, column j = sequence
    bool mine = false;                               // does one of this lane's sequences advance?
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int n = col0 + 16 * c + j;
        mine = mine || (n < a.N && (!a.ulen || a.u < a.ulen[n]));
    }
    // wave-uniform: every sequence of the wave's column tiles is finished (or padding).  Lengths are fixed, so these columns never advance again,
    // the head picks nothing from them and the layer above (same columns, same test) returns here as well: their state is never read again
    // and need not follow the buffer swap.  Steps at or beyond the longest sequence of a call are launches of such waves only.
    if (!__any(mine)) return;
    const size_t bs = (size_t)4 * 4 * H;             // float4s per 16-block of the image: [g][4H]
    const float4* wp = a.w16 + (size_t)g * 4 * H + 16 * ub + j;
    f32x4 acc[4][CT];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* xl[CT];
    if (a.xa) {
#pragma unroll
        for (int c = 0; c < CT; ++c) xl[c] = a.xa + (size_t)(col0 + 16 * c + j) * H + 4 * g;
        lm_accum<CT>(wp, H, bs, K16, xl, acc);
        wp += (size_t)K16 * bs;
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) xl[c] = a.hp + (size_t)(col0 + 16 * c + j) * H + 4 * g;
    lm_accum<CT>(wp, H, bs, K16, xl, acc);
    // ---- the cell
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int n = col0 + 16 * c + j;
        const bool live = n < a.N;
        const bool adv = live && (!a.ulen || a.u < a.ulen[n]);
        const float* add = a.bias;
        if (a.gin) {
            int y = 0;
            if (live && a.tok_off >= 0) y = a.tok[(long long)n * a.tok_stride + a.tok_off];
            y = y < 0 ? 0 : (y >= a.V ? a.V - 1 : y);                // an id outside the table is never scored (status 2): keep the load in bounds
            add = a.gin + (size_t)y * 4 * H;
        }
        float* cr = a.c + (size_t)n * H + unit0;
        const float4 cold4 = *reinterpret_cast<const float4*>(cr);
        const float4 ai = *reinterpret_cast<const float4*>(add + unit0), af = *reinterpret_cast<const float4*>(add + H + unit0);
        const float4 ag = *reinterpret_cast<const float4*>(add + 2 * H + unit0), ao = *reinterpret_cast<const float4*>(add + 3 * H + unit0);
        const float cold[4] = {cold4.x, cold4.y, cold4.z, cold4.w};
        const float bi[4] = {ai.x, ai.y, ai.z, ai.w}, bf[4] = {af.x, af.y, af.z, af.w}, bg[4] = {ag.x, ag.y, ag.z, ag.w}, bo[4] = {ao.x, ao.y, ao.z, ao.w};
        float cn[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ig = sigmoid_precise(acc[0][c][e] + bi[e]), fg = sigmoid_precise(acc[1][c][e] + bf[e]);
            const float gg = tanhf(acc[2][c][e] + bg[e]), og = sigmoid_precise(acc[3][c][e] + bo[e]);
            const float cv = fg * cold[e] + ig * gg;
            const float hv = og * tanhf(cv);
            const size_t hi = (size_t)n * H + kperm(unit0 + e);
            a.hn[hi] = adv ? hv : a.hp[hi];          // (n, unit) belongs to this lane alone
            cn[e] = adv ? cv : cold[e];
        }
        *reinterpret_cast<float4*>(cr) = make_float4(cn[0], cn[1], cn[2], cn[3]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- lengths, status
struct PrepArgs {
    const int* tokens; const long long* len; int N, umax, V;
    int* ulen; int* status; float* score;
};

__global__ __launch_bounds__(256) void lm_prep_kernel(const PrepArgs a) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= a.N) return;
    const long long ul = a.len[n];
    int st = 0, U = 0;
    if (ul < 0 || ul > a.umax) st = 2;
    else {
        U = (int)ul;
        for (int u = 0; u < U; ++u) {
            const int c = a.tokens[(size_t)n * a.umax + u];
            if (c < 1 || c >= a.V) st = 2;
        }
    }
    a.status[n] = st;
    a.ulen[n] = st ? -1 : U;                         // -1: the sequence never advances and every token_logp of its row is -inf
    a.score[n] = st ? -INFINITY : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- fc head
struct HeadArgs {
    const float4* wfc16; const float* bfc;
    const float* h;          // the top layer's h of this step [Np][H], k-permuted
    const int* tokens; const int* ulen;
    float* token_logp;       // [N][umax] or null
    float* score;            // [N]
    float* logits;           // FULL: [N][V]
    int u, umax, N, H, V; float tmp;
};

// running (max, sum exp) of a sequence's logits: merge of two partial results; an empty part is (-inf, 0)
__device__ __forceinline__ void ms_merge(float& m, float& s, float om, float os) {
    const float nm = fmaxf(m, om);
    const float ea = m == -INFINITY ? 0.f : expf(m - nm), eb = om == -INFINITY ? 0.f : expf(om - nm);
    s = s * ea + os * eb;
    m = nm;
}

template <bool FULL>
__global__ __launch_bounds__(HT) void lm_head_kernel(const HeadArgs a) {
    __shared__ int s_y[HC];
    __shared__ float s_m[HW][HC], s_s[HW][HC], s_label[HC];
    const int H = a.H, V = a.V, K16 = H / 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
    const int c0 = blockIdx.x * HC;                  // < Np
    if (!FULL) {
        if (tid < HC) {
            const int n = c0 + tid;
            int y = -1;                              // -1: nothing to pick (beyond the batch, beyond the sequence, a refused sequence)
            if (n < a.N && a.u < a.ulen[n]) y = a.tokens[(size_t)n * a.umax + a.u];
            s_y[tid] = y;
            s_label[tid] = -INFINITY;
        }
        __syncthreads();
    }
    if (!FULL) {
        bool none = true;                            // workgroup-uniform: nothing to score in these 32 columns at this position
        for (int i = 0; i < HC; ++i) none = none && s_y[i] < 0;
        if (none) {
            if (tid < HC && c0 + tid < a.N && a.token_logp) a.token_logp[(size_t)(c0 + tid) * a.umax + a.u] = a.ulen[c0 + tid] < 0 ? -INFINITY : 0.f;
            return;
        }
    }
    const int ntile = (V + 15) / 16;
    const size_t bs = (size_t)4 * V;                 // float4s per 16-block of the weight image: [g][n]
    const float* x0 = a.h + (size_t)(c0 + j) * H + 4 * g;
    const float* x1 = a.h + (size_t)(c0 + 16 + j) * H + 4 * g;
    const int y0 = FULL ? -1 : s_y[j], y1 = FULL ? -1 : s_y[16 + j];
    float m0 = -INFINITY, m1 = -INFINITY, r0 = 0.f, r1 = 0.f;     // the lane's running (max, sum) of sequences j and 16 + j
    for (int tp = wave; 2 * tp < ntile; tp += HW) {
        const float4* wp[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int n = 16 * (2 * tp + i) + j;
            wp[i] = a.wfc16 + (size_t)g * V + (n < V ? n : V - 1);     // clamped: rows at or beyond V are masked below
        }
        f32x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
        float4 wn[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) wn[i] = wp[i][0];
        for (int q = 0; q < K16; ++q) {
            float4 wv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) wv[i] = wn[i];
            const int qn = q + 1 < K16 ? q + 1 : q;                  // last pass: a harmless re-load
#pragma unroll
            for (int i = 0; i < 2; ++i) wn[i] = wp[i][(size_t)qn * bs];
            const float4 xa = *reinterpret_cast<const float4*>(x0 + 16 * q);
            const float4 xb = *reinterpret_cast<const float4*>(x1 + 16 * q);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i].x, xa.x, acc[i][0], 0, 0, 0);
                acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i].x, xb.x, acc[i][1], 0, 0, 0);
                acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i].y, xa.y, acc[i][0], 0, 0, 0);
                acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i].y, xb.y, acc[i][1], 0, 0, 0);
                acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i].z, xa.z, acc[i][0], 0, 0, 0);
                acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i].z, xb.z, acc[i][1], 0, 0, 0);
                acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i].w, xa.w, acc[i][0], 0, 0, 0);
                acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i].w, xb.w, acc[i][1], 0, 0, 0);
            }
        }
        // ---- epilogue of the pair: row 4 g + e of tile i = vocabulary entry n, column j = sequence
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int nb = 16 * (2 * tp + i) + 4 * g;
            if (FULL) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int n = nb + e;
                    if (n < V) {
                        const float bias = a.bfc[n];
                        if (c0 + j < a.N) a.logits[(size_t)(c0 + j) * V + n] = acc[i][0][e] + bias;
                        if (c0 + 16 + j < a.N) a.logits[(size_t)(c0 + 16 + j) * V + n] = acc[i][1][e] + bias;
                    }
                }
            } else {
                float v0[4], v1[4];
                float t0 = -INFINITY, t1 = -INFINITY;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int n = nb + e;
                    const float bias = a.bfc[n < V ? n : V - 1];
                    v0[e] = n < V ? (acc[i][0][e] + bias) / a.tmp : -INFINITY;
                    v1[e] = n < V ? (acc[i][1][e] + bias) / a.tmp : -INFINITY;
                    t0 = fmaxf(t0, v0[e]); t1 = fmaxf(t1, v1[e]);
                    if (n == y0) s_label[j] = v0[e];
                    if (n == y1) s_label[16 + j] = v1[e];
                }
                if (nb < V) {                        // at least one entry: nb itself
                    float p0 = 0.f, p1 = 0.f;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { p0 += expf(v0[e] - t0); p1 += expf(v1[e] - t1); }     // exp(-inf) = 0 for the masked entries
                    ms_merge(m0, r0, t0, p0);
                    ms_merge(m1, r1, t1, p1);
                }
            }
        }
    }
    if (FULL) return;
    // ---- merge the k-slots of the wave (g = 0 + 1, 2 + 3, then the two halves), then the waves in order
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const float om0 = __shfl_xor(m0, o), os0 = __shfl_xor(r0, o), om1 = __shfl_xor(m1, o), os1 = __shfl_xor(r1, o);
        if (!(lane & o)) { ms_merge(m0, r0, om0, os0); ms_merge(m1, r1, om1, os1); }
    }
    if (g == 0) { s_m[wave][j] = m0; s_s[wave][j] = r0; s_m[wave][16 + j] = m1; s_s[wave][16 + j] = r1; }
    __syncthreads();
    if (tid < HC && c0 + tid < a.N) {
        const int n = c0 + tid;
        float out = a.ulen[n] < 0 ? -INFINITY : 0.f;                 // a refused sequence: -inf; at or beyond the length: 0
        if (s_y[tid] >= 0) {
            float m = s_m[0][tid], s = s_s[0][tid];
#pragma unroll
            for (int q = 1; q < HW; ++q) ms_merge(m, s, s_m[q][tid], s_s[q][tid]);
            out = s_label[tid] - (m + logf(s));
            a.score[n] += out;                       // one launch per position on one stream: u ascending
        }
        if (a.token_logp) a.token_logp[(size_t)n * a.umax + a.u] = out;
    }
}

// ---------------------------------------------------------------------------------------------------------------- decode-step state in / out
// natural (L, N, H) <-> the workspace's k-permuted h / natural c with Np columns; src null = zeros
__global__ __launch_bounds__(256) void lm_state_in_kernel(const float* h_in, const float* c_in, float* state, size_t layer_floats, int L, int N, int Np, int H) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)L * Np * H) return;
    const int k = (int)(i % H), n = (int)((i / H) % Np), l = (int)(i / ((size_t)H * Np));
    const bool live = n < N;
    const size_t src = ((size_t)l * N + n) * H + k;
    float* base = state + (size_t)l * layer_floats;
    base[(size_t)n * H + kperm(k)] = live && h_in ? h_in[src] : 0.f;
    base[(size_t)2 * Np * H + (size_t)n * H + k] = live && c_in ? c_in[src] : 0.f;
}

__global__ __launch_bounds__(256) void lm_state_out_kernel(const float* state, size_t layer_floats, float* h_out, float* c_out, int L, int N, int Np, int H) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)L * N * H) return;
    const int k = (int)(i % H), n = (int)((i / H) % N), l = (int)(i / ((size_t)H * N));
    const float* base = state + (size_t)l * layer_floats;
    if (h_out) h_out[i] = base[(size_t)Np * H + (size_t)n * H + kperm(k)];       // buffer 1: the step's output
    if (c_out) c_out[i] = base[(size_t)2 * Np * H + (size_t)n * H + k];
}

void* upload(EcLm* lm, const void* src, size_t bytes) {
    void* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) return nullptr;
    lm->allocs.push_back(d);
    if (src && hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}

const EcRnntHostT* need(EcLm* lm, const std::string& key, std::initializer_list<int64_t> shape, std::string& err) {
    auto it = lm->host.find(key);
    if (it == lm->host.end()) { if (err.empty()) err = "missing tensor " + key; return nullptr; }
    if (it->second.shape != std::vector<int64_t>(shape)) { if (err.empty()) err = "bad shape for " + key; return nullptr; }
    return &it->second;
}

// one LSTM step of layer l on buffers cur -> 1 - cur of the state
int launch_step(const EcLm* lm, float* state, size_t layer_floats, int l, int cur, int N, const int* tok, long long tok_stride, int tok_off, const int* ulen, int u,
                hipStream_t s) {
    const int H = lm->cfg.dim_model, Np = npad(N);
    const size_t buf = (size_t)Np * H;
    float* base = state + (size_t)l * layer_floats;
    StepArgs a{};
    a.w16 = lm->w16[l];
    a.xa = l ? state + (size_t)(l - 1) * layer_floats + (size_t)(1 - cur) * buf : nullptr;
    a.hp = base + (size_t)cur * buf;
    a.hn = base + (size_t)(1 - cur) * buf;
    a.c = base + 2 * buf;
    a.gin = l ? nullptr : lm->gin0;
    a.bias = l ? lm->bsum[l] : nullptr;
    a.tok = tok; a.tok_stride = tok_stride; a.tok_off = tok_off; a.ulen = ulen;
    a.u = u; a.N = N; a.H = H; a.V = lm->cfg.vocab_size;
    const int tiles = Np / 16, hb = (H / 16 + SW - 1) / SW;
    // column tiles per weight float4: 4 where the batch has them (rows per streamed weight byte decide the kernel at large N)
    if (N > 32) hipLaunchKernelGGL(lm_lstm_step_kernel<4>, dim3(hb, tiles / 4), dim3(ST), 0, s, a);
    else if (N > 16) hipLaunchKernelGGL(lm_lstm_step_kernel<2>, dim3(hb, tiles / 2), dim3(ST), 0, s, a);
    else hipLaunchKernelGGL(lm_lstm_step_kernel<1>, dim3(hb, tiles), dim3(ST), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace

extern "C" {

EcLm* effconf_lm_create(const EcLmConfig* c) {
    if (!c) { ec_fail("null config"); return nullptr; }
    if (const char* e = cfg_check(*c)) { ec_fail(e); return nullptr; }
    EcLm* lm = new EcLm();
    lm->cfg = *c;
    return lm;
}

void effconf_lm_destroy(EcLm* lm) {
    if (!lm) return;
    for (void* p : lm->allocs) (void)hipFree(p);
    delete lm;
}

int effconf_lm_load_tensor(EcLm* lm, const char* key, const float* host, const int64_t* shape, int32_t ndim) {
    if (!lm || !key || !host || (ndim > 0 && !shape)) return ec_fail("null argument");
    EcRnntHostT t;
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= shape[i]; }
    t.data.assign(host, host + n);
    lm->host[key] = std::move(t);
    lm->finalized = false;
    return 0;
}

int effconf_lm_finalize(EcLm* lm) {
    if (!lm) return ec_fail("null handle");
    const int H = lm->cfg.dim_model, V = lm->cfg.vocab_size, L = lm->cfg.num_layers;
    // every tensor is looked up before the first device call: a missing key is reported without a GPU
    std::string err;
    const EcRnntHostT* emb = need(lm, "decoder.embedding.weight", {V, H}, err);
    const EcRnntHostT* wfc = need(lm, "fc.weight", {V, H}, err);
    const EcRnntHostT* bfc = need(lm, "fc.bias", {V}, err);
    const EcRnntHostT *wih[MAX_L], *whh[MAX_L], *bih[MAX_L], *bhh[MAX_L];
    for (int l = 0; l < L; ++l) {
        const std::string p = "decoder.rnn.", sfx = "_l" + std::to_string(l);
        wih[l] = need(lm, p + "weight_ih" + sfx, {4 * H, H}, err);
        whh[l] = need(lm, p + "weight_hh" + sfx, {4 * H, H}, err);
        bih[l] = need(lm, p + "bias_ih" + sfx, {4 * H}, err);
        bhh[l] = need(lm, p + "bias_hh" + sfx, {4 * H}, err);
    }
    if (!err.empty()) return ec_fail(err.c_str());
    for (void* p : lm->allocs) (void)hipFree(p);
    lm->allocs.clear();
    lm->finalized = false;
    bool ok = true;
    for (int l = 0; l < L; ++l) {
        std::vector<float> bs(4 * H);
        for (int i = 0; i < 4 * H; ++i) bs[i] = bih[l]->data[i] + bhh[l]->data[i];
        lm->bsum[l] = (const float*)upload(lm, bs.data(), bs.size() * 4);
        if (l == 0) {
            const std::vector<float> img = kperm16(whh[0]->data, 4 * H, H);
            lm->w16[0] = (const float4*)upload(lm, img.data(), img.size() * 4);
        } else {
            std::vector<float> cat((size_t)4 * H * 2 * H);           // [W_ih_l | W_hh_l]: rows of 2H
            for (int r = 0; r < 4 * H; ++r) {
                std::copy(wih[l]->data.begin() + (size_t)r * H, wih[l]->data.begin() + (size_t)(r + 1) * H, cat.begin() + (size_t)r * 2 * H);
                std::copy(whh[l]->data.begin() + (size_t)r * H, whh[l]->data.begin() + (size_t)(r + 1) * H, cat.begin() + (size_t)r * 2 * H + H);
            }
            const std::vector<float> img = kperm16(cat, 4 * H, 2 * H);
            lm->w16[l] = (const float4*)upload(lm, img.data(), img.size() * 4);
        }
        ok = ok && lm->bsum[l] && lm->w16[l];
    }
    {
        const std::vector<float> img = kperm16(wfc->data, V, H);
        lm->wfc16 = (const float4*)upload(lm, img.data(), img.size() * 4);
    }
    lm->bfc = (const float*)upload(lm, bfc->data.data(), bfc->data.size() * 4);
    float* d_emb = (float*)upload(lm, emb->data.data(), emb->data.size() * 4);
    float* d_wih = (float*)upload(lm, wih[0]->data.data(), wih[0]->data.size() * 4);
    float* d_gin = (float*)upload(lm, nullptr, (size_t)V * 4 * H * 4);
    if (!ok || !lm->wfc16 || !lm->bfc || !d_emb || !d_wih || !d_gin) return ec_fail("lm: device allocation / upload failed");
    // Gin0[y] = W_ih0 emb[y] + (b_ih0 + b_hh0) for every token id; row 0 from the embedding row the checkpoint holds
    if (launch_sgemm_nt(d_emb, H, d_wih, H, lm->bsum[0], d_gin, 4 * H, V, 4 * H, H, nullptr) != 0) return ec_fail("lm: Gin GEMM launch failed");
    if (hipDeviceSynchronize() != hipSuccess) return ec_fail("lm: Gin GEMM failed");
    for (void* p : {(void*)d_emb, (void*)d_wih}) {       // only the Gin GEMM read them
        (void)hipFree(p);
        lm->allocs.erase(std::find(lm->allocs.begin(), lm->allocs.end(), p));
    }
    lm->gin0 = d_gin;
    lm->finalized = true;
    return 0;
}

size_t effconf_lm_workspace_bytes(const EcLm* lm, int32_t n, int32_t u_max) {
    if (const char* e = shape_check(lm, n, u_max)) { ec_fail(e); return 0; }
    return lm_layout(lm->cfg, n).total;
}

int effconf_lm_score(EcLm* lm, const int32_t* tokens, const int64_t* token_len, int32_t n, int32_t u_max, float lm_tmp, float* token_logp, float* score,
                     int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (!lm || !lm->finalized) return ec_fail("lm handle not finalized");
    if (const char* e = shape_check(lm, n, u_max)) return ec_fail(e);
    if (!(lm_tmp > 0.f) || !std::isfinite(lm_tmp)) return ec_fail("lm: lm_tmp must be > 0");
    if (n == 0) return 0;
    if (!token_len || !score || !status || !workspace || (u_max > 0 && !tokens)) return ec_fail("null argument");
    const LmLayout L = lm_layout(lm->cfg, n);
    if (workspace_bytes < L.total) return ec_fail("workspace too small (effconf_lm_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    int* ulen = reinterpret_cast<int*>(ws + L.ulen);
    float* state = reinterpret_cast<float*>(ws + L.state);
    const int H = lm->cfg.dim_model, V = lm->cfg.vocab_size, NL = lm->cfg.num_layers, Np = npad(n);
    const size_t layer_floats = L.layer / 4;
    PrepArgs p{tokens, reinterpret_cast<const long long*>(token_len), n, u_max, V, ulen, status, score};
    hipLaunchKernelGGL(lm_prep_kernel, dim3((n + 255) / 256), dim3(256), 0, s, p);
    if (hipGetLastError() != hipSuccess) return ec_fail("lm_prep launch failed");
    if (u_max == 0) return 0;
    if (hipMemsetAsync(state, 0, (size_t)NL * L.layer, s) != hipSuccess) return ec_fail("lm: clearing the state failed");
    for (int u = 0; u < u_max; ++u) {
        const int cur = u & 1;
        for (int l = 0; l < NL; ++l)
            if (launch_step(lm, state, layer_floats, l, cur, n, tokens, u_max, u - 1, ulen, u, s) != 0) return ec_fail("lm_lstm_step launch failed");
        HeadArgs h{};
        h.wfc16 = lm->wfc16; h.bfc = lm->bfc;
        h.h = state + (size_t)(NL - 1) * layer_floats + (size_t)(1 - cur) * Np * H;
        h.tokens = tokens; h.ulen = ulen; h.token_logp = token_logp; h.score = score; h.logits = nullptr;
        h.u = u; h.umax = u_max; h.N = n; h.H = H; h.V = V; h.tmp = lm_tmp;
        hipLaunchKernelGGL(lm_head_kernel<false>, dim3(Np / HC), dim3(HT), 0, s, h);
        if (hipGetLastError() != hipSuccess) return ec_fail("lm_head launch failed");
    }
    return 0;
}

int effconf_lm_step(EcLm* lm, const int32_t* tokens, const float* h_in, const float* c_in, int32_t n, float* logits, float* h_out, float* c_out,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!lm || !lm->finalized) return ec_fail("lm handle not finalized");
    if (const char* e = shape_check(lm, n, 0)) return ec_fail(e);
    if (n == 0) return 0;
    if (!tokens || !logits || !workspace) return ec_fail("null argument");
    const LmLayout L = lm_layout(lm->cfg, n);
    if (workspace_bytes < L.total) return ec_fail("workspace too small (effconf_lm_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    float* state = reinterpret_cast<float*>(ws + L.state);
    const int H = lm->cfg.dim_model, V = lm->cfg.vocab_size, NL = lm->cfg.num_layers, Np = npad(n);
    const size_t layer_floats = L.layer / 4;
    const size_t cells = (size_t)NL * Np * H;
    hipLaunchKernelGGL(lm_state_in_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, h_in, c_in, state, layer_floats, NL, n, Np, H);
    if (hipGetLastError() != hipSuccess) return ec_fail("lm_state_in launch failed");
    for (int l = 0; l < NL; ++l)
        if (launch_step(lm, state, layer_floats, l, 0, n, tokens, 1, 0, nullptr, 0, s) != 0) return ec_fail("lm_lstm_step launch failed");
    HeadArgs h{};
    h.wfc16 = lm->wfc16; h.bfc = lm->bfc;
    h.h = state + (size_t)(NL - 1) * layer_floats + (size_t)Np * H;
    h.logits = logits; h.N = n; h.H = H; h.V = V; h.tmp = 1.f;
    hipLaunchKernelGGL(lm_head_kernel<true>, dim3(Np / HC), dim3(HT), 0, s, h);
    if (hipGetLastError() != hipSuccess) return ec_fail("lm_head launch failed");
    if (h_out || c_out) {
        const size_t outs = (size_t)NL * n * H;
        hipLaunchKernelGGL(lm_state_out_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, s, state, layer_floats, h_out, c_out, NL, n, Np, H);
        if (hipGetLastError() != hipSuccess) return ec_fail("lm_state_out launch failed");
    }
    return 0;
}

}  // extern "C"
