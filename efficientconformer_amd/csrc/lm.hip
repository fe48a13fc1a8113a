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
//     with k permuted as the weight images (kperm, decode_common.h): a lane's B operand of a 16-block is ONE 16-byte load, and no LDS is used (16
//     state vectors at H = 4096 are 256 KiB).  Layer 0: K = H against W_hh, the input term from the table Gin0[y] = W_ih0 emb[y] + b_ih0 + b_hh0
//     (built at finalize as effconf_rnnt_finalize builds gin).  Layers l >= 1: K = 2H against the image of [W_ih_l | W_hh_l]: first the layer
//     below's h of THIS step, then this layer's h of the previous step; k ascends within each part.  h is double buffered between steps; a
//     sequence with u >= len keeps (h, c) through a select, and a wave whose column tiles hold finished sequences only returns at once
//     (wave-uniform; nothing reads such a state again; LanguageModel sorts the sequences by length, so such tiles exist).
//   * lm_head_kernel<FULL>: fc as a GEMM over the vocabulary tiles of 32 sequences per workgroup (vocab_lse_tiles, the loop rnnt_joint_kernel runs).  FULL = false: the
//     lane's running (max, sum exp) of (acc + b) / tmp and the pick of column y_u, merged in a fixed order (k-slots of a wave, then waves 0 .. 7);
//     ONE float per (sequence, position) leaves the kernel, and score[n] += it (a launch per position: u ascending).  FULL = true (the decode
//     step): the raw logits row acc + b.  V % 16 != 0: rows clamped on load, masked with -inf.
//   * ecdec::lm_columns_step (decode_common.h; not part of the C ABI): the decode step on the LM nodes of the fused RNN-T beam search (rnnt_beam.hip) - the live
//     requests of all utterances packed into the first columns of the step state, the two kernels above, the new states scattered back to the nodes.
// A column of an MFMA tile depends on that column of B alone and unused columns are zero: a sequence's results are bit-identical alone, in any
// batch, in any order, under a larger u_max, with garbage behind its length and on a workspace filled with any byte (the state is cleared by a
// memset on the stream, nothing else is read before it is written).
#include "decode_common.h"

#include <algorithm>
#include <cmath>

int ec_fail(const char* msg);

using namespace ecrnnt;
using namespace ecdec;

struct EcLm {
    EcLmConfig cfg;
    EcHostTensors host;
    DeviceAllocs allocs;
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
constexpr int MAX_H = 4096, MAX_L = 4, MAX_U = 4096;
constexpr int MAX_N = 1 << 21;   // the step grid's y extent is Np / 64 at most: 32768 < 65536


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
            const LstmState s = lstm_cell(acc[0][c][e] + bi[e], acc[1][c][e] + bf[e], acc[2][c][e] + bg[e], acc[3][c][e] + bo[e], cold[e]);
            const size_t hi = (size_t)n * H + kperm(unit0 + e);
            a.hn[hi] = adv ? s.h : a.hp[hi];         // (n, unit) belongs to this lane alone
            cn[e] = adv ? s.c : cold[e];
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
    const int st = transcript_status(a.len[n], a.umax, a.tokens + (size_t)n * a.umax, a.V);
    a.status[n] = st;
    a.ulen[n] = st ? -1 : (int)a.len[n];             // -1: the sequence never advances and every token_logp of its row is -inf
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

// vocab_lse_tiles' picks for the lane's two sequences j and 16 + j: the label entry of each (scoring), or the whole row (the decode step; null: beyond the batch)
struct LmLabelPick {
    float* label; int y0, y1;                        // this lane's slot of s_label (the second sequence's is 16 further)
    __device__ __forceinline__ void operator()(int n, float v0, float v1) const {
        if (n == y0) label[0] = v0;
        if (n == y1) label[16] = v1;
    }
};
struct LmLogitsPick {
    float* row0; float* row1;
    __device__ __forceinline__ void operator()(int n, float v0, float v1) const {
        if (row0) row0[n] = v0;
        if (row1) row1[n] = v1;
    }
};

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
    const float* x0 = a.h + (size_t)(c0 + j) * H + 4 * g;
    const float* x1 = a.h + (size_t)(c0 + 16 + j) * H + 4 * g;
    float ms[4];                                     // the lane's running (max, sum) of sequences j and 16 + j
    if (FULL) {                                      // the raw logits row acc + b: tmp = 1 (x / 1 = x), the running sums are dead code
        if (a.ulen) {                                // the column step of the fused beam search: workgroup-uniform, no live column among these 32
            bool any = false;
            for (int i = 0; i < HC; ++i) any = any || (c0 + i < a.N && a.ulen[c0 + i] > 0);
            if (!any) return;
        }
        float* row0 = c0 + j < a.N ? a.logits + (size_t)(c0 + j) * V : nullptr;
        float* row1 = c0 + 16 + j < a.N ? a.logits + (size_t)(c0 + 16 + j) * V : nullptr;
        vocab_lse_tiles<1, HW>(a.wfc16, a.bfc, V, K16, x0, x1, 1.f, LmLogitsPick{row0, row1}, ms);
        return;
    }
    vocab_lse_tiles<1, HW>(a.wfc16, a.bfc, V, K16, x0, x1, a.tmp, LmLabelPick{s_label + j, s_y[j], s_y[16 + j]}, ms);
    const float lse = vocab_lse_merge<HW>(ms, s_m, s_s);
    if (tid < HC && c0 + tid < a.N) {
        const int n = c0 + tid;
        float out = a.ulen[n] < 0 ? -INFINITY : 0.f;                 // a refused sequence: -inf; at or beyond the length: 0
        if (s_y[tid] >= 0) {
            out = s_label[tid] - lse;
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

// one LSTM step of layer l on buffers cur -> 1 - cur of the state
int launch_step(const EcLm* lm, float* state, size_t layer_floats, int l, int cur, int N, const int* tok, long long tok_stride, int tok_off, const int* ulen, int u,
                hipStream_t s) {
    const int H = lm->cfg.dim_model, Np = lm_npad(N);
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

// ---------------------------------------------------------------------------------------------------------------- the fused beam search's column step
// The live requests are packed into the first columns of the step state, in request order: an evaluation batch seldom fills its 16 columns, and a column tile
// without a live column costs nothing.  LM nodes ([layer][h k-permuted | c], then the node's row) <-> the packed state.  Columns at or beyond the live count keep
// whatever the state holds: a column of an MFMA tile depends on that column alone, and nothing reads its results.
__device__ __forceinline__ float* lm_node(const LmColumns& a, int n, int node) {
    return reinterpret_cast<float*>(a.utt + (size_t)(n / a.cols_per_utt) * a.per_utt + a.lmnodes) + (size_t)node * a.node_floats;
}

// slot[n] = the packed column of request n (-1: not live), slot[ncol + d] = the token of packed column d, ulen[d] = d < live count.  One workgroup: thread t owns
// the requests t * per .. t * per + per - 1, an inclusive scan over the threads' counts orders them.
constexpr int IT = 1024;
__global__ __launch_bounds__(IT) void lm_columns_index_kernel(const LmColumns a, int* ulen) {
    __shared__ int s_cnt[IT];
    const int tid = threadIdx.x, per = (a.ncol + IT - 1) / IT, lo = tid * per, hi = lo + per < a.ncol ? lo + per : a.ncol;
    int cnt = 0;
    for (int n = lo; n < hi; ++n) cnt += a.req[n].w != 0;
    s_cnt[tid] = cnt;
    __syncthreads();
    for (int o = 1; o < IT; o <<= 1) {
        const int v = tid >= o ? s_cnt[tid - o] : 0;
        __syncthreads();
        s_cnt[tid] += v;
        __syncthreads();
    }
    int d = s_cnt[tid] - cnt;
    const int total = s_cnt[IT - 1];
    for (int n = lo; n < hi; ++n) {
        const int4 rq = a.req[n];                    // token, source node (-1: zero state), destination node, live
        a.slot[n] = rq.w ? d : -1;
        if (rq.w) a.slot[a.ncol + d++] = rq.x;
    }
    for (int n = lo; n < hi; ++n) ulen[n] = n < total ? 1 : 0;
}

__global__ __launch_bounds__(256) void lm_columns_in_kernel(const LmColumns a, float* state, size_t layer_floats, int L, int Np, int H) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.ncol * L * H) return;
    const int k = (int)(i % H), l = (int)((i / H) % L), n = (int)(i / ((size_t)H * L));
    const int d = a.slot[n];
    if (d < 0) return;
    const int src_node = a.req[n].y;
    const float* src = src_node >= 0 ? lm_node(a, n, src_node) + (size_t)l * 2 * H : nullptr;
    float* base = state + (size_t)l * layer_floats;
    base[(size_t)d * H + k] = src ? src[k] : 0.f;                                  // buffer 0: the step's input
    base[(size_t)2 * Np * H + (size_t)d * H + k] = src ? src[H + k] : 0.f;
}

__global__ __launch_bounds__(256) void lm_columns_out_kernel(const LmColumns a, const float* state, size_t layer_floats, int L, int Np, int H) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.ncol * L * H) return;
    const int k = (int)(i % H), l = (int)((i / H) % L), n = (int)(i / ((size_t)H * L));
    const int d = a.slot[n];
    if (d < 0) return;
    float* dst = lm_node(a, n, a.req[n].z) + (size_t)l * 2 * H;
    const float* base = state + (size_t)l * layer_floats;
    dst[k] = base[(size_t)Np * H + (size_t)d * H + k];                             // buffer 1: the step's output
    dst[H + k] = base[(size_t)2 * Np * H + (size_t)d * H + k];
}

}  // namespace

const EcLmConfig* ecdec::lm_handle_config(const EcLm* lm, bool finalized) { return lm && (lm->finalized || !finalized) ? &lm->cfg : nullptr; }

int ecdec::lm_columns_step(const EcLm* lm, const LmColumns& a, char* lm_ws, hipStream_t s) {
    const LmLayout L = lm_layout(lm->cfg, a.ncol);
    int* ulen = reinterpret_cast<int*>(lm_ws + L.ulen);
    float* state = reinterpret_cast<float*>(lm_ws + L.state);
    const int H = lm->cfg.dim_model, V = lm->cfg.vocab_size, NL = lm->cfg.num_layers, Np = lm_npad(a.ncol);
    const size_t layer_floats = L.layer / 4, cells = (size_t)a.ncol * NL * H;
    const unsigned grid = (unsigned)((cells + 255) / 256);
    hipLaunchKernelGGL(lm_columns_index_kernel, dim3(1), dim3(IT), 0, s, a, ulen);
    hipLaunchKernelGGL(lm_columns_in_kernel, dim3(grid), dim3(256), 0, s, a, state, layer_floats, NL, Np, H);
    if (hipGetLastError() != hipSuccess) return -1;
    for (int l = 0; l < NL; ++l)
        if (launch_step(lm, state, layer_floats, l, 0, a.ncol, a.slot + a.ncol, 1, 0, ulen, 0, s) != 0) return -1;
    HeadArgs h{};
    h.wfc16 = lm->wfc16; h.bfc = lm->bfc;
    h.h = state + (size_t)(NL - 1) * layer_floats + (size_t)Np * H;
    h.ulen = ulen; h.logits = a.logits; h.N = a.ncol; h.H = H; h.V = V; h.tmp = 1.f;
    hipLaunchKernelGGL(lm_head_kernel<true>, dim3(Np / HC), dim3(HT), 0, s, h);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(lm_columns_out_kernel, dim3(grid), dim3(256), 0, s, a, state, layer_floats, NL, Np, H);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

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
    lm->allocs.free_all();
    delete lm;
}

int effconf_lm_load_tensor(EcLm* lm, const char* key, const float* host, const int64_t* shape, int32_t ndim) {
    if (!lm || !key || !host || (ndim > 0 && !shape)) return ec_fail("null argument");
    host_tensor_put(lm->host, key, host, shape, ndim);
    lm->finalized = false;
    return 0;
}

int effconf_lm_finalize(EcLm* lm) {
    if (!lm) return ec_fail("null handle");
    const int H = lm->cfg.dim_model, V = lm->cfg.vocab_size, L = lm->cfg.num_layers;
    // every tensor is looked up before the first device call: a missing key is reported without a GPU
    std::string err;                                 // the first tensor that is missing or misshapen
    auto need = [&](const std::string& key, std::initializer_list<int64_t> shape) {
        std::string e;
        const EcRnntHostT* t = ::need(lm->host, key, shape, e);
        if (!t && err.empty()) err = e;
        return t;
    };
    const EcRnntHostT* emb = need("decoder.embedding.weight", {V, H});
    const EcRnntHostT* wfc = need("fc.weight", {V, H});
    const EcRnntHostT* bfc = need("fc.bias", {V});
    const EcRnntHostT *wih[MAX_L], *whh[MAX_L], *bih[MAX_L], *bhh[MAX_L];
    for (int l = 0; l < L; ++l) {
        const std::string p = "decoder.rnn.", sfx = "_l" + std::to_string(l);
        wih[l] = need(p + "weight_ih" + sfx, {4 * H, H});
        whh[l] = need(p + "weight_hh" + sfx, {4 * H, H});
        bih[l] = need(p + "bias_ih" + sfx, {4 * H});
        bhh[l] = need(p + "bias_hh" + sfx, {4 * H});
    }
    if (!err.empty()) return ec_fail(err.c_str());
    lm->allocs.free_all();
    lm->finalized = false;
    bool ok = true;
    for (int l = 0; l < L; ++l) {
        std::vector<float> bs(4 * H);
        for (int i = 0; i < 4 * H; ++i) bs[i] = bih[l]->data[i] + bhh[l]->data[i];
        lm->bsum[l] = (const float*)lm->allocs.upload(bs.data(), bs.size() * 4);
        if (l == 0) {
            const std::vector<float> img = kperm16(whh[0]->data, 4 * H, H);
            lm->w16[0] = (const float4*)lm->allocs.upload(img.data(), img.size() * 4);
        } else {
            std::vector<float> cat((size_t)4 * H * 2 * H);           // [W_ih_l | W_hh_l]: rows of 2H
            for (int r = 0; r < 4 * H; ++r) {
                std::copy(wih[l]->data.begin() + (size_t)r * H, wih[l]->data.begin() + (size_t)(r + 1) * H, cat.begin() + (size_t)r * 2 * H);
                std::copy(whh[l]->data.begin() + (size_t)r * H, whh[l]->data.begin() + (size_t)(r + 1) * H, cat.begin() + (size_t)r * 2 * H + H);
            }
            const std::vector<float> img = kperm16(cat, 4 * H, 2 * H);
            lm->w16[l] = (const float4*)lm->allocs.upload(img.data(), img.size() * 4);
        }
        ok = ok && lm->bsum[l] && lm->w16[l];
    }
    {
        const std::vector<float> img = kperm16(wfc->data, V, H);
        lm->wfc16 = (const float4*)lm->allocs.upload(img.data(), img.size() * 4);
    }
    lm->bfc = (const float*)lm->allocs.upload(bfc->data.data(), bfc->data.size() * 4);
    float* d_emb = (float*)lm->allocs.upload(emb->data.data(), emb->data.size() * 4);
    float* d_wih = (float*)lm->allocs.upload(wih[0]->data.data(), wih[0]->data.size() * 4);
    float* d_gin = (float*)lm->allocs.upload(nullptr, (size_t)V * 4 * H * 4);
    if (!ok || !lm->wfc16 || !lm->bfc || !d_emb || !d_wih || !d_gin) return ec_fail("lm: device allocation / upload failed");
    // Gin0[y] = W_ih0 emb[y] + (b_ih0 + b_hh0) for every token id; row 0 from the embedding row the checkpoint holds
    if (launch_sgemm_nt(d_emb, H, d_wih, H, lm->bsum[0], d_gin, 4 * H, V, 4 * H, H, nullptr) != 0) return ec_fail("lm: Gin GEMM launch failed");
    if (hipDeviceSynchronize() != hipSuccess) return ec_fail("lm: Gin GEMM failed");
    lm->allocs.release(d_emb);                           // only the Gin GEMM read them
    lm->allocs.release(d_wih);
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
    char* ws = WsPlan::base(workspace);
    int* ulen = reinterpret_cast<int*>(ws + L.ulen);
    float* state = reinterpret_cast<float*>(ws + L.state);
    const int H = lm->cfg.dim_model, V = lm->cfg.vocab_size, NL = lm->cfg.num_layers, Np = lm_npad(n);
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
    char* ws = WsPlan::base(workspace);
    float* state = reinterpret_cast<float*>(ws + L.state);
    const int H = lm->cfg.dim_model, V = lm->cfg.vocab_size, NL = lm->cfg.num_layers, Np = lm_npad(n);
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
