// The decoders' common layer: what rnnt.hip (greedy: per-utterance and cluster kernels), rnnt_beam.hip, rnnt_lattice.hip, rnnt_align.hip, lm.hip, ctc_beam.hip and
// ctc_align.hip share, each piece once - the fp32-MFMA mat-vec, the LSTM cell and its 16-column MFMA step, the vocabulary log-softmax GEMM loop, transcript
// validation and the host handles' tensor / allocation plumbing.  The workspace layouts are in decode_layout.h (plain C++).
// The prediction network's weights live in the k-major / k-permuted images effconf_rnnt_finalize builds; the fp32-MFMA mat-vec
// below keeps the k order of every dot product ascending whatever the number of state vectors (columns) it multiplies.
#pragma once
#include "kernels.h"
#include "common.h"
#include "decode_layout.h"

#include <algorithm>
#include <initializer_list>
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

// ---- the LSTM cell (torch gate order i, f, g, o) of every decoder: the four pre-activations and the old cell state -> (c, h).  The greedy, cluster, beam, lattice
// and LM kernels are held to identical tokens and scores by the tests; this function is what makes them the same arithmetic.
struct LstmState { float c, h; };
__device__ __forceinline__ LstmState lstm_cell(float pi, float pf, float pg, float po, float cold) {
    const float ig = sigmoid_precise(pi), fg = sigmoid_precise(pf), gg = tanhf(pg), og = sigmoid_precise(po);
    const float c = fg * cold + ig * gg;
    return {c, og * tanhf(c)};
}

// ---- one LSTM step of 16 sequences (the columns of the MFMA tiles) for the 16 hidden units 16 ub .. 16 ub + 15: gates = Gin[y] + W_hh h as four gate tiles
// (rows q H + 16 ub + j), then the cell; row 4 g + e of the tiles = hidden unit, column j = lane & 15 = sequence.  x_lane: the lane's entry of its column's h in
// LDS (k-permuted).  Col describes the lane's column:
//   const float* gin      Gin row of the column's token
//   bool live             false: no cell is computed, put() sees h = c = 0
//   float c_old(unit)     the old cell state
//   void put(unit, h, c)  where the new state goes
template <class Col>
__device__ __forceinline__ void lstm_step16(const RnntDev& w, int ub, const float* x_lane, const Col col) {
    const int H = w.H, j = threadIdx.x & 15, g = (threadIdx.x & 63) >> 4;
    int nrow[4];
    f32x4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { nrow[q] = q * H + 16 * ub + j; acc[q] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    mfma_rows16_any<4>(w.whh16, 4 * H, H / 16, nrow, x_lane, acc);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int unit = 16 * ub + 4 * g + e;
        LstmState s{0.f, 0.f};
        if (col.live) s = lstm_cell(acc[0][e] + col.gin[unit], acc[1][e] + col.gin[H + unit], acc[2][e] + col.gin[2 * H + unit], acc[3][e] + col.gin[3 * H + unit], col.c_old(unit));
        col.put(unit, s.h, s.c);
    }
}

// ---- the vocabulary log-softmax GEMM of the lattice's joint kernel and the LM head: logits[n][c] = W[n] . x[c] + b[n] over the 16-row tiles of W16 ([K16][4][V],
// kperm16) against 32 columns = two 16-column groups (x0 / x1: the lane's entries of columns j and 16 + j, k-permuted), fp32 operands, k ascending.  Wave `wave` of
// NWAVES owns the tile pairs wave, wave + NWAVES, ..; DEPTH 16-blocks of weight loads are in flight per tile (each kernel's own instruction schedule).  Per tile pair
// the epilogue forms v = (acc + b) / tmp, hands every entry n < V to pick(n, v of column j, v of column 16 + j), and keeps the lane's running (max, sum exp) of its
// two columns in ms = {m0, s0, m1, s1}.  V % 16 != 0: rows clamped on load, masked with -inf.
// running (max, sum exp): merge of two partial results; an empty part is (-inf, 0)
__device__ __forceinline__ void ms_merge(float& m, float& s, float om, float os) {
    const float nm = fmaxf(m, om);
    const float ea = m == -INFINITY ? 0.f : expf(m - nm), eb = om == -INFINITY ? 0.f : expf(om - nm);
    s = s * ea + os * eb;
    m = nm;
}

template <int DEPTH, int NWAVES, class Pick>
__device__ __forceinline__ void vocab_lse_tiles(const float4* __restrict__ W16, const float* __restrict__ bias, int V, int K16, const float* x0, const float* x1,
                                                float tmp, const Pick pick, float (&ms)[4]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
    const int ntile = (V + 15) / 16;
    const size_t bs = (size_t)4 * V;                 // float4s per 16-block of the weight image: [g][n]
    float m0 = -INFINITY, m1 = -INFINITY, r0 = 0.f, r1 = 0.f;
    for (int tp = wave; 2 * tp < ntile; tp += NWAVES) {
        const float4* wp[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int n = 16 * (2 * tp + i) + j;
            wp[i] = W16 + (size_t)g * V + (n < V ? n : V - 1);     // clamped: rows at or beyond V are masked below
        }
        f32x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
        float4 wc[DEPTH][2], wn[DEPTH][2];           // [16-block in flight][tile]
#pragma unroll
        for (int q = 0; q < DEPTH; ++q)
#pragma unroll
            for (int i = 0; i < 2; ++i) wc[q][i] = wp[i][(size_t)(q < K16 ? q : K16 - 1) * bs];
        for (int q0 = 0; q0 < K16; q0 += DEPTH) {
#pragma unroll
            for (int q = 0; q < DEPTH; ++q) {
                const int qn = q0 + DEPTH + q < K16 ? q0 + DEPTH + q : K16 - 1;      // past the end: a harmless re-load
#pragma unroll
                for (int i = 0; i < 2; ++i) wn[q][i] = wp[i][(size_t)qn * bs];
            }
#pragma unroll
            for (int q = 0; q < DEPTH; ++q) {
                if (q0 + q < K16) {
                    const float4 xa = *reinterpret_cast<const float4*>(x0 + 16 * (q0 + q));
                    const float4 xb = *reinterpret_cast<const float4*>(x1 + 16 * (q0 + q));
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[q][i].x, xa.x, acc[i][0], 0, 0, 0);
                        acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[q][i].x, xb.x, acc[i][1], 0, 0, 0);
                        acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[q][i].y, xa.y, acc[i][0], 0, 0, 0);
                        acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[q][i].y, xb.y, acc[i][1], 0, 0, 0);
                        acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[q][i].z, xa.z, acc[i][0], 0, 0, 0);
                        acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[q][i].z, xb.z, acc[i][1], 0, 0, 0);
                        acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[q][i].w, xa.w, acc[i][0], 0, 0, 0);
                        acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[q][i].w, xb.w, acc[i][1], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < DEPTH; ++q)
#pragma unroll
                for (int i = 0; i < 2; ++i) wc[q][i] = wn[q][i];
        }
        // ---- epilogue of the pair: row 4 g + e of tile i = vocabulary entry n, column j = cell / sequence
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int nb = 16 * (2 * tp + i) + 4 * g;
            float v0[4], v1[4];
            float t0 = -INFINITY, t1 = -INFINITY;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int n = nb + e;
                const float b = bias[n < V ? n : V - 1];
                v0[e] = n < V ? (acc[i][0][e] + b) / tmp : -INFINITY;
                v1[e] = n < V ? (acc[i][1][e] + b) / tmp : -INFINITY;
                t0 = fmaxf(t0, v0[e]); t1 = fmaxf(t1, v1[e]);
                if (n < V) pick(n, v0[e], v1[e]);
            }
            if (nb < V) {                            // at least one entry: nb itself
                float p0 = 0.f, p1 = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) { p0 += expf(v0[e] - t0); p1 += expf(v1[e] - t1); }     // exp(-inf) = 0 for the masked entries
                ms_merge(m0, r0, t0, p0);
                ms_merge(m1, r1, t1, p1);
            }
        }
    }
    ms[0] = m0; ms[1] = r0; ms[2] = m1; ms[3] = r1;
}

// The lanes' running (max, sum exp) of vocab_lse_tiles -> lse = max + log(sum) of column threadIdx.x (threads 0 .. 31; the others get 0), merged in a fixed order:
// the k-slots of a wave (g = 0 + 1, 2 + 3, then the two halves), then the waves ascending.  One barrier; s_m / s_s: [NWAVES][32] floats of LDS.
template <int NWAVES>
__device__ __forceinline__ float vocab_lse_merge(float (&ms)[4], float (&s_m)[NWAVES][32], float (&s_s)[NWAVES][32]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
    float m0 = ms[0], r0 = ms[1], m1 = ms[2], r1 = ms[3];
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const float om0 = __shfl_xor(m0, o), os0 = __shfl_xor(r0, o), om1 = __shfl_xor(m1, o), os1 = __shfl_xor(r1, o);
        if (!(lane & o)) { ms_merge(m0, r0, om0, os0); ms_merge(m1, r1, om1, os1); }
    }
    if (g == 0) { s_m[wave][j] = m0; s_s[wave][j] = r0; s_m[wave][16 + j] = m1; s_s[wave][16 + j] = r1; }
    __syncthreads();
    if (tid >= 32) return 0.f;
    float m = s_m[0][tid], s = s_s[0][tid];
#pragma unroll
    for (int q = 1; q < NWAVES; ++q) ms_merge(m, s, s_m[q][tid], s_s[q][tid]);
    return m + logf(s);
}

// ---- transcripts: lengths arrive as int64 and are clamped to what the buffers hold; a transcript is refused (status 2) when its length is outside 0 .. u_max or
// one of its tokens outside 1 .. V - 1 (y null: the length alone).  Tokens without frames (status 1) is the caller's rule: it knows its frames.
__device__ __forceinline__ int clamp_len(long long v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }
__device__ __forceinline__ bool token_refused(int c, int V) { return c < 1 || c >= V; }
__device__ __forceinline__ int transcript_status(long long len, int u_max, const int* y, int V) {
    if (len < 0 || len > u_max) return 2;
    int st = 0;
    if (y)
        for (int u = 0; u < (int)len; ++u)
            if (token_refused(y[u], V)) st = 2;
    return st;
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

// ---- host: the tensors a handle (EcRnnt, EcLm) was given, and the device memory its finalize owns
struct EcRnntHostT { std::vector<int64_t> shape; std::vector<float> data; };
using EcHostTensors = std::map<std::string, EcRnntHostT>;

inline void host_tensor_put(EcHostTensors& host, const char* key, const float* data, const int64_t* shape, int32_t ndim) {
    EcRnntHostT t;
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= shape[i]; }
    t.data.assign(data, data + n);
    host[key] = std::move(t);
}

// the tensor `key` of that shape, or null with err naming it (a later failure overwrites an earlier one)
inline const EcRnntHostT* need(const EcHostTensors& host, const std::string& key, std::initializer_list<int64_t> shape, std::string& err) {
    auto it = host.find(key);
    if (it == host.end()) { err = "missing tensor " + key; return nullptr; }
    if (it->second.shape != std::vector<int64_t>(shape)) { err = "bad shape for " + key; return nullptr; }
    return &it->second;
}

struct DeviceAllocs {
    std::vector<void*> ptrs;
    void* upload(const void* src, size_t bytes) {                     // hipMalloc (+ copy when src); null on failure
        void* d = nullptr;
        if (hipMalloc(&d, bytes) != hipSuccess) return nullptr;
        ptrs.push_back(d);
        if (src && hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return d;
    }
    void release(void* p) {                                            // one of upload()'s, early
        (void)hipFree(p);
        ptrs.erase(std::find(ptrs.begin(), ptrs.end(), p));
    }
    void free_all() {
        for (void* p : ptrs) (void)hipFree(p);
        ptrs.clear();
    }
};

// ---- lm.hip's column step, for the fused beam search of rnnt_beam.hip (internal: not part of the C ABI).  One LM step of `ncol` columns on the caller's
// stream: pack the live requests into the first columns of the step state (slot[n]: request n's packed column, -1 when it is not live; slot[ncol + d]: the token
// of packed column d), gather the (h, c) of their source nodes (-1: zeros), lm_lstm_step_kernel per layer (a column tile without a live column returns at once),
// lm_head_kernel<true> for the raw logits rows logits[packed column][V], scatter the new (h, c) to the destination nodes.  A request is int4 {token, source
// node, destination node, live}; request n belongs to utterance n / cols_per_utt, whose LM nodes of node_floats floats start at utt + that * per_utt + lmnodes.
// lm_ws: the 256-aligned region of lm_layout(cfg, ncol).  Every column's result is that of effconf_lm_step on it alone, wherever it is packed.
struct EcLm;
namespace ecdec {
struct LmColumns {
    const int4* req; int ncol, cols_per_utt;
    int* slot;                                                        // [2 * ncol]
    char* utt; size_t per_utt, lmnodes; int node_floats;
    float* logits;
};
const EcLmConfig* lm_handle_config(const EcLm* lm, bool finalized);    // null: no handle, or (finalized asked for) not finalized
int lm_columns_step(const EcLm* lm, const LmColumns& a, char* lm_ws, hipStream_t s);
}  // namespace ecdec

struct EcRnnt {
    EcRnntConfig cfg;
    EcHostTensors host;
    DeviceAllocs allocs;
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
