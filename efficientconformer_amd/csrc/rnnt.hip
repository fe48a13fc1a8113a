// RNN-T greedy decode (gfx950): prediction network (Embedding + 1-layer LSTM), joint network and the greedy loop.
//
// Reference: Transducer.gready_search_decoding (models/transducer.py:139-186), RnnDecoder.forward
// (models/decoders.py:41-70: Embedding -> nn.LSTM, batch_first, 1 layer), JointNetwork.forward in decoding mode
// (models/joint_networks.py:80-104: linear_encoder(f) + linear_decoder(g) -> tanh -> linear_joint), and
// max_consec_dec_step (transducer.py:83, 173).
//
// The reference decodes one utterance at a time with one joint_network call (three nn.Linear, a softmax and an
// .argmax() host sync) per (frame, token) decision.  Here:
//   * everything input-independent is hoisted into tables at finalize():  Gin[y] = W_ih emb[y] + b_ih + b_hh for every
//     token id y (the LSTM only ever sees embedding rows), so a decoder step is one 4H x H mat-vec;
//   * linear_encoder(f) is one fp32 GEMM over all (b, t) per batch (the reference recomputes it per decision,
//     joint_networks.py:82);
//   * the sequential part runs as ONE persistent workgroup per utterance: state (h, c, g_dec, z) lives in LDS, weights
//     stream from L2 in a k-major float4 layout (W4[k/4][n] = W[n][4k/4 .. +3]) so that a wave's loads are contiguous
//     1 KB rows, and RNNT_KF consecutive encoder frames are evaluated speculatively per pass over the joint weight
//     (between two emitted tokens the decoder output does not change, so the extra frames are exactly the frames the
//     reference would evaluate next as long as it keeps reading blanks).
// All arithmetic is fp32 (the decisions feed back into the recurrence: one flipped argmax changes every later token,
// so the head is kept at the reference's precision; softmax().log().argmax() of transducer.py:164 is argmax(logits)).
// Bound: L2 -> CU bandwidth on the weights (4H*H*4 + J*H*4 bytes per token, V*J*4 per joint pass).
#include "decode_common.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include <type_traits>

int ec_fail(const char* msg);

using namespace ecrnnt;
using namespace ecdec;

namespace {

constexpr int NT = 512;        // threads per utterance
constexpr int KF = 4;          // encoder frames per joint pass
constexpr int JMC = 2;         // joint columns per thread and pass

// ------------------------------------------------------------------------------------------------------------------
// fp32 GEMM  C[m][n] = sum_k A[m][k] * B[n][k] + bias[n]   (nn.Linear semantics), K % 4 == 0.  64x64x16 tiles.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sgemm_nt_kernel(const float* __restrict__ A, int lda, const float* __restrict__ Bw, int ldb,
                                                       const float* __restrict__ bias, float* __restrict__ C, int ldc, int M, int N, int K) {
    __shared__ float As[16][68], Bs[16][68];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int lr = tid >> 2, lk = (tid & 3) * 4;
    const int am = m0 + lr < M ? m0 + lr : M - 1, bn = n0 + lr < N ? n0 + lr : N - 1;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 16) {
        const int kk = k0 + lk < K ? k0 + lk : K - 4;                       // clamped, masked below
        float4 a = *reinterpret_cast<const float4*>(A + (size_t)am * lda + kk);
        float4 b = *reinterpret_cast<const float4*>(Bw + (size_t)bn * ldb + kk);
        if (k0 + lk >= K) { a = make_float4(0.f, 0.f, 0.f, 0.f); b = a; }
        __syncthreads();
        As[lk + 0][lr] = a.x; As[lk + 1][lr] = a.y; As[lk + 2][lr] = a.z; As[lk + 3][lr] = a.w;
        Bs[lk + 0][lr] = b.x; Bs[lk + 1][lr] = b.y; Bs[lk + 2][lr] = b.z; Bs[lk + 3][lr] = b.w;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const float4 av = *reinterpret_cast<const float4*>(&As[k][ty * 4]);
            const float4 bv = *reinterpret_cast<const float4*>(&Bs[k][tx * 4]);
            const float ar[4] = {av.x, av.y, av.z, av.w}, br[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(ar[i], br[j], acc[i][j]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tx * 4 + j;
            if (n < N) C[(size_t)m * ldc + n] = acc[i][j] + (bias ? bias[n] : 0.f);
        }
    }
}

}  // namespace

int ecrnnt::launch_sgemm_nt(const float* A, int lda, const float* Bw, int ldb, const float* bias, float* C, int ldc, int M, int N, int K, hipStream_t s) {
    if (M <= 0 || N <= 0) return 0;
    if (K % 4 || K < 4) return -2;
    hipLaunchKernelGGL(sgemm_nt_kernel, dim3((N + 63) / 64, (M + 63) / 64), dim3(256), 0, s, A, lda, Bw, ldb, bias, C, ldc, M, N, K);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

namespace {

// ------------------------------------------------------------------------------------------------------------------
// mat-vec against a k-major float4 weight image: y[n] = sum_k W[n][k] x[k], W4[(k/4)*N + n] = W[n][k..k+3].
// Thread owns columns n = n0 + tid + NT*m (m < MC); x is NX vectors in LDS (pitch xp floats), read as broadcasts.
// ------------------------------------------------------------------------------------------------------------------
template <int MC, int NX>
__device__ __forceinline__ void matvec(const float4* __restrict__ W4, int N, int K4, int n0, const float* xs, int xp, float (&acc)[MC][NX]) {
    int col[MC];
#pragma unroll
    for (int m = 0; m < MC; ++m) {
        const int n = n0 + (int)threadIdx.x + NT * m;
        col[m] = n < N ? n : N - 1;                                          // clamped: garbage columns are never used
#pragma unroll
        for (int x = 0; x < NX; ++x) acc[m][x] = 0.f;
    }
#pragma unroll 4
    for (int k4 = 0; k4 < K4; ++k4) {
        float4 w[MC];
#pragma unroll
        for (int m = 0; m < MC; ++m) w[m] = W4[(size_t)k4 * N + col[m]];
#pragma unroll
        for (int x = 0; x < NX; ++x) {
            const float4 xv = *reinterpret_cast<const float4*>(xs + x * xp + 4 * k4);
#pragma unroll
            for (int m = 0; m < MC; ++m)
                acc[m][x] = fmaf(w[m].w, xv.w, fmaf(w[m].z, xv.z, fmaf(w[m].y, xv.y, fmaf(w[m].x, xv.x, acc[m][x]))));
        }
    }
}


// One prediction-network step on token y and the decoder projection the joint reads: h, c -> h', c' (sg: the gate pre-activations), gd = linear_decoder(h') + bias.
// Ends behind a barrier.
__device__ __forceinline__ void decoder_step(const RnntDev& w, int y, float* sh, float* sc, float* sg, float* sgd) {
    const int H = w.H, J = w.J, tid = threadIdx.x;
    // ---- decoder step: gates = Gin[y] + W_hh h   (torch LSTM gate order i, f, g, o)
    for (int n0 = 0; n0 < 4 * H; n0 += NT * 5) {
        float acc[5][1];
        matvec<5, 1>(w.whh4, 4 * H, H / 4, n0, sh, H, acc);
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            const int n = n0 + tid + NT * m;
            if (n < 4 * H) sg[n] = acc[m][0] + w.gin[(size_t)y * 4 * H + n];
        }
    }
    __syncthreads();
    for (int j = tid; j < H; j += NT) {
        const LstmState s = lstm_cell(sg[j], sg[H + j], sg[2 * H + j], sg[3 * H + j], sc[j]);
        sc[j] = s.c;
        sh[j] = s.h;
    }
    __syncthreads();
    // ---- gd = linear_decoder(h)
    for (int n0 = 0; n0 < J; n0 += NT * 2) {
        float acc[2][1];
        matvec<2, 1>(w.wd4, J, H / 4, n0, sh, H, acc);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int n = n0 + tid + NT * m;
            if (n < J) sgd[n] = acc[m][0] + w.bd[n];
        }
    }
    __syncthreads();
}

// What a resumed decode adds to the whole-utterance one: workgroup b decodes the new frames of stream streams[b], whose record (h[H], c[H], gd[J] = linear_decoder(h) +
// bias; primed[stream] != 0: the record holds the state at a frame boundary) it reads on entry and writes on exit.  At a frame boundary, and only there, the consecutive
// counter is 0, the LSTM has consumed every emitted token and gd is what the next joint evaluation reads - so nothing else is carried.
struct StreamIo {
    const int* streams;      // [n] stream ids
    int* primed;             // [max_streams]
    float* rec;              // records, rec_floats apart
    int rec_floats, max_streams;
    int* token_frames;       // [n][max_tok] push-local frame of every token, -1 behind them; nullable
    int* decoder_steps;      // [n] LSTM steps of this push; nullable
};

// One workgroup = one utterance (STREAM: one stream's push).  fe: [B][T][J] = linear_encoder(f) incl. bias.  The whole-utterance decode is "resume from a fresh state,
// write no state": STREAM = false compiles every stream access away.
template <bool STREAM>
__device__ __forceinline__ void greedy_body(const RnntDev& w, const float* __restrict__ fe, const int64_t* __restrict__ lens, int T, int* __restrict__ tokens,
                                            int* __restrict__ counts, int max_tok, const StreamIo& io) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int H = w.H, J = w.J, V = w.V;
    float* sh = lds;                       // [H]   h
    float* sc = sh + H;                    // [H]   c
    float* sg = sc + H;                    // [4H]  gate pre-activations
    float* sgd = sg + 4 * H;               // [J]   linear_decoder(h)
    float* sz = sgd + J;                   // [KF][J] tanh(fe + gd)
    float* sbv = sz + KF * J;              // [KF][NT/64] wave-best values
    int* sbi = reinterpret_cast<int*>(sbv + KF * (NT / 64));   // [KF][NT/64] wave-best indices
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    float* rec = nullptr;
    int sid = 0;
    bool primed = false;
    if constexpr (STREAM) {
        sid = io.streams[b];
        if (sid < 0 || sid >= io.max_streams) {          // uniform: the whole workgroup leaves, nothing but the length is written
            if (tid == 0) counts[b] = -1;
            return;
        }
        rec = io.rec + (size_t)sid * io.rec_floats;
        primed = io.primed[sid] != 0;
    }
    int Tb = (int)lens[b];
    Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    if (STREAM && primed) {                              // a record whose flag is clear is never read
        for (int i = tid; i < 2 * H; i += NT) sh[i] = rec[i];
        for (int i = tid; i < J; i += NT) sgd[i] = rec[2 * H + i];
    } else {
        for (int i = tid; i < 2 * H; i += NT) sh[i] = 0.f;   // hidden = None -> zeros (decoders.py:59-60)
    }
    __syncthreads();
    int y = 0, enc_step = 0, consec = 0, ntok = 0;       // y = x.new_zeros(1,1) (transducer.py:151)
    int nsteps = 0;
    bool run_dec = !primed;                              // a primed stream runs no decoder step and no decoder projection until it emits a token
    const float* feb = fe + (size_t)b * T * J;

    while (enc_step < Tb) {
        if (!STREAM || run_dec) {
            decoder_step(w, y, sh, sc, sg, sgd);
            ++nsteps;
        }
        run_dec = true;
        // ---- joint loop: KF frames per pass, until a token is emitted or the utterance ends
        bool emitted = false;
        while (!emitted && enc_step < Tb) {
            for (int i = tid; i < KF * J; i += NT) {
                const int kf = i / J, j = i - kf * J;
                const int t = enc_step + kf < Tb ? enc_step + kf : Tb - 1;    // clamped: frames past the end are never consulted
                sz[i] = tanhf(feb[(size_t)t * J + j] + sgd[j]);
            }
            __syncthreads();
            float bv[KF]; int bi[KF];
#pragma unroll
            for (int kf = 0; kf < KF; ++kf) { bv[kf] = -INFINITY; bi[kf] = 0x7fffffff; }
            for (int n0 = 0; n0 < V; n0 += NT * JMC) {
                float acc[JMC][KF];
                matvec<JMC, KF>(w.wj4, V, J / 4, n0, sz, J, acc);
#pragma unroll
                for (int m = 0; m < JMC; ++m) {
                    const int n = n0 + tid + NT * m;
                    const bool ok = n < V;
                    const float bz = w.bj[ok ? n : V - 1];
#pragma unroll
                    for (int kf = 0; kf < KF; ++kf) {
                        const float v = acc[m][kf] + bz;
                        if (ok && (v > bv[kf] || (v == bv[kf] && n < bi[kf]))) { bv[kf] = v; bi[kf] = n; }
                    }
                }
            }
#pragma unroll
            for (int kf = 0; kf < KF; ++kf) {
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) {
                    const float ov = __shfl_xor(bv[kf], o);
                    const int oi = __shfl_xor(bi[kf], o);
                    if (ov > bv[kf] || (ov == bv[kf] && oi < bi[kf])) { bv[kf] = ov; bi[kf] = oi; }
                }
                if (lane == 0) { sbv[kf * (NT / 64) + wave] = bv[kf]; sbi[kf * (NT / 64) + wave] = bi[kf]; }
            }
            __syncthreads();
            // ---- every thread walks the KF decisions identically (transducer.py:158-176)
#pragma unroll
            for (int kf = 0; kf < KF; ++kf) {
                if (emitted || enc_step >= Tb) break;
                float v = sbv[kf * (NT / 64)]; int pred = sbi[kf * (NT / 64)];
#pragma unroll
                for (int q = 1; q < NT / 64; ++q) {
                    const float ov = sbv[kf * (NT / 64) + q]; const int oi = sbi[kf * (NT / 64) + q];
                    if (ov > v || (ov == v && oi < pred)) { v = ov; pred = oi; }
                }
                if (pred == 0 || consec == w.max_consec) { consec = 0; ++enc_step; }
                else {
                    ++consec;
                    if (tid == 0 && ntok < max_tok) {
                        tokens[(size_t)b * max_tok + ntok] = pred;
                        if (STREAM && io.token_frames) io.token_frames[(size_t)b * max_tok + ntok] = enc_step;
                    }
                    ++ntok;
                    y = pred;
                    emitted = true;
                }
            }
            __syncthreads();     // sz / sbv are rewritten by the next pass
        }
    }
    if (tid == 0) counts[b] = ntok < max_tok ? ntok : max_tok;
    for (int i = ntok + tid; i < max_tok; i += NT) tokens[(size_t)b * max_tok + i] = 0;
    if constexpr (STREAM) {
        if (io.token_frames)
            for (int i = ntok + tid; i < max_tok; i += NT) io.token_frames[(size_t)b * max_tok + i] = -1;
        if (tid == 0 && io.decoder_steps) io.decoder_steps[b] = nsteps;
        if (Tb > 0) {                                    // the loop ended behind a blank or a forced decision: a frame boundary.  No frame: the record stays as it is
            for (int i = tid; i < 2 * H; i += NT) rec[i] = sh[i];
            for (int i = tid; i < J; i += NT) rec[2 * H + i] = sgd[i];
            if (tid == 0) io.primed[sid] = 1;
        }
    }
}

__global__ __launch_bounds__(NT) void rnnt_greedy_kernel(RnntDev w, const float* __restrict__ fe, const int64_t* __restrict__ lens,
                                                         int T, int* __restrict__ tokens, int* __restrict__ counts, int max_tok) {
    greedy_body<false>(w, fe, lens, T, tokens, counts, max_tok, StreamIo{});
}

// One workgroup = the new frames of one listed stream.  fe: [n][T][J] of the push.
__global__ __launch_bounds__(NT) void rnnt_greedy_resume_kernel(RnntDev w, const float* __restrict__ fe, const int64_t* __restrict__ lens,
                                                                int T, int* __restrict__ tokens, int* __restrict__ counts, int max_tok, StreamIo io) {
    greedy_body<true>(w, fe, lens, T, tokens, counts, max_tok, io);
}


// ------------------------------------------------------------------------------------------------------------------
// Cluster decode: CW workgroups share CU utterances and run them in lockstep rounds.  Every workgroup owns 1/CW of the
// LSTM's hidden units (their 4 gate columns and cell state), of the decoder projection's columns and of the vocabulary, so the
// weights a round streams from L2 are read ONCE per cluster instead of once per utterance, and the per-step latency of an
// utterance drops from "10.7 MB through one CU" to "1.3 MB through each of CW CUs" plus three cluster barriers
// (counter in global memory: agent-scope release / acquire, bounded spin).  State machines (token, frame, counters) are
// replicated: every workgroup takes the same decisions from the same exchanged argmax candidates.  The three mat-vec phases run on
// the fp32 matrix pipe (mfma_rows16 below) with the k order of every dot product ascending as in rnnt_greedy_kernel, the rest (libm
// tanhf / expf, the decisions) is that kernel's code: both produce identical tokens (tests: the reference's goldens and 165 k tokens
// of tools/rnnt_diag.py).  Round 3, per round of a 256-utterance decode: 206 k -> 112 k cycles (140 -> 46 ms per decode).
// ------------------------------------------------------------------------------------------------------------------
// Two cluster shapes <CW workgroups, CU utterances, CKF encoder frames per joint pass>, CU * CKF = 16 = the columns of an MFMA tile:
//   <8, 8, 2>    round 3's: 32 clusters at B = 256, every one of them streams the whole 10.7 MB (Transducer-Medium) per round - 342 MB per round through the
//                L2s, which is what a round costs; the gate / decoder-projection tiles use 8 of their 16 columns
//   <16, 16, 1>  round 6 (option cluster_shape = 1): 16 clusters - half the bytes per round and per workgroup, all 16 columns of every tile used; the state of 16
//                utterances (h, linear_decoder(h), one joint input each) is 3 x 16 x 640 x 4 B = 123 KB of LDS, so no second speculative frame.
//                MEASURED (profiles/r6_33_rnnt_cluster_shapes.txt): 41.9 ms against 42.4 ms at B = 256 - and B = 64 (8 clusters instead of 32) takes the same
//                40 ms: a decode is ~1090 lockstep rounds of ~38 us whatever the bytes per round, i.e. the round is a LATENCY chain (three cluster barriers +
//                exchange reloads + three dependent 160-MFMA accumulator chains), not the L2 stream the byte count suggests.  Kept as an option, not the default
//                (a blank-only decode costs 3.4 ms instead of 1.9: one frame per joint pass).
constexpr int CNT = 512;
constexpr int CLB = 8;         // weight loads kept in flight per thread (H/4 and J/4 must be multiples)

struct ClusterArgs {
    RnntDev w;
    const float* fe; const int64_t* lens; int T, B;
    int* tokens; int* counts; int max_tok;
    float* xh; float* xgd; float* xav; int* xai; unsigned* cnt; int* status;     // exchange buffers (per cluster), barrier counters
    int ncl, by_slice;
};


// Exchange data and the barrier counter are accessed with relaxed agent-scope atomics (sc1 loads / stores served at the coherent
// level) instead of plain accesses bracketed by agent-scope release / acquire fences: the fences cost a full L2 write-back +
// invalidate per workgroup per barrier (~40 us each here; three barriers per round made the cluster no faster than one workgroup per
// utterance).  Ordering: every wave drains its stores (s_waitcnt vmcnt(0) in __syncthreads) before thread 0 bumps the counter; the
// consumers read only after thread 0 has seen the counter and a second __syncthreads.
__device__ __forceinline__ void xstore(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void xstorei(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float xload(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int xloadi(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <int CW>
__device__ __forceinline__ bool cluster_sync(unsigned* cnt, unsigned& epoch, int* status) {
    __syncthreads();
    epoch += CW;
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        long spins = 0;
        while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < epoch) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > (1l << 26)) { __hip_atomic_store(status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }   // never hang the GPU
        }
    }
    __syncthreads();
    return __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
}


// exchange buffers -> registers, three 16-byte loads per lane in flight (sc1: served at the coherent level, as xload; plain loads instead of
// atomics so that they pipeline - the relaxed atomic loads were issued one at a time, 13k cycles per round for two 20 KB reloads).  The
// cluster barrier in front orders them against the producers' stores.
__device__ __forceinline__ void xload3(const float* p0, const float* p1, const float* p2, float4& a, float4& b, float4& c) {
    asm volatile("global_load_dwordx4 %0, %3, off sc1\n\tglobal_load_dwordx4 %1, %4, off sc1\n\tglobal_load_dwordx4 %2, %5, off sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(a), "=&v"(b), "=&v"(c) : "v"(p0), "v"(p1), "v"(p2) : "memory");
}

template <int CW, int CU, int CKF>
__global__ __launch_bounds__(CNT) void rnnt_cluster_kernel(const ClusterArgs a) {
    static_assert(CU * CKF == 16 && CU <= 16, "one MFMA column tile of joint inputs");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const RnntDev& w = a.w;
    const int H = w.H, J = w.J, V = w.V;
    const int HU = H / CW, JU = J / CW, VU = (V + CW - 1) / CW;
    float* sh = lds;                         // [CU][H]   h of every utterance
    float* sgd = sh + CU * H;                // [CU][J]
    float* sz = sgd + CU * J;                // [CU*CKF][J]
    float* sc = sz + CU * CKF * J;           // [CU][HU]  cell state of this workgroup's units
    float* sg = sc + CU * HU;                // [CU][4*HU] gate pre-activations
    float* sred = sg + CU * 4 * HU;          // [CU*CKF][8] partial argmax values, then indices
    int* sredi = reinterpret_cast<int*>(sred + CU * CKF * 8);
    __shared__ int s_y[CU], s_step[CU], s_consec[CU], s_ntok[CU], s_need[CU], s_T[CU], s_pred[CU * CKF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // workgroup -> (cluster, slice).  by_slice: consecutive workgroups are the CW = 8 slices of one cluster, i.e. slice k of EVERY cluster
    // runs on XCD k (workgroups are dealt to the 8 XCDs round-robin) and that XCD's L2 only ever holds slice k of the weights (1.3 of the
    // 10.7 MB: resident); otherwise the members of a cluster share an XCD (ncl % 8 == 0) and its L2 sees all 10.7 MB per round.
    const int cl = a.by_slice ? blockIdx.x / CW : blockIdx.x % a.ncl, wg = a.by_slice ? blockIdx.x % CW : blockIdx.x / a.ncl;
    const int u0 = cl * CU;
    float* xh = a.xh + (size_t)cl * CU * H;
    float* xgd = a.xgd + (size_t)cl * CU * J;
    float* xav = a.xav + (size_t)cl * CW * CU * CKF;
    int* xai = a.xai + (size_t)cl * CW * CU * CKF;
    unsigned* cnt = a.cnt + cl * 64;          // one counter per 256-byte line
    unsigned epoch = 0;

    for (int i = tid; i < CU * H; i += CNT) sh[i] = 0.f;             // hidden = None -> zeros
    for (int i = tid; i < CU * J; i += CNT) sgd[i] = 0.f;
    for (int i = tid; i < CU * HU; i += CNT) sc[i] = 0.f;
    if (tid < CU) {
        const int b = u0 + tid;
        int Tb = b < a.B ? (int)a.lens[b] : 0;
        Tb = Tb < 0 ? 0 : (Tb > a.T ? a.T : Tb);
        s_T[tid] = Tb; s_y[tid] = 0; s_step[tid] = 0; s_consec[tid] = 0; s_ntok[tid] = 0; s_need[tid] = Tb > 0;
    }
    __syncthreads();

    bool ok = true;
    while (ok) {
        bool active = false, dec = false;
#pragma unroll
        for (int u = 0; u < CU; ++u) { const bool act = s_step[u] < s_T[u]; active |= act; dec |= act && s_need[u]; }
        if (!active) break;
        if (dec) {
            // ---- phase 1: gates of this workgroup's units (4 HU rows of W_hh as 16-row tiles, dealt to the waves), cell update, h slice out
            {
                const int ntile = 4 * HU / 16;                             // HU % 4 == 0 (cluster_supported)
                const int j = lane & 15, g = lane >> 4;
                const float* xl = sh + (j % CU) * H + 4 * g;                // columns 8 .. 15 of B repeat the 8 utterances (results unused)
                auto run = [&](auto ntl_c) __attribute__((always_inline)) {
                    constexpr int NTL = decltype(ntl_c)::value;
                    int nrow[NTL];
                    f32x4 acc[NTL];
#pragma unroll
                    for (int i = 0; i < NTL; ++i) {
                        const int r = 16 * (wave + 8 * i) + j;             // local gate row of this lane's A operand
                        nrow[i] = (r / HU) * H + wg * HU + r % HU;
                        acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                    mfma_rows16<NTL>(w.whh16, 4 * H, H / 16, nrow, xl, acc);
                    if (j < CU) {
#pragma unroll
                        for (int i = 0; i < NTL; ++i)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int r = 16 * (wave + 8 * i) + 4 * g + e;
                                const int n = (r / HU) * H + wg * HU + r % HU;
                                sg[j * 4 * HU + r] = acc[i][e] + w.gin[(size_t)s_y[j] * 4 * H + n];
                            }
                    }
                };
                const int mine = (ntile - wave + 7) / 8;                   // tiles wave, wave + 8, ...
                if (mine == 1) run(std::integral_constant<int, 1>{});
                else if (mine == 2) run(std::integral_constant<int, 2>{});
                else if (mine == 3) run(std::integral_constant<int, 3>{});
                else if (mine >= 4) run(std::integral_constant<int, 4>{});
            }
            __syncthreads();
            for (int i = tid; i < CU * HU; i += CNT) {
                const int u = i / HU, unit = i - u * HU;
                float hv = sh[u * H + kperm(wg * HU + unit)];
                if (s_need[u] && s_step[u] < s_T[u]) {
                    const float* g = sg + u * 4 * HU + unit;
                    const LstmState s = lstm_cell(g[0], g[HU], g[2 * HU], g[3 * HU], sc[i]);
                    sc[i] = s.c;
                    hv = s.h;
                }
                xstore(xh + u * H + wg * HU + unit, hv);
            }
            ok = cluster_sync<CW>(cnt, epoch, a.status);
            for (int i0 = tid; i0 < CU * H / 4; i0 += 3 * CNT) {         // h of every utterance, k-permuted (see mfma_rows16)
                const int n4 = CU * H / 4, i1 = i0 + CNT, i2 = i0 + 2 * CNT;
                float4 v[3];
                xload3(xh + 4 * i0, xh + 4 * (i1 < n4 ? i1 : i0), xh + 4 * (i2 < n4 ? i2 : i0), v[0], v[1], v[2]);
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const int i = 4 * (i0 + e * CNT);
                    if (i < CU * H) {
                        float* d = sh + (i / H) * H + kperm(i % H);           // elements i .. i + 3 sit 4 floats apart
                        d[0] = v[e].x; d[4] = v[e].y; d[8] = v[e].z; d[12] = v[e].w;
                    }
                }
            }
            __syncthreads();
            // ---- phase 2: this workgroup's columns of linear_decoder(h): JU rows of W_d as 16-row tiles
            {
                const int ntile = (JU + 15) / 16;
                const int j = lane & 15, g = lane >> 4;
                for (int t = wave; t < ntile; t += 8) {
                    int nrow[1];
                    const int lr = 16 * t + j;
                    nrow[0] = wg * JU + (lr < JU ? lr : JU - 1);
                    f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
                    mfma_rows16<1>(w.wd16, J, H / 16, nrow, sh + (j % CU) * H + 4 * g, acc);
                    if (j < CU) {
                        const int u = j;
                        const bool upd = s_need[u] && s_step[u] < s_T[u];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int lc = 16 * t + 4 * g + e, n = wg * JU + lc;
                            if (lc < JU) xstore(xgd + u * J + n, upd ? acc[0][e] + w.bd[n] : sgd[u * J + n]);
                        }
                    }
                }
            }
            ok = cluster_sync<CW>(cnt, epoch, a.status) && ok;
            for (int i0 = tid; i0 < CU * J / 4; i0 += 3 * CNT) {
                const int n4 = CU * J / 4, i1 = i0 + CNT, i2 = i0 + 2 * CNT;
                float4 v[3];
                xload3(xgd + 4 * i0, xgd + 4 * (i1 < n4 ? i1 : i0), xgd + 4 * (i2 < n4 ? i2 : i0), v[0], v[1], v[2]);
                *reinterpret_cast<float4*>(sgd + 4 * i0) = v[0];
                if (i1 < n4) *reinterpret_cast<float4*>(sgd + 4 * i1) = v[1];
                if (i2 < n4) *reinterpret_cast<float4*>(sgd + 4 * i2) = v[2];
            }
            __syncthreads();
        }
        // ---- phase 3: joint on CKF frames per utterance, this workgroup's slice of the vocabulary
        for (int q0 = tid; q0 < CU * CKF * J / 4; q0 += 4 * CNT) {       // four 16-byte loads of linear_encoder(f) in flight per lane
            const int n4 = CU * CKF * J / 4, J4 = J / 4;
            float4 fv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int q = q0 + e * CNT < n4 ? q0 + e * CNT : q0;
                const int row = q / J4, u = row / CKF, kf = row - u * CKF;
                const int b = u0 + u < a.B ? u0 + u : a.B - 1;
                int t = s_step[u] + kf;
                t = t < s_T[u] ? t : (s_T[u] > 0 ? s_T[u] - 1 : 0);
                fv[e] = *reinterpret_cast<const float4*>(a.fe + ((size_t)b * a.T + t) * J + 4 * (q - row * J4));
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int q = q0 + e * CNT;
                if (q < n4) {
                    const int row = q / J4, j = 4 * (q - row * J4), u = row / CKF;
                    const float4 gd = *reinterpret_cast<const float4*>(sgd + u * J + j);
                    float* d = sz + row * J + kperm(j);                       // elements j .. j + 3 sit 4 floats apart
                    d[0] = tanhf(fv[e].x + gd.x); d[4] = tanhf(fv[e].y + gd.y); d[8] = tanhf(fv[e].z + gd.z); d[12] = tanhf(fv[e].w + gd.w);
                }
            }
        }
        __syncthreads();
        {   // VU vocabulary rows of W_j as 16-row tiles (one per wave) against the CU * CKF = 16 joint inputs; partial argmax per wave
            const int ntile = (VU + 15) / 16;                              // <= 8 (cluster_supported)
            const int j = lane & 15, g = lane >> 4;
            float bv = -INFINITY; int bi = 0x7fffffff;
            if (wave < ntile) {
                int nrow[1];
                const int lr = 16 * wave + j;
                const int nn = wg * VU + lr;
                nrow[0] = (lr < VU && nn < V) ? nn : V - 1;
                f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
                mfma_rows16<1>(w.wj16, V, J / 16, nrow, sz + j * J + 4 * g, acc);
#pragma unroll
                for (int e = 0; e < 4; ++e) {                              // rows 4 g + e of the tile, column j = (utterance, frame)
                    const int lc = 16 * wave + 4 * g + e, n = wg * VU + lc;
                    if (lc < VU && n < V) {
                        const float v = acc[0][e] + w.bj[n];
                        if (v > bv || (v == bv && n < bi)) { bv = v; bi = n; }
                    }
                }
            }
#pragma unroll
            for (int o = 16; o <= 32; o <<= 1) {                           // the 4 lane groups hold different rows of the same column
                const float ov = __shfl_xor(bv, o); const int oi = __shfl_xor(bi, o);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            if (lane < 16) { sred[lane * 8 + wave] = bv; sredi[lane * 8 + wave] = bi; }
        }
        __syncthreads();
        if (tid < CU * CKF) {
            float bv = sred[tid * 8]; int bi = sredi[tid * 8];
            for (int q = 1; q < 8; ++q) {
                const float ov = sred[tid * 8 + q]; const int oi = sredi[tid * 8 + q];
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            xstore(xav + wg * CU * CKF + tid, bv); xstorei(xai + wg * CU * CKF + tid, bi);
        }
        ok = cluster_sync<CW>(cnt, epoch, a.status) && ok;
        if (tid < CU * CKF) {
            float bv = xload(xav + tid); int bi = xloadi(xai + tid);
            for (int q = 1; q < CW; ++q) {
                const float ov = xload(xav + q * CU * CKF + tid); const int oi = xloadi(xai + q * CU * CKF + tid);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            s_pred[tid] = bi;
        }
        __syncthreads();
        // ---- decisions (transducer.py:158-176), identical in every workgroup
        if (tid < CU) {
            const int u = tid, b = u0 + u;
            int step = s_step[u], consec = s_consec[u], ntok = s_ntok[u], need = 0;
            for (int kf = 0; kf < CKF && step < s_T[u]; ++kf) {
                const int pred = s_pred[u * CKF + kf];
                if (pred == 0 || consec == w.max_consec) { consec = 0; ++step; }
                else {
                    ++consec;
                    if (wg == 0 && b < a.B && ntok < a.max_tok) a.tokens[(size_t)b * a.max_tok + ntok] = pred;
                    ++ntok;
                    s_y[u] = pred;
                    need = 1;
                    break;
                }
            }
            s_step[u] = step; s_consec[u] = consec; s_ntok[u] = ntok; s_need[u] = need;
        }
        __syncthreads();
    }
    if (wg == 0) {
        for (int u = 0; u < CU; ++u) {
            const int b = u0 + u;
            if (b >= a.B) continue;
            const int ntok = s_ntok[u] < a.max_tok ? s_ntok[u] : a.max_tok;
            if (tid == 0) a.counts[b] = ntok;
            for (int i = ntok + tid; i < a.max_tok; i += CNT) a.tokens[(size_t)b * a.max_tok + i] = 0;
        }
    }
}

template <int CW, int CU, int CKF>
struct ClusterShape {
    static GreedyLayout layout(const EcRnntConfig& c, int batch, int t_out) { return greedy_layout(c, batch, t_out, CW, CU, CKF); }
    static size_t lds_bytes(int H, int J) { const int HU = H / CW; return (size_t)(CU * H + CU * J + CU * CKF * J + CU * HU + CU * 4 * HU + CU * CKF * 16) * 4; }
    static bool supported(const EcRnntConfig& c) {
        // 16-blocks of k in groups of CMB; whole 16-row tiles of gate rows; at most 4 gate tiles per wave and one vocabulary tile per wave; the state in LDS
        return c.dim_decoder % (16 * CMB) == 0 && c.dim_joint % (16 * CMB) == 0 && c.dim_decoder % (4 * CW) == 0 && c.dim_joint % CW == 0 &&
               4 * (c.dim_decoder / CW) <= 16 * 8 * 4 && (c.vocab_size + CW - 1) / CW <= 128 && lds_bytes(c.dim_decoder, c.dim_joint) <= 160 * 1024 - 512;
    }
};
using ShapeA = ClusterShape<8, 8, 2>;
using ShapeB = ClusterShape<16, 16, 1>;

// Which kernel decodes `batch` utterances: 0 rnnt_greedy_kernel (one workgroup per utterance), 1 ShapeA, 2 ShapeB - the one decision of effconf_rnnt_greedy, and
// what effconf_rnnt_greedy_route reports.  A cluster shape runs when the config allows it and either it is forced (cluster_decode = 1, every workgroup resident:
// at most 256) or - auto - the batch fills two of its clusters and all its workgroups are resident (by-cluster mapping: at most half of the CUs: two decodes on
// two streams must not starve each other's cluster-mates, a spinning workgroup keeps its CU; by-slice mapping: a cluster is CW CONSECUTIVE workgroups, whatever
// part of a launch is resident consists of whole clusters plus at most one split at the dispatch frontier, so a launch may use every CU).
// cluster_shape = 1 asks for ShapeB first; where ShapeB does not run (config or batch) the decision is cluster_shape = 0's.  A forced ShapeA is returned whatever
// the batch: beyond 256 utterances the launch refuses (no quiet per-utterance decode of a forced cluster decode).
int greedy_route(const EcRnntConfig& c, int cluster_mode, int cluster_shape, int by_slice, int batch) {
    if (cluster_mode == 0 || batch <= 0) return 0;
    auto fits = [&](int cw, int cu) { return batch >= 2 * cu && ((batch + cu - 1) / cu) * cw <= (by_slice ? 256 : 128); };
    if (cluster_shape == 1 && ShapeB::supported(c) && (cluster_mode == 1 ? ((batch + 15) / 16) * 16 <= 256 : fits(16, 16))) return 2;
    if (ShapeA::supported(c) && (cluster_mode == 1 || fits(8, 8))) return 1;
    return 0;
}

using HostT = EcRnntHostT;

// W [N][K] row-major -> float4 image [K/4][N]
std::vector<float> kmajor4(const std::vector<float>& W, int N, int K) {
    std::vector<float> o((size_t)N * K);
    for (int k4 = 0; k4 < K / 4; ++k4)
        for (int n = 0; n < N; ++n)
            for (int e = 0; e < 4; ++e) o[((size_t)k4 * N + n) * 4 + e] = W[(size_t)n * K + 4 * k4 + e];
    return o;
}

}  // namespace

extern "C" {

EcRnnt* effconf_rnnt_create(const EcRnntConfig* c) {
    if (!c) { ec_fail("null config"); return nullptr; }
    if (c->num_layers != 1) { ec_fail("RnnDecoder with num_layers == 1 is native (every shipped Transducer config)"); return nullptr; }
    if (c->joint_mode != 0 || c->joint_act != 0) { ec_fail("joint network: 'sum' + 'tanh' is native (every shipped Transducer config)"); return nullptr; }
    if (c->dim_encoder % 4 || c->dim_decoder % 4 || c->dim_joint % 4 || c->dim_encoder < 4 || c->dim_decoder < 4 || c->dim_joint < 4 ||
        c->vocab_size < 2 || c->max_consec_dec_step < 0) { ec_fail("dims must be positive multiples of 4"); return nullptr; }
    EcRnnt* r = new EcRnnt();
    r->cfg = *c;
    return r;
}

void effconf_rnnt_destroy(EcRnnt* r) {
    if (!r) return;
    r->allocs.free_all();
    delete r;
}

int effconf_rnnt_load_tensor(EcRnnt* r, const char* key, const float* host, const int64_t* shape, int32_t ndim) {
    if (!r || !key || !host) return ec_fail("null argument");
    host_tensor_put(r->host, key, host, shape, ndim);
    r->finalized = false;
    return 0;
}

int effconf_rnnt_finalize(EcRnnt* r) {
    if (!r) return ec_fail("null handle");
    r->allocs.free_all();
    const int H = r->cfg.dim_decoder, J = r->cfg.dim_joint, V = r->cfg.vocab_size, De = r->cfg.dim_encoder;
    std::string err;
    const HostT* emb = need(r->host, "decoder.embedding.weight", {V, H}, err);
    const HostT* wih = need(r->host, "decoder.rnn.weight_ih_l0", {4 * H, H}, err);
    const HostT* whh = need(r->host, "decoder.rnn.weight_hh_l0", {4 * H, H}, err);
    const HostT* bih = need(r->host, "decoder.rnn.bias_ih_l0", {4 * H}, err);
    const HostT* bhh = need(r->host, "decoder.rnn.bias_hh_l0", {4 * H}, err);
    const HostT* we = need(r->host, "joint_network.linear_encoder.weight", {J, De}, err);
    const HostT* be = need(r->host, "joint_network.linear_encoder.bias", {J}, err);
    const HostT* wd = need(r->host, "joint_network.linear_decoder.weight", {J, H}, err);
    const HostT* bd = need(r->host, "joint_network.linear_decoder.bias", {J}, err);
    const HostT* wj = need(r->host, "joint_network.linear_joint.weight", {V, J}, err);
    const HostT* bj = need(r->host, "joint_network.linear_joint.bias", {V}, err);
    if (!emb || !wih || !whh || !bih || !bhh || !we || !be || !wd || !bd || !wj || !bj) return ec_fail(err.c_str());
    std::vector<float> bsum(4 * H);
    for (int i = 0; i < 4 * H; ++i) bsum[i] = bih->data[i] + bhh->data[i];
    const std::vector<float> whh4 = kmajor4(whh->data, 4 * H, H), wd4 = kmajor4(wd->data, J, H), wj4 = kmajor4(wj->data, V, J);
    float* d_emb = (float*)r->allocs.upload(emb->data.data(), emb->data.size() * 4);
    float* d_wih = (float*)r->allocs.upload(wih->data.data(), wih->data.size() * 4);
    float* d_bsum = (float*)r->allocs.upload(bsum.data(), bsum.size() * 4);
    float* d_gin = (float*)r->allocs.upload(nullptr, (size_t)V * 4 * H * 4);
    r->dev.whh4 = (const float4*)r->allocs.upload(whh4.data(), whh4.size() * 4);
    r->dev.wd4 = (const float4*)r->allocs.upload(wd4.data(), wd4.size() * 4);
    r->dev.bd = (const float*)r->allocs.upload(bd->data.data(), bd->data.size() * 4);
    r->dev.wj4 = (const float4*)r->allocs.upload(wj4.data(), wj4.size() * 4);
    r->dev.bj = (const float*)r->allocs.upload(bj->data.data(), bj->data.size() * 4);
    r->dev.whh16 = r->dev.wd16 = r->dev.wj16 = nullptr;
    if (ShapeA::supported(r->cfg) || ShapeB::supported(r->cfg) || beam_dims_supported(r->cfg)) {
        const std::vector<float> a16 = kperm16(whh->data, 4 * H, H), b16 = kperm16(wd->data, J, H), c16 = kperm16(wj->data, V, J);
        r->dev.whh16 = (const float4*)r->allocs.upload(a16.data(), a16.size() * 4);
        r->dev.wd16 = (const float4*)r->allocs.upload(b16.data(), b16.size() * 4);
        r->dev.wj16 = (const float4*)r->allocs.upload(c16.data(), c16.size() * 4);
        if (!r->dev.whh16 || !r->dev.wd16 || !r->dev.wj16) return ec_fail("device allocation / upload failed");
    }
    r->we = (float*)r->allocs.upload(we->data.data(), we->data.size() * 4);
    r->be = (float*)r->allocs.upload(be->data.data(), be->data.size() * 4);
    r->wd = (float*)r->allocs.upload(wd->data.data(), wd->data.size() * 4);
    if (!d_emb || !d_wih || !d_bsum || !d_gin || !r->dev.whh4 || !r->dev.wd4 || !r->dev.bd || !r->dev.wj4 || !r->dev.bj || !r->we || !r->be || !r->wd)
        return ec_fail("device allocation / upload failed");
    // Gin[y] = W_ih emb[y] + (b_ih + b_hh)   for every token id (Embedding rows are the only LSTM inputs, decoders.py:55)
    if (launch_sgemm_nt(d_emb, H, d_wih, H, d_bsum, d_gin, 4 * H, V, 4 * H, H, nullptr) != 0) return ec_fail("Gin GEMM launch failed");
    if (hipDeviceSynchronize() != hipSuccess) return ec_fail("Gin GEMM failed");
    r->dev.gin = d_gin;
    r->dev.H = H; r->dev.J = J; r->dev.V = V; r->dev.max_consec = r->cfg.max_consec_dec_step;
    r->finalized = true;
    return 0;
}

size_t effconf_rnnt_workspace_bytes(const EcRnnt* r, int32_t batch, int32_t t_out) {
    if (!r || batch < 0 || t_out < 0) return 0;
    return std::max(ShapeA::layout(r->cfg, batch, t_out).total, ShapeB::layout(r->cfg, batch, t_out).total);     // whichever decode runs: fe is the first region of both
}

int effconf_rnnt_set_option(EcRnnt* r, const char* name, int32_t value) {
    if (!r || !name) return ec_fail("null argument");
    if (!strcmp(name, "cluster_decode")) { r->cluster_mode = value; return 0; }
    if (!strcmp(name, "cluster_by_slice")) { r->cluster_by_slice = value != 0; return 0; }
    if (!strcmp(name, "cluster_shape")) {
        if (value < -1 || value > 1) return ec_fail("cluster_shape must be -1 (default), 0 or 1");
        r->cluster_shape = value;
        return 0;
    }
    if (!strcmp(name, "beam_eval_batch")) {
        if (value < 1 || value > 16) return ec_fail("beam_eval_batch must be 1 .. 16");
        r->beam_eval_batch = value;
        return 0;
    }
    return ec_fail("unknown option");
}

int effconf_rnnt_greedy_route(const EcRnnt* r, int32_t batch) {
    if (!r) return ec_fail("null handle");
    return greedy_route(r->cfg, r->cluster_mode, r->cluster_shape, r->cluster_by_slice, batch);
}

int32_t effconf_rnnt_max_tokens(const EcRnnt* r, int32_t t_out) {
    if (!r || t_out < 0) return 0;
    const int m = r->cfg.max_consec_dec_step * t_out;
    return m > 1 ? m : 1;
}

int effconf_rnnt_greedy(EcRnnt* r, const float* enc_out, const int64_t* out_len, int32_t batch, int32_t t_out,
                        int32_t* tokens, int32_t* token_len, int32_t max_tokens, void* workspace, size_t workspace_bytes, void* stream) {
    if (!r || !r->finalized) return ec_fail("rnnt handle not finalized");
    if (batch == 0) return 0;
    if (!enc_out || !out_len || !tokens || !token_len || !workspace) return ec_fail("null argument");
    if (batch < 0 || t_out <= 0 || max_tokens < effconf_rnnt_max_tokens(r, t_out)) return ec_fail("bad shape / token buffer smaller than max_consec_dec_step * T_out");
    if (workspace_bytes < effconf_rnnt_workspace_bytes(r, batch, t_out)) return ec_fail("workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int H = r->cfg.dim_decoder, J = r->cfg.dim_joint, De = r->cfg.dim_encoder;
    char* ws = WsPlan::base(workspace);
    float* fe = reinterpret_cast<float*>(ws + ShapeA::layout(r->cfg, batch, t_out).fe);
    // linear_encoder(f) for every frame of the batch, once (joint_networks.py:82 recomputes it per decision)
    if (launch_sgemm_nt(enc_out, De, r->we, De, r->be, fe, J, batch * t_out, J, De, s) != 0) return ec_fail("linear_encoder GEMM launch failed");
    auto run_cluster = [&](auto shape, auto cw_c, auto cu_c, auto ckf_c) -> int {
        using Shape = decltype(shape);
        constexpr int CW = decltype(cw_c)::value, CU = decltype(cu_c)::value, CKF = decltype(ckf_c)::value;
        const GreedyLayout L = Shape::layout(r->cfg, batch, t_out);
        const int ncl = L.ncl;
        if (ncl * CW > 256) return ec_fail("cluster decode needs every workgroup resident: batch <= 256");
        ClusterArgs a{};
        a.w = r->dev; a.fe = fe; a.lens = out_len; a.T = t_out; a.B = batch; a.tokens = tokens; a.counts = token_len; a.max_tok = max_tokens;
        a.ncl = ncl; a.by_slice = r->cluster_by_slice;
        a.cnt = reinterpret_cast<unsigned*>(ws + L.sync); a.status = reinterpret_cast<int*>(ws + L.status);
        a.xh = reinterpret_cast<float*>(ws + L.xh);
        a.xgd = reinterpret_cast<float*>(ws + L.xgd);
        a.xav = reinterpret_cast<float*>(ws + L.xav);
        a.xai = reinterpret_cast<int*>(ws + L.xai);
        if (hipMemsetAsync(ws + L.sync, 0, L.sync_bytes, s) != hipSuccess) return ec_fail("memset failed");
        const size_t lds = Shape::lds_bytes(H, J);
        static LdsAttr attr;
        ensure_dynamic_lds(reinterpret_cast<const void*>(&rnnt_cluster_kernel<CW, CU, CKF>), (int)lds, attr);
        hipLaunchKernelGGL((rnnt_cluster_kernel<CW, CU, CKF>), dim3(ncl * CW), dim3(CNT), lds, s, a);
        return hipGetLastError() == hipSuccess ? 0 : ec_fail("rnnt cluster launch failed");
    };
    const int route = greedy_route(r->cfg, r->cluster_mode, r->cluster_shape, r->cluster_by_slice, batch);
    if (route == 2) return run_cluster(ShapeB{}, std::integral_constant<int, 16>{}, std::integral_constant<int, 16>{}, std::integral_constant<int, 1>{});
    if (route == 1) return run_cluster(ShapeA{}, std::integral_constant<int, 8>{}, std::integral_constant<int, 8>{}, std::integral_constant<int, 2>{});
    const size_t lds = (size_t)(2 * H + 4 * H + J + KF * J + 2 * KF * (NT / 64)) * 4;
    hipLaunchKernelGGL(rnnt_greedy_kernel, dim3(batch), dim3(NT), lds, s, r->dev, fe, out_len, t_out, tokens, token_len, max_tokens);
    return hipGetLastError() == hipSuccess ? 0 : ec_fail("rnnt_greedy launch failed");
}

// ---- the greedy decode resumed per stream (include/effconf.h)
size_t effconf_rnnt_stream_state_bytes(const EcRnnt* r, int32_t max_streams) {
    if (!r) { ec_fail("null handle"); return 0; }
    if (max_streams < 1) { ec_fail("max_streams must be >= 1"); return 0; }
    return rnnt_stream_layout(r->cfg, max_streams).total;
}

int effconf_rnnt_stream_init(EcRnnt* r, void* state, size_t state_bytes, int32_t max_streams, void* stream) {
    if (!r) return ec_fail("null handle");
    if (!state) return ec_fail("null argument");
    if (max_streams < 1) return ec_fail("max_streams must be >= 1");
    const RnntStreamLayout L = rnnt_stream_layout(r->cfg, max_streams);
    if (state_bytes < L.total) return ec_fail("stream state buffer too small (effconf_rnnt_stream_state_bytes)");
    // the flags alone: a record whose flag is clear is never read
    if (hipMemsetAsync(WsPlan::base(state) + L.primed, 0, (size_t)max_streams * 4, (hipStream_t)stream) != hipSuccess) return ec_fail("memset failed");
    return 0;
}

int effconf_rnnt_stream_reset(EcRnnt* r, void* state, int32_t max_streams, int32_t stream_id, void* stream) {
    if (!r) return ec_fail("null handle");
    if (!state) return ec_fail("null argument");
    if (max_streams < 1 || stream_id < 0 || stream_id >= max_streams) return ec_fail("stream id outside 0 .. max_streams - 1");
    const RnntStreamLayout L = rnnt_stream_layout(r->cfg, max_streams);
    if (hipMemsetAsync(WsPlan::base(state) + L.primed + (size_t)stream_id * 4, 0, 4, (hipStream_t)stream) != hipSuccess) return ec_fail("memset failed");
    return 0;
}

size_t effconf_rnnt_stream_workspace_bytes(const EcRnnt* r, int32_t n, int32_t t_new) {
    if (!r) { ec_fail("null handle"); return 0; }
    if (n < 0 || t_new <= 0) { ec_fail("n must be >= 0 and t_new > 0"); return 0; }
    return rnnt_stream_ws(r->cfg, n, t_new).total;
}

int effconf_rnnt_greedy_resume(EcRnnt* r, void* state, int32_t max_streams, const int32_t* streams, const float* enc_out, const int64_t* out_len,
                               int32_t n, int32_t t_new, int32_t* tokens, int32_t* token_frames, int32_t* token_len, int32_t* decoder_steps,
                               int32_t max_tokens, void* workspace, size_t workspace_bytes, void* stream) {
    if (!r || !r->finalized) return ec_fail("rnnt handle not finalized");
    if (n < 0 || t_new <= 0 || max_streams < 1) return ec_fail("bad shape: n >= 0, t_new > 0, max_streams >= 1");
    if (max_tokens < effconf_rnnt_max_tokens(r, t_new)) return ec_fail("token buffer smaller than max_consec_dec_step * t_new");
    if (workspace_bytes < rnnt_stream_ws(r->cfg, n, t_new).total) return ec_fail("workspace too small");
    if (n == 0) return 0;
    if (!state || !streams || !enc_out || !out_len || !tokens || !token_len || !workspace) return ec_fail("null argument");
    hipStream_t s = (hipStream_t)stream;
    const int H = r->cfg.dim_decoder, J = r->cfg.dim_joint, De = r->cfg.dim_encoder;
    float* fe = reinterpret_cast<float*>(WsPlan::base(workspace) + rnnt_stream_ws(r->cfg, n, t_new).fe);
    // rows are independent: a frame's fe is bit-identical however the frames are grouped into pushes
    if (launch_sgemm_nt(enc_out, De, r->we, De, r->be, fe, J, n * t_new, J, De, s) != 0) return ec_fail("linear_encoder GEMM launch failed");
    const RnntStreamLayout L = rnnt_stream_layout(r->cfg, max_streams);
    char* st = WsPlan::base(state);
    StreamIo io{};
    io.streams = streams; io.primed = reinterpret_cast<int*>(st + L.primed); io.rec = reinterpret_cast<float*>(st + L.rec);
    io.rec_floats = (int)(L.rec_bytes / 4); io.max_streams = max_streams; io.token_frames = token_frames; io.decoder_steps = decoder_steps;
    const size_t lds = (size_t)(2 * H + 4 * H + J + KF * J + 2 * KF * (NT / 64)) * 4;
    hipLaunchKernelGGL(rnnt_greedy_resume_kernel, dim3(n), dim3(NT), lds, s, r->dev, fe, out_len, t_new, tokens, token_len, max_tokens, io);
    return hipGetLastError() == hipSuccess ? 0 : ec_fail("rnnt_greedy_resume launch failed");
}

}  // extern "C"
