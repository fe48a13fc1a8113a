// CTC forced alignment and transcript scoring (gfx950): for head logits x (T, V) and a target y (U tokens, blank = 0), the best path
// (Viterbi) and the total probability (CTC forward algorithm) over one trellis of T frames and S = 2 U + 1 states.
//
//   lp[t][c] = x[t][c] / tmp - max_c - log sum_c exp(x[t][c] / tmp - max_c)   (fp32)
// is log_softmax, what the reference's CTC loss (torch.nn.CTCLoss on log_softmax outputs) uses.  It stays finite where the beam kernel's
// softmax().log() (ctc_beam.hip: what ctcdecode is fed) gives -inf, so a target through an improbable token has a finite score here.
// Extended target e[2 u + 1] = y[u], e[even] = 0.  State s at frame t is entered from s, from s - 1, and from s - 2 when s is odd and
// e[s] != e[s - 2].  Start: s in {0, 1} at t = 0 (written as a virtual frame -1 that holds 0 in state 0 and -inf elsewhere: the same
// values, no special first frame).  End: s in {S - 1, S - 2} at t = len - 1.
//   forward:  a[t][s] = lse(a[t-1][s], a[t-1][s-1], a[t-1][s-2]) + lp[t][e[s]],   log_likelihood = lse(a[S-1], a[S-2])
//   Viterbi:  v[t][s] = max(...) + lp[t][e[s]] with the smaller step winning ties (stay, then +1, then +2: strict > in that order);
//             the path ends in S - 1 when v[S-1] >= v[S-2];  score = v of the end state.
// Every value of an utterance is computed by the same instructions in the same order whatever the batch, the T / U padding or the run:
// a state's value does not depend on which thread owns it, and the emission pass assigns columns to lanes by column index alone.
//
// Two kernels.
//   * ctc_emit_kernel: one wave per valid frame row (b, t < len[b]).  Column quad q = 4 q .. 4 q + 3 belongs to lane q % 64, whatever the
//     row's address: a row whose base is 16-byte aligned is read with 16-byte loads, any other row (V % 4 != 0 puts three rows in four off
//     the 16-byte grid) with four dword loads per quad, and the last quad is guarded per element.  (Deviation from "16-byte loads + a
//     scalar head / tail split at the aligned addresses": that split would change the order of the fp32 sum with the row's alignment, i.e.
//     with the utterance's position in the batch.)  Writes only lp[blank] and lp[y[u]], u < U_b: emit[b][t][0 .. U_b].
//   * ctc_trellis_kernel<SPT, VIT>: one persistent workgroup of 256 threads per utterance.  Thread i owns the states i n .. i n + n - 1,
//     n = ceil(S_b / 256) <= SPT (the launch's bound, from u_max).  a and v are double buffered in LDS, one barrier per frame, the next
//     frame's emissions are loaded under the current frame's work.  States at or beyond S_b inside the owned runs are computed like the
//     others (blank emission, no skip) and never read by a valid state - transitions only go up - so the frame loop has no
//     lane-divergent branch: whole waves without a valid state skip the frame's arithmetic (a scalar branch).
//     Backpointers: 2 bits per (t, s), kept per THREAD - ceil(n / 4) bytes per thread and frame, a row of 64 (waves in use) ceil(n / 4)
//     bytes per frame - so that no two threads write one byte (deviation from a dense T S / 4 image, which would need a cross-lane pack
//     or atomics in the frame loop).  They live in LDS when len rows fit beside the state buffers (128 KiB of LDS per workgroup at the
//     most), otherwise in the workspace; the backtrace (one thread) then walks len dependent loads from LDS or, for long utterances,
//     from memory.  A parallel epilogue turns the path into frame_token, the token spans and the per-token sums.
//   VIT = false (all four alignment outputs NULL): the forward half alone, no v, no backpointers; log_likelihood is bit-identical.
#include "decode_common.h"

#include <cmath>

int ec_fail(const char* msg);

using namespace ecrnnt;
using namespace ecdec;

namespace {

constexpr int AT = CTC_ALIGN_THREADS;             // threads per utterance
constexpr int MAXV = 1024;                        // largest vocabulary
constexpr int MAXU = 2047;                        // largest target: S <= 4095 <= 16 states per thread
constexpr int LDS_MAX = 128 * 1024;               // LDS per workgroup at the most (160 KiB per CU)

const char* ctc_align_check(int32_t batch, int32_t t_out, int32_t vocab, int32_t u_max) {
    if (vocab < 2 || vocab > MAXV) return "ctc align: vocab must be in 2 .. 1024";
    if (u_max < 0 || u_max > MAXU) return "ctc align: u_max must be in 0 .. 2047";
    if (batch < 0 || t_out < 0) return "ctc align: bad shape";
    if ((int64_t)batch * t_out >= (1ll << 31)) return "ctc align: batch * t_out too large";
    return nullptr;
}

struct CtcAlignArgs {
    const float* logits; const int64_t* lens; const int* targets; const int64_t* target_len;
    int T, V, umax, E; float tmp;
    float* emit; int* path; unsigned char* bp; size_t bp_utt;
    int lds_bp;                                   // bytes of LDS behind the state buffers
    float* ll; float* score; int* status;
    int* frame_token; int* token_start; int* token_end; float* token_logp;
};

// ---------------------------------------------------------------------------------------------------------------- emissions
__global__ __launch_bounds__(AT) void ctc_emit_kernel(const CtcAlignArgs a, const int rows) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (AT / 64) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int b = r / a.T, t = r - b * a.T, V = a.V;
    if (t >= clamp_len(a.lens[b], a.T)) return;   // the whole wave: rows at or beyond len are never read
    const int U = clamp_len(a.target_len[b], a.umax);
    const float* row = a.logits + (size_t)r * V;
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    float x[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c0 = 4 * (lane + 64 * j);
        if (vec && c0 + 3 < V) {
            const float4 q = *reinterpret_cast<const float4*>(row + c0);
            x[4 * j] = q.x; x[4 * j + 1] = q.y; x[4 * j + 2] = q.z; x[4 * j + 3] = q.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) x[4 * j + i] = c0 + i < V ? row[c0 + i] : 0.f;
        }
    }
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[4 * j + i] = x[4 * j + i] / a.tmp;
            if (4 * (lane + 64 * j) + i < V) m = fmaxf(m, x[4 * j + i]);
        }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) sum += 4 * (lane + 64 * j) + i < V ? expf(x[4 * j + i] - m) : 0.f;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    const float lsum = logf(sum);
    float* out = a.emit + (size_t)r * a.E;
    const int* y = a.targets + (size_t)b * a.umax;
    for (int u = lane; u <= U; u += 64) {          // slot 0: blank, slot 1 + u: y[u]
        const int c = u == 0 ? 0 : y[u - 1];
        out[u] = (c >= 0 && c < V) ? (row[c] / a.tmp - m) - lsum : 0.f;      // an id outside the vocabulary: status 2, the value is not used
    }
}

// ---------------------------------------------------------------------------------------------------------------- trellis
// three-way logaddexp in the logf form of the CTC loss this kernel follows (rnnt_align.hip's lse2 is its two-way sibling); ctc_beam.hip's lse is the log1pf
// form of the prefix beam search: different formulas on purpose
__device__ __forceinline__ float lse3(float p, float q, float r) {
    const float m = fmaxf(fmaxf(p, q), r);
    const float ms = m == -INFINITY ? 0.f : m;
    const float v = ms + logf(expf(p - ms) + expf(q - ms) + expf(r - ms));
    return m == -INFINITY ? -INFINITY : v;
}

template <int SPT, bool VIT>
__global__ __launch_bounds__(AT) void ctc_trellis_kernel(const CtcAlignArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NS = AT * SPT + 2;               // states + the two -inf slots in front of state 0
    float* A0 = reinterpret_cast<float*>(smem);
    float* A1 = A0 + NS;
    float* V0 = A1 + NS;
    float* V1 = V0 + NS;
    unsigned char* lbp = reinterpret_cast<unsigned char*>(V1 + NS);
    __shared__ int s_bad, s_rep;

    const int tid = threadIdx.x, b = blockIdx.x, T = a.T;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int len = clamp_len(a.lens[b], T);
    const int U = clamp_len(a.target_len[b], a.umax);
    const int S = 2 * U + 1;
    const int n = (S + AT - 1) / AT;               // states per thread of THIS utterance, <= SPT
    const int wb = (n + 3) >> 2;                   // backpointer bytes per thread and frame
    const int nwav = (S + 64 * n - 1) / (64 * n);  // waves that own a valid state
    const int rb = nwav * 64 * wb;                 // backpointer bytes per frame
    const int* y = a.targets + (size_t)b * a.umax;
    const float* em = a.emit + (size_t)b * T * a.E;

    if (tid == 0) { s_bad = 0; s_rep = 0; }
    __syncthreads();
    {
        int bad = 0, rep = 0;
        for (int u = tid; u < U; u += AT) {
            const int c = y[u];
            bad |= token_refused(c, a.V);
            rep += (u > 0 && c == y[u - 1]);
        }
        if (bad) atomicOr(&s_bad, 1);
        if (rep) atomicAdd(&s_rep, rep);
    }
    for (int i = tid; i < NS; i += AT) {           // the virtual frame -1: 0 in state 0
        const float v = i == 2 ? 0.f : -INFINITY;
        A0[i] = v; A1[i] = -INFINITY;
        if (VIT) { V0[i] = v; V1[i] = -INFINITY; }
    }
    __syncthreads();
    const int status = s_bad ? 2 : (len < U + s_rep ? 1 : 0);
    const bool run = status == 0;
    unsigned char* bp = nullptr;
    if (VIT) bp = (size_t)len * rb <= (size_t)a.lds_bp ? lbp : a.bp + (size_t)b * a.bp_utt;

    float ll = run ? 0.f : -INFINITY, sc = ll;    // len = 0 (then U = 0): the empty path
    if (run && len > 0) {
        int eidx[SPT];
        bool skip[SPT];
        float nx[SPT];
#pragma unroll
        for (int k = 0; k < SPT; ++k) {
            const int s = tid * n + k;
            const bool tok = k < n && s < S && (s & 1);
            eidx[k] = tok ? 1 + (s >> 1) : 0;
            skip[k] = tok && s >= 3 && y[s >> 1] != y[(s >> 1) - 1];
            nx[k] = k < n ? em[eidx[k]] : 0.f;
        }
        const bool active = wave < nwav;
        float* Ap = A0; float* Ac = A1; float* Vp = V0; float* Vc = V1;
        for (int t = 0; t < len; ++t) {
            float e[SPT];
#pragma unroll
            for (int k = 0; k < SPT; ++k) e[k] = nx[k];
            if (t + 1 < len) {                     // the next frame's emissions under this frame's work
#pragma unroll
                for (int k = 0; k < SPT; ++k)
                    if (k < n) nx[k] = em[(size_t)(t + 1) * a.E + eidx[k]];
            }
            if (active) {
                unsigned bits = 0u;
#pragma unroll
                for (int k = 0; k < SPT; ++k) {
                    if (k < n) {
                        const int i = tid * n + k + 2;
                        Ac[i] = lse3(Ap[i], Ap[i - 1], skip[k] ? Ap[i - 2] : -INFINITY) + e[k];
                        if (VIT) {
                            float best = Vp[i];
                            unsigned st = 0u;
                            const float v1 = Vp[i - 1], v2 = skip[k] ? Vp[i - 2] : -INFINITY;
                            if (v1 > best) { best = v1; st = 1u; }
                            if (v2 > best) { best = v2; st = 2u; }
                            Vc[i] = best + e[k];
                            bits |= st << (2 * k);
                        }
                    }
                }
                if (VIT) {
                    unsigned char* p = bp + (size_t)t * rb + tid * wb;
#pragma unroll
                    for (int j = 0; j < (SPT + 3) / 4; ++j)
                        if (j < wb) p[j] = (unsigned char)(bits >> (8 * j));
                }
            }
            __syncthreads();
            float* x = Ap; Ap = Ac; Ac = x;
            x = Vp; Vp = Vc; Vc = x;
        }
        // ---- the ends (S - 1 and S - 2), then the backtrace
        ll = lse3(Ap[S + 1], S >= 2 ? Ap[S] : -INFINITY, -INFINITY);
        if (VIT) {
            int s = S - 1;
            if (S >= 2 && Vp[S] > Vp[S + 1]) s = S - 2;
            sc = Vp[s + 2];
            if (tid == 0) {
                int* path = a.path + (size_t)b * T;
                for (int t = len - 1; t >= 0; --t) {
                    path[t] = s;
                    const int own = s / n, k = s - own * n;
                    s -= (bp[(size_t)t * rb + own * wb + (k >> 2)] >> (2 * (k & 3))) & 3;
                }
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        a.ll[b] = ll;
        a.status[b] = status;
        if (VIT && a.score) a.score[b] = sc;
    }
    if (!VIT) return;
    // ---- epilogue: frame_token, the token spans (the runs of the path) and the per-token sums
    const int* path = a.path + (size_t)b * T;
    int* sstart = reinterpret_cast<int*>(V0);       // the state buffers are free now
    int* send = reinterpret_cast<int*>(V1);
    for (int u = tid; u < U; u += AT) { sstart[u] = -1; send[u] = -1; }     // a token no frame carries (NaN logits): an empty span
    __syncthreads();
    for (int t = tid; t < T; t += AT) {
        const bool in = run && t < len;
        const int s = in ? path[t] : 0;
        if (a.frame_token) a.frame_token[(size_t)b * T + t] = (s & 1) ? (s >> 1) : -1;
        if (s & 1) {
            if (t == 0 || path[t - 1] != s) sstart[s >> 1] = t;
            if (t == len - 1 || path[t + 1] != s) send[s >> 1] = t + 1;
        }
    }
    __syncthreads();
    for (int u = tid; u < a.umax; u += AT) {
        const bool in = run && u < U;
        const int t0 = in ? sstart[u] : -1, t1 = in ? send[u] : -1;
        float w = 0.f;
        for (int t = t0; t < t1; ++t) w += em[(size_t)t * a.E + 1 + u];
        const size_t o = (size_t)b * a.umax + u;
        if (a.token_start) a.token_start[o] = t0;
        if (a.token_end) a.token_end[o] = t1;
        if (a.token_logp) a.token_logp[o] = w;
    }
}

template <int SPT, bool VIT>
int launch_trellis(const CtcAlignArgs& a, int batch, int lds, hipStream_t s) {
    static LdsAttr attr;
    ensure_dynamic_lds(reinterpret_cast<const void*>(&ctc_trellis_kernel<SPT, VIT>), lds, attr);
    hipLaunchKernelGGL((ctc_trellis_kernel<SPT, VIT>), dim3(batch), dim3(AT), lds, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <bool VIT>
int launch_trellis_spt(int spt, const CtcAlignArgs& a, int batch, int lds, hipStream_t s) {
    switch (spt) {
        case 1: return launch_trellis<1, VIT>(a, batch, lds, s);
        case 2: return launch_trellis<2, VIT>(a, batch, lds, s);
        case 4: return launch_trellis<4, VIT>(a, batch, lds, s);
        case 8: return launch_trellis<8, VIT>(a, batch, lds, s);
        default: return launch_trellis<16, VIT>(a, batch, lds, s);
    }
}

}  // namespace

extern "C" {

size_t effconf_ctc_align_workspace_bytes(int32_t batch, int32_t t_out, int32_t vocab, int32_t u_max) {
    if (const char* e = ctc_align_check(batch, t_out, vocab, u_max)) { ec_fail(e); return 0; }
    return ctc_align_layout(batch, t_out, u_max).total;
}

int effconf_ctc_align(const float* logits, const int64_t* out_len, int32_t batch, int32_t t_out, int32_t vocab, const int32_t* targets,
                      const int64_t* target_len, int32_t u_max, float temperature, float* log_likelihood, float* score, int32_t* status,
                      int32_t* frame_token, int32_t* token_start, int32_t* token_end, float* token_logp, void* workspace,
                      size_t workspace_bytes, void* stream) {
    if (const char* e = ctc_align_check(batch, t_out, vocab, u_max)) return ec_fail(e);
    if (!(temperature > 0.f) || !std::isfinite(temperature)) return ec_fail("ctc align: temperature must be > 0");
    if (batch == 0) return 0;
    if (!out_len || !target_len || !log_likelihood || !status || !workspace || (t_out > 0 && !logits) || (u_max > 0 && !targets))
        return ec_fail("null argument");
    const CtcAlignLayout L = ctc_align_layout(batch, t_out, u_max);
    if (workspace_bytes < L.total) return ec_fail("workspace too small (effconf_ctc_align_workspace_bytes)");
    char* ws = WsPlan::base(workspace);
    const bool vit = frame_token || token_start || token_end || token_logp;
    if (vit && !score) return ec_fail("null argument");
    CtcAlignArgs a{};
    a.logits = logits; a.lens = out_len; a.targets = targets; a.target_len = target_len;
    a.T = t_out; a.V = vocab; a.umax = u_max; a.E = L.E; a.tmp = temperature;
    a.emit = reinterpret_cast<float*>(ws + L.emit); a.path = reinterpret_cast<int*>(ws + L.path);
    a.bp = reinterpret_cast<unsigned char*>(ws + L.bp); a.bp_utt = L.bp_utt;
    a.ll = log_likelihood; a.score = score; a.status = status;
    a.frame_token = frame_token; a.token_start = token_start; a.token_end = token_end; a.token_logp = token_logp;
    const int states = 4 * (AT * L.spt + 2) * 4;
    const size_t want = vit ? (size_t)t_out * L.rbmax : 0;
    a.lds_bp = (int)(want < (size_t)(LDS_MAX - states) ? want : (size_t)(LDS_MAX - states));
    const int lds = (states + a.lds_bp + 15) & ~15;
    hipStream_t s = (hipStream_t)stream;
    const int rows = batch * t_out;
    if (rows > 0) {
        hipLaunchKernelGGL(ctc_emit_kernel, dim3((rows + AT / 64 - 1) / (AT / 64)), dim3(AT), 0, s, a, rows);
        if (hipGetLastError() != hipSuccess) return ec_fail("ctc_emit launch failed");
    }
    const int rc = vit ? launch_trellis_spt<true>(L.spt, a, batch, lds, s) : launch_trellis_spt<false>(L.spt, a, batch, lds, s);
    return rc == 0 ? 0 : ec_fail("ctc_trellis launch failed");
}

}  // extern "C"
