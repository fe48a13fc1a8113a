// RNN-T lattice dynamic programs (gfx950): from the two planes of rnnt_lattice.hip, lp_blank[t][u] and lp_label[t][u] (t < T, u <= U),
//   forward:  a[t][u] = logaddexp(a[t-1][u] + lp_blank[t-1][u], a[t][u-1] + lp_label[t][u-1]),  a[0][0] = 0
//             log_likelihood = a[T-1][U] + lp_blank[T-1][U]                      (= -rnnt_loss of the planes)
//   Viterbi:  the same recursion with max; the label move (from (t, u-1)) is taken only when STRICTLY greater, equality takes the blank
//             (time) move from (t-1, u);  score = v[T-1][U] + lp_blank[T-1][U], the best path's log-probability with every blank.
// One workgroup per utterance runs the anti-diagonals d = t + u: thread u owns column u and is at frame t = d - u.  The value from (t-1, u)
// is the thread's own previous one (a register), the value from (t, u-1) its left neighbour's of the previous diagonal (LDS, double
// buffered: one barrier per diagonal); the two plane entries of the next diagonal are loaded under the current one's arithmetic.
// Back-pointers: one bit per cell (1 = label move), packed per THREAD - thread u fills a 32-bit word over 32 frames and writes it to
// bp[u][t / 32] - so no two threads share a word; they live in the workspace.  One thread traces back from (T-1, U):
// token_frame[u] = the frame at which token u is emitted, token_logp[u] = lp_label there.
// VIT = false (score NULL): the forward half alone, no v, no back-pointers; log_likelihood is bit-identical.
// Every value of an utterance is computed by the same instructions in the same order whatever the batch and the T / U padding.
#include "decode_common.h"

#include <cmath>

int ec_fail(const char* msg);

using namespace ecrnnt;
using namespace ecdec;

namespace {

constexpr int MAXU = 1023;

const char* rnnt_align_check(int32_t batch, int32_t t_out, int32_t u_max) {
    if (u_max < 0 || u_max > MAXU) return "rnnt align: u_max must be in 0 .. 1023";
    if (batch < 0 || t_out < 0) return "rnnt align: bad shape";
    if ((int64_t)batch * t_out * (u_max + 1) >= (1ll << 31)) return "rnnt align: batch * t_out * (u_max + 1) must be below 2^31";
    return nullptr;
}

struct RnntAlignArgs {
    const float* lpb; const float* lpl; const int64_t* lens; const int64_t* target_len;
    int T, umax, E, wpu;
    unsigned* bp; size_t bp_utt;
    float* ll; float* score; int* token_frame; float* token_logp; int* status;
};

// logaddexp in the logf form of the RNN-T loss this kernel follows; ctc_align.hip's lse3 is its three-way sibling, ctc_beam.hip's lse a different formula
// (log1pf, after the CTC beam search's reference): three functions on purpose
__device__ __forceinline__ float lse2(float p, float q) {
    const float m = fmaxf(p, q);
    const float ms = m == -INFINITY ? 0.f : m;
    const float v = ms + logf(expf(p - ms) + expf(q - ms));
    return m == -INFINITY ? -INFINITY : v;
}

template <bool VIT>
__global__ __launch_bounds__(1024) void rnnt_dp_kernel(const RnntAlignArgs a) {
    __shared__ float sA[2][MAXU + 1], sV[2][MAXU + 1];
    const int tid = threadIdx.x, b = blockIdx.x, E = a.E;
    const int T = clamp_len(a.lens[b], a.T);
    int st = a.status[b];                            // the lattice's verdict on the tokens; the length is checked again
    if (transcript_status(a.target_len[b], a.umax, nullptr, 0)) st = 2;
    const int U = st == 2 ? 0 : (int)a.target_len[b];
    if (st == 0 && T == 0 && U > 0) st = 1;
    const bool run = st == 0 && T > 0;
    const float* lpb = a.lpb + (size_t)b * a.T * E;
    const float* lpl = a.lpl + (size_t)b * a.T * E;
    unsigned* bp = VIT ? reinterpret_cast<unsigned*>(reinterpret_cast<char*>(a.bp) + (size_t)b * a.bp_utt) : nullptr;

    if (VIT) {                                       // rows past U_b (and every row of an utterance that is not aligned): -1 / 0
        for (int u = tid; u < a.umax; u += blockDim.x) {
            if (a.token_frame) a.token_frame[(size_t)b * a.umax + u] = -1;
            if (a.token_logp) a.token_logp[(size_t)b * a.umax + u] = 0.f;
        }
    }
    float ll = st == 0 ? 0.f : -INFINITY, sc = ll;  // no frames and no tokens: the empty path
    if (run) {
        const int u = tid;
        const bool col = u <= U;
        float av = -INFINITY, vv = -INFINITY;        // a / v of (t - 1, u): the thread's previous cell
        unsigned bits = 0u;
        // the plane entries of diagonal 0: only (0, 0), which has no predecessor
        float nb = 0.f, nl = 0.f;
        const int D = T + U;                         // diagonals 0 .. T - 1 + U
        for (int d = 0; d < D; ++d) {
            const int t = d - u;
            const bool on = col && t >= 0 && t < T;
            const float eb = nb, el = nl;
            {                                        // diagonal d + 1: (t + 1, u) is entered from (t, u) by a blank and from (t + 1, u - 1) by a label
                const int t1 = t + 1;
                const bool on1 = col && t1 >= 0 && t1 < T;
                nb = on1 && t1 > 0 ? lpb[(size_t)(t1 - 1) * E + u] : 0.f;
                nl = on1 && u > 0 ? lpl[(size_t)t1 * E + u - 1] : 0.f;
            }
            if (on) {
                const float* Ap = sA[(d + 1) & 1];
                const float pa = t > 0 ? av + eb : -INFINITY;
                const float qa = u > 0 ? Ap[u - 1] + el : -INFINITY;
                av = d == 0 ? 0.f : lse2(pa, qa);
                sA[d & 1][u] = av;
                if (VIT) {
                    const float* Vp = sV[(d + 1) & 1];
                    const float pv = t > 0 ? vv + eb : -INFINITY;
                    const float qv = u > 0 ? Vp[u - 1] + el : -INFINITY;
                    const bool lab = qv > pv;
                    vv = d == 0 ? 0.f : (lab ? qv : pv);
                    sV[d & 1][u] = vv;
                    bits |= (lab ? 1u : 0u) << (t & 31);
                    if ((t & 31) == 31 || t == T - 1) { bp[(size_t)u * a.wpu + (t >> 5)] = bits; bits = 0u; }
                }
            }
            __syncthreads();
        }
        // ---- the end (T - 1, U): thread U's last cell
        if (u == U) {
            const float last = lpb[(size_t)(T - 1) * E + U];
            sA[0][0] = av + last;
            if (VIT) sV[0][0] = vv + last;
        }
        __syncthreads();
        ll = sA[0][0];
        if (VIT) sc = sV[0][0];
        if (VIT && tid == 0) {
            int t = T - 1, uu = U;
            while (t > 0 || uu > 0) {
                const bool lab = uu > 0 && (t == 0 || ((bp[(size_t)uu * a.wpu + (t >> 5)] >> (t & 31)) & 1u));
                if (lab) {
                    --uu;
                    if (a.token_frame) a.token_frame[(size_t)b * a.umax + uu] = t;
                    if (a.token_logp) a.token_logp[(size_t)b * a.umax + uu] = lpl[(size_t)t * E + uu];
                } else {
                    --t;
                }
            }
        }
    }
    if (tid == 0) {
        a.ll[b] = ll;
        a.status[b] = st;
        if (VIT) a.score[b] = sc;
    }
}

}  // namespace

extern "C" {

size_t effconf_rnnt_align_workspace_bytes(int32_t batch, int32_t t_out, int32_t u_max) {
    if (const char* e = rnnt_align_check(batch, t_out, u_max)) { ec_fail(e); return 0; }
    return rnnt_align_layout(batch, t_out, u_max).total;
}

int effconf_rnnt_align(const float* lp_blank, const float* lp_label, const int64_t* out_len, const int64_t* target_len, int32_t batch,
                       int32_t t_out, int32_t u_max, float* log_likelihood, float* score, int32_t* token_frame, float* token_logp,
                       int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (const char* e = rnnt_align_check(batch, t_out, u_max)) return ec_fail(e);
    if (batch == 0) return 0;
    if (!out_len || !target_len || !log_likelihood || !status || !workspace || (t_out > 0 && (!lp_blank || !lp_label))) return ec_fail("null argument");
    if (!score && (token_frame || token_logp)) return ec_fail("null argument");
    const RnntAlignLayout L = rnnt_align_layout(batch, t_out, u_max);
    if (workspace_bytes < L.total) return ec_fail("workspace too small (effconf_rnnt_align_workspace_bytes)");
    char* ws = WsPlan::base(workspace);
    RnntAlignArgs a{};
    a.lpb = lp_blank; a.lpl = lp_label; a.lens = out_len; a.target_len = target_len;
    a.T = t_out; a.umax = u_max; a.E = u_max + 1; a.wpu = L.wpu;
    a.bp = reinterpret_cast<unsigned*>(ws + L.bp); a.bp_utt = L.bp_utt;
    a.ll = log_likelihood; a.score = score; a.token_frame = token_frame; a.token_logp = token_logp; a.status = status;
    const int threads = ((u_max + 1 + 63) / 64) * 64;     // one thread per column of the widest lattice
    hipStream_t s = (hipStream_t)stream;
    if (score) hipLaunchKernelGGL(rnnt_dp_kernel<true>, dim3(batch), dim3(threads), 0, s, a);
    else hipLaunchKernelGGL(rnnt_dp_kernel<false>, dim3(batch), dim3(threads), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : ec_fail("rnnt_dp launch failed");
}

}  // extern "C"
