// CTC prefix beam search (gfx950): ModelCTC.beam_search_decoding of the reference (models/model_ctc.py:138-181), i.e. ctcdecode's
// CTCBeamDecoder with blank 0, cutoff_top_n = V and cutoff_prob 1 (nothing pruned by probability), without the n-gram scorer.
//
// A prefix is a token string without blanks with pb / pnb = log P(ending in blank / in a non-blank); its score is s = lse(pb, pnb).
// Per frame, with lp = (logits / tmp).softmax().log() (fp32; -inf where the fp32 probability is 0), every beam member P gives
//   b'(P) = lp[0] + s(P),  nb'(P) = lp[last(P)] + pnb(P) (P != empty)  and for c != 0, Q = P c:  nb'(Q) += lp[c] + (c == last(P) ? pb(P) : s(P)),
// with += a log-sum-exp.  The best `beam` candidates survive, ordered by score desc, then last token asc (empty prefix = -1), then the
// canonical index (members in rank order, then the extensions by (parent rank, token)).
//
// ONE persistent workgroup runs one utterance, frame after frame; the next frame's logits are loaded under the current frame's work.
//   * Exact pruning: of a member's plain extensions (c not blank, not last(P), P c not a member) only its best `beam` can survive, and they
//     lie among the frame's K = 2 beam + 1 most probable tokens (at most beam + 1 tokens are not plain).  K is found by a radix select
//     over the 32-bit order keys of lp (4 histogram passes in LDS), then ordered by (lp desc, id asc).  So a frame has at most
//     beam (members) + beam (repeat extensions) + beam * beam (plain extensions) candidates; merges into members are added to the members.
//   * Selection: the rank of a candidate is the number of candidates that come before it (total order, so ranks are unique), one
//     64-bit compare per pair of packed (score, last token, canonical index) keys.
//   * Prefix identity is string identity: an append-only trie of (parent node, token) in the workspace with a (parent, token) -> node hash
//     index, so a prefix that leaves the beam and comes back gets its old node, and "P c is a member" is a compare of (parent, token).
// All arithmetic of an utterance is in a fixed order, so its results do not depend on the batch, the T padding or the run.
#include "decode_common.h"

#include <cmath>

int ec_fail(const char* msg);

using namespace ecdec;

namespace {

constexpr int CT = 256;                           // threads per utterance
constexpr int CNW = CT / 64;                      // waves
constexpr int MAXB = 32;                          // largest beam
constexpr int MAXV = 1024;                        // largest vocabulary
constexpr int TPT = MAXV / CT;                    // tokens per thread (contiguous: thread i owns i TPT .. i TPT + TPT - 1)
constexpr int MAXK = 2 * MAXB + 1;                // top tokens per frame
constexpr int MAXS = 2 * MAXB + MAXB * MAXB;      // candidate slots: members, repeat extensions, plain extensions
constexpr unsigned long long HEMPTY = ~0ull;

const char* ctc_beam_check(int32_t batch, int32_t t_out, int32_t vocab, int32_t beam) {
    if (beam < 1 || beam > MAXB) return "ctc beam search: beam must be in 1 .. 32";
    if (vocab < 2 || vocab > MAXV) return "ctc beam search: vocab must be in 2 .. 1024";
    if (batch < 0 || t_out < 0) return "ctc beam search: bad shape";
    if ((int64_t)beam * t_out >= (1ll << 24)) return "ctc beam search: beam * t_out too large";
    return nullptr;
}

struct CtcBeamArgs {
    const float* logits; const int64_t* lens;
    int T, V, beam; float tmp;
    char* utt; int* stats; CtcBeamLayout L;
    int* tokens; int* token_len; float* score;
};

// logaddexp in the log1pf form of the prefix beam search this kernel follows; rnnt_align.hip's lse2 and ctc_align.hip's lse3 are the logf form of the losses
// they follow: different formulas on purpose
__device__ __forceinline__ float lse(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + log1pf(expf(-fabsf(a - b)));
}

// lp -> unsigned key with the same order (larger lp, larger key)
__device__ __forceinline__ unsigned okey(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// candidate order as one integer, larger = earlier: score desc (-0 counts as +0), then ck asc; 0 = empty slot
__device__ __forceinline__ unsigned long long cand_key(float s, int ck) {
    return ((unsigned long long)okey(s == 0.f ? 0.f : s) << 32) | (unsigned)(0x7fffffff - ck);
}

__device__ __forceinline__ unsigned hash_slot(int par, int c, unsigned mask) {
    unsigned h = (unsigned)par * 0x9E3779B1u ^ ((unsigned)c + 0x7F4A7C15u) * 0x85EBCA77u;
    h ^= h >> 16;
    return h & mask;
}

__device__ __forceinline__ unsigned long long hload(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(CT) void ctc_beam_kernel(const CtcBeamArgs a) {
    __shared__ float slp[MAXV];                   // the frame's log-probabilities
    __shared__ int spos[MAXV];                    // token -> position in the frame's top-K list, -1 otherwise
    __shared__ unsigned hist[2][256];
    __shared__ unsigned long long selk[MAXK];     // top-K tokens, unordered: (okey(lp) << 32) | ~id, larger = earlier
    __shared__ int stop[MAXK];                    // top-K tokens in (lp desc, id asc) order
    __shared__ float sredm[CNW], sreds[CNW];
    __shared__ int sscan[CNW];
    // the beam, double buffered by frame parity, rank order
    __shared__ int bnode[2][MAXB], blast[2][MAXB], bpar[2][MAXB], bdep[2][MAXB];
    __shared__ float bpb[2][MAXB], bpnb[2][MAXB], bs[2][MAXB];
    __shared__ int bpm[MAXB];                     // rank of the member whose prefix is this member's parent, -1: none
    __shared__ unsigned bexcl[MAXB][3];           // top-K positions that are not plain extensions of the member
    // candidates: [0, n) members, [n, 2n) repeat extensions, [2n, 2n + n beam) plain extensions (member i: 2n + i beam + r)
    __shared__ float cs[MAXS], cpb[MAXS], cpnb[MAXS];
    __shared__ int ck[MAXS];                      // ((last token + 1) << 16) | canonical index; INT_MAX: empty slot
    __shared__ unsigned long long ckey[MAXS];     // cand_key(cs, ck); 0: empty slot
    __shared__ int nsel[MAXB];                    // candidate slot of each rank of the next beam
    __shared__ int s_n, s_nn, s_nsel, s_nvalid, s_digit, s_need;

    const CtcBeamLayout& L = a.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, V = a.V, beam = a.beam, T = a.T;
    const int K = 2 * beam + 1 < V ? 2 * beam + 1 : V;
    long long lenll = a.lens[b];
    const int len = lenll < 0 ? 0 : (lenll > T ? T : (int)lenll);
    char* base = a.utt + (size_t)b * L.per_utt;
    int4* trace = reinterpret_cast<int4*>(base + L.trace);
    int4* nodes = reinterpret_cast<int4*>(base + L.nodes);
    unsigned long long* hkeys = reinterpret_cast<unsigned long long*>(base + L.hkeys);
    int* hvals = reinterpret_cast<int*>(base + L.hvals);
    const unsigned hmask = (unsigned)L.hcap - 1;
    const float* lrow = a.logits + (size_t)b * T * V;

    for (int i = tid; i < L.hcap; i += CT) __hip_atomic_store(hkeys + i, HEMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int i = tid; i < MAXV; i += CT) spos[i] = -1;
    hist[0][tid] = 0u;
    if (tid == 0) {
        nodes[0] = make_int4(-1, -1, 0, 0);
        bnode[0][0] = 0; blast[0][0] = -1; bpar[0][0] = -1; bdep[0][0] = 0;
        bpb[0][0] = 0.f; bpnb[0][0] = -INFINITY; bs[0][0] = 0.f;
        s_n = 1; s_nn = 1; s_nsel = 0; s_nvalid = 0;
    }
    float nx[TPT];
#pragma unroll
    for (int q = 0; q < TPT; ++q) {
        const int v = tid * TPT + q;
        nx[q] = (len > 0 && v < V) ? lrow[v] : 0.f;
    }
    int cur = 0;
    long long ncand = 0;
    __syncthreads();

    for (int t = 0; t < len; ++t) {
        float x[TPT];
#pragma unroll
        for (int q = 0; q < TPT; ++q) x[q] = nx[q];
        if (t + 1 < len) {                         // prefetch frame t + 1 under this frame's work
#pragma unroll
            for (int q = 0; q < TPT; ++q) {
                const int v = tid * TPT + q;
                if (v < V) nx[q] = lrow[(size_t)(t + 1) * V + v];
            }
        }
        // ---- lp = (x / tmp).softmax().log() in fp32
        float m = -INFINITY;
#pragma unroll
        for (int q = 0; q < TPT; ++q) {
            const int v = tid * TPT + q;
            x[q] = x[q] / a.tmp;
            if (v < V) m = fmaxf(m, x[q]);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) sredm[wave] = m;
        __syncthreads();
        m = sredm[0];
#pragma unroll
        for (int w = 1; w < CNW; ++w) m = fmaxf(m, sredm[w]);
        float e[TPT], ssum = 0.f;
#pragma unroll
        for (int q = 0; q < TPT; ++q) {
            const int v = tid * TPT + q;
            e[q] = v < V ? expf(x[q] - m) : 0.f;
            ssum += e[q];
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ssum += __shfl_xor(ssum, o);
        if (lane == 0) sreds[wave] = ssum;
        __syncthreads();
        ssum = sreds[0];
#pragma unroll
        for (int w = 1; w < CNW; ++w) ssum += sreds[w];
        unsigned key[TPT];
#pragma unroll
        for (int q = 0; q < TPT; ++q) {
            const int v = tid * TPT + q;
            key[q] = 0u;
            if (v < V) {
                const float l = logf(e[q] / ssum);
                slp[v] = l;
                key[q] = okey(l);
            }
        }
        // ---- radix select: the K-th largest key (8 bits per pass); `need` = how many keys equal to it are taken
        unsigned prefix = 0u, pmask = 0u;
        int need = K;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            unsigned* h = hist[pass & 1];
#pragma unroll
            for (int q = 0; q < TPT; ++q)
                if (tid * TPT + q < V && (key[q] & pmask) == prefix) atomicAdd(h + ((key[q] >> shift) & 255u), 1u);
            hist[(pass + 1) & 1][tid] = 0u;
            __syncthreads();
            if (wave == 0) {                       // lane l holds digits 255 - 4 l .. 252 - 4 l (descending)
                unsigned hv[4], c = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) { hv[j] = h[255 - 4 * lane - j]; c += hv[j]; }
                const int incl = wave_incl_scan((int)c, lane), excl = incl - (int)c;
                if (excl < need && incl >= need) {
                    int cum = excl, j = 0;
                    while (cum + (int)hv[j] < need) { cum += (int)hv[j]; ++j; }
                    s_digit = 255 - 4 * lane - j;
                    s_need = need - cum;
                }
            }
            __syncthreads();
            prefix |= (unsigned)s_digit << shift;
            pmask |= 255u << shift;
            need = s_need;
        }
        // ---- the K tokens: keys above the threshold, and the `need` lowest ids among the keys equal to it
        int nt = 0;
#pragma unroll
        for (int q = 0; q < TPT; ++q) nt += (tid * TPT + q < V && key[q] == prefix);
        const int incl = wave_incl_scan(nt, lane);
        if (lane == 63) sscan[wave] = incl;
        __syncthreads();
        int toff = incl - nt;
        for (int w = 0; w < wave; ++w) toff += sscan[w];
#pragma unroll
        for (int q = 0; q < TPT; ++q) {
            const int v = tid * TPT + q;
            if (v >= V) continue;
            bool sel = key[q] > prefix;
            if (key[q] == prefix) { sel = toff < need; ++toff; }
            if (sel) selk[atomicAdd(&s_nsel, 1)] = ((unsigned long long)key[q] << 32) | (0xffffffffu - (unsigned)v);
        }
        const int n = s_n;
        // parent member of every member (a compare of nodes: node identity is string identity)
        if (tid < n) {
            const int par = bpar[cur][tid];
            int pm = -1;
            if (par >= 0)
                for (int j = 0; j < n; ++j) if (bnode[cur][j] == par) pm = j;
            bpm[tid] = pm;
        }
        __syncthreads();
        if (tid < K) {                             // order the K tokens by (lp desc, id asc): one 64-bit compare per pair
            const unsigned long long kv = selk[tid];
            int r = 0;
#pragma unroll 8
            for (int j = 0; j < K; ++j) r += selk[j] > kv;
            const int v = (int)(0xffffffffu - (unsigned)kv);
            stop[r] = v;
            spos[v] = r;
        }
        const int S = 2 * n + n * beam;
        for (int j = 2 * n + tid; j < S; j += CT) { ck[j] = 0x7fffffff; ckey[j] = 0ull; }
        __syncthreads();
        // ---- members: exclusion masks, the member candidate (merges included) and the repeat extension
        if (tid < n) {
            const int i = tid, li = blast[cur][i];
            unsigned ex[3] = {0u, 0u, 0u};
            auto setb = [&](int p) { if (p >= 0) ex[p >> 5] |= 1u << (p & 31); };
            setb(spos[0]);
            if (li >= 0) setb(spos[li]);
            bool rep = li >= 0;
            for (int k = 0; k < n; ++k)
                if (bpm[k] == i) {
                    const int lk = blast[cur][k];
                    setb(spos[lk]);
                    if (lk == li) rep = false;     // P last(P) is a member: the repeat term goes to that member
                }
            bexcl[i][0] = ex[0]; bexcl[i][1] = ex[1]; bexcl[i][2] = ex[2];
            const float si = bs[cur][i];
            float nb = li >= 0 ? slp[li] + bpnb[cur][i] : -INFINITY;
            const int pm = bpm[i];
            if (pm >= 0) nb = lse(nb, slp[li] + (li == blast[cur][pm] ? bpb[cur][pm] : bs[cur][pm]));
            const float bb = slp[0] + si;
            cs[i] = lse(bb, nb); cpb[i] = bb; cpnb[i] = nb; ck[i] = ((li + 1) << 16) | i; ckey[i] = cand_key(cs[i], ck[i]);
            if (rep) {
                const float r = slp[li] + bpb[cur][i];
                cs[n + i] = r; cpb[n + i] = -INFINITY; cpnb[n + i] = r; ck[n + i] = ((li + 1) << 16) | (n + i * V + li);
                ckey[n + i] = cand_key(r, ck[n + i]);
            } else {
                ck[n + i] = 0x7fffffff; ckey[n + i] = 0ull;
            }
        }
        __syncthreads();
        // ---- plain extensions: member i's r-th plain token in top-K order, r < beam
        for (int j = tid; j < n * K; j += CT) {
            const int i = j / K, p = j - i * K;
            const unsigned w = bexcl[i][p >> 5];
            if (w & (1u << (p & 31))) continue;
            int r = __popc(~w & ((1u << (p & 31)) - 1u));
            for (int q = 0; q < (p >> 5); ++q) r += __popc(~bexcl[i][q]);
            if (r >= beam) continue;
            const int c = stop[p], slot = 2 * n + i * beam + r;
            const float nb = slp[c] + bs[cur][i];
            const int k = ((c + 1) << 16) | (n + i * V + c);
            cs[slot] = nb; cpb[slot] = -INFINITY; cpnb[slot] = nb; ck[slot] = k; ckey[slot] = cand_key(nb, k);
        }
        __syncthreads();
        if (tid < K) spos[stop[tid]] = -1;
        // ---- selection: rank = number of candidates before this one (one 64-bit compare per pair; empty slots never count)
        for (int j = tid; j < S; j += CT) {
            const unsigned long long kj = ckey[j];
            if (kj == 0ull) continue;
            int r = 0;
#pragma unroll 8
            for (int q = 0; q < S; ++q) r += ckey[q] > kj;
            if (r < beam) nsel[r] = j;
            atomicAdd(&s_nvalid, 1);
        }
        __syncthreads();
        // ---- the next beam: nodes of new prefixes (old node if the string was seen before), trace
        if (wave == 0) {
            const int nv = s_nvalid, nnew = nv < beam ? nv : beam, nn0 = s_nn, nxt = cur ^ 1;
            int node = -1, last = -1, par = -1, dep = 0;
            float pb = -INFINITY, pnb = -INFINITY, sc = -INFINITY;
            bool isnew = false;
            unsigned long long hk = 0ull;
            if (lane < nnew) {
                const int j = nsel[lane], kj = ck[j], idx = kj & 0xffff;
                pb = cpb[j]; pnb = cpnb[j]; sc = cs[j];
                if (idx < n) {
                    node = bnode[cur][idx]; last = blast[cur][idx]; par = bpar[cur][idx]; dep = bdep[cur][idx];
                } else {
                    const int i = (idx - n) / V, c = idx - n - i * V;
                    par = bnode[cur][i]; last = c; dep = bdep[cur][i] + 1;
                    hk = ((unsigned long long)(unsigned)par << 32) | (unsigned)c;
                    unsigned sl = hash_slot(par, c, hmask);
                    for (unsigned pr = 0; pr <= hmask; ++pr) {
                        const unsigned long long k = hload(hkeys + sl);
                        if (k == hk) { node = __hip_atomic_load(hvals + sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
                        if (k == HEMPTY) break;
                        sl = (sl + 1) & hmask;
                    }
                    isnew = node < 0;
                }
            }
            const unsigned long long nm = __ballot(isnew);
            if (isnew) {
                node = nn0 + __popcll(nm & ((1ull << lane) - 1ull));
                nodes[node] = make_int4(par, last, dep, 0);
                unsigned sl = hash_slot(par, last, hmask);
                for (unsigned pr = 0; pr <= hmask; ++pr) {
                    if (atomicCAS(hkeys + sl, HEMPTY, hk) == HEMPTY) {
                        __hip_atomic_store(hvals + sl, node, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        break;
                    }
                    sl = (sl + 1) & hmask;
                }
            }
            if (lane < beam) trace[(size_t)t * beam + lane] = make_int4(node, __float_as_int(pb), __float_as_int(pnb), __float_as_int(sc));
            if (lane < nnew) {
                bnode[nxt][lane] = node; blast[nxt][lane] = last; bpar[nxt][lane] = par; bdep[nxt][lane] = dep;
                bpb[nxt][lane] = pb; bpnb[nxt][lane] = pnb; bs[nxt][lane] = sc;
            }
            if (lane == 0) {
                ncand += nv;
                s_nn = nn0 + __popcll(nm); s_n = nnew; s_nvalid = 0; s_nsel = 0;
            }
        }
        __syncthreads();
        cur ^= 1;
    }
    // ---- outputs in rank order: tokens by walking the trie from each member's node
    const int n = s_n;
    if (tid < beam) {
        int* out = a.tokens + ((size_t)b * beam + tid) * T;
        int d = 0;
        float sc = -INFINITY;
        if (tid < n) {
            d = bdep[cur][tid];
            sc = bs[cur][tid];
            int node = bnode[cur][tid];
            for (int i = d - 1; i >= 0; --i) { const int4 nd = nodes[node]; out[i] = nd.y; node = nd.x; }
        }
        a.token_len[(size_t)b * beam + tid] = d;
        a.score[(size_t)b * beam + tid] = sc;
    }
    for (int j = tid; j < beam * T; j += CT) {
        const int r = j / T, i = j - r * T;
        if (i >= (r < n ? bdep[cur][r] : 0)) a.tokens[((size_t)b * beam + r) * T + i] = 0;
    }
    if (tid == 0) {
        a.stats[4 * b + 0] = len;
        a.stats[4 * b + 1] = (int)(ncand < 0x7fffffffll ? ncand : 0x7fffffffll);
        a.stats[4 * b + 2] = s_nn;
        a.stats[4 * b + 3] = 0;
    }
}

}  // namespace

extern "C" {

size_t effconf_ctc_beam_workspace_bytes(int32_t batch, int32_t t_out, int32_t vocab, int32_t beam) {
    if (const char* e = ctc_beam_check(batch, t_out, vocab, beam)) { ec_fail(e); return 0; }
    return ctc_beam_layout(batch, t_out, beam).total;
}

int effconf_ctc_beam(const float* logits, const int64_t* out_len, int32_t batch, int32_t t_out, int32_t vocab, int32_t beam,
                     float temperature, int32_t* tokens, int32_t* token_len, float* score, void* workspace, size_t workspace_bytes,
                     void* stream) {
    if (const char* e = ctc_beam_check(batch, t_out, vocab, beam)) return ec_fail(e);
    if (!(temperature > 0.f) || !std::isfinite(temperature)) return ec_fail("ctc beam search: temperature must be > 0");
    if (batch == 0) return 0;
    if (!out_len || !token_len || !score || !workspace || (t_out > 0 && (!logits || !tokens))) return ec_fail("null argument");
    const CtcBeamLayout L = ctc_beam_layout(batch, t_out, beam);
    if (workspace_bytes < L.total) return ec_fail("workspace too small (effconf_ctc_beam_workspace_bytes)");
    char* ws = WsPlan::base(workspace);
    CtcBeamArgs a{};
    a.logits = logits; a.lens = out_len; a.T = t_out; a.V = vocab; a.beam = beam; a.tmp = temperature;
    a.utt = ws + L.utt; a.stats = reinterpret_cast<int*>(ws + L.stats); a.L = L;
    a.tokens = tokens; a.token_len = token_len; a.score = score;
    hipLaunchKernelGGL(ctc_beam_kernel, dim3(batch), dim3(CT), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : ec_fail("ctc_beam launch failed");
}

}  // extern "C"
