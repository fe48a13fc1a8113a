// The CTC prefix beam search of ctc_beam.hip (the specification and the design are in that file's header comment): ctc_beam_search<LM, STREAM>, one workgroup of CT
// threads per utterance, called by the three kernels.  LM: the fused search, ranked by total, resumable between LM rounds.  STREAM: workgroup b runs
// stream sz.streams[b] over the frames of one push; frames and trace are push-local (0 .. len - 1), beam and trie live in the stream's block of the state (6l).  A
// branch under `if constexpr` is not compiled into the instances it is not for.  The beam that outlives a launch is ONE record (decode_layout.h, CTC_REC_*), loaded
// and stored by one function each; the frame loop is the phases of 6c, one function each, on the workgroup's LDS (CtcBeamShared) and the thread's CtcBeamThread.
#pragma once
#include "decode_common.h"

#include <cstdint>

namespace ecctc {

using namespace ecdec;

constexpr int CT = 256;                           // threads per utterance
constexpr int CNW = CT / 64;                      // waves
constexpr int MAXB = 32;                          // largest beam
constexpr int MAXV = 1024;                        // largest vocabulary
constexpr int TPT = MAXV / CT;                    // tokens per thread (contiguous: thread i owns i TPT .. i TPT + TPT - 1)
constexpr int MAXK = 2 * MAXB + 1;                // top tokens per frame
constexpr int MAXS = 2 * MAXB + MAXB * MAXB;      // candidate slots: members, repeat extensions, plain extensions
constexpr unsigned long long HEMPTY = ~0ull;
static_assert(MAXB == CTC_BEAM_MAXB, "the record's arrays hold the largest beam");

struct CtcBeamArgs {
    const float* logits; const int64_t* lens;
    int T, V, beam; float tmp;
    char* utt; int* stats; CtcBeamLayout L;
    int* tokens; int* token_len; float* score;
};

// the fused search's side of the arguments (empty for the plain search)
struct CtcLmSide {
    int4* req;               // [B][beam] requests of the round: token, source slot, destination slot, live
    const int* slot;         // [B * beam] packed column of every request of the last LM step
    const float* logits;     // [packed column][V] raw logits rows of the last LM step
    int* resume;             // [B][CTC_BEAM_LM_REC_INTS] the utterances' records
    int* active;             // utterances suspended in this launch
    size_t lmnodes, trace2;  // offsets inside an utterance
    int nls;                 // floats of a slot's state; its row follows
    float w, tmp, bonus;
    float* total; float* lm_score;
};

// the resumed search's side of the arguments (empty for the two whole-utterance kernels).  There a.utt / a.L.per_utt / a.L.trace address the push's traces in the
// workspace, a.L.nodes / hkeys / hvals / hcap are those of a stream's block, a.T is t_new and tokens / token_len / score are (n, nbest, ..)
struct CtcStreamSide {
    const int* streams;      // [n] listed stream ids
    int* primed;             // [max_streams] 1: the record holds the stream's beam at a frame boundary
    char* blocks;            // the streams' blocks, per_stream apart: record, trie nodes, hash
    size_t per_stream, rec;  // rec: the record inside a block
    int max_streams, max_frames, nbest, max_tokens;
    int* stable_len;         // [n]
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

// a + w x and total(Q) with every operation rounded on its own, in the order of model_ctc.select_nbest.  The pragma: the compiler's default contraction would
// fuse a product into the sum that follows it (also through the _rn intrinsics, which are plain operators)
__device__ __forceinline__ float lm_scaled_sum(float a, float w, float x) {
#pragma clang fp contract(off)
    const float wx = w * x;
    return a + wx;
}

__device__ __forceinline__ float fused_total(float s, float L, int len, float w, float bonus) {
#pragma clang fp contract(off)
    const float bl = bonus * (float)len;
    return lm_scaled_sum(s, w, L) + bl;
}

// ---- the workgroup's LDS, one struct per instance.  The frame-global top-K is the plain search's alone, L and the LM slots the fused search's: the other instance
// gets an empty base.  Every array starts at a multiple of 16 bytes (those whose size is no such multiple come last in their part), so that two keys of a rank
// loop, four bins and the waves' four partial results are one ds_read_b128 each
struct CtcSearchShared {
    unsigned long long ckey[MAXS];                // cand_key(rank, ck) of the candidates; 0: empty slot
    float slp[MAXV];                              // the frame's log-probabilities
    float sredm[CNW], sreds[CNW];
    // the beam, double buffered by frame parity, rank order
    int bnode[2][MAXB], blast[2][MAXB], bpar[2][MAXB], bdep[2][MAXB];
    float bpb[2][MAXB], bpnb[2][MAXB], bs[2][MAXB];
    int bpm[MAXB];                                // rank of the member whose prefix is this member's parent, -1: none
    // candidates: [0, n) members, [n, 2n) repeat extensions, [2n, 2n + n beam) plain extensions (member i: 2n + i beam + r)
    float cs[MAXS], cpb[MAXS], cpnb[MAXS];
    int ck[MAXS];                                 // ((last token + 1) << 16) | canonical index; INT_MAX: empty slot
    int nsel[MAXB];                               // candidate slot of each rank of the next beam
};
template <bool ON> struct CtcTopKShared {};
template <> struct CtcTopKShared<true> {
    unsigned hist[2][256];
    int sscan[CNW];
    int spos[MAXV];                               // token -> position in the frame's top-K list, -1 otherwise
    unsigned bexcl[MAXB][3];                      // top-K positions that are not plain extensions of the member
    unsigned long long selk[MAXK];                // top-K tokens, unordered: (okey(lp) << 32) | ~id, larger = earlier
    int stop[MAXK];                               // top-K tokens in (lp desc, id asc) order
    int ntop, digit, need;                        // tokens in selk; the radix pass's digit and what is still needed of it
};
template <bool ON> struct CtcFusedShared {};
template <> struct CtcFusedShared<true> {
    float bL[2][MAXB], cL[MAXS];                  // L of the members and of the candidates
    int bslot[2][MAXB], spend[MAXB];              // the members' LM slots; whether a member's row is still the LM step's raw logits
    int susp;
};
template <bool LM> struct CtcBeamShared : CtcSearchShared, CtcTopKShared<!LM>, CtcFusedShared<LM> {
    int n, nn, nvalid;                            // members, trie nodes, the frame's candidates
};
// four workgroups of the plain search per CU (4 x 39640 of 163840 bytes; above 40960 one is lost): no instance may grow
static_assert(sizeof(CtcBeamShared<false>) == 39640 && sizeof(CtcBeamShared<true>) == 37296 && sizeof(CtcSearchShared) % 16 == 0, "LDS of the search");

// what a thread knows for the whole launch
struct CtcBeamThread {
    int tid, lane, wave, b, V, beam, K;
    int4* trace; int4* nodes;                     // the launch's trace [frame][rank]; the trie
    unsigned long long* hkeys; int* hvals; unsigned hmask;
    float* lmn; float2* trace2; int nf;           // the fused search: the utterance's LM slots, its second trace, floats of a slot
};

// ---- the record -> the beam in buffer 0 (a resumed launch); ncand and nreq are thread 0's
template <bool LM>
__device__ __forceinline__ void load_beam(CtcBeamShared<LM>& sh, const CtcBeamThread& c, const int* rec, long long& ncand, int& nreq) {
    const int* ra = rec + CTC_REC_HEAD;
    const int tid = c.tid, rn = rec[CTC_REC_N] < c.beam ? rec[CTC_REC_N] : c.beam;
    if (tid < rn) {
        sh.bnode[0][tid] = ra[tid]; sh.blast[0][tid] = ra[MAXB + tid]; sh.bpar[0][tid] = ra[2 * MAXB + tid]; sh.bdep[0][tid] = ra[3 * MAXB + tid];
        sh.bpb[0][tid] = __int_as_float(ra[4 * MAXB + tid]); sh.bpnb[0][tid] = __int_as_float(ra[5 * MAXB + tid]);
        sh.bs[0][tid] = __int_as_float(ra[6 * MAXB + tid]);
        if constexpr (LM) { sh.bL[0][tid] = __int_as_float(ra[7 * MAXB + tid]); sh.bslot[0][tid] = ra[8 * MAXB + tid]; sh.spend[tid] = ra[9 * MAXB + tid]; }
    }
    if (tid == 0) {
        sh.n = rn; sh.nn = rec[CTC_REC_NN]; sh.nvalid = 0;
        ncand = ((long long)rec[CTC_REC_NCHI] << 32) | (unsigned)rec[CTC_REC_NCLO];
        if constexpr (LM) nreq = rec[CTC_REC_NREQ];
    }
}

// ---- the beam in buffer `cur` -> the record, with `frames` frames consumed
template <bool LM>
__device__ __forceinline__ void store_beam(const CtcBeamShared<LM>& sh, const CtcBeamThread& c, int* rec, int cur, int frames, long long ncand, int nreq) {
    int* ra = rec + CTC_REC_HEAD;
    const int tid = c.tid;
    if (tid < sh.n) {
        ra[tid] = sh.bnode[cur][tid]; ra[MAXB + tid] = sh.blast[cur][tid]; ra[2 * MAXB + tid] = sh.bpar[cur][tid]; ra[3 * MAXB + tid] = sh.bdep[cur][tid];
        ra[4 * MAXB + tid] = __float_as_int(sh.bpb[cur][tid]); ra[5 * MAXB + tid] = __float_as_int(sh.bpnb[cur][tid]);
        ra[6 * MAXB + tid] = __float_as_int(sh.bs[cur][tid]);
        if constexpr (LM) { ra[7 * MAXB + tid] = __float_as_int(sh.bL[cur][tid]); ra[8 * MAXB + tid] = sh.bslot[cur][tid]; ra[9 * MAXB + tid] = sh.spend[tid]; }
    }
    if (tid == 0) {
        rec[CTC_REC_FRAMES] = frames; rec[CTC_REC_N] = sh.n; rec[CTC_REC_NN] = sh.nn;
        rec[CTC_REC_NCLO] = (int)(unsigned)(ncand & 0xffffffffll); rec[CTC_REC_NCHI] = (int)(ncand >> 32);
        if constexpr (LM) { rec[CTC_REC_PHASE] = 1; rec[CTC_REC_NREQ] = nreq; }
    }
}

// ---- the fused search, on resume: the rows the LM step left as raw logits -> log softmax(x / lm_tmp) in the member's slot: logf(expf(x / lm_tmp - max) / sum), one
// wave per row, lane l owns tokens l, 64 + l, ..; the sum is a fixed butterfly over the lanes' partial sums
__device__ __forceinline__ void lm_pending_rows(CtcBeamShared<true>& sh, const CtcBeamThread& c, const CtcLmSide& fz) {
    const int n0 = sh.n, lane = c.lane, V = c.V;
    for (int r = c.wave; r < n0; r += CNW) {
        if (!sh.spend[r]) continue;
        const int col = fz.slot[(size_t)c.b * c.beam + r];                          // the packed column of this rank's request (live, so >= 0)
        const float* src = fz.logits + (size_t)(col < 0 ? 0 : col) * V;
        float* dst = c.lmn + (size_t)sh.bslot[0][r] * c.nf + fz.nls;
        float xv[MAXV / 64], mx = -INFINITY;
#pragma unroll
        for (int q = 0; q < MAXV / 64; ++q) {
            const int v = lane + 64 * q;
            xv[q] = v < V ? src[v] / fz.tmp : -INFINITY;
            mx = fmaxf(mx, xv[q]);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        float sm = 0.f;
#pragma unroll
        for (int q = 0; q < MAXV / 64; ++q) { xv[q] = lane + 64 * q < V ? expf(xv[q] - mx) : 0.f; sm += xv[q]; }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sm += __shfl_xor(sm, o);
#pragma unroll
        for (int q = 0; q < MAXV / 64; ++q)
            if (lane + 64 * q < V) dst[lane + 64 * q] = logf(xv[q] / sm);
    }
    __syncthreads();
    if (c.tid < MAXB) sh.spend[c.tid] = 0;
}

// ---- frame log-softmax: lp = (x / tmp).softmax().log() in fp32 -> slp, and the order keys of the thread's tokens
template <bool LM>
__device__ __forceinline__ void frame_log_softmax(CtcBeamShared<LM>& sh, const CtcBeamThread& c, float tmp, float (&x)[TPT], unsigned (&key)[TPT]) {
    const int tid = c.tid, lane = c.lane, wave = c.wave, V = c.V;
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < TPT; ++q) {
        const int v = tid * TPT + q;
        x[q] = x[q] / tmp;
        if (v < V) m = fmaxf(m, x[q]);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) sh.sredm[wave] = m;
    __syncthreads();
    m = sh.sredm[0];
#pragma unroll
    for (int w = 1; w < CNW; ++w) m = fmaxf(m, sh.sredm[w]);
    float e[TPT], ssum = 0.f;
#pragma unroll
    for (int q = 0; q < TPT; ++q) {
        const int v = tid * TPT + q;
        e[q] = v < V ? expf(x[q] - m) : 0.f;
        ssum += e[q];
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ssum += __shfl_xor(ssum, o);
    if (lane == 0) sh.sreds[wave] = ssum;
    __syncthreads();
    ssum = sh.sreds[0];
#pragma unroll
    for (int w = 1; w < CNW; ++w) ssum += sh.sreds[w];
#pragma unroll
    for (int q = 0; q < TPT; ++q) {
        const int v = tid * TPT + q;
        key[q] = 0u;
        if (v < V) {
            const float l = logf(e[q] / ssum);
            sh.slp[v] = l;
            key[q] = okey(l);
        }
    }
}

// ---- top-K select (the plain search): the frame's K most probable tokens in (lp desc, id asc) order -> stop, spos
__device__ __forceinline__ void topk_select(CtcBeamShared<false>& sh, const CtcBeamThread& c, const unsigned (&key)[TPT]) {
    const int tid = c.tid, lane = c.lane, wave = c.wave, V = c.V, K = c.K;
    // radix select: the K-th largest key (8 bits per pass); `need` = how many keys equal to it are taken
    unsigned prefix = 0u, pmask = 0u;
    int need = K;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        unsigned* h = sh.hist[pass & 1];
#pragma unroll
        for (int q = 0; q < TPT; ++q)
            if (tid * TPT + q < V && (key[q] & pmask) == prefix) atomicAdd(h + ((key[q] >> shift) & 255u), 1u);
        sh.hist[(pass + 1) & 1][tid] = 0u;
        __syncthreads();
        if (wave == 0) {                           // lane l holds digits 255 - 4 l .. 252 - 4 l (descending)
            unsigned hv[4], cnt = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) { hv[j] = h[255 - 4 * lane - j]; cnt += hv[j]; }
            const int incl = wave_incl_scan((int)cnt, lane), excl = incl - (int)cnt;
            if (excl < need && incl >= need) {
                int cum = excl, j = 0;
                while (cum + (int)hv[j] < need) { cum += (int)hv[j]; ++j; }
                sh.digit = 255 - 4 * lane - j;
                sh.need = need - cum;
            }
        }
        __syncthreads();
        prefix |= (unsigned)sh.digit << shift;
        pmask |= 255u << shift;
        need = sh.need;
    }
    // the K tokens: keys above the threshold, and the `need` lowest ids among the keys equal to it
    int nt = 0;
#pragma unroll
    for (int q = 0; q < TPT; ++q) nt += (tid * TPT + q < V && key[q] == prefix);
    const int incl = wave_incl_scan(nt, lane);
    if (lane == 63) sh.sscan[wave] = incl;
    __syncthreads();
    int toff = incl - nt;
    for (int w = 0; w < wave; ++w) toff += sh.sscan[w];
#pragma unroll
    for (int q = 0; q < TPT; ++q) {
        const int v = tid * TPT + q;
        if (v >= V) continue;
        bool sel = key[q] > prefix;
        if (key[q] == prefix) { sel = toff < need; ++toff; }
        if (sel) sh.selk[atomicAdd(&sh.ntop, 1)] = ((unsigned long long)key[q] << 32) | (0xffffffffu - (unsigned)v);
    }
    __syncthreads();
    if (tid < K) {                                 // order the K tokens by (lp desc, id asc): one 64-bit compare per pair
        const unsigned long long kv = sh.selk[tid];
        int r = 0;
#pragma unroll 8
        for (int j = 0; j < K; ++j) r += sh.selk[j] > kv;
        const int v = (int)(0xffffffffu - (unsigned)kv);
        sh.stop[r] = v;
        sh.spos[v] = r;
    }
}

// ---- candidates of the members: the member candidate (merges included) and the repeat extension, ranked by s (the fused search: by total); the plain search
// also notes the top-K positions that are not plain extensions of the member
template <bool LM>
__device__ __forceinline__ void member_candidates(CtcBeamShared<LM>& sh, const CtcBeamThread& c, const CtcLmSide& fz, int n, int cur) {
    if (c.tid >= n) return;
    auto rank = [&](float s, float Lq, int depth) { return LM ? fused_total(s, Lq, depth, fz.w, fz.bonus) : s; };
    const int i = c.tid, li = sh.blast[cur][i], di = sh.bdep[cur][i], V = c.V;
    unsigned ex[3] = {0u, 0u, 0u};
    auto setb = [&](int p) { if (p >= 0) ex[p >> 5] |= 1u << (p & 31); };
    if constexpr (!LM) {
        setb(sh.spos[0]);
        if (li >= 0) setb(sh.spos[li]);
    }
    bool rep = li >= 0;
    for (int k = 0; k < n; ++k)
        if (sh.bpm[k] == i) {
            const int lk = sh.blast[cur][k];
            if constexpr (!LM) setb(sh.spos[lk]);
            if (lk == li) rep = false;             // P last(P) is a member: the repeat term goes to that member
        }
    if constexpr (!LM) { sh.bexcl[i][0] = ex[0]; sh.bexcl[i][1] = ex[1]; sh.bexcl[i][2] = ex[2]; }
    const float si = sh.bs[cur][i];
    float Li = 0.f;
    if constexpr (LM) Li = sh.bL[cur][i];
    float nb = li >= 0 ? sh.slp[li] + sh.bpnb[cur][i] : -INFINITY;
    const int pm = sh.bpm[i];
    if (pm >= 0) nb = lse(nb, sh.slp[li] + (li == sh.blast[cur][pm] ? sh.bpb[cur][pm] : sh.bs[cur][pm]));
    const float bb = sh.slp[0] + si;
    sh.cs[i] = lse(bb, nb); sh.cpb[i] = bb; sh.cpnb[i] = nb; sh.ck[i] = ((li + 1) << 16) | i;
    if constexpr (LM) sh.cL[i] = Li;
    sh.ckey[i] = cand_key(rank(sh.cs[i], Li, di), sh.ck[i]);
    if (rep) {
        const float r = sh.slp[li] + sh.bpb[cur][i];
        float Lq = 0.f;
        if constexpr (LM) { Lq = Li + c.lmn[(size_t)sh.bslot[cur][i] * c.nf + fz.nls + li]; sh.cL[n + i] = Lq; }
        sh.cs[n + i] = r; sh.cpb[n + i] = -INFINITY; sh.cpnb[n + i] = r; sh.ck[n + i] = ((li + 1) << 16) | (n + i * V + li);
        sh.ckey[n + i] = cand_key(rank(r, Lq, di + 1), sh.ck[n + i]);
    } else {
        sh.ck[n + i] = 0x7fffffff; sh.ckey[n + i] = 0ull;
    }
}

// ---- plain extensions, the plain search: member i's r-th plain token in top-K order, r < beam
__device__ __forceinline__ void plain_extensions_topk(CtcBeamShared<false>& sh, const CtcBeamThread& c, int n, int cur) {
    const int K = c.K, beam = c.beam, V = c.V;
    for (int j = c.tid; j < n * K; j += CT) {
        const int i = j / K, p = j - i * K;
        const unsigned w = sh.bexcl[i][p >> 5];
        if (w & (1u << (p & 31))) continue;
        int r = __popc(~w & ((1u << (p & 31)) - 1u));
        for (int q = 0; q < (p >> 5); ++q) r += __popc(~sh.bexcl[i][q]);
        if (r >= beam) continue;
        const int tok = sh.stop[p], slot = 2 * n + i * beam + r;
        const float nb = sh.slp[tok] + sh.bs[cur][i];
        const int k = ((tok + 1) << 16) | (n + i * V + tok);
        sh.cs[slot] = nb; sh.cpb[slot] = -INFINITY; sh.cpnb[slot] = nb; sh.ck[slot] = k; sh.ckey[slot] = cand_key(nb, k);
    }
}

// ---- plain extensions, the fused search: one wave per member; lane l owns tokens l, 64 + l, ..; `beam` rounds of a wave-wide maximum of (a_P desc, id asc) over
// the member's plain tokens (not blank, not last(P), P c not a member), a_P[c] = lp[c] + w row_P[c]
__device__ __forceinline__ void plain_extensions_lm(CtcBeamShared<true>& sh, const CtcBeamThread& c, const CtcLmSide& fz, int n, int cur) {
    const int lane = c.lane, V = c.V, beam = c.beam;
    for (int i = c.wave; i < n; i += CNW) {
        const float* row = c.lmn + (size_t)sh.bslot[cur][i] * c.nf + fz.nls;
        const int li = sh.blast[cur][i], di = sh.bdep[cur][i];
        const float si = sh.bs[cur][i], Li = sh.bL[cur][i];
        unsigned avail = 0u, akey[MAXV / 64];
#pragma unroll
        for (int q = 0; q < MAXV / 64; ++q) {
            const int v = lane + 64 * q;
            akey[q] = 0u;
            if (v < V) {
                akey[q] = okey(lm_scaled_sum(sh.slp[v], fz.w, row[v]));
                if (v != 0 && v != li) avail |= 1u << q;
            }
        }
        for (int k = 0; k < n; ++k)
            if (sh.bpm[k] == i) {
                const int lk = sh.blast[cur][k];
                if ((lk & 63) == lane) avail &= ~(1u << (lk >> 6));
            }
        for (int r = 0; r < beam; ++r) {
            unsigned bk = 0u;
            int bq = -1;
#pragma unroll
            for (int q = 0; q < MAXV / 64; ++q)
                if (((avail >> q) & 1u) && (bq < 0 || akey[q] > bk)) { bk = akey[q]; bq = q; }
            unsigned long long p = bq >= 0 ? ((unsigned long long)bk << 32) | (0xffffffffu - (unsigned)(lane + 64 * bq)) : 0ull;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const unsigned long long op = __shfl_xor(p, o);
                p = op > p ? op : p;
            }
            if (p == 0ull) break;                  // wave-uniform: no plain token is left
            const int tok = (int)(0xffffffffu - (unsigned)p);
            if ((tok & 63) == lane) avail &= ~(1u << (tok >> 6));
            if (lane == 0) {
                const int slot = 2 * n + i * beam + r;
                const float nb = sh.slp[tok] + si, Lq = Li + row[tok];
                const int k = ((tok + 1) << 16) | (n + i * V + tok);
                sh.cs[slot] = nb; sh.cpb[slot] = -INFINITY; sh.cpnb[slot] = nb; sh.cL[slot] = Lq; sh.ck[slot] = k;
                sh.ckey[slot] = cand_key(fused_total(nb, Lq, di + 1, fz.w, fz.bonus), k);
            }
        }
    }
}

// ---- selection: rank = number of candidates before this one (one 64-bit compare per pair; empty slots never count)
template <bool LM>
__device__ __forceinline__ void select_candidates(CtcBeamShared<LM>& sh, const CtcBeamThread& c, int S) {
    for (int j = c.tid; j < S; j += CT) {
        const unsigned long long kj = sh.ckey[j];
        if (kj == 0ull) continue;
        int r = 0;
#pragma unroll 8
        for (int q = 0; q < S; ++q) r += sh.ckey[q] > kj;
        if (r < c.beam) sh.nsel[r] = j;
        atomicAdd(&sh.nvalid, 1);
    }
}

// ---- next beam and trie (wave 0): nodes of new prefixes (old node if the string was seen before), the trace of frame t, the beam in the other buffer; the fused
// search: the entrants' LM slots and the round's requests.  ncand and nreq are lane 0's
template <bool LM>
__device__ __forceinline__ void next_beam(CtcBeamShared<LM>& sh, const CtcBeamThread& c, const CtcLmSide& fz, int n, int cur, int t, int len, long long& ncand,
                                          int& nreq) {
    const int lane = c.lane, beam = c.beam, V = c.V;
    const unsigned hmask = c.hmask;
    const int nv = sh.nvalid, nnew = nv < beam ? nv : beam, nn0 = sh.nn, nxt = cur ^ 1;
    int node = -1, last = -1, par = -1, dep = 0;
    float pb = -INFINITY, pnb = -INFINITY, sc = -INFINITY;
    bool isnew = false;
    unsigned long long hk = 0ull;
    float Lm = 0.f; int lslot = 0; bool enters = false;      // the fused search: L, LM slot (entrants: their parent's), entered the beam as an extension
    if (lane < nnew) {
        const int j = sh.nsel[lane], kj = sh.ck[j], idx = kj & 0xffff;
        pb = sh.cpb[j]; pnb = sh.cpnb[j]; sc = sh.cs[j];
        if constexpr (LM) Lm = sh.cL[j];
        if (idx < n) {
            node = sh.bnode[cur][idx]; last = sh.blast[cur][idx]; par = sh.bpar[cur][idx]; dep = sh.bdep[cur][idx];
            if constexpr (LM) lslot = sh.bslot[cur][idx];
        } else {
            const int i = (idx - n) / V, tok = idx - n - i * V;
            if constexpr (LM) { lslot = sh.bslot[cur][i]; enters = true; }
            par = sh.bnode[cur][i]; last = tok; dep = sh.bdep[cur][i] + 1;
            hk = ((unsigned long long)(unsigned)par << 32) | (unsigned)tok;
            unsigned sl = hash_slot(par, tok, hmask);
            for (unsigned pr = 0; pr <= hmask; ++pr) {
                const unsigned long long k = hload(c.hkeys + sl);
                if (k == hk) { node = __hip_atomic_load(c.hvals + sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
                if (k == HEMPTY) break;
                sl = (sl + 1) & hmask;
            }
            isnew = node < 0;
        }
    }
    const unsigned long long nm = __ballot(isnew);
    if (isnew) {
        node = nn0 + __popcll(nm & ((1ull << lane) - 1ull));
        c.nodes[node] = make_int4(par, last, dep, LM ? __float_as_int(Lm) : 0);      // L(P): set when the node is created, read ever after
        unsigned sl = hash_slot(par, last, hmask);
        for (unsigned pr = 0; pr <= hmask; ++pr) {
            if (atomicCAS(c.hkeys + sl, HEMPTY, hk) == HEMPTY) {
                __hip_atomic_store(c.hvals + sl, node, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
            sl = (sl + 1) & hmask;
        }
    }
    if (lane < beam) c.trace[(size_t)t * beam + lane] = make_int4(node, __float_as_int(pb), __float_as_int(pnb), __float_as_int(sc));
    if (lane < nnew) {
        sh.bnode[nxt][lane] = node; sh.blast[nxt][lane] = last; sh.bpar[nxt][lane] = par; sh.bdep[nxt][lane] = dep;
        sh.bpb[nxt][lane] = pb; sh.bpnb[nxt][lane] = pnb; sh.bs[nxt][lane] = sc;
    }
    if constexpr (LM) {
        if (enters && !isnew) Lm = __int_as_float(c.nodes[node].w);      // a prefix seen before: the L its node holds
        // an entrant takes the lowest of the slots 1 .. 2 beam that no member of the old beam holds (bit s - 1 = slot s): its parent's state stays
        // valid until the LM step has run, and no survivor's slot is taken
        unsigned long long used = 0ull;
        for (int k = 0; k < n; ++k)
            if (sh.bslot[cur][k] > 0) used |= 1ull << (sh.bslot[cur][k] - 1);
        const unsigned long long em = __ballot(enters);
        const bool susp = em != 0ull && t + 1 < len;                   // after the last frame no row is needed any more
        int myslot = lslot;
        if (enters) {
            unsigned long long fr = ~used & (2 * beam >= 64 ? ~0ull : (1ull << (2 * beam)) - 1ull);
            for (int k = __popcll(em & ((1ull << lane) - 1ull)); k > 0; --k) fr &= fr - 1ull;
            myslot = __ffsll((long long)fr);                           // >= 1: at most beam bits are used, at most beam candidates enter
        }
        if (lane < beam) {
            c.trace2[(size_t)t * beam + lane] = lane < nnew ? make_float2(Lm, fused_total(sc, Lm, dep, fz.w, fz.bonus)) : make_float2(0.f, -INFINITY);
            if (susp) fz.req[(size_t)c.b * beam + lane] = enters ? make_int4(last, lslot, myslot, 1) : make_int4(0, 0, 0, 0);
        }
        if (lane < nnew) { sh.bL[nxt][lane] = Lm; sh.bslot[nxt][lane] = myslot; sh.spend[lane] = enters ? 1 : 0; }
        if (lane == 0) { sh.susp = susp ? 1 : 0; nreq += susp ? __popcll(em) : 0; }
    }
    if (lane == 0) {
        ncand += nv;
        sh.nn = nn0 + __popcll(nm); sh.n = nnew; sh.nvalid = 0;
        if constexpr (!LM) sh.ntop = 0;
    }
}

template <bool LM, bool STREAM>
__device__ __forceinline__ void ctc_beam_search(const CtcBeamArgs& a, const CtcLmSide& fz, const CtcStreamSide& sz) {
    static_assert(!(LM && STREAM), "a fused streaming search is not built: the LM slots would have to persist too");
    __shared__ alignas(16) CtcBeamShared<LM> sh;
    const CtcBeamLayout& L = a.L;
    const int tid = threadIdx.x, b = blockIdx.x, V = a.V, beam = a.beam, T = a.T;
    CtcBeamThread c{};
    c.tid = tid; c.lane = tid & 63; c.wave = tid >> 6; c.b = b; c.V = V; c.beam = beam;
    c.K = 2 * beam + 1 < V ? 2 * beam + 1 : V;
    long long lenll = a.lens[b];
    const int len = lenll < 0 ? 0 : (lenll > T ? T : (int)lenll);
    auto refuse = [&](int code) { if (tid < sz.nbest) a.token_len[(size_t)b * sz.nbest + tid] = code; };
    const int sid = STREAM ? sz.streams[b] : b;
    // STREAM, the first guard, before any address of the state is formed (workgroup-uniform)
    if (STREAM && (sid < 0 || sid >= sz.max_streams)) { refuse(-1); return; }
    char* base = a.utt + (size_t)b * L.per_utt;
    char* tbase = STREAM ? sz.blocks + (size_t)sid * sz.per_stream : base;     // where the trie lives
    c.trace = reinterpret_cast<int4*>(base + L.trace);
    c.nodes = reinterpret_cast<int4*>(tbase + L.nodes);
    c.hkeys = reinterpret_cast<unsigned long long*>(tbase + L.hkeys);
    c.hvals = reinterpret_cast<int*>(tbase + L.hvals);
    c.hmask = (unsigned)L.hcap - 1;
    const float* lrow = a.logits + (size_t)b * T * V;
    // the record of a search that goes on in a later launch.  fresh: it holds nothing yet; frames0: the frames it has consumed
    int* rec = nullptr; bool fresh = true;
    if constexpr (LM) {
        rec = fz.resume + (size_t)b * CTC_BEAM_LM_REC_INTS;
        if (rec[CTC_REC_PHASE] == 2) return;       // finished in an earlier launch (workgroup-uniform)
        fresh = rec[CTC_REC_PHASE] == 0;
        c.lmn = reinterpret_cast<float*>(base + fz.lmnodes);
        c.trace2 = reinterpret_cast<float2*>(base + fz.trace2);
        c.nf = fz.nls + V;
    }
    if constexpr (STREAM) {
        rec = reinterpret_cast<int*>(tbase + sz.rec);
        fresh = sz.primed[sid] == 0;
    }
    const int frames0 = fresh ? 0 : rec[CTC_REC_FRAMES];
    const int t0 = STREAM ? 0 : frames0;           // STREAM: the push's frames are 0 .. len - 1, the stream's frames0 .. frames0 + len - 1
    // STREAM, the second guard: it has read the stream's flag and, where that is set, the frame count of its record - nothing else, and nothing is written (uniform)
    if (STREAM && len > sz.max_frames - frames0) { refuse(-2); return; }

    long long ncand = 0;                           // thread 0: candidates scored
    int nreq = 1;                                  // the fused search, thread 0: LM rows asked for (the root's is the first)
    if constexpr (!LM) {                           // the LDS the radix select counts on, set in every launch
        for (int i = tid; i < MAXV; i += CT) sh.spos[i] = -1;
        sh.hist[0][tid] = 0u;
        if (tid == 0) sh.ntop = 0;
    }
    if (fresh) {
        // STREAM: a push without frames writes nothing to the state (the beam of a stream that never had a frame is the empty prefix, in LDS alone)
        const int hinit = !STREAM || len > 0 ? L.hcap : 0;
        for (int i = tid; i < hinit; i += CT) __hip_atomic_store(c.hkeys + i, HEMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid == 0) {
            if (!STREAM || len > 0) c.nodes[0] = make_int4(-1, -1, 0, 0);
            sh.bnode[0][0] = 0; sh.blast[0][0] = -1; sh.bpar[0][0] = -1; sh.bdep[0][0] = 0;
            sh.bpb[0][0] = 0.f; sh.bpnb[0][0] = -INFINITY; sh.bs[0][0] = 0.f;
            sh.n = 1; sh.nn = 1; sh.nvalid = 0;
            if constexpr (LM) { sh.bL[0][0] = 0.f; sh.bslot[0][0] = 0; sh.spend[0] = 1; }      // the root's row: request 0 of the LM step before the first launch
        }
    } else {
        load_beam(sh, c, rec, ncand, nreq);        // the beam as the suspended launch, or the stream's last push with frames, left it
    }
    float nx[TPT];
#pragma unroll
    for (int q = 0; q < TPT; ++q) {
        const int v = tid * TPT + q;
        nx[q] = (t0 < len && v < V) ? lrow[(size_t)t0 * V + v] : 0.f;
    }
    int cur = 0;
    __syncthreads();
    if constexpr (LM) lm_pending_rows(sh, c, fz);

    for (int t = t0; t < len; ++t) {
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
        unsigned key[TPT];
        frame_log_softmax(sh, c, a.tmp, x, key);
        // parent member of every member (a compare of nodes: node identity is string identity)
        const int n = sh.n;
        if (tid < n) {
            const int par = sh.bpar[cur][tid];
            int pm = -1;
            if (par >= 0)
                for (int j = 0; j < n; ++j) if (sh.bnode[cur][j] == par) pm = j;
            sh.bpm[tid] = pm;
        }
        if constexpr (!LM) topk_select(sh, c, key);
        const int S = 2 * n + n * beam;
        for (int j = 2 * n + tid; j < S; j += CT) { sh.ck[j] = 0x7fffffff; sh.ckey[j] = 0ull; }
        __syncthreads();
        member_candidates(sh, c, fz, n, cur);
        if constexpr (!LM) {
            __syncthreads();
            plain_extensions_topk(sh, c, n, cur);
            __syncthreads();
            if (tid < c.K) sh.spos[sh.stop[tid]] = -1;
        } else {
            plain_extensions_lm(sh, c, fz, n, cur);
            __syncthreads();
        }
        select_candidates(sh, c, S);
        __syncthreads();
        if (c.wave == 0) next_beam(sh, c, fz, n, cur, t, len, ncand, nreq);
        __syncthreads();
        cur ^= 1;
        if constexpr (LM) {
            if (sh.susp) {                         // workgroup-uniform: save the beam, wait for the LM step
                store_beam(sh, c, rec, cur, t + 1, ncand, nreq);
                if (tid == 0) atomicAdd(fz.active, 1);
                return;
            }
        }
    }

    const int n = sh.n;
    if (STREAM && len > 0) {                       // the record: only after a push with frames
        store_beam(sh, c, rec, cur, frames0 + len, ncand, nreq);
        if (tid == 0) sz.primed[sid] = 1;
    }
    // ---- outputs of the beam as it stands, in rank order: tokens by walking the trie from each member's node (token_len is the true depth; tokens beyond MT are
    // not written), zero tails
    const int nbest = STREAM ? sz.nbest : beam, MT = STREAM ? sz.max_tokens : T;
    if (tid < nbest) {
        int* out = a.tokens + ((size_t)b * nbest + tid) * MT;
        int d = 0;
        float sc = -INFINITY;
        if (tid < n) {
            d = sh.bdep[cur][tid];
            sc = sh.bs[cur][tid];
            int node = sh.bnode[cur][tid];
            for (int i = d - 1; i >= 0; --i) {
                const int4 nd = c.nodes[node];
                if (i < MT) out[i] = nd.y;
                node = nd.x;
            }
        }
        a.token_len[(size_t)b * nbest + tid] = d;
        a.score[(size_t)b * nbest + tid] = sc;
        if constexpr (LM) {
            const float Lm = tid < n ? sh.bL[cur][tid] : 0.f;
            fz.lm_score[(size_t)b * beam + tid] = Lm;
            fz.total[(size_t)b * beam + tid] = tid < n ? fused_total(sc, Lm, d, fz.w, fz.bonus) : -INFINITY;
            fz.req[(size_t)b * beam + tid] = make_int4(0, 0, 0, 0);           // nothing to ask of the rounds other utterances still need
        }
    }
    for (int j = tid; j < nbest * MT; j += CT) {
        const int r = j / MT, i = j - r * MT;
        if (i >= (r < n ? sh.bdep[cur][r] : 0)) a.tokens[((size_t)b * nbest + r) * MT + i] = 0;
    }
    // STREAM: the longest common prefix of all members (one wave): lift every member's node to the smallest depth, then step the parents together until all agree.
    // Node identity is string identity, so equal nodes at equal depth are equal prefixes; at depth 0 every node is the root
    if (STREAM && c.wave == 0) {
        const int lane = c.lane;
        int node = lane < n ? sh.bnode[cur][lane] : 0, d = lane < n ? sh.bdep[cur][lane] : 0x7fffffff, dmin = d;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { const int od = __shfl_xor(dmin, o); dmin = od < dmin ? od : dmin; }
        if (lane < n)
            for (; d > dmin; --d) node = c.nodes[node].x;
        while (dmin > 0 && __ballot(lane < n && node != __shfl(node, 0)) != 0ull) {      // wave-uniform; lane 0 is always a member
            if (lane < n) node = c.nodes[node].x;
            --dmin;
        }
        if (lane == 0) sz.stable_len[b] = dmin;
    }
    if (tid == 0) {
        a.stats[4 * b + 0] = len;
        a.stats[4 * b + 1] = (int)(ncand < 0x7fffffffll ? ncand : 0x7fffffffll);
        a.stats[4 * b + 2] = sh.nn;
        a.stats[4 * b + 3] = STREAM ? frames0 + len : (LM ? nreq : 0);
        if constexpr (LM) rec[CTC_REC_PHASE] = 2;
    }
}

}  // namespace ecctc
