// RNN-T beam search (gfx950): Transducer.beam_search_decoding of the reference (models/transducer.py:188-327) without the
// neural-LM and n-gram terms (the state of a plain checkpoint load: no LM checkpoint, no n-gram file).
//
// Per utterance the reference keeps two hypothesis lists.  For each encoder frame t: A = B, B = [], then until B holds `beam`
// hypotheses: pop the hypothesis of A with the largest score / len(prediction) (first maximum in list order), run the decoder on
// (prediction[-1], state), the joint on (f[t], g), logP = (logits / tmp).softmax().log(), and for each of the top `beam` entries
// append a child: blank -> B (same prediction, the parent's OLD state), any other label -> A (label appended, state = the new one).
// The answer is the best hypothesis of B after the last frame (transducer.py:319-323).
//
// Here ONE persistent workgroup runs one utterance; the reference's pop order is replayed exactly on rows computed ahead of it:
//   * a hypothesis's logP row is a pure function of (last token, state, t), so up to `beam_eval_batch` not-yet-evaluated hypotheses of
//     A - the best first, then in pop order (score / len descending, list order on ties) - are evaluated together as the 16 columns of
//     fp32 MFMA tiles (mfma_rows16, the weight images of effconf_rnnt_finalize): the weights stream once per batch instead of once per
//     hypothesis.  Every column's arithmetic is independent of the others (k ascending, unused columns zero), so a row does not depend
//     on what shared its batch: batch 1 and batch 16 give bit-identical results;
//   * a blank child keeps (last token, state) of its parent, so its decoder output at the next frame IS the parent's: hypotheses carry
//     their decoder node (h', c', linear_decoder(h')) and only the children that appended a label need an LSTM step;
//   * predictions are a parent-linked trail of tokens, materialised when a hypothesis is popped (not for every child appended to A).
// Scores are fp32 sums and score / len an IEEE fp32 division, as in the reference (logp_score is a 0-dim fp32 tensor).
//
// Bounds: at most max_expansions pops per frame (status 1 when B is still short: the reference would loop on), at most max_tokens
// tokens in the answer (status 2); a capped utterance returns no tokens.  All storage is in the caller's workspace, sized by
// effconf_rnnt_beam_workspace_bytes from (batch, T, beam, max_expansions).
//
// With a neural LM (effconf_rnnt_beam_lm; transducer.py:259-273, 291-306): logP += lm_weight * (logits_lm / lm_tmp).softmax().log() before the top-k, a label
// child takes the LM's new state and a blank child keeps its parent's.  A hypothesis' LM row is a function of (last token, LM state) - not of t - so it follows the
// decoder node: LM nodes (state, row) live on the index space of the decoder nodes and are carried with them; the LM runs once per label-appended hypothesis that
// gets evaluated.  The LM step is chip-wide (lm.hip: at 4096 x 3 a step streams 1.5 GB of weights and 16 state vectors exceed a CU's LDS), so the search runs in
// rounds on the caller's stream: beam_search<true> - the SAME loop, beam_search<false> is the plain kernel - stops when its next evaluation batch holds pending
// columns, writes one request per such column (token, source node, destination node), saves its loop state (frame, na, nb, pops, used, ntrail, the selected
// columns, the counters; everything else already is in global memory) and exits; ecdec::lm_columns_step runs the LM once for the requests of ALL utterances; the
// next launch turns each delivered logits row into the node's row, evaluates the decoder and the joint as before, forms logP[v] + lm_weight * logP_lm[v] for all V
// entries (multiply and add rounded separately, as the reference's two tensor operations), takes the top `beam` of that row, pops and runs on to its next stop.  A
// batch of carried columns alone needs no LM and is evaluated without leaving the kernel; a finished utterance's workgroup returns at once.  The host reads the
// number of suspended utterances once per round (4 bytes and a stream synchronise): the entry cannot be captured in a graph.
#include "decode_common.h"

#include <cmath>
#include <cstring>

int ec_fail(const char* msg);

using namespace ecrnnt;
using namespace ecdec;

namespace {

constexpr int BT = 512;          // threads per utterance
constexpr int BNW = BT / 64;     // waves
constexpr int MAXC = 16;         // columns of an MFMA tile = largest beam and evaluation batch
constexpr int SLACK = BEAM_SLACK;

enum : int { H_READY = 1, H_POPPED = 2, H_EVAL = 4 };   // flags; bits 4.. hold the evaluation slot

// One hypothesis.  READY: `node` is its decoder output (a carried blank child); otherwise (pending) `node` is its state (-1: zeros) and
// y the token the decoder runs on.  After evaluation `node` is the decoder output in both cases.  `lab` >= 0: a label appended to the
// trail `trail` when the hypothesis is popped (len already counts it).
struct Hyp { float key; float score; int len; int trail; int lab; int y; int node; int flags; };
static_assert(sizeof(Hyp) == BEAM_HYP_BYTES, "Hyp");

size_t beam_lds_bytes(const EcRnntConfig& c) {
    const int H = c.dim_decoder, J = c.dim_joint, P = H > J ? H : J;
    return (size_t)MAXC * (P + H + c.vocab_size) * 4;
}

struct BeamArgs {
    RnntDev w;
    const float* fe; const int64_t* lens; int T, B;
    int nb, max_tok; float tmp;
    char* utt; int* stats; BeamLayout L;
    int* tokens; int* counts; float* score; int* status;
};

// the LM side of the fused search (beam_search<true>); the plain kernel passes an empty one
struct BeamLmSide {
    int4* req;               // [B][16] requests of this round: token, source node (-1: zero state), destination node, live
    int* resume;             // [B][BEAM_LM_RESUME_INTS] loop state of a suspended utterance; [0]: 0 start, 1 suspended, 2 finished
    int* active;             // utterances suspended in this round (cleared before every launch)
    const int* slot;         // [B][16] the row of `logits` a request of the previous round was answered in (lm.hip packs the live requests)
    const float* logits;     // [rows][V] raw LM logits of the previous round's requests
    size_t lmnodes;          // an utterance's LM nodes: [nnodes][nls + V]
    int nls; float w, tmp;   // state floats of a node; lm_weight, lm_tmp
};
enum : int { R_PHASE, R_T, R_NA, R_NB, R_POPS, R_USED, R_NTRAIL, R_NC, R_NBATCH, R_NEVAL, R_NPOP, R_COLS = 16 };
static_assert(R_COLS + MAXC <= BEAM_LM_RESUME_INTS && MAXC == BEAM_LM_COLS, "resume record");

// (v, i) before (bv, bi) in pop order: larger value, then smaller index; i < 0 = none
__device__ __forceinline__ bool before(float v, int i, float bv, int bi) { return i >= 0 && (bi < 0 || v > bv || (v == bv && i < bi)); }

// block-wide first maximum; every thread returns the same (v, i).  Two barriers: callable back to back.
__device__ __forceinline__ void block_best(float& v, int& i, float* s_rv, int* s_ri) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(v, o); const int oi = __shfl_xor(i, o);
        if (before(ov, oi, v, i)) { v = ov; i = oi; }
    }
    if ((threadIdx.x & 63) == 0) { s_rv[threadIdx.x >> 6] = v; s_ri[threadIdx.x >> 6] = i; }
    __syncthreads();
    v = s_rv[0]; i = s_ri[0];
#pragma unroll
    for (int q = 1; q < BNW; ++q)
        if (before(s_rv[q], s_ri[q], v, i)) { v = s_rv[q]; i = s_ri[q]; }
    __syncthreads();
}

// lstm_step16's view of one hypothesis column: a pending column steps from its state node (null: zeros) into its output node and into sy (the mat-vec operand
// of linear_decoder, k-permuted); a ready column only zeroes its sy entries
struct BeamColumn {
    const float* gin; bool live; const float* from; float* to; float* sy; int H;
    __device__ __forceinline__ float c_old(int unit) const { return from ? from[H + unit] : 0.f; }
    __device__ __forceinline__ void put(int unit, float h, float c) const {
        if (live) { to[unit] = h; to[H + unit] = c; }
        sy[kperm(unit)] = h;
    }
};

// The search of one utterance by one workgroup.  LM = false: from the start to the answer.  LM = true: from the start or the saved state to the next evaluation
// batch with pending columns (suspended) or to the answer.
template <bool LM>
__device__ __forceinline__ void beam_search(const BeamArgs& a, const BeamLmSide& m) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const RnntDev& w = a.w;
    const BeamLayout& L = a.L;
    const int H = w.H, J = w.J, V = w.V, P = H > J ? H : J, beam = L.beam, ns = L.ns;
    float* sx = lds;                       // [16][P] LSTM input h, then joint input z (k-permuted, see mfma_rows16)
    float* sy = sx + MAXC * P;             // [16][H] h' (k-permuted)
    float* sl = sy + MAXC * H;             // [16][V] logits / tmp
    __shared__ float s_rv[BNW];
    __shared__ int s_ri[BNW];
    __shared__ int s_col[MAXC], s_cy[MAXC], s_cst[MAXC], s_cout[MAXC], s_cpend[MAXC];
    __shared__ int s_na, s_nb, s_pops, s_used, s_ntrail, s_status;
    __shared__ float s_pscore;
    __shared__ int s_plen, s_ptrail, s_pnode, s_pslot;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
    const int b = blockIdx.x;
    char* base = a.utt + (size_t)b * L.per_utt;
    float* nodes = reinterpret_cast<float*>(base + L.nodes);
    float* topv = reinterpret_cast<float*>(base + L.topv);
    int* topl = reinterpret_cast<int*>(base + L.topl);
    Hyp* A = reinterpret_cast<Hyp*>(base + L.a);
    Hyp* Bh = reinterpret_cast<Hyp*>(base + L.b);
    int2* trail = reinterpret_cast<int2*>(base + L.trail);
    int Tb = (int)a.lens[b];
    Tb = Tb < 0 ? 0 : (Tb > a.T ? a.T : Tb);
    const float* feb = a.fe + (size_t)b * a.T * J;
    int n_batch = 0, n_eval = 0, n_pop = 0;                              // thread 0's counters (workspace statistics)
    float* lmn = LM ? reinterpret_cast<float*>(base + m.lmnodes) : nullptr;
    const int nlm = LM ? m.nls + V : 0;                                  // floats of an LM node: state, then the row
    int* rec = LM ? m.resume + (size_t)b * BEAM_LM_RESUME_INTS : nullptr;
    int t0 = 0, r_nc = 0;
    bool resumed = false;                                                // the selected columns' LM rows were delivered: evaluate them
    if (LM) {
        const int phase = rec[R_PHASE];
        if (phase == 2) return;                                          // finished in an earlier round
        resumed = phase == 1;
    }
    if (LM && resumed) {
        t0 = rec[R_T]; r_nc = rec[R_NC]; n_batch = rec[R_NBATCH]; n_eval = rec[R_NEVAL]; n_pop = rec[R_NPOP];
        if (tid < MAXC) s_col[tid] = rec[R_COLS + tid];
        if (tid == 0) { s_na = rec[R_NA]; s_nb = rec[R_NB]; s_pops = rec[R_POPS]; s_used = rec[R_USED]; s_ntrail = rec[R_NTRAIL]; s_status = 0; }
    } else if (tid == 0) {
        trail[0] = make_int2(0, -1);                                     // prediction [0] (transducer.py:219)
        A[0] = Hyp{0.f, 0.f, 1, 0, -1, 0, -1, 0};                         // score 0, zero state, pending on token 0
        s_na = 1; s_nb = 0; s_pops = 0; s_used = 0; s_ntrail = 1; s_status = 0;
    }
    __syncthreads();

    for (int t = t0; t < Tb; ++t) {
        if (t > 0 && !resumed) {
            // ---- A = B: carry the beam's decoder nodes into this frame's carry set (the other set holds the previous frame's sources)
            const int par = t & 1;
            for (int i = tid; i < beam * ns; i += BT) {
                const int h = i / ns, e = i - h * ns;
                nodes[(size_t)(par * beam + h) * ns + e] = nodes[(size_t)Bh[h].node * ns + e];
            }
            if (LM)                                                      // and their LM nodes: state and row
                for (int i = tid; i < beam * nlm; i += BT) {
                    const int h = i / nlm, e = i - h * nlm;
                    lmn[(size_t)(par * beam + h) * nlm + e] = lmn[(size_t)Bh[h].node * nlm + e];
                }
            __syncthreads();
            if (tid < beam) {
                const Hyp h = Bh[tid];
                A[tid] = Hyp{h.key, h.score, h.len, h.trail, -1, 0, par * beam + tid, H_READY};
            }
            if (tid == 0) { s_na = beam; s_nb = 0; s_pops = 0; s_used = 0; }
            __syncthreads();
        }
        while (true) {
            const int na = s_na, nbh = s_nb, pops = s_pops, used = s_used;
            int best, nc = r_nc;
            bool eval = true;
            if (LM && resumed) {
                best = s_col[0];                                         // the batch selected before the LM step
            } else {
                if (nbh >= beam) break;
                if (pops >= L.maxexp) { if (tid == 0) s_status = 1; break; }
                // ---- the hypothesis the reference pops next: max score / len over A, first in list order (transducer.py:240)
                float bv = -INFINITY; int bi = -1;
                for (int i = tid; i < na; i += BT) {
                    const Hyp& h = A[i];
                    if (!(h.flags & H_POPPED) && before(h.key, i, bv, bi)) { bv = h.key; bi = i; }
                }
                block_best(bv, bi, s_rv, s_ri);
                best = bi;
                eval = !(A[best].flags & H_EVAL);
                if (eval) {
                    // ---- evaluation batch: the best, then the next unevaluated hypotheses in pop order, as far as the frame's slots allow
                    int lim = SLACK + 1 + pops - used;
                    lim = lim < a.nb ? lim : a.nb;
                    nc = 1;
                    if (tid == 0) s_col[0] = best;
                    float pv = bv; int pi = best;
                    while (nc < lim) {
                        float cv = -INFINITY; int ci = -1;
                        for (int i = tid; i < na; i += BT) {
                            const Hyp& h = A[i];
                            if (!(h.flags & (H_POPPED | H_EVAL)) && (h.key < pv || (h.key == pv && i > pi)) && before(h.key, i, cv, ci)) { cv = h.key; ci = i; }
                        }
                        block_best(cv, ci, s_rv, s_ri);
                        if (ci < 0) break;
                        if (tid == 0) s_col[nc] = ci;
                        ++nc;
                        pv = cv; pi = ci;
                    }
                }
            }
            if (eval) {
                __syncthreads();                                         // s_col
                if (tid < MAXC) {
                    int pend = 0, y = 0, st = -1, out = 0;
                    if (tid < nc) {
                        const Hyp h = A[s_col[tid]];
                        pend = !(h.flags & H_READY);
                        y = h.y;
                        st = pend ? h.node : -1;
                        out = pend ? 2 * beam + used + tid : h.node;      // a pending hypothesis gets the frame slot's node
                    }
                    s_cpend[tid] = pend; s_cy[tid] = y; s_cst[tid] = st; s_cout[tid] = out;
                }
                __syncthreads();
                bool anypend = false;
#pragma unroll
                for (int c = 0; c < MAXC; ++c) anypend |= s_cpend[c] != 0;
                if (LM && anypend && !resumed) {
                    // ---- suspended: the pending columns need their LM step first.  One request per column, the loop state, and out
                    if (tid < MAXC) {
                        m.req[(size_t)b * MAXC + tid] = make_int4(s_cy[tid], s_cst[tid], s_cout[tid], s_cpend[tid]);
                        rec[R_COLS + tid] = tid < nc ? s_col[tid] : 0;
                    }
                    if (tid == 0) {
                        rec[R_PHASE] = 1; rec[R_T] = t; rec[R_NA] = na; rec[R_NB] = nbh; rec[R_POPS] = pops; rec[R_USED] = used; rec[R_NTRAIL] = s_ntrail;
                        rec[R_NC] = nc; rec[R_NBATCH] = n_batch; rec[R_NEVAL] = n_eval; rec[R_NPOP] = n_pop;
                        atomicAdd(m.active, 1);
                    }
                    return;
                }
                if (LM && resumed) {
                    // ---- the delivered logits rows -> the nodes' rows (logits_lm / lm_tmp).softmax().log() (transducer.py:267-270), one wave per column
                    for (int c = wave; c < nc; c += BNW) {
                        if (!s_cpend[c]) continue;
                        const float* x = m.logits + (size_t)m.slot[(size_t)b * MAXC + c] * V;
                        float* row = lmn + (size_t)s_cout[c] * nlm + m.nls;
                        float mx = -INFINITY;
                        for (int v = lane; v < V; v += 64) mx = fmaxf(mx, x[v] / m.tmp);
#pragma unroll
                        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
                        float s = 0.f;
                        for (int v = lane; v < V; v += 64) s += expf(x[v] / m.tmp - mx);
#pragma unroll
                        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
                        for (int v = lane; v < V; v += 64) row[v] = logf(expf(x[v] / m.tmp - mx) / s);
                    }
                    resumed = false;
                }
                if (anypend) {
                    // ---- LSTM step of the pending columns: gates = Gin[y] + W_hh h (torch gate order i, f, g, o), 16 units x 4 gates per tile set
                    for (int i = tid; i < MAXC * H; i += BT) {
                        const int c = i / H, k = i - c * H;
                        sx[c * P + kperm(k)] = s_cpend[c] && s_cst[c] >= 0 ? nodes[(size_t)s_cst[c] * ns + k] : 0.f;
                    }
                    __syncthreads();
                    const bool pend = s_cpend[j] != 0;
                    const BeamColumn col{w.gin + (size_t)s_cy[j] * 4 * H, pend, s_cst[j] >= 0 ? nodes + (size_t)s_cst[j] * ns : nullptr,
                                         nodes + (size_t)s_cout[j] * ns, sy + j * H, H};
                    for (int ub = wave; ub < H / 16; ub += BNW) lstm_step16(w, ub, sx + j * P + 4 * g, col);
                    __syncthreads();
                    // ---- linear_decoder(h') of the pending columns
                    for (int tt = wave; tt < J / 16; tt += BNW) {
                        int nrow[1] = {16 * tt + j};
                        f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
                        mfma_rows16_any<1>(w.wd16, J, H / 16, nrow, sy + j * H + 4 * g, acc);
                        if (pend) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int n = 16 * tt + 4 * g + e;
                                nodes[(size_t)s_cout[j] * ns + 2 * H + n] = acc[0][e] + w.bd[n];
                            }
                        }
                    }
                    __syncthreads();
                }
                // ---- joint input z = tanh(linear_encoder(f[t]) + linear_decoder(g)) of every column (unused columns zero)
                for (int i = tid; i < MAXC * J; i += BT) {
                    const int c = i / J, k = i - c * J;
                    sx[c * P + kperm(k)] = c < nc ? tanhf(feb[(size_t)t * J + k] + nodes[(size_t)s_cout[c] * ns + 2 * H + k]) : 0.f;
                }
                __syncthreads();
                // ---- logits = linear_joint(z), divided by the temperature (transducer.py:255)
                for (int tt = wave; tt < (V + 15) / 16; tt += BNW) {
                    const int lr = 16 * tt + j;
                    int nrow[1] = {lr < V ? lr : V - 1};
                    f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
                    mfma_rows16_any<1>(w.wj16, V, J / 16, nrow, sx + j * P + 4 * g, acc);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int n = 16 * tt + 4 * g + e;
                        if (n < V) sl[j * V + n] = (acc[0][e] + w.bj[n]) / a.tmp;
                    }
                }
                __syncthreads();
                // ---- per column: softmax().log() (transducer.py:258) and the top `beam` entries, one wave per column
                for (int c = wave; c < nc; c += BNW) {
                    float* lc = sl + c * V;
                    float mx = -INFINITY;
                    for (int v = lane; v < V; v += 64) mx = fmaxf(mx, lc[v]);
#pragma unroll
                    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
                    float s = 0.f;
                    for (int v = lane; v < V; v += 64) s += expf(lc[v] - mx);
#pragma unroll
                    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
                    if (LM) {
                        // logP += lm_weight * logP_lm over the whole row (transducer.py:273): two roundings, no contraction.  A lane rereads its own entries only
                        const float* lr = lmn + (size_t)s_cout[c] * nlm + m.nls;
                        for (int v = lane; v < V; v += 64) lc[v] = __fadd_rn(logf(expf(lc[v] - mx) / s), __fmul_rn(m.w, lr[v]));
                    }
                    const int slot = used + c;
                    float pv2 = INFINITY; int pi2 = -1;
                    for (int r = 0; r < beam; ++r) {                     // descending, lower label first on equal values
                        float cv = -INFINITY; int ci = -1;
                        for (int v = lane; v < V; v += 64) {
                            const float x = lc[v];
                            if ((x < pv2 || (x == pv2 && v > pi2)) && before(x, v, cv, ci)) { cv = x; ci = v; }
                        }
#pragma unroll
                        for (int o = 32; o >= 1; o >>= 1) {
                            const float ov = __shfl_xor(cv, o); const int oi = __shfl_xor(ci, o);
                            if (before(ov, oi, cv, ci)) { cv = ov; ci = oi; }
                        }
                        if (lane == 0) { topv[(size_t)slot * beam + r] = LM ? cv : logf(expf(cv - mx) / s); topl[(size_t)slot * beam + r] = ci; }
                        pv2 = cv; pi2 = ci;
                    }
                }
                if (tid < nc) {
                    Hyp* h = A + s_col[tid];
                    h->node = s_cout[tid];
                    h->flags |= H_EVAL | ((used + tid) << 4);
                }
                if (tid == 0) { s_used = used + nc; ++n_batch; n_eval += nc; }
                __syncthreads();
            }
            // ---- pop: children in top-k order, blank -> B, labels -> A (transducer.py:280-317)
            if (tid == 0) {
                Hyp h = A[best];
                int tr = h.trail;
                if (h.lab >= 0) { tr = s_ntrail++; trail[tr] = make_int2(h.lab, h.trail); }
                A[best].flags = h.flags | H_POPPED;
                s_pscore = h.score; s_plen = h.len; s_ptrail = tr; s_pnode = h.node; s_pslot = h.flags >> 4;
                ++n_pop;
            }
            __syncthreads();
            if (tid < beam) {
                const int slot = s_pslot;
                const int lab = topl[(size_t)slot * beam + tid];
                const float sc = s_pscore + topv[(size_t)slot * beam + tid];
                if (lab == 0) {
                    Bh[nbh] = Hyp{sc / (float)s_plen, sc, s_plen, s_ptrail, -1, 0, s_pnode, 0};
                } else {
                    int before_me = 0;
                    for (int r = 0; r < tid; ++r) before_me += topl[(size_t)slot * beam + r] != 0;
                    A[na + before_me] = Hyp{sc / (float)(s_plen + 1), sc, s_plen + 1, s_ptrail, lab, lab, s_pnode, 0};
                }
            }
            if (tid == 0) {
                int blank = 0;
                for (int r = 0; r < beam; ++r) blank += topl[(size_t)s_pslot * beam + r] == 0;
                s_na = na + beam - blank; s_nb = nbh + blank; s_pops = pops + 1;
            }
            __syncthreads();
        }
        __syncthreads();                                                 // s_status
        if (s_status) break;
    }
    __syncthreads();
    // ---- answer: max over B by score / len, first in list order (transducer.py:320); no frames: the start hypothesis
    int st = s_status;
    float sc = 0.f; int len = 1, tr = 0;
    if (!st && Tb > 0) {
        float bv = -INFINITY; int bi = -1;
        for (int i = tid; i < beam; i += BT)
            if (before(Bh[i].key, i, bv, bi)) { bv = Bh[i].key; bi = i; }
        block_best(bv, bi, s_rv, s_ri);
        sc = Bh[bi].score; len = Bh[bi].len; tr = Bh[bi].trail;
    }
    int ntok = len - 1;
    if (!st && ntok > a.max_tok) st = 2;
    if (st) { ntok = 0; sc = 0.f; }
    int* out = a.tokens + (size_t)b * a.max_tok;
    if (tid == 0) {
        for (int i = ntok - 1; i >= 0; --i) { const int2 e = trail[tr]; out[i] = e.x; tr = e.y; }
        a.counts[b] = ntok; a.score[b] = sc; a.status[b] = st;
        a.stats[4 * b + 0] = n_batch; a.stats[4 * b + 1] = n_eval; a.stats[4 * b + 2] = n_pop; a.stats[4 * b + 3] = Tb;
    }
    for (int i = ntok + tid; i < a.max_tok; i += BT) out[i] = 0;
    if (LM) {                                                            // finished: no request of this utterance is live in any later round
        if (tid < MAXC) m.req[(size_t)b * MAXC + tid] = make_int4(0, -1, 0, 0);
        if (tid == 0) rec[R_PHASE] = 2;
    }
}

__global__ __launch_bounds__(BT) void rnnt_beam_kernel(const BeamArgs a) { beam_search<false>(a, BeamLmSide{}); }

__global__ __launch_bounds__(BT) void rnnt_beam_lm_kernel(const BeamArgs a, const BeamLmSide m) { beam_search<true>(a, m); }

const char* beam_check(const EcRnnt* r, int32_t batch, int32_t t_out, int32_t beam, int32_t max_expansions, int32_t max_tokens) {
    if (!r) return "null handle";
    if (!beam_dims_supported(r->cfg)) return "beam search: decoder and joint widths must be multiples of 16";
    if (beam_lds_bytes(r->cfg) > 160 * 1024 - 1024) return "beam search: decoder / joint / vocabulary widths exceed the LDS of one workgroup";
    if (beam < 1 || beam > MAXC || beam > r->cfg.vocab_size) return "beam search: beam must be in 1 .. min(16, vocab_size)";
    if (max_expansions < 1 || max_expansions > (1 << 16)) return "beam search: max_expansions must be in 1 .. 65536";
    if (max_tokens < 1) return "beam search: max_tokens must be >= 1";
    if (batch < 0 || t_out < 1) return "beam search: bad shape";
    if ((int64_t)t_out * max_expansions >= (1ll << 30)) return "beam search: t_out * max_expansions too large";
    return nullptr;
}

// the fused entry's own rules, after beam_check; *mc: the LM's config
const char* beam_lm_check(const EcRnnt* r, const EcLm* lm, bool finalized, int32_t batch, const EcLmConfig** mc) {
    *mc = lm_handle_config(lm, finalized);
    if (!*mc) return "beam search: lm handle not finalized";
    if ((*mc)->vocab_size != r->cfg.vocab_size) return "beam search: the LM's vocab_size differs from the transducer's";
    if ((int64_t)batch * MAXC > (1 << 21)) return "beam search: at most 2^17 utterances per call with an LM";
    return nullptr;
}

}  // namespace

extern "C" {

size_t effconf_rnnt_beam_lm_workspace_bytes(const EcRnnt* r, const EcLm* lm, int32_t batch, int32_t t_out, int32_t beam, int32_t max_expansions,
                                            int32_t max_tokens) {
    if (const char* e = beam_check(r, batch, t_out, beam, max_expansions, max_tokens)) { ec_fail(e); return 0; }
    const EcLmConfig* mc;
    if (const char* e = beam_lm_check(r, lm, false, batch, &mc)) { ec_fail(e); return 0; }
    return beam_lm_layout(r->cfg, *mc, batch, t_out, beam, max_expansions).total;
}

int effconf_rnnt_beam_lm(EcRnnt* r, EcLm* lm, const float* enc_out, const int64_t* out_len, int32_t batch, int32_t t_out, int32_t beam, float temperature,
                         float lm_weight, float lm_tmp, int32_t max_expansions, int32_t* tokens, int32_t* token_len, float* score, int32_t* status,
                         int32_t max_tokens, int32_t* rounds_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!r || !r->finalized) return ec_fail("rnnt handle not finalized");
    if (const char* e = beam_check(r, batch, t_out, beam, max_expansions, max_tokens)) return ec_fail(e);
    const EcLmConfig* mc;
    if (const char* e = beam_lm_check(r, lm, true, batch, &mc)) return ec_fail(e);
    if (!(temperature > 0.f) || !std::isfinite(temperature)) return ec_fail("beam search: temperature must be > 0");
    if (!(lm_weight > 0.f) || !std::isfinite(lm_weight)) return ec_fail("beam search: lm_weight must be > 0 (0: effconf_rnnt_beam)");
    if (!(lm_tmp > 0.f) || !std::isfinite(lm_tmp)) return ec_fail("beam search: lm_tmp must be > 0");
    if (rounds_out) *rounds_out = 0;
    if (batch == 0) return 0;
    if (!enc_out || !out_len || !tokens || !token_len || !score || !status || !workspace) return ec_fail("null argument");
    if (!r->dev.whh16 || !r->dev.wd16 || !r->dev.wj16) return ec_fail("beam search: MFMA weight images missing (finalize)");
    const BeamLmLayout L = beam_lm_layout(r->cfg, *mc, batch, t_out, beam, max_expansions);
    if (workspace_bytes < L.total) return ec_fail("workspace too small (effconf_rnnt_beam_lm_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    const int J = r->cfg.dim_joint, De = r->cfg.dim_encoder;
    char* ws = WsPlan::base(workspace);
    float* fe = reinterpret_cast<float*>(ws + L.s.fe);
    if (launch_sgemm_nt(enc_out, De, r->we, De, r->be, fe, J, batch * t_out, J, De, s) != 0) return ec_fail("linear_encoder GEMM launch failed");
    BeamArgs a{};
    a.w = r->dev; a.fe = fe; a.lens = out_len; a.T = t_out; a.B = batch;
    a.nb = r->beam_eval_batch < MAXC ? r->beam_eval_batch : MAXC; a.max_tok = max_tokens; a.tmp = temperature;
    a.utt = ws + L.s.utt; a.stats = reinterpret_cast<int*>(ws + L.s.stats); a.L = L.s;
    a.tokens = tokens; a.counts = token_len; a.score = score; a.status = status;
    BeamLmSide m{};
    m.req = reinterpret_cast<int4*>(ws + L.req); m.resume = reinterpret_cast<int*>(ws + L.resume); m.active = reinterpret_cast<int*>(ws + L.counter);
    m.slot = reinterpret_cast<const int*>(ws + L.slot); m.logits = reinterpret_cast<const float*>(ws + L.logits); m.lmnodes = L.lmnodes; m.nls = L.nls; m.w = lm_weight; m.tmp = lm_tmp;
    LmColumns col{};
    col.req = m.req; col.ncol = batch * MAXC; col.cols_per_utt = MAXC; col.slot = reinterpret_cast<int*>(ws + L.slot); col.utt = a.utt; col.per_utt = L.s.per_utt; col.lmnodes = L.lmnodes;
    col.node_floats = L.nls + L.vocab; col.logits = reinterpret_cast<float*>(ws + L.logits);
    const size_t lds = beam_lds_bytes(r->cfg);
    static LdsAttr attr;
    ensure_dynamic_lds(reinterpret_cast<const void*>(&rnnt_beam_lm_kernel), (int)lds, attr);
    if (hipMemsetAsync(m.resume, 0, (size_t)batch * BEAM_LM_RESUME_INTS * 4, s) != hipSuccess) return ec_fail("beam search: clearing the resume records failed");
    // every round pops at least one hypothesis of every utterance that is still searching; the last round finds nothing suspended
    const int64_t bound = (int64_t)t_out * ((int64_t)max_expansions + 1) + 1;
    for (int64_t round = 0;; ++round) {
        if (round > bound) return ec_fail("beam search: the rounds did not end (internal error)");
        if (hipMemsetAsync(m.active, 0, 4, s) != hipSuccess) return ec_fail("beam search: clearing the round counter failed");
        hipLaunchKernelGGL(rnnt_beam_lm_kernel, dim3(batch), dim3(BT), lds, s, a, m);
        if (hipGetLastError() != hipSuccess) return ec_fail("rnnt_beam_lm launch failed");
        int active = 0;
        if (hipMemcpyAsync(&active, m.active, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return ec_fail("beam search: reading the round counter failed");
        if (rounds_out) *rounds_out = (int32_t)(round + 1);
        if (active == 0) return 0;
        if (lm_columns_step(lm, col, ws + L.lm, s) != 0) return ec_fail("beam search: LM step launch failed");
    }
}


size_t effconf_rnnt_beam_workspace_bytes(const EcRnnt* r, int32_t batch, int32_t t_out, int32_t beam, int32_t max_expansions, int32_t max_tokens) {
    if (const char* e = beam_check(r, batch, t_out, beam, max_expansions, max_tokens)) { ec_fail(e); return 0; }
    return beam_layout(r->cfg, batch, t_out, beam, max_expansions).total;
}

int effconf_rnnt_beam(EcRnnt* r, const float* enc_out, const int64_t* out_len, int32_t batch, int32_t t_out, int32_t beam, float temperature,
                      int32_t max_expansions, int32_t* tokens, int32_t* token_len, float* score, int32_t* status, int32_t max_tokens,
                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!r || !r->finalized) return ec_fail("rnnt handle not finalized");
    if (const char* e = beam_check(r, batch, t_out, beam, max_expansions, max_tokens)) return ec_fail(e);
    if (!(temperature > 0.f) || !std::isfinite(temperature)) return ec_fail("beam search: temperature must be > 0");
    if (batch == 0) return 0;
    if (!enc_out || !out_len || !tokens || !token_len || !score || !status || !workspace) return ec_fail("null argument");
    if (!r->dev.whh16 || !r->dev.wd16 || !r->dev.wj16) return ec_fail("beam search: MFMA weight images missing (finalize)");
    const BeamLayout L = beam_layout(r->cfg, batch, t_out, beam, max_expansions);
    if (workspace_bytes < L.total) return ec_fail("workspace too small (effconf_rnnt_beam_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    const int J = r->cfg.dim_joint, De = r->cfg.dim_encoder;
    char* ws = WsPlan::base(workspace);
    float* fe = reinterpret_cast<float*>(ws + L.fe);
    // linear_encoder(f) for every frame of the batch, once (joint_networks.py:82 recomputes it per decision)
    if (launch_sgemm_nt(enc_out, De, r->we, De, r->be, fe, J, batch * t_out, J, De, s) != 0) return ec_fail("linear_encoder GEMM launch failed");
    BeamArgs a{};
    a.w = r->dev; a.fe = fe; a.lens = out_len; a.T = t_out; a.B = batch;
    a.nb = r->beam_eval_batch < MAXC ? r->beam_eval_batch : MAXC; a.max_tok = max_tokens; a.tmp = temperature;
    a.utt = ws + L.utt; a.stats = reinterpret_cast<int*>(ws + L.stats); a.L = L;
    a.tokens = tokens; a.counts = token_len; a.score = score; a.status = status;
    const size_t lds = beam_lds_bytes(r->cfg);
    static LdsAttr attr;
    ensure_dynamic_lds(reinterpret_cast<const void*>(&rnnt_beam_kernel), (int)lds, attr);
    hipLaunchKernelGGL(rnnt_beam_kernel, dim3(batch), dim3(BT), lds, s, a);
    return hipGetLastError() == hipSuccess ? 0 : ec_fail("rnnt_beam launch failed");
}

}  // extern "C"
