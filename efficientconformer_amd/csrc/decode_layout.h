// Workspace layouts of the seven decoder files (rnnt.hip, rnnt_beam.hip, rnnt_lattice.hip, rnnt_align.hip, lm.hip, ctc_beam.hip, ctc_align.hip), written on
// one plan type.  Plain C++ without a HIP call: every `effconf_*_workspace_bytes` and every entry point's carve read the same function, and
// tools/decoder_layout_sanitize.cpp compiles this header for the host alone.
//
// The rule, once: a region starts at a multiple of 256 bytes from the base; the base is the caller's pointer aligned up to 256 bytes (once); the size an entry
// reports is the end of the last region plus ONE 256-byte slack, which that alignment can spend at the most.
#pragma once
#include "../../include/effconf.h"

#include <cstddef>
#include <cstdint>

namespace ecdec {

struct WsPlan {
    size_t end = 0;
    static size_t up(size_t x) { return (x + 255) & ~(size_t)255; }
    size_t take(size_t bytes) { const size_t off = up(end); end = off + bytes; return off; }
    size_t stride() const { return up(end); }                        // a sub-plan (one utterance's regions) as the element of an array
    size_t total() const { return end + 256; }
    static char* base(void* p) { return reinterpret_cast<char*>(up(reinterpret_cast<uintptr_t>(p))); }
};

// ---------------------------------------------------------------------------------------------------------------- rnnt.hip: greedy
// fe = linear_encoder(f) [B][T][J]; cluster decode <CW workgroups, CU utterances, CKF frames> adds, per cluster: one barrier counter per 256-byte line, then ONE
// status word behind the counters (sync: cleared by one memset before every launch), and the exchange buffers of h, linear_decoder(h) and the argmax candidates.
struct GreedyLayout { int ncl; size_t fe, sync, status, sync_bytes, xh, xgd, xav, xai, total; };

inline GreedyLayout greedy_layout(const EcRnntConfig& c, int batch, int t_out, int CW, int CU, int CKF) {
    GreedyLayout L{};
    WsPlan p;
    L.ncl = (batch + CU - 1) / CU;
    L.fe = p.take((size_t)batch * t_out * c.dim_joint * 4);
    L.sync_bytes = (size_t)L.ncl * 256 + 256;
    L.sync = p.take(L.sync_bytes);
    L.status = L.sync + (size_t)L.ncl * 256;
    L.xh = p.take((size_t)L.ncl * CU * c.dim_decoder * 4);
    L.xgd = p.take((size_t)L.ncl * CU * c.dim_joint * 4);
    L.xav = p.take((size_t)L.ncl * CW * CU * CKF * 4);
    L.xai = p.take((size_t)L.ncl * CW * CU * CKF * 4);
    L.total = p.total();
    return L;
}

// ---------------------------------------------------------------------------------------------------------------- rnnt.hip: greedy, resumed per stream
// The caller's state buffer: i32 primed[max_streams], then one record per stream, rec_bytes apart: f32 h[H], c[H], gd[J] = linear_decoder(h) + bias.  The workspace
// of a push is its fe = linear_encoder(f) [n][t_new][J] alone.
struct RnntStreamLayout { size_t primed, rec, rec_bytes, total; };

inline RnntStreamLayout rnnt_stream_layout(const EcRnntConfig& c, int max_streams) {
    RnntStreamLayout L{};
    WsPlan u;                                                            // one stream
    u.take(((size_t)2 * c.dim_decoder + c.dim_joint) * 4);
    L.rec_bytes = u.stride();
    WsPlan p;
    L.primed = p.take((size_t)max_streams * 4);
    L.rec = p.take((size_t)max_streams * L.rec_bytes);
    L.total = p.total();
    return L;
}

struct RnntStreamWs { size_t fe, total; };

inline RnntStreamWs rnnt_stream_ws(const EcRnntConfig& c, int n, int t_new) {
    RnntStreamWs L{};
    WsPlan p;
    L.fe = p.take((size_t)n * t_new * c.dim_joint * 4);
    L.total = p.total();
    return L;
}

// ---------------------------------------------------------------------------------------------------------------- rnnt_beam.hip
constexpr int BEAM_SLACK = 64;      // evaluated, not yet popped hypotheses per frame (room for evaluating ahead of the pops)
constexpr int BEAM_HYP_BYTES = 32;  // sizeof(Hyp)

struct BeamLayout {
    int beam, maxexp, ecap, acap, tcap, ns, nnodes;
    size_t stats, fe, utt, per_utt;                                      // byte offsets / stride
    size_t nodes, topv, topl, a, b, trail, total;
};

// one utterance's regions of the search on the plan `u` (beam_layout and beam_lm_layout continue from here)
inline void beam_utt_regions(BeamLayout& L, WsPlan& u, const EcRnntConfig& c, int t_out, int beam, int maxexp) {
    L.beam = beam; L.maxexp = maxexp;
    L.ecap = maxexp + BEAM_SLACK;                                        // evaluations per frame: one per pop + the slack
    L.acap = beam + maxexp * beam;                                       // A: the carried beam + beam children per pop
    L.tcap = 1 + t_out * maxexp;                                         // trail: the start token + one entry per pop
    L.ns = 2 * c.dim_decoder + c.dim_joint;                              // node: h', c', linear_decoder(h')
    L.nnodes = 2 * beam + L.ecap;                                        // two carry sets (previous / next frame) + the frame's arena
    L.nodes = u.take((size_t)L.nnodes * L.ns * 4);
    L.topv = u.take((size_t)L.ecap * beam * 4);
    L.topl = u.take((size_t)L.ecap * beam * 4);
    L.a = u.take((size_t)L.acap * BEAM_HYP_BYTES);
    L.b = u.take((size_t)beam * BEAM_HYP_BYTES);
    L.trail = u.take((size_t)L.tcap * 8);
}

inline BeamLayout beam_layout(const EcRnntConfig& c, int batch, int t_out, int beam, int maxexp) {
    BeamLayout L{};
    WsPlan u;                                                            // one utterance
    beam_utt_regions(L, u, c, t_out, beam, maxexp);
    L.per_utt = u.stride();
    WsPlan p;
    L.stats = p.take((size_t)batch * 16);
    L.fe = p.take((size_t)batch * t_out * c.dim_joint * 4);
    L.utt = p.take((size_t)batch * L.per_utt);
    L.total = p.total();
    return L;
}

// ---------------------------------------------------------------------------------------------------------------- rnnt_lattice.hip
struct LatLayout { size_t tlen, ulen, start, h, gd, fe, total; };        // byte offsets

inline LatLayout lat_layout(const EcRnntConfig& c, int batch, int t_out, int u_max) {
    LatLayout L{};
    WsPlan p;
    L.tlen = p.take((size_t)batch * 4);
    L.ulen = p.take((size_t)batch * 4);
    L.start = p.take(((size_t)batch + 1) * 4);
    L.h = p.take((size_t)batch * (u_max + 1) * c.dim_decoder * 4);
    L.gd = p.take((size_t)batch * (u_max + 1) * c.dim_joint * 4);
    L.fe = p.take(WsPlan::up((size_t)batch * t_out * c.dim_joint * 4));   // rounded: the size this entry has reported since it exists
    L.total = p.total();
    return L;
}

// ---------------------------------------------------------------------------------------------------------------- rnnt_align.hip
struct RnntAlignLayout { int wpu; size_t bp, bp_utt, total; };           // back-pointer words per column, byte offsets

inline RnntAlignLayout rnnt_align_layout(int batch, int t_out, int u_max) {
    RnntAlignLayout L{};
    L.wpu = (t_out + 31) / 32;
    WsPlan u;
    u.take((size_t)(u_max + 1) * L.wpu * 4);
    L.bp_utt = u.stride();
    WsPlan p;
    L.bp = p.take((size_t)batch * L.bp_utt);
    L.total = p.total();
    return L;
}

// ---------------------------------------------------------------------------------------------------------------- lm.hip
constexpr int LM_NPADQ = 64;        // the state holds the sequences rounded up to this many columns: every column tile a kernel touches exists
inline int lm_npad(int n) { return (n + LM_NPADQ - 1) / LM_NPADQ * LM_NPADQ; }

// i32 ulen[n]; then per layer l: h[l][2][Np][H] (k-permuted), c[l][Np][H]
struct LmLayout { size_t ulen, state, layer, total; };

inline LmLayout lm_layout(const EcLmConfig& c, int n) {
    LmLayout L{};
    WsPlan p;
    L.ulen = p.take((size_t)n * 4);
    L.layer = (size_t)3 * lm_npad(n) * c.dim_model * 4;
    L.state = p.take((size_t)c.num_layers * L.layer);
    L.total = p.total();
    return L;
}

// ---------------------------------------------------------------------------------------------------------------- rnnt_beam.hip with a neural LM (shallow fusion)
// The search's regions, and per utterance an LM node array on the index space of the decoder nodes: node = the LM's state after the hypothesis' last token
// ([layer][h k-permuted | c], 2 * layers * dim_model floats), then its row lm_weight is applied to (vocab floats).  Per call: one request (token, source node,
// destination node, live) per column, BEAM_LM_COLS columns per utterance, and its packed column + the packed columns' tokens (slot); one resume record per utterance; the round's counter of suspended utterances; the
// dense state of one LM step over batch * BEAM_LM_COLS columns (lm_layout) and its raw logits rows.
constexpr int BEAM_LM_COLS = 16;          // columns of an evaluation batch at the most
constexpr int BEAM_LM_RESUME_INTS = 32;   // phase, frame, na, nb, pops, used, ntrail, status, columns, three counters, then the selected columns

struct BeamLmLayout {
    BeamLayout s;                                                        // s.total is not set: `total` below is the call's size
    int nls, vocab;                                                      // floats of an LM node's state; its row follows
    size_t lmnodes;                                                      // inside an utterance
    size_t req, slot, resume, counter, lm, logits, total;
    LmLayout lml;                                                        // offsets from `lm`
};

inline BeamLmLayout beam_lm_layout(const EcRnntConfig& c, const EcLmConfig& m, int batch, int t_out, int beam, int maxexp) {
    BeamLmLayout L{};
    WsPlan u;
    beam_utt_regions(L.s, u, c, t_out, beam, maxexp);
    L.nls = 2 * m.num_layers * m.dim_model;
    L.vocab = m.vocab_size;
    L.lmnodes = u.take((size_t)L.s.nnodes * (L.nls + L.vocab) * 4);
    L.s.per_utt = u.stride();
    const int ncol = batch * BEAM_LM_COLS;
    L.lml = lm_layout(m, ncol);
    WsPlan p;
    L.s.stats = p.take((size_t)batch * 16);
    L.s.fe = p.take((size_t)batch * t_out * c.dim_joint * 4);
    L.s.utt = p.take((size_t)batch * L.s.per_utt);
    L.req = p.take((size_t)ncol * 16);
    L.slot = p.take((size_t)ncol * 8);
    L.resume = p.take((size_t)batch * BEAM_LM_RESUME_INTS * 4);
    L.counter = p.take(4);
    L.lm = p.take(L.lml.total - 256);                                    // a sub-plan: its own slack is not needed inside an aligned region
    L.logits = p.take((size_t)ncol * m.vocab_size * 4);
    L.total = p.total();
    return L;
}

// ---------------------------------------------------------------------------------------------------------------- ctc_beam.hip
struct CtcBeamLayout {
    int ncap, hcap;                               // trie nodes, hash slots per utterance
    size_t stats, utt, per_utt, trace, nodes, hkeys, hvals, total;
};

inline CtcBeamLayout ctc_beam_layout(int batch, int t_out, int beam) {
    CtcBeamLayout L{};
    L.ncap = 1 + beam * t_out;                    // the empty prefix + at most `beam` new prefixes per frame
    int h = 1;
    while (h < 2 * L.ncap) h <<= 1;
    L.hcap = h;
    WsPlan u;                                     // one utterance
    L.trace = u.take((size_t)t_out * beam * 16);
    L.nodes = u.take((size_t)L.ncap * 16);
    L.hkeys = u.take((size_t)h * 8);
    L.hvals = u.take((size_t)h * 4);
    L.per_utt = u.stride();
    WsPlan p;
    L.stats = p.take((size_t)batch * 16);
    L.utt = p.take((size_t)batch * L.per_utt);
    L.total = p.total();
    return L;
}

// ---------------------------------------------------------------------------------------------------------------- ctc_beam.hip: the plain search, resumed per stream
// The beam as a record, defined once for the two searches that carry a beam from one launch to the next: a head of CTC_REC_HEAD i32 (the enum; the rest unused),
// then [CTC_BEAM_MAXB] each of the members' node, last token, parent node, depth (i32), pb, pnb, s (f32) in rank order - CTC_BEAM_REC_INTS, the record of a stream,
// whose bytes include/effconf.h documents - and then, for the fused search alone, L (f32), LM slot and row pending (i32): CTC_BEAM_LM_REC_INTS.
constexpr int CTC_BEAM_MAXB = 32;                                        // ctc_beam_search.h's largest beam
enum : int { CTC_REC_FRAMES = 0,                                         // frames consumed: where the next launch goes on
             CTC_REC_N, CTC_REC_NN, CTC_REC_NCLO, CTC_REC_NCHI,          // members, trie nodes, candidates scored (lo, hi)
             CTC_REC_PHASE, CTC_REC_NREQ,                                // the fused search: 0 start (the entry's memset), 1 suspended, 2 finished; LM rows asked for
             CTC_REC_HEAD = 16 };
constexpr int CTC_BEAM_REC_INTS = CTC_REC_HEAD + 7 * CTC_BEAM_MAXB;
constexpr int CTC_BEAM_LM_REC_INTS = CTC_BEAM_REC_INTS + 3 * CTC_BEAM_MAXB;

// The caller's state buffer: i32 primed[max_streams], then one block per stream, per_stream apart: the record (CTC_BEAM_REC_INTS i32) and the stream's trie - nodes
// int4 [ncap], hash keys u64 [hcap], hash nodes i32 [hcap], ncap = 1 + beam * max_frames, hcap as ctc_beam_layout's.  The workspace of a push: stats[n][4] and its
// trace [t_new][beam] int4 per listed stream.

struct CtcBeamStreamLayout {
    int ncap, hcap;
    size_t primed, blocks, per_stream, rec, nodes, hkeys, hvals, total;  // rec .. hvals: inside a stream's block
};

inline CtcBeamStreamLayout ctc_beam_stream_layout(int max_streams, int max_frames, int beam) {
    CtcBeamStreamLayout L{};
    L.ncap = 1 + beam * max_frames;
    int h = 1;
    while (h < 2 * L.ncap) h <<= 1;
    L.hcap = h;
    WsPlan u;                                     // one stream
    L.rec = u.take((size_t)CTC_BEAM_REC_INTS * 4);
    L.nodes = u.take((size_t)L.ncap * 16);
    L.hkeys = u.take((size_t)h * 8);
    L.hvals = u.take((size_t)h * 4);
    L.per_stream = u.stride();
    WsPlan p;
    L.primed = p.take((size_t)max_streams * 4);
    L.blocks = p.take((size_t)max_streams * L.per_stream);
    L.total = p.total();
    return L;
}

struct CtcBeamStreamWs { size_t stats, trace, per_trace, total; };

inline CtcBeamStreamWs ctc_beam_stream_ws(int n, int t_new, int beam) {
    CtcBeamStreamWs L{};
    WsPlan u;                                     // one listed stream
    u.take((size_t)t_new * beam * 16);
    L.per_trace = u.stride();
    WsPlan p;
    L.stats = p.take((size_t)n * 16);
    L.trace = p.take((size_t)n * L.per_trace);
    L.total = p.total();
    return L;
}

// ---------------------------------------------------------------------------------------------------------------- ctc_beam.hip with a neural LM (shallow fusion)
// The search's regions, and per utterance: a second trace {f32 L, f32 total} per frame and rank, and 2 * beam + 1 LM slots of the node layout lm_columns_step
// reads and writes ([layer][h k-permuted | c], 2 * layers * dim_model floats, then the slot's row: vocab floats).  Per call: one request (token, source slot,
// destination slot, live) per rank of every utterance's beam with its packed column + the packed columns' tokens (slot); one record of CTC_BEAM_LM_REC_INTS per
// utterance; the round's counter of suspended utterances; the dense state of one LM step over batch * beam columns (lm_layout) and its raw logits rows.

struct CtcBeamLmLayout {
    CtcBeamLayout s;                                                     // s.total is not set: `total` below is the call's size
    int nls, vocab, nslots;                                              // floats of an LM slot's state (its row follows), slots per utterance
    size_t trace2, lmnodes;                                              // inside an utterance
    size_t req, slot, resume, counter, lm, logits, total;
    LmLayout lml;                                                        // offsets from `lm`
};

inline CtcBeamLmLayout ctc_beam_lm_layout(const EcLmConfig& m, int batch, int t_out, int beam) {
    CtcBeamLmLayout L{};
    L.s = ctc_beam_layout(batch, t_out, beam);
    WsPlan u;                                                            // one utterance: the plain search's regions at their offsets, then the LM's
    u.take(L.s.per_utt);
    L.nls = 2 * m.num_layers * m.dim_model;
    L.vocab = m.vocab_size;
    L.nslots = 2 * beam + 1;
    L.trace2 = u.take((size_t)t_out * beam * 8);
    L.lmnodes = u.take((size_t)L.nslots * (L.nls + L.vocab) * 4);
    L.s.per_utt = u.stride();
    const int ncol = batch * beam;
    L.lml = lm_layout(m, ncol);
    WsPlan p;
    L.s.stats = p.take((size_t)batch * 16);
    L.s.utt = p.take((size_t)batch * L.s.per_utt);
    L.req = p.take((size_t)ncol * 16);
    L.slot = p.take((size_t)ncol * 8);
    L.resume = p.take((size_t)batch * CTC_BEAM_LM_REC_INTS * 4);
    L.counter = p.take(4);
    L.lm = p.take(L.lml.total - 256);                                    // a sub-plan: its own slack is not needed inside an aligned region
    L.logits = p.take((size_t)ncol * m.vocab_size * 4);
    L.total = p.total();
    return L;
}

// ---------------------------------------------------------------------------------------------------------------- ctc_align.hip
constexpr int CTC_ALIGN_THREADS = 256;            // threads per utterance

inline int ctc_align_spt(int u_max) {             // the launch's states per thread: 1, 2, 4, 8 or 16
    const int s = 2 * u_max + 1;
    int spt = 1;
    while (CTC_ALIGN_THREADS * spt < s) spt <<= 1;
    return spt;
}

struct CtcAlignLayout {
    int E, spt, rbmax;                            // emission row stride, states per thread at the most, backpointer bytes per frame at the most
    size_t emit, path, bp, bp_utt, total;
};

inline CtcAlignLayout ctc_align_layout(int batch, int t_out, int u_max) {
    CtcAlignLayout L{};
    L.E = u_max + 1;
    L.spt = ctc_align_spt(u_max);
    L.rbmax = CTC_ALIGN_THREADS * ((L.spt + 3) / 4);
    WsPlan u;
    u.take((size_t)t_out * L.rbmax);
    L.bp_utt = u.stride();
    WsPlan p;
    L.emit = p.take((size_t)batch * t_out * L.E * 4);
    L.path = p.take((size_t)batch * t_out * 4);
    L.bp = p.take((size_t)batch * L.bp_utt);
    L.total = p.total();
    return L;
}

}  // namespace ecdec
