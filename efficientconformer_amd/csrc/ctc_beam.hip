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
//
// With a neural LM (effconf_ctc_beam_lm, ctc_beam_lm_kernel: ctc_beam_search<true, false>): candidates are ranked by
//   total(Q) = s(Q) + lm_weight * L(Q) + length_bonus * |Q|      (fp32, every operation rounded on its own, in that order)
// with L(()) = 0, L(P c) = L(P) + row_P[c], row_P = log softmax(fc(h_P) / lm_tmp), h_P the LSTM state after [0] + P.  L is stored in the trie node when the
// node is created, so every later use of the prefix sees the same bits.  The acoustic recursion is untouched.
//   * Exact pruning: a member's plain extensions score total(P) + lp[c] + w row_P[c] + bonus (up to rounding): only its `beam` best by a_P[c] = lp[c] + w row_P[c]
//     can survive.  The select is per member (one wave per member: `beam` rounds of a wave-wide maximum over the plain tokens, order a desc, id asc); the
//     frame-global top-K is not used.  Rows are read from the member's LM slot in global memory (L2), never staged in LDS.
//   * LM slots: an utterance has 2 beam + 1 slots of the node layout ecdec::lm_columns_step reads and writes (state, then the row).  Slot 0 is the empty
//     prefix's for the whole call.  A member keeps its slot while it stays in the beam; a candidate that enters the beam as an extension takes the lowest slot
//     of 1 .. 2 beam that no member of the OLD beam holds (its parent is one of them and must stay valid until the LM step has run; the survivors are among
//     them too).  The old beam holds at most `beam` of these slots and at most `beam` candidates enter, so 2 beam slots plus the root always suffice.
//   * Rounds: when a frame's new beam holds members without a row, the workgroup saves its beam to its record (decode_layout.h), writes one request (token, parent's
//     slot, its slot, live) per rank, counts itself in the round counter and exits; the host runs ONE LM step for the requests of all utterances and
//     launches again.  On resume the raw logits rows are turned into log-softmax rows in the slots (one wave per row).  An utterance whose new beam needs no
//     LM goes on in the same launch; a finished utterance's workgroup returns at once; the hash index is initialised in the first launch only.
//
// Resumed per stream (effconf_ctc_beam_resume, ctc_beam_resume_kernel: ctc_beam_search<false, true>): the plain search over the frames of one
// push.  The search never looks ahead, so all it knows after a frame is the beam (per member: node, last token, parent, depth, pb, pnb, s) and the append-only trie
// with its hash; both live in the stream's block of a caller-provided state buffer and outlive the call, so the beam after any pushes is bit for bit the beam of one
// whole call.  A push's frames and trace are push-local; the trie is sized for max_frames frames of the stream.  Outputs: the ranks' tokens, lengths and scores as
// the beam stands, and stable_len - the length of the common prefix of ALL members, which every later hypothesis begins with.
#include "ctc_beam_search.h"

#include <cmath>

int ec_fail(const char* msg);

using namespace ecctc;

namespace {

const char* ctc_beam_check(int32_t batch, int32_t t_out, int32_t vocab, int32_t beam) {
    if (beam < 1 || beam > MAXB) return "ctc beam search: beam must be in 1 .. 32";
    if (vocab < 2 || vocab > MAXV) return "ctc beam search: vocab must be in 2 .. 1024";
    if (batch < 0 || t_out < 0) return "ctc beam search: bad shape";
    if ((int64_t)beam * t_out >= (1ll << 24)) return "ctc beam search: beam * t_out too large";
    return nullptr;
}

// the shape of a stream state: ctc_beam_check's limits with max_frames in t_out's place
const char* ctc_beam_stream_check(int32_t max_streams, int32_t max_frames, int32_t beam) {
    if (max_streams < 1) return "ctc beam search: max_streams must be >= 1";
    if (max_frames < 1) return "ctc beam search: max_frames must be >= 1";
    if (max_streams > (1 << 20)) return "ctc beam search: max_streams must be at most 2^20";
    return ctc_beam_check(0, max_frames, 2, beam);
}

const char* ctc_beam_tmp_check(float temperature) {
    return temperature > 0.f && std::isfinite(temperature) ? nullptr : "ctc beam search: temperature must be > 0";
}

// what every entry passes to the search; the workspace side (utt, stats, L) is the entry's own
CtcBeamArgs ctc_beam_args(const float* logits, const int64_t* lens, int32_t t, int32_t vocab, int32_t beam, float temperature, int32_t* tokens,
                          int32_t* token_len, float* score) {
    CtcBeamArgs a{};
    a.logits = logits; a.lens = lens; a.T = t; a.V = vocab; a.beam = beam; a.tmp = temperature;
    a.tokens = tokens; a.token_len = token_len; a.score = score;
    return a;
}

__global__ __launch_bounds__(CT) void ctc_beam_kernel(const CtcBeamArgs a) { ctc_beam_search<false, false>(a, CtcLmSide{}, CtcStreamSide{}); }

__global__ __launch_bounds__(CT) void ctc_beam_lm_kernel(const CtcBeamArgs a, const CtcLmSide fz) { ctc_beam_search<true, false>(a, fz, CtcStreamSide{}); }

// one workgroup per listed stream: the plain search over the push's frames, from and to the stream's record
__global__ __launch_bounds__(CT) void ctc_beam_resume_kernel(const CtcBeamArgs a, const CtcStreamSide sz) { ctc_beam_search<false, true>(a, CtcLmSide{}, sz); }

// before the first search launch: every utterance asks for the empty prefix's row, request (token 0, no source, slot 0) at rank 0
__global__ __launch_bounds__(256) void ctc_beam_lm_root_kernel(int4* req, int ncol, int beam) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < ncol) req[i] = i % beam == 0 ? make_int4(0, -1, 0, 1) : make_int4(0, 0, 0, 0);
}

// the fused entry's own rules, after ctc_beam_check; *mc: the LM's config
const char* ctc_beam_lm_check(const EcLm* lm, int32_t batch, int32_t vocab, int32_t beam, const EcLmConfig** mc) {
    *mc = lm_handle_config(lm, false);
    if (!*mc) return "ctc beam search: null lm handle";
    if ((*mc)->vocab_size != vocab) return "ctc beam search: the LM's vocab_size differs from vocab";
    if ((int64_t)batch * beam > (1 << 21)) return "ctc beam search: batch * beam must be at most 2^21 with an LM";
    return nullptr;
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
    if (const char* e = ctc_beam_tmp_check(temperature)) return ec_fail(e);
    if (batch == 0) return 0;
    if (!out_len || !token_len || !score || !workspace || (t_out > 0 && (!logits || !tokens))) return ec_fail("null argument");
    const CtcBeamLayout L = ctc_beam_layout(batch, t_out, beam);
    if (workspace_bytes < L.total) return ec_fail("workspace too small (effconf_ctc_beam_workspace_bytes)");
    char* ws = WsPlan::base(workspace);
    CtcBeamArgs a = ctc_beam_args(logits, out_len, t_out, vocab, beam, temperature, tokens, token_len, score);
    a.utt = ws + L.utt; a.stats = reinterpret_cast<int*>(ws + L.stats); a.L = L;
    hipLaunchKernelGGL(ctc_beam_kernel, dim3(batch), dim3(CT), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : ec_fail("ctc_beam launch failed");
}

// ---- the plain search resumed per stream (include/effconf.h)
size_t effconf_ctc_beam_stream_state_bytes(int32_t max_streams, int32_t max_frames, int32_t beam) {
    if (const char* e = ctc_beam_stream_check(max_streams, max_frames, beam)) { ec_fail(e); return 0; }
    return ctc_beam_stream_layout(max_streams, max_frames, beam).total;
}

int effconf_ctc_beam_stream_init(void* state, size_t state_bytes, int32_t max_streams, int32_t max_frames, int32_t beam, void* stream) {
    if (const char* e = ctc_beam_stream_check(max_streams, max_frames, beam)) return ec_fail(e);
    if (!state) return ec_fail("null argument");
    const CtcBeamStreamLayout L = ctc_beam_stream_layout(max_streams, max_frames, beam);
    if (state_bytes < L.total) return ec_fail("stream state buffer too small (effconf_ctc_beam_stream_state_bytes)");
    // the flags alone: a record whose flag is clear is never read, and the kernel initialises a stream's hash at its first frame
    if (hipMemsetAsync(WsPlan::base(state) + L.primed, 0, (size_t)max_streams * 4, (hipStream_t)stream) != hipSuccess) return ec_fail("memset failed");
    return 0;
}

int effconf_ctc_beam_stream_reset(void* state, int32_t max_streams, int32_t stream_id, void* stream) {
    if (!state) return ec_fail("null argument");
    if (max_streams < 1 || stream_id < 0 || stream_id >= max_streams) return ec_fail("stream id outside 0 .. max_streams - 1");
    // primed[] is the first region of every layout: its offset depends on nothing
    if (hipMemsetAsync(WsPlan::base(state) + (size_t)stream_id * 4, 0, 4, (hipStream_t)stream) != hipSuccess) return ec_fail("memset failed");
    return 0;
}

size_t effconf_ctc_beam_stream_workspace_bytes(int32_t n, int32_t t_new, int32_t beam) {
    if (const char* e = ctc_beam_check(n, t_new, 2, beam)) { ec_fail(e); return 0; }
    return ctc_beam_stream_ws(n, t_new, beam).total;
}

int effconf_ctc_beam_resume(void* state, int32_t max_streams, int32_t max_frames, int32_t beam, const int32_t* streams, const float* logits,
                            const int64_t* out_len, int32_t n, int32_t t_new, int32_t vocab, float temperature, int32_t nbest, int32_t* tokens,
                            int32_t* token_len, float* score, int32_t* stable_len, int32_t max_tokens, void* workspace, size_t workspace_bytes,
                            void* stream) {
    if (const char* e = ctc_beam_stream_check(max_streams, max_frames, beam)) return ec_fail(e);
    if (const char* e = ctc_beam_check(n, t_new, vocab, beam)) return ec_fail(e);
    if (nbest < 1 || nbest > beam) return ec_fail("ctc beam search: nbest must be in 1 .. beam");
    if (max_tokens < 1 || max_tokens > (1 << 24)) return ec_fail("ctc beam search: max_tokens must be in 1 .. 2^24 (no hypothesis is longer than max_frames)");
    if (const char* e = ctc_beam_tmp_check(temperature)) return ec_fail(e);
    const CtcBeamStreamWs W = ctc_beam_stream_ws(n, t_new, beam);
    if (workspace_bytes < W.total) return ec_fail("workspace too small (effconf_ctc_beam_stream_workspace_bytes)");
    if (n == 0) return 0;
    if (!state || !streams || !out_len || !tokens || !token_len || !score || !stable_len || !workspace || (t_new > 0 && !logits)) return ec_fail("null argument");
    const CtcBeamStreamLayout S = ctc_beam_stream_layout(max_streams, max_frames, beam);
    char* ws = WsPlan::base(workspace);
    char* st = WsPlan::base(state);
    CtcBeamArgs a = ctc_beam_args(logits, out_len, t_new, vocab, beam, temperature, tokens, token_len, score);
    a.utt = ws + W.trace; a.stats = reinterpret_cast<int*>(ws + W.stats);
    a.L.ncap = S.ncap; a.L.hcap = S.hcap; a.L.per_utt = W.per_trace; a.L.trace = 0; a.L.nodes = S.nodes; a.L.hkeys = S.hkeys; a.L.hvals = S.hvals;
    CtcStreamSide sz{};
    sz.streams = streams; sz.primed = reinterpret_cast<int*>(st + S.primed); sz.blocks = st + S.blocks; sz.per_stream = S.per_stream; sz.rec = S.rec;
    sz.max_streams = max_streams; sz.max_frames = max_frames; sz.nbest = nbest; sz.max_tokens = max_tokens; sz.stable_len = stable_len;
    hipLaunchKernelGGL(ctc_beam_resume_kernel, dim3(n), dim3(CT), 0, (hipStream_t)stream, a, sz);
    return hipGetLastError() == hipSuccess ? 0 : ec_fail("ctc_beam_resume launch failed");
}

size_t effconf_ctc_beam_lm_workspace_bytes(const EcLm* lm, int32_t batch, int32_t t_out, int32_t vocab, int32_t beam) {
    if (const char* e = ctc_beam_check(batch, t_out, vocab, beam)) { ec_fail(e); return 0; }
    const EcLmConfig* mc;
    if (const char* e = ctc_beam_lm_check(lm, batch, vocab, beam, &mc)) { ec_fail(e); return 0; }
    return ctc_beam_lm_layout(*mc, batch, t_out, beam).total;
}

int effconf_ctc_beam_lm(EcLm* lm, const float* logits, const int64_t* out_len, int32_t batch, int32_t t_out, int32_t vocab, int32_t beam,
                        float temperature, float lm_weight, float lm_tmp, float length_bonus, int32_t* tokens, int32_t* token_len, float* total,
                        float* am_score, float* lm_score, int32_t* rounds_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (const char* e = ctc_beam_check(batch, t_out, vocab, beam)) return ec_fail(e);
    const EcLmConfig* mc;
    if (const char* e = ctc_beam_lm_check(lm, batch, vocab, beam, &mc)) return ec_fail(e);
    if (const char* e = ctc_beam_tmp_check(temperature)) return ec_fail(e);
    if (!(lm_weight > 0.f) || !std::isfinite(lm_weight)) return ec_fail("ctc beam search: lm_weight must be > 0 (0: effconf_ctc_beam)");
    if (!(lm_tmp > 0.f) || !std::isfinite(lm_tmp)) return ec_fail("ctc beam search: lm_tmp must be > 0");
    if (!std::isfinite(length_bonus)) return ec_fail("ctc beam search: length_bonus must be finite");
    if (!lm_handle_config(lm, true)) return ec_fail("ctc beam search: lm handle not finalized");
    if (rounds_out) *rounds_out = 0;
    if (batch == 0) return 0;
    if (!out_len || !token_len || !total || !am_score || !lm_score || !workspace || (t_out > 0 && (!logits || !tokens))) return ec_fail("null argument");
    const CtcBeamLmLayout L = ctc_beam_lm_layout(*mc, batch, t_out, beam);
    if (workspace_bytes < L.total) return ec_fail("workspace too small (effconf_ctc_beam_lm_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    char* ws = WsPlan::base(workspace);
    CtcBeamArgs a = ctc_beam_args(logits, out_len, t_out, vocab, beam, temperature, tokens, token_len, am_score);
    a.utt = ws + L.s.utt; a.stats = reinterpret_cast<int*>(ws + L.s.stats); a.L = L.s;
    CtcLmSide fz{};
    fz.req = reinterpret_cast<int4*>(ws + L.req); fz.slot = reinterpret_cast<const int*>(ws + L.slot); fz.logits = reinterpret_cast<const float*>(ws + L.logits);
    fz.resume = reinterpret_cast<int*>(ws + L.resume); fz.active = reinterpret_cast<int*>(ws + L.counter);
    fz.lmnodes = L.lmnodes; fz.trace2 = L.trace2; fz.nls = L.nls; fz.w = lm_weight; fz.tmp = lm_tmp; fz.bonus = length_bonus;
    fz.total = total; fz.lm_score = lm_score;
    const int ncol = batch * beam;
    LmColumns col{};
    col.req = fz.req; col.ncol = ncol; col.cols_per_utt = beam; col.slot = reinterpret_cast<int*>(ws + L.slot);
    col.utt = a.utt; col.per_utt = L.s.per_utt; col.lmnodes = L.lmnodes; col.node_floats = L.nls + L.vocab; col.logits = reinterpret_cast<float*>(ws + L.logits);
    if (hipMemsetAsync(fz.resume, 0, (size_t)batch * CTC_BEAM_LM_REC_INTS * 4, s) != hipSuccess) return ec_fail("ctc beam search: clearing the resume records failed");
    hipLaunchKernelGGL(ctc_beam_lm_root_kernel, dim3((ncol + 255) / 256), dim3(256), 0, s, fz.req, ncol, beam);
    if (hipGetLastError() != hipSuccess) return ec_fail("ctc_beam_lm_root launch failed");
    if (lm_columns_step(lm, col, ws + L.lm, s) != 0) return ec_fail("ctc beam search: LM step launch failed");
    // every launch advances each unfinished utterance by at least one frame; the last one finds nothing suspended
    for (int round = 0;; ++round) {
        if (round >= t_out + 2) return ec_fail("ctc beam search: the rounds did not end (internal error)");
        if (hipMemsetAsync(fz.active, 0, 4, s) != hipSuccess) return ec_fail("ctc beam search: clearing the round counter failed");
        hipLaunchKernelGGL(ctc_beam_lm_kernel, dim3(batch), dim3(CT), 0, s, a, fz);
        if (hipGetLastError() != hipSuccess) return ec_fail("ctc_beam_lm launch failed");
        int active = 0;
        if (hipMemcpyAsync(&active, fz.active, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return ec_fail("ctc beam search: reading the round counter failed");
        if (rounds_out) *rounds_out = round + 1;
        if (active == 0) return 0;
        if (lm_columns_step(lm, col, ws + L.lm, s) != 0) return ec_fail("ctc beam search: LM step launch failed");
    }
}

}  // extern "C"
