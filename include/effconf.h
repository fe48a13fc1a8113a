/* libeffconf — MI355X (gfx950) native Efficient Conformer encoder forward path.  C ABI.
 *
 * The reference (burchim/EfficientConformer) has no plugin/FFI layer: its seam for this path is the
 * Python class models.encoders.ConformerEncoder (reference models/encoders.py:44), constructed from
 * the `encoder_params` dict (encoders.py:46-95) and called as `encoder(x, x_len)` at
 * models/model_ctc.py:63, 93, 159, models/transducer.py:94, 145, 206 and models/model.py:552, 639.
 * This header is what a native replacement of that seam exports; the Python class
 * efficientconformer_amd.ConformerEncoder binds it with ctypes.
 *
 * Conventions
 *   - every `dev` pointer is caller-owned DEVICE memory (HIP); the library never frees it;
 *   - packed weights are the only memory the library owns (allocated in effconf_encoder_finalize,
 *     released by effconf_encoder_destroy);
 *   - all work is enqueued on the `stream` argument (a hipStream_t passed as void*; NULL = default
 *     stream); no call synchronises the device or allocates in the forward path (graph-capturable);
 *   - return value 0 = ok, negative = error, message via effconf_last_error() (thread-local);
 *   - no C++ exceptions or torch types cross this boundary.
 */
#ifndef EFFCONF_H
#define EFFCONF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is compiled with -fvisibility=hidden: the declarations of this header (and of effconf_debug.h) are its ONLY dynamic symbols
 * (tests/test_abi_and_host.py checks `nm -D`); the internal launch_* / pack_* C++ functions of csrc/kernels.h are not linkable. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* 2: EcConfig gained causal / left_context / right_context
 * 3: the effconf_debug_* entries left libeffconf.so for libeffconf_debug.so (round 5), hidden visibility for everything this header does not
 *    declare, the label-exact "split" mode takes ragged batches and causal / streaming configurations (round 6) */
#define EFFCONF_ABI_VERSION 3

/* Per-block hyper-parameters, already resolved from the per-stage lists exactly as
 * ConformerEncoder.__init__ does (reference encoders.py:80-95). */
typedef struct EcBlock {
    int32_t dim_model;    /* D   : input / attention width                                  */
    int32_t dim_expand;   /* De  : output width (== D except in the two transition blocks)  */
    int32_t ff_ratio;     /* FFN hidden = ff_ratio * dim                                    */
    int32_t num_heads;    /* H                                                              */
    int32_t kernel_size;  /* depthwise conv taps (odd, <= 31)                               */
    int32_t group_size;   /* attention group size G (odd)                                   */
    int32_t max_pos;      /* max_pos_encoding of this block's relative table                */
    int32_t conv_stride;  /* 1 or 2 (progressive downsampling, blocks.py:106-117)           */
} EcBlock;

/* Mirrors the reference `encoder_params` keys that reach the hot path (encoders.py:50-94). */
typedef struct EcConfig {
    int32_t n_mels, sample_rate, n_fft, win_length, hop_length;  /* modules.py:77-85           */
    int32_t normalize; float mean, std;                          /* modules.py:103-104         */
    int32_t sub_layers;                                          /* Conv2dSubsampling layers   */
    int32_t sub_filters[4];                                      /* channels per layer         */
    int32_t num_blocks;
    const EcBlock* blocks;
    int32_t vocab_size;                                          /* >0: CTC head `fc` present  */
    /* streaming / causal (encoders.py:68, 94): contexts in frames AFTER the subsampling, as StreamingMask gets them - key j of query i
     * masked iff j - i > right_context or j - i < -left_context; >= 2^30 = unlimited (the shipped configs pass max_pos_encoding);
     * causal = 1: causal relative tables (attentions.py:506, 1243-1247), depthwise convs pre-padded (k - 1, 0) (layers.py:97-101), and
     * the caller passes right_context = 0 (encoders.py:68).  bf16 path, attention2.hip head widths (<= 160 padded) only. */
    int32_t causal, left_context, right_context;
} EcConfig;

typedef struct EcEncoder EcEncoder;

int effconf_abi_version(void);
const char* effconf_last_error(void);

/* ---- lifetime + weights ------------------------------------------------------------------- */
/* Test hook: with EFFCONF_POISON_GUARDS=<KiB> (>0; at least 16 KiB is used) in the environment at create time, finalize places every
 * packed parameter buffer between two guard regions of 0xFF bytes (NaN as bf16 and fp32), so an out-of-bounds parameter read shows
 * up in the output (tests/test_gpu_exact_and_sweep.py::test_no_kernel_reads_past_a_parameter_buffer, tools/poison_sweep.py).  Read
 * once here, never on the forward path.  The Python wrapper has the matching EFFCONF_POISON_WORKSPACE=<byte> hook for the
 * caller-owned workspace (efficientconformer_amd/_native.py: every workspace the wrappers allocate). */
EcEncoder* effconf_encoder_create(const EcConfig* cfg);
void effconf_encoder_destroy(EcEncoder* enc);
/* Hand over one reference state_dict tensor (HOST fp32, contiguous, reference layout) by its key
 * without the "encoder." prefix, e.g. "blocks.3.feed_forward_module1.layers.1.weight",
 * "subsampling_module.layers.0.1.running_var", "fc.weight" (reference models/model.py:361-384,
 * model_ctc.py:77-88 decide which keys exist).  Keys the packer does not know are kept and ignored;
 * effconf_encoder_finalize reports the first REQUIRED key that is missing or mis-shaped. */
int effconf_encoder_load_tensor(EcEncoder* enc, const char* key, const float* host, const int64_t* shape, int32_t ndim);
/* Fold BatchNorm(eval) into the convolutions, cast to bf16, pad to MFMA-friendly shapes, build the
 * sinusoid / window / filterbank tables and upload.  Fails (-1) if a required tensor is missing. */
int effconf_encoder_finalize(EcEncoder* enc);

/* ---- forward ------------------------------------------------------------------------------ */
/* Bytes of scratch a forward of this shape needs (n = samples per row if from_audio, else mel frames).  Since the head-major layout left,
 * the Q / K / V buffers are rows x D for rectangular batches too (as for ragged ones): the answer is smaller than it was wherever the grouped
 * head width is no multiple of 32.  Query it; do not assume an earlier value. */
size_t effconf_encoder_workspace_bytes(const EcEncoder* enc, int32_t batch, int32_t n, int32_t from_audio);
/* Output frames T_out for an input of n samples / mel frames (encoders.py:139 bookkeeping). */
int32_t effconf_encoder_out_frames(const EcEncoder* enc, int32_t n, int32_t from_audio);

/* ConformerEncoder.forward(x, x_len) (reference encoders.py:97-142), eval mode.
 *   audio   dev f32 (batch, n_samples)   zero-padded rows (utils/preprocessing.py:38)
 *   x_len   dev i64 (batch)              valid samples per row
 *   out     dev f32 (batch, T_out, D_last)
 *   out_len dev i64 (batch)
 * The third value of the reference's return tuple (attention maps no caller consumes) is not produced. */
int effconf_encoder_forward(EcEncoder* enc, const float* audio, const int64_t* x_len, int32_t batch, int32_t n_samples,
                            float* out, int64_t* out_len, void* workspace, size_t workspace_bytes, void* stream);
/* Same, entered after AudioPreprocessing: mel dev f32 (batch, n_mels, n_frames), mel_len in frames.
 * This is the parity boundary ("identical mel inputs"). */
int effconf_encoder_forward_mel(EcEncoder* enc, const float* mel, const int64_t* mel_len, int32_t batch, int32_t n_frames,
                                float* out, int64_t* out_len, void* workspace, size_t workspace_bytes, void* stream);

/* Ragged batch: the same forward with every utterance at ITS OWN length - no pad frames exist, so utterance b's output is what the
 * reference computes for that utterance alone (batch size 1; the reference's batched output differs from it by the pad-frame leakage of
 * SURVEY.md 8a), independent of what else is in the batch.  All utterances share one concatenated row space and one set of launches.
 *   x          dev f32 (batch, n) audio rows or (batch, n_mels, n) mel (from_audio = 0); n = the row pitch (content behind x_len unused)
 *   x_len      dev i64 (batch); x_len_host: the same lengths on the HOST (grids and the workspace are sized from them)
 *              CONTRACT: x_len_host[b] == x_len[b] for every b.  The library cannot compare them without a synchronisation and does not:
 *              the kernels index rows with the device copy inside grids / a workspace sized from the host copy, so a device length that
 *              exceeds its host twin is an out-of-bounds access.  (The Python wrapper checks on request: ConformerEncoder.check_host_lengths.)
 *   out        dev f32 (batch, out_frames, D_last): utterance b's T_out(b) frames, zeros behind them; out_frames >= the longest T_out
 * Workspace: effconf_encoder_workspace_bytes_ragged(enc, x_len_host, batch, n, from_audio), under the options the forward will run with.  Front ends:
 * sublinear2.hip / sublinear3.hip and the one-layer conv + GEMM route write the ragged rows themselves; the two-layer subsampler runs on the rectangular
 * image (zero padding at every utterance's own end) and gathers the valid rows.  The size holds the front end's scratch only where the chosen route
 * ("fuse_subsample" below) uses it: none for the fused kernels (before, every ragged route but sublinear2.hip under "fuse_subsample" = 2 reserved the
 * subsampler's output rows and a rectangular Linear output - EfficientConformer Large under defaults, any model under "fuse_subsample" = 3), the subsampler's
 * output rows for conv + GEMM (no rectangular Linear output any more), both plus the layer-1 image for two layers.  Rectangular sizes are unchanged.
 * Needs head widths <= 160 (attention2.hip); bf16 path only. */
size_t effconf_encoder_workspace_bytes_ragged(const EcEncoder* enc, const int64_t* x_len_host, int32_t batch, int32_t n, int32_t from_audio);
int effconf_encoder_forward_ragged(EcEncoder* enc, const float* x, const int64_t* x_len, const int64_t* x_len_host, int32_t batch, int32_t n,
                                   int32_t from_audio, float* out, int32_t out_frames, int64_t* out_len, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* AudioPreprocessing.forward alone (reference modules.py:87-106): audio -> (batch, n_mels, n//hop+1). */
int effconf_mel_frontend(EcEncoder* enc, const float* audio, int32_t batch, int32_t n_samples, float* mel, void* stream);

/* CTC head + greedy decode (reference model_ctc.py:49, 90-133): fc, per-frame argmax, drop blanks,
 * collapse repeats, stop at out_len.  labels dev i32 (batch, T_out) zero-filled tail, label_len dev i32 (batch).
 * logits (dev f32 (batch, T_out, vocab)) may be NULL.  Needs batch*T_out*4 bytes of workspace. */
int effconf_ctc_greedy(EcEncoder* enc, const float* enc_out, const int64_t* out_len, int32_t batch, int32_t t_out,
                       int32_t* labels, int32_t* label_len, float* logits, void* workspace, size_t workspace_bytes, void* stream);
/* The same head on bf16 rows (dev bf16 (batch, T_out, D_last)): what a rank holds after the all-gather of encoder outputs on a bf16 wire
 * (reference sharding: main.py:33-35, 217-220; the head itself: model_ctc.py:49, 90-133).  bf16 path only.  x = x_hi exactly, so the split head issues
 * two MFMAs per 16 k instead of three and skips the conversion pass; logits and labels are bit-identical to effconf_ctc_greedy on the same values
 * widened to fp32. */
int effconf_ctc_greedy_bf16(EcEncoder* enc, const uint16_t* enc_out_bf16, const int64_t* out_len, int32_t batch, int32_t t_out,
                            int32_t* labels, int32_t* label_len, float* logits, void* workspace, size_t workspace_bytes, void* stream);
/* The same head with the top-2 logit margin of every frame, for margin-gated label-exact decoding (ModelCTC.greedy_exact: an utterance whose
 * smallest bf16 margin is at least a band >= the per-frame spread of (bf16 logit - split logit) keeps its bf16 labels).
 * enc_out: dev f32 rows, or dev bf16 rows with enc_is_bf16 != 0 (then as effconf_ctc_greedy_bf16: bf16 path only).  The head kernel is chosen as in
 * the two entries above (option ctc_mfma, the label-exact modes, the row type); labels, label_len and logits are bit-identical to theirs.
 *   frame_margin dev f32 (batch, t_out), may be NULL: largest minus second largest logit of the frame, the fp32 subtraction of the values `logits`
 *                holds (= topk(logits, 2) differenced); 0 for a duplicated maximum (the label stays the first index).  Every frame of the
 *                rectangle is written, valid or not.
 *   min_margin   dev f32 (batch): the smallest frame_margin over frames < out_len[b] (clamped to [0, t_out]); +inf for out_len 0.  A NaN margin
 *                (a frame of NaN logits) wins over every number.
 *   min_frame    dev i32 (batch): the first frame that holds min_margin; -1 for out_len 0.
 * logits may be NULL.  Needs batch*T_out*8 bytes of workspace. */
int effconf_ctc_greedy_margin(EcEncoder* enc, const void* enc_out, int32_t enc_is_bf16, const int64_t* out_len, int32_t batch, int32_t t_out,
                              int32_t* labels, int32_t* label_len, float* logits, float* frame_margin, float* min_margin, int32_t* min_frame,
                              void* workspace, size_t workspace_bytes, void* stream);

/* CTC prefix beam search: ModelCTC.beam_search_decoding (reference model_ctc.py:138-181, ctcdecode's CTCBeamDecoder with blank 0,
 * cutoff_top_n = vocab, cutoff_prob 1) without the n-gram (KenLM) terms, one persistent workgroup per utterance.  logits dev f32
 * (batch, t_out, vocab), e.g. the logits output of effconf_ctc_greedy; per frame logP = (logits / temperature).softmax().log() in fp32.
 * out_len dev i64 (batch), clamped to [0, t_out]; frames at or beyond it are never read.  1 <= beam <= 32, 2 <= vocab <= 1024,
 * temperature > 0.  Outputs, ranked best first: tokens dev i32 (batch, beam, t_out) with zero-filled tails, token_len dev i32
 * (batch, beam), score dev f32 (batch, beam) = log(P_blank + P_nonblank) of the prefix (ctcdecode's beam_scores are -score).  Ranks
 * without a hypothesis have length 0 and score -inf; len 0 gives the empty prefix with score 0.
 * Workspace (effconf_ctc_beam_workspace_bytes; the library aligns the pointer up to 256 bytes; al(x) = x rounded up to 256):
 *   [0, 16 batch)            i32 stats[batch][4]: frames decoded, candidates scored (sum over frames), trie nodes used, 0
 *   al(16 batch) + b * U     utterance b, U = al(16 t_out beam) + al(16 N) + al(8 H) + al(4 H), N = 1 + beam t_out trie nodes,
 *                            H = smallest power of two >= 2 N:
 *     trace [t_out][beam]    {i32 node, f32 pb, f32 pnb, f32 score} of the beam after frame t, in rank order (t < len only; a rank
 *                            without a member has node -1 and -inf values)
 *     nodes [N]              {i32 parent, i32 token, i32 length, i32 0}; node 0 is the empty prefix (-1, -1, 0); a prefix's node is
 *                            the same for as long as the call runs (a prefix created again gets its old node)
 *     hash keys u64 [H], hash nodes i32 [H]   the (parent, token) -> node index
 * effconf_ctc_beam_workspace_bytes returns 0 for arguments effconf_ctc_beam rejects. */
size_t effconf_ctc_beam_workspace_bytes(int32_t batch, int32_t t_out, int32_t vocab, int32_t beam);
int effconf_ctc_beam(const float* logits, const int64_t* out_len, int32_t batch, int32_t t_out, int32_t vocab, int32_t beam,
                     float temperature, int32_t* tokens, int32_t* token_len, float* score, void* workspace, size_t workspace_bytes,
                     void* stream);

/* Streaming CTC prefix beam search: effconf_ctc_beam resumed per stream, push by push (one workgroup per listed stream).  The search visits frames
 * in order and never looks ahead, so the beam of a stream after its pushes, whatever their pattern, is bit for bit that of one effconf_ctc_beam call on the same
 * frames (tokens, lengths, scores, and the per-frame trace).  Not part of it: LM fusion (effconf_ctc_beam_lm), a compaction of the trie for unbounded streams.
 * State: one caller-provided device buffer of effconf_ctc_beam_stream_state_bytes(max_streams, max_frames, beam) bytes.  From the buffer's address aligned up to
 * 256 bytes (al(x) = x rounded up to 256):
 *   offset 0                              i32 primed[max_streams]   1: the record holds the stream's beam at a frame boundary
 *   offset al(4 max_streams) + s * P      the block of stream s, P = al(960) + al(16 N) + al(8 H) + al(4 H), N = 1 + beam max_frames trie nodes, H = smallest power
 *                                         of two >= 2 N:
 *     record i32 [240]                    head [16]: frames consumed, members, trie nodes, candidates scored (lo, hi), 11 unused; then [32] each of the members'
 *                                         node, last token, parent node, depth (i32) and pb, pnb, score (f32), in rank order
 *     nodes [N], hash keys u64 [H], hash nodes i32 [H]   the stream's trie, as in effconf_ctc_beam's workspace; it only grows until the stream is reset
 * effconf_ctc_beam_stream_init clears every flag, effconf_ctc_beam_stream_reset the flag of one stream (which then starts a new utterance); both write nothing
 * else.  A record whose flag is clear is never read; the kernel initialises a stream's hash at its first frame.  max_frames counts logit frames per utterance.
 * effconf_ctc_beam_resume: max_streams, max_frames, beam as the state was sized with; streams dev i32 (n) DISTINCT stream ids; logits dev f32 (n, t_new, vocab) the
 * new frames of the listed streams (t_new = 0 with logits NULL: every listed stream gets a read-only push); out_len dev i64 (n), clamped to [0, t_new]: frames at
 * or beyond it are never read.  A stream with out_len 0 keeps its record untouched and gets the outputs of its beam as it stands (a stream that never had a frame:
 * the empty prefix with score 0).  Outputs, ranks 0 .. nbest - 1 (1 <= nbest <= beam) of the beam after the push: tokens dev i32 (n, nbest, max_tokens) with
 * zero-filled tails; token_len dev i32 (n, nbest) the true length, also where it exceeds max_tokens (it never exceeds the frames the stream has consumed); score dev
 * f32 (n, nbest); stable_len dev i32 (n) the length of the longest common prefix of ALL members of the beam: every later hypothesis of the stream begins with these
 * tokens.  A listed id outside 0 .. max_streams - 1 gets token_len = -1 for its ranks, a push that would take a stream past max_frames token_len = -2; nothing else
 * is written for either, and the state stays as it was.
 * Workspace (effconf_ctc_beam_stream_workspace_bytes):
 *   [0, 16 n)                             i32 stats[n][4]: frames of the push, candidates scored so far, trie nodes so far, frames consumed so far
 *   al(16 n) + i * al(16 t_new beam)      trace [t_new][beam] of listed stream i: {i32 node, f32 pb, f32 pnb, f32 score} after each frame of the push, as effconf_ctc_beam's
 * Refused before any launch: effconf_ctc_beam's limits (beam 1 .. 32, vocab 2 .. 1024, beam * max_frames < 2^24), max_streams or max_frames < 1, nbest outside
 * 1 .. beam, max_tokens outside 1 .. 2^24, a temperature that is not finite and positive, a short workspace, null arguments; effconf_ctc_beam_stream_init refuses a short state
 * buffer.  The two size queries return 0 for arguments the entries reject. */
size_t effconf_ctc_beam_stream_state_bytes(int32_t max_streams, int32_t max_frames, int32_t beam);
int effconf_ctc_beam_stream_init(void* state, size_t state_bytes, int32_t max_streams, int32_t max_frames, int32_t beam, void* stream);
int effconf_ctc_beam_stream_reset(void* state, int32_t max_streams, int32_t stream_id, void* stream);
size_t effconf_ctc_beam_stream_workspace_bytes(int32_t n, int32_t t_new, int32_t beam);
int effconf_ctc_beam_resume(void* state, int32_t max_streams, int32_t max_frames, int32_t beam, const int32_t* streams, const float* logits,
                            const int64_t* out_len, int32_t n, int32_t t_new, int32_t vocab, float temperature, int32_t nbest, int32_t* tokens,
                            int32_t* token_len, float* score, int32_t* stable_len, int32_t max_tokens, void* workspace, size_t workspace_bytes,
                            void* stream);

/* CTC forced alignment and transcript scoring: for every utterance the best alignment (Viterbi) of a given target to the frames and the
 * total CTC log-likelihood log P(target | audio) (-torch.nn.functional.ctc_loss of the log_softmax), one trellis of t_out frames and
 * 2 U + 1 states, blank 0.  logits dev f32 (batch, t_out, vocab), e.g. the logits output of effconf_ctc_greedy; per frame
 * lp = log_softmax(logits / temperature) in fp32 (finite where the beam search's softmax().log() is -inf).  out_len dev i64 (batch), clamped
 * to [0, t_out]; target_len dev i64 (batch), clamped to [0, u_max]; targets dev i32 (batch, u_max).  Frames at or beyond out_len and
 * target slots at or beyond target_len are never read.  2 <= vocab <= 1024, 0 <= u_max <= 2047, temperature > 0.
 * Outputs (dev): log_likelihood f32 (batch); score f32 (batch) = the sum of lp along the best path; status i32 (batch):
 *   0 ok;  1 infeasible: out_len < U + (number of adjacent equal target pairs);  2 a target id outside 1 .. vocab - 1 (wins over 1).
 *   With status 1 / 2 both scores are -inf, frame_token and the token spans are -1 and token_logp is 0.  out_len 0 with U 0 is ok: scores 0.
 * frame_token i32 (batch, t_out): the target INDEX u emitted at frame t, -1 for a blank and at or beyond out_len; token_start / token_end
 * i32 (batch, u_max): first frame and last frame + 1 of token u, -1 at or beyond target_len; token_logp f32 (batch, u_max): the sum of lp
 * over the token's frames, 0 at or beyond target_len.  Ties: the smaller step wins (stay, +1, +2), the path ends in the last blank when both
 * ends are equal.  frame_token, token_start, token_end and token_logp may each be NULL; when all four are NULL the Viterbi half is skipped
 * (scoring only: score may be NULL and is not written; log_likelihood is bit-identical to the full call's).  An utterance's results do not
 * depend on the batch, on t_out / u_max beyond its own lengths, or on the run.
 * Workspace (effconf_ctc_align_workspace_bytes; the library aligns the pointer up to 256 bytes; al(x) = x rounded up to 256):
 *   [0, al(4 batch t_out (u_max + 1)))   f32 emit[batch][t_out][u_max + 1]: lp[blank], lp[target[0]], ... of every frame below out_len
 *   + al(4 batch t_out)                  i32 path[batch][t_out]: the state (2 u + 1: token u, even: a blank) of the best path per frame
 *   + batch * al(t_out R)                backpointers of utterances too long for LDS: per frame 64 w ceil(n / 4) bytes, n = ceil((2 U + 1) / 256)
 *                                        states per thread, w = ceil((2 U + 1) / (64 n)) waves; thread i's byte j holds the steps (2 bits each,
 *                                        0 stay / 1 / 2) into its states i n + 4 j .. i n + 4 j + 3;  R = 256 ceil(n_max / 4) with n_max =
 *                                        ceil((2 u_max + 1) / 256) rounded up to a power of two
 * effconf_ctc_align_workspace_bytes returns 0 for arguments effconf_ctc_align rejects. */
size_t effconf_ctc_align_workspace_bytes(int32_t batch, int32_t t_out, int32_t vocab, int32_t u_max);
int effconf_ctc_align(const float* logits, const int64_t* out_len, int32_t batch, int32_t t_out, int32_t vocab, const int32_t* targets,
                      const int64_t* target_len, int32_t u_max, float temperature, float* log_likelihood, float* score, int32_t* status,
                      int32_t* frame_token, int32_t* token_start, int32_t* token_end, float* token_logp, void* workspace,
                      size_t workspace_bytes, void* stream);

/* (Grouped)RelPosMultiHeadSelfAttention core alone (reference attentions.py:549-718 between the input projections and the output
 * projection): natural-layout bf16 device buffers qu = Q + u, k, v of (batch * Tp, dim) rows (Tp = frames rounded up to the group
 * size; pad rows: qu = u, k = v = 0), e = pos_layer(R) of (2 Tp - group, dim) rows, dvu = (v - u) per head column as fp32
 * [heads][dvu_ld] (dvu_ld >= head width rounded up to 32, zero beyond the head width), lens = valid frames per utterance (i32).
 * out: bf16 (batch * frames, ld_out) un-grouped attention output.  variant 0 = attention.hip, 1 / 2 = attention2.hip (see the
 * "attention_v2" option).  Needs 512 bytes of readable slack behind qu / k / v / e (16-byte chunk loads may run past a head span). */
int effconf_relpos_attention(const uint16_t* qu, const uint16_t* k, const uint16_t* v, const uint16_t* e, const float* dvu, int32_t dvu_ld,
                             const int32_t* lens, int32_t batch, int32_t heads, int32_t frames, int32_t group, int32_t dim, uint16_t* out,
                             int32_t ld_out, int32_t variant, void* stream);

/* ---- per-kernel entry points (unit tests of ONE module on the product kernels) -------------------------------- */
/* Each runs one module of Conformer block `block` of a finalized encoder on caller-owned device buffers and is tested against the
 * reference's per-module outputs (tests/golden/tiny_*.npz `trace/blocks.N.*`).  `workspace`: effconf_module_workspace_bytes(enc,
 * batch, frames) bytes (for effconf_subsample: frames = mel frames).  fp32 rows are dense: (rows, D) row-major. */
size_t effconf_module_workspace_bytes(const EcEncoder* enc, int32_t batch, int32_t frames);
/* FeedForwardModule + half-step residual (reference modules.py:385-395, blocks.py:122, 132): y = x + 1/2 FFN_which(LayerNorm(x));
 * which = 1 (feed_forward_module1, width dim_model) or 2 (feed_forward_module2, width dim_expand).  y may alias x. */
int effconf_ffn(EcEncoder* enc, int32_t block, int32_t which, const float* x, int32_t rows, float* y, void* workspace, size_t workspace_bytes,
                void* stream);
/* ConvolutionModule (reference modules.py:511-525; layers.py:122-136): LayerNorm -> pointwise-1 + GLU -> depthwise conv (stride of the
 * block) + BatchNorm(eval) + Swish -> pointwise-2; NO residual.  x f32 (batch * frames, dim_model) -> y f32 (batch * frames_out, dim_expand),
 * frames_out = (frames - 1) / conv_stride + 1. */
int effconf_conv_module(EcEncoder* enc, int32_t block, const float* x, int32_t batch, int32_t frames, float* y, void* workspace,
                        size_t workspace_bytes, void* stream);
/* Conv2dSubsampling + transpose + Linear (reference modules.py:232-249, encoders.py:113-116): mel f32 (batch, n_mels, n_frames) ->
 * y f32 (batch * T1, dim_model of block 0), T1 = frames after the subsampling layers.  Honours the "fuse_subsample" option. */
int effconf_subsample(EcEncoder* enc, const float* mel, int32_t batch, int32_t n_frames, float* y, void* workspace, size_t workspace_bytes,
                      void* stream);
/* y = LayerNorm_which(x + alpha * r), r may be NULL: the residual / norm glue of ConformerBlock.forward (reference blocks.py:119-137).
 * which: 0 FFN1 pre-norm, 1 attention pre-norm, 2 conv-module pre-norm (width dim_model); 3 FFN2 pre-norm, 4 block-final norm (dim_expand). */
int effconf_layernorm_residual(EcEncoder* enc, int32_t block, int32_t which, const float* x, const float* r, float alpha, int32_t rows,
                               float* y, void* stream);

/* ---- RNN-T greedy decode (next row after the encoder: BASELINE.json configs[3]) ------------------ */
/* Replaces Transducer.gready_search_decoding's per-utterance Python loop (reference models/transducer.py:139-186) for
 * the shipped Transducer configs: RnnDecoder = Embedding + 1-layer LSTM (models/decoders.py:41-70) and
 * JointNetwork(joint_mode "sum", act "tanh", models/joint_networks.py:35-104).  All arithmetic fp32. */
typedef struct EcRnntConfig {
    int32_t dim_encoder;          /* encoder_params["dim_model"][-1]                (transducer.py:76)  */
    int32_t dim_decoder;          /* decoder_params["dim_model"] (embedding = LSTM hidden, decoders.py:46-47) */
    int32_t dim_joint;            /* joint_params["dim_model"]                      (joint_networks.py:41) */
    int32_t vocab_size;           /* decoder_params["vocab_size"]; token 0 = blank / start (transducer.py:151, 167) */
    int32_t num_layers;           /* decoder_params["num_layers"]: 1 is native                                   */
    int32_t max_consec_dec_step;  /* decoder_params.get("max_consec_dec_step", 5)  (transducer.py:83)            */
    int32_t joint_mode;           /* 0 = "sum" (native); "concat" is rejected                                    */
    int32_t joint_act;            /* 0 = "tanh" (native); others rejected                                        */
} EcRnntConfig;

typedef struct EcRnnt EcRnnt;

EcRnnt* effconf_rnnt_create(const EcRnntConfig* cfg);
void effconf_rnnt_destroy(EcRnnt* r);
/* state_dict tensors (HOST fp32) by reference key: "decoder.embedding.weight", "decoder.rnn.{weight,bias}_{ih,hh}_l0",
 * "joint_network.linear_{encoder,decoder,joint}.{weight,bias}". */
int effconf_rnnt_load_tensor(EcRnnt* r, const char* key, const float* host, const int64_t* shape, int32_t ndim);
/* Builds the per-token LSTM input table Gin[y] = W_ih emb[y] + b_ih + b_hh and the k-major weight images; uploads. */
int effconf_rnnt_finalize(EcRnnt* r);
size_t effconf_rnnt_workspace_bytes(const EcRnnt* r, int32_t batch, int32_t t_out);
/* Upper bound of emitted tokens per utterance: max_consec_dec_step * T_out (transducer.py:167-176). */
int32_t effconf_rnnt_max_tokens(const EcRnnt* r, int32_t t_out);
/* enc_out dev f32 (batch, T_out, dim_encoder), out_len dev i64 (batch) -> tokens dev i32 (batch, max_tokens), zero-filled
 * tails (the leading start token of the reference's `y` is not included: transducer.py:179 decodes y[:, 1:]),
 * token_len dev i32 (batch). */
/* "cluster_decode": -1 auto (default: batches of 16..256 utterances decode in clusters of 8 workgroups x 8 utterances that share the
 * weight streams and run their three mat-vec phases on the fp32 matrix pipe), 0 one workgroup per utterance, 1 force (batch <= 256).
 * A cluster's workgroups synchronise through global memory.  "cluster_by_slice" (default 1): a cluster is 8 CONSECUTIVE workgroups, so
 * slice k of the weights is only ever read through XCD k's L2 and any resident part of a launch consists of whole clusters (decodes that
 * share the GPU cannot starve each other); 0: the members of a cluster share an XCD and must all be resident - auto then stops at 128
 * utterances.  The spin is bounded: a starved cluster gives up with undefined tokens instead of hanging.  All paths produce identical
 * tokens.  "cluster_shape" (round 6): 0 (default) clusters of 8 workgroups x 8 utterances x 2 encoder frames per joint pass, 1 = 16 x 16 x 1 where the
 * decoder / joint widths leave LDS for it (<= 768; half the weight bytes per round - measured no faster: profiles/r6_33_rnnt_cluster_shapes.txt);
 * where 16 x 16 x 1 does not run (config or batch) the decision is that of 0.  -1 = 0; any other value is refused. */
int effconf_rnnt_set_option(EcRnnt* r, const char* name, int32_t value);
/* The kernel effconf_rnnt_greedy runs for `batch` utterances under the config and the options set so far: 0 one workgroup per utterance,
 * 1 clusters of 8 x 8 x 2, 2 clusters of 16 x 16 x 1 (-1: null handle).  Host only: needs neither finalize nor a device.  A forced cluster
 * decode ("cluster_decode" = 1) of more than 256 utterances reports 1 and effconf_rnnt_greedy refuses it. */
int effconf_rnnt_greedy_route(const EcRnnt* r, int32_t batch);
int effconf_rnnt_greedy(EcRnnt* r, const float* enc_out, const int64_t* out_len, int32_t batch, int32_t t_out,
                        int32_t* tokens, int32_t* token_len, int32_t max_tokens, void* workspace, size_t workspace_bytes,
                        void* stream);

/* Streaming greedy decode: effconf_rnnt_greedy resumed per stream, push by push (one workgroup per listed stream; the cluster kernels are not part of it).  The
 * tokens of a stream, whatever its push pattern, are those of one effconf_rnnt_greedy ("cluster_decode" = 0) call on the same frames.
 * State: one caller-provided device buffer of effconf_rnnt_stream_state_bytes(r, max_streams) bytes.  From the buffer's address aligned up to 256 bytes:
 *   offset 0                                   i32 primed[max_streams]   1: the record holds the stream's state at a frame boundary
 *   offset up256(4 * max_streams) + s * R      f32 h[dim_decoder], c[dim_decoder], gd[dim_joint] of stream s, R = up256(4 * (2 * dim_decoder + dim_joint))
 * (h, c: the prediction network's LSTM state after every token emitted so far; gd = linear_decoder(h) + bias, what the next joint evaluation reads).
 * effconf_rnnt_stream_init clears every flag, effconf_rnnt_stream_reset the flag of one stream (which then starts a new utterance: zero state, start token 0);
 * both write nothing else, and a record whose flag is clear is never read.  Several state buffers may be used with one handle.
 * effconf_rnnt_greedy_resume: streams dev i32 (n) DISTINCT stream ids, enc_out dev f32 (n, t_new, dim_encoder) the new frames of the listed streams, out_len
 * dev i64 (n) how many of them each stream has (0 allowed: its record is left untouched) -> tokens dev i32 (n, max_tokens), zero-filled tails; token_frames
 * (nullable) dev i32 (n, max_tokens): the push-local frame at which each token was emitted, -1 behind them; token_len dev i32 (n); decoder_steps (nullable)
 * dev i32 (n): prediction-network steps this push ran - a primed stream runs none until it emits a token, so over a stream's life they sum to tokens + 1 (0
 * for a stream that never had a frame).  A listed id outside 0 .. max_streams - 1 gets token_len = -1 and nothing else is written for it.
 * max_tokens >= effconf_rnnt_max_tokens(r, t_new): the bound holds per push, the consecutive-token counter is 0 at every frame boundary.  The workspace
 * (effconf_rnnt_stream_workspace_bytes) holds linear_encoder(enc_out) of the push.  Refused before any launch: a handle that is not finalized, n < 0,
 * t_new <= 0, a short token buffer or workspace; effconf_rnnt_stream_init refuses a short state buffer.  The two size queries return 0 for arguments the
 * entries reject. */
size_t effconf_rnnt_stream_state_bytes(const EcRnnt* r, int32_t max_streams);
int effconf_rnnt_stream_init(EcRnnt* r, void* state, size_t state_bytes, int32_t max_streams, void* stream);
int effconf_rnnt_stream_reset(EcRnnt* r, void* state, int32_t max_streams, int32_t stream_id, void* stream);
size_t effconf_rnnt_stream_workspace_bytes(const EcRnnt* r, int32_t n, int32_t t_new);
int effconf_rnnt_greedy_resume(EcRnnt* r, void* state, int32_t max_streams, const int32_t* streams, const float* enc_out, const int64_t* out_len,
                               int32_t n, int32_t t_new, int32_t* tokens, int32_t* token_frames, int32_t* token_len, int32_t* decoder_steps,
                               int32_t max_tokens, void* workspace, size_t workspace_bytes, void* stream);

/* RNN-T beam search: Transducer.beam_search_decoding (transducer.py:188-327) without the neural-LM / n-gram terms, one persistent
 * workgroup per utterance.  1 <= beam <= min(16, vocab_size), temperature > 0 (decoding_params["tmp"]), dim_decoder and dim_joint
 * multiples of 16.  At most max_expansions hypotheses are expanded per frame and at most max_tokens tokens returned; status dev i32
 * (batch): 0 ok, 1 expansion cap hit (the reference would keep expanding), 2 token cap hit - a capped utterance returns no tokens.
 * tokens dev i32 (batch, max_tokens) without the start token, zero-filled tails; token_len dev i32 (batch); score dev f32 (batch): the
 * fp32 logp_score of the chosen hypothesis.  Option "beam_eval_batch" (effconf_rnnt_set_option, 1 .. 16, default 16): hypotheses
 * evaluated per pass over the weights; every setting gives bit-identical results.  After the call the first 16 * batch bytes of the
 * 256-byte aligned workspace hold per-utterance i32 counters (evaluation batches, evaluated hypotheses, expansions, frames).
 * effconf_rnnt_beam_workspace_bytes returns 0 for arguments effconf_rnnt_beam rejects. */
size_t effconf_rnnt_beam_workspace_bytes(const EcRnnt* r, int32_t batch, int32_t t_out, int32_t beam, int32_t max_expansions,
                                         int32_t max_tokens);
int effconf_rnnt_beam(EcRnnt* r, const float* enc_out, const int64_t* out_len, int32_t batch, int32_t t_out, int32_t beam,
                      float temperature, int32_t max_expansions, int32_t* tokens, int32_t* token_len, float* score, int32_t* status,
                      int32_t max_tokens, void* workspace, size_t workspace_bytes, void* stream);

/* RNN-T lattice (csrc/rnnt_lattice.hip): for a known transcript, the two log-probabilities per lattice cell the RNN-T loss and a forced
 * alignment need, without the (batch, T, U + 1, vocab) logits of transducer.py:88-107.  targets dev i32 (batch, u_max), blank excluded,
 * target_len dev i64 (batch).  For t < out_len[b] and u <= target_len[b], with logits(t, u) = linear_joint(tanh(linear_encoder(f[t]) +
 * linear_decoder(g_u))) and g_u the prediction network's output after [0, y_1 .. y_u]:
 *   lp_blank[b][t][u] = log_softmax(logits / temperature)[0],  lp_label[b][t][u] = log_softmax(logits / temperature)[y_b[u]] (-inf at
 *   u = target_len[b]);  both dev f32 (batch, t_out, u_max + 1), 0 outside the utterance's rectangle.  fp32 operands on the fp32 matrix
 * pipe; a cell depends on its own utterance only.  status dev i32 (batch): 0 ok, 1 tokens but no frames, 2 a token outside 1 .. vocab - 1
 * or target_len outside 0 .. u_max (the utterance's rows of both planes are 0).  u_max <= 1023, batch * t_out * (u_max + 1) < 2^31,
 * dim_decoder and dim_joint multiples of 16; effconf_rnnt_lattice_workspace_bytes returns 0 for arguments effconf_rnnt_lattice rejects. */
size_t effconf_rnnt_lattice_workspace_bytes(const EcRnnt* r, int32_t batch, int32_t t_out, int32_t u_max);
int effconf_rnnt_lattice(EcRnnt* r, const float* enc_out, const int64_t* out_len, int32_t batch, int32_t t_out, const int32_t* targets,
                         const int64_t* target_len, int32_t u_max, float temperature, float* lp_blank, float* lp_label, int32_t* status,
                         void* workspace, size_t workspace_bytes, void* stream);
/* RNN-T lattice dynamic programs (csrc/rnnt_align.hip) on such planes (any planes of that shape): log_likelihood dev f32 (batch) =
 * log P(y | x) over all monotone paths (= -rnnt_loss), and - unless score is NULL (then token_frame / token_logp must be NULL too: the
 * forward recursion alone, bit-identical log_likelihood) - score dev f32 (batch) = the best path's log-probability including its blanks,
 * token_frame dev i32 (batch, u_max) = the frame at which token u is emitted, token_logp dev f32 (batch, u_max) = lp_label at that cell;
 * rows at or beyond target_len[b] are -1 / 0.  Ties take the blank (time) move.  status dev i32 (batch) is read (the lattice's status,
 * or zeros) and written: a non-zero status is kept, 1 = tokens but no frames, 2 = target_len outside 0 .. u_max; such an utterance has both
 * scores -inf, token_frame -1 and token_logp 0.  No frames and no tokens: status 0, both scores 0. */
size_t effconf_rnnt_align_workspace_bytes(int32_t batch, int32_t t_out, int32_t u_max);
int effconf_rnnt_align(const float* lp_blank, const float* lp_label, const int64_t* out_len, const int64_t* target_len, int32_t batch,
                       int32_t t_out, int32_t u_max, float* log_likelihood, float* score, int32_t* token_frame, float* token_logp,
                       int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* ---- LSTM language model (csrc/lm.hip): n-best rescoring and the decode step ------------------------------------------ */
/* The reference's LanguageModel (models/lm.py:33-81, configs/LM-RNN.json): RnnDecoder = Embedding + num_layers LSTM layers of width dim_model
 * (models/decoders.py:41-70; torch gate order i, f, g, o; b_ih + b_hh), then fc (dim_model -> vocab_size).  All arithmetic fp32 on the fp32
 * matrix pipe.  dim_model a multiple of 16 in 16 .. 4096, 1 <= num_layers <= 4, vocab_size >= 2: anything else is refused at create. */
typedef struct EcLmConfig {
    int32_t vocab_size;           /* lm_params["vocab_size"] = tokenizer_params["vocab_size"]; token 0 = blank / start (lm.py:71) */
    int32_t dim_model;            /* lm_params["dim_model"]: embedding = LSTM hidden width                                        */
    int32_t num_layers;           /* lm_params["num_layers"]                                                                      */
} EcLmConfig;

typedef struct EcLm EcLm;

EcLm* effconf_lm_create(const EcLmConfig* cfg);
void effconf_lm_destroy(EcLm* lm);
/* state_dict tensors (HOST fp32) by reference key: "decoder.embedding.weight", "decoder.rnn.{weight,bias}_{ih,hh}_l{k}", "fc.{weight,bias}". */
int effconf_lm_load_tensor(EcLm* lm, const char* key, const float* host, const int64_t* shape, int32_t ndim);
/* Builds the layer-0 input table Gin0[y] = W_ih0 emb[y] + b_ih0 + b_hh0 (the embedding row of id 0 as the checkpoint holds it) and the
 * k-permuted weight images (W_hh0; [W_ih_l | W_hh_l] for l >= 1; fc); uploads.  A missing or mis-shaped tensor is reported before any
 * device call. */
int effconf_lm_finalize(EcLm* lm);
/* RNN-T beam search with neural-LM shallow fusion (transducer.py:259-273, 291-306): as effconf_rnnt_beam, with
 *   logP += lm_weight * (lm.decode(y, hidden_lm) / lm_tmp).softmax().log()
 * added to the joint's log-probabilities before the top `beam` entries are taken; a label child takes the LM's new state, a blank child keeps its
 * parent's.  The n-gram terms of the reference are not implemented.  lm: a finalized handle whose vocab_size is the transducer's; lm_weight > 0 and
 * lm_tmp > 0, both finite (weight 0 is effconf_rnnt_beam).  Outputs, status codes, zero-filled tails and the four counters at the head of the workspace
 * as effconf_rnnt_beam.  The search kernel (one workgroup per utterance) and one LM step over batch * 16 columns (the kernels of effconf_lm_step: the
 * LM's weights stream once per step for all utterances) alternate on `stream`; after every search launch the host reads the number of utterances that
 * wait for the LM (4 bytes, one stream synchronise), so the call returns with the results complete and CANNOT be captured in a graph.  At most
 * t_out * (max_expansions + 1) + 2 search launches; rounds_out (host, may be NULL) receives their number.  A row's results do not depend on the rows
 * sharing the call, on "beam_eval_batch" or on the workspace's contents.  The workspace holds, per utterance, an LM node (2 * num_layers * dim_model
 * + vocab_size floats) beside each of the 2 * beam + max_expansions + 64 decoder nodes: callers split large batches (rows are independent).
 * effconf_rnnt_beam_lm_workspace_bytes needs no finalized handles and returns 0 for arguments effconf_rnnt_beam_lm rejects. */
size_t effconf_rnnt_beam_lm_workspace_bytes(const EcRnnt* r, const EcLm* lm, int32_t batch, int32_t t_out, int32_t beam, int32_t max_expansions,
                                            int32_t max_tokens);
int effconf_rnnt_beam_lm(EcRnnt* r, EcLm* lm, const float* enc_out, const int64_t* out_len, int32_t batch, int32_t t_out, int32_t beam,
                         float temperature, float lm_weight, float lm_tmp, int32_t max_expansions, int32_t* tokens, int32_t* token_len,
                         float* score, int32_t* status, int32_t max_tokens, int32_t* rounds_out, void* workspace, size_t workspace_bytes,
                         void* stream);

/* CTC prefix beam search with neural-LM shallow fusion: effconf_ctc_beam's search with the candidates of every frame ranked by
 *   total(Q) = s(Q) + lm_weight * L(Q) + length_bonus * |Q|        (fp32, every operation rounded on its own, in this order)
 * s(Q) = log(P_blank + P_nonblank) as in effconf_ctc_beam, L(Q) = the LM's log-probability of the token string under LanguageModel's convention (the LM reads
 * [0, Q_0, ..]; effconf_lm_score's fp32 sum in ascending position, rows log softmax(fc(h) / lm_tmp)).  L of a prefix is computed once, when its trie node is
 * created, and kept in the node.  Ties: total desc, last token asc, canonical index, as effconf_ctc_beam.  Exact pruning is per member: of a member's plain
 * extensions only its `beam` best by lp[c] + lm_weight * row[c] are scored.  The reference has no such search (ctcdecode fuses KenLM only).
 * lm: a finalized handle whose vocab_size is `vocab`; lm_weight > 0 and lm_tmp > 0, finite (weight 0 is effconf_ctc_beam); length_bonus finite;
 * effconf_ctc_beam's limits; batch * beam <= 2^21.  Outputs, ranked by total: tokens / token_len as effconf_ctc_beam, total, am_score (= s) and lm_score (= L)
 * dev f32 (batch, beam); ranks without a hypothesis have length 0, total and am_score -inf, lm_score 0.
 * The search kernel (one workgroup per utterance, resumable) and one LM step over batch * beam columns (the kernels of effconf_lm_step) alternate on `stream`:
 * an utterance whose new beam holds prefixes without an LM row saves its beam and waits; after every search launch the host reads the number of waiting
 * utterances (4 bytes, one stream synchronise), so the call returns with the results complete and CANNOT be captured in a graph.  Every launch advances each
 * unfinished utterance by at least one frame: at most t_out + 2 search launches; rounds_out (host, may be NULL) receives their number.  A row's results
 * do not depend on the rows sharing the call or on the workspace's contents.
 * Workspace (effconf_ctc_beam_lm_workspace_bytes; needs no finalized handle, 0 for arguments the call rejects), S = 2 num_layers dim_model + vocab floats:
 *   stats as effconf_ctc_beam, the fourth word = LM rows the utterance asked for (the empty prefix's included); utterance b at al(16 batch) + b * U', U' = U + al(8 t_out beam) + al(4 (2 beam + 1) S), U and its regions as effconf_ctc_beam,
 *   a node's fourth word = the f32 L of its prefix:
 *     trace2 [t_out][beam]   {f32 L, f32 total} of the beam after frame t (a rank without a member: 0, -inf)
 *     LM slots [2 beam + 1]  per slot: per layer h (k-permuted as effconf_lm_workspace_bytes describes) and c, then the slot's log-probability row [vocab]
 *   then requests int4 [batch beam], packed columns i32 [2 batch beam], resume records i32 [batch][336], the round counter, the LM step's state
 *   (effconf_lm_workspace_bytes' layout for batch * beam sequences) and its raw logits rows f32 [batch beam][vocab]. */
size_t effconf_ctc_beam_lm_workspace_bytes(const EcLm* lm, int32_t batch, int32_t t_out, int32_t vocab, int32_t beam);
int effconf_ctc_beam_lm(EcLm* lm, const float* logits, const int64_t* out_len, int32_t batch, int32_t t_out, int32_t vocab, int32_t beam,
                        float temperature, float lm_weight, float lm_tmp, float length_bonus, int32_t* tokens, int32_t* token_len, float* total,
                        float* am_score, float* lm_score, int32_t* rounds_out, void* workspace, size_t workspace_bytes, void* stream);

/* Workspace of effconf_lm_score and effconf_lm_step (the latter: any u_max, e.g. 0): 256 + al(4 n) + num_layers * 3 * Np * dim_model * 4 bytes,
 * Np = n rounded up to 64, al(x) = x rounded up to 256.  After the 256-byte aligned pointer: i32 ulen[n]; at al(4 n) per layer l the blocks
 * h[2][Np][dim_model] (k permuted within every 16: position (k & ~15) | ((k & 3) << 2) | ((k >> 2) & 3); step u reads buffer u & 1 and
 * writes the other one for the column groups that still hold an unfinished sequence) and c[Np][dim_model].  Returns 0 for arguments the calls
 * reject: n outside 0 .. 2^21, u_max outside 0 .. 4096, n * u_max >= 2^31. */
size_t effconf_lm_workspace_bytes(const EcLm* lm, int32_t n, int32_t u_max);
/* Scores n token sequences: tokens dev i32 (n, u_max), token_len dev i64 (n).  With x = [0, y_0 .. y_{U-1}] and h_u the top layer's output after
 * x_0 .. x_u from zero state: token_logp[u] = log_softmax(fc(h_u) / lm_tmp)[y_u] for u < U (0 at or beyond U), score = their fp32 sum in
 * ascending u (U = 0: 0).  status dev i32 (n): 0 ok; 2 a token among the first U outside 1 .. vocab_size - 1 or token_len outside 0 .. u_max -
 * then score and the row of token_logp are -inf and the rest of the batch is untouched.  token_logp dev f32 (n, u_max) may be NULL.  Token slots
 * at or beyond token_len never influence a result.  Step-major: per position one launch per layer and one head launch, no (n, u_max, vocab)
 * tensor; a sequence's results are bit-identical in any batch, order, u_max and on any workspace content.  lm_tmp > 0. */
int effconf_lm_score(EcLm* lm, const int32_t* tokens, const int64_t* token_len, int32_t n, int32_t u_max, float lm_tmp, float* token_logp,
                     float* score, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
/* LanguageModel.decode(x, hidden) (lm.py:55-63): one token per sequence, tokens dev i32 (n) in 0 .. vocab_size - 1 (ids outside are clamped),
 * h_in / c_in dev f32 (num_layers, n, dim_model) or NULL = zeros -> logits dev f32 (n, vocab_size): the raw fc outputs, no temperature;
 * h_out / c_out (num_layers, n, dim_model), may be NULL, may alias h_in / c_in.  The same kernels as effconf_lm_score. */
int effconf_lm_step(EcLm* lm, const int32_t* tokens, const float* h_in, const float* c_in, int32_t n, float* logits, float* h_out, float* c_out,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Options.  "cache_pos_embeddings" = 1: the positional projections E = pos_layer(R) (reference attentions.py:588, 678)
 * are input independent; they live in the workspace and are recomputed only when that workspace last held a forward of
 * another batch size or number of frames.  The library remembers one tag per workspace pointer (the 16 most recently used),
 * so a caller that alternates workspaces (one per stream) keeps all of them warm.  Enable ONLY if the caller leaves the
 * workspaces untouched between forwards; setting the option again (to any value) forgets every tag — do that when a
 * workspace is freed and its address may be reused.  Host calls on one handle must not run concurrently (they only enqueue).
 * "fuse_subsample" (default 2): conv-subsampling + Linear (one subsampling layer; two layers have one route) as 0 = separate conv and GEMM kernels,
 *   1 = sublinear.hip (tiled GEMM whose A tile is produced by a VALU convolution; rectangular batches), 2 = sublinear2.hip (row-stationary, the convolution
 *   on the MFMA pipe with a bf16 hi / lo operand split; 80 mels, <= 192 filters / columns), 3 = sublinear3.hip (the same fusion in chunks of (output
 *   frequency, 32 channels), any channel count, widths up to 384; bit-identical to sublinear2.hip where both exist, slower there).  A value whose kernel is
 *   not built for the shape takes the next lower one that is; with 2, front ends wider than 128 channels / columns - EfficientConformer Medium, Large -
 *   run sublinear3.hip (option "sub3_auto", default 1).  The precedence in full: csrc/routes.h front_route (printed by effconf_debug_routes).
 * "tiled_auto" (default 1; round 6): with "wide_gemm" = 0, a configuration whose widest stage lies in ("tiled_min_k" = 256, 384] - EfficientConformer Medium's
 *   D = 360 - runs that stage as LayerNorm + tiled GEMMs instead of the row-stationary kernels (+ 2.3 % on Medium; decided per configuration at finalize,
 *   never per batch: one rounding path per handle).  0 = the row-stationary kernels as before.
 * "fuse_chain" (default 1): 0 runs every GEMM of a block as its own kernel instead of the fused row-local chains (chain.hip);
 *   with the debug trace this exposes the intermediate residual-stream states that otherwise only exist in registers.
 * "attention_v2" (default 1): 0 = attention.hip; 1 = attention2.hip (same tiling; V read through ds_read_b64_tr_b16 instead of being
 *   transposed on the way into LDS, hoisted staging addresses, no column masks off the buffer tails, deferred accumulator rescale);
 *   2 = attention2.hip with 32 queries per wave (one wave per SIMD: measured slower, kept for experiments).  Head widths above 160 (padded)
 *   always use attention.hip.  Results agree to fp32 summation order (variant 1's deferred rescale: to bf16 rounding of P).
 * "wide_gemm" (default 0): tile choice of the tiled GEMM layers (the widths the row-stationary kernels do not hold): 0 by shape,
 *     1 always csrc/gemm.hip (128 x 128, register staged), 2 / 3 csrc/gemm256.hip with 256 x 256 / 256 x 128 tiles wherever it applies.
 * "ctc_mfma" (default 2): the CTC head (fc + argmax).  2: split-bf16 operands on the bf16 MFMA (x_hi W_hi + x_hi W_lo + x_lo W_hi, fp32
 *   accumulation: logits within ~2^-16 relative of the fp32 head) - bf16 path only, the fp32-operand mode runs 1; 1: the fp32 MFMA; 0: the VALU
 *   kernel.  1 and 0 are k-ordered fp32 fma chains: bit-identical logits and labels.
 * "chain_small_m" (default 4096): chain launches (csrc/chain.hip) of at most this many rows run 2-wave workgroups (64 rows) instead of 8-wave ones:
 *   small-batch latency (B <= 8 utterances of 10 s); a wave computes its 32 rows identically in both shapes, so outputs do not depend on it.  0 = off.
 * "dwconv_mfma" (default 1; round 5): stride-1 depthwise convolutions on the matrix pipe (csrc/conv.hip dwconv_mfma_kernel: 4 x 4 x 4 Toeplitz blocks, one per
 *   channel, fp32 taps as bf16 hi + lo halves): 1 = kernel size 15, 2 = also 31 / 7, 0 = the VALU kernel everywhere.  Outputs agree with the VALU kernel's
 *   up to the summation order (a bf16 output may move by one ulp).
 * "chain_pair" (default 5): kernel selection of the chains at padded width 256: 5 = csrc/chain3.hip for chain A and csrc/chain2.hip for chain B,
 *   0 = csrc/chain.hip everywhere (the reference; bit-identical).  Any other value is refused.
 * "chain_full_max" (widest stage that runs chain A as one kernel; set before finalize to widen), "exact_attention" (0 tiled / 2 tiled with 16-row workgroups / 1 one wave per query row; fp32 mode, bit-identical): tuning / test switches of the kernel launchers that were
 *   process-global EFFCONF_* environment variables until round 2; per handle now.  (Still read from the environment, once: EFFCONF_POISON_GUARDS at
 *   create.  The in-kernel phase profilers - EFFCONF_{CHAIN,CHAIN2,CHAIN3,ATTN,FFN}_PHASES - and EFFCONF_ATTN_ABLATE exist in the tuning library of
 *   tools/build_ablate.py only.)
 * Removed options (tuning-only kernel variants; set_option now fails with "unknown option"): "chain_count_stores", "chain_variant", "chain_pair_min_d",
 *   "chain_pair_min_m", "chain_nt", "chain_w2cm", "rs_variant", "ffn_variant", "attn_waves"; and "head_major_odd", the head-major [B][H][Tg][dpad] Q / K / V / E layout nothing ran any more (the attention kernels read the
 *   rows [B*Tp][D] the GEMMs write at any alignment).  No exported symbol or struct changed.
 * "exact_fp32" (default 0): fp32-operand precision mode (csrc/exact.hip): every GEMM on fp32 MFMA, fp32 attention / convolutions,
 *   so that greedy CTC label sequences equal the reference's CPU fp32 path (model_ctc.py:99-133) wherever its top-2 logit margins
 *   exceed fp32 summation-order noise; ~10x slower than the default bf16-operand path.  Set to 1 BEFORE effconf_encoder_finalize
 *   (the fp32 tensors are uploaded there; the workspace query then covers both modes); afterwards it toggles the mode per handle.
 *   2 (round 4, csrc/split.hip; round 6, csrc/sxf.hip + sxf_chain.hip): fp32 tensors with every GEMM and the attention products on the fp16
 *   matrix pipe, each operand split into two fp16 numbers (three MFMAs per product, products accurate to ~2^-21): label sequences identical to the
 *   reference's on every golden and on the bench's oracle samples of Small / Medium / Large.  Round 6: ONE attention kernel per block with the scores on the
 *   CU, the row-local work of a block as two kernels, the front end as one kernel, ragged batches, causal and streaming configurations - 2.6x the bf16 step on
 *   EfficientConformerCTCSmall (5.7x in round 5), 2.4x / 2.7x on Medium / Large.  Set to 2 BEFORE finalize (the split weight images are built there; such a handle then serves 2, 1 and 0);
 *   a handle finalized with 1 refuses 2.
 * "split_chain" (default 1), "split_ffn" (default 1): split mode on the fused row-local kernels of csrc/sxf_chain.hip.  split_chain: the row-local work of a
 *   block as two chain kernels where their images exist (they contain the feed-forward modules, so split_ffn = 0 switches them off too).  split_ffn: a
 *   feed-forward module that stands alone (split_chain = 0, a trace without trace_fused, a block whose other chain images were refused for range) runs as one
 *   kernel - the FFN-only form of the chain kernel, on the chain's own image - where that image exists; 0 = LayerNorm + two split GEMMs.
 *   0 / 0 = LayerNorm, split GEMM, GLU kernels per module (tests: the same results within a few 1e-6, another summation order).  A debug trace
 *   (effconf_encoder_trace_*) runs the per-module kernels around the FFN-only form: the chains never write the intermediate states.
 * "trace_fused" (default 0; tests): 1 = a debug trace of the split mode keeps the fused kernels an untraced forward runs (csrc/sxf_sub.hip, csrc/sxf_chain.hip;
 *   the output is bit-identical to the untraced forward's) and records what THEY write to memory: "linear", per block "x_ffn1" (after a head launch or a merged
 *   tail + head), "q" / "k" / "v" (Q without u; chunk-padding rows are never written), "e" (the fp32 positional projection), "att_o", "x_mhsa", "glu", "dw",
 *   "conv_res" (transition blocks) and "out" only where no head is merged into chain A's tail.  "subsample" / "x_conv" exist on the per-module route only.
 * "split_sublin" (default 1; round 6, csrc/sxf_sub.hip): split mode, one-layer subsampler (the EfficientConformer configurations): Conv2d + BatchNorm + Swish + flatten
 *   + Linear as ONE kernel whose (frames, C F') activation stays in registers (the conv as a 16-tap MFMA product whose accumulators are the B fragments of the
 *   Linear's product), ragged batches on the frames that exist; 0 = fp32 VALU convolution + split GEMM (+ row gather) - the same results within a few 1e-6.
 *   Small split step 14.6 -> 12.9 ms.  A debug trace runs the per-module kernels (it wants the "subsample" activation).
 * MODE MATRIX (what a forward accepts; everything else returns an error, never a silent fallback):
 *   bf16 path (exact_fp32 = 0): rectangular batches (effconf_encoder_forward / _forward_mel), ragged batches (effconf_encoder_forward_ragged; head
 *     widths <= 160 padded), streaming contexts / causal configurations (EcConfig; natural Q / K / V layout, head widths <= 160 padded), attention
 *     maps (effconf_encoder_set_attention_outputs; ragged batches since round 4: rectangles sized for the LONGEST utterance, utterance b's own
 *     Tg(b) x Tg(b) block = its map run alone, zeros elsewhere).
 *   split mode (exact_fp32 = 2; round 6): rectangular AND ragged batches, finite left_context / right_context AND causal configurations (causal relative
 *     tables, causal depthwise padding); attention maps on rectangular batches (they run round 4's scores-in-memory kernels of csrc/split.hip).
 *   fp32 mode (exact_fp32 = 1): rectangular batches, attention maps, finite left_context / right_context; NOT ragged batches, NOT causal configurations
 *     (the forward fails). */
int effconf_encoder_set_option(EcEncoder* enc, const char* name, int32_t value);

/* ---- per-launch event profiler (bench / tuning only) --------------------------------------- */
/* When enabled every kernel launch of the forward is bracketed by two hipEventRecord on the caller's stream.
 * Classes: 0 mel, 1 subsample conv, 2 FFN GEMMs, 3 other GEMMs, 4 LayerNorm, 5 attention, 6 depthwise conv, 7 misc.
 * effconf_profile_read synchronises the device and returns, for one class, the summed kernel time, the number of
 * launches and the summed ALGORITHMIC flops / bytes of those launches since the last enable. */
int effconf_profile_enable(EcEncoder* enc, int32_t enable);
int effconf_profile_read(EcEncoder* enc, int32_t cls, double* total_ms, int64_t* launches, double* flops, double* bytes);

/* ---- debug trace (tests only) ------------------------------------------------------------- */
/* When a trace arena is set, every forward copies its intermediate tensors into it (device-to-device,
 * same stream).  Entries describe name / byte offset / rows / cols / leading dim / dtype (0=f32, 1=bf16, 2=i32). */
int effconf_encoder_set_trace(EcEncoder* enc, void* dev_arena, size_t bytes);
int32_t effconf_encoder_trace_count(const EcEncoder* enc);
int effconf_encoder_trace_entry(const EcEncoder* enc, int32_t i, char* name64, int64_t* offset, int64_t* rows, int64_t* cols,
                                int64_t* ld, int32_t* dtype);

/* ---- diagnostics: include/effconf_debug.h, exported by the SEPARATE library libeffconf_debug.so (tests and tools only); libeffconf.so has none of them */

/* ---- attention maps: the third return value of the reference's ConformerEncoder.forward (encoders.py:126-142: att_w of every block,
 * (batch, heads, Tg, Tg) softmax rows; no caller on the hot path reads them, so they are opt-in).  effconf_encoder_attention_dims fills
 * heads[k] / tg[k] per block for inputs of n samples (from_audio) or mel frames; effconf_encoder_set_attention_outputs registers one device
 * buffer of batch * heads[k] * tg[k] * tg[k] floats per block (null entries skip a block; maps = null or n_blocks = 0 clears the
 * registration) - every following effconf_encoder_forward / _forward_ragged writes them (ragged: dims for n = the longest utterance; bf16 path: recomputed in fp32 from the bf16
 * Q / K / E operands; fp32 path: the kernel's own probabilities). */
int effconf_encoder_attention_dims(EcEncoder* enc, int32_t n, int32_t from_audio, int32_t* heads, int32_t* tg);
int effconf_encoder_set_attention_outputs(EcEncoder* enc, float* const* maps, int32_t n_blocks);

/* ---- self-conditioned CTC (the reference's ConformerEncoderInterCTC, encoders.py:144-215): after every listed block
 *     p = softmax(linear_expand_k(x));  x = x + linear_proj_k(p)
 * effconf_encoder_set_interctc: between create and finalize; blocks = n distinct block indices, vocab_size in 2..1024, every listed block's dim_expand
 * <= 768 (checked at finalize, which then also requires linear_expand_<k>.{weight (V, De), bias (V)} and linear_proj_<k>.{weight (De, V), bias (De)}
 * through effconf_encoder_load_tensor).  n = 0 removes the steps.
 * effconf_encoder_set_interctc_outputs: like effconf_encoder_set_attention_outputs - one device buffer per LISTED block in block order (null = skip,
 * probs = null or n = 0 clears); every following forward writes the fp32 probabilities (batch, T_k, V), T_k = frames leaving block k (ragged
 * batches: T_k of the longest utterance, an utterance's own frames and zeros behind them).
 * effconf_interctc: ONE step of listed block `block` on the product kernel: x, y fp32 (rows, dim_expand) dense, y may alias x; probs (rows, V) or
 * null.  workspace is not used by the bf16 kernel (may be null). */
int effconf_encoder_set_interctc(EcEncoder* enc, const int32_t* blocks, int32_t n, int32_t vocab_size);
int effconf_encoder_set_interctc_outputs(EcEncoder* enc, float* const* probs, int32_t n);
int effconf_interctc(EcEncoder* enc, int32_t block, const float* x, int32_t rows, float* y, float* probs, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ---- chunked streaming: the two frame-mixing kernels of a causal encoder that sees its input a chunk at a time, alone on caller-provided
 * operands and state.  All arrays indexed by stream are device int32 [streams]; max_rows (host) >= every rows[b].
 * effconf_stream_attention: stream b owns the rows [row_off[b], row_off[b] + round_up(rows[b], group)) of qu = Q + u, k, v (bf16 rows of `dim`
 *   columns; group-padding rows of a final chunk: qu = u, k = v = 0) and of out (bf16 rows of ld_out columns; group-padding rows are written as
 *   zeros).  rows[b] = 0: the stream idles.  pos[b] = absolute grouped position of its first query, cached[b] = valid grouped rows of its cache (the
 *   positions pos - cached .. pos - 1).  k_cache / v_cache: [streams][capacity] slots of group * dim bf16, a ring - the grouped row of absolute
 *   position p lives in slot p % capacity; no other slot is read.  e: the causal table in its own order, e_rows grouped rows of group * dim bf16 =
 *   pos_layer(sinusoid(group * e_rows - 1 .. 0)): the distance i - j reads grouped row e_rows - 1 - (i - j) at every position;
 *   e_rows > min(band_left, largest position).  Key j is visible
 *   to query i iff 0 <= i - j <= band_left (>= 2^30: unlimited).  dvu: (v - u) per head column [heads][dvu_ld] fp32, zero beyond the head width.
 *   qu, k, e and the rings need 16 bytes of readable slack behind their last row.  append != 0: the chunk's K / V rows then join the rings (of a
 *   chunk longer than the ring its last `capacity` grouped rows); the caller advances pos and sets cached = min(cached + new rows, capacity).
 * effconf_stream_dwconv: causal depthwise convolution (ksize 7 / 15 / 31, stride 1 / 2) + folded BatchNorm + Swish of the rows
 *   g[in_off[b] .. + rows[b]) (bf16, ld columns, ld % 8 == 0) -> out[out_off[b] .. + (rows[b] - 1) / stride + 1).  taps: folded fp32 [ksize][channels],
 *   bias [channels].  state: [streams][ksize - 1][ld] bf16, the rows in front of the chunk, of which the LAST hist[b] are valid (the others read as
 *   zero, whatever they hold).  A chunk of a stride-2 layer starts on an even absolute row.  update_state != 0: the state then becomes the last
 *   ksize - 1 rows of [state | chunk]; the caller sets hist = min(hist + rows, ksize - 1). */
/* Streaming sessions.  A session keeps, for max_streams independent streams of a CAUSAL bf16 encoder, per block the attention keys / values of the left context
 * (a ring of the band's length; an unlimited left_context: as many grouped rows as max_frames mel frames give - max_frames = 0 is then refused) and the last
 * kernel_size - 1 inputs of the depthwise convolution, in ONE caller-provided device buffer of effconf_stream_state_bytes bytes that must outlive the session
 * (its contents need no initialisation).  Refused with the reason: plans that are not causal, right_context > 0, precision "split" / "fp32", InterCTC
 * encoders, the two-layer subsampler.
 * effconf_stream_align: chunk granularity in subsampled rows (12 for every Efficient Conformer: 24 mel frames): every chunk of a stream but its last is a multiple.
 * effconf_stream_push_mel: one round.  `streams`: n distinct stream ids (host); rows[b] >= 1 (host): subsampled rows stream streams[b] encodes now - a
 *   multiple of the alignment unless this is the stream's last chunk.  mel: device fp32 (n, n_mels, mel_pitch), mel_pitch >= 2 max(rows) + 2; column c of
 *   stream b = its mel frame 2 done_b - 2 + c (done_b = rows encoded before this round), ZERO in front of the utterance's first frame and behind its last one.
 *   A row t reads the mel frames 2 t - 1 .. 2 t + 1, so after N frames of an unfinished stream N / 2 rows are complete; an ended stream has (N - 1) / 2 + 1.
 *   out: (n, out_frames, D_last) fp32, zero behind every stream's new frames; out_len: device int64 [n], the new output frames.  The concatenation of a stream's
 *   outputs is the whole-utterance causal forward of its mel frames.  effconf_stream_reset: the stream starts a new utterance. */
typedef struct EcStream EcStream;
int32_t effconf_stream_align(const EcEncoder* enc);
size_t effconf_stream_state_bytes(const EcEncoder* enc, int32_t max_streams, int32_t max_frames);
EcStream* effconf_stream_create(EcEncoder* enc, int32_t max_streams, int32_t max_frames, void* state, size_t state_bytes);
void effconf_stream_destroy(EcStream* session);
int effconf_stream_reset(EcStream* session, int32_t stream);
size_t effconf_stream_workspace_bytes(const EcStream* session, int32_t n, int32_t max_rows, int32_t mel_pitch);
int effconf_stream_push_mel(EcStream* session, const int32_t* streams, int32_t n, const float* mel, int32_t mel_pitch, const int32_t* rows, float* out,
                            int32_t out_frames, int64_t* out_len, void* workspace, size_t workspace_bytes, void* stream);
int effconf_stream_attention(const uint16_t* qu, const uint16_t* k, const uint16_t* v, const uint16_t* e, int32_t e_rows, const float* dvu, int32_t dvu_ld,
                             uint16_t* k_cache, uint16_t* v_cache, int32_t capacity, const int32_t* row_off, const int32_t* rows, const int32_t* cached,
                             const int32_t* pos, int32_t streams, int32_t max_rows, int32_t heads, int32_t group, int32_t dim, int32_t band_left,
                             uint16_t* out, int32_t ld_out, int32_t append, void* stream);
int effconf_stream_dwconv(const uint16_t* g, int32_t ld, int32_t channels, const float* taps, const float* bias, int32_t ksize, int32_t stride,
                          uint16_t* state, const int32_t* in_off, const int32_t* rows, const int32_t* hist, const int32_t* out_off, int32_t streams,
                          int32_t max_rows, uint16_t* out, int32_t update_state, void* stream);

/* ---- host helper of the batching front door (reference: utils/preprocessing.py:33-45, collate_fn_pad zero-pads a sorted batch) -------
 * Copies n host rows src[i][0 .. len[i]) to dst + i * pitch (floats) on `threads` host threads, zero-filling dst[i][len[i] .. pitch) when
 * zero_pad != 0 (ragged batches never read the pad samples: pass 0).  dst is typically pinned memory, so that ONE H2D copy follows.  No
 * device work, no stream; returns when the copy is complete. */
int effconf_host_pack_rows(const float* const* src, const int64_t* len, int32_t n, float* dst, int64_t pitch, int32_t zero_pad,
                           int32_t threads);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* EFFCONF_H */
