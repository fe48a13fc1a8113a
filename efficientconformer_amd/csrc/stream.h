// Launch API of the chunked streaming kernels (stream.hip): attention of a chunk's queries against a per-stream K / V cache, and the causal depthwise
// convolution whose left halo is a per-stream state.  Same conventions as kernels.h: device pointers owned by the caller, one stream, nothing allocates or syncs.
#pragma once
#include "common.h"

#include <vector>

// Streams: stream b owns, this round, the rows [row_off[b], row_off[b] + round_up(rows[b], G)) of the chunk row space (rows of D columns, as the Q / K / V
// projection writes them; the group-padding rows of a final chunk hold Qu = u, K = V = 0) and ceil(rows[b] / G) grouped query rows.  rows[b] = 0: nothing to
// do for that stream.  pos[b] = absolute grouped position of its first query; cached[b] = valid grouped rows of its cache, the positions pos - cached .. pos - 1.
//
// Cache: a ring per stream, [B][cap] slots of G * D bf16 for K and for V.  INVARIANT: the grouped row of absolute position p lives in slot p % cap, and only the
// slots of the positions pos - cached .. pos - 1 are ever read (cached <= cap).  Both buffers need 16 bytes of slack behind the last slot (16-byte chunk loads
// of a head span's tail; what they read behind the span is masked).
// Positional rows: the causal table in its own order, n_dist grouped rows of G * D - pos_layer(sinusoid(G n_dist - 1 .. 0)), so the distance delta = i - j
// reads grouped row n_dist - 1 - delta whatever the position: projected once per session.  Distances >= n_dist are never visible when
// n_dist > min(band_l, largest position).  qu, k, e and the rings need 16 bytes of readable slack behind their last row.
// slot (dev [B] or null = identity): the place of stream b of this round in the rings / states.
// Key j is visible to query i (absolute grouped positions) iff 0 <= i - j <= band_l and j >= pos - cached.
struct StreamAttnParams {
    const bf16_t *qu, *k, *v;          // the chunk's rows [rows][D]
    const bf16_t* e; int n_dist;
    const float* dvu; int dvu_ld;      // (v - u) per head column [H][dvu_ld], zero beyond d
    bf16_t *kc, *vc; int cap;          // the rings (cap = 0: no cache, cached must be 0)
    const int *row_off, *rows, *cached, *pos;     // dev [B]
    const int* slot;
    int B, H, G, D, d, dpad;
    int max_rows;                      // host: >= every rows[b] (sizes the grid)
    int band_l;                        // >= 2^30: unlimited
    bf16_t* out; int ldo;              // [rows][ldo]: the un-grouped attention output at the chunk's rows; group-padding rows are written as zeros
    float scale;                       // 1 / sqrt(d)
};
bool stream_attention_supported(int dpad);
int launch_stream_attention(const StreamAttnParams& p, hipStream_t s);
// the chunk's K and V rows join the rings (slots (pos + t) % cap); of a chunk longer than the ring only its last cap grouped rows.  The caller then advances
// pos by the chunk's grouped rows and sets cached = min(cached + them, cap)
int launch_stream_kv_append(const StreamAttnParams& p, hipStream_t s);

// Causal depthwise convolution (k taps, stride s, folded BatchNorm, Swish) of stream b's chunk rows g[in_off[b] .. + rows[b]) -> out[out_off[b] .. + (rows[b] - 1) / s + 1).
// The k - 1 rows in front of the chunk are the stream's state [k - 1][ld] (state + slot(b) * (k - 1) * ld), of which the LAST hist[b] rows are valid (the rest reads
// as zero: hist = 0 before the first chunk).  A chunk of a strided block starts on an even absolute row.  launch_stream_dwconv_state then makes the state the
// last k - 1 rows of [state | chunk]; the caller sets hist = min(hist + rows, k - 1).
struct StreamDwParams {
    const bf16_t* g; int ld, C;        // ld % 8 == 0, ld >= C
    const float *w_kc, *bias;          // folded taps [k][C], bias [C] (launch_dwconv's)
    int ksize, stride;
    bf16_t* state;
    const int *in_off, *rows, *hist, *out_off;    // dev [B]
    const int* slot;                   // as StreamAttnParams::slot
    const int* out_end;                // dev [B] or null: the rows [out_off + outputs, out_end) are written as zeros (group padding of the next block)
    int B, max_rows;
    bf16_t* out;
};
int launch_stream_dwconv(const StreamDwParams& p, hipStream_t s);
int launch_stream_dwconv_state(const StreamDwParams& p, hipStream_t s);

// One round of a streaming session as forward_core (forward_bf16.hip) sees it: the round's streams are the "utterances" of a ragged batch whose rows are the
// chunks' rows, every row-local kernel runs as in a whole-utterance ragged forward, and the three frame-mixing places read this instead -
//   the front end: mel (B, n_mels, mel_pitch), stream b's column c = its mel frame 2 done_b - 2 + c (zeros in front of the utterance and behind its end), run as a
//     RECTANGULAR batch into `xrect` ((B, T1r, D0), T1r = (mel_pitch - 1) / 2 + 1); chunk row i of stream b is its row i + 1
//   attention: stream_attention_kernel on the block's rings and table, then the append
//   depthwise convolution: stream_dwconv_kernel on the block's state, then its update
struct StreamRound {
    const float* mel; int mel_pitch;
    float* xrect; bf16_t *sub, *sub1;          // front-end scratch of the rectangular run
    const int* slot;                           // dev [B]: the streams' places in the session state
    struct Block {
        bf16_t *kc, *vc; int cap;
        const bf16_t* e; int n_dist;
        bf16_t* conv;
        const int *cached, *pos, *hist;        // dev [B], this round's values
    };
    std::vector<Block> blk;
};
