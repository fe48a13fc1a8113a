// What the two forward schedules (forward_bf16.hip, forward_exact.hip) and the C ABI (encoder.hip) share: the shapes of a batch, the two workspace layouts, the
// per-launch profiler, the debug trace, and the parts of a forward that do not depend on the number format - lengths and ragged descriptors, the streaming band,
// the positional-embedding cache decision, the ragged epilogue.  Plain data and functions; internal to libeffconf.
#pragma once
#include "encoder_state.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

// Timing-only ablation build (tools/build_ablate.py: -DEFFCONF_ABLATE into a SEPARATE library, never the product): EFFCONF_SKIP = bit mask of kernel
// families whose launches are dropped (1 attention, 2 chain A, 4 chain B, 8 depthwise conv, 16 mel, 32 subsampling, 64 glue) - what a family costs the
// STEP when three row ranges overlap on three streams (results are wrong by construction)
#ifdef EFFCONF_ABLATE
inline int ablate_mask() { static const int m = getenv("EFFCONF_SKIP") ? atoi(getenv("EFFCONF_SKIP")) : 0; return m; }
#define EC_ABL(bit, stmt) do { if (!(ablate_mask() & (bit))) { stmt; } } while (0)
#else
#define EC_ABL(bit, stmt) do { stmt; } while (0)
#endif

// ------------------------------------------------------------------ shapes + workspace layouts
struct Shapes {
    int B, Tm, T1;                 // Tm / T1: mel frames / frames after the subsampling (of the LONGEST utterance when ragged)
    std::vector<int> Tin, Tout;    // frames entering / leaving each block (longest utterance when ragged)
    // rows of the residual stream entering / leaving each block and of the Q / K / V buffers: B * T (B * Tp for Q / K / V), or - ragged -
    // the sum over the utterances of their frames rounded up to the block's attention group size
    std::vector<long long> Min, Mout, Mq;
    bool ragged = false;
    std::vector<int> wgs, tiles;   // ragged: attention workgroups (heads x 64-query tiles) and depthwise-conv tiles (128 frames) per block
    std::vector<double> tg2;       // ragged: sum over the utterances of (grouped length)^2 per block (attention flop accounting)
    long long Mfinal = 0;          // ragged: rows of the encoder output (sum of the utterances' output frames)
};

inline Shapes make_shapes(const EcEncoder* e, int B, int Tm) {
    Shapes s; s.B = B; s.Tm = Tm;
    int t = Tm;
    for (int i = 0; i < e->cfg.sub_layers; ++i) t = (t - 1) / 2 + 1;
    s.T1 = t;
    for (const EcBlock& b : e->blocks) {
        s.Tin.push_back(t);
        s.Min.push_back((long long)B * t);
        s.Mq.push_back((long long)B * ec_round_up(t, b.group_size));
        if (b.conv_stride > 1) t = (t - 1) / b.conv_stride + 1;
        s.Tout.push_back(t);
        s.Mout.push_back((long long)B * t);
    }
    return s;
}

// ragged batch: `tm[b]` mel frames of every utterance (host).  The same length chain as lengths_ragged_kernel (floor divisions of positive
// numbers), accumulated into the totals the host needs for grids and the workspace.
inline Shapes make_shapes_ragged(const EcEncoder* e, const std::vector<int>& tm) {
    const int B = (int)tm.size(), nb = (int)e->blocks.size();
    int tmax = 0;
    for (int v : tm) tmax = std::max(tmax, v);
    Shapes s = make_shapes(e, B, tmax);
    s.ragged = true;
    s.Min.assign(nb, 0); s.Mout.assign(nb, 0); s.Mq.assign(nb, 0); s.wgs.assign(nb, 0); s.tiles.assign(nb, 0); s.tg2.assign(nb, 0.0);
    for (int b = 0; b < B; ++b) {
        int t = tm[b];
        for (int i = 0; i < e->cfg.sub_layers; ++i) t = (t - 1) / 2 + 1;
        for (int k = 0; k < nb; ++k) {
            const EcBlock& bk = e->blocks[k];
            const int G = bk.group_size, Gn = k + 1 < nb ? e->blocks[k + 1].group_size : 1;
            const int tp = ec_round_up(t, G);
            s.Min[k] += tp; s.Mq[k] += tp;
            s.wgs[k] += bk.num_heads * ec_cdiv(tp / G, 64);
            s.tg2[k] += (double)(tp / G) * (tp / G);
            if (bk.conv_stride > 1) t = (t - 1) / bk.conv_stride + 1;
            const int top = ec_round_up(t, Gn);
            s.Mout[k] += top;
            s.tiles[k] += ec_cdiv(top, 128);
        }
        s.Mfinal += t;
    }
    return s;
}

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

// byte offsets into the caller's workspace.  bf16 schedule (forward_bf16.hip: make_workspace)
struct Workspace {
    size_t total = 0;
    size_t mel, sub, sub1, x0, x1, a, hbuf, qu, kh, vt, eh, o, gbuf, cbuf, xs, lens, preds;
    size_t mel_len = 0, row_off = 0, wg_off = 0, tile_off = 0;     // ragged descriptors (ints)
    size_t xrect = 0;                                              // ragged + unfused front end: rectangular Linear output before the gather
    size_t icp = 0;                                                // InterCTC handles: (rows, V) fp32 probabilities of one step - the trace's copy, a ragged batch's side output before it is padded
    std::vector<size_t> eh_blk;   // per-block E (kept across forwards for the cache)
};
// label-exact schedule (forward_exact.hip: make_xworkspace); the mel image of an audio forward sits behind `total`
struct XWorkspace { size_t total = 0, conv1, sub, x0, x1, a, h, q, k, v, e, o, p1, g, c, lens, scores = 0; size_t qkv_stride = 0;
                    std::vector<size_t> ep_blk;      // sxf.hip forward: the E image of every block (input-independent: kept warm between forwards, as the bf16 path's)
                    size_t kp = 0, vp = 0, ep = 0, xs = 0, xrect = 0, mel_len = 0, row_off = 0, wg_off = 0, tile_off = 0; };     // sxf.hip forward: operand images (bytes / 4), decimated rows, ragged descriptors
Workspace make_workspace(const EcEncoder* e, const Shapes& s, bool from_audio);
XWorkspace make_xworkspace(const EcEncoder* e, const Shapes& s);

// ------------------------------------------------------------------ the two schedules: enqueue one forward on `st` (no allocation, no synchronisation, no
// host <-> device copy: graph-capturable).  mel (B, n_mels, s.Tm) fp32; out (B, frames, D_last), ragged batches (s.ragged, out_frames > 0): zero filled
// behind every utterance's own last frame
struct StreamRound;   // stream.h: a round of a streaming session (ragged shapes; the front end, attention and depthwise convolution read the session's state)
int forward_core(EcEncoder* e, const float* mel, const int64_t* in_len, int from_audio, const Shapes& s, const Workspace& w, char* ws, float* out,
                 int64_t* out_len, hipStream_t st, int out_frames, const StreamRound* sr = nullptr);
int forward_exact(EcEncoder* e, const float* mel, const int64_t* in_len, int from_audio, const Shapes& s, const XWorkspace& w, char* ws, float* out,
                  int64_t* out_len, hipStream_t st, int out_frames);

// ------------------------------------------------------------------ per-launch profiler
struct ProfScope {
    EcEncoder* e; hipStream_t st; bool on;
    ProfScope(EcEncoder* e_, hipStream_t st_, int cls, double flops, double bytes) : e(e_), st(st_), on(e_->prof_on) {
        if (!on) return;
        if (e->prof_next + 2 > e->prof_ev.size()) {
            for (int i = 0; i < 2; ++i) { hipEvent_t ev; (void)hipEventCreate(&ev); e->prof_ev.push_back(ev); }
        }
        e->prof_rec.push_back(ProfRec{cls, flops, bytes});
        (void)hipEventRecord(e->prof_ev[e->prof_next], st);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(e->prof_ev[e->prof_next + 1], st);
        e->prof_next += 2;
    }
};
#define PROF(cls, flops, bytes) ProfScope _prof_scope(e, st, (cls), (double)(flops), (double)(bytes))

enum ProfClass { PC_MEL = 0, PC_SUBCONV = 1, PC_GEMM_FFN = 2, PC_GEMM_OTHER = 3, PC_LAYERNORM = 4, PC_ATTENTION = 5,
                 PC_DWCONV = 6, PC_MISC = 7, PC_COUNT = 8 };

// ------------------------------------------------------------------ debug trace: a copy of an activation into the caller's arena (dtype 0 fp32, 1 bf16); an entry
// that does not fit is dropped
inline void trace_add(EcEncoder* e, hipStream_t st, const char* name, const void* ptr, int64_t rows, int64_t cols, int64_t ld, int dtype) {
    if (!e->trace_arena) return;
    const size_t esz = dtype == 1 ? 2 : 4;
    const size_t bytes = (size_t)rows * ld * esz;
    const size_t off = al(e->trace_used);
    if (off + bytes > e->trace_bytes) return;
    (void)hipMemcpyAsync(e->trace_arena + off, ptr, bytes, hipMemcpyDeviceToDevice, st);
    TraceEntry t{};
    snprintf(t.name, sizeof(t.name), "%s", name);
    t.offset = (int64_t)off; t.rows = rows; t.cols = cols; t.ld = ld; t.dtype = dtype;
    e->trace.push_back(t);
    e->trace_used = off + bytes;
}
// entry "blocks.<k>.<what>"
inline void trace_block(EcEncoder* e, hipStream_t st, int k, const char* what, const void* ptr, int64_t rows, int64_t cols, int64_t ld, int dtype) {
    if (!e->trace_arena) return;
    char nm[64];
    snprintf(nm, sizeof(nm), "blocks.%d.%s", k, what);
    trace_add(e, st, nm, ptr, rows, cols, ld, dtype);
}

// ------------------------------------------------------------------ the format-independent parts of a forward
// Lengths of a batch on the device: lens[k * B + b] = frames of utterance b entering block k (k = blocks: leaving the last).  Ragged batches (kernels.h:
// RaggedRows / RaggedConv) add the descriptor arrays lengths_ragged_kernel leaves in the workspace; null for rectangular ones.
struct BatchRows {
    const Shapes* s = nullptr;
    int B = 0, nb = 0;
    int* lens = nullptr;
    const int *mel_len = nullptr, *row_off = nullptr, *wg_off = nullptr, *tile_off = nullptr;
    const int* lens_at(int k) const { return lens + (size_t)k * B; }
    const int* off_at(int k) const { return row_off + (size_t)k * (B + 1); }
    // rows entering block k (k = blocks: the encoder's output rows)
    RaggedRows rows_at(int k) const {
        RaggedRows r{}; r.off = off_at(k); r.len = lens_at(k); r.n = B;
        r.rows = (int)(k < nb ? s->Min[k] : s->Mfinal); r.tmax = k < nb ? s->Tin[k] : s->Tout[nb - 1];
        return r;
    }
    // block k's strided view: Mo = rows leaving it.  tiled: with the 128-frame output tiles of dwconv.hip's kernels (the bf16 schedule)
    RaggedConv conv_at(int k, int Mo, bool tiled) const {
        RaggedConv rc{};
        rc.in_off = off_at(k); rc.in_len = lens_at(k); rc.out_off = off_at(k + 1); rc.out_len = lens_at(k + 1); rc.n = B; rc.out_rows = Mo;
        if (tiled) { rc.tile_off = tile_off + (size_t)k * (B + 1); rc.tiles = s->tiles[k]; }
        return rc;
    }
};

// Parameter block of the chunked front end (sub_chunked.h) in either format: image `im`, mel (B, n_mels, s.Tm) -> y (s.Min[0] rows, D0); rg = null: rectangular
// rows (b, t), else the batch's ragged descriptors
inline SubChunkParams sub_chunk_params(const EcEncoder* e, const SubChunkImg& im, const float* mel, const Shapes& s, const BatchRows* rg, float* y) {
    SubChunkParams sp{};
    sp.mel = mel; sp.B = s.B; sp.F = e->cfg.n_mels; sp.Tm = s.Tm;
    if (rg) { const RaggedRows r0 = rg->rows_at(0); sp.mel_len = rg->mel_len; sp.off = r0.off; sp.len = r0.len; sp.rows_max = ec_round_up(s.Tin[0], e->blocks[0].group_size); }
    else { sp.To = s.T1; sp.rows_max = s.T1; }
    sp.cimg = im.cimg; sp.wimg = im.wimg; sp.bias = im.bias; sp.ncb = im.ncb; sp.Fo = im.fo;
    sp.y = y; sp.ldy = sp.N = e->blocks[0].dim_model;
    return sp;
}

// Start of every forward: empties the trace, enqueues the lengths kernel (out_len = the lengths leaving the encoder) and records the mel image of an audio forward
template <class W>
int begin_forward(EcEncoder* e, hipStream_t st, const Shapes& s, const W& w, char* ws, const float* mel, const int64_t* in_len, int from_audio, int64_t* out_len,
                  BatchRows* r) {
    const EcConfig& c = e->cfg;
    e->trace.clear(); e->trace_used = 0;
    r->s = &s; r->B = s.B; r->nb = (int)e->blocks.size();
    r->lens = reinterpret_cast<int*>(ws + w.lens);
    {
        PROF(PC_MISC, 0, 0);
        if (s.ragged) {
            int* ml = reinterpret_cast<int*>(ws + w.mel_len); int* ro = reinterpret_cast<int*>(ws + w.row_off);
            int* wo = reinterpret_cast<int*>(ws + w.wg_off); int* to = reinterpret_cast<int*>(ws + w.tile_off);
            EC_TRY(launch_lengths_ragged(in_len, s.B, from_audio, c.hop_length, c.sub_layers, e->block_stride, e->block_group, e->block_heads, r->nb, r->lens, ml,
                                         ro, wo, to, out_len, st));
            r->mel_len = ml; r->row_off = ro; r->wg_off = wo; r->tile_off = to;
        } else {
            EC_TRY(launch_lengths(in_len, s.B, from_audio, c.hop_length, c.sub_layers, e->block_stride, r->nb, r->lens, out_len, st));
        }
    }
    if (from_audio) trace_add(e, st, "mel", mel, (int64_t)s.B * c.n_mels, s.Tm, s.Tm, 0);
    return 0;
}

// End of a ragged forward: the rows of the last block, every utterance padded with zeros to out_frames, into `out`
inline int emit_ragged(EcEncoder* e, hipStream_t st, const BatchRows& r, const float* x, int out_frames, float* out) {
    const int D = e->blocks.back().dim_expand;
    const RaggedRows rl = r.rows_at(r.nb);
    PROF(PC_MISC, 0, (double)r.s->Mfinal * D * 4 + (double)r.B * out_frames * D * 4);
    EC_TRY(launch_emit_rows(x, D, rl.off, rl.len, r.B, out_frames, out, st));
    return 0;
}

// Streaming mask of a block: built after the subsampling, sliced ::stride after every strided block before this one (mask_stride = the product of those strides)
// and ::G in grouped attention (encoders.py:132-136, attentions.py:698): grouped positions compare (mask_stride * G) * (j - i) with the contexts
struct Band { int l, r; };
inline Band band(const EcConfig& c, int mask_stride, int G) {
    const long long unit = (long long)mask_stride * G;
    return Band{(int)std::min<long long>(c.left_context / unit, 1 << 30), (int)std::min<long long>(c.right_context / unit, 1 << 30)};
}

// E = pos_layer(R) of block k depends on the block and the frame count entering it only.  With option cache_pos_embeddings and the caller's workspace left
// untouched between forwards, the small projections are skipped for an unchanged shape.  `layout` tells the schedules (and their buffer layouts) apart on one
// workspace; usable = false: this forward neither reads nor leaves a cache (its buffers lie over whatever another schedule left there).
// While the stream is being CAPTURED into a hipGraph nothing executes: the projections must be part of the graph (a replay recomputes them) and the
// workspace must not be tagged warm (an eager forward before the first replay would read E nobody wrote)
struct ECache { bool hit = false, put = false; int tag = 0; size_t layout = 0; };
inline ECache e_cache_begin(EcEncoder* e, hipStream_t st, const void* ws, const Shapes& s, size_t layout, bool usable) {
    ECache c;
    // (the LONGEST utterance's frame count in a ragged batch, where s.Tm is only the input's row pitch)
    c.tag = s.ragged ? -(s.Tin[0] + 1) : s.Tm; c.layout = layout;
    if (usable) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        const bool capturing = hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
        c.put = !capturing;
        c.hit = !capturing && e->e_cache_on && e->e_cache_hit(ws, s.B, c.tag, layout);
    }
    if (!c.hit) e->e_cache_drop(ws);       // re-tagged (e_cache_end) only after every projection of this forward was enqueued
    return c;
}
inline void e_cache_end(EcEncoder* e, const void* ws, const Shapes& s, const ECache& c) {
    if (c.put) e->e_cache_put(ws, s.B, c.tag, c.layout);
}
