// Chunked streaming sessions of a causal encoder: the state of `max_streams` streams in ONE caller-provided device buffer - per block the
// K / V rings and the depthwise convolution's left halo of every stream, the block's positional table (projected once, at the first push) and this round's
// descriptors - and the host-side position counters.  A push is ONE round of forward_core (forward_bf16.hip) over the chunks' rows as a ragged batch; nothing of
// the block loop lives here.
#include "forward_common.h"
#include "routes.h"
#include "stream.h"

#include <cstring>

struct EcStream {
    EcEncoder* e = nullptr;
    int S = 0, max_frames = 0;
    char* state = nullptr;
    struct Blk { size_t kc, vc, conv, e; int cap, n_dist, rows_max; };
    std::vector<Blk> blk;
    size_t desc = 0, desc_bytes = 0, total = 0;
    std::vector<std::vector<int>> rows_in, cached, hist;      // [block][stream]: rows the block has seen, valid ring rows, valid halo rows
    bool e_ready = false;
    // descriptors travel through pinned host slots; a slot is reused only after the copy out of it has completed
    static constexpr int NSLOT = 4;
    char* pinned = nullptr; hipEvent_t ev[NSLOT] = {}; bool ev_used[NSLOT] = {}; int next = 0;
};

namespace {

// Chunk granularity in subsampled rows: every block needs its chunks to start on a multiple of its attention group (in ITS rows) and strided blocks on a
// multiple of their stride - in subsampled rows, group x (product of the strides before the block) and the cumulative stride behind a strided block
int stream_align_rows(const EcEncoder* e) {
    auto gcd = [](long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; };
    long long l = 1, ms = 1;
    for (const EcBlock& b : e->blocks) {
        const long long g = (long long)b.group_size * ms;
        l = l / gcd(l, g) * g;
        ms *= b.conv_stride;
        l = l / gcd(l, ms) * ms;
    }
    return (int)l;
}

std::string stream_refusal(const EcEncoder* e) {
    if (!e || !e->finalized) return "encoder not finalized";
    if (!e->cfg.causal) return "streaming sessions need a causal plan (causal: true): the symmetric depthwise padding and the two-sided relative positions of other plans look ahead";
    if (e->cfg.right_context != 0) return "streaming sessions with lookahead (right_context > 0) are not native";
    if (e->exact_on) return "streaming sessions run on the bf16 path (precision \"split\" / \"fp32\" is not native)";
    if (!e->ic_blocks.empty()) return "streaming sessions of InterCTC encoders are not native";
    if (e->cfg.sub_layers != 1) return "streaming sessions need the one-layer subsampler (the two-layer subsampler of the plain Conformer configurations is not native here)";
    for (const EcBlock& b : e->blocks)
        if (!stream_attention_supported(ec_round_up(b.group_size * b.dim_model / b.num_heads, 32))) return "head width not served by the streaming attention kernel";
    return "";
}

// the layout of the state buffer (max_frames = 0: sized for utterances up to max_pos_encoding)
bool stream_layout(const EcEncoder* e, int S, int max_frames, EcStream* out, std::string* why) {
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += al(bytes); return o; };
    int t = max_frames > 0 ? (max_frames - 1) / 2 + 1 : 0, ms = 1;
    out->blk.clear();
    for (const EcBlock& b : e->blocks) {
        const int G = b.group_size, D = b.dim_model, H = b.num_heads, dpad = ec_round_up(G * D / H, 32);
        const int bl = std::min(band(e->cfg, ms, G).l, b.max_pos / G);      // no sequence is longer than max_pos_encoding: an unlimited context ends there
        const int tg = ec_cdiv(t, G);
        EcStream::Blk k{};
        k.cap = max_frames > 0 ? std::min(bl, tg) : bl;
        k.n_dist = (max_frames > 0 ? std::min(bl, std::max(tg - 1, 0)) : bl) + 1;
        k.rows_max = max_frames > 0 ? t : 0;
        k.n_dist = std::max(std::min(k.n_dist, b.max_pos / G), 1);      // no sequence is longer than max_pos_encoding: larger distances do not exist
        const size_t GD = (size_t)G * D;
        k.kc = take((size_t)S * k.cap * GD * 2 + 256);
        k.vc = take((size_t)S * k.cap * GD * 2 + 256);
        k.conv = take((size_t)S * (b.kernel_size - 1) * ld8(b.dim_expand) * 2 + 256);
        k.e = take((size_t)k.n_dist * std::max((size_t)H * dpad, GD) * 2 + 512);
        out->blk.push_back(k);
        ms *= b.conv_stride;
        if (b.conv_stride > 1) t = t > 0 ? (t - 1) / b.conv_stride + 1 : 0;
    }
    out->desc_bytes = al((size_t)S * 8) + al((size_t)S * 4) * (1 + 3 * e->blocks.size());
    out->desc = take(out->desc_bytes);
    out->total = off;
    return true;
}

struct FrontWin { size_t sub, sub1, xrect, total; int T1; };
FrontWin front_window(const EcEncoder* e, int n, int mel_pitch) {
    FrontWin f{};
    f.T1 = (mel_pitch - 1) / 2 + 1;
    const FrontScratch fs = front_scratch(e, false, (size_t)n, (size_t)mel_pitch, (size_t)f.T1);
    size_t off = 0;
    f.sub = off; off += al(fs.sub);
    f.sub1 = off; off += al(fs.sub1);
    f.xrect = off; off += al(((size_t)n * f.T1 + 1) * e->lin.N * 4);
    f.total = off;
    return f;
}

std::vector<int> round_tm(const int32_t* rows, int n) { std::vector<int> tm(n); for (int b = 0; b < n; ++b) tm[b] = 2 * rows[b] - 1; return tm; }

}  // namespace

extern "C" {

int32_t effconf_stream_align(const EcEncoder* e) {
    if (!e || e->blocks.empty()) { fail("null encoder"); return 0; }
    return stream_align_rows(e);
}

size_t effconf_stream_state_bytes(const EcEncoder* e, int32_t max_streams, int32_t max_frames) {
    const std::string r = stream_refusal(e);
    if (!r.empty()) { fail(r); return 0; }
    if (max_streams <= 0 || max_frames < 0) { fail("bad argument"); return 0; }
    EcStream s; std::string why;
    if (!stream_layout(e, max_streams, max_frames, &s, &why)) { fail(why); return 0; }
    return s.total;
}

EcStream* effconf_stream_create(EcEncoder* e, int32_t max_streams, int32_t max_frames, void* state, size_t state_bytes) {
    const std::string r = stream_refusal(e);
    if (!r.empty()) { fail(r); return nullptr; }
    if (max_streams <= 0 || max_frames < 0 || !state) { fail("bad argument"); return nullptr; }
    EcStream* s = new EcStream();
    std::string why;
    if (!stream_layout(e, max_streams, max_frames, s, &why)) { fail(why); delete s; return nullptr; }
    if (state_bytes < s->total) { fail("stream state buffer too small (effconf_stream_state_bytes)"); delete s; return nullptr; }
    s->e = e; s->S = max_streams; s->max_frames = max_frames; s->state = reinterpret_cast<char*>(state);
    const size_t nb = e->blocks.size();
    s->rows_in.assign(nb, std::vector<int>(max_streams, 0)); s->cached = s->rows_in; s->hist = s->rows_in;
    if (hipHostMalloc(reinterpret_cast<void**>(&s->pinned), s->desc_bytes * EcStream::NSLOT, hipHostMallocDefault) != hipSuccess) { fail("pinned allocation failed"); delete s; return nullptr; }
    for (int i = 0; i < EcStream::NSLOT; ++i) (void)hipEventCreateWithFlags(&s->ev[i], hipEventDisableTiming);
    return s;
}

void effconf_stream_destroy(EcStream* s) {
    if (!s) return;
    for (int i = 0; i < EcStream::NSLOT; ++i) if (s->ev[i]) (void)hipEventDestroy(s->ev[i]);
    if (s->pinned) (void)hipHostFree(s->pinned);
    delete s;
}

int effconf_stream_reset(EcStream* s, int32_t stream) {
    if (!s || stream < 0 || stream >= s->S) return fail("stream_reset: bad stream");
    for (size_t k = 0; k < s->rows_in.size(); ++k) s->rows_in[k][stream] = s->cached[k][stream] = s->hist[k][stream] = 0;      // what the buffers hold is never read again
    return 0;
}

size_t effconf_stream_workspace_bytes(const EcStream* s, int32_t n, int32_t max_rows, int32_t mel_pitch) {
    if (!s || n <= 0 || n > s->S || max_rows <= 0 || mel_pitch < 2 * max_rows + 2) { fail("stream_workspace_bytes: bad argument (mel_pitch >= 2 max_rows + 2)"); return 0; }
    std::vector<int> tm(n, 2 * max_rows - 1);
    Shapes sh = make_shapes_ragged(s->e, tm);
    return al(make_workspace(s->e, sh, false).total) + front_window(s->e, n, mel_pitch).total;
}

int effconf_stream_push_mel(EcStream* s, const int32_t* streams, int32_t n, const float* mel, int32_t mel_pitch, const int32_t* rows, float* out,
                            int32_t out_frames, int64_t* out_len, void* workspace, size_t workspace_bytes, void* stream) {
    if (!s || !streams || !mel || !rows || !out || !out_len || !workspace || n <= 0 || n > s->S) return fail("stream_push_mel: bad argument");
    EcEncoder* e = s->e;
    const std::string r = stream_refusal(e);           // the encoder may have changed its precision since the session was created
    if (!r.empty()) return fail(r);
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)e->blocks.size(), S = s->S;
    int max_rows = 0;
    std::vector<char> seen(S, 0);
    for (int b = 0; b < n; ++b) {
        if (streams[b] < 0 || streams[b] >= S || seen[streams[b]]) return fail("stream_push_mel: stream ids must be distinct and < max_streams");
        seen[streams[b]] = 1;
        if (rows[b] <= 0) return fail("stream_push_mel: every listed stream brings at least one row");
        max_rows = std::max(max_rows, rows[b]);
    }
    if (mel_pitch < 2 * max_rows + 2) return fail("stream_push_mel: mel_pitch must be >= 2 max(rows) + 2");
    // every block's view of the chunks: rows entering it, and the checks that keep a chunk on the block's grid
    std::vector<std::vector<int>> nin(nb, std::vector<int>(n));
    for (int b = 0; b < n; ++b) {
        int t = rows[b];
        for (int k = 0; k < nb; ++k) {
            const EcBlock& bk = e->blocks[k];
            const int had = s->rows_in[k][streams[b]];
            if (had % bk.group_size || had % bk.conv_stride)
                return fail("stream_push_mel: a stream's earlier chunk was no multiple of the alignment (effconf_stream_align) - only its last chunk may be");
            if (s->blk[k].rows_max && had + t > s->blk[k].rows_max) return fail("stream_push_mel: the stream grows beyond the session's max_frames");
            if (had + t > bk.max_pos) return fail("stream_push_mel: the stream grows beyond max_pos_encoding");
            nin[k][b] = t;
            if (bk.conv_stride > 1) t = (t - 1) / bk.conv_stride + 1;
        }
    }
    Shapes sh = make_shapes_ragged(e, round_tm(rows, n));
    if (sh.Tout.back() > out_frames) return fail("out_frames smaller than the longest chunk's output");
    const Workspace w = make_workspace(e, sh, false);
    const FrontWin fw = front_window(e, n, mel_pitch);
    if (workspace_bytes < al(w.total) + fw.total) return fail("workspace too small (effconf_stream_workspace_bytes)");
    char* ws = reinterpret_cast<char*>(workspace);
    char* fws = ws + al(w.total);

    // ---- this round's descriptors: host slot -> the state buffer
    const int slot = s->next; s->next = (s->next + 1) % EcStream::NSLOT;
    if (s->ev_used[slot] && hipEventSynchronize(s->ev[slot]) != hipSuccess) return fail("stream_push_mel: event wait failed");
    char* hd = s->pinned + (size_t)slot * s->desc_bytes;
    char* dd = s->state + s->desc;
    const size_t i8 = al((size_t)S * 8), i4 = al((size_t)S * 4);
    int64_t* h_len = reinterpret_cast<int64_t*>(hd);
    int* h_slot = reinterpret_cast<int*>(hd + i8);
    auto h_blk = [&](int k, int which) { return reinterpret_cast<int*>(hd + i8 + i4 * (1 + 3 * k + which)); };
    auto d_blk = [&](int k, int which) { return reinterpret_cast<const int*>(dd + i8 + i4 * (1 + 3 * k + which)); };
    for (int b = 0; b < n; ++b) {
        h_len[b] = 2 * (int64_t)rows[b] - 1;            // "mel frames" whose subsampled length is rows[b]: the ragged descriptors are the chunks'
        h_slot[b] = streams[b];
        for (int k = 0; k < nb; ++k) {
            h_blk(k, 0)[b] = s->cached[k][streams[b]];
            h_blk(k, 1)[b] = s->rows_in[k][streams[b]] / e->blocks[k].group_size;
            h_blk(k, 2)[b] = s->hist[k][streams[b]];
        }
    }
    if (hipMemcpyAsync(dd, hd, s->desc_bytes, hipMemcpyHostToDevice, st) != hipSuccess) return fail("stream_push_mel: descriptor copy failed");
    (void)hipEventRecord(s->ev[slot], st); s->ev_used[slot] = true;

    // ---- the positional tables: E = pos_layer(sinusoid(G n_dist - 1 .. 0)) per block, once per session (forward_core's projection, the table's last rows)
    if (!s->e_ready) {
        for (int k = 0; k < nb; ++k) {
            const EcBlock& bk = e->blocks[k];
            const BlockW& W = e->bw[k];
            const int D = bk.dim_model, erows = bk.group_size * s->blk[k].n_dist;
            GemmParams pe{};
            pe.A = W.pos_table + (size_t)(bk.max_pos - erows) * ld8(D); pe.lda = ld8(D);
            pe.W = W.pos.w; pe.ldw = W.pos.ldw; pe.bias = W.pos.bias;
            pe.M = erows; pe.N = D; pe.K = D;
            pe.C = s->state + s->blk[k].e; pe.ldc = D;
            PROF(PC_GEMM_OTHER, 2.0 * erows * (double)D * D, (double)erows * D * 4 + (double)D * D * 2);
            EC_TRY(launch_gemm(pe, EPI_BF16, st));
        }
        s->e_ready = true;
    }

    StreamRound sr;
    sr.mel = mel; sr.mel_pitch = mel_pitch;
    sr.sub = reinterpret_cast<bf16_t*>(fws + fw.sub); sr.sub1 = reinterpret_cast<bf16_t*>(fws + fw.sub1); sr.xrect = reinterpret_cast<float*>(fws + fw.xrect);
    sr.slot = reinterpret_cast<const int*>(dd + i8);
    for (int k = 0; k < nb; ++k) {
        StreamRound::Block bk{};
        bk.kc = reinterpret_cast<bf16_t*>(s->state + s->blk[k].kc); bk.vc = reinterpret_cast<bf16_t*>(s->state + s->blk[k].vc); bk.cap = s->blk[k].cap;
        bk.e = reinterpret_cast<const bf16_t*>(s->state + s->blk[k].e); bk.n_dist = s->blk[k].n_dist;
        bk.conv = reinterpret_cast<bf16_t*>(s->state + s->blk[k].conv);
        bk.cached = d_blk(k, 0); bk.pos = d_blk(k, 1); bk.hist = d_blk(k, 2);
        sr.blk.push_back(bk);
    }
    EC_TRY(forward_core(e, nullptr, reinterpret_cast<const int64_t*>(dd), 0, sh, w, ws, out, out_len, st, out_frames, &sr));

    for (int b = 0; b < n; ++b)
        for (int k = 0; k < nb; ++k) {
            const EcBlock& bk = e->blocks[k];
            const int sid = streams[b], t = nin[k][b];
            s->rows_in[k][sid] += t;
            s->cached[k][sid] = std::min(s->cached[k][sid] + ec_cdiv(t, bk.group_size), s->blk[k].cap);
            s->hist[k][sid] = std::min(s->hist[k][sid] + t, bk.kernel_size - 1);
        }
    return 0;
}

}  // extern "C"
