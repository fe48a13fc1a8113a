// libeffconf host side: the C ABI declared in include/effconf.h - the handle's life cycle, the workspace-size queries, the three forward entries on one
// dispatcher, the CTC greedy head, options, profiler and trace readers.  The handle's state: encoder_state.h; weight packing: pack.h / pack.hip; the forward
// schedules: forward_common.h, forward_bf16.hip (with the per-module entries), forward_exact.hip; the diagnostic entries: encoder_debug.hip.
// Everything the forward path does is "enqueue kernels on the caller's stream": no allocation, no synchronisation, no host<->device copies (graph-capturable).
#include "forward_common.h"
#include "pack.h"
#include "routes.h"

#include <cstring>

namespace {

thread_local std::string g_err;

}  // namespace

int ec_fail(const char* msg) { g_err = msg ? msg : "error"; return -1; }   // shared with pack.hip and rnnt.hip

const void* ec_upload(EcEncoder* e, const void* src, size_t used) {
    if (e->dry) {
        // dry run: hash (length, contents) instead of copying; the per-buffer hashes add up, so the digest does not depend on the order of the uploads
        static const char nowhere[16] = {0};
        const unsigned char* p = static_cast<const unsigned char*>(src);
        uint64_t h = 0xcbf29ce484222325ull ^ used;
        size_t i = 0;
        for (; i + 8 <= used; i += 8) { uint64_t w; memcpy(&w, p + i, 8); h = (h ^ w) * 0x100000001b3ull; h ^= h >> 29; }
        for (; i < used; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
        e->dry->sum += h * 0x9E3779B97F4A7C15ull + 1; e->dry->buffers += 1; e->dry->bytes += (int64_t)used;
        return nowhere;
    }
    // guard > 0 (EFFCONF_POISON_GUARDS, a test hook read once at create): every parameter buffer sits between two guard regions of 0xFF
    // bytes (NaN as bf16 and as fp32), so a read past either end of a packed weight shows up in the output instead of depending on
    // what the allocator happened to place next to it
    const size_t guard = e->guard_bytes;
    void* d = nullptr;
    size_t bytes = std::max<size_t>((used + 15) / 16 * 16, 16);
    if (hipMalloc(&d, bytes + 2 * guard) != hipSuccess) return nullptr;
    e->allocs.push_back(d);
    char* base = static_cast<char*>(d) + guard;
    if (guard && (hipMemset(d, 0xFF, guard) != hipSuccess || hipMemset(base + used, 0xFF, bytes - used + guard) != hipSuccess)) return nullptr;
    if (used && hipMemcpy(base, src, used, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return base;
}

namespace {

// Behind the three forward entries: picks the schedule and its workspace layout, checks the caller's workspace, turns audio (in = samples, row pitch n) into the
// mel image in the workspace's mel slot, and enqueues the schedule.  s: the batch's shapes (ragged: with s.Tm = the input's row pitch); out_frames: 0 for
// rectangular batches
int forward_dispatch(EcEncoder* e, const float* in, const int64_t* in_len, int from_audio, int n, const Shapes& s, float* out, int out_frames, int64_t* out_len,
                     void* workspace, size_t workspace_bytes, hipStream_t st) {
    char* ws = reinterpret_cast<char*>(workspace);
    const size_t mel_bytes = from_audio ? al((size_t)s.B * e->cfg.n_mels * s.Tm * 4) : 0;
    Workspace w; XWorkspace xw;
    size_t mel_off;
    if (e->exact_on) { xw = make_xworkspace(e, s); mel_off = xw.total; }      // mel behind the label-exact workspace (the mel kernel is fp32 in every mode)
    else { w = make_workspace(e, s, from_audio != 0); mel_off = w.mel; }
    if (workspace_bytes < (e->exact_on ? xw.total + mel_bytes : w.total)) return fail("workspace too small");
    const float* mel = in;
    if (from_audio) {
        float* m = reinterpret_cast<float*>(ws + mel_off);
        PROF(PC_MEL, 0, (double)s.B * n * 4 + (double)s.B * e->cfg.n_mels * s.Tm * 4);
        // (ablation build: the ragged bf16 forward's mel launch is the one tools/ablate_bench.py drops)
        EC_ABL(s.ragged && !e->exact_on ? 16 : 0, EC_TRY(launch_mel(in, s.B, n, e->mel, e->cfg.n_fft, e->cfg.hop_length, e->cfg.n_mels, s.Tm, e->cfg.normalize,
                                                                    e->cfg.mean, e->cfg.std, m, st, s.ragged ? in_len : nullptr)));
        mel = m;
    }
    // label-exact modes: forward_exact chooses the kernel family (split mode on the fused kernels of sxf*.hip; attention maps are a by-product of split.hip's /
    // exact.hip's scores-in-memory kernels only)
    if (e->exact_on) return forward_exact(e, mel, in_len, from_audio, s, xw, ws, out, out_len, st, out_frames);
    return forward_core(e, mel, in_len, from_audio, s, w, ws, out, out_len, st, out_frames);
}

// ragged batches: every utterance's own length (host) -> its mel frames; false = a length out of range
bool ragged_host_lengths(const EcEncoder* e, const int64_t* host_len, int32_t batch, int32_t n, int32_t from_audio, std::vector<int>* tm) {
    tm->resize(batch);
    for (int b = 0; b < batch; ++b) {
        const int64_t l = host_len[b];
        if (l > n || (from_audio ? l <= e->cfg.n_fft / 2 : l < 1)) return false;
        (*tm)[b] = from_audio ? (int)(l / e->cfg.hop_length + 1) : (int)l;
    }
    return true;
}

}  // namespace

// =================================================================== C ABI
extern "C" {

int effconf_abi_version(void) { return EFFCONF_ABI_VERSION; }
const char* effconf_last_error(void) { return g_err.c_str(); }

EcEncoder* effconf_encoder_create(const EcConfig* cfg) {
    if (!cfg || cfg->num_blocks <= 0 || !cfg->blocks) { fail("null / empty config"); return nullptr; }
    if (cfg->sub_layers < 1 || cfg->sub_layers > 2) { fail("Conv2dSubsampling with 1 or 2 layers is native"); return nullptr; }
    if (cfg->sub_layers == 2 && (cfg->sub_filters[0] % 8 || cfg->sub_filters[1] % 8 || cfg->n_mels % 16)) { fail("two-layer subsampler needs filters % 8 == 0, n_mels % 16 == 0"); return nullptr; }
    { const std::string merr = mel_config_error(*cfg); if (!merr.empty()) { fail(merr); return nullptr; } }
    if (cfg->n_mels % 4) { fail("n_mels = " + std::to_string(cfg->n_mels) + ": must be a multiple of 4 (16-byte rows of the mel image)"); return nullptr; }
    for (int i = 0; i < cfg->num_blocks; ++i) {
        const EcBlock& b = cfg->blocks[i];
        if (b.dim_model % 4 || b.dim_expand % 4 || b.kernel_size > 31 || !(b.kernel_size & 1) || !(b.group_size & 1) ||
            (b.group_size * b.dim_model) % b.num_heads || b.conv_stride < 1 || b.conv_stride > 2 ||
            ec_round_up(b.group_size * b.dim_model / b.num_heads, 32) > 192) {
            fail("unsupported block hyper-parameters at block " + std::to_string(i)); return nullptr;
        }
    }
    if (cfg->left_context < 0 || cfg->right_context < 0) { fail("left_context / right_context must be >= 0"); return nullptr; }
    EcEncoder* e = new EcEncoder();
    e->cfg = *cfg;
    e->blocks.assign(cfg->blocks, cfg->blocks + cfg->num_blocks);
    e->cfg.blocks = e->blocks.data();
    if (const char* g = getenv("EFFCONF_POISON_GUARDS")) e->guard_bytes = atoi(g) > 0 ? (size_t)(atoi(g) > 16 ? atoi(g) : 16) * 1024 : 0;   // value = guard size in KiB (at least 16)   // once per encoder, never on the forward path
    return e;
}

void effconf_encoder_destroy(EcEncoder* e) {
    if (!e) return;
    for (void* p : e->allocs) (void)hipFree(p);
    delete e;
}

int effconf_encoder_load_tensor(EcEncoder* e, const char* key, const float* host, const int64_t* shape, int32_t ndim) {
    if (!e || !key || !host) return fail("null argument");
    HostTensor t;
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= shape[i]; }
    t.data.assign(host, host + n);
    e->host[key] = std::move(t);
    e->finalized = false;
    return 0;
}

int effconf_encoder_finalize(EcEncoder* e) {
    if (!e) return fail("null encoder");
    for (void* p : e->allocs) (void)hipFree(p);
    e->allocs.clear();
    if (int rc = pack_encoder(e)) return rc;
    for (void* p : e->allocs) if (!p) return fail("device allocation failed");
    if (hipDeviceSynchronize() != hipSuccess) return fail("upload failed");
    e->host.clear();
    e->e_cache.clear();
    e->tiled_auto_on = tiled_auto_rule(e);
    e->finalized = true;
    return 0;
}

size_t effconf_encoder_workspace_bytes(const EcEncoder* e, int32_t batch, int32_t n, int32_t from_audio) {
    if (!e || batch <= 0 || n <= 0) return 0;
    const int Tm = from_audio ? n / e->cfg.hop_length + 1 : n;
    const Shapes s = make_shapes(e, batch, Tm);
    size_t bytes = make_workspace(e, s, from_audio != 0).total;
    if (e->exact_pack) bytes = std::max(bytes, make_xworkspace(e, s).total + (from_audio ? al((size_t)batch * e->cfg.n_mels * Tm * 4) : 0));
    return bytes;
}

int32_t effconf_encoder_out_frames(const EcEncoder* e, int32_t n, int32_t from_audio) {
    if (!e || n <= 0) return 0;
    const int Tm = from_audio ? n / e->cfg.hop_length + 1 : n;
    return make_shapes(e, 1, Tm).Tout.back();
}

int effconf_encoder_forward_mel(EcEncoder* e, const float* mel, const int64_t* mel_len, int32_t batch, int32_t n_frames,
                                float* out, int64_t* out_len, void* workspace, size_t workspace_bytes, void* stream) {
    if (!e || !e->finalized) return fail("encoder not finalized");
    if (!mel || !mel_len || !out || !workspace || batch <= 0 || n_frames <= 0) return fail("bad argument");
    return forward_dispatch(e, mel, mel_len, 0, n_frames, make_shapes(e, batch, n_frames), out, 0, out_len, workspace, workspace_bytes, (hipStream_t)stream);
}

int effconf_encoder_forward(EcEncoder* e, const float* audio, const int64_t* x_len, int32_t batch, int32_t n_samples,
                            float* out, int64_t* out_len, void* workspace, size_t workspace_bytes, void* stream) {
    if (!e || !e->finalized) return fail("encoder not finalized");
    if (!audio || !x_len || !out || !workspace || batch <= 0 || n_samples <= e->cfg.n_fft / 2) return fail("bad argument");
    const Shapes s = make_shapes(e, batch, n_samples / e->cfg.hop_length + 1);
    return forward_dispatch(e, audio, x_len, 1, n_samples, s, out, 0, out_len, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- ragged batches: every utterance at its own length (the reference's result for that utterance ALONE: no pad frames exist)
size_t effconf_encoder_workspace_bytes_ragged(const EcEncoder* e, const int64_t* x_len_host, int32_t batch, int32_t n, int32_t from_audio) {
    if (!e || !x_len_host || batch <= 0 || n <= 0) return 0;
    std::vector<int> tm;
    if (!ragged_host_lengths(e, x_len_host, batch, n, from_audio, &tm)) return 0;
    const Shapes s = make_shapes_ragged(e, tm);
    Shapes full = s; full.Tm = from_audio ? n / e->cfg.hop_length + 1 : n;      // the mel image keeps the input's row pitch
    size_t bytes = make_workspace(e, full, from_audio != 0).total;
    if (e->exact_pack) bytes = std::max(bytes, make_xworkspace(e, full).total + (from_audio ? al((size_t)batch * e->cfg.n_mels * full.Tm * 4) : 0));
    return bytes;
}

int effconf_encoder_forward_ragged(EcEncoder* e, const float* x, const int64_t* x_len, const int64_t* x_len_host, int32_t batch, int32_t n,
                                   int32_t from_audio, float* out, int32_t out_frames, int64_t* out_len, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    if (!e || !e->finalized) return fail("encoder not finalized");
    if (e->exact_on && !split_fused_ok(e))
        return fail("ragged batches run on the bf16 path and in the split mode (exact_fp32 = 2, head widths <= 144); exact_fp32 = 1 keeps rectangular batches");
    if (e->exact_on && !e->att_out.empty()) return fail("attention maps of a ragged batch: bf16 path only");
    if (!x || !x_len || !x_len_host || !out || !workspace || batch <= 0 || n <= 0 || out_frames <= 0) return fail("bad argument");
    std::vector<int> tm;
    if (!ragged_host_lengths(e, x_len_host, batch, n, from_audio, &tm)) return fail("ragged lengths out of range (audio: n_fft / 2 < len <= n; mel: 1 <= len <= n)");
    Shapes s = make_shapes_ragged(e, tm);
    if (s.Tout.back() > out_frames) return fail("out_frames smaller than the longest utterance's output");
    s.Tm = from_audio ? n / e->cfg.hop_length + 1 : n;        // pitch of the mel image = the input's row pitch (every utterance masks at its own length)
    return forward_dispatch(e, x, x_len, from_audio, n, s, out, out_frames, out_len, workspace, workspace_bytes, (hipStream_t)stream);
}

int effconf_mel_frontend(EcEncoder* e, const float* audio, int32_t batch, int32_t n_samples, float* mel, void* stream) {
    if (!e || !e->finalized) return fail("encoder not finalized");
    if (!audio || !mel) return fail("mel_frontend: null argument");
    if (batch > 0 && n_samples <= e->cfg.n_fft / 2) return fail("mel_frontend: n_samples must exceed n_fft / 2 (reflect padding)");
    const int Tm = n_samples / e->cfg.hop_length + 1;
    EC_TRY(launch_mel(audio, batch, n_samples, e->mel, e->cfg.n_fft, e->cfg.hop_length, e->cfg.n_mels, Tm,
                      e->cfg.normalize, e->cfg.mean, e->cfg.std, mel, (hipStream_t)stream));
    return 0;
}

int effconf_ctc_greedy(EcEncoder* e, const float* enc_out, const int64_t* out_len, int32_t batch, int32_t t_out,
                       int32_t* labels, int32_t* label_len, float* logits, void* workspace, size_t workspace_bytes, void* stream) {
    if (!e || !e->finalized) return fail("encoder not finalized");
    if (!e->fc_wt) return fail("no CTC head (fc.weight / fc.bias) loaded");
    if (workspace_bytes < (size_t)batch * t_out * 4) return fail("workspace too small");
    int* preds = reinterpret_cast<int*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    // bf16 path: split-bf16 operands on the bf16 matrix pipe (ctc_mfma = 2, the default); fp32-operand mode: the fp32 matrix pipe, bit-identical
    // to the VALU kernel (the label-exact mode keeps the reference's fp32 head)
    const int mode = e->exact_on && e->ctc_mfma == 2 ? 1 : e->ctc_mfma;
    if (mode == 2 && e->fc_hi && launch_ctc_split(enc_out, batch * t_out, e->blocks.back().dim_expand, e->fc_hi, e->fc_lo, e->fc_b, e->cfg.vocab_size,
                                                  preds, logits, st) == 0) {
    } else
    EC_TRY(launch_ctc_argmax(enc_out, batch * t_out, e->blocks.back().dim_expand, e->fc_wt, e->fc_b, e->cfg.vocab_size,
                             preds, logits, st, mode != 0));
    EC_TRY(launch_ctc_collapse(preds, out_len, batch, t_out, labels, label_len, st));
    return 0;
}

int effconf_ctc_greedy_bf16(EcEncoder* e, const uint16_t* enc_out_bf16, const int64_t* out_len, int32_t batch, int32_t t_out,
                            int32_t* labels, int32_t* label_len, float* logits, void* workspace, size_t workspace_bytes, void* stream) {
    if (!e || !e->finalized) return fail("encoder not finalized");
    if (e->exact_on) return fail("effconf_ctc_greedy_bf16 belongs to the bf16 path (the label-exact modes keep fp32 rows and the fp32 head)");
    if (!e->fc_hi || !e->fc_lo) return fail("no CTC head (fc.weight / fc.bias) loaded");
    if (workspace_bytes < (size_t)batch * t_out * 4) return fail("workspace too small");
    int* preds = reinterpret_cast<int*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    EC_TRY(launch_ctc_split(reinterpret_cast<const float*>(enc_out_bf16), batch * t_out, e->blocks.back().dim_expand, e->fc_hi, e->fc_lo, e->fc_b,
                            e->cfg.vocab_size, preds, logits, st, 1));
    EC_TRY(launch_ctc_collapse(preds, out_len, batch, t_out, labels, label_len, st));
    return 0;
}

int effconf_ctc_greedy_margin(EcEncoder* e, const void* enc_out, int32_t enc_is_bf16, const int64_t* out_len, int32_t batch, int32_t t_out,
                              int32_t* labels, int32_t* label_len, float* logits, float* frame_margin, float* min_margin, int32_t* min_frame,
                              void* workspace, size_t workspace_bytes, void* stream) {
    if (!e || !e->finalized) return fail("encoder not finalized");
    if (!e->fc_wt) return fail("no CTC head (fc.weight / fc.bias) loaded");
    if (enc_is_bf16 && e->exact_on) return fail("effconf_ctc_greedy_margin: bf16 rows belong to the bf16 path (the label-exact modes keep fp32 rows and the fp32 head)");
    if (enc_is_bf16 && (!e->fc_hi || !e->fc_lo)) return fail("no CTC head (fc.weight / fc.bias) loaded");
    if (batch < 0 || t_out < 0) return fail("effconf_ctc_greedy_margin: negative batch / t_out");
    if (!min_margin || !min_frame) return fail("effconf_ctc_greedy_margin: min_margin and min_frame are outputs, not optional");
    if (workspace_bytes < (size_t)batch * t_out * 8) return fail("workspace too small");
    int* preds = reinterpret_cast<int*>(workspace);
    float* margin = frame_margin ? frame_margin : reinterpret_cast<float*>(preds + (size_t)batch * t_out);
    hipStream_t st = (hipStream_t)stream;
    const int D = e->blocks.back().dim_expand, V = e->cfg.vocab_size;
    // the head kernel of effconf_ctc_greedy / effconf_ctc_greedy_bf16 for the same handle state, in its margin instance
    if (enc_is_bf16) {
        EC_TRY(launch_ctc_split(reinterpret_cast<const float*>(enc_out), batch * t_out, D, e->fc_hi, e->fc_lo, e->fc_b, V, preds, logits, st, 1, margin));
    } else {
        const float* x = reinterpret_cast<const float*>(enc_out);
        const int mode = e->exact_on && e->ctc_mfma == 2 ? 1 : e->ctc_mfma;
        if (mode == 2 && e->fc_hi && launch_ctc_split(x, batch * t_out, D, e->fc_hi, e->fc_lo, e->fc_b, V, preds, logits, st, 0, margin) == 0) {
        } else
        EC_TRY(launch_ctc_argmax(x, batch * t_out, D, e->fc_wt, e->fc_b, V, preds, logits, st, mode != 0, margin));
    }
    EC_TRY(launch_ctc_collapse(preds, out_len, batch, t_out, labels, label_len, st, margin, min_margin, min_frame));
    return 0;
}

/* Attention maps (reference encoders.py:126-142): maps[k] = device buffer of batch x heads[k] x tg[k] x tg[k] floats for block k, or null. */
int effconf_encoder_attention_dims(EcEncoder* e, int32_t n, int32_t from_audio, int32_t* heads, int32_t* tg) {
    if (!e || !e->finalized || !heads || !tg) return fail("effconf_encoder_attention_dims: null argument / encoder not finalized");
    if (n < 0) return fail("effconf_encoder_attention_dims: negative length");
    const Shapes s = make_shapes(e, 1, from_audio ? n / e->cfg.hop_length + 1 : n);
    for (size_t k = 0; k < e->blocks.size(); ++k) {
        const EcBlock& b = e->blocks[k];
        heads[k] = b.num_heads;
        tg[k] = ec_round_up(s.Tin[k], b.group_size) / b.group_size;
    }
    return 0;
}

int effconf_encoder_set_attention_outputs(EcEncoder* e, float* const* maps, int32_t n_blocks) {
    if (!e) return fail("null encoder");
    if (!maps || n_blocks == 0) { e->att_out.clear(); return 0; }
    if (n_blocks != (int)e->blocks.size()) return fail("effconf_encoder_set_attention_outputs: one pointer per block (null = skip that block)");
    e->att_out.assign(maps, maps + n_blocks);
    return 0;
}

/* Self-conditioned CTC (reference encoders.py:144-215) */
int effconf_encoder_set_interctc(EcEncoder* e, const int32_t* blocks, int32_t n, int32_t vocab_size) {
    if (!e) return fail("null encoder");
    if (n < 0 || (n > 0 && !blocks)) return fail("effconf_encoder_set_interctc: null / negative block list");
    std::vector<int> ks(blocks, blocks + n);
    std::sort(ks.begin(), ks.end());
    for (int i = 0; i < n; ++i) {
        if (ks[i] < 0 || ks[i] >= (int)e->blocks.size()) return fail("effconf_encoder_set_interctc: block " + std::to_string(ks[i]) + " is outside 0.." + std::to_string(e->blocks.size() - 1));
        if (i > 0 && ks[i] == ks[i - 1]) return fail("effconf_encoder_set_interctc: block " + std::to_string(ks[i]) + " is listed twice");
    }
    if (n > 0 && vocab_size < 2) return fail("effconf_encoder_set_interctc: vocab_size must be >= 2");
    e->ic_blocks = ks; e->ic_vocab = n > 0 ? vocab_size : 0; e->ic_out.clear();
    e->finalized = false;          // the images of the steps are built by finalize (which also refuses what the kernel does not take)
    return 0;
}

int effconf_encoder_set_interctc_outputs(EcEncoder* e, float* const* probs, int32_t n) {
    if (!e) return fail("null encoder");
    if (!probs || n == 0) { e->ic_out.clear(); return 0; }
    if (n != (int)e->ic_blocks.size()) return fail("effconf_encoder_set_interctc_outputs: one pointer per InterCTC block in block order (null = skip that block)");
    e->ic_out.assign(probs, probs + n);
    return 0;
}

int effconf_encoder_set_option(EcEncoder* e, const char* name, int32_t value) {
    if (!e || !name) return fail("null argument");
    if (!strcmp(name, "fuse_subsample")) { if (value < 0 || value > 3) return fail("fuse_subsample: 0, 1, 2 or 3"); e->fuse_subsample = value; return 0; }
    if (!strcmp(name, "fuse_chain")) { e->fuse_chain = value != 0; return 0; }
    if (!strcmp(name, "ctc_mfma")) { if (value < 0 || value > 2) return fail("ctc_mfma: 0 (VALU), 1 (fp32 MFMA) or 2 (split-bf16 MFMA)"); e->ctc_mfma = value; return 0; }
    if (!strcmp(name, "wide_gemm")) { if (value < 0 || (value > 3 && value < 16)) return fail("wide_gemm: 0 (by shape), 1 (never), 2 (256-column tile), 3 (128-column tile), >= 16 (by shape with this many 256 x 256 tiles as the threshold)"); e->wide_gemm = value; return 0; }
    if (!strcmp(name, "attention_v2")) { if (value != 0 && value != 1 && value != 2) return fail("attention_v2: 0, 1 or 2"); e->attention_v2 = value; return 0; }
    // former EFFCONF_* environment switches (process-global statics): per-handle options now
    if (!strcmp(name, "chain_full_max")) { if (value < 0 || value > 256) return fail("chain_full_max: widest stage (0..256) that runs chain A as ONE kernel"); e->chain_full_max = value; return 0; }   // widening takes effect at the next finalize (the combined constant blocks are built there)
    if (!strcmp(name, "chain_max_dim")) { e->chain_max_dim = value; return 0; }
    if (!strcmp(name, "chain_small_m")) { e->chain_small_m = value; return 0; }
    if (!strcmp(name, "chain_pair")) { if (value != 0 && value != 5) return fail("chain_pair: 0 (chain.hip everywhere) or 5 (chain3.hip for chain A, chain2.hip for chain B at padded width 256)"); e->chain_pair = value; return 0; }
    if (!strcmp(name, "dwconv_mfma")) { if (value < 0 || value > 2) return fail("dwconv_mfma: 0, 1 (kernel size 15) or 2 (15 / 31 / 7)"); e->dwconv_mfma = value; return 0; }
    if (!strcmp(name, "tiled_min_k")) { e->tiled_min_k = value; return 0; }
    if (!strcmp(name, "tiled_auto")) { e->tiled_auto = value; return 0; }      // 2: every layer with K in (tiled_min_k, 384] whatever the widest stage (tuning)
    if (!strcmp(name, "split_ffn")) { e->split_ffn = value != 0; return 0; }
    if (!strcmp(name, "split_sublin")) { e->split_sublin = value != 0; return 0; }
    if (!strcmp(name, "sub3_auto")) { e->sub3_auto = value != 0; return 0; }
    if (!strcmp(name, "split_chain")) { e->split_chain = value != 0; return 0; }
    if (!strcmp(name, "trace_fused")) { e->trace_fused = value != 0; return 0; }
    if (!strcmp(name, "exact_attention")) { if (value < 0 || value > 2) return fail("exact_attention: 0 (tiled), 2 (tiled, 16-row workgroups) or 1 (one wave per query row)"); e->exact_attention = value; return 0; }
    if (!strcmp(name, "cache_pos_embeddings")) { e->e_cache_on = value != 0; e->e_cache.clear(); return 0; }
    if (!strcmp(name, "exact_fp32")) {
        // 0 = bf16 path, 1 = fp32 operands on the fp32 matrix pipe (exact.hip), 2 = split fp16 operand pairs on the fp16 matrix pipe (split.hip)
        if (!e->finalized) { e->exact_pack = e->exact_on = value != 0; e->exact_split = value == 2; return 0; }
        if (value && !e->exact_pack) return fail("exact_fp32 must be requested before effconf_encoder_finalize (the fp32 weights are uploaded there)");
        if (value == 2 && e->xsplit.empty()) return fail("exact_fp32 = 2 must be requested before effconf_encoder_finalize (the split weight images are built there)");
        e->exact_on = value != 0; e->exact_split = value == 2;
        return 0;
    }
    return fail(std::string("unknown option ") + name);
}

int effconf_profile_enable(EcEncoder* e, int32_t enable) {
    if (!e) return fail("null encoder");
    e->prof_on = enable != 0; e->prof_next = 0; e->prof_rec.clear();
    return 0;
}

int effconf_profile_read(EcEncoder* e, int32_t cls, double* total_ms, int64_t* launches, double* flops, double* bytes) {
    if (!e || cls < 0 || cls >= PC_COUNT) return fail("bad profile class");
    if (hipDeviceSynchronize() != hipSuccess) return fail("sync failed");
    double ms = 0, fl = 0, by = 0; int64_t n = 0;
    for (size_t i = 0; i < e->prof_rec.size(); ++i) {
        if (e->prof_rec[i].cls != cls) continue;
        float t = 0.f;
        if (hipEventElapsedTime(&t, e->prof_ev[2 * i], e->prof_ev[2 * i + 1]) != hipSuccess) return fail("event read failed");
        ms += t; fl += e->prof_rec[i].flops; by += e->prof_rec[i].bytes; ++n;
    }
    *total_ms = ms; *launches = n; *flops = fl; *bytes = by;
    return 0;
}

int effconf_encoder_set_trace(EcEncoder* e, void* dev_arena, size_t bytes) {
    if (!e) return fail("null encoder");
    e->trace_arena = reinterpret_cast<char*>(dev_arena); e->trace_bytes = bytes; e->trace_used = 0; e->trace.clear();
    return 0;
}
int32_t effconf_encoder_trace_count(const EcEncoder* e) { return e ? (int32_t)e->trace.size() : 0; }
int effconf_encoder_trace_entry(const EcEncoder* e, int32_t i, char* name64, int64_t* offset, int64_t* rows, int64_t* cols,
                                int64_t* ld, int32_t* dtype) {
    if (!e || i < 0 || i >= (int)e->trace.size()) return fail("bad trace index");
    const TraceEntry& t = e->trace[i];
    memcpy(name64, t.name, 64);
    *offset = t.offset; *rows = t.rows; *cols = t.cols; *ld = t.ld; *dtype = t.dtype;
    return 0;
}

}  // extern "C"
