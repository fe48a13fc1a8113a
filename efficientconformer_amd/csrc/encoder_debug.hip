// The effconf_debug_* entries of include/effconf_debug.h: libeffconf_debug.so only (tests and tools), never linked into libeffconf.so.
#include "encoder_state.h"
#include "pack.h"
#include "routes.h"

#include <cstdio>
#include "../../include/effconf_debug.h"

namespace {

// The packing runs on a scratch copy `t` of the handle that borrows the host tensors, so e itself never holds a packed pointer: it stays not finalized, and a
// later effconf_encoder_finalize works as if this had not run.  No HIP call: the copy owns no device buffer and upload only hashes (and returns a non-null
// token, so "image exists" reads as after a real finalize).  then(t): what to read off the packed copy
template <class F>
int dry_pack(EcEncoder* e, EcEncoder::PackDigest* d, F then) {
    std::map<std::string, HostTensor> host = std::move(e->host);
    e->host.clear();
    EcEncoder t(*e);
    t.host = std::move(host);
    t.cfg.blocks = t.blocks.data();
    t.allocs.clear();
    t.dry = d;
    const int rc = pack_encoder(&t);
    e->host = std::move(t.host);
    if (rc == 0) { t.tiled_auto_on = tiled_auto_rule(&t); then(t); }
    return rc;
}

const char* const kFront[] = {"two_layer", "chunked", "row_stationary", "tiled_fused", "conv_gemm"};
const char* const kHead[] = {"prev_tail", "chain", "modules"};
const char* const kTail[] = {"full", "tail", "modules"};

}  // namespace

extern "C" {

int effconf_debug_pack_digest(EcEncoder* e, uint64_t* digest, int64_t* buffers, int64_t* bytes) {
    if (!e) return fail("null encoder");
    EcEncoder::PackDigest d;
    const int rc = dry_pack(e, &d, [](const EcEncoder&) {});
    if (digest) *digest = d.sum;
    if (buffers) *buffers = d.buffers;
    if (bytes) *bytes = d.bytes;
    return rc;
}

int effconf_debug_routes(EcEncoder* e, int32_t ragged, char* text, size_t cap) {
    if (!e || !text || !cap) return fail("null argument");
    std::string out;
    EcEncoder::PackDigest d;
    const int rc = dry_pack(e, &d, [&](const EcEncoder& t) {
        char ln[256];
        const FrontScratch fs = front_scratch(&t, ragged != 0, 1, 64, 32);
        snprintf(ln, sizeof(ln), "front %s sub=%d sub1=%d xrect=%d\n", kFront[front_route(&t, ragged != 0)], fs.sub != 0, fs.sub1 != 0, fs.xrect != 0);
        out += ln;
        for (size_t k = 0; k < t.blocks.size(); ++k) {
            const EcBlock& b = t.blocks[k];
            const BlockRoutes r = block_routes(&t, k);
            const bool hm = r.head == HEAD_MODULES, tm = r.tail == TAIL_MODULES, bm = !r.chain_b;
            const AttentionRoute ar = attention_route(&t, ec_round_up(b.group_size * b.dim_model / b.num_heads, 32), ragged != 0, false);      // full context
            auto pick = [](bool applies, bool yes, const char* a, const char* n) { return !applies ? "-" : (yes ? a : n); };
            snprintf(ln, sizeof(ln), "block %d D=%d De=%d head=%s ffn1=%s qkv=%s attention=%s b=%s outp=%s pw1=%s dw=%s res=%s tail=%s pw2=%s ffn2=%s\n", (int)k, b.dim_model,
                     b.dim_expand, kHead[r.head], pick(hm, r.ffn1_fused, "fused", "tiled"), pick(hm, r.qkv_rs, "ln_rs", "ln+tiled"),
                     ar.refusal ? "refused" : (ar.waves == 0 ? "attention" : (ar.waves == 1 ? "attention2/1" : "attention2/2")), r.chain_b ? "chain" : "modules",
                     pick(bm, r.outp_rs, "rs", "tiled"), pick(bm, r.pw1_rs, "ln_rs", "ln+tiled"), r.dw_mfma && t.bw[k].dw_a ? "mfma" : "valu",
                     pick(b.dim_model != b.dim_expand, r.res_rs, "rs", "tiled"), kTail[r.tail], pick(tm, r.pw2_rs, "rs", "tiled"), pick(tm, r.ffn2_fused, "ln_fused", "ln+tiled"));
            out += ln;
        }
        for (int k : t.ic_blocks) {      // handles with self-conditioned CTC steps only (a handle that finalize would refuse never gets here)
            snprintf(ln, sizeof(ln), "interctc %d De=%d V=%d route=%s\n", k, t.blocks[k].dim_expand, t.ic_vocab, interctc_route(&t, k) == IC_FUSED ? "fused" : "refused");
            out += ln;
        }
        if (!t.exact_split) return;
        // the label-exact split schedule, per kind of forward: as it runs untraced, with a debug trace (option trace_fused decides), with attention maps requested
        const char* const kinds[] = {"untraced", "traced", "maps"};
        for (int kind = 0; kind < 3; ++kind) {
            const ExactForwardRoutes f = exact_forward_routes(&t, kind == 1, kind == 2);
            snprintf(ln, sizeof(ln), "split %s family=%s front=%s causal=%s\n", kinds[kind], f.fused ? "fused" : "modules", f.sublin ? "sublin" : "modules", f.refusal ? "refused" : "ok");
            out += ln;
            for (size_t k = 0; k < t.blocks.size(); ++k) {
                const EcBlock& b = t.blocks[k];
                const ExactBlockRoutes r = exact_block_routes(&t, f, k, true, true);      // rectangular and ragged batches alike: a block reads the rows its predecessor wrote
                auto pick = [](bool applies, bool yes) { return !applies ? "-" : (yes ? "fused" : "ln+gemms"); };
                snprintf(ln, sizeof(ln), "split %s block %d D=%d De=%d head=%s ffn1=%s attention=%s b=%s tail=%s ffn2=%s\n", kinds[kind], (int)k, b.dim_model, b.dim_expand, kHead[r.head],
                         pick(r.head == HEAD_MODULES, r.ffn1_fused), f.fused ? "sxf" : (exact_attention_split(&t, b.group_size * b.dim_model / b.num_heads, b.num_heads) ? "sx" : "ex"),
                         r.chain_b ? "chain" : "modules", kTail[r.tail], pick(r.tail == TAIL_MODULES, r.ffn2_fused));
                out += ln;
            }
        }
    });
    if (rc) return rc;
    if (out.size() + 1 > cap) return fail("effconf_debug_routes: text buffer too small");
    memcpy(text, out.c_str(), out.size() + 1);
    return 0;
}

int effconf_debug_relpos_attention(const uint16_t* qu, const uint16_t* k, const uint16_t* v, const uint16_t* e, const float* dvu, int32_t dvu_ld,
                                   const int64_t* lens_dev, const int64_t* lens_host, int32_t batch, int32_t heads, int32_t frames, int32_t group, int32_t dim,
                                   uint16_t* out, int32_t ld_out, int32_t variant, int32_t band_l, int32_t band_r, int32_t causal, int32_t ragged,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    if (!qu || !k || !v || !e || !dvu || !lens_dev || !lens_host || !out || !workspace) return fail("null argument");
    if (batch <= 0 || heads <= 0 || frames <= 0 || group <= 0 || !(group & 1) || dim <= 0 || (group * dim) % heads) return fail("bad attention shape");
    const int Tp = ec_round_up(frames, group), Tg = Tp / group, d = group * dim / heads, dpad = ec_round_up(d, 32);
    if (dpad > 192 || dvu_ld < dpad || ld_out < dim) return fail("unsupported head width / leading dimension");
    if (variant < 0 || variant > 2) return fail("attention variant: 0, 1 or 2");
    if (band_l < 0 || band_r < 0) return fail("band_l / band_r: grouped positions >= 0 (>= Tg: unlimited)");
    if (causal && band_r != 0) return fail("causal attention: band_r must be 0 (the kernel masks j > i through the band only)");
    // ---- the forward's route under option attention_v2 = variant (forward_bf16.hip), refusals included: all of it before the first HIP call
    const bool rg = ragged != 0, streaming = causal || band_l < Tg || band_r < Tg;
    EcEncoder opt;
    opt.attention_v2 = variant;
    const AttentionRoute ar = attention_route(&opt, dpad, rg, streaming);
    if (ar.refusal) return fail(ar.refusal);
    if (ar.waves != variant)
        return fail("the forward's route runs another kernel than the variant asked for (attention_route: streaming and ragged batches on attention2.hip variant 1, padded head width 192 on attention.hip)");
    if (workspace_bytes < ((size_t)7 * batch + 8) * 4) return fail("workspace too small");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int* wsi = reinterpret_cast<int*>(workspace);

    AttnParams ap{};
    ap.qu = qu; ap.kh = k; ap.vt = v; ap.eh = e; ap.dvu = dvu; ap.dvu_ld = dvu_ld;
    ap.B = batch; ap.H = heads; ap.T = frames; ap.G = group; ap.D = dim; ap.d = d; ap.dpad = dpad; ap.Tg = Tg; ap.Tgp = ec_round_up(Tg, 8);
    ap.q_bstride = (long long)Tp * dim; ap.q_hstride = d; ap.q_rowstride = group * dim; ap.e_hstride = d; ap.e_rowstride = group * dim;
    ap.out = out; ap.ldo = ld_out; ap.scale = 1.0f / std::sqrt((float)d);
    ap.band_l = band_l; ap.band_r = band_r; ap.causal = causal ? 1 : 0;
    if (rg) {
        // the descriptors of begin_forward (forward_common.h) for an encoder of ONE block without subsampling; the host totals as make_shapes_ragged takes them
        int tmax = 0, nwg = 0;
        for (int b = 0; b < batch; ++b) {
            if (lens_host[b] < 0 || lens_host[b] > frames) return fail("ragged lengths: 0 .. frames");
            tmax = std::max(tmax, (int)lens_host[b]);
            nwg += heads * ec_cdiv(ec_round_up((int)lens_host[b], group) / group, 64);
        }
        if (tmax != frames) return fail("ragged batch: frames = the longest utterance (the positional rows are built for it)");
        int* cfg = wsi;                                            // block_stride, group, heads of the one block
        int* lens = cfg + 4;                                       // [2][batch]: entering / leaving the block
        int* mel_len = lens + 2 * batch;
        int* row_off = mel_len + batch;                            // [2][batch + 1]
        int* wg_off = row_off + 2 * (batch + 1);
        int* tile_off = wg_off + (batch + 1);
        const int host_cfg[3] = {1, group, heads};
        if (hipMemcpyAsync(cfg, host_cfg, sizeof(host_cfg), hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail("copy failed");
        EC_TRY(launch_lengths_ragged(lens_dev, batch, 0, 1, 0, cfg, cfg + 1, cfg + 2, 1, lens, mel_len, row_off, wg_off, tile_off, nullptr, st));
        ap.lens = lens; ap.rag_off = row_off; ap.rag_wg = wg_off; ap.rag_nwg = nwg; ap.rag_tgmax = Tg;
    } else {
        EC_TRY(launch_lengths(lens_dev, batch, 0, 1, 0, nullptr, 0, wsi, nullptr, st));
        ap.lens = wsi;
    }
    if (ar.waves) EC_TRY(launch_relpos_attention2(ap, ar.waves, st));
    else EC_TRY(launch_relpos_attention(ap, st));
    return 0;
}

int effconf_debug_mel(EcEncoder* e, int32_t variant, int32_t extra_lds, const float* audio, int32_t batch, int32_t n_samples, float* mel,
                      uint32_t* counters, void* stream) {
    if (!e || !e->finalized) return fail("encoder not finalized");
    const int Tm = n_samples / e->cfg.hop_length + 1;
    EC_TRY(launch_mel_debug(variant, extra_lds, audio, batch, n_samples, e->mel, e->cfg.n_fft, e->cfg.hop_length, e->cfg.n_mels, Tm,
                            e->cfg.normalize, e->cfg.mean, e->cfg.std, mel, counters, (hipStream_t)stream));
    return 0;
}

int effconf_debug_neighbour(int32_t kind, int32_t blocks, int32_t lds_bytes, int32_t iters, float* buf, size_t n_floats, void* stream) {
    EC_TRY(launch_debug_neighbour(kind, blocks, lds_bytes, iters, buf, n_floats, (hipStream_t)stream));
    return 0;
}

int effconf_debug_gemm(const uint16_t* a, int32_t lda, const uint16_t* w, int32_t ldw, const float* bias, int32_t m, int32_t n, int32_t k,
                       int32_t epi, int32_t wide, void* c, int32_t ldc, const float* r, int32_t ldr, float alpha, void* stream) {
    if (!a || !w || !bias || !c) return fail("null argument");
    if (epi < EPI_F32 || epi > EPI_GLU_BF16 || (epi == EPI_RESID_F32 && !r)) return fail("epilogue: 0 f32, 1 bf16, 2 swish bf16, 3 residual f32, 4 GLU bf16");
    if (wide < 0 || wide > 3) return fail("wide: 0 .. 3");
    GemmParams p{};
    p.A = a; p.lda = lda; p.W = w; p.ldw = ldw; p.bias = bias; p.M = m; p.N = n; p.K = k;
    p.C = c; p.ldc = ldc; p.R = r; p.ldr = ldr; p.alpha = alpha; p.wide = wide;
    if (wide >= 2 && !gemm256_supported(p, epi)) return fail("gemm256 does not take this shape / alignment");
    EC_TRY(launch_gemm(p, epi, (hipStream_t)stream));
    return 0;
}

int effconf_debug_sx_gemm(const float* a, int32_t lda, const uint16_t* w_hi, const uint16_t* w_lo, int32_t ldh, const float* bias, int32_t m, int32_t n,
                          int32_t k, int32_t epi, float* c, int32_t ldc, const float* r, int32_t ldr, float alpha, void* stream) {
    SxGemmParams q{};
    q.g.A = a; q.g.lda = lda; q.g.bias = bias; q.g.M = m; q.g.N = n; q.g.K = k; q.g.C = c; q.g.ldc = ldc; q.g.R = r; q.g.ldr = ldr; q.g.alpha = alpha; q.g.epi = epi;
    q.Whi = w_hi; q.Wlo = w_lo; q.ldh = ldh;
    const int rc = launch_sx_gemm(q, reinterpret_cast<hipStream_t>(stream));
    return rc ? fail("sx_gemm launch failed rc=" + std::to_string(rc)) : 0;
}

int effconf_debug_pack_dwconv_mfma(const float* w_kc, int32_t ksize, int32_t channels, uint16_t* dst, size_t dst_elems) {
    if (!w_kc || !dst || channels <= 0) return fail("null argument");
    if (!dwconv_mfma_supported(ksize, 1)) return fail("kernel size: 15, 31 or 7");
    if (dst_elems != (size_t)channels * 4 * dwconv_mfma_groups(ksize) * 8) return fail("dst: channels * 4 * groups * 8 bf16");
    pack_dwconv_mfma(w_kc, ksize, channels, dst);          // host memory in, host memory out
    return 0;
}

int effconf_debug_dwconv(const uint16_t* g, int32_t batch, int32_t frames, int32_t channels, int32_t ld, const float* w_kc_host, const float* bias_host,
                         int32_t ksize, int32_t stride, int32_t use_mfma, int32_t causal, uint16_t* out, void* stream) {
    if (!g || !w_kc_host || !bias_host || !out || batch <= 0 || frames <= 0 || channels <= 0 || ld < channels || ld % 8) return fail("bad argument");
    if (use_mfma && !dwconv_mfma_supported(ksize, stride)) return fail("dwconv_mfma_kernel: stride 1, kernel size 15, 31 or 7");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float *dw = nullptr, *db = nullptr; uint16_t* dt = nullptr;
    std::vector<uint16_t> tab;
    if (use_mfma) { tab.resize((size_t)channels * 4 * dwconv_mfma_groups(ksize) * 8); pack_dwconv_mfma(w_kc_host, ksize, channels, tab.data()); }
    // test-only entry: temporary device copies of the taps, synchronous
    if (hipMalloc(&dw, (size_t)ksize * channels * 4) != hipSuccess || hipMalloc(&db, (size_t)channels * 4) != hipSuccess ||
        (use_mfma && hipMalloc(&dt, tab.size() * 2) != hipSuccess)) return fail("hipMalloc failed");
    (void)hipMemcpy(dw, w_kc_host, (size_t)ksize * channels * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(db, bias_host, (size_t)channels * 4, hipMemcpyHostToDevice);
    if (use_mfma) (void)hipMemcpy(dt, tab.data(), tab.size() * 2, hipMemcpyHostToDevice);
    const int to = (frames - 1) / stride + 1;
    const int rc = launch_dwconv(g, batch, frames, to, channels, ld, dw, db, ksize, stride, out, st, nullptr, causal, use_mfma ? dt : nullptr);
    (void)hipStreamSynchronize(st);
    (void)hipFree(dw); (void)hipFree(db); if (dt) (void)hipFree(dt);
    return rc ? fail("launch_dwconv failed rc=" + std::to_string(rc)) : 0;
}

int effconf_debug_spin(double microseconds, void* stream) {
    if (launch_debug_spin(microseconds, reinterpret_cast<hipStream_t>(stream)) != 0) return fail("spin launch failed");
    return 0;
}

int effconf_debug_lds_fill(int32_t mode, int32_t blocks, int32_t waves, const void* src, size_t window, int32_t kib_per_wave, int32_t passes, uint64_t* out, void* stream) {
    EC_TRY(launch_debug_lds_fill(mode, blocks, waves, reinterpret_cast<const char*>(src), window, kib_per_wave, passes, reinterpret_cast<unsigned long long*>(out), (hipStream_t)stream));
    return 0;
}

int effconf_debug_victim(int32_t kind, int32_t blocks, int32_t iters, float* out, void* stream) {
    EC_TRY(launch_debug_victim(kind, blocks, iters, out, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
