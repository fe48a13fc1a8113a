// State of an encoder handle shared by encoder.hip (the C ABI), forward_*.hip (the forward schedules) and pack.hip (the packing steps of
// effconf_encoder_finalize): the handle, its per-block packed weights, the host tensors loaded before finalize, and the error helpers.  Internal to libeffconf.
#pragma once
#include "kernels.h"
#include "../../include/effconf.h"

#include <map>
#include <string>
#include <vector>

int ec_fail(const char* msg);   // encoder.hip: sets the thread's effconf_last_error text, returns -1 (shared with rnnt.hip)
inline int fail(const std::string& m) { return ec_fail(m.c_str()); }
#define EC_TRY(expr) do { int _rc = (expr); if (_rc != 0) return fail(std::string(#expr) + " failed rc=" + std::to_string(_rc)); } while (0)

inline int ld8(int d) { return ec_round_up(d, 8); }

struct HostTensor { std::vector<float> data; std::vector<int64_t> shape; };

struct PackedLinear { const bf16_t* w = nullptr; const float* bias = nullptr; int N = 0, K = 0, ldw = 0; std::vector<float> hbias; /* host copy of the padded bias */ };
struct SubChunkImg { const uint16_t *cimg = nullptr, *wimg = nullptr; const float* bias = nullptr; int ncb = 0, fo = 0; };   // kernels.h: SubChunkParams (null wimg: not built)
struct LNp { const float* g = nullptr; const float* b = nullptr; };

struct BlockW {
    LNp ln_ffn1, ln_att, ln_conv, ln_ffn2, ln_out;
    PackedLinear ffn1_a, ffn1_b, qkv, qkv_nat, pos, outp, pw1, pw2, res, ffn2_a, ffn2_b;
    const bf16_t *ffn1_bp = nullptr, *ffn2_bp = nullptr;   // W2 with the hidden index permuted per 16 (rsgemm.hip)
    const float *u = nullptr, *v = nullptr, *dw_w = nullptr, *dw_b = nullptr;
    const uint16_t* dw_a3 = nullptr;             // pack_dwconv_mfma3: third tap plane, only where the folded taps are large (finalize)
    const uint16_t* dw_a = nullptr;              // pack_dwconv_mfma: Toeplitz rows of the depthwise taps for dwconv_mfma_kernel (stride-1 layers)
    const float* dvu = nullptr; int dvu_ld = 0;   // (v - u) per head column [H][dvu_ld], zero beyond d (attention derives Q + v from Q + u)
    const bf16_t* pos_table = nullptr;   // [2*max_pos-1][ld8(D)], row r <-> position max_pos-1-r
    // fused row-local chains (chain.hip): every weight with its K index permuted per 16; FFN second weight / bias pre-scaled by 1/2
    bool chain_in = false, chain_out = false;          // chain-packed weights exist for the D-wide / De-wide parts of the block
    PackedLinear c_outp, c_pw1, c_pw2, c_qkv, c_f1a, c_f2a;
    const bf16_t *c_f1b_cm = nullptr, *c_f2b_cm = nullptr;      // the same second weights chunk-major (chain3.hip, padded width 256 only): every 32-hidden-unit slab contiguous, in LDS slot order
    const bf16_t *c_f1b = nullptr, *c_f2b = nullptr; const float *c_f1b2 = nullptr, *c_f2b2 = nullptr;
    int c_qkv_chunks = 0, c_pw1_chunks = 0;
    std::vector<float> h_ln_out_g, h_ln_out_b, h_u, h_v, h_f1b2, h_f2b2;     // host copies for the chains' constant blocks
    // split mode (sxf_chain.hip): images in the accumulator layout's k order - out-proj / pointwise-2 (F2), pointwise-1 with GLU row pairs / Q | K | V (F1, pre-norm
    // folded), the two feed-forward modules xc_f (each on its own: null = LayerNorm + two GEMMs for that module) with b2 / 2 and their chunks of 32 hidden units;
    // biases of the F2 products
    const float* xf_b2[2] = {nullptr, nullptr}; int xf_nch[2] = {0, 0};
    const uint16_t *xc_wo = nullptr, *xc_p1 = nullptr, *xc_p2 = nullptr, *xc_qkv = nullptr, *xc_f[2] = {nullptr, nullptr};
    const float *xc_bo = nullptr, *xc_bp2 = nullptr; int xc_nch_p1 = 0;
    bool xc_in = false, xc_out = false;          // the D-wide (out-proj, pointwise-1, FFN1, Q K V) / De-wide (pointwise-2, FFN2) images exist
    const float *cc_b = nullptr, *cc_head = nullptr, *cc_tail = nullptr, *cc_full = nullptr;   // constant blocks (chain_const_layout)
};

struct TraceEntry { char name[64]; int64_t offset, rows, cols, ld; int32_t dtype; };
struct ProfRec { int cls; double flops, bytes; };

struct EcEncoder {
    EcConfig cfg;
    std::vector<EcBlock> blocks;
    std::map<std::string, HostTensor> host;
    bool finalized = false;
    std::vector<void*> allocs;
    int wide_gemm = 0;                    // option "wide_gemm": GemmParams::wide of every tiled GEMM (0 by shape, 1 never, 2 / 3 forced)
    struct PackDigest { uint64_t sum = 0; int64_t buffers = 0, bytes = 0; };
    PackDigest* dry = nullptr;            // effconf_debug_pack_digest (diagnostic library): upload hashes every buffer into *dry and copies nothing to a device
    size_t guard_bytes = 0;               // EFFCONF_POISON_GUARDS (test hook): NaN-filled guard regions around every parameter buffer
    // packed
    const float *sub_w9 = nullptr, *sub_b = nullptr;
    PackedLinear lin;
    const bf16_t* lin_fused = nullptr; int lin_fused_ld = 0;   // Linear weight in the fused kernel's K order (sublinear.hip)
    SubChunkImg sub3, xsub;               // images of the chunked front end (one-layer subsampler only): bf16 (sublinear3.hip) and split mode (sxf_sub.hip)
    const bf16_t* lin_rs = nullptr; const float* conv_tab = nullptr;   // sublinear2.hip: Linear weight [F/2][32 NT][32 CG] (K-permuted per 16), conv taps [32 CG][16]
    int fuse_subsample = 2;                  // front-end kernels: 0 conv + GEMM, 1 sublinear.hip, 2 sublinear2.hip, 3 sublinear3.hip - each where its image exists; the precedence: routes.h front_route
    bool fuse_chain = true;                  // row-local chains (chain.hip) where supported
    int ctc_mfma = 2;                        // CTC head: 2 split-bf16 operands on the bf16 MFMA (bf16 path; fp32 mode falls back to 1), 1 fp32 MFMA (bit-identical to 0), 0 the VALU kernel
    int attention_v2 = 1;                    // 0: attention.hip; 1 (default) / 2: attention2.hip variants where they support the head width (padded <= 160)
    // tuning / test options that used to be process-global environment switches (effconf_encoder_set_option)
    int chain_full_max = 192;
    int dwconv_mfma = 1;                         // stride-1 depthwise convolutions on the matrix pipe (conv.hip dwconv_mfma_kernel): 1 = kernel size 15 (the Efficient Conformer
                                                 // family), 2 = also 31 / 7 (equally accurate, profiles/r5_35_dw_accuracy.txt, but ConformerCTC-Small's 5-frame test utterance sits ON the
                                                 // stated tolerance with either kernel and crosses it with this one's rounding: 0.0608 against 0.06), 0 = dwconv_kernel (VALU) everywhere
    int chain_pair = 5;                      // 5: chain3.hip (chain A) / chain2.hip (chain B) at padded width 256 (D = 240: 147 -> 119 us per tail + head); 0: chain.hip everywhere (the reference the tests compare against)
    int chain_small_m = 4096;                // chain launches of at most this many rows run as 2-wave workgroups (small-batch latency; bit-identical rows)
    int chain_max_dim = 256;                 // fused chains only for stage widths <= this (tuning: wider stages on the per-GEMM / tiled kernels)
    int tiled_auto = 1;                      // wide_gemm = 0: configurations whose widest stage lies in (tiled_min_k, 384] (EfficientConformer Medium: D = 360) send that stage to LayerNorm + the tiled
                                             // GEMMs (+ 2.3 % on Medium, profiles/r6_100_*; neutral where wider stages exist - Large - which keep the row-stationary kernels there); 0 = as before round 6's last session
    bool tiled_auto_on = false;              // the rule's outcome for this configuration (finalize)
    int tiled_min_k = 256;                   // with wide_gemm >= 2: layers with K > this leave the row-stationary kernels for LayerNorm + tiled GEMMs
    std::vector<float*> att_out;             // per block: device buffer [B][H][Tg][Tg] for the softmax maps of the next forward, or null
    int split_chain = 1;                     // split mode: the row-local work of a block as two kernels (sxf_chain.hip) where the width is built; 0 = per-module kernels (tests)
    int sub3_auto = 1;                       // with fuse_subsample = 2: front ends wider than 128 channels / columns on sublinear3.hip (0: the narrower kernels where built, else conv + GEMM)
    int split_sublin = 1;                    // split mode: Conv2dSubsampling + Linear as one kernel (sxf_sub.hip) for the one-layer subsampler; 0 = conv kernel + GEMM [+ row gather] (tests)
    int split_ffn = 1;                       // split mode: a feed-forward module outside a chain as one kernel (sxf_chain.hip's FFN-only form) where its image exists; 0 = LayerNorm + two GEMMs, and no chains (tests)
    bool trace_fused = false;                // split mode: a debug trace keeps the fused kernels (sxf_sub.hip, sxf_chain.hip) and records what THEY write; 0 = a trace selects the per-module kernels
    int exact_attention = 0;                 // fp32 mode: 0 tiled attention kernel (2: its 16-row shape), 1 one wave per query row (round 2's); bit-identical
    // two-layer subsampler (plain Conformer configs): layer-2 implicit-GEMM weight [N][9*Cp] (tap, c_in), folded bias, Cp
    const bf16_t* sub2_w = nullptr; const float* sub2_b = nullptr; int sub2_cp = 0;
    std::vector<BlockW> bw;
    const float *fc_wt = nullptr, *fc_b = nullptr;
    const bf16_t *fc_hi = nullptr, *fc_lo = nullptr;      // fc.weight as split-bf16 MFMA B fragments (launch_ctc_split)
    const int* block_stride = nullptr;
    const int *block_group = nullptr, *block_heads = nullptr;     // ragged batches: attention group size / heads per block (device)
    MelTables mel{};
    // trace
    char* trace_arena = nullptr; size_t trace_bytes = 0, trace_used = 0;
    std::vector<TraceEntry> trace;
    // positional-embedding cache: E = pos_layer(R) depends only on (block, T); when the caller keeps the SAME workspace
    // untouched between forwards (opt-in), the 15-18 small E projections are skipped for an unchanged T
    // One tag per workspace: callers that alternate workspaces (one per stream) keep every one of them warm.
    bool e_cache_on = false;
    struct ECacheTag { const void* ws; int batch, tm; size_t layout; };   // layout: offset of the first E buffer (ragged batches: it moves with the row totals)
    std::vector<ECacheTag> e_cache;          // most recently used last; at most E_CACHE_MAX entries
    static constexpr size_t E_CACHE_MAX = 16;
    bool e_cache_hit(const void* ws, int batch, int tm, size_t layout) const {   // the workspace layout depends on (batch, tm) [+ the row totals]
        for (const ECacheTag& t : e_cache) if (t.ws == ws) return t.batch == batch && t.tm == tm && t.layout == layout;
        return false;
    }
    void e_cache_put(const void* ws, int batch, int tm, size_t layout) {
        e_cache_drop(ws);
        if (e_cache.size() >= E_CACHE_MAX) e_cache.erase(e_cache.begin());
        e_cache.push_back({ws, batch, tm, layout});
    }
    void e_cache_drop(const void* ws) {
        for (size_t i = 0; i < e_cache.size(); ++i) if (e_cache[i].ws == ws) { e_cache.erase(e_cache.begin() + i); break; }
    }
    // fp32-operand "exact" mode (exact.hip): raw fp32 state-dict tensors on the device by key, fp32 sinusoid tables,
    // per-layer BatchNorm scale / shift of the subsampling convs
    bool exact_pack = false, exact_on = false;
    // exact_fp32 = 2: the same schedule with every GEMM / the attention products on the fp16 matrix pipe with split operands (split.hip)
    bool exact_split = false;
    struct SplitW { const uint16_t *hi, *lo; int ldh; };
    std::map<std::string, SplitW> xsplit;    // Linear / 1x1 conv weights by state-dict prefix (+ the stacked "...mhsa.qkv_layer")
    std::map<std::string, const float*> xw;
    std::map<std::pair<int, int>, const float*> xtab;
    const float *xsub_scale[2] = {nullptr, nullptr}, *xsub_shift[2] = {nullptr, nullptr};
    // self-conditioned CTC (effconf_encoder_set_interctc): the listed blocks in block order, the vocabulary, and per listed block the images of interctc.hip -
    // linear_expand_k as a plain packed Linear (rows = vocabulary entries), linear_proj_k with its K (vocabulary) index in accumulator order
    struct InterCtcW { PackedLinear expand; const bf16_t* proj = nullptr; int proj_ld = 0; const float* proj_b = nullptr; };
    std::vector<int> ic_blocks; int ic_vocab = 0;
    std::vector<InterCtcW> ic_w;             // [ic_blocks.size()], filled by finalize
    std::vector<float*> ic_out;              // per listed block: device buffer for the probabilities of the next forward, or null
    int ic_index(size_t k) const {           // position of block k among the listed blocks, -1: no step after block k
        for (size_t i = 0; i < ic_blocks.size(); ++i) if (ic_blocks[i] == (int)k) return (int)i;
        return -1;
    }
    // per-launch event profiler (bench / tuning only; off by default)
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev;          // pairs
    std::vector<ProfRec> prof_rec;
    size_t prof_next = 0;
};

// The one function of the packing path that touches HIP (encoder.hip): `bytes` of host memory into a device buffer of their own, owned by the handle
const void* ec_upload(EcEncoder* e, const void* src, size_t bytes);
template <class T>
const T* upload(EcEncoder* e, const std::vector<T>& v) { return static_cast<const T*>(ec_upload(e, v.data(), v.size() * sizeof(T))); }

inline const HostTensor* find(const EcEncoder* e, const std::string& k) {
    auto it = e->host.find(k);
    return it == e->host.end() ? nullptr : &it->second;
}
