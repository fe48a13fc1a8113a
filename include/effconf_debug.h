/* effconf_debug.h - diagnostic entry points of libeffconf_debug.so (efficientconformer_amd/_build.py builds it beside the product library).
 *
 * libeffconf_debug.so = every object of libeffconf.so + csrc/debug.hip (hazard reproducer, spin, LDS-fill probe), the packed-fp32 diagnostic build of
 * csrc/mel.hip, and the entry points below.  It exports the whole product ABI (include/effconf.h) as well, so a test can run on it alone; nothing of the
 * package loads it (tests / tools: efficientconformer_amd._lib.load_debug()).  The product library carries none of these symbols and no packed-fp32 kernel.
 */
#ifndef EFFCONF_DEBUG_H
#define EFFCONF_DEBUG_H
#include "effconf.h"
#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* effconf_mel_frontend with a diagnostic variant of mel_kernel (csrc/mel.hip: 1 canaries, 2 self-verifying hand-offs,
 * 4 workgroup barriers, 8 the build WITH packed-fp32 VALU instructions = round 1's hazardous kernel; bits combine), `extra_lds` bytes of unused dynamic LDS per workgroup, and 8 u32 counters (dev). */
int effconf_debug_mel(EcEncoder* enc, int32_t variant, int32_t extra_lds, const float* audio, int32_t batch, int32_t n_samples,
                      float* mel, uint32_t* counters, void* stream);
/* One synthetic kernel that loads a single compute-unit resource (csrc/debug.hip): kind 0 LDS 16-byte hammer, 1 VALU +
 * transcendental, 2 global loads, 3 global stores, 4 MFMA, 5 LDS publish + barrier loop, 6 LDS 4-byte hammer. */
int effconf_debug_neighbour(int32_t kind, int32_t blocks, int32_t lds_bytes, int32_t iters, float* buf, size_t n_floats, void* stream);
/* One Linear layer on the tiled bf16 GEMM kernels alone (kernel-level tests and tuning of csrc/gemm.hip and csrc/gemm256.hip; reference
 * models/layers.py:57-67): c = epilogue(a w^T + bias).  a: bf16 [m][lda]; w: bf16 [>= round_up(n, 128)][ldw = round_up(k, 64)], zero
 * padded (for GLU: rows interleaved per 32 channels, a | b); bias: [>= round_up(n, 128)].  epi: 0 fp32 [m][ldc], 1 bf16, 2 Swish
 * bf16, 3 fp32 r + alpha * (...), 4 GLU bf16 [m][n / 2].  wide: 0 tile picked by shape, 1 the 128 x 128 kernel, 2 / 3 the LDS-DMA
 * kernel with 256 x 256 / 256 x 128 tiles.  All pointers are device pointers. */
int effconf_debug_gemm(const uint16_t* a, int32_t lda, const uint16_t* w, int32_t ldw, const float* bias, int32_t m, int32_t n, int32_t k,
                       int32_t epi, int32_t wide, void* c, int32_t ldc, const float* r, int32_t ldr, float alpha, void* stream);

/* One self-contained victim: 16 chains per lane of a single instruction class (0 v_fma_f32, 1 v_pk_fma_f32, 2 v_pk_mul/add_f32,
 * 3 v_log/v_exp_f32, 4 v_mul/v_add_f32, 5 integer, 6 wave-local LDS exchange); out dev f32 (blocks * 256 * 16). */
int effconf_debug_victim(int32_t kind, int32_t blocks, int32_t iters, float* out, void* stream);
/* One Linear layer on the split-precision GEMM kernel alone (csrc/split.hip; kernel-level tests and tools/sx_gemm_bench.py): c = epilogue(a w^T
 * + bias) with a fp32 [m][lda], w given as its two fp16 images h = fp16(w), l = fp16((w - h) * 2048), each packed k-tile major [ldh / 32][n][32]
 * (ldh = round_up(k, 32), zero padded: element (row, col) at ((col / 32) * n + row) * 32 + col % 32), products accurate to ~2^-21.  epi: 0 plain, 1 Swish, 2 c = r + alpha * (...).  All pointers are device pointers. */
int effconf_debug_sx_gemm(const float* a, int32_t lda, const uint16_t* w_hi, const uint16_t* w_lo, int32_t ldh, const float* bias, int32_t m, int32_t n,
                          int32_t k, int32_t epi, float* c, int32_t ldc, const float* r, int32_t ldr, float alpha, void* stream);
/* HOST function (no GPU): the A-operand table of dwconv_mfma_kernel (csrc/conv.hip) for folded depthwise taps w_kc [ksize][channels] (fp32):
 * dst [channels][4 rows i][groups q = (ksize + 6) / 4][bf16 hi (4 taps) | bf16 lo (4 taps)] of w[4 q + k - i] (zero outside the taps); tests/test_abi_and_host.py. */
int effconf_debug_pack_dwconv_mfma(const float* w_kc, int32_t ksize, int32_t channels, uint16_t* dst, size_t dst_elems);
/* The depthwise-convolution stage of the ConvolutionModule alone (reference modules.py:516-518 with BatchNorm folded into the taps; csrc/conv.hip): g dev bf16
 * [batch * frames][ld] (GLU output) -> out dev bf16 [batch * ((frames - 1) / stride + 1)][ld] = Swish(sum_j w[j][c] gpad[s t + j][c] + bias[c]); w_kc_host
 * [ksize][channels] / bias_host [channels]: HOST fp32 (the entry uploads them, builds the Toeplitz table for use_mfma = 1 and synchronises: tests only).
 * use_mfma: 1 = dwconv_mfma_kernel (stride 1, kernel size 15 / 31 / 7), 0 = dwconv_kernel (VALU).  causal: pre-padding (k - 1, 0) instead of "same". */
int effconf_debug_dwconv(const uint16_t* g, int32_t batch, int32_t frames, int32_t channels, int32_t ld, const float* w_kc_host, const float* bias_host,
                         int32_t ksize, int32_t stride, int32_t use_mfma, int32_t causal, uint16_t* out, void* stream);
/* One idle wave that occupies `stream` for `microseconds` (tools/overlap_probe.py: the duration of an xGMI transfer a single GPU cannot make). */
int effconf_debug_spin(double microseconds, void* stream);
/* diagnostics (tools/lds_fill_rate_probe.py): `blocks` workgroups of `waves` waves each walk the same `window` bytes of `src` (dev) into LDS, `kib_per_wave`
 * (multiple of 8) 1-KiB wave-instructions per wave and pass; mode 0 = LDS-DMA (global_load_lds_dwordx4), 1 = loads + ds_write_b128.
 * out (dev, 2 * blocks uint64): {cycles, bytes} per workgroup. */
int effconf_debug_lds_fill(int32_t mode, int32_t blocks, int32_t waves, const void* src, size_t window, int32_t kib_per_wave, int32_t passes, uint64_t* out, void* stream);

/* HOST function (no GPU, no HIP call): a dry run of effconf_encoder_finalize on the tensors loaded into `enc` (csrc/pack.hip: every packing step), with the copy
 * to the device replaced by a hash of each buffer (length + contents; the per-buffer hashes are combined order-independently).  Returns what finalize would
 * return (effconf_last_error carries the same text) and the digest, the number of buffers and their bytes.  `enc` itself is left as it was - not finalized, no
 * packed pointer, the host tensors kept - so a later effconf_encoder_finalize works as if this had not run.  The sinusoid and mel tables go through libm:
 * compare digests within one machine only (tools/pack_digest.py, tests/test_pack_host.py). */
int effconf_debug_pack_digest(EcEncoder* enc, uint64_t* digest, int64_t* buffers, int64_t* bytes);

/* HOST function (no GPU, no HIP call): which kernels a forward of `enc` would run under its current options (csrc/routes.h - the functions the forward
 * itself reads), after the same dry run of the packing as above, so `enc` need not be finalized and is left as it was.  Writes NUL-terminated text into
 * `text` (`cap` bytes; 256 per block + 256 suffice): one line "front <two_layer|chunked|row_stationary|tiled_fused|conv_gemm> sub=.. sub1=.. xrect=.." (the
 * route of a rectangular / ragged batch and the workspace scratch it needs) and one line per block, "block k D=.. De=.. head=<prev_tail|chain|modules> ffn1=..
 * qkv=.. attention=<attention|attention2/1|attention2/2|refused> b=<chain|modules> outp=.. pw1=.. dw=<mfma|valu> res=.. tail=<full|tail|modules> pw2=.. ffn2=..";
 * a field that does not apply to the block's route reads "-".  Attention is reported for full context (no streaming mask).
 * A handle set to exact_fp32 = 2 gets, after these, the label-exact split schedule (`cap`: 1024 per block suffice) for each kind of forward, <kind> = untraced |
 * traced (a debug trace is recorded: option trace_fused decides) | maps (attention maps requested): "split <kind> family=<fused|modules> front=<sublin|modules>
 * causal=<ok|refused>" and per block "split <kind> block k D=.. De=.. head=<prev_tail|chain|modules> ffn1=<fused|ln+gemms|-> attention=<sxf|sx|ex>
 * b=<chain|modules> tail=<full|tail|modules> ffn2=<fused|ln+gemms|->" (attention of the per-module family: for a batch of one utterance). */
int effconf_debug_routes(EcEncoder* enc, int32_t ragged, char* text, size_t cap);

/* The attention kernels alone over the whole AttnParams contract (csrc/kernels.h; tests/test_gpu_attention_edges.py): effconf_relpos_attention's operands and
 * layout - qu / k / v dev bf16 rows of `dim` columns with the chunk-padding rows in place, e the positional rows [2 Tp - group][dim], dvu [heads][dvu_ld],
 * out [rows][ld_out] - plus the streaming band, causal tables and ragged batches.  band_l / band_r: grouped positions, >= Tg = unlimited, passed on as they
 * are; causal: e holds Tp rows (the non-negative distances) and band_r must be 0, as the forward's plan guarantees - the kernel masks j > i through the band only.
 * lens_dev: dev int64 [batch] valid frames, lens_host: the same numbers on the host (as a forward gets both).  The int32 lengths the kernel reads are written
 * into `workspace` (dev, (7 batch + 8) * 4 bytes) by the forward's own length kernels.
 * ragged = 0: rows b * Tp + t, `frames` per utterance (keys behind lens[b] masked; every query row computed).
 * ragged = 1: utterances concatenated, each padded to a multiple of `group`, every frame valid; frames = the longest length (e is built for it); the
 *   descriptors rag_off / rag_wg come from launch_lengths_ragged as in a forward (one block, no subsampling), rag_nwg from lens_host.
 * variant 0 attention.hip, 1 / 2 attention2.hip: routed through attention_route (csrc/routes.h) as under option attention_v2 = variant, so streaming or
 * ragged with variant 0 or padded head width 192 is refused with the forward's text; a route that would run another variant than the one asked for is refused too. */
int effconf_debug_relpos_attention(const uint16_t* qu, const uint16_t* k, const uint16_t* v, const uint16_t* e, const float* dvu, int32_t dvu_ld,
                                   const int64_t* lens_dev, const int64_t* lens_host, int32_t batch, int32_t heads, int32_t frames, int32_t group, int32_t dim,
                                   uint16_t* out, int32_t ld_out, int32_t variant, int32_t band_l, int32_t band_r, int32_t causal, int32_t ragged,
                                   void* workspace, size_t workspace_bytes, void* stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
