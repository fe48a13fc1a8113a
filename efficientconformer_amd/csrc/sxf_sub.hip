// Split-precision front end as ONE kernel (round 6): Conv2d(1, C, 3 x 3, stride 2, pad 1) + folded BatchNorm + Swish + transpose / flatten + Linear
// (reference modules.py:232-249 Conv2dSubsampling, encoders.py:113-116) for the one-layer subsampler of the EfficientConformer configurations.
//
// The per-module path (exact.hip ex_conv2d_flat1_kernel + split.hip sx_gemm_kernel [+ gather_rows_kernel for ragged batches]) writes the (frames, C F') fp32
// activation to HBM and reads it back - 2 x 2.8 GB per Small step at B = 256, 2.6 of the split step's 21 serial milliseconds - and runs both on the rectangle a row
// range's LONGEST utterance spans.  Here the activation never leaves the registers; the structure is that of sxf_chain.hip's FFN stage (a wave keeps 32 frames, TRANSPOSED: frames = MFMA
// columns = lanes), with the 3 x 3 mel patch in the place of the normalised row:
//   * hidden unit (f', c) = Swish(BN(conv)) of output frequency f' and channel c; chunk = 32 channels of one f' (k index c F' + f' of the Linear, encoders.py:114);
//   * first product  H^T = Wc_cb P_f'^T : A operand = the conv taps of 32 channels (9 taps x BN scale, the BN shift + conv bias in tap 9 against a constant 1; 16-wide
//     k-step), B operand = this lane's patch mel[2 f' - 1 .. 2 f' + 1][2 t - 1 .. 2 t + 1] (zero outside the utterance's own image: what it sees when run alone), three
//     MFMAs (h h, h l, l h); the patch rows are carried from f' to f' + 1 (row 2 f' + 1 is the next patch's first) and the next two rows are requested one f' ahead;
//   * Swish on the accumulator registers, which ARE the B fragments of the second product  Y^T += Wl_chunk H^T  (k order of the Linear's image permuted to the
//     accumulator layout at pack time, encoder.hip); Linear images stream through the two-stage LDS ring of sxf_chain.hip (one LDS-only barrier per chunk);
//   * ragged batches: workgroup = (utterance, 128 frames); rows off[b] + t, the group-padding rows behind an utterance's last frame are written as zeros (what
//     gather_rows_kernel left there).  Arithmetic: same-scale split (sx_common.h split2s): mel at 2^6, activations at 2^8, weights at 2^10, one fp32 accumulator per sum.
#include "kernels.h"
#include "sx_common.h"

namespace {

using namespace sx;

constexpr float SP = 64.0f, SA = 256.0f, SW = 1024.0f;           // operand scales: mel patch, hidden activation, weights (pack.hip packs both images with SW)
constexpr float UNS1 = 1.0f / (SP * SW), UNS2 = 1.0f / (SA * SW);

#define SUB_PIN(v) asm volatile("" : "+v"(v))
// The split format of sub_chunked.h: every operand as two fp16 halves at one scale (sx_common.h split2s), three MFMAs per product (h h, h l, l h) on one fp32
// accumulator: the first product at the scale SP SW, the second - two weight planes in the ring - at SA SW
struct F16Fmt {
    typedef f16x8 frag;
    static constexpr int PLANES = 2, KINDS = 3, OCC2_MAX = 4;
    typedef f16x8 Hidden[2][2];                                 // [h | l][k-step]
    static __device__ __forceinline__ f32x16 mfma(const f16x8& a, const f16x8& b, const f32x16& c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ void split_patch(const float (&v)[8], f16x8& ah, f16x8& al) {
        uint32_t hh[4], ll[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) split2s(v[2 * e] * SP, v[2 * e + 1] * SP, hh[e], ll[e]);
        ah = as_f16x8(make_uint4(hh[0], hh[1], hh[2], hh[3])); al = as_f16x8(make_uint4(ll[0], ll[1], ll[2], ll[3]));
    }
    // Swish (modules.py:240) of a finished first-product chunk -> split B fragments of the second product, as 184 single-instruction steps (the scheme of sxf_chain.hip:
    // exp through v_exp_f32 with the rounding of its argument corrected to first order, 1 / x by v_rcp_f32).  Four values at a time, stage-major inside the four;
    // value r = register r of the accumulators <-> k position 8 kh + (r & 7) of k-step r >> 3.  Every step ends in an empty volatile asm on its result: the steps are
    // pure arithmetic, which instruction selection otherwise sinks behind the last MFMA whatever fences stand in the source.
    struct SwishState { float x[16], y[16], w[16]; uint32_t hh[8], ll[8]; };
    static constexpr int SWISH_STEPS = 16 * 11 + 8;
    static __device__ __forceinline__ void swish_step(int idx, const f32x16& h, SwishState& q) {
        const int g = idx / 46, o = idx - 46 * g;
        if (o >= 44) { const int pr = 2 * g + (o - 44); split2s(q.x[2 * pr], q.x[2 * pr + 1], q.hh[pr], q.ll[pr]); SUB_PIN(q.hh[pr]); SUB_PIN(q.ll[pr]); return; }
        const int stage = (o >> 2) + 2, r = 4 * g + (o & 3);
        switch (stage) {
            case 2: q.x[r] = h[r] * UNS1; SUB_PIN(q.x[r]); break;
            case 3: q.y[r] = fminf(-q.x[r], 87.0f); SUB_PIN(q.y[r]); break;
            case 4: q.w[r] = q.y[r] * 1.44269502162933349609375f; SUB_PIN(q.w[r]); break;
            case 5: q.y[r] = fmaf(q.y[r], 1.44269502162933349609375f, -q.w[r]); SUB_PIN(q.y[r]); break;
            case 6: q.w[r] = __builtin_amdgcn_exp2f(q.w[r]); SUB_PIN(q.w[r]); break;
            case 7: q.y[r] = q.y[r] * 0.693147180559945f; SUB_PIN(q.y[r]); break;
            case 8: q.w[r] = fmaf(q.w[r], q.y[r], q.w[r]); SUB_PIN(q.w[r]); break;
            case 9: q.w[r] = 1.0f + q.w[r]; SUB_PIN(q.w[r]); break;
            case 10: q.w[r] = __builtin_amdgcn_rcpf(q.w[r]); SUB_PIN(q.w[r]); break;
            case 11: q.x[r] = q.x[r] * SA; SUB_PIN(q.x[r]); break;
            default: q.x[r] = q.x[r] * q.w[r]; SUB_PIN(q.x[r]); break;
        }
    }
    static __device__ __forceinline__ void swish_pack(const SwishState& q, Hidden& n) {
#pragma unroll
        for (int s = 0; s < 2; ++s) { n[0][s] = as_f16x8(make_uint4(q.hh[4 * s], q.hh[4 * s + 1], q.hh[4 * s + 2], q.hh[4 * s + 3])); n[1][s] = as_f16x8(make_uint4(q.ll[4 * s], q.ll[4 * s + 1], q.ll[4 * s + 2], q.ll[4 * s + 3])); }
    }
    static __device__ __forceinline__ const f16x8& hid(const Hidden& hb, int kind, int s2) { return hb[kind == 1][s2]; }
    static __device__ __forceinline__ float out(float acc, float bias) { return fmaf(acc, UNS2, bias); }
};

}  // namespace

#define SUB_CHUNKED_FMT F16Fmt
#define SUB_CHUNKED_KERNEL sxf_sublin_kernel
#include "sub_chunked.h"

int launch_sxf_sublin(const SubChunkParams& p, hipStream_t s) {
    return launch_sub_chunked(p, s);
}
