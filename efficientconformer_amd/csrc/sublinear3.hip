// Fused Conv2dSubsampling + Linear, third form (round 6): chunked over (output frequency, 32 channels) so that ANY channel count and model width fits.
//
// Reference: Conv2dSubsampling.forward (models/modules.py:232-249, one layer, C_in = 1: Conv2d 3x3 s2 p1 -> BatchNorm2d(eval) -> Swish -> reshape to
// (B, C*F/2, T1)) + transpose + nn.Linear(C*F/2 -> D0) of ConformerEncoder.forward (encoders.py:113-116).
//
// sublinear2.hip keeps one output frequency's whole weight slab (D0 rows x C columns) in LDS: 74 KB per slab at C = D0 = 180 (two slabs, one 4-wave workgroup
// per CU: 1.1 ms per Medium step, 3.5 x its Swish's VALU floor) and no instance at C = D0 = 360, where the front end runs as a convolution kernel + a K = 14400
// GEMM with the (frames, 14400) bf16 activation written to HBM and read back (8.4 GB per Large step).  Here - the bf16 sibling of sxf_sub.hip - a wave keeps 32
// frames (lanes = frames) and walks chunks of 32 channels at one output frequency f':
//   * first product  H^T = Wc_cb P_f'^T : the 3 x 3 convolution as ONE 16-wide MFMA k-step (A operand = 9 folded taps of 32 channels + the folded bias in tap 9
//     against a constant 1; B operand = this lane's own mel patch), fp32-accurate on bf16 MFMAs by splitting both operands (hi hi + hi lo + lo hi, as sublinear2.hip);
//   * Swish on the accumulator registers, rounded to bf16: they ARE the B fragments of the second product  Y^T += Wl_chunk H^T  (k order of the Linear's image
//     permuted to the accumulator layout at pack time); the 32 x D0 x 32 weight chunk (12 - 24 KB) streams through a two-stage LDS ring, so two or three workgroups
//     share a CU and one's Swish runs under another's MFMAs; inside a wave the second product of chunk c carries the Swish of chunk c + 1 between its MFMAs;
//   * ragged batches: workgroup = (utterance, 128 frames); the rows behind an utterance's last frame (group padding) are written as zeros.
#include "kernels.h"

namespace {

__device__ __forceinline__ uint32_t hi_bits(float x) { return __float_as_uint(x) & 0xFFFF0000u; }     // bf16 by truncation: hi + lo = x to 16 + 8 bits

#define SUB3_PIN(v) asm volatile("" : "+v"(v))
// The bf16 format of sub_chunked.h: fp32-accurate first product on bf16 MFMAs by splitting both operands (hi hi + hi lo + lo hi, as sublinear2.hip), the Swish-ed
// hidden units rounded to bf16, one weight plane and one MFMA per (tile, k-step) of the second product
struct Bf16Fmt {
    typedef bf16x8 frag;
    static constexpr int PLANES = 1, KINDS = 1, OCC2_MAX = 6;
    typedef bf16x8 Hidden[1][2];                                // [plane][k-step]
    static __device__ __forceinline__ f32x16 mfma(const bf16x8& a, const bf16x8& b, const f32x16& c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ void split_patch(const float (&v)[8], bf16x8& ah, bf16x8& al) {
        uint32_t hh[4], ll[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t h0 = hi_bits(v[2 * e]), h1 = hi_bits(v[2 * e + 1]);
            hh[e] = (h0 >> 16) | h1;
            ll[e] = pack_bf2(v[2 * e] - __uint_as_float(h0), v[2 * e + 1] - __uint_as_float(h1));
        }
        ah = as_bf16x8(make_uint4(hh[0], hh[1], hh[2], hh[3])); al = as_bf16x8(make_uint4(ll[0], ll[1], ll[2], ll[3]));
    }
    // Swish of a finished first-product chunk -> bf16 B fragments of the second product, as single-instruction steps (x sigmoid(x) through v_exp_f32 / v_rcp_f32 as
    // common.h swishf_): four values at a time, stage-major inside the four; value r = register r of the accumulators <-> k position 8 kh + (r & 7) of k-step r >> 3.
    // Every step ends in an empty volatile asm on its result (sxf_chain.hip: pure arithmetic otherwise sinks behind the last MFMA whatever fences stand in the source).
    struct SwishState { float x[16], w[16]; uint32_t hh[8]; };
    static constexpr int SWISH_STEPS = 16 * 5 + 8;
    static __device__ __forceinline__ void swish_step(int idx, const f32x16& h, SwishState& q) {
        const int g = idx / 22, o = idx - 22 * g;
        if (o >= 20) { const int pr = 2 * g + (o - 20); q.hh[pr] = pack_bf2(q.x[2 * pr], q.x[2 * pr + 1]); SUB3_PIN(q.hh[pr]); return; }
        const int stage = o >> 2, r = 4 * g + (o & 3);
        switch (stage) {
            case 0: q.w[r] = h[r] * -1.44269504088896f; SUB3_PIN(q.w[r]); break;
            case 1: q.w[r] = __builtin_amdgcn_exp2f(q.w[r]); SUB3_PIN(q.w[r]); break;
            case 2: q.w[r] = 1.0f + q.w[r]; SUB3_PIN(q.w[r]); break;
            case 3: q.w[r] = __builtin_amdgcn_rcpf(q.w[r]); SUB3_PIN(q.w[r]); break;
            default: q.x[r] = h[r] * q.w[r]; SUB3_PIN(q.x[r]); break;
        }
    }
    static __device__ __forceinline__ void swish_pack(const SwishState& q, Hidden& nb) {
#pragma unroll
        for (int s = 0; s < 2; ++s) nb[0][s] = as_bf16x8(make_uint4(q.hh[4 * s], q.hh[4 * s + 1], q.hh[4 * s + 2], q.hh[4 * s + 3]));
    }
    static __device__ __forceinline__ const bf16x8& hid(const Hidden& hb, int, int s2) { return hb[0][s2]; }
    static __device__ __forceinline__ float out(float acc, float bias) { return acc + bias; }
};

}  // namespace

#define SUB_CHUNKED_FMT Bf16Fmt
#define SUB_CHUNKED_KERNEL sublinear3_kernel
#include "sub_chunked.h"

int launch_sublinear3(const SubChunkParams& p, hipStream_t s) {
    return launch_sub_chunked(p, s);
}
