// Weight packing: the layout vocabulary - one K order, the element encoders - of the image builders in pack.hip, which turn state-dict tensors into the images
// the kernels read.  Everything in namespace pack (here and there) is host arithmetic: host arrays and sizes in, std::vector out, no HIP call and no handle, so a
// layout can be checked on a machine without a GPU (effconf_debug_pack_digest, tools/pack_digest.py).  pack_encoder is the sequence of steps behind effconf_encoder_finalize.
#pragma once
#include "encoder_state.h"

#include <cmath>
#include <cstring>

// Largest |value x 2^10| the fused split images (sxf_sub / sxf_chain) hold as two fp16 halves (fp16 max 65504): |w| < 63.48 after
// folding.  An image with a value beyond it is not built - that block / the front end runs the per-module split kernels - and the per-module
// images (h = fp16(w)) refuse |w| >= kSplitImgMax itself (split-mode operand envelopes).  Nothing is clamped.
constexpr float kSplitImgMax = 65000.f;
// Largest per-channel L2 norm of the BatchNorm-folded depthwise taps the matrix-pipe kernel runs on two bf16 tap planes (hi + lo); above it a third; see pack_block
constexpr float kDwMfmaTwoPlaneNorm = 6.0f;

// The front end's geometry: "" or the reason it cannot run, naming the field (effconf_encoder_create, and again in front of the mel tables)
std::string mel_config_error(const EcConfig& c);
// effconf_encoder_finalize without its device epilogue: every packing step on the loaded host tensors; 0 or fail(...)
int pack_encoder(EcEncoder* e);

namespace pack {

using Img = std::vector<uint16_t>;

// THE K order of every image whose operand is a converted MFMA accumulator tile (chain*.hip, rsgemm.hip, sublinear2/3.hip, sxf_*.hip): inside a 16-block,
// position 8 kh + e holds feature 8 (e >> 2) + 4 kh + (e & 3) - accumulator register e of lane half kh.  An involution; bits above the 16-block pass through.
inline int acc16(int k) { return (k & ~15) + 8 * ((k >> 2) & 1) + 4 * ((k >> 3) & 1) + (k & 3); }

// ---- element encoders
inline uint16_t f16_bits(float f) { _Float16 h = (_Float16)f; uint16_t u; memcpy(&u, &h, 2); return u; }
inline float bf16_value(uint16_t b) { const uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; }
inline uint16_t bf16_rn(float f) {                                 // bf16, round to nearest even
    uint32_t u; memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
// A two-plane element: writes the halves of v, false = v is outside the format's range (nothing written).  double in: folded products arrive unrounded.
using PairEnc = bool (*)(double v, uint16_t* hi, uint16_t* lo);
inline bool bf16_pair_trunc(double v, uint16_t* hi, uint16_t* lo) {        // hi = the top 16 bits of fp32(v), lo = bf16(v - hi)
    const float f = (float)v; uint32_t u; memcpy(&u, &f, 4);
    *hi = (uint16_t)(u >> 16); *lo = bf16_rn(f - bf16_value(*hi));
    return true;
}
inline bool bf16_pair_round(double v, uint16_t* hi, uint16_t* lo) {        // hi = bf16(v), lo = bf16(v - hi)
    const float f = (float)v;
    *hi = bf16_rn(f); *lo = bf16_rn(f - bf16_value(*hi));
    return true;
}
inline bool bf16_single(double v, uint16_t* hi, uint16_t*) { *hi = bf16_rn((float)v); return true; }     // one plane (lo unused)
inline bool f16_pair_s10(double v, uint16_t* hi, uint16_t* lo) {           // same-scale halves at 2^10 (sx_common.h split2s): h = fp16(v 2^10), l = fp16(v 2^10 - h)
    const float ws = (float)(v * 1024.0);
    if (!(std::fabs(ws) < kSplitImgMax)) return false;
    const _Float16 h = (_Float16)ws;
    *hi = f16_bits((float)h); *lo = f16_bits(ws - (float)h);
    return true;
}
inline bool f16_pair_2048(float w, uint16_t* hi, uint16_t* lo) {           // per-module split images: h = fp16(w), l = fp16((w - h) * 2048); |w - h| <= 2^-11 |w|: |l| < 2^15
    if (!(std::fabs(w) < kSplitImgMax)) return false;
    const _Float16 h = (_Float16)w;
    *hi = f16_bits((float)h); *lo = f16_bits((w - (float)h) * 2048.0f);
    return true;
}

}  // namespace pack
