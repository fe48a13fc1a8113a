// The chunked front end, said once: Conv2dSubsampling (one layer, C_in = 1: Conv2d 3x3 s2 p1 -> BatchNorm2d(eval) -> Swish; reference modules.py:232-249) + transpose /
// flatten + nn.Linear (encoders.py:113-116) as ONE kernel whose (frames, C F') activation never leaves the registers.  sublinear3.hip (bf16) and sxf_sub.hip (split
// precision) compile this body with their number format; what a format is made of, and how a source uses this file, stands at the end of this comment.
//   * a wave keeps 32 frames, TRANSPOSED (frames = MFMA columns = lanes), and walks chunks of 32 channels at one output frequency f' (k index c F' + f' of the Linear);
//   * first product  H^T = Wc_cb P_f'^T : the 3 x 3 convolution as ONE 16-wide MFMA k-step - A operand = 9 folded taps of 32 channels + the folded bias / BN shift in
//     tap 9 against a constant 1, B operand = this lane's patch mel[2 f' - 1 .. 2 f' + 1][2 t - 1 .. 2 t + 1] (zero outside the utterance's own image: what it sees when
//     run alone) - with both operands split in two halves: three MFMAs (h h, h l, l h) on one accumulator; the patch rows are carried from f' to f' + 1 (row 2 f' + 1
//     is the next patch's first) and the next two rows are requested one f' ahead;
//   * Swish on the accumulator registers, which ARE the B fragments of the second product  Y^T += Wl_chunk H^T  (k order of the Linear's image permuted to the
//     accumulator layout at pack time, pack.hip); the Linear image streams through a two-stage register-staged LDS ring (one LDS-only barrier per chunk), so two or
//     three workgroups share a CU and one's Swish runs under another's MFMAs; inside a wave the second product of chunk c carries the Swish of chunk c + 1 between
//     its MFMAs, the order fixed in the source;
//   * ragged batches: workgroup = (utterance, 128 frames); rows off[b] + t, the group-padding rows behind an utterance's last frame are written as zeros.
// A format (static members only): frag + mfma (the 32x32x16 operand type and its builtin); PLANES weight planes per chunk in the ring and KINDS MFMAs per (tile,
// k-step) of the second product (kind 2 takes plane 1); split_patch (8 patch values -> operand halves); SwishState / SWISH_STEPS / swish_step / swish_pack (the
// Swish as single-instruction steps and its result: Hidden = the B fragments [plane][k-step]); hid (the fragment kind `kind` multiplies); out (accumulator + bias ->
// y); OCC2_MAX (most output tiles at which two workgroups share a CU: the kernel's __launch_bounds__).
// Use: a source defines its format, then SUB_CHUNKED_FMT (its name) and SUB_CHUNKED_KERNEL (the name of its __global__ template <int NT2>), and includes this
// file, once: the body below IS that kernel.  As `sub_chunked_body<Fmt, NT2>(p)` called from two one-line kernels - the same statements inside a function inlined
// into the kernel - every instance was compiled to a shorter but slower stream (0.6 - 1.5 % per launch at 4 and 6 tiles, profiles/sub_chunked_parity.txt); so were
// the Swish-ed fragments as a struct of arrays instead of a plain array.  In this form the four bf16 instances are the instruction streams they were as a kernel
// of their own.
#ifndef SUB_CHUNKED_FMT
#error "define SUB_CHUNKED_FMT and SUB_CHUNKED_KERNEL before including sub_chunked.h"
#endif
#include "kernels.h"

namespace {

constexpr int SUB_ROW2 = 80;                                     // bytes per Linear image row in LDS: 32 hidden units (64 B) + 16

template <class Fmt, int NT2>
struct SubChunkLds {
    static constexpr int DP2 = 32 * NT2, STAGE = Fmt::PLANES * DP2 * SUB_ROW2;
    static constexpr int PIECES = 4 * Fmt::PLANES * DP2;         // 16-byte pieces of a chunk (all planes)
    static constexpr int NPC = (PIECES + 255) / 256;
    static constexpr int CW = 2 * 32 * 32;                       // bytes of one channel block's conv taps: hi [32][16] | lo [32][16]
};

template <int NT2>
__global__ __launch_bounds__(256, (NT2 <= SUB_CHUNKED_FMT::OCC2_MAX ? 2 : 1)) void SUB_CHUNKED_KERNEL(const SubChunkParams p) {
    using Fmt = SUB_CHUNKED_FMT;
    using L = SubChunkLds<Fmt, NT2>;
    using frag = typename Fmt::frag;
    using Hidden = typename Fmt::Hidden;
    using SwishState = typename Fmt::SwishState;
    constexpr int DP2 = L::DP2, NPC = L::NPC, ROW2 = SUB_ROW2, PLANES = Fmt::PLANES, KINDS = Fmt::KINDS, SWISH_STEPS = Fmt::SWISH_STEPS;
    extern __shared__ __attribute__((aligned(16))) char sm[];
    char* const sCW = sm + 2 * L::STAGE;                         // conv taps of all channel blocks (resident)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, kh = lane >> 5;
    const int b = blockIdx.y, t0 = blockIdx.x * 128;
    const int nrows = p.off ? p.off[b + 1] - p.off[b] : p.To;    // rows this utterance owns in the output (ragged: group padded)
    const int nvalid = p.len ? p.len[b] : p.To;                  // frames that exist
    if (t0 >= nrows) return;                                     // the grid is sized for the longest utterance (whole workgroup leaves)
    const long long row0 = p.off ? (long long)p.off[b] : (long long)b * p.To;
    const int Tv = p.mel_len ? p.mel_len[b] : p.Tm;              // the utterance's own mel frames: the convolution's zero padding starts behind them
    const int t = t0 + 32 * wave + lr;
    const int tc = t < nvalid ? t : nvalid - 1;
    typedef uint32_t u4v __attribute__((ext_vector_type(4)));
    // ---- the Linear ring: this thread's pieces of a chunk (global: contiguous; LDS: padded rows)
    uint32_t loff[NPC];
#pragma unroll
    for (int it = 0; it < NPC; ++it) {
        if constexpr (PLANES == 1) {
            const int q = tid + 256 * it, n = q >> 2, ch = q & 3;
            loff[it] = (uint32_t)(n * ROW2 + ch * 16);
        } else {
            const int q = tid + 256 * it, pl = q / (4 * DP2), rem = q - pl * 4 * DP2, n = rem >> 2, ch = rem & 3;
            loff[it] = (uint32_t)(pl * DP2 * ROW2 + n * ROW2 + ch * 16);
        }
    }
    const int nchunk = p.Fo * p.ncb;
    const char* wsrc = reinterpret_cast<const char*>(p.wimg) + (size_t)tid * 16;
    constexpr size_t CB = (size_t)L::PIECES * 16;
    u4v wreg[NPC];
    auto fetch = [&](int c) __attribute__((always_inline)) {
        c = c < nchunk ? c : nchunk - 1;                         // past the end: the last chunk again (never published)
#pragma unroll
        for (int it = 0; it < NPC; ++it)
            if (L::PIECES % 256 == 0 || tid + 256 * it < L::PIECES) wreg[it] = *reinterpret_cast<const u4v*>(wsrc + (size_t)c * CB + (size_t)it * 4096);
    };
    auto publish = [&](char* st) __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < NPC; ++it)
            if (L::PIECES % 256 == 0 || tid + 256 * it < L::PIECES) *reinterpret_cast<u4v*>(st + loff[it]) = wreg[it];
    };
    fetch(0);
    // ---- conv taps -> LDS (ncb blocks x 2 KB, contiguous copy)
    for (int q = tid; q < p.ncb * (L::CW / 16); q += 256)
        *reinterpret_cast<u4v*>(sCW + q * 16) = *reinterpret_cast<const u4v*>(reinterpret_cast<const char*>(p.cimg) + (size_t)q * 16);
    // ---- patch rows: mel[f][2 tc - 1 + j], j = 0 .. 2, zero outside [0, F) x [0, Tv): unconditional loads at clamped addresses, masked by select
    const float* mb = p.mel + (size_t)b * p.F * p.Tm;
    int tau[3]; bool tok[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { const int x = 2 * tc - 1 + j; tok[j] = x >= 0 && x < Tv; tau[j] = tok[j] ? x : 0; }
    auto load_row = [&](int f, float (&dst)[3]) __attribute__((always_inline)) {
        const bool fok = f >= 0 && f < p.F;
        const float* r = mb + (size_t)(fok ? f : 0) * p.Tm;
#pragma unroll
        for (int j = 0; j < 3; ++j) { const float v = r[tau[j]]; dst[j] = fok && tok[j] ? v : 0.f; }
    };
    float pr[3][3], nx[2][3];
    load_row(-1, pr[0]); load_row(0, pr[1]); load_row(1, pr[2]);
    f32x16 oacc[NT2];
#pragma unroll
    for (int tt = 0; tt < NT2; ++tt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[tt][r] = 0.f;
    auto patch_frags = [&](frag& ah, frag& al) __attribute__((always_inline)) {
        // this lane's patch as split B fragments: taps 3 i + j; lane half 0 holds taps 0 .. 7, half 1 tap 8, the constant of the bias column (tap 9) and zeros
        float v[8];
        v[0] = kh ? pr[2][2] : pr[0][0]; v[1] = kh ? 1.0f : pr[0][1]; v[2] = kh ? 0.f : pr[0][2];
        v[3] = kh ? 0.f : pr[1][0]; v[4] = kh ? 0.f : pr[1][1]; v[5] = kh ? 0.f : pr[1][2];
        v[6] = kh ? 0.f : pr[2][0]; v[7] = kh ? 0.f : pr[2][1];
        Fmt::split_patch(v, ah, al);
    };
    // H^T = Wc_cb P^T (32 channels x 32 frames): one 16-wide k-step, the three operand-half products on ONE accumulator (three accumulators - no wait between the
    // MFMAs - cost 48 v_accvgpr_write zeros, 48 v_accvgpr_read and 32 adds per chunk: 40 % of the bf16 loop's VALU instructions, profiles/r6_94_*)
    auto first_product = [&](int cb, const frag& ah, const frag& al, f32x16& h) __attribute__((always_inline)) {
        const char* cw = sCW + cb * L::CW + lr * 32 + 16 * kh;
        const frag wh = *reinterpret_cast<const frag*>(cw), wl = *reinterpret_cast<const frag*>(cw + 32 * 32);
        f32x16 z0;
#pragma unroll
        for (int r = 0; r < 16; ++r) z0[r] = 0.f;
        h = Fmt::mfma(wh, ah, z0);
        h = Fmt::mfma(wh, al, h);
        h = Fmt::mfma(wl, ah, h);
    };
    constexpr int GS = NT2 < 4 ? NT2 : 4, NG = (NT2 + GS - 1) / GS, NU = 2 * NG, NM = 2 * KINDS * NT2, Q = (SWISH_STEPS + NM - 1) / NM, LASTG = NT2 - (NG - 1) * GS;
    static_assert(NM * Q >= SWISH_STEPS, "every Swish step has its MFMA");
    // one pipeline step: Y^T += Wl_c H_c^T (stage c & 1; units = (group of up to four output tiles, k-step), MFMAs kind-major over the tiles: consecutive instructions
    // hit different accumulators) with the Swish of chunk c + 1 = (., cb1) BETWEEN its MFMAs, the order fixed in the source (a fence per MFMA, its quota of Swish steps
    // behind it: independent work that, left in sequence, kept the matrix pipe idle under the VALU and the VALU idle under the MFMA queue); fragment reads run one
    // unit ahead
    auto step = [&](int c, int cb1, const frag& ah, const frag& al, Hidden& hb) __attribute__((always_inline)) {
        if (c + 1 < nchunk) publish(sm + ((c + 1) & 1) * L::STAGE);      // stage (c + 1) & 1 was read in iteration c - 1: every wave is past the barrier that closed it
        fetch(c + 2);
        __builtin_amdgcn_sched_barrier(0);
        f32x16 h;
        first_product(cb1, ah, al, h);
        const char* w2 = sm + (c & 1) * L::STAGE + lr * ROW2 + 16 * kh;
        frag vw[PLANES][NU][GS];
        auto load_unit = [&](int u) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < GS; ++i) {
                const int tt = (u >> 1) * GS + i, s2 = u & 1;
                if (tt < NT2) {
#pragma unroll
                    for (int pl = 0; pl < PLANES; ++pl) vw[pl][u][i] = *reinterpret_cast<const frag*>(w2 + pl * DP2 * ROW2 + 32 * tt * ROW2 + 32 * s2);
                }
            }
        };
        SwishState q;
        __builtin_amdgcn_sched_barrier(0);
        load_unit(0);
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int s2 = u & 1, gq = u >> 1, gsz = gq == NG - 1 ? LASTG : GS;
            const int base = KINDS * (2 * GS * gq + s2 * gsz);           // MFMAs before this unit (a function of the loop indices only: every Swish step index below is a constant)
#pragma unroll
            for (int kind = 0; kind < KINDS; ++kind)
#pragma unroll
                for (int i = 0; i < GS; ++i) {
                    const int tt = gq * GS + i;
                    if (tt < NT2) {
                        __builtin_amdgcn_sched_barrier(0);
                        if (kind == 0 && i == 0 && u + 1 < NU) load_unit(u + 1);
                        oacc[tt] = Fmt::mfma(vw[kind == 2 ? 1 : 0][u][i], Fmt::hid(hb, kind, s2), oacc[tt]);
                        const int m0 = (base + kind * gsz + i) * Q;
#pragma unroll
                        for (int j = 0; j < Q; ++j) if (m0 + j < SWISH_STEPS) Fmt::swish_step(m0 + j, h, q);
                    }
                }
        }
        __builtin_amdgcn_sched_barrier(0);
        Fmt::swish_pack(q, hb);
        lds_barrier();
    };
    publish(sm);
    fetch(1);
    lds_barrier();
    frag ah, al;
    Hidden hb;
    {   // chunk 0: first product + Swish alone
        load_row(2, nx[0]); load_row(3, nx[1]);
        patch_frags(ah, al);
        f32x16 h;
        first_product(0, ah, al, h);
        SwishState q;
#pragma unroll
        for (int j = 0; j < SWISH_STEPS; ++j) Fmt::swish_step(j, h, q);
        Fmt::swish_pack(q, hb);
    }
    int c = 0;
    for (int fo = 0; fo < p.Fo; ++fo) {
        for (int cb = 0; cb + 1 < p.ncb; ++cb, ++c) step(c, cb + 1, ah, al, hb);
        // the last channel block of this f': its partner is the first chunk of f' + 1 - advance the patch (rows requested one f' ahead), request the one after
#pragma unroll
        for (int j = 0; j < 3; ++j) { pr[0][j] = pr[2][j]; pr[1][j] = nx[0][j]; pr[2][j] = nx[1][j]; }
        load_row(2 * fo + 4, nx[0]); load_row(2 * fo + 5, nx[1]);       // behind the image: zeros, never used
        patch_frags(ah, al);
        step(c, 0, ah, al, hb);                                          // behind the last chunk: a product nobody consumes
        ++c;
    }
    // ---- y = Y + bias for the frames that exist, zeros for the group-padding rows; feature of register (tt, r) = 32 tt + 8 (r >> 2) + 4 kh + (r & 3)
    if (t < nrows) {
        float* yr = p.y + (size_t)(row0 + t) * p.ldy;
        const bool live = t < nvalid;
#pragma unroll
        for (int tt = 0; tt < NT2; ++tt)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const int f = 32 * tt + 8 * rq + 4 * kh;
                if (f >= p.N) continue;                          // N % 4 == 0: a quad is inside or outside as a whole
                const float4 bz = *reinterpret_cast<const float4*>(p.bias + f);
                float4 o;
                o.x = live ? Fmt::out(oacc[tt][4 * rq + 0], bz.x) : 0.f; o.y = live ? Fmt::out(oacc[tt][4 * rq + 1], bz.y) : 0.f;
                o.z = live ? Fmt::out(oacc[tt][4 * rq + 2], bz.z) : 0.f; o.w = live ? Fmt::out(oacc[tt][4 * rq + 3], bz.w) : 0.f;
                *reinterpret_cast<float4*>(yr + f) = o;
            }
    }
}

// One instance: the LDS bound (two ring stages + the resident conv taps <= 160 KB, else -2) and the launch
template <int NT2>
int launch_sub_chunked_tiles(const SubChunkParams& p, hipStream_t s) {
    using L = SubChunkLds<SUB_CHUNKED_FMT, NT2>;
    const int lds = 2 * L::STAGE + p.ncb * L::CW;
    if (lds > 160 * 1024) return -2;
    static LdsAttr attr;
    ensure_dynamic_lds(reinterpret_cast<const void*>(&SUB_CHUNKED_KERNEL<NT2>), lds, attr);
    hipLaunchKernelGGL((SUB_CHUNKED_KERNEL<NT2>), dim3((p.rows_max + 127) / 128, p.B), dim3(256), lds, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The instance sub_chunked_tiles(N) names; an empty batch is no launch, a shape no instance serves is refused (-2)
int launch_sub_chunked(const SubChunkParams& p, hipStream_t s) {
    if (p.B <= 0 || p.rows_max <= 0) return 0;
    if (!p.mel || !p.cimg || !p.wimg || !p.bias || !p.y || p.N % 4 || p.ldy % 4 || p.ncb <= 0 || p.Fo <= 0 || p.B > 65535) return -2;
    switch (sub_chunked_tiles(p.N)) {
        case 1: return launch_sub_chunked_tiles<1>(p, s);
        case 4: return launch_sub_chunked_tiles<4>(p, s);
        case 6: return launch_sub_chunked_tiles<6>(p, s);
        case 12: return launch_sub_chunked_tiles<12>(p, s);
    }
    return -2;
}

}  // namespace
