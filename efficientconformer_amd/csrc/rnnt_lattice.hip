// RNN-T lattice (gfx950): for encoder outputs f (T frames) and a transcript y (U tokens, blank = 0) the two numbers per lattice cell
// (t, u), t < T, u <= U, that the RNN-T loss and a forced alignment need,
//   lp_blank[t][u] = log_softmax(logits(t, u) / tmp)[0]          (stay in column u, go to frame t + 1)
//   lp_label[t][u] = log_softmax(logits(t, u) / tmp)[y[u]]       (emit token u at frame t, go to column u + 1; -inf at u = U)
//   logits(t, u)   = W_j tanh(linear_encoder(f[t]) + linear_decoder(g_u)) + b_j,   g_u = the prediction network's output after [0, y_1 .. y_u]
// (reference transducer.py:88-107 + the log_softmax of the loss) without the (B, T, U + 1, V) tensor: the logits of a cell live in MFMA
// accumulators and leave them as a running (max, sum) and two picked columns.
//
// Four launches on the caller's stream.
//   * rnnt_lattice_prep_kernel (one workgroup): status per utterance (2: y_len outside 0 .. u_max or a token outside 1 .. V - 1; 1: tokens
//     but no frames), the clamped lengths, and the exclusive prefix sum of the cell counts T_b (U_b + 1) - the joint kernel walks the
//     cells of the batch as ONE dense list, so ragged batches cost what their cells cost and nothing for the padding.
//   * rnnt_prednet_kernel: the teacher-forced prediction network.  One workgroup per 16 utterances = the 16 columns of the fp32 MFMA tiles
//     of lstm_step16 (decode_common.h, the beam search's LSTM step as well: gates = Gin[y] + W_hh h, torch gate order i, f, g, o, sigmoid_precise / tanhf, k
//     ascending); the workgroup loops over u = 0 .. u_max and writes h_u.  A column's arithmetic does not depend on the other 15.
//   * linear_decoder over all B (u_max + 1) rows and linear_encoder over all B T rows: launch_sgemm_nt, as the beam search does.
//   * rnnt_joint_kernel: a tiled GEMM with M = cells, K = J, N = V.  A workgroup (8 waves) owns 32 consecutive cells of the dense list: it
//     builds z = tanh(fe + gd) ONCE into LDS (k-permuted, the B operand of the MFMAs: 32 x J fp32 = 80 KiB at J = 640, so the N
//     dimension is what is chunked), then every wave walks pairs of 16-row tiles of W_j against the two 16-cell column groups
//     (v_mfma_f32_16x16x4_f32, exact fp32 operands, k ascending: one weight float4 and one z float4 per lane feed eight MFMAs).  Epilogue
//     per tile pair: (acc + b_j) / tmp, the lane's running (max, sum) and the two picked columns; at the end the lanes of a cell are
//     merged in a fixed order (k-slots 0..3 of the wave, then waves 0..7), lse = max + log(sum).
// Operands: fp32 on the fp32 matrix pipe.  bf16 hi / lo operand planes (three bf16 MFMAs per product) keep 16 mantissa bits per operand:
// the logits would carry a relative error of ~2^-16 per product against the 8 x float32-noise bound the planes are held to.
// Every value of a cell is computed by the same instructions in the same order wherever the cell sits in the dense list: a plane entry
// depends on its own utterance only.  Cells outside an utterance's rectangle are 0 in both planes (a memset before the joint kernel).
#include "decode_common.h"

#include <cmath>

int ec_fail(const char* msg);

using namespace ecrnnt;
using namespace ecdec;

namespace {

constexpr int PT = 512;          // threads of the prediction-network and joint workgroups
constexpr int PNW = PT / 64;     // waves
constexpr int MAXC = 16;         // utterances per prediction-network workgroup = columns of an MFMA tile
constexpr int CT = 32;           // cells per joint workgroup: two column groups
constexpr int ZPAD = 4;          // floats between z rows: the 16 lanes of a k-slot read 16 different bank quads
constexpr int MAXU = 1023;

size_t joint_lds_bytes(const EcRnntConfig& c) { return (size_t)CT * (c.dim_joint + ZPAD) * 4; }
size_t pred_lds_bytes(const EcRnntConfig& c) { return (size_t)3 * MAXC * c.dim_decoder * 4; }

const char* lat_check(const EcRnnt* r, int32_t batch, int32_t t_out, int32_t u_max) {
    if (!r) return "null handle";
    if (!beam_dims_supported(r->cfg)) return "rnnt lattice: decoder and joint widths must be multiples of 16";
    if (joint_lds_bytes(r->cfg) > 150 * 1024 || pred_lds_bytes(r->cfg) > 150 * 1024) return "rnnt lattice: decoder / joint widths exceed the LDS of one workgroup";
    if (u_max < 0 || u_max > MAXU) return "rnnt lattice: u_max must be in 0 .. 1023";
    if (batch < 0 || t_out < 0) return "rnnt lattice: bad shape";
    if ((int64_t)batch * t_out * (u_max + 1) >= (1ll << 31)) return "rnnt lattice: batch * t_out * (u_max + 1) must be below 2^31";
    return nullptr;
}

struct LatArgs {
    RnntDev w;
    const int64_t* out_len; const int64_t* target_len; const int* targets;
    int B, T, umax; float tmp;
    int* tlen; int* ulen; int* start; int* status;
    float* h; const float* gd; const float* fe;
    float* lpb; float* lpl;
};

// ---------------------------------------------------------------------------------------------------------------- lengths, status, cell list
__global__ __launch_bounds__(PT) void rnnt_lattice_prep_kernel(const LatArgs a) {
    __shared__ int s_part[PT];
    const int tid = threadIdx.x, B = a.B;
    const int per = (B + PT - 1) / PT;               // consecutive utterances per thread
    int sum = 0;
    for (int i = 0; i < per; ++i) {
        const int b = tid * per + i;
        if (b >= B) break;
        int Tb = clamp_len(a.out_len[b], a.T);
        int st = transcript_status(a.target_len[b], a.umax, a.targets + (size_t)b * a.umax, a.w.V);
        int U = st ? 0 : (int)a.target_len[b];
        if (st == 2) Tb = 0;                         // no cells: the planes' rows stay 0
        else if (Tb == 0 && U > 0) st = 1;
        a.status[b] = st; a.tlen[b] = Tb; a.ulen[b] = U;
        sum += Tb * (U + 1);
    }
    s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < PT; ++i) { const int v = s_part[i]; s_part[i] = run; run += v; }
        a.start[B] = run;
    }
    __syncthreads();
    int run = s_part[tid];
    for (int i = 0; i < per; ++i) {
        const int b = tid * per + i;
        if (b >= B) break;
        a.start[b] = run;
        run += a.tlen[b] * (a.ulen[b] + 1);
    }
}

// ---------------------------------------------------------------------------------------------------------------- prediction network
// lstm_step16's view of one utterance column: c in LDS (natural order), h into the other half of the LDS double buffer (k-permuted) and, for an utterance of the
// batch, into the workspace row of this step.  (column, unit) belongs to one lane alone.
struct PredColumn {
    const float* gin; float* c; float* hn; float* out;
    static constexpr bool live = true;
    __device__ __forceinline__ float c_old(int unit) const { return c[unit]; }
    __device__ __forceinline__ void put(int unit, float h, float cv) const {
        c[unit] = cv;
        hn[kperm(unit)] = h;
        if (out) out[unit] = h;
    }
};

__global__ __launch_bounds__(PT) void rnnt_prednet_kernel(const LatArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const RnntDev& w = a.w;
    const int H = w.H;
    float* hx[2] = {lds, lds + MAXC * H};            // [16][H] h (k-permuted, see mfma_rows16), double buffered
    float* sc = lds + 2 * MAXC * H;                  // [16][H] c
    __shared__ int s_y[2][MAXC];                     // double buffered: a wave writes step u + 1's tokens while others still read step u's
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
    const int b0 = blockIdx.x * MAXC;
    for (int i = tid; i < MAXC * H; i += PT) { hx[0][i] = 0.f; sc[i] = 0.f; }
    const int bj = b0 + j;
    const bool live = bj < a.B;
    for (int u = 0; u <= a.umax; ++u) {
        if (tid < MAXC) {                            // the token the decoder runs on: 0 (start), then y[u - 1]; 0 past the transcript
            const int b = b0 + tid;
            int y = 0;
            if (b < a.B && u >= 1 && u <= a.ulen[b]) y = a.targets[(size_t)b * a.umax + u - 1];
            s_y[u & 1][tid] = y;
        }
        __syncthreads();                             // s_y, and the previous step's h
        const PredColumn col{w.gin + (size_t)s_y[u & 1][j] * 4 * H, sc + j * H, hx[(u + 1) & 1] + j * H,
                             live ? a.h + ((size_t)bj * (a.umax + 1) + u) * H : nullptr};
        for (int ub = wave; ub < H / 16; ub += PNW) lstm_step16(w, ub, hx[u & 1] + j * H + 4 * g, col);
    }
}

// ---------------------------------------------------------------------------------------------------------------- joint lattice
// vocab_lse_tiles' pick of the lane's two cells j and 16 + j: the blank entry and each cell's label entry
struct LatticePick {
    float* blank; float* label; int y0, y1;          // this lane's slots of s_blank / s_label (the second cell's are 16 further)
    __device__ __forceinline__ void operator()(int n, float v0, float v1) const {
        if (n == 0) { blank[0] = v0; blank[16] = v1; }
        if (n == y0) label[0] = v0;
        if (n == y1) label[16] = v1;
    }
};

__global__ __launch_bounds__(PT) void rnnt_joint_kernel(const LatArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sz[];     // [CT][J + ZPAD] z, k-permuted
    __shared__ int s_b[CT], s_t[CT], s_u[CT], s_y[CT];
    __shared__ float s_m[PNW][CT], s_s[PNW][CT], s_blank[CT], s_label[CT];
    const RnntDev& w = a.w;
    const int J = w.J, V = w.V, P = J + ZPAD, K16 = J / 16, E = a.umax + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
    const int total = a.start[a.B];
    const int c0 = blockIdx.x * CT;
    if (c0 >= total) return;                         // the whole workgroup
    if (tid < CT) {
        const int c = c0 + tid;
        int b = -1, t = 0, u = 0, y = -1;
        if (c < total) {
            b = ragged_find(a.start, a.B, c);        // the last b with start[b] <= c (utterances without cells share a start)
            const int r = c - a.start[b], eu = a.ulen[b] + 1;
            t = r / eu; u = r - t * eu;
            y = u < a.ulen[b] ? a.targets[(size_t)b * a.umax + u] : -1;
        }
        s_b[tid] = b; s_t[tid] = t; s_u[tid] = u; s_y[tid] = y;
        s_blank[tid] = 0.f; s_label[tid] = -INFINITY;
    }
    __syncthreads();
    // ---- z = tanh(linear_encoder(f[t]) + linear_decoder(g_u)), once per cell; cells beyond the list: zeros
    for (int i = tid; i < CT * (J / 4); i += PT) {
        const int c = i / (J / 4), k = 4 * (i - c * (J / 4));
        float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        const int b = s_b[c];
        if (b >= 0) {
            const float4 fe = *reinterpret_cast<const float4*>(a.fe + ((size_t)b * a.T + s_t[c]) * J + k);
            const float4 gd = *reinterpret_cast<const float4*>(a.gd + ((size_t)b * E + s_u[c]) * J + k);
            z = make_float4(tanhf(fe.x + gd.x), tanhf(fe.y + gd.y), tanhf(fe.z + gd.z), tanhf(fe.w + gd.w));
        }
        float* zr = sz + c * P;
        zr[kperm(k)] = z.x; zr[kperm(k + 1)] = z.y; zr[kperm(k + 2)] = z.z; zr[kperm(k + 3)] = z.w;
    }
    __syncthreads();
    // ---- logits tile by tile: wave `wave` owns the tile pairs wave, wave + 8, ..; acc[i][c] = tile i of the pair x column group c
    float ms[4];                                     // the lane's running (max, sum) of cells j and 16 + j
    vocab_lse_tiles<2, PNW>(w.wj16, w.bj, V, K16, sz + j * P + 4 * g, sz + (16 + j) * P + 4 * g, a.tmp, LatticePick{s_blank + j, s_label + j, s_y[j], s_y[16 + j]}, ms);
    const float lse = vocab_lse_merge<PNW>(ms, s_m, s_s);
    if (tid < CT && s_b[tid] >= 0) {
        const size_t o = ((size_t)s_b[tid] * a.T + s_t[tid]) * E + s_u[tid];
        a.lpb[o] = s_blank[tid] - lse;
        a.lpl[o] = s_y[tid] >= 0 ? s_label[tid] - lse : -INFINITY;
    }
}

}  // namespace

extern "C" {

size_t effconf_rnnt_lattice_workspace_bytes(const EcRnnt* r, int32_t batch, int32_t t_out, int32_t u_max) {
    if (const char* e = lat_check(r, batch, t_out, u_max)) { ec_fail(e); return 0; }
    return lat_layout(r->cfg, batch, t_out, u_max).total;
}

int effconf_rnnt_lattice(EcRnnt* r, const float* enc_out, const int64_t* out_len, int32_t batch, int32_t t_out, const int32_t* targets,
                         const int64_t* target_len, int32_t u_max, float temperature, float* lp_blank, float* lp_label, int32_t* status,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!r || !r->finalized) return ec_fail("rnnt handle not finalized");
    if (const char* e = lat_check(r, batch, t_out, u_max)) return ec_fail(e);
    if (!(temperature > 0.f) || !std::isfinite(temperature)) return ec_fail("rnnt lattice: temperature must be > 0");
    if (batch == 0) return 0;
    if (!out_len || !target_len || !status || !workspace || (t_out > 0 && (!enc_out || !lp_blank || !lp_label)) || (u_max > 0 && !targets))
        return ec_fail("null argument");
    if (!r->dev.whh16 || !r->dev.wj16 || !r->wd) return ec_fail("rnnt lattice: MFMA weight images missing (finalize)");
    const LatLayout L = lat_layout(r->cfg, batch, t_out, u_max);
    if (workspace_bytes < L.total) return ec_fail("workspace too small (effconf_rnnt_lattice_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    const int H = r->cfg.dim_decoder, J = r->cfg.dim_joint, De = r->cfg.dim_encoder, E = u_max + 1;
    char* ws = WsPlan::base(workspace);
    LatArgs a{};
    a.w = r->dev; a.out_len = out_len; a.target_len = target_len; a.targets = targets;
    a.B = batch; a.T = t_out; a.umax = u_max; a.tmp = temperature;
    a.tlen = reinterpret_cast<int*>(ws + L.tlen); a.ulen = reinterpret_cast<int*>(ws + L.ulen); a.start = reinterpret_cast<int*>(ws + L.start);
    a.status = status;
    a.h = reinterpret_cast<float*>(ws + L.h);
    float* gd = reinterpret_cast<float*>(ws + L.gd);
    float* fe = reinterpret_cast<float*>(ws + L.fe);
    a.gd = gd; a.fe = fe; a.lpb = lp_blank; a.lpl = lp_label;
    hipLaunchKernelGGL(rnnt_lattice_prep_kernel, dim3(1), dim3(PT), 0, s, a);
    if (hipGetLastError() != hipSuccess) return ec_fail("rnnt_lattice_prep launch failed");
    const size_t cells = (size_t)batch * t_out * E;
    if (cells == 0) return 0;
    if (hipMemsetAsync(lp_blank, 0, cells * 4, s) != hipSuccess || hipMemsetAsync(lp_label, 0, cells * 4, s) != hipSuccess)
        return ec_fail("rnnt lattice: clearing the planes failed");
    static LdsAttr pattr, jattr;
    const size_t plds = pred_lds_bytes(r->cfg), jlds = joint_lds_bytes(r->cfg);
    ensure_dynamic_lds(reinterpret_cast<const void*>(&rnnt_prednet_kernel), (int)plds, pattr);
    hipLaunchKernelGGL(rnnt_prednet_kernel, dim3((batch + MAXC - 1) / MAXC), dim3(PT), plds, s, a);
    if (hipGetLastError() != hipSuccess) return ec_fail("rnnt_prednet launch failed");
    if (launch_sgemm_nt(a.h, H, r->wd, H, r->dev.bd, gd, J, batch * E, J, H, s) != 0)
        return ec_fail("linear_decoder GEMM launch failed");
    if (launch_sgemm_nt(enc_out, De, r->we, De, r->be, fe, J, batch * t_out, J, De, s) != 0) return ec_fail("linear_encoder GEMM launch failed");
    ensure_dynamic_lds(reinterpret_cast<const void*>(&rnnt_joint_kernel), (int)jlds, jattr);
    hipLaunchKernelGGL(rnnt_joint_kernel, dim3((unsigned)((cells + CT - 1) / CT)), dim3(PT), jlds, s, a);
    return hipGetLastError() == hipSuccess ? 0 : ec_fail("rnnt_joint launch failed");
}

}  // extern "C"
