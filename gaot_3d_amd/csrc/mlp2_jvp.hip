// Forward-mode tangents of the per-node two-layer MLP in ONE pass, exact fp32:
//     y[n][c]    = sum_j W2[c][j] gelu(z[n][j]) + b2[c],                 z = W1 x + b1
//     dy_d[n][c] = sum_j W2[c][j] gelu'(z[n][j]) (W1 dx_d)[n][j]         for up to three tangent planes dx_d
// -- the decoder's projection 32 -> {64, 128, 256} -> 1..4 (reference magno.py:793-797) under `sample_jacobian`, whose chain of GEMM
// and activation-derivative launches (mlp.py: _jvp_rows, fused=False) writes and re-reads a [rows, hidden] fp32 tensor per plane and
// layer.  Here the hidden layer of the value and of every tangent plane stays in registers.
//
// The VALUE is the GEMM chain's bit for bit (gaot_gemm precision 0, gemm.hip; for hidden = 64 the second layer runs as
// gaot_rowlin_fwd, which is gaot_gemm's arithmetic too): v_mfma_f32_32x32x2_f32, instruction (q, s) of a layer taking
// k = 8 q + 4 half + s with k ascending over the whole reduction, the bias added AFTER the product, erf-GELU (gelu_f), the second
// layer's N padded to one 32-column block with zero weight rows.
//
// Layout: layer 1 is formed TRANSPOSED -- the W1 fragment is the A operand (hidden unit on the lane), x the B operand (row on the
// lane) -- so accumulator register r of hidden block ob holds hidden unit 32 ob + mfma32_row(r, half) of row lane & 31: exactly the
// A operand of layer 2's instruction r of that block in k_gemm's order.  The activated block goes from accumulator to operand without
// LDS.  The transposed product rounds as the untransposed one: the same products, the same k order inside the instruction.
// One wave owns 32 rows and walks all hidden blocks in ascending order; W1, b1 and W2 sit in LDS once per workgroup and their
// fragments are shared by all planes.  The tangent planes take the same path without bias: u_d = W1 dx_d, v_d = gelu'(z) u_d, then
// the same padded second layer.
//
// A row's result depends on that row alone (not on N, the row's position, its wave or workgroup); a plane's result does not depend
// on the other planes; a zero tangent plane gives zeros (every product is 0).  Grid-stride over 128-row tiles, no atomics, no
// workspace, no host synchronisation.
#include "common.h"

namespace {

constexpr int JV_IN = 32;          // input width
constexpr int JV_ROWS = 128;       // rows per workgroup and pass (4 waves x 32)
constexpr int JV_GRID_CAP = 512;   // two workgroups per CU
constexpr int JV_W1S = JV_IN + 4;  // row stride of W1 in LDS: 16-byte fragments, 16 consecutive lanes on 64 distinct banks

struct JvArgs {
    const float* x;
    const float* dx[3];
    const float* w1;
    const float* b1;
    const float* w2;
    const float* b2;   // or null
    float* y;
    float* jac;
    int64_t n, ldy, js_row, js_chan, js_dir;
    int oc;
};

__device__ __forceinline__ float f4at(const float4& v, int s) { return s == 0 ? v.x : s == 1 ? v.y : s == 2 ? v.z : v.w; }

template <int NOB, int T>
__global__ __launch_bounds__(256, 2) void k_mlp2_jvp(const JvArgs a) {
    constexpr int H = 32 * NOB;
    constexpr int W2S = H + 4;
    __shared__ __attribute__((aligned(16))) float w1s[H * JV_W1S];
    __shared__ __attribute__((aligned(16))) float w2s[4 * W2S];     // rows oc .. 3 are zero
    __shared__ __attribute__((aligned(16))) float b1s[H];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hf = lane >> 5;
    for (int i = threadIdx.x; i < H * JV_IN; i += 256) w1s[(i >> 5) * JV_W1S + (i & 31)] = a.w1[i];
    for (int i = threadIdx.x; i < 4 * H; i += 256) {
        const int c = i / H, j = i % H;
        w2s[c * W2S + j] = c < a.oc ? a.w2[c * H + j] : 0.f;
    }
    for (int i = threadIdx.x; i < H; i += 256) b1s[i] = a.b1[i];
    __syncthreads();
    const bool wlane = l31 < 4;      // the lanes whose column of the padded second layer can hold a weight
    const float* w2l = w2s + (l31 & 3) * W2S + 4 * hf;
    const float b2v = (a.b2 && l31 < a.oc) ? a.b2[l31] : 0.f;

    for (int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * 32; row0 < a.n; row0 += (int64_t)gridDim.x * JV_ROWS) {
        // B operand of layer 1: this lane's row, k = 8 q + 4 hf + s.  Rows past the end repeat the last row; nothing of them is stored.
        const int64_t row = row0 + l31 < a.n ? row0 + l31 : a.n - 1;
        float4 xf[1 + T][4];
#pragma unroll
        for (int p = 0; p <= T; ++p) {
            const float* src = (p == 0 ? a.x : a.dx[p > 0 ? p - 1 : 0]) + row * JV_IN + 4 * hf;
#pragma unroll
            for (int q = 0; q < 4; ++q) xf[p][q] = *reinterpret_cast<const float4*>(src + 8 * q);
        }
        f32x16 acc2[1 + T];
#pragma unroll
        for (int p = 0; p <= T; ++p)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc2[p][r] = 0.f;

#pragma unroll 1
        for (int ob = 0; ob < NOB; ++ob) {
            f32x16 z[1 + T];      // z, then u_d = W1 dx_d
#pragma unroll
            for (int p = 0; p <= T; ++p)
#pragma unroll
                for (int r = 0; r < 16; ++r) z[p][r] = 0.f;
            const float* w1l = w1s + (32 * ob + l31) * JV_W1S + 4 * hf;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 wf = *reinterpret_cast<const float4*>(w1l + 8 * q);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int p = 0; p <= T; ++p)
                        z[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4at(wf, s), f4at(xf[p][q], s), z[p], 0, 0, 0);
            }
            // register r: hidden unit 32 ob + 8 (r / 4) + 4 hf + r % 4 -- layer 2's k of instruction r
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 bq = *reinterpret_cast<const float4*>(b1s + 32 * ob + 8 * q + 4 * hf);
                float4 wq = *reinterpret_cast<const float4*>(w2l + 32 * ob + 8 * q);
                if (!wlane) wq = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int r = 4 * q + s;
                    float v = z[0][r];
                    v += f4at(bq, s);
                    const float w = f4at(wq, s);
                    acc2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(gelu_f(v), w, acc2[0], 0, 0, 0);
                    if (T > 0) {
                        const float g = gelu_grad_f(v);
#pragma unroll
                        for (int p = 1; p <= T; ++p) acc2[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(g * z[p][r], w, acc2[p], 0, 0, 0);
                    }
                }
            }
        }
        // acc2[p][r]: row row0 + mfma32_row(r, hf), channel l31
        if (l31 < a.oc) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t m = row0 + mfma32_row(r, hf);
                if (m >= a.n) continue;
                float v = acc2[0][r];
                v += b2v;
                a.y[m * a.ldy + l31] = v;
#pragma unroll
                for (int p = 1; p <= T; ++p) a.jac[m * a.js_row + l31 * a.js_chan + (p - 1) * a.js_dir] = acc2[p][r];
            }
        }
    }
}

bool shape_ok(int in_dim, int hidden, int out_dim, int num_tangents) {
    return in_dim == JV_IN && (hidden == 64 || hidden == 128 || hidden == 256) && out_dim >= 1 && out_dim <= 4 && num_tangents >= 0 &&
           num_tangents <= 3;
}

template <int NOB>
void launch_t(const JvArgs& a, int t, int grid, hipStream_t st) {
    switch (t) {
        case 0: GAOT_KLAUNCH((k_mlp2_jvp<NOB, 0>), dim3(grid), dim3(256), 0, st, a); break;
        case 1: GAOT_KLAUNCH((k_mlp2_jvp<NOB, 1>), dim3(grid), dim3(256), 0, st, a); break;
        case 2: GAOT_KLAUNCH((k_mlp2_jvp<NOB, 2>), dim3(grid), dim3(256), 0, st, a); break;
        default: GAOT_KLAUNCH((k_mlp2_jvp<NOB, 3>), dim3(grid), dim3(256), 0, st, a); break;
    }
}

}  // namespace

extern "C" int gaot_mlp2_jvp_supported(int in_dim, int hidden, int out_dim, int num_tangents, int act) {
    return (shape_ok(in_dim, hidden, out_dim, num_tangents) && act == GAOT_ACT_GELU) ? 1 : 0;
}

extern "C" int gaot_mlp2_jvp(const float* x, const float* dx0, const float* dx1, const float* dx2, int num_tangents, int64_t num_rows,
                             int in_dim, int hidden, int out_dim, const float* w1, const float* b1, const float* w2, const float* b2,
                             float* y, int64_t ldy, float* jac, int64_t jac_row_stride, int64_t jac_chan_stride, int64_t jac_dir_stride,
                             gaot_stream_t stream) {
    GAOT_ENTER();
    GAOT_CHECK_ARG(num_rows >= 0, "negative size");
    if (!shape_ok(in_dim, hidden, out_dim, num_tangents)) {
        gaot_set_error("gaot_mlp2_jvp: supported shapes are in = 32, hidden in {64, 128, 256}, out in 1..4, 0..3 tangents "
                       "(got %d -> %d -> %d, %d tangents)", in_dim, hidden, out_dim, num_tangents);
        return GAOT_ERR_UNSUPPORTED;
    }
    if (num_rows == 0) return GAOT_OK;
    GAOT_CHECK_ARG(x && w1 && b1 && w2 && y, "null pointer");
    GAOT_CHECK_ARG(ldy >= out_dim, "ldy is smaller than out_dim");
    const float* dxs[3] = {dx0, dx1, dx2};
    for (int d = 0; d < num_tangents; ++d) GAOT_CHECK_ARG(dxs[d] && ((uintptr_t)dxs[d] & 15) == 0, "null or unaligned tangent plane");
    GAOT_CHECK_ARG(((uintptr_t)x & 15) == 0, "x must be 16-byte aligned");
    GAOT_CHECK_ARG(num_tangents == 0 || (jac && jac_row_stride > 0 && jac_chan_stride > 0 && jac_dir_stride > 0),
                   "null Jacobian or non-positive stride");
    JvArgs a;
    a.x = x;
    for (int d = 0; d < 3; ++d) a.dx[d] = d < num_tangents ? dxs[d] : x;
    a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.y = y; a.jac = jac;
    a.n = num_rows; a.ldy = ldy; a.js_row = jac_row_stride; a.js_chan = jac_chan_stride; a.js_dir = jac_dir_stride; a.oc = out_dim;
    hipStream_t st = (hipStream_t)stream;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(num_rows, JV_ROWS), JV_GRID_CAP));
    if (hidden == 64) launch_t<2>(a, num_tangents, grid, st);
    else if (hidden == 128) launch_t<4>(a, num_tangents, grid, st);
    else launch_t<8>(a, num_tangents, grid, st);
    GAOT_LAUNCH_CHECK();
    return GAOT_OK;
}
