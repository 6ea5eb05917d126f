// Directional 2-jets of the per-node two-layer MLP in ONE pass, exact fp32: gaot_mlp2_jvp's scheme (mlp2_jvp.hip) with one more
// plane per direction.  With z = W1 x + b1 and, per direction d (up to three), a first-order plane dx_d and a second-order plane ddx_d:
//     y[n][c]    = sum_j W2[c][j] gelu(z[n][j]) + b2[c]
//     d1_d[n][c] = sum_j W2[c][j] gelu'(z[n][j]) u_d[n][j]                                      u_d = W1 dx_d
//     d2_d[n][c] = sum_j W2[c][j] (gelu''(z[n][j]) u_d[n][j]^2 + gelu'(z[n][j]) w_d[n][j])      w_d = W1 ddx_d
// -- the decoder's projection 32 -> {64, 128, 256} -> 1..4 under `sample_hessian` / `sample_laplacian`.  The second layer of a d2
// plane takes ONE operand per hidden unit, so a direction costs two second-layer chains, not three.
//
// Layout, operand order and rounding are k_mlp2_jvp's: layer 1 TRANSPOSED (the W1 fragment is the A operand, the row is on the lane),
// so that the activated accumulator block is layer 2's A operand without LDS; instruction (q, s) of a layer takes k = 8 q + 4 half + s
// with k ascending; the bias after the product; erf-GELU; the second layer's N padded to one 32-column block with zero weight rows.
// Hence y is gaot_mlp2_jvp's value and d1_d its tangent for the same dx_d, bit for bit.  A row's result depends on that row alone, a
// direction's planes on that direction alone; zero dx and ddx give zeros (every product is 0).
//
// Registers: 1 + 2 T planes of 16 input, 16 first-layer and 16 second-layer registers each -- 336 at T = 3, beyond the 256 of two waves
// per SIMD -- so one workgroup per CU (__launch_bounds__(256, 1)); the projection is the small stage of the pipeline.  W1, b1 and W2
// sit in LDS once per workgroup.  Grid-stride over 128-row tiles, no scratch, no atomics, no workspace, no host synchronisation.
#include "common.h"

namespace {

constexpr int J2_IN = 32;          // input width
constexpr int J2_ROWS = 128;       // rows per workgroup and pass (4 waves x 32)
constexpr int J2_GRID_CAP = 256;   // one workgroup per CU
constexpr int J2_W1S = J2_IN + 4;  // row stride of W1 in LDS (k_mlp2_jvp's)

struct J2Args {
    const float* x;
    const float* dx[3];
    const float* ddx[3];
    const float* w1;
    const float* b1;
    const float* w2;
    const float* b2;   // or null
    float* y;          // or null: the value is not stored
    float* d1;
    float* d2;
    int64_t n, ldy, s_row, s_chan, s_dir;
    int oc;
};

__device__ __forceinline__ float f4at(const float4& v, int s) { return s == 0 ? v.x : s == 1 ? v.y : s == 2 ? v.z : v.w; }

// planes: 0 the value, 1 + 2 d the first-order plane of direction d, 2 + 2 d its second-order plane
template <int NOB, int T>
__global__ __launch_bounds__(256, 1) void k_mlp2_jet2(const J2Args a) {
    constexpr int H = 32 * NOB;
    constexpr int W2S = H + 4;
    constexpr int NP = 1 + 2 * T;
    __shared__ __attribute__((aligned(16))) float w1s[H * J2_W1S];
    __shared__ __attribute__((aligned(16))) float w2s[4 * W2S];     // rows oc .. 3 are zero
    __shared__ __attribute__((aligned(16))) float b1s[H];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hf = lane >> 5;
    for (int i = threadIdx.x; i < H * J2_IN; i += 256) w1s[(i >> 5) * J2_W1S + (i & 31)] = a.w1[i];
    for (int i = threadIdx.x; i < 4 * H; i += 256) {
        const int c = i / H, j = i % H;
        w2s[c * W2S + j] = c < a.oc ? a.w2[c * H + j] : 0.f;
    }
    for (int i = threadIdx.x; i < H; i += 256) b1s[i] = a.b1[i];
    __syncthreads();
    const bool wlane = l31 < 4;      // the lanes whose column of the padded second layer can hold a weight
    const float* w2l = w2s + (l31 & 3) * W2S + 4 * hf;
    const float b2v = (a.b2 && l31 < a.oc) ? a.b2[l31] : 0.f;

    for (int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * 32; row0 < a.n; row0 += (int64_t)gridDim.x * J2_ROWS) {
        // B operand of layer 1: this lane's row, k = 8 q + 4 hf + s.  Rows past the end repeat the last row; nothing of them is stored.
        const int64_t row = row0 + l31 < a.n ? row0 + l31 : a.n - 1;
        float4 xf[NP][4];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int d = p > 0 ? (p - 1) >> 1 : 0;
            const float* src = (p == 0 ? a.x : (p & 1) ? a.dx[d] : a.ddx[d]) + row * J2_IN + 4 * hf;
#pragma unroll
            for (int q = 0; q < 4; ++q) xf[p][q] = *reinterpret_cast<const float4*>(src + 8 * q);
        }
        f32x16 acc2[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc2[p][r] = 0.f;

#pragma unroll 1
        for (int ob = 0; ob < NOB; ++ob) {
            f32x16 z[NP];      // z, then u_d = W1 dx_d and w_d = W1 ddx_d
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int r = 0; r < 16; ++r) z[p][r] = 0.f;
            const float* w1l = w1s + (32 * ob + l31) * J2_W1S + 4 * hf;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 wf = *reinterpret_cast<const float4*>(w1l + 8 * q);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int p = 0; p < NP; ++p)
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
                    const float g = gelu_grad_f(v);
                    const float g2 = gelu_grad2_f(v);
#pragma unroll
                    for (int d = 0; d < T; ++d) {
                        const float u = z[1 + 2 * d][r];
                        acc2[1 + 2 * d] = __builtin_amdgcn_mfma_f32_32x32x2f32(g * u, w, acc2[1 + 2 * d], 0, 0, 0);
                        acc2[2 + 2 * d] = __builtin_amdgcn_mfma_f32_32x32x2f32(fmaf(g, z[2 + 2 * d][r], g2 * u * u), w, acc2[2 + 2 * d], 0, 0, 0);
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
                if (a.y) {
                    float v = acc2[0][r];
                    v += b2v;
                    a.y[m * a.ldy + l31] = v;
                }
#pragma unroll
                for (int d = 0; d < T; ++d) {
                    const int64_t o = m * a.s_row + l31 * a.s_chan + d * a.s_dir;
                    a.d1[o] = acc2[1 + 2 * d][r];
                    a.d2[o] = acc2[2 + 2 * d][r];
                }
            }
        }
    }
}

bool shape_ok(int in_dim, int hidden, int out_dim, int nd) {
    return in_dim == J2_IN && (hidden == 64 || hidden == 128 || hidden == 256) && out_dim >= 1 && out_dim <= 4 && nd >= 1 && nd <= 3;
}

template <int NOB>
void launch_t(const J2Args& a, int t, int grid, hipStream_t st) {
    switch (t) {
        case 1: GAOT_KLAUNCH((k_mlp2_jet2<NOB, 1>), dim3(grid), dim3(256), 0, st, a); break;
        case 2: GAOT_KLAUNCH((k_mlp2_jet2<NOB, 2>), dim3(grid), dim3(256), 0, st, a); break;
        default: GAOT_KLAUNCH((k_mlp2_jet2<NOB, 3>), dim3(grid), dim3(256), 0, st, a); break;
    }
}

}  // namespace

extern "C" int gaot_mlp2_jet2_supported(int in_dim, int hidden, int out_dim, int nd, int act) {
    return (shape_ok(in_dim, hidden, out_dim, nd) && act == GAOT_ACT_GELU) ? 1 : 0;
}

extern "C" int gaot_mlp2_jet2(const float* x, const float* dx0, const float* dx1, const float* dx2, const float* ddx0, const float* ddx1,
                              const float* ddx2, int nd, int64_t num_rows, int in_dim, int hidden, int out_dim, const float* w1,
                              const float* b1, const float* w2, const float* b2, float* y, int64_t ldy, float* d1, float* d2,
                              int64_t row_stride, int64_t chan_stride, int64_t dir_stride, gaot_stream_t stream) {
    GAOT_ENTER();
    GAOT_CHECK_ARG(num_rows >= 0, "negative size");
    if (!shape_ok(in_dim, hidden, out_dim, nd)) {
        gaot_set_error("gaot_mlp2_jet2: supported shapes are in = 32, hidden in {64, 128, 256}, out in 1..4, 1..3 directions "
                       "(got %d -> %d -> %d, %d directions)", in_dim, hidden, out_dim, nd);
        return GAOT_ERR_UNSUPPORTED;
    }
    if (num_rows == 0) return GAOT_OK;
    GAOT_CHECK_ARG(x && w1 && b1 && w2 && d1 && d2, "null pointer");
    GAOT_CHECK_ARG(!y || ldy >= out_dim, "ldy is smaller than out_dim");
    GAOT_CHECK_ARG(row_stride > 0 && chan_stride > 0 && dir_stride > 0, "non-positive stride");
    GAOT_CHECK_ARG(((uintptr_t)x & 15) == 0, "x must be 16-byte aligned");
    const float* dx[3] = {dx0, dx1, dx2};
    const float* ddx[3] = {ddx0, ddx1, ddx2};
    J2Args a;
    a.x = x;
    for (int d = 0; d < 3; ++d) {
        if (d < nd) GAOT_CHECK_ARG(dx[d] && ddx[d] && (((uintptr_t)dx[d] | (uintptr_t)ddx[d]) & 15) == 0, "null or unaligned direction plane");
        a.dx[d] = d < nd ? dx[d] : x;
        a.ddx[d] = d < nd ? ddx[d] : x;
    }
    a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.y = y; a.d1 = d1; a.d2 = d2;
    a.n = num_rows; a.ldy = ldy; a.s_row = row_stride; a.s_chan = chan_stride; a.s_dir = dir_stride; a.oc = out_dim;
    hipStream_t st = (hipStream_t)stream;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(num_rows, J2_ROWS), J2_GRID_CAP));
    if (hidden == 64) launch_t<2>(a, nd, grid, st);
    else if (hidden == 128) launch_t<4>(a, nd, grid, st);
    else launch_t<8>(a, nd, grid, st);
    GAOT_LAUNCH_CHECK();
    return GAOT_OK;
}
