// Backward of the per-node two-layer MLP  y = W2 gelu(W1 x + b1) + b2  in ONE pass, exact fp32: the exact-fp32 sibling of
// gaot_mlp2_bwd (mlp2.hip, bf16 operands) for the decoder's projection 32 -> {64, 128, 256} -> 1..4 (reference magno.py:793-797)
// under MAGNODecoder.sample_vjp_params.  From x, W1, b1, W2 and d_out [rows, out] it writes
//     d_x  = dz W1,   d_W1 = dz^T x,   d_b1 = colsum(dz),   d_W2 = d_out^T gelu(z),        z = W1 x + b1,  dz = (d_out W2) * gelu'(z)
// and z, gelu(z), gelu'(z) and dz live in registers (one transposed copy of a 32 x 32 block of dz in LDS): the GEMM chain writes and
// re-reads three [rows, hidden] fp32 tensors for the same five results.  d_b2 is the column sum of d_out (gaot_colsum).
//
// Every product is v_mfma_f32_32x32x2_f32, instruction (q, s) of a K = 32 reduction taking k = 8 q + 4 half + s -- the layer-1 operand
// layout and the W1 image in LDS (row stride 36) of mlp2_jvp.hip.  A workgroup takes 128 rows per pass in four sub-tiles of 32 rows; a
// wave OWNS hidden blocks (32 units each: hidden / 128 per wave, for hidden = 64 two waves own one each and two only load and sum),
// so its accumulators for d_W1 and d_W2 live in registers over the whole grid-stride loop.  Per sub-tile and owned block:
//     z [row on registers][hidden on lanes]     = x W1^T                      (16 instructions; A = x, B = W1 from LDS)
//     dy                                         = d_out W2^T                  (2, K padded to 4 with zeros)
//     g = gelu(z + b1), dz = dy * gelu'(z + b1)                                 (erf-GELU, common.h)
//     d_W2 [channel][hidden]                    += d_out^T g                   (16; the accumulator registers are the B operand)
//     d_W1^T [feature][hidden]                  += x^T dz                      (16; likewise)
//     d_b1 [hidden]                             += sum over the lane's 16 rows (the two halves are added once, at the end)
//     d_x^T [feature][row]                      += W1^T dz^T                   (16; dz through the wave's LDS tile, transposed)
// The waves' partial d_x (each over its own hidden units) are added through LDS in wave order, so a row's d_x depends on that row
// alone -- not on N, the row's position or its workgroup.  Rows past the end take d_out = 0 and add nothing.
//
// Weight-gradient partials go per workgroup into three tables [workgroup][hidden * 32] | [workgroup][hidden] | [workgroup][out * hidden]
// that gaot_reduce_multi sums in a fixed order (lanes = 4): no atomics, bit-reproducible for a given N.
#include "common.h"

namespace {

constexpr int BF_IN = 32;          // input width
constexpr int BF_ROWS = 128;       // rows per workgroup and pass (4 sub-tiles of 32)
constexpr int BF_GRID_CAP = 512;   // two workgroups per CU
constexpr int BF_W1S = BF_IN + 4;  // row stride of W1 in LDS (mlp2_jvp.hip)
constexpr int BF_DZS = 36;         // row stride of the dz tile [row][hidden]: 16-byte fragments
constexpr int BF_DXS = 33;         // row stride of the d_x^T partial [feature][row]

struct BfArgs {
    const float* x;
    const float* w1;
    const float* b1;
    const float* w2;
    const float* dout;
    float* dx;
    float* wpart;
    int64_t n;
    int oc;
};

__device__ __forceinline__ float bf_f4at(const float4& v, int s) { return s == 0 ? v.x : s == 1 ? v.y : s == 2 ? v.z : v.w; }

// LDS operations of one wave complete in order; this keeps the compiler from moving them across the hand-over
__device__ __forceinline__ void bf_wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int NOB>
__global__ __launch_bounds__(256, 2) void k_mlp2_bwd_f32(const BfArgs a) {
    constexpr int H = 32 * NOB, OBW = NOB >= 4 ? NOB / 4 : 1, NW = NOB >= 4 ? 4 : NOB;   // NW: waves that own hidden blocks
    __shared__ __attribute__((aligned(16))) float w1s[H * BF_W1S];
    // per wave: the dz tile [32 rows][BF_DZS], then (its last use is behind the wave) the wave's d_x^T partial [32 features][BF_DXS]
    __shared__ __attribute__((aligned(16))) float tile[4][32 * BF_DZS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hf = lane >> 5;
    const bool owner = wave < NW;
    for (int i = threadIdx.x; i < H * BF_IN; i += 256) w1s[(i >> 5) * BF_W1S + (i & 31)] = a.w1[i];

    float b1l[OBW], w2f[OBW][2], db1[OBW];
    f32x16 dw1[OBW], dw2;      // dw2: row 4 o + c of the accumulator is channel c of owned block o
#pragma unroll
    for (int o = 0; o < OBW; ++o) {
        const int j = 32 * (wave * OBW + o) + l31;      // this lane's hidden unit of block o
        b1l[o] = owner ? a.b1[j] : 0.f;
#pragma unroll
        for (int s = 0; s < 2; ++s) w2f[o][s] = (owner && 2 * s + hf < a.oc) ? a.w2[(2 * s + hf) * H + j] : 0.f;
        db1[o] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) dw1[o][r] = 0.f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) dw2[r] = 0.f;
    float* mytile = tile[wave];
    __syncthreads();

#pragma unroll 1
    for (int64_t row0 = (int64_t)blockIdx.x * BF_ROWS; row0 < a.n; row0 += (int64_t)gridDim.x * BF_ROWS) {
#pragma unroll 1
        for (int t = 0; t < 4; ++t) {
            const int64_t sub0 = row0 + 32 * t;
            if (sub0 >= a.n) break;      // uniform over the workgroup
            if (owner) {
                // operands of this sub-tile, at 32-bit offsets from its first row.  Rows past the end repeat the last row with
                // d_out = 0: dz = 0, nothing is added.
                const int last = (int)std::min<int64_t>(a.n - 1 - sub0, 31);
                const float* xs = a.x + sub0 * BF_IN;
                const float* ds = a.dout + sub0 * a.oc;
                const bool rok = l31 <= last;
                const int lr = rok ? l31 : last;
                float4 xf[4];            // x [row = l31][k = 8 q + 4 hf + s]
#pragma unroll
                for (int q = 0; q < 4; ++q) xf[q] = *reinterpret_cast<const float4*>(xs + lr * BF_IN + 4 * hf + 8 * q);
                float dof[2];            // d_out [row = l31][c = 2 s + hf]
#pragma unroll
                for (int s = 0; s < 2; ++s) dof[s] = (rok && 2 * s + hf < a.oc) ? ds[lr * a.oc + 2 * s + hf] : 0.f;
                float xt[16], dor[16];   // x [row of register r][feature = l31], d_out [row of register r][c = l31 % 4] on lanes < 4 OBW
                const bool dlane = l31 < 4 * OBW && (l31 & 3) < a.oc;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = mfma32_row(r, hf);
                    xt[r] = xs[(m <= last ? m : last) * BF_IN + l31];
                    dor[r] = (dlane && m <= last) ? ds[m * a.oc + (l31 & 3)] : 0.f;
                }
                f32x16 dxt;              // d_x^T [feature][row] over this wave's hidden units
#pragma unroll
                for (int r = 0; r < 16; ++r) dxt[r] = 0.f;
#pragma unroll
                for (int o = 0; o < OBW; ++o) {
                    const int ob = wave * OBW + o;
                    f32x16 z, dy;
#pragma unroll
                    for (int r = 0; r < 16; ++r) z[r] = 0.f;
                    const float* w1l = w1s + (32 * ob + l31) * BF_W1S + 4 * hf;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 wf = *reinterpret_cast<const float4*>(w1l + 8 * q);
#pragma unroll
                        for (int s = 0; s < 4; ++s) z = __builtin_amdgcn_mfma_f32_32x32x2f32(bf_f4at(xf[q], s), bf_f4at(wf, s), z, 0, 0, 0);
                    }
                    // register r: row sub0 + mfma32_row(r, hf), hidden unit 32 ob + l31.  z -> gelu'(z) in place, gelu(z) goes straight
                    // into d_W2's product (block o's d_out on lanes 4 o .. 4 o + 3); dy is formed after, so it is not live beside the erf
                    const bool mine = (l31 >> 2) == o;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = z[r] + b1l[o];
                        dw2 = __builtin_amdgcn_mfma_f32_32x32x2f32(mine ? dor[r] : 0.f, gelu_f(v), dw2, 0, 0, 0);
                        z[r] = gelu_grad_f(v);
                        if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // four erf evaluations in flight, not sixteen
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int r = 0; r < 16; ++r) dy[r] = 0.f;
#pragma unroll
                    for (int s = 0; s < 2; ++s) dy = __builtin_amdgcn_mfma_f32_32x32x2f32(dof[s], w2f[o][s], dy, 0, 0, 0);
                    float s1 = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        z[r] *= dy[r];
                        s1 += z[r];
                    }
                    db1[o] += s1;
#pragma unroll
                    for (int r = 0; r < 16; ++r) dw1[o] = __builtin_amdgcn_mfma_f32_32x32x2f32(xt[r], z[r], dw1[o], 0, 0, 0);
                    // dz [row][hidden] through the wave's tile: read back with the row on the lane, k = hidden 8 q + 4 hf + s
                    bf_wave_order();
#pragma unroll
                    for (int r = 0; r < 16; ++r) mytile[mfma32_row(r, hf) * BF_DZS + l31] = z[r];
                    bf_wave_order();
                    const float* w1c = w1s + (32 * ob + 4 * hf) * BF_W1S + l31;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 df = *reinterpret_cast<const float4*>(mytile + l31 * BF_DZS + 8 * q + 4 * hf);
#pragma unroll
                        for (int s = 0; s < 4; ++s)
                            dxt = __builtin_amdgcn_mfma_f32_32x32x2f32(w1c[(8 * q + s) * BF_W1S], bf_f4at(df, s), dxt, 0, 0, 0);
                    }
                }
                bf_wave_order();
#pragma unroll
                for (int r = 0; r < 16; ++r) mytile[mfma32_row(r, hf) * BF_DXS + l31] = dxt[r];
            }
            __syncthreads();
            // d_x [row][k] = the owners' partials in wave order; thread = (row, 4 features): a row's 128 bytes from 8 threads
            {
                const int row = threadIdx.x >> 3, k0 = (threadIdx.x & 7) * 4;
                if (sub0 + row < a.n) {
                    float v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float s = tile[0][(k0 + k) * BF_DXS + row];
#pragma unroll
                        for (int w = 1; w < NW; ++w) s += tile[w][(k0 + k) * BF_DXS + row];
                        v[k] = s;
                    }
                    *reinterpret_cast<float4*>(a.dx + (sub0 + row) * BF_IN + k0) = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
            __syncthreads();
        }
    }
    if (!owner) return;
    float* wp1 = a.wpart + (int64_t)blockIdx.x * (H * BF_IN);
    float* wpb = a.wpart + (int64_t)gridDim.x * (H * BF_IN) + (int64_t)blockIdx.x * H;
    float* wp2 = a.wpart + (int64_t)gridDim.x * (H * BF_IN + H) + (int64_t)blockIdx.x * (a.oc * H);
#pragma unroll
    for (int o = 0; o < OBW; ++o) {
        const int j = 32 * (wave * OBW + o) + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) wp1[(int64_t)j * BF_IN + mfma32_row(r, hf)] = dw1[o][r];      // register r: feature, lane: hidden
        const float d1 = db1[o] + __shfl_xor(db1[o], 32, 64);
        if (hf == 0) wpb[j] = d1;
        if (hf == o) {      // d_W2: register c of half o is accumulator row 4 o + c = channel c of block o
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < a.oc) wp2[c * H + j] = dw2[c];
        }
    }
}

bool shape_ok(int in_dim, int hidden, int out_dim) {
    return in_dim == BF_IN && (hidden == 64 || hidden == 128 || hidden == 256) && out_dim >= 1 && out_dim <= 4;
}

int64_t parts_of(int64_t num_rows) { return std::min<int64_t>(ceil_div(std::max<int64_t>(num_rows, 0), BF_ROWS), BF_GRID_CAP); }

}  // namespace

extern "C" int gaot_mlp2_bwd_f32_supported(int in_dim, int hidden, int out_dim, int act) {
    return (shape_ok(in_dim, hidden, out_dim) && act == GAOT_ACT_GELU) ? 1 : 0;
}

extern "C" size_t gaot_mlp2_bwd_f32_workspace_bytes(int hidden, int out_dim) {
    if (hidden <= 0 || out_dim <= 0) return 64;
    return sizeof(float) * (size_t)BF_GRID_CAP * ((size_t)hidden * BF_IN + hidden + (size_t)out_dim * hidden) + 64;
}

extern "C" int64_t gaot_mlp2_bwd_f32_parts(int64_t num_rows) { return parts_of(num_rows); }

extern "C" int gaot_mlp2_bwd_f32(const float* x, int64_t num_rows, int in_dim, int hidden, int out_dim, const float* w1, const float* b1,
                                 const float* w2, const float* d_out, float* d_x, float* d_w1, float* d_b1, float* d_w2,
                                 void* workspace, size_t workspace_bytes, gaot_stream_t stream) {
    GAOT_ENTER();
    GAOT_CHECK_ARG(num_rows >= 0, "negative size");
    if (!shape_ok(in_dim, hidden, out_dim)) {
        gaot_set_error("gaot_mlp2_bwd_f32: supported shapes are in = 32, hidden in {64, 128, 256}, out in 1..4 (got %d -> %d -> %d)",
                       in_dim, hidden, out_dim);
        return GAOT_ERR_UNSUPPORTED;
    }
    GAOT_CHECK_ARG((d_w1 && d_b1 && d_w2) || (!d_w1 && !d_b1 && !d_w2), "d_w1, d_b1 and d_w2 go together");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n1 = (int64_t)hidden * BF_IN, n2 = hidden, n3 = (int64_t)out_dim * hidden;
    if (num_rows == 0) {      // no launch: the three weight gradients are exact zeros
        if (d_w1) {
            if (hipMemsetAsync(d_w1, 0, sizeof(float) * n1, st) != hipSuccess || hipMemsetAsync(d_b1, 0, sizeof(float) * n2, st) != hipSuccess ||
                hipMemsetAsync(d_w2, 0, sizeof(float) * n3, st) != hipSuccess) {
                gaot_set_error("gaot_mlp2_bwd_f32: cannot clear the weight gradients");
                return GAOT_ERR_LAUNCH;
            }
        }
        return GAOT_OK;
    }
    GAOT_CHECK_ARG(x && w1 && b1 && w2 && d_out && d_x, "null pointer");
    GAOT_CHECK_ARG((((uintptr_t)x | (uintptr_t)d_x) & 15) == 0, "x and d_x must be 16-byte aligned");
    GAOT_CHECK_ARG(workspace && ((uintptr_t)workspace & 3) == 0 && workspace_bytes >= gaot_mlp2_bwd_f32_workspace_bytes(hidden, out_dim),
                   "workspace null, unaligned or too small");
    const int grid = (int)parts_of(num_rows);
    float* wpart = (float*)workspace;
    BfArgs a{x, w1, b1, w2, d_out, d_x, wpart, num_rows, out_dim};
    if (hidden == 64) GAOT_KLAUNCH((k_mlp2_bwd_f32<2>), dim3(grid), dim3(256), 0, st, a);
    else if (hidden == 128) GAOT_KLAUNCH((k_mlp2_bwd_f32<4>), dim3(grid), dim3(256), 0, st, a);
    else GAOT_KLAUNCH((k_mlp2_bwd_f32<8>), dim3(grid), dim3(256), 0, st, a);
    GAOT_LAUNCH_CHECK();
    if (!d_w1) return GAOT_OK;      // the three tables stay in the workspace for gaot_reduce_multi (lanes = 4)
    const gaot_reduce_desc_t descs[3] = {{wpart, d_w1, n1, grid, 4}, {wpart + grid * n1, d_b1, n2, grid, 4},
                                         {wpart + grid * (n1 + n2), d_w2, n3, grid, 4}};
    return gaot_reduce_multi(descs, 3, stream);
}
