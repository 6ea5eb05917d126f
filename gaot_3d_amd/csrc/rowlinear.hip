// Thin fp32 linears over many rows in ONE pass:  y = act([x_0 | x_1 | ...] W^T + b)  and its autograd -- the per-point /
// per-token linears around the two GNOs (lifting, GeoEmbed MLP, recovery: reference magno.py:494,571-575,771-775 and
// geoembed.py), 3 .. 64 columns wide over 131 K .. 500 K rows.  As GEMM launches each of them wrote, re-read and re-wrote its
// output once per input (the concatenation chained through the residual operand), and the backward read dy once per weight
// block, once per input gradient and once for the bias; here every row of every operand is read once and written once.
//
// Arithmetic: v_mfma_f32_32x32x2_f32 -- exact fp32 products, fp32 accumulation (what precision 0 means in gemm.hip) -- in
// the ORDER of the GEMM launches these kernels replace, so the results are theirs bit for bit:
//   * a product's k runs as in k_gemm: instruction t takes k = 8 (t / 4) + 4 half + t % 4 (zero columns pad to 16);
//   * forward: one accumulator per input, y = act(acc_0 + b), then y = acc_i + y for the further inputs (the residual chain);
//   * dW: the rows are cut into the split-K ranges of gaot_gemm's plan (gaot_gemm_dw_plan), one wave per range, the partials
//     summed by gaot_reduce_multi with the plan's lane count; db: the row chunks and the eight row lanes of gaot_colsum.
// A row's result depends on that row alone: not on M, not on the row's position, not on the wave or workgroup that took it.
//
// One wave = 32 rows per pass, a workgroup = 4 waves = 128 rows, grid-stride over the row tiles.  Columns go in blocks of 32:
// NNB blocks of outputs, NKB blocks of inputs (an input of 33 .. 64 columns is two blocks), NNB * NKB <= 4.
// Every global access is the same pattern: lane = column of the block, half-wave = row parity, 16 loads for the 32 rows of a
// tile (`load_tile`) -- whole 128-byte row segments.  That is already the operand layout of the weight-gradient product
// (dW[n][k] = sum_rows dz[row][n] x[row][k]: rows are the MFMA's k).  The products whose k is a COLUMN (forward: x W^T,
// backward: dz W) take their row operand through a wave-private LDS tile written [row][col] and read back with the row on
// the lane; W sits in LDS once per workgroup, zero-padded to the block grid.
//
// Backward: dz = dy (* (y > 0) for ReLU, from the SAVED OUTPUT -- no pre-activation is kept).  A wave walks one split range
// of rows: dW accumulates in registers and leaves as that split's partial row ([splits][N * Ktot]); the input gradients of
// its rows are written on the way.  The launch's last workgroups form db's partial rows ([chunks][N]) from a second read of
// dy (mostly from cache).  No atomics, reruns bit-identical.
#include "common.h"

namespace {

constexpr int RL_MAXIN = 4;        // inputs
constexpr int RL_MAXKB = 4;        // 32-column blocks over all inputs
constexpr int RL_ROWS = 128;       // rows per workgroup and pass
constexpr int RL_GRID_CAP = 512;   // forward: two workgroups per CU
constexpr int RL_XS = 33;          // row stride of a wave's [32][32] tile (odd: row-on-lane reads hit 32 banks)
constexpr int RL_DZS = 65;         // row stride of a wave's [32][64] dz tile

struct RlArgs {
    const float* x[RL_MAXKB];   // per input block: the input it belongs to
    float* dx[RL_MAXKB];        //                  that input's gradient, or null
    int K[RL_MAXKB];            //                  the input's width
    int c0[RL_MAXKB];           //                  first column of the block in its input
    int w0[RL_MAXKB];           //                  first column of the block in W
    const float* W;             // [N][Ktot]
    const float* b;             // [N] or null
    int64_t M;
    int N, Ktot, relu;
};

// v[i] = p[row0 + mfma32_row(i, hf)][col] for the 32 rows of a tile (instruction i of a product over the rows takes rows
// 8 (i / 4) + 4 hf + i % 4: k_gemm's order), 0 from row `end` on; the loads are unconditional (clamped) so all 16 are requested together
__device__ __forceinline__ void load_tile(const float* __restrict__ p, int64_t row0, int64_t end, int ld, int col, bool colok, int hf,
                                          float (&v)[16]) {
    float t[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t row = row0 + mfma32_row(i, hf);
        const bool ok = colok && row < end;
        t[i] = p[ok ? row * ld + col : 0];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = (colok && row0 + mfma32_row(i, hf) < end) ? t[i] : 0.f;
}

// W -> ws[n][32 kb + kk] (row stride 32 NKB + 1), zero outside [N] x the block's real columns
template <int NNB, int NKB>
__device__ __forceinline__ void stage_w(const RlArgs& a, float* ws) {
    constexpr int WS = 32 * NKB + 1;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
        const int kw = a.K[kb] - a.c0[kb];   // real columns from the block's first one on
        for (int i = threadIdx.x; i < 32 * NNB * 32; i += 256) {
            const int n = i >> 5, kk = i & 31;
            const bool ok = n < a.N && kk < kw;
            ws[n * WS + 32 * kb + kk] = ok ? a.W[(int64_t)n * a.Ktot + a.w0[kb] + kk] : 0.f;
        }
    }
}

template <int NNB, int NKB>
__global__ __launch_bounds__(256) void k_rowlin_fwd(const RlArgs a, float* __restrict__ y) {
    constexpr int WS = 32 * NKB + 1;
    __shared__ float ws[32 * NNB * WS];
    __shared__ float xs_all[4][32 * RL_XS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hf = lane >> 5;
    float* xs = xs_all[wave];
    stage_w<NNB, NKB>(a, ws);
    __syncthreads();
    float bn[NNB];
#pragma unroll
    for (int nb = 0; nb < NNB; ++nb) bn[nb] = (a.b && 32 * nb + l31 < a.N) ? a.b[32 * nb + l31] : 0.f;
    for (int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * 32; row0 < a.M; row0 += (int64_t)gridDim.x * RL_ROWS) {
        f32x16 acc[NNB], yr[NNB];       // the running input's product; the result so far
#pragma unroll
        for (int nb = 0; nb < NNB; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[nb][r] = 0.f; yr[nb][r] = 0.f; }
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            if (kb > 0 && a.c0[kb] == 0) {      // a further input begins: close the one before it
#pragma unroll
                for (int nb = 0; nb < NNB; ++nb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        yr[nb][r] = a.w0[kb - 1] - a.c0[kb - 1] == 0 ? acc[nb][r] + bn[nb] : acc[nb][r] + yr[nb][r];
                        acc[nb][r] = 0.f;
                    }
            }
            const int kw = min(32, a.K[kb] - a.c0[kb]);
            float v[16];
            load_tile(a.x[kb], row0, a.M, a.K[kb], a.c0[kb] + l31, l31 < kw, hf, v);
            __builtin_amdgcn_wave_barrier();      // the previous block's reads are issued (LDS runs a wave's operations in order)
#pragma unroll
            for (int i = 0; i < 16; ++i) xs[mfma32_row(i, hf) * RL_XS + l31] = v[i];
            __builtin_amdgcn_wave_barrier();
            const int steps = 4 * ((kw + 7) >> 3);   // k = 8 (t / 4) + 4 hf + t % 4; columns past the width are zero
            for (int t = 0; t < steps; ++t) {
                const int k = 8 * (t >> 2) + 4 * hf + (t & 3);
                const float xa = xs[l31 * RL_XS + k];
#pragma unroll
                for (int nb = 0; nb < NNB; ++nb)
                    acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa, ws[(32 * nb + l31) * WS + 32 * kb + k], acc[nb], 0, 0, 0);
            }
        }
        const bool single = a.w0[NKB - 1] - a.c0[NKB - 1] == 0;     // the last input is the first one
#pragma unroll
        for (int nb = 0; nb < NNB; ++nb) {
            const int n = 32 * nb + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = row0 + mfma32_row(r, hf);
                float v;
                if (single) {
                    v = acc[nb][r] + bn[nb];
                    if (a.relu) v = v > 0.f ? v : 0.f;
                } else {
                    v = acc[nb][r] + yr[nb][r];
                }
                if (row < a.M && n < a.N) y[row * a.N + n] = v;
            }
        }
    }
}

// nsw workgroups of four waves walk the `splits` row ranges of kps rows (dW partial rows + the rows' input gradients); the
// workgroups behind them form one db partial row each from rpc rows, as gaot_colsum's kernels do: eight row lanes, each adding
// every eighth row in row order, then the lanes in lane order
template <int NNB, int NKB>
__global__ __launch_bounds__(256) void k_rowlin_bwd(const RlArgs a, const float* __restrict__ dy, const float* __restrict__ y,
                                                    float* __restrict__ part_w, float* __restrict__ part_b, int splits, int64_t kps,
                                                    int nsw, int64_t rpc) {
    constexpr int WS = 32 * NKB + 1;
    __shared__ float ws[32 * NNB * WS];
    __shared__ float dzs_all[4][32 * RL_DZS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hf = lane >> 5;
    if ((int)blockIdx.x >= nsw) {
        float (*sm)[33] = reinterpret_cast<float (*)[33]>(dzs_all);
        const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
        const int64_t c = (int64_t)blockIdx.x - nsw;
        const int64_t r0 = c * rpc, r1 = (r0 + rpc < a.M) ? r0 + rpc : a.M;
#pragma unroll
        for (int nb = 0; nb < NNB; ++nb) {
            const int n = 32 * nb + cx;
            float s = 0.f;
            if (n < a.N) {
                int64_t r = r0 + ry;
                for (; r + 24 < r1; r += 32) {      // four rows requested together, added in row order
                    float d[4], yv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) d[u] = dy[(r + 8 * u) * a.N + n];
                    if (a.relu) {
#pragma unroll
                        for (int u = 0; u < 4; ++u) yv[u] = y[(r + 8 * u) * a.N + n];
#pragma unroll
                        for (int u = 0; u < 4; ++u) d[u] = yv[u] > 0.f ? d[u] : 0.f;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) s += d[u];
                }
                for (; r < r1; r += 8) {
                    float d = dy[r * a.N + n];
                    if (a.relu) d = y[r * a.N + n] > 0.f ? d : 0.f;
                    s += d;
                }
            }
            __syncthreads();
            sm[ry][cx] = s;
            __syncthreads();
            if (ry == 0 && n < a.N) {
                float t = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) t += sm[j][cx];
                part_b[c * a.N + n] = t;
            }
        }
        return;
    }
    float* dzs = dzs_all[wave];
    bool any_dx = false;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) any_dx = any_dx || a.dx[kb] != nullptr;
    if (any_dx) stage_w<NNB, NKB>(a, ws);
    __syncthreads();
    const int sp = blockIdx.x * 4 + wave;
    if (sp >= splits) return;
    const int64_t kbeg = (int64_t)sp * kps, kend = (kbeg + kps < a.M) ? kbeg + kps : a.M;
    f32x16 dw[NNB][NKB];
#pragma unroll
    for (int nb = 0; nb < NNB; ++nb)
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) dw[nb][kb][r] = 0.f;
    for (int64_t row0 = kbeg; row0 < kend; row0 += 32) {
        float dz[NNB][16];
#pragma unroll
        for (int nb = 0; nb < NNB; ++nb) {
            const int n = 32 * nb + l31;
            load_tile(dy, row0, kend, a.N, n, n < a.N, hf, dz[nb]);
            if (a.relu) {
                float yv[16];
                load_tile(y, row0, kend, a.N, n, n < a.N, hf, yv);
#pragma unroll
                for (int i = 0; i < 16; ++i) dz[nb][i] = yv[i] > 0.f ? dz[nb][i] : 0.f;
            }
        }
        // dW[n][k] += sum over the tile's rows (instruction t: rows 8 (t / 4) + 4 hf + t % 4) of dz[row][n] x[row][k]
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            const int kw = a.K[kb] - a.c0[kb];
            float xv[16];
            load_tile(a.x[kb], row0, kend, a.K[kb], a.c0[kb] + l31, l31 < kw, hf, xv);
#pragma unroll
            for (int t = 0; t < 16; ++t)
#pragma unroll
                for (int nb = 0; nb < NNB; ++nb) dw[nb][kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(dz[nb][t], xv[t], dw[nb][kb], 0, 0, 0);
        }
        if (any_dx) {
            // dx[row][k] = sum_n dz[row][n] W[n][k]: dz through the wave's tile to get the row on the lane
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int nb = 0; nb < NNB; ++nb)
#pragma unroll
                for (int i = 0; i < 16; ++i) dzs[mfma32_row(i, hf) * RL_DZS + 32 * nb + l31] = dz[nb][i];
            __builtin_amdgcn_wave_barrier();
            const int steps = 8 * ((a.N + 15) >> 4);     // n = 8 (t / 4) + 4 hf + t % 4, zero columns pad to 16
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                if (a.dx[kb] == nullptr) continue;
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                for (int t = 0; t < steps; ++t) {
                    const int n = 8 * (t >> 2) + 4 * hf + (t & 3);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dzs[l31 * RL_DZS + n], ws[n * WS + 32 * kb + l31], acc, 0, 0, 0);
                }
                const int col = a.c0[kb] + l31;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t row = row0 + mfma32_row(r, hf);
                    if (row < kend && col < a.K[kb]) a.dx[kb][row * a.K[kb] + col] = acc[r];
                }
            }
        }
    }
    // this split's partial row, in dW's own layout [N][Ktot]
    float* pw = part_w + (int64_t)sp * a.N * a.Ktot;
#pragma unroll
    for (int nb = 0; nb < NNB; ++nb)
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            const bool colok = a.c0[kb] + l31 < a.K[kb];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = 32 * nb + mfma32_row(r, hf);
                if (n < a.N && colok) pw[n * a.Ktot + a.w0[kb] + l31] = dw[nb][kb][r];
            }
        }
}

// the block grid of a call: NNB output blocks, NKB input blocks; false when the shapes are outside the kernels' set
bool plan(const int* ks, int nin, int N, int* nnb, int* nkb) {
    if (!ks || nin < 1 || nin > RL_MAXIN || N < 1 || N > 64) return false;
    int kb = 0;
    for (int i = 0; i < nin; ++i) {
        if (ks[i] < 1 || ks[i] > 64) return false;
        kb += (ks[i] + 31) / 32;
    }
    *nnb = (N + 31) / 32;
    *nkb = kb;
    return kb <= RL_MAXKB && *nnb * kb <= 4;
}

int fill_args(RlArgs& a, const float* const* xs, float* const* dxs, const int* ks, int nin, const float* W, const float* b, int64_t M,
              int N, int relu) {
    int kb = 0, w0 = 0;
    for (int i = 0; i < nin; ++i) {
        for (int c0 = 0; c0 < ks[i]; c0 += 32, ++kb) {
            a.x[kb] = xs[i]; a.dx[kb] = dxs ? dxs[i] : nullptr; a.K[kb] = ks[i]; a.c0[kb] = c0; a.w0[kb] = w0 + c0;
        }
        w0 += ks[i];
    }
    for (; kb < RL_MAXKB; ++kb) { a.x[kb] = nullptr; a.dx[kb] = nullptr; a.K[kb] = 0; a.c0[kb] = 0; a.w0[kb] = 0; }
    a.W = W; a.b = b; a.M = M; a.N = N; a.Ktot = w0; a.relu = relu;
    return w0;
}

// the row ranges of the backward: dW's split-K plan (gemm.hip) and gaot_colsum's chunks
struct RlPlan { int splits, lanes; int64_t kps; int chunks; int64_t rpc; };
RlPlan rl_plan(int64_t M, int N) {
    RlPlan p;
    // gaot_gemm planned one product per input, dW_i [N][K_i]: with N <= 64 and K_i <= 64 each is ONE output tile whatever K_i is, and
    // the plan and its lane count (N * K_i <= 4 096) then depend on the row count alone -- 64 stands for every admissible K_i
    gaot_gemm_dw_plan(N, 64, M, &p.splits, &p.kps, &p.lanes);
    p.chunks = (int)std::min<int64_t>(256, std::max<int64_t>(1, ceil_div(M, 64)));
    p.rpc = ceil_div(M, p.chunks);
    return p;
}

int rl_grid(int64_t M) { return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(M, RL_ROWS), RL_GRID_CAP)); }

#define RL_DISPATCH(KERNEL, ...)                                                                                    \
    switch (nnb * 8 + nkb) {                                                                                         \
        case 9: GAOT_KLAUNCH((KERNEL<1, 1>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                      \
        case 10: GAOT_KLAUNCH((KERNEL<1, 2>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                     \
        case 11: GAOT_KLAUNCH((KERNEL<1, 3>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                     \
        case 12: GAOT_KLAUNCH((KERNEL<1, 4>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                     \
        case 17: GAOT_KLAUNCH((KERNEL<2, 1>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                     \
        case 18: GAOT_KLAUNCH((KERNEL<2, 2>), dim3(grid), dim3(256), 0, st, __VA_ARGS__); break;                     \
        default: return GAOT_ERR_UNSUPPORTED;                                                                        \
    }

}  // namespace

extern "C" int gaot_rowlin_supported(const int* ks, int nin, int N) {
    int nnb, nkb;
    return plan(ks, nin, N, &nnb, &nkb) ? 1 : 0;
}

extern "C" int gaot_rowlin_plan(int64_t M, int N, int* w_parts, int* w_lanes, int* b_parts) {
    GAOT_CHECK_ARG(M >= 1 && N >= 1 && N <= 64 && w_parts && w_lanes && b_parts, "bad size or null pointer");
    const RlPlan p = rl_plan(M, N);
    *w_parts = p.splits; *w_lanes = p.lanes; *b_parts = p.chunks;
    return GAOT_OK;
}

extern "C" int gaot_rowlin_fwd(const float* const* xs, const int* ks, int nin, const float* W, const float* b, int64_t M, int N, int relu,
                               float* y, gaot_stream_t stream) {
    GAOT_ENTER();
    int nnb, nkb;
    if (!plan(ks, nin, N, &nnb, &nkb)) {
        gaot_set_error("gaot_rowlin_fwd: 1..4 inputs of 1..64 columns, N <= 64 and at most 4 blocks of 32 x 32 weights are supported");
        return GAOT_ERR_UNSUPPORTED;
    }
    GAOT_CHECK_ARG(M >= 0, "negative size");
    GAOT_CHECK_ARG(!relu || nin == 1, "ReLU is supported for one input only (the GEMM chain it stands in for has no activation)");
    if (M == 0) return GAOT_OK;
    GAOT_CHECK_ARG(xs && W && y, "null pointer");
    for (int i = 0; i < nin; ++i) GAOT_CHECK_ARG(xs[i], "null input");
    RlArgs a;
    fill_args(a, xs, nullptr, ks, nin, W, b, M, N, relu);
    hipStream_t st = (hipStream_t)stream;
    const int grid = rl_grid(M);
    RL_DISPATCH(k_rowlin_fwd, a, y);
    GAOT_LAUNCH_CHECK();
    return GAOT_OK;
}

extern "C" int gaot_rowlin_bwd(const float* const* xs, const int* ks, int nin, const float* W, const float* dy, const float* y, int64_t M,
                               int N, int relu, float* const* dxs, float* dw_part, float* db_part, gaot_stream_t stream) {
    GAOT_ENTER();
    int nnb, nkb;
    if (!plan(ks, nin, N, &nnb, &nkb)) {
        gaot_set_error("gaot_rowlin_bwd: 1..4 inputs of 1..64 columns, N <= 64 and at most 4 blocks of 32 x 32 weights are supported");
        return GAOT_ERR_UNSUPPORTED;
    }
    GAOT_CHECK_ARG(M > 0, "no rows (the caller returns zero gradients)");
    GAOT_CHECK_ARG(!relu || nin == 1, "ReLU is supported for one input only");
    GAOT_CHECK_ARG(xs && W && dy && dw_part && db_part && (!relu || y), "null pointer");
    for (int i = 0; i < nin; ++i) GAOT_CHECK_ARG(xs[i], "null input");
    RlArgs a;
    fill_args(a, xs, dxs, ks, nin, W, nullptr, M, N, relu);
    hipStream_t st = (hipStream_t)stream;
    const RlPlan p = rl_plan(M, N);
    const int nsw = (p.splits + 3) / 4, grid = nsw + p.chunks;
    RL_DISPATCH(k_rowlin_bwd, a, dy, y, dw_part, db_part, p.splits, p.kps, nsw, p.rpc);
    GAOT_LAUNCH_CHECK();
    return GAOT_OK;
}
