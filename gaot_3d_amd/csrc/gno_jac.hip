// The fused GNO forward on a regular k-neighbour list WITH its spatial derivative: one launch writes the transform's value and
// its Jacobian with respect to the query coordinate (gaot_gno_fwd_knn_jac), in forward mode.
//
// With a query's neighbour list held fixed only the three query columns of the kernel MLP's first layer see x_q, so the derivative
// is three tangent vectors carried through the per-edge MLP beside the value and reduced by the same fixed-k row sums:
//     z_0 = W_0 [y_s ; x_q] + b_0 (+ t[s]),   h_0 = gelu(z_0),   dh_0^d = gelu'(z_0) * W_0[:, 3+d]        (no matrix product)
//     z_l = W_l h_{l-1} + b_l,                h_l = gelu(z_l),   dh_l^d = gelu'(z_l) * (W_l dh_{l-1}^d)
//     k   = W_L h_{NH-1} + b_L,                                  dk^d   = W_L dh_{NH-1}^d
//     out_q = (1/k) sum_e k_e * f[s_e],       jac_q^d = (1/k) sum_e dk_e^d * f[s_e]                       (kernel-only: without f)
// Nothing is stored between layers and no backward runs.
//
// The kernel is k_gno_fwd with a KnnFwd list (gno.hip) at T = 1: edges on the MFMA lane axis, weights transposed in LDS, the last
// layer transposed so that channels land on lanes, fixed_k_rows finishing the rows in the tile -- here once per plane (value, d/dx,
// d/dy, d/dz).  Exact fp32 (v_mfma_f32_32x32x2_f32) whatever the library's precision mode.  The VALUE plane performs gaot_gno_fwd_knn's
// precision-0 operations in its order (same products, gelu_fast's expression), so the two agree bit for bit.
//
// Registers: one 64-wide layer of a 32-edge tile is 32 VGPRs per lane; value + three tangents are 128, gelu'(z_l) 32 more, the next
// layer's accumulators 32.  gelu' is held once per layer and the next layer's tangents are produced one direction at a time (each
// overwrites its input when its 32 accumulators are complete).  One workgroup per CU (__launch_bounds__(256, 1)): the LDS holds up
// to 59.1 KiB of weights plus a 4-plane staging tile of 16 KiB per wave (123.6 KiB of 160 at four hidden layers).  No scratch, no
// atomics, plain vector stores only.
#include "gno_common.h"

namespace {

using namespace gno;

constexpr int H = 64, C = 32, KB = H / 32, NP = 4;   // planes: value, d/dx, d/dy, d/dz

template <int NH>
struct JacLds {
    static constexpr int w0 = 0;                                 // [IN0P][H]
    static constexpr int b0 = w0 + IN0P * H;                     // [H]
    static constexpr int wl = b0 + H;                            // (NH-1) x ([H][H] + [H])
    static constexpr int wL = wl + (NH - 1) * (H * H + H);       // [H][32]
    static constexpr int bL = wL + H * C;                        // [32]
    static constexpr int weights_end = bL + C;
    static constexpr int stage = weights_end;                    // [4 waves][NP][32][C]
    static constexpr int ids = stage + 4 * NP * 32 * C;          // [4 waves][32] (int)
    static constexpr size_t bytes = sizeof(float) * (size_t)(ids + 4 * 32);
};

// gelu_fast's value (its own expression: bit-identical) and gelu_fast_pair's derivative; t, p, e are shared
__device__ __forceinline__ void gelu_fast_tangent(float x, float& g, float& dg) {
    const float u = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, u, 1.0f));
    const float e = __builtin_amdgcn_exp2f(-0.72134752044448170368f * x * x);
    float p = fmaf(t, 0.5f * 1.061405429f, 0.5f * -1.453152027f);
    p = fmaf(t, p, 0.5f * 1.421413741f);
    p = fmaf(t, p, 0.5f * -0.284496736f);
    p = fmaf(t, p, 0.5f * 0.254829592f);
    const float h = t * p * e;                    // Phi(-|x|)
    g = fmaf(-fabsf(x), h, fmaxf(x, 0.f));
    const float cdf = x >= 0.f ? 1.0f - h : h;
    dg = fmaf(x * e, 0.39894228040143267794f, cdf);
}

template <int NH, int MODE>
__global__ __launch_bounds__(256, 1) void k_gno_fwd_knn_jac(MlpPtrs mlp, const float* __restrict__ y_pos,
                                                            const float* __restrict__ x_pos, const float* __restrict__ f_y,
                                                            const float* __restrict__ ttab, const int* __restrict__ nbr, int lk,
                                                            int64_t E, float* __restrict__ out, float* __restrict__ jac) {
    using L = JacLds<NH>;
    extern __shared__ __attribute__((aligned(16))) float lds[];

    // ---- weights -> LDS, transposed to [in][out] (k_gno_fwd's image) ---------------------------------
    for (int i = threadIdx.x; i < IN0P * H; i += 256) {
        const int k = i / H, j = i % H;
        lds[L::w0 + i] = (k < IN0) ? mlp.w[0][j * IN0 + k] : 0.f;
    }
    for (int i = threadIdx.x; i < H; i += 256) lds[L::b0 + i] = mlp.b[0][i];
#pragma unroll
    for (int l = 1; l < NH; ++l) {
        float* wt = lds + L::wl + (l - 1) * (H * H + H);
        for (int i = threadIdx.x; i < H * H; i += 256) {
            const int j = i / H, k = i % H;
            wt[k * H + j] = mlp.w[l][i];
        }
        for (int i = threadIdx.x; i < H; i += 256) wt[H * H + i] = mlp.b[l][i];
    }
    for (int i = threadIdx.x; i < C * H; i += 256) {
        const int c = i / H, k = i % H;
        lds[L::wL + k * C + c] = mlp.w[NH][i];
    }
    for (int i = threadIdx.x; i < C; i += 256) lds[L::bL + i] = mlp.b[NH][i];
    __syncthreads();

    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int l31 = lane & 31, hf = lane >> 5;
    float* stage = lds + L::stage + wave * (NP * 32 * C);
    int* ids = (int*)(lds + L::ids) + wave * 32;
    const int64_t plane = (E >> lk) * C;   // one [Nq][32] plane of jac

    const int64_t n_tiles = (E + 31) / 32;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t base = tile * 32;
        // MLP input k = 2i+hf of this lane's edge: [y.x y.y y.z x.x x.y x.z][2i+hf], i = 0..2 (edges past E: row 0, a valid row)
        float bin[3];
        int sid;
        {
            const int64_t e = base + l31;
            const bool valid = e < E;
            sid = valid ? nbr[e] : 0;
            const int q = valid ? (int)(e >> lk) : 0;
            const float* ys = y_pos + (int64_t)sid * 3;
            const float* xq = x_pos + (int64_t)q * 3;
            bin[0] = ys[hf];
            bin[1] = hf ? xq[0] : ys[2];
            bin[2] = xq[1 + hf];
            if (hf == 0) ids[l31] = sid;
        }
        // ---- layer 0: 6 -> H; the tangent of direction d is gelu'(z_0) times column 3+d of W_0 ------------
        f32x16 h[KB], hd[3][KB];
#pragma unroll
        for (int ob = 0; ob < KB; ++ob) {
            f32x16 z;
#pragma unroll
            for (int r = 0; r < 16; ++r) z[r] = lds[L::b0 + 32 * ob + mfma32_row(r, hf)];
            if constexpr (MODE != MODE_LINEAR) {
                const float* tr = ttab + (int64_t)sid * NLH + 32 * ob + 4 * hf;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 v = *reinterpret_cast<const float4*>(tr + 8 * j);
                    z[4 * j + 0] += v.x;
                    z[4 * j + 1] += v.y;
                    z[4 * j + 2] += v.z;
                    z[4 * j + 3] += v.w;
                }
            }
#pragma unroll
            for (int i = 0; i < IN0 / 2; ++i) {
                const float a = lds[L::w0 + (2 * i + hf) * H + 32 * ob + l31];
                z = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bin[i], z, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float g, dg;
                gelu_fast_tangent(z[r], g, dg);
                h[ob][r] = g;
                const int j = 32 * ob + mfma32_row(r, hf);
#pragma unroll
                for (int d = 0; d < 3; ++d) hd[d][ob][r] = dg * lds[L::w0 + (3 + d) * H + j];
            }
        }
        // ---- hidden layers H -> H: the value, gelu' once, then one direction at a time -------------------
#pragma unroll
        for (int l = 1; l < NH; ++l) {
            const float* wt = lds + L::wl + (l - 1) * (H * H + H);
            f32x16 zn[KB];
#pragma unroll
            for (int ob = 0; ob < KB; ++ob) {
#pragma unroll
                for (int r = 0; r < 16; ++r) zn[ob][r] = wt[H * H + 32 * ob + mfma32_row(r, hf)];
#pragma unroll
                for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float a = wt[(32 * kb + mfma32_row(r, hf)) * H + 32 * ob + l31];
                        zn[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, h[kb][r], zn[ob], 0, 0, 0);
                    }
            }
            f32x16 dg[KB];
#pragma unroll
            for (int ob = 0; ob < KB; ++ob)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float g, d;
                    gelu_fast_tangent(zn[ob][r], g, d);
                    h[ob][r] = g;
                    dg[ob][r] = d;
                }
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                f32x16 u[KB];
#pragma unroll
                for (int ob = 0; ob < KB; ++ob) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) u[ob][r] = 0.f;
#pragma unroll
                    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float a = wt[(32 * kb + mfma32_row(r, hf)) * H + 32 * ob + l31];
                            u[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, hd[d][kb][r], u[ob], 0, 0, 0);
                        }
                }
#pragma unroll
                for (int ob = 0; ob < KB; ++ob)
#pragma unroll
                    for (int r = 0; r < 16; ++r) hd[d][ob][r] = dg[ob][r] * u[ob][r];
            }
        }
        // ---- last layer, transposed: K'[e][c] = sum_k Hlast[k][e] * WL[c][k] (+ bL[c] on the value plane) ----
        wave_lds_fence();  // ids visible to the whole wave
        [[maybe_unused]] float fv[16];
        if constexpr (MODE != MODE_KERNELONLY) {
#pragma unroll
            for (int r = 0; r < 16; ++r) fv[r] = f_y[(int64_t)ids[mfma32_row(r, hf)] * C + l31];
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            f32x16 acc;
            const float bl = p == 0 ? lds[L::bL + l31] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = bl;
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float b = lds[L::wL + (32 * kb + mfma32_row(r, hf)) * C + l31];
                    const float a = p == 0 ? h[kb][r] : hd[p == 0 ? 0 : p - 1][kb][r];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
                }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int el = mfma32_row(r, hf);
                if constexpr (MODE == MODE_KERNELONLY) stage[(p * 32 + el) * C + l31] = acc[r];
                else stage[(p * 32 + el) * C + l31] = acc[r] * fv[r];
            }
        }
        wave_lds_fence();
        // ---- fixed-k row means: half 0 finishes the value and d/dx, half 1 d/dy and d/dz -------------------
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = 2 * hf + i;
            float* dst = p == 0 ? out : jac + (int64_t)(p - 1) * plane;
            fixed_k_rows<C>(stage + p * 32 * C, C, l31, base, lk, E, dst);
        }
        wave_lds_fence();
    }
}

template <int NH, int MODE>
int launch_jac(const MlpPtrs& p, const float* y_pos, const float* x_pos, const float* f_y, const float* ttab, const int* nbr, int lk,
               int64_t E, float* out, float* jac, hipStream_t st) {
    constexpr size_t lds = JacLds<NH>::bytes;
    auto kern = k_gno_fwd_knn_jac<NH, MODE>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
        gaot_set_error("gaot_gno_fwd_knn_jac: cannot set dynamic LDS %zu: %s", lds, hipGetErrorString(e));
        return GAOT_ERR_LAUNCH;
    }
    const int64_t n_tiles = ceil_div(E, 32);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n_tiles, 4), 256));   // one workgroup per CU
    GAOT_KLAUNCH(kern, dim3(grid), dim3(256), lds, st, p, y_pos, x_pos, f_y, ttab, nbr, lk, E, out, jac);
    return GAOT_OK;
}

}  // namespace

extern "C" int gaot_gno_fwd_knn_jac(const gaot_mlp_t* mlp, int mode, const float* y_pos, const float* x_pos, const float* f_y,
                                    const float* src_table, const int32_t* nbr, int k, int64_t num_queries, float* out, float* jac,
                                    gaot_stream_t stream) {
    GAOT_ENTER();
    GAOT_CHECK_ARG(mlp, "null mlp");
    if (!(mlp->channels == C && mlp->hidden == H && mlp->n_hidden >= 1 && mlp->n_hidden <= 4)) {
        gaot_set_error("gaot_gno_fwd_knn_jac: unsupported MLP shape (n_hidden=%d hidden=%d channels=%d)", mlp->n_hidden, mlp->hidden,
                       mlp->channels);
        return GAOT_ERR_UNSUPPORTED;
    }
    GAOT_CHECK_ARG(mode == MODE_LINEAR || mode == MODE_NONLINEAR || mode == MODE_KERNELONLY,
                   "mode must be 0 (linear), 1 (nonlinear) or 2 (nonlinear_kernelonly)");
    GAOT_CHECK_ARG(k == 1 || k == 2 || k == 4 || k == 8 || k == 16 || k == 32, "k must be 1, 2, 4, 8, 16 or 32 (a divisor of the 32-edge tile)");
    GAOT_CHECK_ARG(num_queries >= 0, "negative size");
    GAOT_CHECK_ARG(num_queries <= (int64_t)INT32_MAX / k, "num_queries * k beyond int32 (sample the queries in chunks)");
    GAOT_CHECK_ARG(y_pos && x_pos && nbr && out && jac && (f_y || mode == MODE_KERNELONLY), "null pointer");
    GAOT_CHECK_ARG(mode == MODE_LINEAR || src_table, "null src_table");
    MlpPtrs p;
    for (int l = 0; l <= mlp->n_hidden; ++l) {
        p.w[l] = mlp->weight[l];
        p.b[l] = mlp->bias[l];
        GAOT_CHECK_ARG(p.w[l] && p.b[l], "null MLP parameter");
    }
    if (num_queries == 0) return GAOT_OK;
    hipStream_t st = (hipStream_t)stream;
    const int lk = __builtin_ctz((unsigned)k);
    const int64_t num_edges = num_queries * k;
    int rc = GAOT_OK;
#define GNO_JAC_CASE(NH_, MODE_)                                                                                 \
    case NH_ * 3 + MODE_:                                                                                        \
        rc = launch_jac<NH_, MODE_>(p, y_pos, x_pos, f_y, src_table, nbr, lk, num_edges, out, jac, st);          \
        break;
#define GNO_JAC_CASES(NH_) GNO_JAC_CASE(NH_, MODE_LINEAR) GNO_JAC_CASE(NH_, MODE_NONLINEAR) GNO_JAC_CASE(NH_, MODE_KERNELONLY)
    switch (mlp->n_hidden * 3 + mode) {
        GNO_JAC_CASES(1) GNO_JAC_CASES(2) GNO_JAC_CASES(3) GNO_JAC_CASES(4)
    }
#undef GNO_JAC_CASES
#undef GNO_JAC_CASE
    if (rc != GAOT_OK) return rc;
    GAOT_LAUNCH_CHECK();
    return GAOT_OK;
}
