// The ADJOINT of the fused GNO forward WITH its spatial derivative (gaot_gno_fwd_knn_jac / gaot_gno_fwd_jac, gno_jac.hip) with respect
// to f_y, for the 'linear' transform: both the value and the three tangent planes are linear in f_y,
//     out_q   = (1/deg q) sum_{e -> q} K(y_t, x_q)     * f[t]
//     jac_q^d = (1/deg q) sum_{e -> q} d_d K(y_t, x_q) * f[t]          d = 0, 1, 2
// so for cotangents G on out and J_d on jac^d
//     df[t] = sum_{e: src = t} ( K_e * G[q_e] + sum_d d_d K_e * J_d[q_e] ) / deg(q_e)
// -- the per-edge work of the tangent kernel (value plus three tangent chains through the kernel MLP, forward mode), the four planes
// contracted with four gathered cotangent rows into ONE plane, reduced by TOKEN as gaot_gno_adj reduces it.  No MLP backward, no
// weight gradients, no atomics.  The three directions cannot be collapsed into one tangent: J_d differs per channel.
//
// The tile loop is k_gno_fwd_knn_jac's (weights transposed in LDS, layer 0 with gelu'(z_0) * W_0[:, 3+d], hidden layers value then
// one direction at a time, the last layer transposed so that channels land on lanes) on the SOURCE-sorted lists of gaot_gno_adj:
// src_s = the token (the row of y_pos and the segment key), dst_s = the query (the row of x_pos and of the cotangents).  In the
// epilogue a lane gathers G[q][c] and J_d[q][c] for its 16 accumulator rows and accumulates plane by plane into one register tile --
// the value term first, then one fma per direction d = 0, 1, 2 --, multiplies by 1/deg(q) (from rowptr_dst; the constant 1/k of a
// regular list when it is null) and stages ONE [32][32] plane per wave.  segment_walk<32>(sum) with two partial slots per tile and
// k_segment_fixup<32> in tile order finish the rows: a fixed summation order, bit-reproducible run to run, and exact zeros for
// tokens without edges.  Exact fp32 (v_mfma_f32_32x32x2_f32) whatever the library's precision mode.
//
// LDS: up to 59.1 KiB of weights, 4 KiB of staging and 256 bytes of ids per wave: 76.1 KiB at four hidden layers, so by LDS two
// workgroups fit a CU's 160 KiB where the tangent kernel (16 KiB of staging per wave) fits one.  By registers they do not: value, three
// tangents, gelu' and the next accumulators are the tangent kernel's 224+ registers, and bounded to 256 (two waves per SIMD) the
// instantiations with three and four hidden layers spill 204 / 272 bytes per lane to scratch.  So: one workgroup per CU
// (__launch_bounds__(256, 1)), no scratch in any instantiation (profiles/gno_adj_jac_isa_equal.txt).
#include "gno_common.h"

namespace {

using namespace gno;

constexpr int H = 64, C = 32, KB = H / 32;

template <int NH>
struct AdjJacLds {
    static constexpr int w0 = 0;                                 // [IN0P][H]
    static constexpr int b0 = w0 + IN0P * H;                     // [H]
    static constexpr int wl = b0 + H;                            // (NH-1) x ([H][H] + [H])
    static constexpr int wL = wl + (NH - 1) * (H * H + H);       // [H][32]
    static constexpr int bL = wL + H * C;                        // [32]
    static constexpr int weights_end = bL + C;
    static constexpr int stage = weights_end;                    // [4 waves][32][C]
    static constexpr int ids = stage + 4 * 32 * C;               // [4 waves][2][32] (int): the edges' queries, then their tokens
    static constexpr size_t bytes = sizeof(float) * (size_t)(ids + 4 * 2 * 32);
};

constexpr int WG_PER_CU = 1;

template <int NH>
__global__ __launch_bounds__(256, WG_PER_CU) void k_gno_adj_jac(MlpPtrs mlp, const float* __restrict__ y_pos,
                                                                const float* __restrict__ x_pos, const float* __restrict__ gout,
                                                                const float* __restrict__ gjac, int64_t plane,
                                                                const int* __restrict__ src_s, const int* __restrict__ dst_s,
                                                                const int* __restrict__ rowptr_src, const int* __restrict__ rowptr_dst,
                                                                float inv_k, int64_t E, float* __restrict__ grad_f,
                                                                float* __restrict__ part) {
    using L = AdjJacLds<NH>;
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
    float* stage = lds + L::stage + wave * (32 * C);
    int* qids = (int*)(lds + L::ids) + wave * (2 * 32);
    int* tids = qids + 32;

    const int64_t n_tiles = (E + 31) / 32;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t base = tile * 32;
        // MLP input k = 2i+hf of this lane's edge: [y.x y.y y.z x.x x.y x.z][2i+hf], i = 0..2 (edges past E: rows 0, valid rows)
        float bin[3];
        float aw;   // 1 / deg(q) of this lane's edge (edges past E: 0)
        {
            const int64_t e = base + l31;
            const bool valid = e < E;
            const int s = valid ? src_s[e] : 0;
            const int q = valid ? dst_s[e] : 0;
            const float* ys = y_pos + (int64_t)s * 3;
            const float* xq = x_pos + (int64_t)q * 3;
            bin[0] = ys[hf];
            bin[1] = hf ? xq[0] : ys[2];
            bin[2] = xq[1 + hf];
            aw = !valid ? 0.f : (rowptr_dst ? 1.0f / (float)(rowptr_dst[q + 1] - rowptr_dst[q]) : inv_k);
            if (hf == 0) {   // the rows gathered are the query's, the segment key the token
                qids[l31] = q;
                tids[l31] = valid ? s : -1;
            }
        }
        // ---- layer 0: 6 -> H; the tangent of direction d is gelu'(z_0) times column 3+d of W_0 ------------
        f32x16 h[KB], hd[3][KB];
#pragma unroll
        for (int ob = 0; ob < KB; ++ob) {
            f32x16 z;
#pragma unroll
            for (int r = 0; r < 16; ++r) z[r] = lds[L::b0 + 32 * ob + mfma32_row(r, hf)];
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
        // ---- last layer, transposed: K'[e][c] = sum_k Hlast[k][e] * WL[c][k] (+ bL[c] on the value plane), contracted plane by
        // plane with the gathered cotangent rows: o[e][c] = K[e][c] G[q_e][c], then += d_d K[e][c] J_d[q_e][c] for d = 0, 1, 2 ----
        wave_lds_fence();  // ids visible to the whole wave
        int64_t grow[16];  // the cotangent row of accumulator row r: q * 32 + c
#pragma unroll
        for (int r = 0; r < 16; ++r) grow[r] = (int64_t)qids[mfma32_row(r, hf)] * C + l31;
        f32x16 o;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float* gp = p == 0 ? gout : gjac + (int64_t)(p - 1) * plane;
            float gv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) gv[r] = gp[grow[r]];
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
            for (int r = 0; r < 16; ++r) o[r] = p == 0 ? acc[r] * gv[r] : fmaf(acc[r], gv[r], o[r]);
        }
        // 1 / deg(q): lane el holds edge el of the tile, el = mfma32_row(r, 0) + 4 hf: two scalar reads and a select (as AdjFwd)
        const int wa = __builtin_bit_cast(int, aw);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int a0 = __builtin_amdgcn_readlane(wa, mfma32_row(r, 0)), a1 = __builtin_amdgcn_readlane(wa, mfma32_row(r, 0) + 4);
            stage[mfma32_row(r, hf) * C + l31] = o[r] * __builtin_bit_cast(float, hf ? a1 : a0);
        }
        wave_lds_fence();
        // ---- sums by token: the lower half walks the tile, lane = channel ------------------------------------
        if (hf == 0) segment_walk<C>(stage, C, tids, l31, base, rowptr_src, grad_f, part, false);
        wave_lds_fence();
    }
}

template <int NH>
int launch_adj_jac(const MlpPtrs& p, const float* y_pos, const float* x_pos, const float* gout, const float* gjac, int64_t plane,
                   const int* src_s, const int* dst_s, const int* rowptr_src, const int* rowptr_dst, float inv_k, int64_t E,
                   float* grad_f, float* part, hipStream_t st) {
    constexpr size_t lds = AdjJacLds<NH>::bytes;
    auto kern = k_gno_adj_jac<NH>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
        gaot_set_error("gaot_gno_adj_jac: cannot set dynamic LDS %zu: %s", lds, hipGetErrorString(e));
        return GAOT_ERR_LAUNCH;
    }
    const int64_t n_tiles = ceil_div(E, 32);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n_tiles, 4), 256 * WG_PER_CU));
    GAOT_KLAUNCH(kern, dim3(grid), dim3(256), lds, st, p, y_pos, x_pos, gout, gjac, plane, src_s, dst_s, rowptr_src, rowptr_dst, inv_k,
                 E, grad_f, part);
    return GAOT_OK;
}

}  // namespace

// two 32-float slots per 32-edge tile, as gaot_gno_adj
extern "C" size_t gaot_gno_adj_jac_workspace_bytes(int64_t num_edges) { return gaot_gno_adj_workspace_bytes(num_edges, C); }

extern "C" int gaot_gno_adj_jac(const gaot_mlp_t* mlp, const float* y_pos, const float* x_pos, const float* grad_out,
                                const float* grad_jac, const int32_t* rowptr_dst, int k, const int32_t* src_sorted,
                                const int32_t* dst_sorted, const int32_t* rowptr_src, int64_t num_edges, int64_t num_sources,
                                int64_t num_queries, float* grad_f_y, void* workspace, size_t workspace_bytes, gaot_stream_t stream) {
    GAOT_ENTER();
    GAOT_CHECK_ARG(mlp, "null mlp");
    if (!(mlp->channels == C && mlp->hidden == H && mlp->n_hidden >= 1 && mlp->n_hidden <= 4)) {
        gaot_set_error("gaot_gno_adj_jac: unsupported MLP shape (n_hidden=%d hidden=%d channels=%d)", mlp->n_hidden, mlp->hidden,
                       mlp->channels);
        return GAOT_ERR_UNSUPPORTED;
    }
    GAOT_CHECK_ARG(num_edges >= 0 && num_sources >= 0 && num_queries >= 0, "negative size");
    GAOT_CHECK_ARG(num_edges <= (int64_t)INT32_MAX, "num_edges beyond int32 (take the queries in chunks)");
    GAOT_CHECK_ARG(rowptr_dst || k > 0, "null rowptr_dst needs k > 0 (the degree of every query of a regular list)");
    GAOT_CHECK_ARG(rowptr_dst || num_edges == num_queries * (int64_t)k, "a regular list holds num_queries * k edges");
    GAOT_CHECK_ARG(rowptr_src && (num_sources == 0 || grad_f_y), "null pointer");
    GAOT_CHECK_ARG(workspace_bytes >= gaot_gno_adj_jac_workspace_bytes(num_edges) && (workspace || num_edges == 0),
                   "workspace too small");
    MlpPtrs p;
    for (int l = 0; l <= mlp->n_hidden; ++l) {
        p.w[l] = mlp->weight[l];
        p.b[l] = mlp->bias[l];
        GAOT_CHECK_ARG(p.w[l] && p.b[l], "null MLP parameter");
    }
    if (num_edges > 0) {
        GAOT_CHECK_ARG(y_pos && x_pos && grad_out && src_sorted && dst_sorted, "null pointer");
        GAOT_CHECK_ARG(grad_jac, "null grad_jac (the cotangent of the three tangent planes, [3][num_queries][32])");
        GAOT_CHECK_ARG(num_queries > 0, "edges without queries");
    }
    if (num_sources == 0) return GAOT_OK;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    if (num_edges > 0) {
        const float inv_k = rowptr_dst ? 0.f : 1.0f / (float)k;
        const int64_t plane = num_queries * C;
        int rc = GAOT_OK;
#define GNO_ADJ_JAC_CASE(NH_)                                                                                                      \
    case NH_:                                                                                                                      \
        rc = launch_adj_jac<NH_>(p, y_pos, x_pos, grad_out, grad_jac, plane, src_sorted, dst_sorted, rowptr_src, rowptr_dst, inv_k, \
                                 num_edges, grad_f_y, part, st);                                                                   \
        break;
        switch (mlp->n_hidden) {
            GNO_ADJ_JAC_CASE(1) GNO_ADJ_JAC_CASE(2) GNO_ADJ_JAC_CASE(3) GNO_ADJ_JAC_CASE(4)
        }
#undef GNO_ADJ_JAC_CASE
        if (rc != GAOT_OK) return rc;
    }
    // tokens without edges -> 0 and the rows that straddle tiles, in tile order (num_edges == 0: this launch alone)
    GAOT_KLAUNCH((k_segment_fixup<32>), dim3(segment_fixup_grid(num_sources * 8)), dim3(256), 0, st, rowptr_src, num_sources, part,
                 grad_f_y, 0);
    GAOT_LAUNCH_CHECK();
    return GAOT_OK;
}
