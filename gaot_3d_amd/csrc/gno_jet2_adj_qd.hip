// gaot_gno_adj_jet2 (gno_jet2_adj.hip) with PER-QUERY directions: the adjoint of gaot_gno_fwd_knn_jet2_qd / gaot_gno_fwd_jet2_qd
// (mode 0) with respect to f_y.  `dirs` is a DEVICE array [num_queries][nd][3], 1 <= nd <= 6, read by the kernel:
//     df[t] = sum_{e: src = t} ( K_e * G[q_e] + sum_i D_{v_i(q_e)} K_e * P_i[q_e] + sum_i D^2_{v_i(q_e)} K_e * S_i[q_e] ) / deg(q_e)
// -- what a second derivative along a query's own direction (a wall normal, a local frame) pulls back into the latent.
//
// The body is k_gno_adjqd_jet2's, statement by statement, COPIED here (so that the four host-direction kernels are not rebuilt from
// changed text) with ONE difference: edges sit on the lane axis -- hd[ob][r] is [hidden row][edge = lane & 31] -- so at the top of
// direction pass d a lane loads the three components of direction d of ITS OWN edge's query (the query it wrote to `qids`; an edge
// past E: direction 0) and forms z'_0 with the same fixed-order chain fma(v_z, w_5, fma(v_y, w_4, v_x w_3)) from per-lane instead
// of uniform values.  With the same directions on every query the result is gaot_gno_adj_jet2's bit for bit.  The three components
// are dead after the first layer's z'_0: nothing direction-dependent is held across the layer loop.  Value path, KEEP rule, gather
// order (G, P_0, S_0, P_1, S_1, ...), 1/deg staging, segment_walk<32> and k_segment_fixup<32>: unchanged.  Exact fp32
// (v_mfma_f32_32x32x2_f32) whatever the precision mode, no atomics, bit-reproducible, exact zeros for tokens without edges.
#include "gno_common.h"

namespace {

using namespace gno;

constexpr int H = 64, C = 32, KB = H / 32, MAXD = 6;

template <int NH>
struct AdjJet2Lds {
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

// opaque() and the activation jet gelu_fast_jet2(): gno_common.h

constexpr int WG_PER_CU = 1;

template <int NH>
__global__ __launch_bounds__(256, WG_PER_CU) void k_gno_adjqd_jet2(MlpPtrs mlp, const float* __restrict__ y_pos,
                                                                 const float* __restrict__ x_pos, const float* __restrict__ gout,
                                                                 const float* __restrict__ gd1, const float* __restrict__ gd2,
                                                                 int64_t plane, int64_t plane2, const int* __restrict__ src_s,
                                                                 const int* __restrict__ dst_s, const int* __restrict__ rowptr_src,
                                                                 const int* __restrict__ rowptr_dst, float inv_k, int64_t E,
                                                                 const float* __restrict__ qdirs, int nd,
                                                                   float* __restrict__ grad_f,
                                                                 float* __restrict__ part) {
    using L = AdjJet2Lds<NH>;
    // what the value path leaves for the direction passes: gelu' / gelu'' themselves at ONE hidden layer, z_l from two on.  The forward
    // keeps them at two as well; here, with the register tile `o` and the gathered cotangent rows beside a pass, that instantiation
    // spilled 160 bytes per lane.  The same expression on the same z gives the same bits either way.
    constexpr bool KEEP = NH <= 1;
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
        // ---- the value path, once per tile: gelu' and gelu'' of every hidden layer (or z_l) stay in registers -----
        f32x16 h[KB], sa[NH][KB], sb[KEEP ? NH : 1][KB];   // KEEP: gelu'(z_l), gelu''(z_l); else z_l
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
                float g, a, b;
                gelu_fast_jet2(z[r], g, a, b);
                h[ob][r] = g;
                if constexpr (KEEP) {
                    sa[0][ob][r] = a;
                    sb[0][ob][r] = b;
                } else {
                    sa[0][ob][r] = z[r];
                }
            }
        }
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
#pragma unroll
            for (int ob = 0; ob < KB; ++ob)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float g, a, b;
                    gelu_fast_jet2(zn[ob][r], g, a, b);
                    h[ob][r] = g;
                    if constexpr (KEEP) {
                        sa[l][ob][r] = a;
                        sb[l][ob][r] = b;
                    } else {
                        sa[l][ob][r] = zn[ob][r];
                    }
                }
        }
        // ---- last layer, transposed: K[e][c] = sum_k Hlast[k][e] * WL[c][k] + bL[c], contracted with the gathered rows of G ----
        wave_lds_fence();  // ids visible to the whole wave
        f32x16 o;
        {
            float gv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) gv[r] = gout[(int64_t)qids[mfma32_row(r, hf)] * C + l31];
            f32x16 acc;
            const float bl = lds[L::bL + l31];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = bl;
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float b = lds[L::wL + (32 * kb + mfma32_row(r, hf)) * C + l31];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h[kb][r], b, acc, 0, 0, 0);
                }
#pragma unroll
            for (int r = 0; r < 16; ++r) o[r] = acc[r] * gv[r];
        }

        // ---- one pass per direction: h' and h'' through the layers, then o += D_v K * P_d and o += D_v^2 K * S_d ----
#pragma unroll 1
        for (int d = 0; d < nd; ++d) {
            // direction d of this lane's edge's query (an edge past E: 0)
            float vx = 0.f, vy = 0.f, vz = 0.f;
            if (tids[l31] >= 0) {
                const float* v = qdirs + ((int64_t)qids[l31] * nd + d) * 3;
                vx = v[0];
                vy = v[1];
                vz = v[2];
            }
            f32x16 hd[KB], hdd[KB];
#pragma unroll
            for (int ob = 0; ob < KB; ++ob)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = 32 * ob + mfma32_row(r, hf);
                    const float zd = fmaf(vz, lds[L::w0 + 5 * H + j], fmaf(vy, lds[L::w0 + 4 * H + j], vx * lds[L::w0 + 3 * H + j]));
                    float dg, ddg;
                    if constexpr (KEEP) {
                        dg = sa[0][ob][r];
                        ddg = sb[0][ob][r];
                    } else {
                        float g;
                        gelu_fast_jet2(opaque(sa[0][ob][r]), g, dg, ddg);
                    }
                    hd[ob][r] = dg * zd;
                    hdd[ob][r] = ddg * zd * zd;
                }
#pragma unroll
            for (int l = 1; l < NH; ++l) {
                const float* wt = lds + L::wl + (l - 1) * (H * H + H);
                f32x16 u[KB], w[KB];
#pragma unroll
                for (int ob = 0; ob < KB; ++ob) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) u[ob][r] = 0.f;
#pragma unroll
                    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float a = wt[(32 * kb + mfma32_row(r, hf)) * H + 32 * ob + l31];
                            u[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, hd[kb][r], u[ob], 0, 0, 0);
                        }
                }
#pragma unroll
                for (int ob = 0; ob < KB; ++ob) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) w[ob][r] = 0.f;
#pragma unroll
                    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float a = wt[(32 * kb + mfma32_row(r, hf)) * H + 32 * ob + l31];
                            w[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, hdd[kb][r], w[ob], 0, 0, 0);
                        }
                }
#pragma unroll
                for (int ob = 0; ob < KB; ++ob)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float dg, ddg;
                        if constexpr (KEEP) {
                            dg = sa[l][ob][r];
                            ddg = sb[l][ob][r];
                        } else {
                            float g;
                            gelu_fast_jet2(opaque(sa[l][ob][r]), g, dg, ddg);
                        }
                        hd[ob][r] = dg * u[ob][r];
                        hdd[ob][r] = fmaf(dg, w[ob][r], ddg * u[ob][r] * u[ob][r]);
                    }
            }
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const float* gp = p == 0 ? gd1 + (int64_t)d * plane : gd2 + (int64_t)d * plane2;
                float gv[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) gv[r] = gp[(int64_t)qids[mfma32_row(r, hf)] * C + l31];
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
                for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float b = lds[L::wL + (32 * kb + mfma32_row(r, hf)) * C + l31];
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(p == 0 ? hd[kb][r] : hdd[kb][r], b, acc, 0, 0, 0);
                    }
#pragma unroll
                for (int r = 0; r < 16; ++r) o[r] = fmaf(acc[r], gv[r], o[r]);
            }
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
int launch_adjqd_jet2(const MlpPtrs& p, const float* y_pos, const float* x_pos, const float* gout, const float* gd1, const float* gd2,
                    int64_t plane, int64_t plane2, const int* src_s, const int* dst_s, const int* rowptr_src, const int* rowptr_dst,
                    float inv_k, int64_t E, const float* qdirs, int nd, float* grad_f, float* part, hipStream_t st) {
    constexpr size_t lds = AdjJet2Lds<NH>::bytes;
    auto kern = k_gno_adjqd_jet2<NH>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
        gaot_set_error("gaot_gno_adj_jet2_qd: cannot set dynamic LDS %zu: %s", lds, hipGetErrorString(e));
        return GAOT_ERR_LAUNCH;
    }
    const int64_t n_tiles = ceil_div(E, 32);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n_tiles, 4), 256 * WG_PER_CU));
    GAOT_KLAUNCH(kern, dim3(grid), dim3(256), lds, st, p, y_pos, x_pos, gout, gd1, gd2, plane, plane2, src_s, dst_s, rowptr_src,
                 rowptr_dst, inv_k, E, qdirs, nd, grad_f, part);
    return GAOT_OK;
}

}  // namespace

// gaot_gno_adj_jet2's workspace: two 32-float slots per 32-edge tile
extern "C" size_t gaot_gno_adj_jet2_qd_workspace_bytes(int64_t num_edges) { return gaot_gno_adj_jet2_workspace_bytes(num_edges); }

extern "C" int gaot_gno_adj_jet2_qd(const gaot_mlp_t* mlp, const float* y_pos, const float* x_pos, const float* dirs, int nd,
                                    const float* grad_out, const float* grad_d1, const float* grad_d2, int64_t grad_d2_stride,
                                    const int32_t* rowptr_dst, int k, const int32_t* src_sorted, const int32_t* dst_sorted,
                                    const int32_t* rowptr_src, int64_t num_edges, int64_t num_sources, int64_t num_queries,
                                    float* grad_f_y, void* workspace, size_t workspace_bytes, gaot_stream_t stream) {
    GAOT_ENTER();
    GAOT_CHECK_ARG(mlp, "null mlp");
    if (!(mlp->channels == C && mlp->hidden == H && mlp->n_hidden >= 1 && mlp->n_hidden <= 4)) {
        gaot_set_error("gaot_gno_adj_jet2_qd: unsupported MLP shape (n_hidden=%d hidden=%d channels=%d)", mlp->n_hidden, mlp->hidden,
                       mlp->channels);
        return GAOT_ERR_UNSUPPORTED;
    }
    GAOT_CHECK_ARG(nd >= 1 && nd <= MAXD, "nd must be 1..6 directions");
    GAOT_CHECK_ARG(num_edges >= 0 && num_sources >= 0 && num_queries >= 0, "negative size");
    GAOT_CHECK_ARG(num_edges <= (int64_t)INT32_MAX, "num_edges beyond int32 (take the queries in chunks)");
    GAOT_CHECK_ARG(dirs || num_queries == 0, "null dirs");
    if (dirs) {
        hipPointerAttribute_t attr;   // the directions are read by the kernel: a host pointer is an argument error
        const hipError_t pe = hipPointerGetAttributes(&attr, dirs);
        if (pe != hipSuccess) (void)hipGetLastError();  // ordinary host memory the runtime has never seen
        GAOT_CHECK_ARG(pe == hipSuccess && (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged),
                       "dirs must be a device pointer [num_queries][nd][3] (the kernel reads the directions of every query)");
    }
    GAOT_CHECK_ARG(grad_d2_stride == 0 || grad_d2_stride == num_queries * C,
                   "grad_d2_stride must be num_queries * 32 (one plane per direction) or 0 (one plane for all directions)");
    GAOT_CHECK_ARG(rowptr_dst || k > 0, "null rowptr_dst needs k > 0 (the degree of every query of a regular list)");
    GAOT_CHECK_ARG(rowptr_dst || num_edges == num_queries * (int64_t)k, "a regular list holds num_queries * k edges");
    GAOT_CHECK_ARG(rowptr_src && (num_sources == 0 || grad_f_y), "null pointer");
    GAOT_CHECK_ARG(workspace_bytes >= gaot_gno_adj_jet2_qd_workspace_bytes(num_edges) && (workspace || num_edges == 0),
                   "workspace too small");
    MlpPtrs p;
    for (int l = 0; l <= mlp->n_hidden; ++l) {
        p.w[l] = mlp->weight[l];
        p.b[l] = mlp->bias[l];
        GAOT_CHECK_ARG(p.w[l] && p.b[l], "null MLP parameter");
    }
    if (num_edges > 0) {
        GAOT_CHECK_ARG(y_pos && x_pos && grad_out && src_sorted && dst_sorted, "null pointer");
        GAOT_CHECK_ARG(grad_d1, "null grad_d1 (the cotangent of the nd first-derivative planes, [nd][num_queries][32])");
        GAOT_CHECK_ARG(grad_d2, "null grad_d2 (the cotangent of the second-derivative planes, [nd or 1][num_queries][32])");
        GAOT_CHECK_ARG(num_queries > 0, "edges without queries");
    }
    if (num_sources == 0) return GAOT_OK;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    if (num_edges > 0) {
        const float inv_k = rowptr_dst ? 0.f : 1.0f / (float)k;
        const int64_t plane = num_queries * C;
        int rc = GAOT_OK;
#define GNO_ADJQD_JET2_CASE(NH_)                                                                                                     \
    case NH_:                                                                                                                        \
        rc = launch_adjqd_jet2<NH_>(p, y_pos, x_pos, grad_out, grad_d1, grad_d2, plane, grad_d2_stride, src_sorted, dst_sorted,      \
                                    rowptr_src, rowptr_dst, inv_k, num_edges, dirs, nd, grad_f_y, part, st);                         \
        break;
        switch (mlp->n_hidden) {
            GNO_ADJQD_JET2_CASE(1) GNO_ADJQD_JET2_CASE(2) GNO_ADJQD_JET2_CASE(3) GNO_ADJQD_JET2_CASE(4)
        }
#undef GNO_ADJQD_JET2_CASE
        if (rc != GAOT_OK) return rc;
    }
    // tokens without edges -> 0 and the rows that straddle tiles, in tile order (num_edges == 0: this launch alone)
    GAOT_KLAUNCH((k_segment_fixup<32>), dim3(segment_fixup_grid(num_sources * 8)), dim3(256), 0, st, rowptr_src, num_sources, part,
                 grad_f_y, 0);
    GAOT_LAUNCH_CHECK();
    return GAOT_OK;
}
