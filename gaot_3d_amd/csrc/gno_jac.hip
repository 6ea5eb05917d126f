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
//
// RAGGED rows (gaot_gno_fwd_jac, the by-query list of a 'radius' / 'bidirectional' graph): the same kernel with a JacRows ending its
// arguments.  The per-edge arithmetic is untouched; the query of an edge comes from dst_sorted, the wave keeps its 32 query ids in
// LDS (128 bytes more per wave) and every plane is finished by segment_walk<32> -- complete rows stored as their mean, rows that
// straddle tiles left in the plane's partial buffer -- and by ONE fix-up launch over all four planes (k_jac_rows_fixup).  On a list
// whose rows all have k | 32 edges the two variants perform the same operations in the same order: bit-identical planes.
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
    static constexpr int qids = ids + 4 * 32;                    // row lists only: [4 waves][32] (int), the edges' queries
    static constexpr size_t bytes_rows = sizeof(float) * (size_t)(qids + 4 * 32);
};

// ROW-LIST variant (gaot_gno_fwd_jac): a JacRows as the kernel's last argument (a parameter pack that is empty on regular lists, so
// those instantiations keep their arguments and instructions).  `nbr` is then the by-query list's source ids (src_sorted), the query
// of edge e is dst_s[e] (edges past E: -1, as in k_gno_fwd), lk is not read, and every plane is finished by segment_walk with its
// own partial buffer: part + p * part_plane, two 32-float slots per tile.  PADDING edges -- dst_s[e] = -1 with any valid source id,
// outside every row of rowptr -- are computed and dropped by the walk like the edges past E: a list may begin with some (rowptr[0] > 0)
// so that its rows lie against the 32-edge tiles as they do in a longer list it is a piece of (MAGNODecoder.sample_jacobian's chunks).
struct JacRows {
    const int* dst_s;       // [E]
    const int* rowptr;      // [Nq + 1]
    float* part;            // [NP][n_tiles][2][32]
    int64_t plane;          // Nq * 32: one plane of jac
    int64_t part_plane;     // n_tiles * 2 * 32: one plane of part
};

template <int NH, int MODE, class... Rows>
__global__ __launch_bounds__(256, 1) void k_gno_fwd_knn_jac(MlpPtrs mlp, const float* __restrict__ y_pos,
                                                            const float* __restrict__ x_pos, const float* __restrict__ f_y,
                                                            const float* __restrict__ ttab, const int* __restrict__ nbr, int lk,
                                                            int64_t E, float* __restrict__ out, float* __restrict__ jac, Rows... rows_) {
    using L = JacLds<NH>;
    constexpr bool R = pack_has<JacRows, Rows...>;
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
    int64_t plane;                         // one [Nq][32] plane of jac
    [[maybe_unused]] int* qids = nullptr;
    if constexpr (R) {
        plane = first_arg(rows_...).plane;
        qids = (int*)(lds + L::qids) + wave * 32;
    } else {
        plane = (E >> lk) * C;
    }

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
            int q;
            [[maybe_unused]] int qid = -1;   // row lists: the edge's row; -1 = no row (past E, or a padding edge of the list)
            if constexpr (R) {
                if (valid) qid = first_arg(rows_...).dst_s[e];
                q = qid < 0 ? 0 : qid;       // a valid row to read coordinates from
            } else {
                q = valid ? (int)(e >> lk) : 0;
            }
            const float* ys = y_pos + (int64_t)sid * 3;
            const float* xq = x_pos + (int64_t)q * 3;
            bin[0] = ys[hf];
            bin[1] = hf ? xq[0] : ys[2];
            bin[2] = xq[1 + hf];
            if (hf == 0) {
                ids[l31] = sid;
                if constexpr (R) qids[l31] = qid;
            }
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
        // ---- row means (fixed-k / segmented): half 0 finishes the value and d/dx, half 1 d/dy and d/dz ------
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = 2 * hf + i;
            float* dst = p == 0 ? out : jac + (int64_t)(p - 1) * plane;
            if constexpr (R)
                segment_walk<C>(stage + p * 32 * C, C, qids, l31, base, first_arg(rows_...).rowptr, dst,
                                first_arg(rows_...).part + p * first_arg(rows_...).part_plane, true);
            else
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

// The fix-up of all four planes in one pass over rowptr: on each plane k_segment_fixup<32>'s operations in its order -- rows with no
// edges -> 0, rows spanning several tiles -> the ordered sum of their tile partials, then the division by the degree.
__global__ void k_jac_rows_fixup(const int* __restrict__ rowptr, int64_t Q, const float* __restrict__ part, int64_t part_plane,
                                 float* __restrict__ out, float* __restrict__ jac) {
    constexpr int TPR = C / 4;                                   // threads per row, 16 bytes each
    const int64_t n = Q * TPR, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t q = i / TPR;
        const int c = (int)(i % TPR) * 4;
        const int rb = rowptr[q], re = rowptr[q + 1];
        const int t0 = rb >> 5, t1 = (re - 1) >> 5;
        if (re != rb && t0 == t1) continue;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            float4* o = reinterpret_cast<float4*>((p == 0 ? out : jac + (int64_t)(p - 1) * Q * C) + q * C + c);
            if (re == rb) {
                *o = make_float4(0.f, 0.f, 0.f, 0.f);
                continue;
            }
            const float* pp = part + p * part_plane;
            float4 s = *reinterpret_cast<const float4*>(pp + ((int64_t)t0 * 2 + 1) * C + c);
            for (int t = t0 + 1; t <= t1; ++t) {
                const float4 v = *reinterpret_cast<const float4*>(pp + ((int64_t)t * 2 + 0) * C + c);
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
            const float d = (float)(re - rb);
            s.x /= d; s.y /= d; s.z /= d; s.w /= d;
            *o = s;
        }
    }
}

template <int NH, int MODE>
int launch_jac_rows(const MlpPtrs& p, const float* y_pos, const float* x_pos, const float* f_y, const float* ttab, const int* src_s,
                    const JacRows& rows, int64_t E, float* out, float* jac, hipStream_t st) {
    constexpr size_t lds = JacLds<NH>::bytes_rows;
    auto kern = k_gno_fwd_knn_jac<NH, MODE, JacRows>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
        gaot_set_error("gaot_gno_fwd_jac: cannot set dynamic LDS %zu: %s", lds, hipGetErrorString(e));
        return GAOT_ERR_LAUNCH;
    }
    const int64_t n_tiles = ceil_div(E, 32);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n_tiles, 4), 256));   // one workgroup per CU
    GAOT_KLAUNCH(kern, dim3(grid), dim3(256), lds, st, p, y_pos, x_pos, f_y, ttab, src_s, 0, E, out, jac, rows);
    return GAOT_OK;
}

}  // namespace

// two 32-float slots per 32-edge tile and plane: 1 KiB per tile
extern "C" size_t gaot_gno_fwd_jac_workspace_bytes(int64_t num_edges) {
    return num_edges > 0 ? sizeof(float) * (size_t)(ceil_div(num_edges, 32) * NP * 2 * C) : 0;
}

// The tangent kernel on RAGGED rows (the by-query list of any graph) and the four-plane fix-up: two launches
extern "C" int gaot_gno_fwd_jac(const gaot_mlp_t* mlp, int mode, const float* y_pos, const float* x_pos, const float* f_y,
                                const float* src_table, const int32_t* src_sorted, const int32_t* dst_sorted,
                                const int32_t* rowptr_dst, int64_t num_edges, int64_t num_queries, float* out, float* jac,
                                void* workspace, size_t workspace_bytes, gaot_stream_t stream) {
    GAOT_ENTER();
    GAOT_CHECK_ARG(mlp, "null mlp");
    if (!(mlp->channels == C && mlp->hidden == H && mlp->n_hidden >= 1 && mlp->n_hidden <= 4)) {
        gaot_set_error("gaot_gno_fwd_jac: unsupported MLP shape (n_hidden=%d hidden=%d channels=%d)", mlp->n_hidden, mlp->hidden,
                       mlp->channels);
        return GAOT_ERR_UNSUPPORTED;
    }
    GAOT_CHECK_ARG(mode == MODE_LINEAR || mode == MODE_NONLINEAR || mode == MODE_KERNELONLY,
                   "mode must be 0 (linear), 1 (nonlinear) or 2 (nonlinear_kernelonly)");
    GAOT_CHECK_ARG(num_edges >= 0 && num_queries >= 0, "negative size");
    GAOT_CHECK_ARG(num_edges <= (int64_t)INT32_MAX, "num_edges beyond int32 (sample the queries in chunks)");
    GAOT_CHECK_ARG(rowptr_dst && (num_queries == 0 || (out && jac)), "null pointer");
    if (num_edges > 0) {
        GAOT_CHECK_ARG(y_pos && x_pos && src_sorted && dst_sorted && (f_y || mode == MODE_KERNELONLY), "null pointer");
        GAOT_CHECK_ARG(mode == MODE_LINEAR || src_table, "null src_table");
        GAOT_CHECK_ARG(workspace, "null workspace");
    }
    GAOT_CHECK_ARG(workspace_bytes >= gaot_gno_fwd_jac_workspace_bytes(num_edges), "workspace too small");
    MlpPtrs p;
    for (int l = 0; l <= mlp->n_hidden; ++l) {
        p.w[l] = mlp->weight[l];
        p.b[l] = mlp->bias[l];
        GAOT_CHECK_ARG(p.w[l] && p.b[l], "null MLP parameter");
    }
    if (num_queries == 0) return GAOT_OK;
    hipStream_t st = (hipStream_t)stream;
    const JacRows rows{dst_sorted, rowptr_dst, (float*)workspace, num_queries * C, ceil_div(num_edges, 32) * 2 * C};
    if (num_edges > 0) {
        int rc = GAOT_OK;
#define GNO_JAC_CASE(NH_, MODE_)                                                                                       \
    case NH_ * 3 + MODE_:                                                                                              \
        rc = launch_jac_rows<NH_, MODE_>(p, y_pos, x_pos, f_y, src_table, src_sorted, rows, num_edges, out, jac, st);  \
        break;
#define GNO_JAC_CASES(NH_) GNO_JAC_CASE(NH_, MODE_LINEAR) GNO_JAC_CASE(NH_, MODE_NONLINEAR) GNO_JAC_CASE(NH_, MODE_KERNELONLY)
        switch (mlp->n_hidden * 3 + mode) {
            GNO_JAC_CASES(1) GNO_JAC_CASES(2) GNO_JAC_CASES(3) GNO_JAC_CASES(4)
        }
#undef GNO_JAC_CASES
#undef GNO_JAC_CASE
        if (rc != GAOT_OK) return rc;
    }
    // empty rows -> 0 and the rows that straddle tiles, all four planes (num_edges == 0: this launch alone)
    GAOT_KLAUNCH(k_jac_rows_fixup, dim3(segment_fixup_grid(num_queries * 8)), dim3(256), 0, st, rowptr_dst, num_queries, rows.part,
                 rows.part_plane, out, jac);
    GAOT_LAUNCH_CHECK();
    return GAOT_OK;
}

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
