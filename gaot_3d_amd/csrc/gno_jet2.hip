// The fused GNO forward on a regular k-neighbour list WITH a directional 2-jet: one launch writes the transform's value and, for each
// of nd <= 6 directions v in R^3, its first and second directional derivative with respect to the query coordinate
// (gaot_gno_fwd_knn_jet2) -- what the Hessian (six directions, polarised by the caller) and the Laplacian (three) of a sampled field
// are made of.
//
// With a query's neighbour list held fixed only the three query columns of the first layer see x_q:
//     z_0 = W_0 [y_s ; x_q] + b_0 (+ t[s]),   z'_0 = W_0[:, 3:6] v,            z''_0 = 0
//     h_l = gelu(z_l),                        h'_l = gelu'(z_l) z'_l,          h''_l = gelu''(z_l) z'_l^2 + gelu'(z_l) z''_l
//     z_{l+1} = W_{l+1} h_l + b_{l+1},        z'_{l+1} = W_{l+1} h'_l,         z''_{l+1} = W_{l+1} h''_l
//     out_q = (1/k) sum_e k_e * f[s_e],       d1_q = (1/k) sum_e k'_e * f[s_e], d2_q = (1/k) sum_e k''_e * f[s_e]     (k = z_L)
// (kernel-only mode: without f).  gelu''(z) = phi(z) (2 - z^2).
//
// The kernel is k_gno_fwd_knn_jac's regular-list instantiation (gno_jac.hip): edges on the MFMA lane axis, weights transposed in LDS,
// v_mfma_f32_32x32x2_f32 in both precision modes, the last layer transposed so that channels land on lanes, fixed_k_rows finishing
// each plane.  The directions are looped INSIDE the tile loop: a tile's ids, coordinates and f rows are gathered once, and the VALUE
// PATH IS KEPT, not recomputed: it runs once per tile and writes the value plane.  A direction pass then carries only h' and h'' (32
// registers each) and two sets of accumulators (W h', W h''; 32 each): 2 plane-chains per direction after one for the value -- 7 for
// the Laplacian's three directions, 13 for the Hessian's six -- against 3 per direction when the value is recomputed.  What the value
// path leaves behind depends on the depth: with one or two hidden layers gelu'(z_l) and gelu''(z_l) themselves (64 registers per
// layer); with three or four, where those 192 / 256 registers beside the 128 of a pass made the compiler spill, the pre-activations
// z_l (32 per layer), from which a pass recomputes the two derivatives (VALU work beside the MFMAs, no matrix product).  The same
// expression on the same z gives the same bits, so the contracts below do not depend on the depth.  One workgroup per CU
// (__launch_bounds__(256, 1)) gives a wave the whole 512-entry file.
//
// Bit-level contracts, by construction: the value plane performs gaot_gno_fwd_knn's precision-0 operations in its order (as
// k_gno_fwd_knn_jac's does); z'_0 is the fixed-order chain fma(v_z, w_5, fma(v_y, w_4, v_x w_3)), so for an axis direction e_d it IS
// column 3+d (products with 1 and sums with +-0 are exact) and plane d1 is plane d of gaot_gno_fwd_knn_jac; a direction's pass reads
// nothing another direction wrote, so its planes do not depend on the other directions or their order; a zero direction gives zeros.
//
// The directions arrive BY VALUE in the kernel's arguments (read on the host from a host pointer): no device read of host memory, no
// synchronisation, capturable.  LDS: up to 59.1 KiB of weights plus a 2-plane staging tile of 8 KiB per wave (91.6 KiB of 160 at four
// hidden layers).  No scratch, no atomics, plain vector stores only.
#include "gno_common.h"

namespace {

using namespace gno;

constexpr int H = 64, C = 32, KB = H / 32, MAXD = 6;

template <int NH>
struct Jet2Lds {
    static constexpr int w0 = 0;                                 // [IN0P][H]
    static constexpr int b0 = w0 + IN0P * H;                     // [H]
    static constexpr int wl = b0 + H;                            // (NH-1) x ([H][H] + [H])
    static constexpr int wL = wl + (NH - 1) * (H * H + H);       // [H][32]
    static constexpr int bL = wL + H * C;                        // [32]
    static constexpr int weights_end = bL + C;
    static constexpr int stage = weights_end;                    // [4 waves][2][32][C]
    static constexpr int ids = stage + 4 * 2 * 32 * C;           // [4 waves][32] (int)
    static constexpr size_t bytes = sizeof(float) * (size_t)(ids + 4 * 32);
};

struct Jet2Dirs {
    float v[MAXD][3];
    int nd;
};

// component c of direction d with constant indices only (a dynamic index would put the by-value argument into scratch)
__device__ __forceinline__ float dir_at(const Jet2Dirs& D, int d, int c) {
    float r = D.v[0][c];
#pragma unroll
    for (int i = 1; i < MAXD; ++i) r = d == i ? D.v[i][c] : r;
    return r;
}

// x, as a value the optimiser cannot trace: keeps the recomputation of gelu' / gelu'' from z_l INSIDE the direction loop (hoisted out
// of it as loop-invariant, the derivatives of every layer are live across the loop again and the kernel spills)
__device__ __forceinline__ float opaque(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

// gelu_fast's value (its own expression: bit-identical), gelu_fast_pair's derivative (gelu_fast_tangent of gno_jac.hip) and the
// second derivative phi(x) (2 - x^2); t, p, e are shared
__device__ __forceinline__ void gelu_fast_jet2(float x, float& g, float& dg, float& ddg) {
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
    ddg = 0.39894228040143267794f * e * fmaf(-x, x, 2.0f);
}

template <int NH, int MODE>
__global__ __launch_bounds__(256, 1) void k_gno_fwd_knn_jet2(MlpPtrs mlp, const float* __restrict__ y_pos,
                                                             const float* __restrict__ x_pos, const float* __restrict__ f_y,
                                                             const float* __restrict__ ttab, const int* __restrict__ nbr, int lk,
                                                             int64_t E, const Jet2Dirs dirs, float* __restrict__ out,
                                                             float* __restrict__ d1, float* __restrict__ d2) {
    using L = Jet2Lds<NH>;
    constexpr bool KEEP = NH <= 2;   // what the value path leaves for the direction passes (see the head of this file)
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
    float* stage = lds + L::stage + wave * (2 * 32 * C);
    int* ids = (int*)(lds + L::ids) + wave * 32;
    const int64_t plane = (E >> lk) * C;   // one [Nq][32] plane of d1 / d2

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
        // ---- the value path, once per tile: gelu' and gelu'' of every hidden layer stay in registers -----
        f32x16 h[KB], sa[NH][KB], sb[KEEP ? NH : 1][KB];   // KEEP: gelu'(z_l), gelu''(z_l); else z_l
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
        // ---- last layer, transposed: K'[e][c] = sum_k Hlast[k][e] * WL[c][k] + bL[c]; the value plane is finished by half 0 ----
        wave_lds_fence();  // ids visible to the whole wave
        [[maybe_unused]] float fv[16];
        if constexpr (MODE != MODE_KERNELONLY) {
#pragma unroll
            for (int r = 0; r < 16; ++r) fv[r] = f_y[(int64_t)ids[mfma32_row(r, hf)] * C + l31];
        }
        {
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
            for (int r = 0; r < 16; ++r) {
                const int el = mfma32_row(r, hf);
                if constexpr (MODE == MODE_KERNELONLY) stage[el * C + l31] = acc[r];
                else stage[el * C + l31] = acc[r] * fv[r];
            }
        }
        wave_lds_fence();
        if (hf == 0) fixed_k_rows<C>(stage, C, l31, base, lk, E, out);
        wave_lds_fence();

        // ---- one pass per direction: h' and h'' through the layers, two planes staged, one finished by each half ----
#pragma unroll 1
        for (int d = 0; d < dirs.nd; ++d) {
            const float vx = dir_at(dirs, d, 0), vy = dir_at(dirs, d, 1), vz = dir_at(dirs, d, 2);
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
                for (int r = 0; r < 16; ++r) {
                    const int el = mfma32_row(r, hf);
                    if constexpr (MODE == MODE_KERNELONLY) stage[(p * 32 + el) * C + l31] = acc[r];
                    else stage[(p * 32 + el) * C + l31] = acc[r] * fv[r];
                }
            }
            wave_lds_fence();
            fixed_k_rows<C>(stage + hf * 32 * C, C, l31, base, lk, E, (hf ? d2 : d1) + (int64_t)d * plane);
            wave_lds_fence();
        }
    }
}

template <int NH, int MODE>
int launch_jet2(const MlpPtrs& p, const float* y_pos, const float* x_pos, const float* f_y, const float* ttab, const int* nbr, int lk,
                int64_t E, const Jet2Dirs& dirs, float* out, float* d1, float* d2, hipStream_t st) {
    constexpr size_t lds = Jet2Lds<NH>::bytes;
    auto kern = k_gno_fwd_knn_jet2<NH, MODE>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
        gaot_set_error("gaot_gno_fwd_knn_jet2: cannot set dynamic LDS %zu: %s", lds, hipGetErrorString(e));
        return GAOT_ERR_LAUNCH;
    }
    const int64_t n_tiles = ceil_div(E, 32);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n_tiles, 4), 256));   // one workgroup per CU
    GAOT_KLAUNCH(kern, dim3(grid), dim3(256), lds, st, p, y_pos, x_pos, f_y, ttab, nbr, lk, E, dirs, out, d1, d2);
    return GAOT_OK;
}

}  // namespace

extern "C" int gaot_gno_fwd_knn_jet2(const gaot_mlp_t* mlp, int mode, const float* y_pos, const float* x_pos, const float* f_y,
                                     const float* src_table, const int32_t* nbr, int k, int64_t num_queries, const float* dirs, int nd,
                                     float* out, float* d1, float* d2, gaot_stream_t stream) {
    GAOT_ENTER();
    GAOT_CHECK_ARG(mlp, "null mlp");
    if (!(mlp->channels == C && mlp->hidden == H && mlp->n_hidden >= 1 && mlp->n_hidden <= 4)) {
        gaot_set_error("gaot_gno_fwd_knn_jet2: unsupported MLP shape (n_hidden=%d hidden=%d channels=%d)", mlp->n_hidden, mlp->hidden,
                       mlp->channels);
        return GAOT_ERR_UNSUPPORTED;
    }
    GAOT_CHECK_ARG(mode == MODE_LINEAR || mode == MODE_NONLINEAR || mode == MODE_KERNELONLY,
                   "mode must be 0 (linear), 1 (nonlinear) or 2 (nonlinear_kernelonly)");
    GAOT_CHECK_ARG(k == 1 || k == 2 || k == 4 || k == 8 || k == 16 || k == 32, "k must be 1, 2, 4, 8, 16 or 32 (a divisor of the 32-edge tile)");
    GAOT_CHECK_ARG(nd >= 1 && nd <= MAXD, "nd must be 1..6 directions");
    GAOT_CHECK_ARG(dirs, "null dirs");
    GAOT_CHECK_ARG(num_queries >= 0, "negative size");
    GAOT_CHECK_ARG(num_queries <= (int64_t)INT32_MAX / k, "num_queries * k beyond int32 (sample the queries in chunks)");
    GAOT_CHECK_ARG(y_pos && x_pos && nbr && out && d1 && d2 && (f_y || mode == MODE_KERNELONLY), "null pointer");
    GAOT_CHECK_ARG(mode == MODE_LINEAR || src_table, "null src_table");
    MlpPtrs p;
    for (int l = 0; l <= mlp->n_hidden; ++l) {
        p.w[l] = mlp->weight[l];
        p.b[l] = mlp->bias[l];
        GAOT_CHECK_ARG(p.w[l] && p.b[l], "null MLP parameter");
    }
    if (num_queries == 0) return GAOT_OK;
    Jet2Dirs dv;   // read here, on the host: the kernel takes the directions by value
    dv.nd = nd;
    for (int d = 0; d < MAXD; ++d)
        for (int c = 0; c < 3; ++c) dv.v[d][c] = d < nd ? dirs[d * 3 + c] : 0.f;
    hipStream_t st = (hipStream_t)stream;
    const int lk = __builtin_ctz((unsigned)k);
    const int64_t num_edges = num_queries * k;
    int rc = GAOT_OK;
#define GNO_JET2_CASE(NH_, MODE_)                                                                                      \
    case NH_ * 3 + MODE_:                                                                                              \
        rc = launch_jet2<NH_, MODE_>(p, y_pos, x_pos, f_y, src_table, nbr, lk, num_edges, dv, out, d1, d2, st);        \
        break;
#define GNO_JET2_CASES(NH_) GNO_JET2_CASE(NH_, MODE_LINEAR) GNO_JET2_CASE(NH_, MODE_NONLINEAR) GNO_JET2_CASE(NH_, MODE_KERNELONLY)
    switch (mlp->n_hidden * 3 + mode) {
        GNO_JET2_CASES(1) GNO_JET2_CASES(2) GNO_JET2_CASES(3) GNO_JET2_CASES(4)
    }
#undef GNO_JET2_CASES
#undef GNO_JET2_CASE
    if (rc != GAOT_OK) return rc;
    GAOT_LAUNCH_CHECK();
    return GAOT_OK;
}
