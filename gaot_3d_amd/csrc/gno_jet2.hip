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
//
// RAGGED rows (gaot_gno_fwd_jet2, the by-query list of a 'radius' / 'bidirectional' graph): k_gno_fwd_rows_jet2, the same kernel body
// (gno_jet2_body.inc) with the list handling of gno_jac.hip's JacRows.  The per-edge arithmetic is untouched; the query of an edge
// comes from dst_sorted, the wave keeps its 32 query ids in LDS (128 bytes more per wave) and every one of the 1 + 2 nd planes is
// finished by segment_walk<32> -- complete rows stored as their mean, rows that straddle tiles left in the plane's partial buffer --
// and by ONE fix-up launch over all planes (k_jet2_rows_fixup).  On a list whose rows all have k | 32 edges the two kernels perform
// the same operations in the same order: bit-identical planes.
//
// PER-QUERY directions (gaot_gno_fwd_knn_jet2_qd / gaot_gno_fwd_jet2_qd): k_gno_qd_jet2_knn / k_gno_qd_jet2_rows, the same body once
// more with QD = true -- see Jet2QDirs below.  All 24 instantiations are built without scratch (tests/test_field_directional_cpu.py).
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
    static constexpr int qids = ids + 4 * 32;                    // row lists only: [4 waves][32] (int), the edges' queries
    static constexpr size_t bytes_rows = sizeof(float) * (size_t)(qids + 4 * 32);
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

// PER-QUERY directions (gaot_gno_fwd_knn_jet2_qd / gaot_gno_fwd_jet2_qd): a DEVICE array [Nq][nd][3].  Edges sit on the lane axis and
// every edge belongs to one query, so the direction of a pass is a per-lane value: at the top of the pass each lane loads the three
// components of direction d of ITS edge's query and z'_0 is formed by the same fixed-order fma chain; nothing else in the kernel
// body changes.  Kernels of their own (k_gno_qd_jet2_knn / k_gno_qd_jet2_rows): the host-direction kernels stay what they were.
struct Jet2QDirs {
    const float* v;         // [Nq][nd][3]
    int nd;
};

// the overloads the kernel body's untaken `if constexpr` branch still has to compile against
__device__ __forceinline__ float dir_at(const Jet2QDirs&, int, int) { return 0.f; }
__device__ __forceinline__ const float* qdir_at(const Jet2Dirs&, int64_t) { return nullptr; }
__device__ __forceinline__ const float* qdir_at(const Jet2QDirs& D, int64_t i) { return D.v + i; }

// opaque() and the activation jet gelu_fast_jet2(): gno_common.h

// ROW-LIST variant (gaot_gno_fwd_jet2, k_gno_fwd_rows_jet2): the kernel body (gno_jet2_body.inc) with R = true and a Jet2Rows as the
// kernel's last argument.  As JacRows of gno_jac.hip: `nbr` is the by-query list's source ids (src_sorted), the
// query of edge e is dst_s[e] (-1: no row -- an edge past E, or a PADDING edge of the list; such edges read row 0, are computed and
// are dropped by the walk), lk is not read, and every plane is finished by segment_walk with its own partial buffer, two 32-float
// slots per tile: plane 0 the value, 1 + d direction d's D_v, 1 + nd + d its D_v^2.
struct Jet2Rows {
    const int* dst_s;       // [E]
    const int* rowptr;      // [Nq + 1]
    float* part;            // [1 + 2 nd][n_tiles][2][32]
    int64_t plane;          // Nq * 32: one plane of d1 / d2
    int64_t part_plane;     // n_tiles * 2 * 32: one plane of part
};

template <int NH, int MODE>
__global__ __launch_bounds__(256, 1) void k_gno_fwd_knn_jet2(MlpPtrs mlp, const float* __restrict__ y_pos,
                                                             const float* __restrict__ x_pos, const float* __restrict__ f_y,
                                                             const float* __restrict__ ttab, const int* __restrict__ nbr, int lk,
                                                             int64_t E, const Jet2Dirs dirs, float* __restrict__ out,
                                                             float* __restrict__ d1, float* __restrict__ d2) {
    constexpr bool R = false, QD = false;
    [[maybe_unused]] const Jet2Rows rows{};
#include "gno_jet2_body.inc"
}

// the same arithmetic on RAGGED rows (a name of its own: the regular-list kernels are counted by theirs)
template <int NH, int MODE>
__global__ __launch_bounds__(256, 1) void k_gno_fwd_rows_jet2(MlpPtrs mlp, const float* __restrict__ y_pos,
                                                              const float* __restrict__ x_pos, const float* __restrict__ f_y,
                                                              const float* __restrict__ ttab, const int* __restrict__ nbr, int64_t E,
                                                              const Jet2Dirs dirs, float* __restrict__ out, float* __restrict__ d1,
                                                              float* __restrict__ d2, const Jet2Rows rows) {
    constexpr bool R = true, QD = false;
    [[maybe_unused]] constexpr int lk = 0;   // not read on row lists
#include "gno_jet2_body.inc"
}

// the two kernels along PER-QUERY directions (names of their own: the host-direction kernels are counted by theirs)
template <int NH, int MODE>
__global__ __launch_bounds__(256, 1) void k_gno_qd_jet2_knn(MlpPtrs mlp, const float* __restrict__ y_pos, const float* __restrict__ x_pos,
                                                            const float* __restrict__ f_y, const float* __restrict__ ttab,
                                                            const int* __restrict__ nbr, int lk, int64_t E, const Jet2QDirs dirs,
                                                            float* __restrict__ out, float* __restrict__ d1, float* __restrict__ d2) {
    constexpr bool R = false, QD = true;
    [[maybe_unused]] const Jet2Rows rows{};
#include "gno_jet2_body.inc"
}

template <int NH, int MODE>
__global__ __launch_bounds__(256, 1) void k_gno_qd_jet2_rows(MlpPtrs mlp, const float* __restrict__ y_pos, const float* __restrict__ x_pos,
                                                             const float* __restrict__ f_y, const float* __restrict__ ttab,
                                                             const int* __restrict__ nbr, int64_t E, const Jet2QDirs dirs,
                                                             float* __restrict__ out, float* __restrict__ d1, float* __restrict__ d2,
                                                             const Jet2Rows rows) {
    constexpr bool R = true, QD = true;
    [[maybe_unused]] constexpr int lk = 0;   // not read on row lists
#include "gno_jet2_body.inc"
}

// The fix-up of all 1 + 2 nd planes in one pass over rowptr (k_jac_rows_fixup with a plane count): on each plane
// k_segment_fixup<32>'s operations in its order -- rows with no edges -> 0, rows spanning several tiles -> the ordered sum of their
// tile partials, then the division by the degree.
__global__ void k_jet2_rows_fixup(const int* __restrict__ rowptr, int64_t Q, const float* __restrict__ part, int64_t part_plane, int nd,
                                  float* __restrict__ out, float* __restrict__ d1, float* __restrict__ d2) {
    constexpr int TPR = C / 4;                                   // threads per row, 16 bytes each
    const int64_t n = Q * TPR, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t q = i / TPR;
        const int c = (int)(i % TPR) * 4;
        const int rb = rowptr[q], re = rowptr[q + 1];
        const int t0 = rb >> 5, t1 = (re - 1) >> 5;
        if (re != rb && t0 == t1) continue;
        for (int p = 0; p < 1 + 2 * nd; ++p) {
            float* base = p == 0 ? out : p <= nd ? d1 + (int64_t)(p - 1) * Q * C : d2 + (int64_t)(p - 1 - nd) * Q * C;
            float4* o = reinterpret_cast<float4*>(base + q * C + c);
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

// D: Jet2Dirs (host directions by value) or Jet2QDirs (per-query directions on the device) -- the kernel follows the type
template <int NH, int MODE, class D>
int launch_jet2_rows(const MlpPtrs& p, const float* y_pos, const float* x_pos, const float* f_y, const float* ttab, const int* src_s,
                     const Jet2Rows& rows, int64_t E, const D& dirs, float* out, float* d1, float* d2, hipStream_t st) {
    constexpr size_t lds = Jet2Lds<NH>::bytes_rows;
    constexpr bool QD = std::is_same_v<D, Jet2QDirs>;
    auto kern = [] {
        if constexpr (QD) return k_gno_qd_jet2_rows<NH, MODE>;
        else return k_gno_fwd_rows_jet2<NH, MODE>;
    }();
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
        gaot_set_error("gaot_gno_fwd_jet2%s: cannot set dynamic LDS %zu: %s", QD ? "_qd" : "", lds, hipGetErrorString(e));
        return GAOT_ERR_LAUNCH;
    }
    const int64_t n_tiles = ceil_div(E, 32);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n_tiles, 4), 256));   // one workgroup per CU
    GAOT_KLAUNCH(kern, dim3(grid), dim3(256), lds, st, p, y_pos, x_pos, f_y, ttab, src_s, E, dirs, out, d1, d2, rows);
    return GAOT_OK;
}

template <int NH, int MODE, class D>
int launch_jet2(const MlpPtrs& p, const float* y_pos, const float* x_pos, const float* f_y, const float* ttab, const int* nbr, int lk,
                int64_t E, const D& dirs, float* out, float* d1, float* d2, hipStream_t st) {
    constexpr size_t lds = Jet2Lds<NH>::bytes;
    constexpr bool QD = std::is_same_v<D, Jet2QDirs>;
    auto kern = [] {
        if constexpr (QD) return k_gno_qd_jet2_knn<NH, MODE>;
        else return k_gno_fwd_knn_jet2<NH, MODE>;
    }();
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
        gaot_set_error("gaot_gno_fwd_knn_jet2%s: cannot set dynamic LDS %zu: %s", QD ? "_qd" : "", lds, hipGetErrorString(e));
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

// two 32-float slots per 32-edge tile and plane, 1 + 2 nd planes: 256 (1 + 2 nd) bytes per tile (3.25 KiB at six directions)
extern "C" size_t gaot_gno_fwd_jet2_workspace_bytes(int64_t num_edges, int nd) {
    return num_edges > 0 && nd >= 0 ? sizeof(float) * (size_t)(ceil_div(num_edges, 32) * (1 + 2 * nd) * 2 * C) : 0;
}

// The jet kernel on RAGGED rows (the by-query list of any graph) and the fix-up of its 1 + 2 nd planes: two launches
extern "C" int gaot_gno_fwd_jet2(const gaot_mlp_t* mlp, int mode, const float* y_pos, const float* x_pos, const float* f_y,
                                 const float* src_table, const int32_t* src_sorted, const int32_t* dst_sorted,
                                 const int32_t* rowptr_dst, int64_t num_edges, int64_t num_queries, const float* dirs, int nd,
                                 float* out, float* d1, float* d2, void* workspace, size_t workspace_bytes, gaot_stream_t stream) {
    GAOT_ENTER();
    GAOT_CHECK_ARG(mlp, "null mlp");
    if (!(mlp->channels == C && mlp->hidden == H && mlp->n_hidden >= 1 && mlp->n_hidden <= 4)) {
        gaot_set_error("gaot_gno_fwd_jet2: unsupported MLP shape (n_hidden=%d hidden=%d channels=%d)", mlp->n_hidden, mlp->hidden,
                       mlp->channels);
        return GAOT_ERR_UNSUPPORTED;
    }
    GAOT_CHECK_ARG(mode == MODE_LINEAR || mode == MODE_NONLINEAR || mode == MODE_KERNELONLY,
                   "mode must be 0 (linear), 1 (nonlinear) or 2 (nonlinear_kernelonly)");
    GAOT_CHECK_ARG(nd >= 1 && nd <= MAXD, "nd must be 1..6 directions");
    GAOT_CHECK_ARG(dirs, "null dirs");
    {
        hipPointerAttribute_t attr;   // the directions are read here, on the host: a device pointer is an argument error
        if (hipPointerGetAttributes(&attr, dirs) == hipSuccess)
            GAOT_CHECK_ARG(attr.type != hipMemoryTypeDevice, "dirs must be a host pointer (the directions are passed to the kernel by value)");
        else
            (void)hipGetLastError();  // ordinary host memory the runtime has never seen
    }
    GAOT_CHECK_ARG(num_edges >= 0 && num_queries >= 0, "negative size");
    GAOT_CHECK_ARG(num_edges <= (int64_t)INT32_MAX, "num_edges beyond int32 (sample the queries in chunks)");
    GAOT_CHECK_ARG(rowptr_dst && (num_queries == 0 || (out && d1 && d2)), "null pointer");
    if (num_edges > 0) {
        GAOT_CHECK_ARG(y_pos && x_pos && src_sorted && dst_sorted && (f_y || mode == MODE_KERNELONLY), "null pointer");
        GAOT_CHECK_ARG(mode == MODE_LINEAR || src_table, "null src_table");
        GAOT_CHECK_ARG(workspace, "null workspace");
    }
    GAOT_CHECK_ARG(workspace_bytes >= gaot_gno_fwd_jet2_workspace_bytes(num_edges, nd), "workspace too small");
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
    const Jet2Rows rows{dst_sorted, rowptr_dst, (float*)workspace, num_queries * C, ceil_div(num_edges, 32) * 2 * C};
    if (num_edges > 0) {
        int rc = GAOT_OK;
#define GNO_JET2_CASE(NH_, MODE_)                                                                                               \
    case NH_ * 3 + MODE_:                                                                                                       \
        rc = launch_jet2_rows<NH_, MODE_>(p, y_pos, x_pos, f_y, src_table, src_sorted, rows, num_edges, dv, out, d1, d2, st);   \
        break;
#define GNO_JET2_CASES(NH_) GNO_JET2_CASE(NH_, MODE_LINEAR) GNO_JET2_CASE(NH_, MODE_NONLINEAR) GNO_JET2_CASE(NH_, MODE_KERNELONLY)
        switch (mlp->n_hidden * 3 + mode) {
            GNO_JET2_CASES(1) GNO_JET2_CASES(2) GNO_JET2_CASES(3) GNO_JET2_CASES(4)
        }
#undef GNO_JET2_CASES
#undef GNO_JET2_CASE
        if (rc != GAOT_OK) return rc;
    }
    // empty rows -> 0 and the rows that straddle tiles, all 1 + 2 nd planes (num_edges == 0: this launch alone)
    GAOT_KLAUNCH(k_jet2_rows_fixup, dim3(segment_fixup_grid(num_queries * 8)), dim3(256), 0, st, rowptr_dst, num_queries, rows.part,
                 rows.part_plane, nd, out, d1, d2);
    GAOT_LAUNCH_CHECK();
    return GAOT_OK;
}

// ---- per-query directions: `qdirs` is a DEVICE array [num_queries][nd][3] the kernel reads (no host read: capturable) ------------------
extern "C" int gaot_gno_fwd_knn_jet2_qd(const gaot_mlp_t* mlp, int mode, const float* y_pos, const float* x_pos, const float* f_y,
                                        const float* src_table, const int32_t* nbr, int k, int64_t num_queries, const float* qdirs,
                                        int nd, float* out, float* d1, float* d2, gaot_stream_t stream) {
    GAOT_ENTER();
    GAOT_CHECK_ARG(mlp, "null mlp");
    if (!(mlp->channels == C && mlp->hidden == H && mlp->n_hidden >= 1 && mlp->n_hidden <= 4)) {
        gaot_set_error("gaot_gno_fwd_knn_jet2_qd: unsupported MLP shape (n_hidden=%d hidden=%d channels=%d)", mlp->n_hidden, mlp->hidden,
                       mlp->channels);
        return GAOT_ERR_UNSUPPORTED;
    }
    GAOT_CHECK_ARG(mode == MODE_LINEAR || mode == MODE_NONLINEAR || mode == MODE_KERNELONLY,
                   "mode must be 0 (linear), 1 (nonlinear) or 2 (nonlinear_kernelonly)");
    GAOT_CHECK_ARG(k == 1 || k == 2 || k == 4 || k == 8 || k == 16 || k == 32, "k must be 1, 2, 4, 8, 16 or 32 (a divisor of the 32-edge tile)");
    GAOT_CHECK_ARG(nd >= 1 && nd <= MAXD, "nd must be 1..6 directions");
    GAOT_CHECK_ARG(num_queries >= 0, "negative size");
    GAOT_CHECK_ARG(num_queries <= (int64_t)INT32_MAX / k, "num_queries * k beyond int32 (sample the queries in chunks)");
    if (num_queries > 0) {
        GAOT_CHECK_ARG(qdirs, "null qdirs");
        GAOT_CHECK_ARG(y_pos && x_pos && nbr && out && d1 && d2 && (f_y || mode == MODE_KERNELONLY), "null pointer");
        GAOT_CHECK_ARG(mode == MODE_LINEAR || src_table, "null src_table");
    }
    MlpPtrs p;
    for (int l = 0; l <= mlp->n_hidden; ++l) {
        p.w[l] = mlp->weight[l];
        p.b[l] = mlp->bias[l];
        GAOT_CHECK_ARG(p.w[l] && p.b[l], "null MLP parameter");
    }
    if (num_queries == 0) return GAOT_OK;
    const Jet2QDirs dv{qdirs, nd};
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

extern "C" int gaot_gno_fwd_jet2_qd(const gaot_mlp_t* mlp, int mode, const float* y_pos, const float* x_pos, const float* f_y,
                                    const float* src_table, const int32_t* src_sorted, const int32_t* dst_sorted,
                                    const int32_t* rowptr_dst, int64_t num_edges, int64_t num_queries, const float* qdirs, int nd,
                                    float* out, float* d1, float* d2, void* workspace, size_t workspace_bytes, gaot_stream_t stream) {
    GAOT_ENTER();
    GAOT_CHECK_ARG(mlp, "null mlp");
    if (!(mlp->channels == C && mlp->hidden == H && mlp->n_hidden >= 1 && mlp->n_hidden <= 4)) {
        gaot_set_error("gaot_gno_fwd_jet2_qd: unsupported MLP shape (n_hidden=%d hidden=%d channels=%d)", mlp->n_hidden, mlp->hidden,
                       mlp->channels);
        return GAOT_ERR_UNSUPPORTED;
    }
    GAOT_CHECK_ARG(mode == MODE_LINEAR || mode == MODE_NONLINEAR || mode == MODE_KERNELONLY,
                   "mode must be 0 (linear), 1 (nonlinear) or 2 (nonlinear_kernelonly)");
    GAOT_CHECK_ARG(nd >= 1 && nd <= MAXD, "nd must be 1..6 directions");
    GAOT_CHECK_ARG(num_edges >= 0 && num_queries >= 0, "negative size");
    GAOT_CHECK_ARG(num_edges <= (int64_t)INT32_MAX, "num_edges beyond int32 (sample the queries in chunks)");
    GAOT_CHECK_ARG(rowptr_dst && (num_queries == 0 || (out && d1 && d2)), "null pointer");
    if (num_edges > 0) {
        GAOT_CHECK_ARG(num_queries == 0 || qdirs, "null qdirs");
        GAOT_CHECK_ARG(y_pos && x_pos && src_sorted && dst_sorted && (f_y || mode == MODE_KERNELONLY), "null pointer");
        GAOT_CHECK_ARG(mode == MODE_LINEAR || src_table, "null src_table");
        GAOT_CHECK_ARG(workspace, "null workspace");
    }
    GAOT_CHECK_ARG(workspace_bytes >= gaot_gno_fwd_jet2_workspace_bytes(num_edges, nd), "workspace too small");
    MlpPtrs p;
    for (int l = 0; l <= mlp->n_hidden; ++l) {
        p.w[l] = mlp->weight[l];
        p.b[l] = mlp->bias[l];
        GAOT_CHECK_ARG(p.w[l] && p.b[l], "null MLP parameter");
    }
    if (num_queries == 0) return GAOT_OK;
    const Jet2QDirs dv{qdirs, nd};
    hipStream_t st = (hipStream_t)stream;
    const Jet2Rows rows{dst_sorted, rowptr_dst, (float*)workspace, num_queries * C, ceil_div(num_edges, 32) * 2 * C};
    if (num_edges > 0) {
        int rc = GAOT_OK;
#define GNO_JET2_CASE(NH_, MODE_)                                                                                               \
    case NH_ * 3 + MODE_:                                                                                                       \
        rc = launch_jet2_rows<NH_, MODE_>(p, y_pos, x_pos, f_y, src_table, src_sorted, rows, num_edges, dv, out, d1, d2, st);   \
        break;
#define GNO_JET2_CASES(NH_) GNO_JET2_CASE(NH_, MODE_LINEAR) GNO_JET2_CASE(NH_, MODE_NONLINEAR) GNO_JET2_CASE(NH_, MODE_KERNELONLY)
        switch (mlp->n_hidden * 3 + mode) {
            GNO_JET2_CASES(1) GNO_JET2_CASES(2) GNO_JET2_CASES(3) GNO_JET2_CASES(4)
        }
#undef GNO_JET2_CASES
#undef GNO_JET2_CASE
        if (rc != GAOT_OK) return rc;
    }
    // empty rows -> 0 and the rows that straddle tiles, all 1 + 2 nd planes (num_edges == 0: this launch alone)
    GAOT_KLAUNCH(k_jet2_rows_fixup, dim3(segment_fixup_grid(num_queries * 8)), dim3(256), 0, st, rowptr_dst, num_queries, rows.part,
                 rows.part_plane, nd, out, d1, d2);
    GAOT_LAUNCH_CHECK();
    return GAOT_OK;
}
