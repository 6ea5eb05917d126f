// Fused PointNet GeometricEmbedding (reference src/model/layers/geoembed.py:184-222):
//     pooled[q] = max | mean over the edges e of query q of  relu(W2 relu(W1 (source_pos[src_e] - query_pos[q]) + b1) + b2)
// with W1 [32][D] (D = 1..3 coordinates), W2 [32][32], and its autograd.  No per-edge tensor reaches HBM: the general path
// (edgeops.hip + the GEMM kernels) writes the [E,3] offsets and two [E,32] hidden tensors and reads them back, and its
// backward builds two more [E,32] gradients; here the forward keeps only pooled (+ the arg-max edge per (row, channel))
// and the backward recomputes the hidden layers per edge.  Exact fp32 throughout, fixed summation orders, no atomics.
//
// Mapping.  Edges are in the dst-sorted order of gaot_csr_build, so a query's edges are the contiguous range
// rowptr[q] .. rowptr[q+1].  Workgroup b owns the rows whose FIRST edge lies in [b * span, (b+1) * span) (two binary searches
// in rowptr per workgroup, on the device); its edges are then one contiguous row-aligned range and no row is shared between
// workgroups -- a hub row of thousands of edges belongs to one workgroup, rows without edges belong to the workgroup their
// rowptr value falls into (trailing ones to the last).  The range is walked in tiles of 256 edges, one lane per edge:
//   * a lane forms d, h1 (registers) and h2 with the weights read by scalar loads (wave-uniform addresses, constant address
//     space) straight into the FMAs' SGPR operands;
//   * h2 goes through an LDS tile [edge][32 + 1] to (row, channel) walkers that keep the running max / arg / sum of a
//     row in edge order; a row that continues in the next tile hands its state on through a small LDS carry
//     (double-buffered: the walker that reads a carry and the one that writes the next may differ).
// Backward: the same tiles.  dW2 = sum_e dz2_e (x) h1_e is a product over the edge axis: both factors go through per-wave
// LDS tiles and are read back edge-on-half-wave / channel-on-lane as the operands of v_mfma_f32_32x32x2_f32 (exact fp32,
// a k-ordered fmaf chain); dW1, db1, db2 are lane sums in the same layout.  A workgroup keeps its sums in registers over
// all of its tiles and leaves ONE flat partial row [dW1 | db1 | dW2 | db2]; gaot_reduce_multi completes them in the call.
#include "common.h"

namespace {

constexpr int PN_H = 32;             // width of both layers
constexpr int PN_T = 256;            // edges per tile = threads per workgroup
constexpr int PN_LD = PN_H + 1;      // row stride of the LDS tiles (a column read then touches 32 distinct banks)
constexpr int PN_FWD_GRID = 2048;    // most workgroups of a forward launch
constexpr int PN_BWD_PARTS = 512;    // most workgroups = partial rows of a backward launch, whatever E is
constexpr int PN_MEAN = 1, PN_MAX = 2;   // gaot_segment_reduce's mode codes

struct PnArgs {
    const float* sp; const float* qp;                 // source_pos [S, D], query_pos [Q, D]
    const int* rowptr; const int* src; const int* dst;   // by-query neighbour list: rowptr [Q+1], source and query of every edge
    int Q, E;
    const float* w1; const float* b1; const float* w2; const float* b2;
    long long span;                                    // edges per workgroup, a multiple of PN_T
};

// the weights are read through the constant address space at wave-uniform indices: scalar loads into SGPRs that feed the FMAs
// directly, no LDS staging (as LDS broadcasts the forward measured 5 % slower on the encoder graph of configs[1])
// The scalar cache is not coherent with stores of a running kernel; it is invalidated between launches, which is when the optimizer
// rewrites the weights.  A kernel that updated them itself could not read them this way.
typedef const float __attribute__((address_space(4))) * pn_cptr;
__device__ __forceinline__ pn_cptr pn_const(const float* p) { return (pn_cptr)(uintptr_t)p; }

__host__ __device__ constexpr int pn_nparams(int d) { return PN_H * d + PN_H + PN_H * PN_H + PN_H; }

// first row r in [0, Q] with rowptr[r] >= s (Q when there is none among the rows 0 .. Q-1)
__device__ __forceinline__ int pn_first_row(const int* __restrict__ rowptr, int Q, long long s) {
    int lo = 0, hi = Q;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (rowptr[mid] < s) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the rows [r_lo, r_hi) this workgroup owns (wave-uniform values)
__device__ __forceinline__ void pn_rows(const PnArgs& a, int& r_lo, int& r_hi) {
    const long long s0 = (long long)blockIdx.x * a.span;
    r_lo = __builtin_amdgcn_readfirstlane(pn_first_row(a.rowptr, a.Q, s0));
    r_hi = blockIdx.x + 1 == gridDim.x ? a.Q : __builtin_amdgcn_readfirstlane(pn_first_row(a.rowptr, a.Q, s0 + a.span));
}

// d = source_pos[src] - query_pos[q] (subtract first), z1 = W1 d + b1
template <int D>
__device__ __forceinline__ void pn_layer1(const PnArgs& a, int e, pn_cptr w1s, pn_cptr b1s, float (&d)[D], float (&z1)[PN_H]) {
    const float* s = a.sp + (long long)a.src[e] * D;
    const float* q = a.qp + (long long)a.dst[e] * D;
#pragma unroll
    for (int i = 0; i < D; ++i) d[i] = s[i] - q[i];
#pragma unroll
    for (int j = 0; j < PN_H; ++j) {
        float z = b1s[j];
#pragma unroll
        for (int i = 0; i < D; ++i) z = fmaf(w1s[j * D + i], d[i], z);
        z1[j] = z;
    }
}

// z2[c] = W2[c][:] h1 + b2[c], the row of W2 left in w[] for the caller
__device__ __forceinline__ float pn_layer2_row(pn_cptr w2s, pn_cptr b2s, int c, const float (&h1)[PN_H], float (&w)[PN_H]) {
#pragma unroll
    for (int k = 0; k < PN_H; ++k) w[k] = w2s[c * PN_H + k];
    float z = b2s[c];
#pragma unroll
    for (int k = 0; k < PN_H; ++k) z = fmaf(w[k], h1[k], z);
    return z;
}

template <int D, int MODE>
__global__ __launch_bounds__(PN_T) void k_pointnet_fwd(PnArgs a, float* __restrict__ pooled, int* __restrict__ argmax) {
    __shared__ float tile[PN_T * PN_LD];
    __shared__ float cval[2][PN_H];
    __shared__ int carg[2][PN_H];
    const int tid = threadIdx.x;
    const pn_cptr w1s = pn_const(a.w1), b1s = pn_const(a.b1), w2s = pn_const(a.w2), b2s = pn_const(a.b2);
    int r_lo, r_hi;
    pn_rows(a, r_lo, r_hi);
    if (r_lo >= r_hi) return;
    const int e_hi = a.rowptr[r_hi];
    int r_cur = r_lo, par = 0;
    for (int t0 = a.rowptr[r_lo];; t0 += PN_T) {
        const int n = min(PN_T, e_hi - t0);          // 0: the workgroup owns rows without edges only
        if (tid < n) {
            float d[D], h1[PN_H], w[PN_H];
            pn_layer1<D>(a, t0 + tid, w1s, b1s, d, h1);
#pragma unroll
            for (int j = 0; j < PN_H; ++j) h1[j] = fmaxf(h1[j], 0.f);
#pragma unroll 2
            for (int c = 0; c < PN_H; ++c) tile[tid * PN_LD + c] = fmaxf(pn_layer2_row(w2s, b2s, c, h1, w), 0.f);
        }
        __syncthreads();
        // the rows that start before the end of this tile: up to the row of its last edge (the last tile: all that are left)
        const bool last = t0 + n >= e_hi;
        const int t1 = t0 + n;
        const int r_end = last ? r_hi : a.dst[t1 - 1] + 1;
        const int c = tid & 31;
        for (int r = r_cur + (tid >> 5); r < r_end; r += PN_T / 32) {
            const int lo = a.rowptr[r], hi = a.rowptr[r + 1];
            const int jb = min(hi, t1) - t0;       // positions inside the tile
            int j = max(lo, t0) - t0;
            float best = 0.f;     // max: running maximum; mean: running sum
            int arg = -1;         // max: position of `best` in the dst-sorted edge order
            if (lo < t0) { best = cval[par][c]; arg = carg[par][c]; }      // the row began in an earlier tile
            const float* col = tile + c;
            for (; j + 4 <= jb; j += 4) {           // four loads in flight, then the updates in edge order
                const float v0 = col[j * PN_LD], v1 = col[(j + 1) * PN_LD], v2 = col[(j + 2) * PN_LD], v3 = col[(j + 3) * PN_LD];
                if (MODE == PN_MAX) {
                    if (arg < 0 || v0 > best) { best = v0; arg = t0 + j; }
                    if (v1 > best) { best = v1; arg = t0 + j + 1; }
                    if (v2 > best) { best = v2; arg = t0 + j + 2; }
                    if (v3 > best) { best = v3; arg = t0 + j + 3; }
                } else {
                    best = (((best + v0) + v1) + v2) + v3;
                }
            }
            for (; j < jb; ++j) {
                const float v = col[j * PN_LD];
                if (MODE == PN_MAX) {
                    if (arg < 0 || v > best) { best = v; arg = t0 + j; }      // the first maximal edge wins (k_segment_reduce)
                } else {
                    best += v;
                }
            }
            if (hi <= t1) {
                const long long o = (long long)r * PN_H + c;
                if (MODE == PN_MAX) { pooled[o] = best; argmax[o] = arg; }
                else pooled[o] = best / (float)max(hi - lo, 1);
            } else {                                 // the row goes on in the next tile
                cval[par ^ 1][c] = best;
                carg[par ^ 1][c] = arg;
            }
        }
        if (last) break;
        r_cur = a.rowptr[r_end] > t1 ? r_end - 1 : r_end;
        par ^= 1;
        __syncthreads();
    }
}

// LDS of the backward kernel, in floats
constexpr int PN_WTILE = 64 * PN_LD;                                        // one wave's [64 edges][32 + 1] tile
constexpr int PN_BWD_LDS = PN_T * 4 + PN_T * 3 + 2 * 4 + 8 * PN_WTILE;
static_assert(4 * pn_nparams(3) <= 8 * PN_WTILE, "the waves' partial sums reuse the tiles");

template <int D, int MODE>
__global__ __launch_bounds__(PN_T) void k_pointnet_bwd(PnArgs a, const float* __restrict__ dpool, const int* __restrict__ argmax,
                                                        float* __restrict__ wpart, float* __restrict__ d_query,
                                                        float* __restrict__ d_edge) {
    constexpr int NP = pn_nparams(D);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* dts = smem;                  // d per edge of the tile [256][4]
    float* ddt = dts + PN_T * 4;        // W1^T dz1 per edge of the tile [256][3]
    float* cq = ddt + PN_T * 3;         // carry of the d_query walker [2][4]
    float* tiles = cq + 2 * 4;          // per wave: tile A (h1, then dz1) and tile B (dz2)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    float* tA = tiles + wave * 2 * PN_WTILE;
    float* tB = tA + PN_WTILE;
    const pn_cptr w1s = pn_const(a.w1), b1s = pn_const(a.b1), w2s = pn_const(a.w2), b2s = pn_const(a.b2);
    f32x16 dw2;       // dW2[c = mfma32_row(r, hf)][k = l31] over this wave's edges
#pragma unroll
    for (int r = 0; r < 16; ++r) dw2[r] = 0.f;
    float db2 = 0.f, db1 = 0.f, dw1[D];     // channel l31, over the wave's edges of parity hf
#pragma unroll
    for (int i = 0; i < D; ++i) dw1[i] = 0.f;
    int r_lo, r_hi;
    pn_rows(a, r_lo, r_hi);
    if (r_lo < r_hi) {
        const int e_hi = a.rowptr[r_hi];
        int r_cur = r_lo, par = 0;
        for (int t0 = a.rowptr[r_lo];; t0 += PN_T) {
            const int n = min(PN_T, e_hi - t0);
            const int t1 = t0 + n;
            const bool valid = tid < n;
            const int e = t0 + tid;
            // ---- lane = edge: d, h1, z2 -> dz2, dh1 = W2^T dz2.  A lane past the end carries dz2 = 0, so it adds nothing anywhere
            float d[D], h1[PN_H], dh1[PN_H];
            unsigned m1 = 0;             // bit j: z1[j] > 0
            int q = 0;
            float inv = 0.f;
#pragma unroll
            for (int i = 0; i < D; ++i) d[i] = 0.f;
#pragma unroll
            for (int j = 0; j < PN_H; ++j) h1[j] = 0.f;
            if (valid) {
                q = a.dst[e];
                pn_layer1<D>(a, e, w1s, b1s, d, h1);
#pragma unroll
                for (int j = 0; j < PN_H; ++j) {
                    if (h1[j] > 0.f) m1 |= 1u << j; else h1[j] = 0.f;
                }
                if (MODE == PN_MEAN) inv = 1.0f / (float)(a.rowptr[q + 1] - a.rowptr[q]);
            }
#pragma unroll
            for (int j = 0; j < PN_H; ++j) { tA[lane * PN_LD + j] = h1[j]; dh1[j] = 0.f; }
#pragma unroll
            for (int i = 0; i < D; ++i) dts[tid * 4 + i] = d[i];
            const float* dp = dpool + (long long)q * PN_H;
            const int* ap = argmax + (long long)q * PN_H;       // max mode only
            for (int c0 = 0; c0 < PN_H; c0 += 4) {
                float g[4] = {0.f, 0.f, 0.f, 0.f};
                if (valid) {
                    const float4 gv = *reinterpret_cast<const float4*>(dp + c0);
                    if (MODE == PN_MAX) {
                        const int4 av = *reinterpret_cast<const int4*>(ap + c0);
                        g[0] = av.x == e ? gv.x : 0.f; g[1] = av.y == e ? gv.y : 0.f;
                        g[2] = av.z == e ? gv.z : 0.f; g[3] = av.w == e ? gv.w : 0.f;
                    } else {
                        g[0] = gv.x * inv; g[1] = gv.y * inv; g[2] = gv.z * inv; g[3] = gv.w * inv;
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float w[PN_H];
                    const float z2 = pn_layer2_row(w2s, b2s, c0 + u, h1, w);
                    const float dz = z2 > 0.f ? g[u] : 0.f;
                    tB[lane * PN_LD + c0 + u] = dz;
#pragma unroll
                    for (int k = 0; k < PN_H; ++k) dh1[k] = fmaf(w[k], dz, dh1[k]);
                }
            }
            __syncthreads();
            // ---- lane = (edge parity hf, channel l31): dW2 += dz2 (x) h1 two edges per MFMA, db2 += dz2
#pragma unroll 8
            for (int i = 0; i < 32; ++i) {
                const float av = tB[(2 * i + hf) * PN_LD + l31], bv = tA[(2 * i + hf) * PN_LD + l31];
                dw2 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, dw2, 0, 0, 0);
                db2 += av;
            }
            __syncthreads();
            // ---- lane = edge: dz1 = dh1 (z1 > 0) -> tile A; dd = W1^T dz1
            float dd[D];
#pragma unroll
            for (int i = 0; i < D; ++i) dd[i] = 0.f;
#pragma unroll
            for (int j = 0; j < PN_H; ++j) {
                const float dz = (m1 >> j) & 1u ? dh1[j] : 0.f;
                tA[lane * PN_LD + j] = dz;
#pragma unroll
                for (int i = 0; i < D; ++i) dd[i] = fmaf(w1s[j * D + i], dz, dd[i]);
            }
#pragma unroll
            for (int i = 0; i < D; ++i) ddt[tid * 3 + i] = dd[i];
            if (d_edge && valid) {
#pragma unroll
                for (int i = 0; i < D; ++i) d_edge[(long long)e * D + i] = dd[i];
            }
            __syncthreads();
            // ---- lane = (edge parity, channel): db1 += dz1, dW1 += dz1 (x) d
#pragma unroll 8
            for (int i = 0; i < 32; ++i) {
                const int ee = 2 * i + hf;
                const float av = tA[ee * PN_LD + l31];
                db1 += av;
#pragma unroll
                for (int x = 0; x < D; ++x) dw1[x] = fmaf(av, dts[(wave * 64 + ee) * 4 + x], dw1[x]);
            }
            const bool last = t1 >= e_hi;
            if (d_query) {
                // d_query[r] = -sum of dd over the row's edges, in edge order; one thread per row, state carried across tiles
                const int r_end = last ? r_hi : a.dst[t1 - 1] + 1;
                for (int r = r_cur + tid; r < r_end; r += PN_T) {
                    const int lo = a.rowptr[r], hi = a.rowptr[r + 1];
                    const int jb = min(hi, t1);
                    float s[D];
#pragma unroll
                    for (int i = 0; i < D; ++i) s[i] = lo < t0 ? cq[par * 4 + i] : 0.f;
                    for (int j = max(lo, t0); j < jb; ++j) {
#pragma unroll
                        for (int i = 0; i < D; ++i) s[i] += ddt[(j - t0) * 3 + i];
                    }
                    if (hi <= t1) {
#pragma unroll
                        for (int i = 0; i < D; ++i) d_query[(long long)r * D + i] = 0.f - s[i];
                    } else {
#pragma unroll
                        for (int i = 0; i < D; ++i) cq[(par ^ 1) * 4 + i] = s[i];
                    }
                }
                if (!last) r_cur = a.rowptr[r_end] > t1 ? r_end - 1 : r_end;
                par ^= 1;
            }
            if (last) break;
            __syncthreads();
        }
    }
    // ---- the four waves' sums, added in wave order, leave as this workgroup's partial row [dW1 | db1 | dW2 | db2]
    __syncthreads();
    float* mine = tiles + wave * NP;
    db1 += __shfl_xor(db1, 32, 64);
    db2 += __shfl_xor(db2, 32, 64);
#pragma unroll
    for (int i = 0; i < D; ++i) dw1[i] += __shfl_xor(dw1[i], 32, 64);
    if (hf == 0) {
#pragma unroll
        for (int i = 0; i < D; ++i) mine[l31 * D + i] = dw1[i];
        mine[PN_H * D + l31] = db1;
        mine[PN_H * D + PN_H + PN_H * PN_H + l31] = db2;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) mine[PN_H * D + PN_H + mfma32_row(r, hf) * PN_H + l31] = dw2[r];
    __syncthreads();
    for (int i = tid; i < NP; i += PN_T)
        wpart[(long long)blockIdx.x * NP + i] = ((tiles[i] + tiles[NP + i]) + tiles[2 * NP + i]) + tiles[3 * NP + i];
}

// workgroups of a launch over E edges (at most `cap`) and the edges each of them spans
int pn_grid(int64_t E, int cap, long long* span) {
    const int64_t tiles = std::max<int64_t>(1, ceil_div(E, PN_T));
    const int64_t per = ceil_div(tiles, std::min<int64_t>(tiles, cap));   // tiles per workgroup
    *span = per * PN_T;
    return (int)ceil_div(tiles, per);       // no workgroup without a span of its own (513 tiles under a cap of 512: 257, not 512)
}

int pn_check(const float* source_pos, const float* query_pos, int coord_dim, const int32_t* rowptr, const int32_t* src,
             const int32_t* dst, int64_t Q, int64_t E, const float* w1, const float* b1, const float* w2, const float* b2,
             int mode, const void* argmax) {
    GAOT_CHECK_ARG(coord_dim >= 1 && coord_dim <= 3, "coord_dim must be 1, 2 or 3");
    GAOT_CHECK_ARG(mode == PN_MEAN || mode == PN_MAX, "mode must be 1 (mean) or 2 (max)");
    GAOT_CHECK_ARG(Q >= 0 && E >= 0 && Q < 0x7fffffff && E < 0x7fffffff, "bad size");
    GAOT_CHECK_ARG(Q > 0 || E == 0, "edges without queries");
    GAOT_CHECK_ARG(mode != PN_MAX || argmax || Q == 0, "max pooling needs argmax");
    if (E > 0) {
        GAOT_CHECK_ARG(source_pos && query_pos && rowptr && src && dst && w1 && b1 && w2 && b2, "null pointer");
    }
    return GAOT_OK;
}

#define PN_DISPATCH(D_, MODE_, CALL)                                                            \
    switch ((D_) * 4 + (MODE_)) {                                                               \
        case 1 * 4 + PN_MEAN: { constexpr int D = 1, MODE = PN_MEAN; CALL; } break;            \
        case 1 * 4 + PN_MAX: { constexpr int D = 1, MODE = PN_MAX; CALL; } break;              \
        case 2 * 4 + PN_MEAN: { constexpr int D = 2, MODE = PN_MEAN; CALL; } break;            \
        case 2 * 4 + PN_MAX: { constexpr int D = 2, MODE = PN_MAX; CALL; } break;              \
        case 3 * 4 + PN_MEAN: { constexpr int D = 3, MODE = PN_MEAN; CALL; } break;            \
        default: { constexpr int D = 3, MODE = PN_MAX; CALL; } break;                          \
    }

template <int D, int MODE>
int pn_bwd_launch(const PnArgs& a, int grid, const float* dpool, const int* argmax, float* wpart, float* d_query, float* d_edge,
                  hipStream_t st) {
    constexpr size_t lds = sizeof(float) * PN_BWD_LDS;       // > 64 KB: dynamic
    auto kern = k_pointnet_bwd<D, MODE>;
    // on every launch: the attribute belongs to the current device, and a cached flag would not be safe between host threads
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
        gaot_set_error("gaot_pointnet_bwd: cannot set dynamic LDS %zu: %s", lds, hipGetErrorString(e));
        return GAOT_ERR_LAUNCH;
    }
    GAOT_KLAUNCH(kern, dim3(grid), dim3(PN_T), lds, st, a, dpool, argmax, wpart, d_query, d_edge);
    return GAOT_OK;
}

}  // namespace

extern "C" int gaot_pointnet_fwd(const float* source_pos, const float* query_pos, int coord_dim, const int32_t* rowptr_dst,
                                 const int32_t* src_sorted, const int32_t* dst_sorted, int64_t num_queries, int64_t num_edges,
                                 const float* w1, const float* b1, const float* w2, const float* b2, int mode, float* pooled,
                                 int32_t* argmax, gaot_stream_t stream) {
    GAOT_ENTER();
    if (int rc = pn_check(source_pos, query_pos, coord_dim, rowptr_dst, src_sorted, dst_sorted, num_queries, num_edges, w1, b1, w2,
                          b2, mode, argmax))
        return rc;
    if (num_queries == 0) return GAOT_OK;
    GAOT_CHECK_ARG(pooled, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (num_edges == 0) {      // every row is empty: zeros and -1, nothing walks the lists
        if (hipMemsetAsync(pooled, 0, sizeof(float) * (size_t)num_queries * PN_H, st) != hipSuccess ||
            (argmax && hipMemsetAsync(argmax, 0xff, sizeof(int32_t) * (size_t)num_queries * PN_H, st) != hipSuccess)) {
            gaot_set_error("gaot_pointnet_fwd: memset failed");
            return GAOT_ERR_LAUNCH;
        }
        return GAOT_OK;
    }
    PnArgs a{source_pos, query_pos, rowptr_dst, src_sorted, dst_sorted, (int)num_queries, (int)num_edges, w1, b1, w2, b2, 0};
    const int grid = pn_grid(num_edges, PN_FWD_GRID, &a.span);
    PN_DISPATCH(coord_dim, mode, GAOT_KLAUNCH((k_pointnet_fwd<D, MODE>), dim3(grid), dim3(PN_T), 0, st, a, pooled, argmax));
    GAOT_LAUNCH_CHECK();
    return GAOT_OK;
}

extern "C" int64_t gaot_pointnet_bwd_parts(int64_t num_edges) {
    long long span;
    return pn_grid(std::max<int64_t>(num_edges, 0), PN_BWD_PARTS, &span);
}

extern "C" int gaot_pointnet_bwd(const float* source_pos, const float* query_pos, int coord_dim, const int32_t* rowptr_dst,
                                 const int32_t* src_sorted, const int32_t* dst_sorted, int64_t num_queries, int64_t num_edges,
                                 const float* w1, const float* b1, const float* w2, const float* b2, int mode,
                                 const float* d_pooled, const int32_t* argmax, float* d_params, float* d_query,
                                 float* d_edge_offset, void* workspace, size_t workspace_bytes, gaot_stream_t stream) {
    GAOT_ENTER();
    if (int rc = pn_check(source_pos, query_pos, coord_dim, rowptr_dst, src_sorted, dst_sorted, num_queries, num_edges, w1, b1, w2,
                          b2, mode, argmax))
        return rc;
    GAOT_CHECK_ARG(d_params, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int np = pn_nparams(coord_dim);
    if (num_edges == 0) {      // no edge: every gradient is zero
        if (hipMemsetAsync(d_params, 0, sizeof(float) * (size_t)np, st) != hipSuccess ||
            (d_query && num_queries > 0 &&
             hipMemsetAsync(d_query, 0, sizeof(float) * (size_t)num_queries * coord_dim, st) != hipSuccess)) {
            gaot_set_error("gaot_pointnet_bwd: memset failed");
            return GAOT_ERR_LAUNCH;
        }
        return GAOT_OK;
    }
    PnArgs a{source_pos, query_pos, rowptr_dst, src_sorted, dst_sorted, (int)num_queries, (int)num_edges, w1, b1, w2, b2, 0};
    const int grid = pn_grid(num_edges, PN_BWD_PARTS, &a.span);
    GAOT_CHECK_ARG(d_pooled, "null pointer");
    GAOT_CHECK_ARG((((uintptr_t)d_pooled | (uintptr_t)argmax) & 15) == 0, "d_pooled and argmax must be 16-byte aligned");
    GAOT_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= sizeof(float) * (size_t)grid * np,
                   "workspace: gaot_pointnet_bwd_parts(num_edges) rows of 32 * coord_dim + 1088 floats, 16-byte aligned");
    float* wpart = (float*)workspace;
    int rc = GAOT_OK;
    PN_DISPATCH(coord_dim, mode, rc = (pn_bwd_launch<D, MODE>(a, grid, d_pooled, argmax, wpart, d_query, d_edge_offset, st)));
    if (rc != GAOT_OK) return rc;
    GAOT_LAUNCH_CHECK();
    const gaot_reduce_desc_t desc = {wpart, d_params, np, grid, 32};
    return gaot_reduce_multi(&desc, 1, stream);
}
