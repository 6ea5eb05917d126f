// Pieces shared by the fp32 (gno.hip) and bf16 (gno_bf16.hip) GNO kernels: the per-lane segmented walk over a
// 32-edge LDS tile, the tile-ordered fix-up of rows that straddle tiles, small structs.
#pragma once
#include <type_traits>

#include "common.h"

namespace gno {

constexpr int IN0 = 6;      // [y_pos(3), x_pos(3)]
constexpr int IN0P = 8;     // padded

// the single argument of a (possibly empty) parameter pack: optional kernel outputs whose absence leaves the kernel's argument
// list as it was
template <class T, class... R>
__device__ __forceinline__ T first_arg(T t, R...) { return t; }
template <class T>
__device__ __forceinline__ T last_arg(T t) { return t; }
template <class T, class U, class... R>
__device__ __forceinline__ auto last_arg(T, U u, R... r) { return last_arg(u, r...); }

// transform_type of the integral transform (reference integral_transform.py:146-157), a compile-time mode of the kernels:
//   LINEAR      k = MLP([y_s, x_q]),         out_q = mean k * f_y[s]
//   NONLINEAR   k = MLP([y_s, x_q, f_y[s]]), out_q = mean k * f_y[s]
//   KERNELONLY  k = MLP([y_s, x_q, f_y[s]]), out_q = mean k
// In the two new modes layer 0 is z_0 = W_0c [y_s, x_q] + b_0 + t[s] with the per-NODE product t = W_0f f_y ([N_y][64] fp32,
// formed once on the row-linear kernels): an edge's layer-0 accumulator starts from b_0 + t[src] instead of b_0.  The backward
// also returns dt[s] = sum_{e: src = s} dz_0[e] ([N_y][64] fp32, from the unrounded dz_0), a segmented sum over the source-sorted
// edge list like grad f_y; dW_0f = dt^T f_y and grad f_y += dt W_0f are the caller's per-node products.
enum { MODE_LINEAR = 0, MODE_NONLINEAR = 1, MODE_KERNELONLY = 2 };
constexpr int NLH = 64;     // row width of t / dt
// the extra operands of the two new modes, passed as the last kernel argument (a parameter pack that is empty in linear mode, so
// those instantiations keep today's kernel arguments)
struct NlFwd {
    const float* t;         // [N_y][64]
};
struct NlBwd {
    const float* t;         // [N_y][64]
    float* dt;              // [N_y][64]
    float* part_dt;         // two 64-float slots per tile: rows of dt that straddle tiles (k_segment_fixup<64, ..>)
};

// WEIGHTED variant (the attention-weighted transform, use_attn): out_q = sum_{e -> q} alpha_e k_e * f_y[s_e] with an fp32 weight per
// edge instead of the mean's 1/deg.  Every per-edge scalar at the ABI is in the DST-sorted edge order: the forward, which walks that
// list, reads alpha at its own edge index; the backward, which walks the source-sorted list, reads alpha and writes
//   dalpha_e = sum_c grad_out[q_e][c] k_e[c] f_y[s_e][c]        (kernel-only mode: without f; the UNWEIGHTED grad_out)
// through the src -> dst position map, each edge exactly once.  The operands ride in the same parameter packs: WFwd LAST in the
// forward's pack, WBwd FIRST in the backward's (before the NlBwd of the nonlinear modes; never together with a coordinate output),
// so first_arg / last_arg keep finding what they found and the unweighted instantiations keep their arguments and instructions.
struct WFwd {
    const float* alpha;     // [E], dst-sorted
};
struct WBwd {
    const float* alpha;     // [E], dst-sorted
    const int* s2d;         // [E]: position in the source-sorted order -> position in the dst-sorted order
    float* dalpha;          // [E], dst-sorted; null: not wanted
};
// REGULAR-LIST variant of the forward (gaot_gno_fwd_knn): every query has exactly k = 2^lk neighbours, k | 32, listed as
// nbr[q*k + j] -- the out_idx of gaot_knn_grid, which IS the by-query list of a k-nearest graph (rowptr[q] = q k, dst[e] = e / k, rows
// in the order a stable sort keeps).  The kernel reads its source ids from nbr, takes the query of edge e as e >> lk and loads no
// dst_sorted / rowptr; no row is empty or straddles a 32-edge tile, so the rows are finished in the tile (fixed_k_rows below: no
// partial buffer, no fix-up launch).  A KnnFwd ENDS the forward's pack (after the NlFwd of the nonlinear modes; never with a WFwd);
// those instantiations are passed null src_s / dst_s / rowptr / part and E = num_queries * k.
struct KnnFwd {
    const int* nbr;         // [num_queries * k]
    int lk;                 // log2(k), 0..5
};
// ADJOINT variant of the linear forward (gaot_gno_adj): the transform out_q = (1/deg q) sum_e k_e * f[s_e] is linear in f, and its
// adjoint  df[t] = sum_{e: src_e = t} k_e * g[q_e] / deg(q_e)  is the same per-edge kernel MLP evaluated forward once, reduced by SOURCE
// instead of by query: the kernel walks the SOURCE-sorted list (src_s = the segment key, dst_s = the query whose coordinates feed
// the MLP and whose cotangent row is gathered through the f_y argument), scales the staged value by 1/deg(q_e) -- from the by-query
// offsets, or the constant 1/k of a regular list when they are null -- and sums the rows (segment_walk, mean = false).  An AdjFwd
// ENDS the forward's pack (linear mode only; never with a WFwd or a KnnFwd).
struct AdjFwd {
    const int* rowptr_dst;  // [num_queries + 1]; null: every query has k edges
    float inv_k;            // 1 / k of a regular list (read when rowptr_dst is null)
};
template <class T, class... P>
constexpr bool pack_has = (std::is_same_v<T, P> || ...);

__device__ __forceinline__ void wave_lds_fence() {
    // LDS ops of one wave execute in order; this only stops the compiler from reordering.
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// gelu_fast's value (its own expression: bit-identical) and gelu_fast_pair's derivative; t, p, e are shared.  The activation of the
// forward-mode kernels (gno_jac.hip, gno_jac_adj.hip)
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

// x, as a value the optimiser cannot trace: keeps the recomputation of gelu' / gelu'' from z_l INSIDE the direction loop (hoisted out
// of it as loop-invariant, the derivatives of every layer are live across the loop again and the kernel spills).  The jet kernels
// (gno_jet2.hip, gno_jet2_adj.hip)
__device__ __forceinline__ float opaque(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

// gelu_fast's value (its own expression: bit-identical), gelu_fast_pair's derivative (gelu_fast_tangent above) and the second
// derivative phi(x) (2 - x^2); t, p, e are shared.  The activation jet of gno_jet2.hip and gno_jet2_adj.hip
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

struct MlpPtrs {
    const float* w[GAOT_MAX_MLP_LAYERS];
    const float* b[GAOT_MAX_MLP_LAYERS];
};
struct MlpGradPtrs {
    float* w[GAOT_MAX_MLP_LAYERS];
    float* b[GAOT_MAX_MLP_LAYERS];
};

// Per-lane walk over one 32-edge tile staged in LDS as stage[e*ld + c]: lane = channel c.
// Complete rows are stored (mean or sum); rows open to the left go to part slot 0, rows open only
// to the right to slot 1 (combined later by k_segment_fixup in tile order).
template <int C>
__device__ __forceinline__ void segment_walk(const float* stage, int ld, const int* ids, int c, int64_t tbase,
                                             const int* __restrict__ rowptr, float* __restrict__ out,
                                             float* __restrict__ part, bool mean) {
    const int64_t tile = tbase >> 5;
    int cur = ids[0];
    float sum = 0.f;
    auto flush = [&](int q, float s) {
        if (q < 0) return;
        const int rb = rowptr[q], re = rowptr[q + 1];
        const bool ol = rb < tbase, orr = re > tbase + 32;
        if (!ol && !orr) {
            out[(int64_t)q * C + c] = mean ? s / (float)(re - rb) : s;
        } else if (ol) {
            part[(tile * 2 + 0) * C + c] = s;
        } else {
            part[(tile * 2 + 1) * C + c] = s;
        }
    };
#pragma unroll 4
    for (int e = 0; e < 32; ++e) {
        const int d = ids[e];
        if (d != cur) {
            flush(cur, sum);
            cur = d;
            sum = 0.f;
        }
        if (d >= 0) sum += stage[e * ld + c];
    }
    flush(cur, sum);
}

// The regular-list epilogue (KnnFwd): the 32 edges of a tile staged as stage[e*ld + c] are 32/k complete rows of k = 2^lk edges, the
// row that ends at edge e being query (tbase + e) >> lk.  Lane = channel c adds a row's k values in edge order starting from 0.f and
// divides by (float)k: the operations, in the order, that segment_walk performs on a complete row of degree k, so the two agree bit
// for bit.  E is a multiple of k: a row lies wholly below E or wholly at / above it (not stored).
template <int C>
__device__ __forceinline__ void fixed_k_rows(const float* stage, int ld, int c, int64_t tbase, int lk, int64_t E,
                                             float* __restrict__ out) {
    const int km1 = (1 << lk) - 1;
    const float fk = (float)(1 << lk);
    float sum = 0.f;
#pragma unroll 4
    for (int e = 0; e < 32; ++e) {
        sum += stage[e * ld + c];
        if ((e & km1) == km1) {
            if (tbase + e < E) out[((tbase + e) >> lk) * C + c] = sum / fk;
            sum = 0.f;
        }
    }
}

// rows with no edges -> 0; rows spanning several tiles -> ordered sum of the tile partials (tiles of 2^SHIFT edges: 32
// for the forward and the fp32 backward, 16 for the bf16 backward, whose waves own 16-edge tiles)
template <int C, int SHIFT = 5>
__global__ void k_segment_fixup(const int* __restrict__ rowptr, int64_t Q, const float* __restrict__ part,
                                float* __restrict__ out, int mean) {
    static_assert(C % 4 == 0, "four channels per thread");
    constexpr int TPR = C / 4;                                   // threads per row, 16 bytes each
    // grid-stride over (row, 16-byte column group): nearly every row lies inside one tile and needs nothing, so the pass is a scan
    // of rowptr -- launched as one thread per item it was bound by the rate at which workgroups start (8 M point rows: 250 K
    // workgroups, 333 / 623 us), not by the 32 MB it reads
    const int64_t n = Q * TPR, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t q = i / TPR;
        const int c = (int)(i % TPR) * 4;
        const int rb = rowptr[q], re = rowptr[q + 1];
        float4* o = reinterpret_cast<float4*>(out + q * C + c);
        if (re == rb) {
            *o = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const int t0 = rb >> SHIFT, t1 = (re - 1) >> SHIFT;
        if (t0 == t1) continue;
        float4 s = *reinterpret_cast<const float4*>(part + ((int64_t)t0 * 2 + 1) * C + c);
        for (int t = t0 + 1; t <= t1; ++t) {
            const float4 v = *reinterpret_cast<const float4*>(part + ((int64_t)t * 2 + 0) * C + c);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        if (mean) {
            const float d = (float)(re - rb);
            s.x /= d; s.y /= d; s.z /= d; s.w /= d;
        }
        *o = s;
    }
}
// grid of the fix-up pass: one thread per item up to 16 workgroups per CU, grid-stride beyond
inline unsigned segment_fixup_grid(int64_t items) {
    const int64_t b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace gno
