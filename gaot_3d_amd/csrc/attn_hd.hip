// Flash attention for every head size dh with dh % 4 == 0, 4 <= dh <= 128 in bf16 mode (reference GroupQueryFlashAttention.forward,
// src/model/layers/attn.py:110-127: head split, GQA repeat, F.scaled_dot_product_attention with no mask, scale
// 1/sqrt(head_dim), dropout on the attention weights) and its autograd.  Never an S x S tensor: every buffer is O(S * D).
//
// Operands are bf16 on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; the softmax runs in fp32 on exp2.  The kernels take the
// fused fp32 projection (q | k | v column blocks, already rotated) and convert to bf16 AT LOAD: when a tile is staged into
// LDS and when a wave reads its own rows into registers -- there is no packing pass and no bf16 copy in memory.  The scale
// is applied to the fp32 score, not to an operand, so forward and both backward passes see the same bf16 products.
//
// A wave owns 32 query rows (forward, dQ) or 32 keys (dK/dV); the other side streams through LDS in 32-row tiles.  As in
// csrc/attn.hip the first product of every chain is oriented so that its accumulator tile -- column on the lane, rows in
// the 16 registers -- is directly the B operand of the next one (the reduction index on the register axis), so P and dS
// never go through LDS:
//   forward : S^T[key][q] = K Q^T  ->  P^T (softmax over registers + one cross-half shuffle);  O^T[d][q] += V^T[d][key] P^T[key][q]
//   dK/dV   : S[q][key], dP[q][key] with the wave's keys on lanes;  dV^T += dO^T P,  dK^T += Q^T dS
//   dQ      : S^T, dP^T with the wave's queries on lanes;            dQ^T += K^T dS^T
// A staged tile has up to two LDS images: rows [32][D + 8] (a fragment = 16 contiguous bytes of one row) for the products
// that sum over d, and the transpose [D][36] (a fragment = two 8-byte runs of one d row) for the products that sum over the
// tile's rows, in the permuted k order an accumulator tile has as an operand: element j of lane half h of k-step s is tile
// row 16 s + 8 (j >> 2) + 4 h + (j & 3).
// dQ has its own pass and dK / dV are summed inside one workgroup over heads and query tiles in a fixed order: no float
// atomics, two runs on the same inputs are bit-identical.  FLOPs: forward 4, dK/dV 8, dQ 6 S^2 D per head -- 18 S^2 D.
//
// Head width and tile width: the true head width dh is a runtime value (addressing is head * dh, the scale 1 / sqrt(dh) comes from
// the host); the tile width D in {32, 64, 96, 128} is a template parameter, the smallest instance >= dh.  dh == D runs the plain
// instances (PAD = false).  dh < D runs the padded ones (PAD = true): heads are adjacent in memory, so every float4 of columns >=
// dh is PREDICATED, never loaded and then zeroed -- an unpredicated load would read the neighbouring head's columns and, for the
// last head of v in the last row, run past the allocation.  The staged LDS images and the register fragments then hold exact
// zeros in the padding, so scores and delta are what the dh columns alone give, the accumulator rows >= dh stay zero, and the
// stores skip them (the next head's columns are not touched).  dh % 4 == 0 keeps every access 16-byte aligned.
#include "common.h"
#include "attn_dropout.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int TP = 36;      // pitch of a transposed image row (32 tile rows + 4): the 32 lanes' 8-byte reads hit 32 bank pairs

struct HdArgs {
    const float* q; const float* k; const float* v;
    float* o; float* lse;                       // lse: [B][H][S] natural log
    int64_t ldq, ldk, ldv, ldo;
    int B, S, H, HKV;
    float scale;
    gdrop::Drop drop;
    int dh;                                     // true head width (<= the tile width D of the instance)
};

struct HdBwdArgs {
    const float* q; const float* k; const float* v; const float* o; const float* d_o; const float* lse;
    float* delta;                                // [B][H][S]
    float* dq; float* dk; float* dv;
    int64_t ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    int B, S, H, HKV;
    float scale;
    gdrop::Drop drop;
    int dh;
};

__device__ __forceinline__ short f2bf(float f) {  // round-to-nearest-even
    const __bf16 b = (__bf16)f;
    return __builtin_bit_cast(short, b);
}
__device__ __forceinline__ uint32_t pk2(float a, float b) {
    return (uint32_t)(unsigned short)f2bf(a) | ((uint32_t)(unsigned short)f2bf(b) << 16);
}
__device__ __forceinline__ float bfr(float f) { return (float)(__bf16)f; }   // f as the matrix cores see it
__device__ __forceinline__ float xhalf(float v) { return __shfl_xor(v, 32, 64); }

// dropout words (csrc/attn_dropout.h), as in csrc/attn.hip -- the accumulator layout is the same: lanes that hold ONE query and the
// 32 keys of a tile in runs of 4 (forward, dQ) read their 8 key-pair words from bw_s; lanes that hold ONE key and runs of queries
// (dK/dV) read the row words of the tile's queries, split into halfword copies [parity][32].
using gdrop::stage_col_words;
using gdrop::keep_bits_cols;

// a [32][D] fp32 tile in flight from global memory to LDS: D / 32 float4 per thread of a 256-thread workgroup
template <int D>
struct Tile {
    float4 v[D / 32];
};
// (PAD: the float4s of columns >= dh are not read and stay zero)
template <int D, bool PAD>
__device__ __forceinline__ void tile_ld(Tile<D>& t, const float* __restrict__ base, int64_t ld, int64_t row0, int64_t nrows, int dh) {
#pragma unroll
    for (int e = 0; e < D / 32; ++e) {
        const int idx = threadIdx.x + 256 * e, r = idx / (D / 4), c4 = idx % (D / 4);
        t.v[e] = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (PAD) {
            if (row0 + r < nrows && 4 * c4 < dh) t.v[e] = *reinterpret_cast<const float4*>(base + (row0 + r) * ld + 4 * c4);
        } else {
            if (row0 + r < nrows) t.v[e] = *reinterpret_cast<const float4*>(base + (row0 + r) * ld + 4 * c4);
        }
    }
}
// rounds the tile to bf16 and writes its row image [32][D + 8] and / or its transposed image [D][TP]
template <int D, bool ROWS, bool TRANS>
__device__ __forceinline__ void tile_st(const Tile<D>& t, short* __restrict__ rows, short* __restrict__ trans) {
#pragma unroll
    for (int e = 0; e < D / 32; ++e) {
        const int idx = threadIdx.x + 256 * e, r = idx / (D / 4), c4 = idx % (D / 4);
        const float4 x = t.v[e];
        if constexpr (ROWS) *reinterpret_cast<uint2*>(rows + r * (D + 8) + 4 * c4) = make_uint2(pk2(x.x, x.y), pk2(x.z, x.w));
        if constexpr (TRANS) {
            trans[(4 * c4 + 0) * TP + r] = f2bf(x.x);
            trans[(4 * c4 + 1) * TP + r] = f2bf(x.y);
            trans[(4 * c4 + 2) * TP + r] = f2bf(x.z);
            trans[(4 * c4 + 3) * TP + r] = f2bf(x.w);
        }
    }
}
// fragment of k-step ks for a product that sums over d: row `row` of a row image, d = 16 ks + 8 hf .. + 7
template <int D>
__device__ __forceinline__ bf16x8 frag_rows(const short* rows, int row, int ks, int hf) {
    return *reinterpret_cast<const bf16x8*>(rows + row * (D + 8) + 16 * ks + 8 * hf);
}
// fragment of k-step s2 for a product that sums over the tile's rows against an accumulator tile: row `d` of a transposed
// image, tile rows 16 s2 + 4 hf .. + 3 and 16 s2 + 8 + 4 hf .. + 3
__device__ __forceinline__ bf16x8 frag_trans(const short* trans, int d, int s2, int hf) {
    typedef short s4 __attribute__((ext_vector_type(4)));
    const s4 lo = *reinterpret_cast<const s4*>(trans + d * TP + 16 * s2 + 4 * hf);
    const s4 hi = *reinterpret_cast<const s4*>(trans + d * TP + 16 * s2 + 8 + 4 * hf);
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// the wave's own rows as B fragments, straight from global memory: lane (l31, hf) holds d = 16 ks + 8 hf .. + 7 of row l31
// (PAD: each of the two float4s of a lane's 8-column run is read only if it lies below dh)
template <int D, bool PAD>
__device__ __forceinline__ void frags_ld(bf16x8 (&f)[D / 16], const float* __restrict__ rowp, bool valid, int hf, int dh) {
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
        if constexpr (PAD) {
            const int c = 16 * ks + 8 * hf;
            if (valid && c < dh) x = *reinterpret_cast<const float4*>(rowp + c);
            if (valid && c + 4 < dh) y = *reinterpret_cast<const float4*>(rowp + c + 4);
        } else if (valid) {
            x = *reinterpret_cast<const float4*>(rowp + 16 * ks + 8 * hf);
            y = *reinterpret_cast<const float4*>(rowp + 16 * ks + 8 * hf + 4);
        }
        f[ks] = bf16x8{f2bf(x.x), f2bf(x.y), f2bf(x.z), f2bf(x.w), f2bf(y.x), f2bf(y.y), f2bf(y.z), f2bf(y.w)};
    }
}
// an accumulator tile as the B operand of the next product: registers 8 s2 .. 8 s2 + 7 are k-step s2
__device__ __forceinline__ void acc_pack(const f32x16& x, bf16x8 (&b)[2]) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int j = 0; j < 8; ++j) b[s2][j] = f2bf(x[8 * s2 + j]);
}
__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}
// acc^T[d][lane] of one 32-wide d block -> row `p` (the lane's query or key), columns 32 t ..: four float4 per lane half
// (PAD: `ncols` = dh - 32 t columns of the block exist; the float4s at or past them belong to the next head and are not written)
template <bool PAD>
__device__ __forceinline__ void store_t(float* __restrict__ p, const f32x16& acc, float sc, int hf, int ncols) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if constexpr (PAD) {
            if (8 * g + 4 * hf >= ncols) continue;
        }
        *reinterpret_cast<float4*>(p + 8 * g + 4 * hf) = make_float4(acc[4 * g] * sc, acc[4 * g + 1] * sc, acc[4 * g + 2] * sc, acc[4 * g + 3] * sc);
    }
}

// ------------------------------------------------------------------------------------------------
// forward: block = 4 waves x 32 queries; grid (ceil(S/128), H, B)
// ------------------------------------------------------------------------------------------------
template <int D, bool PAD, bool DROP>
__global__ __launch_bounds__(256, 2) void k_attn_hd_fwd(HdArgs a) {
    constexpr int NS = D / 16, NT = D / 32;
    const int dh = PAD ? a.dh : D;
    __shared__ __attribute__((aligned(16))) short Ks[32 * (D + 8)];
    __shared__ __attribute__((aligned(16))) short Vt[D * TP];
    __shared__ uint32_t bw_s[16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hf = lane >> 5;
    const int head = blockIdx.y, b = blockIdx.z;
    const int hkv = head / (a.H / a.HKV);
    const int64_t q0 = (int64_t)blockIdx.x * 128 + wave * 32;
    const int64_t rowbase = (int64_t)b * a.S;
    const float* kp = a.k + rowbase * a.ldk + hkv * dh;
    const float* vp = a.v + rowbase * a.ldv + hkv * dh;
    const float sc = a.scale * LOG2E;
    const int64_t qi = q0 + l31;

    bf16x8 qf[NS];
    frags_ld<D, PAD>(qf, a.q + (rowbase + (qi < a.S ? qi : 0)) * a.ldq + head * dh, qi < a.S, hf, dh);
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = zero16();
    float m = -INFINITY, l = 0.f;
    uint32_t aw = 0, ck = 0;
    if constexpr (DROP) {
        const unsigned long long seed = *a.drop.seed;
        const int bh = a.drop.bh(b, head);
        aw = gdrop::row_word(gdrop::row_key(seed, bh), (uint32_t)qi);
        ck = gdrop::col_key(seed, bh);
    }

    Tile<D> kt, vt;
    tile_ld<D, PAD>(kt, kp, a.ldk, 0, a.S, dh);
    tile_ld<D, PAD>(vt, vp, a.ldv, 0, a.S, dh);
    for (int64_t k0 = 0; k0 < a.S; k0 += 32) {
        __syncthreads();
        tile_st<D, true, false>(kt, Ks, nullptr);
        tile_st<D, false, true>(vt, nullptr, Vt);
        if constexpr (DROP) stage_col_words(bw_s, ck, k0);
        __syncthreads();
        if (k0 + 32 < a.S) {
            tile_ld<D, PAD>(kt, kp, a.ldk, k0 + 32, a.S, dh);
            tile_ld<D, PAD>(vt, vp, a.ldv, k0 + 32, a.S, dh);
        }
        // S^T[key][q]
        f32x16 s = zero16();
#pragma unroll
        for (int ks = 0; ks < NS; ++ks)
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(Ks, l31, ks, hf), qf[ks], s, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] *= sc;
        if (k0 + 32 > a.S) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (k0 + mfma32_row(r, hf) >= a.S) s[r] = -INFINITY;
        }
        float mx = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
        mx = fmaxf(mx, xhalf(mx));
        const float mn = fmaxf(m, mx);
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = __builtin_amdgcn_exp2f(s[r] - mn);
            ps += s[r];
        }
        ps += xhalf(ps);
        l = l * alpha + ps;   // the normaliser is the UNdropped row sum
        m = mn;
        if constexpr (DROP) {
            const uint32_t kb = keep_bits_cols(aw, bw_s, hf, a.drop.thr);
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = ((kb >> r) & 1u) ? s[r] : 0.f;
        }
        bf16x8 pb[2];
        acc_pack(s, pb);
        // O^T[d][q] += V^T[d][key] P^T[key][q]
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] *= alpha;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_trans(Vt, 32 * t + l31, s2, hf), pb[s2], acc[t], 0, 0, 0);
        }
    }
    if (qi < a.S) {
        const float inv = DROP ? a.drop.inv_keep / l : 1.f / l;
        float* op = a.o + (rowbase + qi) * a.ldo + head * dh;
#pragma unroll
        for (int t = 0; t < NT; ++t) store_t<PAD>(op + 32 * t, acc[t], inv, hf, dh - 32 * t);
        if (hf == 0) a.lse[((int64_t)b * a.H + head) * a.S + qi] = m * LN2 + logf(l);
    }
}

// ------------------------------------------------------------------------------------------------
// delta[b][h][s] = sum_d dO * O, with dO rounded to bf16 as the dP = dO V^T products see it: dP - delta = dO' (V - O) then holds
// for the SAME dO', so a row of dS sums to zero as in exact arithmetic and a component common to all keys (values) cancels in dQ
// (dK) instead of being multiplied by the rounding error of dO
// ------------------------------------------------------------------------------------------------
template <int D, bool PAD>
__global__ __launch_bounds__(256) void k_attn_hd_delta(HdBwdArgs a) {
    const int dh = PAD ? a.dh : D;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = (int64_t)a.B * a.S * a.H;
    if (i >= n) return;
    const int head = (int)(i % a.H);
    const int64_t row = i / a.H;  // b*S + s
    const float* op = a.o + row * a.ldo + head * dh;
    const float* dp = a.d_o + row * a.lddo + head * dh;
    float s = 0.f;
#pragma unroll 8
    for (int c = 0; c < D / 4; ++c) {
        if constexpr (PAD) {
            if (4 * c >= dh) break;          // the columns from dh on are the next head's
        }
        const float4 x = *reinterpret_cast<const float4*>(op + 4 * c);
        const float4 y = *reinterpret_cast<const float4*>(dp + 4 * c);
        s += x.x * bfr(y.x) + x.y * bfr(y.y) + x.z * bfr(y.z) + x.w * bfr(y.w);
    }
    const int64_t bb = row / a.S, ss = row % a.S;
    a.delta[(bb * a.H + head) * a.S + ss] = s;
}

// ------------------------------------------------------------------------------------------------
// dK / dV: block = 4 waves x 32 keys; grid (ceil(S/128), HKV, B); loops over the group's q heads in head order.
// dK^T and dV^T of the wave's 32 keys stay in 2 * D / 2 accumulator registers (128 at D = 128: one wave per SIMD)
// ------------------------------------------------------------------------------------------------
template <int D, bool PAD, bool DROP>
__global__ __launch_bounds__(256, D <= 64 ? 2 : 1) void k_attn_hd_dkv(HdBwdArgs a) {
    constexpr int NS = D / 16, NT = D / 32;
    const int dh = PAD ? a.dh : D;
    __shared__ __attribute__((aligned(16))) short Qs[32 * (D + 8)];
    __shared__ __attribute__((aligned(16))) short dOs[32 * (D + 8)];
    __shared__ __attribute__((aligned(16))) short Qt[D * TP];
    __shared__ __attribute__((aligned(16))) short dOt[D * TP];
    __shared__ float lse_s[32];
    __shared__ float del_s[32];
    __shared__ uint32_t aw_s[64];
    // dropout: dP = keep * (dO.V) / (1-p); the kernel forms (1-p) * dS (delta staged times (1-p)) and rescales
    // dK -- and dV, accumulated from keep * P -- by 1/(1-p) at the end
    const float dscale = DROP ? a.drop.keep : 1.f;
    unsigned long long seed = 0;
    if constexpr (DROP) seed = *a.drop.seed;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hf = lane >> 5;
    const int hkv = blockIdx.y, b = blockIdx.z;
    const int rep = a.H / a.HKV;
    const int64_t key0 = (int64_t)blockIdx.x * 128 + wave * 32;
    const int64_t rowbase = (int64_t)b * a.S;
    const float sc = a.scale * LOG2E;
    const int64_t ki = key0 + l31;
    bf16x8 kf[NS], vf[NS];
    frags_ld<D, PAD>(kf, a.k + (rowbase + (ki < a.S ? ki : 0)) * a.ldk + hkv * dh, ki < a.S, hf, dh);
    frags_ld<D, PAD>(vf, a.v + (rowbase + (ki < a.S ? ki : 0)) * a.ldv + hkv * dh, ki < a.S, hf, dh);
    f32x16 dkt[NT], dvt[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) { dkt[t] = zero16(); dvt[t] = zero16(); }

    for (int hr = 0; hr < rep; ++hr) {
        const int head = hkv * rep + hr;
        const float* qp = a.q + rowbase * a.ldq + head * dh;
        const float* dop = a.d_o + rowbase * a.lddo + head * dh;
        const float* lsep = a.lse + ((int64_t)b * a.H + head) * a.S;
        const float* delp = a.delta + ((int64_t)b * a.H + head) * a.S;
        Tile<D> qt, dt;
        tile_ld<D, PAD>(qt, qp, a.ldq, 0, a.S, dh);
        tile_ld<D, PAD>(dt, dop, a.lddo, 0, a.S, dh);
        float lt = 0.f, et = 0.f;
        if (threadIdx.x < 32) {
            lt = (threadIdx.x < a.S) ? lsep[threadIdx.x] * LOG2E : INFINITY;
            et = (threadIdx.x < a.S) ? delp[threadIdx.x] * dscale : 0.f;
        }
        uint32_t rk = 0, bsel = 0;
        if constexpr (DROP) {
            const int bh = a.drop.bh(b, head);
            rk = gdrop::row_key(seed, bh);
            const uint32_t bw = gdrop::col_word(gdrop::col_key(seed, bh), (uint32_t)(ki >> 1));
            bsel = (ki & 1) ? (bw >> 16) : (bw & 0xffffu);
        }
        for (int64_t q0 = 0; q0 < a.S; q0 += 32) {
            __syncthreads();
            tile_st<D, true, true>(qt, Qs, Qt);
            tile_st<D, true, true>(dt, dOs, dOt);
            if (threadIdx.x < 32) { lse_s[threadIdx.x] = lt; del_s[threadIdx.x] = et; }
            if constexpr (DROP) {
                if (threadIdx.x < 32) {
                    const uint32_t w = gdrop::row_word(rk, (uint32_t)q0 + threadIdx.x);
                    aw_s[threadIdx.x] = w & 0xffffu;
                    aw_s[32 + threadIdx.x] = w >> 16;
                }
            }
            __syncthreads();
            if (q0 + 32 < a.S) {
                tile_ld<D, PAD>(qt, qp, a.ldq, q0 + 32, a.S, dh);
                tile_ld<D, PAD>(dt, dop, a.lddo, q0 + 32, a.S, dh);
                if (threadIdx.x < 32) {
                    const int64_t qq = q0 + 32 + threadIdx.x;
                    lt = (qq < a.S) ? lsep[qq] * LOG2E : INFINITY;
                    et = (qq < a.S) ? delp[qq] * dscale : 0.f;
                }
            }
            // S[q][key] ; dP[q][key]
            f32x16 s = zero16(), dp = zero16();
#pragma unroll
            for (int ks = 0; ks < NS; ++ks) {
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(Qs, l31, ks, hf), kf[ks], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(dOs, l31, ks, hf), vf[ks], dp, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qr = mfma32_row(r, hf);
                const float p = __builtin_amdgcn_exp2f(s[r] * sc - lse_s[qr]);   // 0 for a query row at or past S (lse = +inf)
                bool keep = true;
                if constexpr (DROP) keep = (aw_s[(l31 & 1) * 32 + qr] ^ bsel) >= a.drop.thr;
                s[r] = keep ? p : 0.f;                                  // (kept) P
                dp[r] = p * ((keep ? dp[r] : 0.f) - del_s[qr]);         // dS (without the 1/sqrt(d) factor)
            }
            bf16x8 pb[2], dsb[2];
            acc_pack(s, pb);
            acc_pack(dp, dsb);
            // dV^T[d][key] += dO^T[d][q] P[q][key] ; dK^T[d][key] += Q^T[d][q] dS[q][key]
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    dvt[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_trans(dOt, 32 * t + l31, s2, hf), pb[s2], dvt[t], 0, 0, 0);
                    dkt[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_trans(Qt, 32 * t + l31, s2, hf), dsb[s2], dkt[t], 0, 0, 0);
                }
        }
        __syncthreads();
    }
    if (ki < a.S) {
        float* dkp = a.dk + (rowbase + ki) * a.lddk + hkv * dh;
        float* dvp = a.dv + (rowbase + ki) * a.lddv + hkv * dh;
        const float vsc = DROP ? a.drop.inv_keep : 1.f, ksc = a.scale * vsc;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            store_t<PAD>(dkp + 32 * t, dkt[t], ksc, hf, dh - 32 * t);
            store_t<PAD>(dvp + 32 * t, dvt[t], vsc, hf, dh - 32 * t);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// dQ: block = 4 waves x 32 queries; grid (ceil(S/128), H, B).  At D = 128 the q and dO fragments (64 registers), dQ^T (64) and
// the staged K / V tiles (32) leave no room for two waves per SIMD
// ------------------------------------------------------------------------------------------------
template <int D, bool PAD, bool DROP>
__global__ __launch_bounds__(256, D <= 64 ? 2 : 1) void k_attn_hd_dq(HdBwdArgs a) {
    constexpr int NS = D / 16, NT = D / 32;
    const int dh = PAD ? a.dh : D;
    __shared__ __attribute__((aligned(16))) short Ks[32 * (D + 8)];
    __shared__ __attribute__((aligned(16))) short Vs[32 * (D + 8)];
    __shared__ __attribute__((aligned(16))) short Kt[D * TP];
    __shared__ uint32_t bw_s[16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hf = lane >> 5;
    const int head = blockIdx.y, b = blockIdx.z;
    const int hkv = head / (a.H / a.HKV);
    const int64_t q0 = (int64_t)blockIdx.x * 128 + wave * 32;
    const int64_t rowbase = (int64_t)b * a.S;
    const float* kp = a.k + rowbase * a.ldk + hkv * dh;
    const float* vp = a.v + rowbase * a.ldv + hkv * dh;
    const float sc = a.scale * LOG2E;
    const int64_t qi = q0 + l31;
    bf16x8 qf[NS], dof[NS];
    frags_ld<D, PAD>(qf, a.q + (rowbase + (qi < a.S ? qi : 0)) * a.ldq + head * dh, qi < a.S, hf, dh);
    frags_ld<D, PAD>(dof, a.d_o + (rowbase + (qi < a.S ? qi : 0)) * a.lddo + head * dh, qi < a.S, hf, dh);
    const float lse2 = (qi < a.S) ? a.lse[((int64_t)b * a.H + head) * a.S + qi] * LOG2E : INFINITY;
    const float del = (qi < a.S) ? a.delta[((int64_t)b * a.H + head) * a.S + qi] * (DROP ? a.drop.keep : 1.f) : 0.f;
    f32x16 dqt[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) dqt[t] = zero16();
    uint32_t aw = 0, ck = 0;
    if constexpr (DROP) {
        const unsigned long long seed = *a.drop.seed;
        const int bh = a.drop.bh(b, head);
        aw = gdrop::row_word(gdrop::row_key(seed, bh), (uint32_t)qi);
        ck = gdrop::col_key(seed, bh);
    }

    Tile<D> kt, vt;
    tile_ld<D, PAD>(kt, kp, a.ldk, 0, a.S, dh);
    tile_ld<D, PAD>(vt, vp, a.ldv, 0, a.S, dh);
    for (int64_t k0 = 0; k0 < a.S; k0 += 32) {
        __syncthreads();
        tile_st<D, true, true>(kt, Ks, Kt);
        tile_st<D, true, false>(vt, Vs, nullptr);
        if constexpr (DROP) stage_col_words(bw_s, ck, k0);
        __syncthreads();
        if (k0 + 32 < a.S) {
            tile_ld<D, PAD>(kt, kp, a.ldk, k0 + 32, a.S, dh);
            tile_ld<D, PAD>(vt, vp, a.ldv, k0 + 32, a.S, dh);
        }
        // S^T[key][q] ; dP^T[key][q]
        f32x16 s = zero16(), dp = zero16();
#pragma unroll
        for (int ks = 0; ks < NS; ++ks) {
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(Ks, l31, ks, hf), qf[ks], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(Vs, l31, ks, hf), dof[ks], dp, 0, 0, 0);
        }
        uint32_t kbits = 0xffffu;
        if constexpr (DROP) kbits = keep_bits_cols(aw, bw_s, hf, a.drop.thr);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float p = __builtin_amdgcn_exp2f(s[r] * sc - lse2);
            if (k0 + mfma32_row(r, hf) >= a.S) p = 0.f;
            dp[r] = p * ((((kbits >> r) & 1u) ? dp[r] : 0.f) - del);
        }
        bf16x8 dsb[2];
        acc_pack(dp, dsb);
        // dQ^T[d][q] += K^T[d][key] dS^T[key][q]
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                dqt[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_trans(Kt, 32 * t + l31, s2, hf), dsb[s2], dqt[t], 0, 0, 0);
    }
    if (qi < a.S) {
        float* dqp = a.dq + (rowbase + qi) * a.lddq + head * dh;
        const float qsc = DROP ? a.scale * a.drop.inv_keep : a.scale;
#pragma unroll
        for (int t = 0; t < NT; ++t) store_t<PAD>(dqp + 32 * t, dqt[t], qsc, hf, dh - 32 * t);
    }
}

bool aligned16(const void* p, int64_t ld) { return (((uintptr_t)p & 15) == 0) && (ld % 4 == 0); }

template <int D, bool PAD>
void launch_fwd(const HdArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)ceil_div(a.S, 128), (unsigned)a.H, (unsigned)a.B);
    if (a.drop.thr) GAOT_KLAUNCH((k_attn_hd_fwd<D, PAD, true>), grid, dim3(256), 0, st, a);
    else GAOT_KLAUNCH((k_attn_hd_fwd<D, PAD, false>), grid, dim3(256), 0, st, a);
}

template <int D, bool PAD>
void launch_bwd(const HdBwdArgs& a, int phase_mask, hipStream_t st) {
    const bool drop = a.drop.thr != 0;
    const int64_t n = (int64_t)a.B * a.S * a.H;
    if (phase_mask & 1) GAOT_KLAUNCH((k_attn_hd_delta<D, PAD>), dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, a);
    if (phase_mask & 2) {
        const dim3 g((unsigned)ceil_div(a.S, 128), (unsigned)a.HKV, (unsigned)a.B);
        if (drop) GAOT_KLAUNCH((k_attn_hd_dkv<D, PAD, true>), g, dim3(256), 0, st, a);
        else GAOT_KLAUNCH((k_attn_hd_dkv<D, PAD, false>), g, dim3(256), 0, st, a);
    }
    if (phase_mask & 4) {
        const dim3 g((unsigned)ceil_div(a.S, 128), (unsigned)a.H, (unsigned)a.B);
        if (drop) GAOT_KLAUNCH((k_attn_hd_dq<D, PAD, true>), g, dim3(256), 0, st, a);
        else GAOT_KLAUNCH((k_attn_hd_dq<D, PAD, false>), g, dim3(256), 0, st, a);
    }
}

// the tile width of a head width: the smallest instance that holds it; the plain instance when they are equal
template <int D>
void launch_fwd_d(const HdArgs& a, hipStream_t st) {
    if (a.dh == D) launch_fwd<D, false>(a, st);
    else launch_fwd<D, true>(a, st);
}
template <int D>
void launch_bwd_d(const HdBwdArgs& a, int phase_mask, hipStream_t st) {
    if (a.dh == D) launch_bwd<D, false>(a, phase_mask, st);
    else launch_bwd<D, true>(a, phase_mask, st);
}

constexpr const char* HEAD_DIM_RULE = "head_dim must be a multiple of 4 with 4 <= head_dim <= 128";
bool head_dim_ok(int head_dim) { return head_dim >= 4 && head_dim <= 128 && head_dim % 4 == 0; }

}  // namespace

extern "C" int gaot_attn_hd_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int64_t ldq,
                                int64_t ldk, int64_t ldv, int64_t ldo, int B, int S, int H, int HKV, int head_dim,
                                float scale, float dropout_p, const unsigned long long* dropout_seed, int head0, int heads_total,
                                gaot_stream_t stream) {
    GAOT_ENTER();
    GAOT_CHECK_ARG(head_dim_ok(head_dim), HEAD_DIM_RULE);
    GAOT_CHECK_ARG(B > 0 && S > 0 && H > 0 && HKV > 0 && H % HKV == 0, "bad shape");
    GAOT_CHECK_ARG(B <= 65535 && H <= 65535, "B and H must fit a grid dimension");
    GAOT_CHECK_ARG(q && k && v && o && lse, "null pointer");
    GAOT_CHECK_ARG(aligned16(q, ldq) && aligned16(k, ldk) && aligned16(v, ldv) && aligned16(o, ldo),
                   "q/k/v/o must be 16-byte aligned with row strides that are multiples of 4 floats");
    GAOT_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f && (dropout_p == 0.f || dropout_seed), "dropout_p in [0,1) and a seed");
    GAOT_CHECK_ARG(heads_total == 0 || (head0 >= 0 && head0 + H <= heads_total), "head0 + H <= heads_total");
    HdArgs a{q, k, v, o, lse, ldq, ldk, ldv, ldo, B, S, H, HKV, scale, gdrop::make_drop(dropout_seed, dropout_p, H, head0, heads_total),
             head_dim};
    if (head_dim <= 32) launch_fwd_d<32>(a, (hipStream_t)stream);
    else if (head_dim <= 64) launch_fwd_d<64>(a, (hipStream_t)stream);
    else if (head_dim <= 96) launch_fwd_d<96>(a, (hipStream_t)stream);
    else launch_fwd_d<128>(a, (hipStream_t)stream);
    GAOT_LAUNCH_CHECK();
    return GAOT_OK;
}

extern "C" int gaot_attn_hd_bwd(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                                const float* lse, float* delta, float* dq, float* dk, float* dv, int64_t ldq, int64_t ldk,
                                int64_t ldv, int64_t ldo, int64_t lddo, int64_t lddq, int64_t lddk, int64_t lddv, int B,
                                int S, int H, int HKV, int head_dim, float scale, float dropout_p,
                                const unsigned long long* dropout_seed, int head0, int heads_total, int phase_mask,
                                gaot_stream_t stream) {
    GAOT_ENTER();
    GAOT_CHECK_ARG(head_dim_ok(head_dim), HEAD_DIM_RULE);
    GAOT_CHECK_ARG(B > 0 && S > 0 && H > 0 && HKV > 0 && H % HKV == 0, "bad shape");
    GAOT_CHECK_ARG(B <= 65535 && H <= 65535, "B and H must fit a grid dimension");
    GAOT_CHECK_ARG(q && k && v && o && d_o && lse && delta && dq && dk && dv, "null pointer");
    GAOT_CHECK_ARG(aligned16(q, ldq) && aligned16(k, ldk) && aligned16(v, ldv) && aligned16(o, ldo) &&
                       aligned16(d_o, lddo) && aligned16(dq, lddq) && aligned16(dk, lddk) && aligned16(dv, lddv),
                   "tensors must be 16-byte aligned with row strides that are multiples of 4 floats");
    GAOT_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f && (dropout_p == 0.f || dropout_seed), "dropout_p in [0,1) and a seed");
    GAOT_CHECK_ARG(heads_total == 0 || (head0 >= 0 && head0 + H <= heads_total), "head0 + H <= heads_total");
    HdBwdArgs a{q, k, v, o, d_o, lse, delta, dq, dk, dv, ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv, B, S, H, HKV, scale,
                gdrop::make_drop(dropout_seed, dropout_p, H, head0, heads_total), head_dim};
    if (head_dim <= 32) launch_bwd_d<32>(a, phase_mask, (hipStream_t)stream);
    else if (head_dim <= 64) launch_bwd_d<64>(a, phase_mask, (hipStream_t)stream);
    else if (head_dim <= 96) launch_bwd_d<96>(a, phase_mask, (hipStream_t)stream);
    else launch_bwd_d<128>(a, phase_mask, (hipStream_t)stream);
    GAOT_LAUNCH_CHECK();
    return GAOT_OK;
}
