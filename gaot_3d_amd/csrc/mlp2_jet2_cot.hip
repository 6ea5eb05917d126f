// The elementwise MIDDLE of the cotangent of the projection's directional 2-jet with a second-order cotangent PER DIRECTION
// (MAGNODecoder._project_cot, the general second-order branch), one launch for nd = 1..6 directions.  With z = W1 x + b1,
// u_i = W1 x'_i, s_i = W1 x''_i and a = erf-GELU the projection's jets are
//     y = W2 a(z) + b2,   y'_i = W2 (a'(z) u_i),   y''_i = W2 (a''(z) u_i^2 + a'(z) s_i)
// and for the cotangents pulled to hidden width, A = g_y W2, A_i = g_d1,i W2, B_i = g_d2,i W2:
//     dz   = a' A + a'' sum_i u_i A_i + sum_i (a''' u_i^2 + a'' s_i) B_i
//     du_i = a' A_i + 2 a'' u_i B_i
//     ds_i = a' B_i
// a' = Phi + z phi, a'' = phi (2 - z^2), a''' = phi z (z^2 - 4) as in mlp2_lap_cot.hip; phi and Phi are evaluated ONCE per element.
// (gaot_mlp2_lap_cot_mid is the case of three directions whose B_i are one plane and whose s_i are summed: it stays as it is.)
// The kernel reads the 1 + 2 nd planes [z (without its bias: b1 is added here); u_0..; s_0..] of one stack and the 1 + 2 nd planes
// [A (or null: zero); A_0..; B_0..] of another over [rows, hidden] and writes the 1 + 2 nd planes [dz; du_0..; ds_0..] STACKED, so
// that the product with W1 that follows is one GEMM.  The direction loop is unrolled on the template argument: every plane offset
// is a compile-time multiple of a stride; both sums over i run in ascending i with one fma per term.  Memory-bound: every element
// is read once and written once with 128-bit loads and stores, fp32 throughout.  A thread's element depends on that element of each
// plane alone, and a thread stores du_i and ds_i after it has read u_i, s_i, A_i and B_i, and dz last -- so the output stack MAY
// ALIAS the A stack or the z stack plane for plane (dz over A / z, du_i over A_i / u_i, ds_i over B_i / s_i): a plane of the
// output only ever overwrites what this thread has already read.  No LDS, no scratch, no atomics.
#include "common.h"

namespace {

constexpr int MAXD = 6;

struct Jet2CotArgs {
    const float* z;    // planes z, u_i at (1 + i) * z_stride, s_i at (1 + nd + i) * z_stride
    const float* b1;   // or null
    const float* a;    // or null: A = 0
    const float* ad;   // planes A_i at i * a_stride, B_i at (nd + i) * a_stride
    float* out;        // planes dz, du_i at (1 + i) * out_stride, ds_i at (1 + nd + i) * out_stride
    int64_t z_stride, a_stride, out_stride, nv;   // nv: float4 elements of one plane
    int hv;                                       // hidden / 4
};

struct GeluD123 {
    float a1, a2, a3;
};

__device__ __forceinline__ GeluD123 gelu_d123(float z) {
    const float z2 = z * z;
    const float phi = 0.39894228040143267794f * expf(-0.5f * z2);
    const float Phi = 0.5f * (1.0f + erff(z * 0.70710678118654752440f));
    return {fmaf(z, phi, Phi), phi * (2.0f - z2), phi * z * (z2 - 4.0f)};
}

// one direction of one element: du, ds and the two running sums (first = the direction is i = 0: the sums start here)
__device__ __forceinline__ void jet2_cot_dir(const GeluD123& g, float u, float s, float Ai, float Bi, bool first, float& ua, float& tb,
                                             float& du, float& ds) {
    const float t = fmaf(g.a3, u * u, g.a2 * s);
    ua = first ? u * Ai : fmaf(u, Ai, ua);
    tb = first ? t * Bi : fmaf(t, Bi, tb);
    du = fmaf(g.a1, Ai, 2.0f * g.a2 * Bi * u);
    ds = g.a1 * Bi;
}

template <int ND>
__global__ __launch_bounds__(256) void k_mlp2_cot_jet2_mid(const Jet2CotArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.nv; i += stride) {
        const int64_t e = i * 4;
        auto ld = [e](const float* p) { return *reinterpret_cast<const float4*>(p + e); };
        float4 z = ld(a.z);
        if (a.b1) {
            const float4 b = *reinterpret_cast<const float4*>(a.b1 + (i % a.hv) * 4);
            z.x += b.x; z.y += b.y; z.z += b.z; z.w += b.w;
        }
        const float4 A = a.a ? ld(a.a) : make_float4(0.f, 0.f, 0.f, 0.f);
        const GeluD123 gx = gelu_d123(z.x), gy = gelu_d123(z.y), gz = gelu_d123(z.z), gw = gelu_d123(z.w);
        float4 ua, tb;
        float* o = a.out + e;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const float4 u = ld(a.z + (1 + d) * a.z_stride), s = ld(a.z + (1 + ND + d) * a.z_stride);
            const float4 Ai = ld(a.ad + d * a.a_stride), Bi = ld(a.ad + (ND + d) * a.a_stride);
            float4 du, ds;
            jet2_cot_dir(gx, u.x, s.x, Ai.x, Bi.x, d == 0, ua.x, tb.x, du.x, ds.x);
            jet2_cot_dir(gy, u.y, s.y, Ai.y, Bi.y, d == 0, ua.y, tb.y, du.y, ds.y);
            jet2_cot_dir(gz, u.z, s.z, Ai.z, Bi.z, d == 0, ua.z, tb.z, du.z, ds.z);
            jet2_cot_dir(gw, u.w, s.w, Ai.w, Bi.w, d == 0, ua.w, tb.w, du.w, ds.w);
            *reinterpret_cast<float4*>(o + (1 + d) * a.out_stride) = du;
            *reinterpret_cast<float4*>(o + (1 + ND + d) * a.out_stride) = ds;
        }
        float4 dz;
        dz.x = fmaf(gx.a1, A.x, fmaf(gx.a2, ua.x, tb.x));
        dz.y = fmaf(gy.a1, A.y, fmaf(gy.a2, ua.y, tb.y));
        dz.z = fmaf(gz.a1, A.z, fmaf(gz.a2, ua.z, tb.z));
        dz.w = fmaf(gw.a1, A.w, fmaf(gw.a2, ua.w, tb.w));
        *reinterpret_cast<float4*>(o) = dz;
    }
}

}  // namespace

extern "C" int gaot_mlp2_jet2_cot_mid(const float* zus, int64_t z_stride, const float* b1, const float* a, const float* ab,
                                      int64_t a_stride, int nd, int64_t num_rows, int hidden, float* out, int64_t out_stride,
                                      gaot_stream_t stream) {
    GAOT_ENTER();
    GAOT_CHECK_ARG(nd >= 1 && nd <= MAXD, "nd must be 1..6 directions");
    GAOT_CHECK_ARG(num_rows >= 0, "negative size");
    GAOT_CHECK_ARG(hidden > 0 && hidden % 4 == 0, "hidden must be a positive multiple of 4");
    const int64_t n = num_rows * hidden;
    GAOT_CHECK_ARG(z_stride >= n && a_stride >= n && out_stride >= n && z_stride % 4 == 0 && a_stride % 4 == 0 && out_stride % 4 == 0,
                   "a plane stride must be a multiple of 4 floats and at least num_rows * hidden");
    if (num_rows == 0) return GAOT_OK;
    GAOT_CHECK_ARG(zus && ab && out, "null pointer");
    GAOT_CHECK_ARG((((uintptr_t)zus | (uintptr_t)b1 | (uintptr_t)a | (uintptr_t)ab | (uintptr_t)out) & 15) == 0,
                   "every plane must be 16-byte aligned");
    Jet2CotArgs k;
    k.z = zus; k.b1 = b1; k.a = a; k.ad = ab; k.out = out;
    k.z_stride = z_stride; k.a_stride = a_stride; k.out_stride = out_stride; k.nv = n / 4; k.hv = hidden / 4;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(k.nv, 256), 256 * 8));
    hipStream_t st = (hipStream_t)stream;
    switch (nd) {
        case 1: GAOT_KLAUNCH(k_mlp2_cot_jet2_mid<1>, dim3(grid), dim3(256), 0, st, k); break;
        case 2: GAOT_KLAUNCH(k_mlp2_cot_jet2_mid<2>, dim3(grid), dim3(256), 0, st, k); break;
        case 3: GAOT_KLAUNCH(k_mlp2_cot_jet2_mid<3>, dim3(grid), dim3(256), 0, st, k); break;
        case 4: GAOT_KLAUNCH(k_mlp2_cot_jet2_mid<4>, dim3(grid), dim3(256), 0, st, k); break;
        case 5: GAOT_KLAUNCH(k_mlp2_cot_jet2_mid<5>, dim3(grid), dim3(256), 0, st, k); break;
        default: GAOT_KLAUNCH(k_mlp2_cot_jet2_mid<6>, dim3(grid), dim3(256), 0, st, k); break;
    }
    GAOT_LAUNCH_CHECK();
    return GAOT_OK;
}
