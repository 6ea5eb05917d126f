// The elementwise MIDDLE of the cotangent of the projection's Laplacian jet (MAGNODecoder._project_lap_vjp), one launch.  With
// z = W1 x + b1, u_d = W1 x'_d (d = 0, 1, 2), s = W1 sum_d x''_d and a = erf-GELU the projection's jets are
//     y = W2 a(z) + b2,   y'_d = W2 (a'(z) u_d),   Lap y = W2 (a''(z) sum_d u_d^2 + a'(z) s)
// and for the cotangents pulled to hidden width, A = g_y W2, A_d = g_y'd W2, A_L = g_Lap W2:
//     dz   = a' A + a'' sum_d u_d A_d + (a''' sum_d u_d^2 + a'' s) A_L
//     du_d = a' A_d + 2 a'' u_d A_L
//     ds   = a' A_L
// a' = Phi + z phi, a'' = phi (2 - z^2), a''' = phi z (z^2 - 4); phi and Phi are evaluated ONCE per element.  The kernel reads the ten
// planes z (without its bias: b1 is added here), u[3], s, A (or null: zero), A_d[3], A_L over [rows, hidden] and writes the five
// planes dz, du[3], ds STACKED, so that the product with W1 that follows is one GEMM.  Memory-bound: every element is read once and
// written once with 128-bit loads and stores, fp32 throughout, a thread's element depends on that element of each plane alone -- so
// the output stack MAY ALIAS the A stack (dz over A, du_d over A_d, ds over A_L) or the z stack (dz over z, du_d over u_d, ds over
// s): a thread reads all its inputs before its first store.  No LDS, no scratch, no atomics.
#include "common.h"

namespace {

struct LapCotArgs {
    const float* z;
    const float* u;
    const float* s;
    const float* b1;   // or null
    const float* a;    // or null: A = 0
    const float* ad;
    const float* al;
    float* out;
    int64_t u_stride, ad_stride, out_stride, nv;   // nv: float4 elements of one plane
    int hv;                                        // hidden / 4
};

__device__ __forceinline__ void lap_cot_elem(float z, float u0, float u1, float u2, float s, float A, float A0, float A1, float A2, float AL,
                                             float& dz, float& du0, float& du1, float& du2, float& ds) {
    const float z2 = z * z;
    const float phi = 0.39894228040143267794f * expf(-0.5f * z2);
    const float Phi = 0.5f * (1.0f + erff(z * 0.70710678118654752440f));
    const float a1 = fmaf(z, phi, Phi);
    const float a2 = phi * (2.0f - z2);
    const float a3 = phi * z * (z2 - 4.0f);
    const float uu = fmaf(u2, u2, fmaf(u1, u1, u0 * u0));
    const float ua = fmaf(u2, A2, fmaf(u1, A1, u0 * A0));
    dz = fmaf(a1, A, fmaf(a2, ua, fmaf(a3, uu, a2 * s) * AL));
    const float t = 2.0f * a2 * AL;
    du0 = fmaf(a1, A0, t * u0);
    du1 = fmaf(a1, A1, t * u1);
    du2 = fmaf(a1, A2, t * u2);
    ds = a1 * AL;
}

__global__ __launch_bounds__(256) void k_mlp2_lap_cot_mid(const LapCotArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.nv; i += stride) {
        const int64_t e = i * 4;
        auto ld = [e](const float* p) { return *reinterpret_cast<const float4*>(p + e); };
        float4 z = ld(a.z);
        if (a.b1) {
            const float4 b = *reinterpret_cast<const float4*>(a.b1 + (i % a.hv) * 4);
            z.x += b.x; z.y += b.y; z.z += b.z; z.w += b.w;
        }
        const float4 u0 = ld(a.u), u1 = ld(a.u + a.u_stride), u2 = ld(a.u + 2 * a.u_stride), s = ld(a.s);
        const float4 A = a.a ? ld(a.a) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 A0 = ld(a.ad), A1 = ld(a.ad + a.ad_stride), A2 = ld(a.ad + 2 * a.ad_stride), AL = ld(a.al);
        float4 dz, d0, d1, d2, ds;
        lap_cot_elem(z.x, u0.x, u1.x, u2.x, s.x, A.x, A0.x, A1.x, A2.x, AL.x, dz.x, d0.x, d1.x, d2.x, ds.x);
        lap_cot_elem(z.y, u0.y, u1.y, u2.y, s.y, A.y, A0.y, A1.y, A2.y, AL.y, dz.y, d0.y, d1.y, d2.y, ds.y);
        lap_cot_elem(z.z, u0.z, u1.z, u2.z, s.z, A.z, A0.z, A1.z, A2.z, AL.z, dz.z, d0.z, d1.z, d2.z, ds.z);
        lap_cot_elem(z.w, u0.w, u1.w, u2.w, s.w, A.w, A0.w, A1.w, A2.w, AL.w, dz.w, d0.w, d1.w, d2.w, ds.w);
        float* o = a.out + e;
        *reinterpret_cast<float4*>(o) = dz;
        *reinterpret_cast<float4*>(o + a.out_stride) = d0;
        *reinterpret_cast<float4*>(o + 2 * a.out_stride) = d1;
        *reinterpret_cast<float4*>(o + 3 * a.out_stride) = d2;
        *reinterpret_cast<float4*>(o + 4 * a.out_stride) = ds;
    }
}

}  // namespace

extern "C" int gaot_mlp2_lap_cot_mid(const float* z, const float* u, int64_t u_stride, const float* s, const float* b1, const float* a,
                                     const float* ad, int64_t ad_stride, const float* al, int64_t num_rows, int hidden, float* out,
                                     int64_t out_stride, gaot_stream_t stream) {
    GAOT_ENTER();
    GAOT_CHECK_ARG(num_rows >= 0, "negative size");
    GAOT_CHECK_ARG(hidden > 0 && hidden % 4 == 0, "hidden must be a positive multiple of 4");
    const int64_t n = num_rows * hidden;
    GAOT_CHECK_ARG(u_stride >= n && ad_stride >= n && out_stride >= n && u_stride % 4 == 0 && ad_stride % 4 == 0 && out_stride % 4 == 0,
                   "a plane stride must be a multiple of 4 floats and at least num_rows * hidden");
    if (num_rows == 0) return GAOT_OK;
    GAOT_CHECK_ARG(z && u && s && ad && al && out, "null pointer");
    GAOT_CHECK_ARG((((uintptr_t)z | (uintptr_t)u | (uintptr_t)s | (uintptr_t)b1 | (uintptr_t)a | (uintptr_t)ad | (uintptr_t)al |
                     (uintptr_t)out) & 15) == 0, "every plane must be 16-byte aligned");
    LapCotArgs k;
    k.z = z; k.u = u; k.s = s; k.b1 = b1; k.a = a; k.ad = ad; k.al = al; k.out = out;
    k.u_stride = u_stride; k.ad_stride = ad_stride; k.out_stride = out_stride; k.nv = n / 4; k.hv = hidden / 4;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(k.nv, 256), 256 * 8));
    GAOT_KLAUNCH(k_mlp2_lap_cot_mid, dim3(grid), dim3(256), 0, (hipStream_t)stream, k);
    GAOT_LAUNCH_CHECK();
    return GAOT_OK;
}
