// What the evaluation kernels share (metrics.hip, plane_metrics.hip, temporal_metrics.hip): the SSIM window and the split of a frame
// into bands of rows, and the operand handling of the kernels that take fp32 or bf16 clips.
#pragma once
#include <math.h>

#include "common.hpp"

// the normalised 11-tap Gaussian (sigma 1.5)
inline void ssim_taps(double (&g)[11])
{
    double sum = 0.0;
    for (int k = 0; k < 11; ++k) { g[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5)); sum += g[k]; }
    for (int k = 0; k < 11; ++k) g[k] /= sum;
}

// bands of R rows until the grid has about target_wgs workgroups of `groups` per band, a band at least min_band rows (its 10 halo rows
// are read again)
inline void ssim_bands(int H, long groups, int target_wgs, int min_band, int& R, int& bands)
{
    long n = (target_wgs + groups - 1) / groups;
    const int most = (H + min_band - 1) / min_band;
    if (n > most) n = most;
    if (n < 1) n = 1;
    R = (H + (int)n - 1) / (int)n;
    bands = (H + R - 1) / R;
}

// a band's rows: it owns [r0, r1) for the squared error and, when `any`, the SSIM output rows [max(r0, 5), min(r1, H - 5)), which read
// the rows [a, e) = 5 above to 5 below them; without output rows [a, e) = [r0, r1)
struct SsimRows {
    int r0, r1, a, e;
    bool any;
};
__device__ __forceinline__ SsimRows ssim_rows(int band, int R, int H)
{
    const int r0 = band * R, r1 = min(r0 + R, H);
    const int o0 = max(r0, 5), o1 = min(r1, H - 5);
    const bool any = o0 < o1;
    return {r0, r1, any ? o0 - 5 : r0, any ? o1 + 5 : r1, any};
}

__device__ __forceinline__ float clamp01(float v, int clamp) { return clamp ? fminf(fmaxf(v, 0.f), 1.f) : v; }

// elements e0 .. e0 + 3 of the n at p (0 past the end), clamped: element by element, or, VEC (n % 4 == 0, e0 % 4 == 0 and p aligned for
// it), by one 16-B fp32 / 8-B bf16 load
template <typename T, bool VEC, typename I>
__device__ __forceinline__ void load4(const T* __restrict__ p, I e0, I n, int clamp, float (&v)[4])
{
    if (VEC) {
        if (e0 < n) VecIO<T, 4>::load(p + e0, v);
        else v[0] = v[1] = v[2] = v[3] = 0.f;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = e0 + i < n ? ldf(p + e0 + i) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = clamp01(v[i], clamp);
}

inline bool dtype_pair_ok(int x_dtype, int y_dtype)
{
    return (x_dtype == VVAE_DT_F32 || x_dtype == VVAE_DT_BF16) && (y_dtype == VVAE_DT_F32 || y_dtype == VVAE_DT_BF16);
}

// f(TypeTag<TX>(), TypeTag<TY>()) for the element types of a valid (x_dtype, y_dtype) -> what f returns
template <typename T> struct TypeTag { using type = T; };
template <typename F>
auto dispatch_dtype_pair(int x_dtype, int y_dtype, F&& f)
{
    if (x_dtype == VVAE_DT_F32 && y_dtype == VVAE_DT_F32) return f(TypeTag<float>(), TypeTag<float>());
    if (x_dtype == VVAE_DT_F32) return f(TypeTag<float>(), TypeTag<bf16_t>());
    if (y_dtype == VVAE_DT_F32) return f(TypeTag<bf16_t>(), TypeTag<float>());
    return f(TypeTag<bf16_t>(), TypeTag<bf16_t>());
}
