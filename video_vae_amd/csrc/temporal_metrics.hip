// Temporal-difference error of a clip against its reconstruction (metrics.temporal_mse): for consecutive frames t - 1, t of x (the clip)
// and y (the reconstruction), both (B, T, H, W, C) fp32 or bf16 (independently), converted to fp32 and (clamp) clamped to [0, 1]:
//
//   tmse[b, t - 1] = mean over H W C of ((y_t - y_{t-1}) - (x_t - x_{t-1}))^2,   t = 1 .. T - 1
//
// A reconstruction that flickers where the clip does not (a seam between windows) scores here although its per-frame errors do not.
// tmse_part_kernel: one workgroup per (pair, chunk of TM_CHUNK values of the frame); each thread sums 4 consecutive values per step in
// fp32 (one 16-B fp32 / 8-B bf16 load per operand and frame when the frames are aligned), then a wave butterfly and a sum over the
// waves in order give one partial per (pair, chunk).  tmse_fold_kernel (one wave per pair) sums a pair's chunks in a fixed order and
// scales by 1 / (H W C).  No atomics, no memset: bitwise reproducible.
#include "ssim_window.hpp"

namespace {

constexpr int TM_THREADS = 256;
constexpr int TM_STEPS = 4;                                    // 4-value steps per thread and chunk
constexpr int TM_CHUNK = TM_THREADS * TM_STEPS * 4;            // values of a frame per workgroup
constexpr long TM_MAX_FRAME = 1L << 30;                        // H W C

// part[(b (T - 1) + t - 1) chunks + chunk]; VEC: n % 4 == 0 and both operands aligned for a 4-value load
template <typename TX, typename TY, bool VEC>
__global__ __launch_bounds__(TM_THREADS) void tmse_part_kernel(const TX* __restrict__ x, const TY* __restrict__ y, float* __restrict__ part,
                                                               int T, long n, int chunks, int clamp)
{
    __shared__ float wsum[TM_THREADS / 64];
    const long blk = blockIdx.x;
    const long pair = blk / chunks;
    const int chunk = (int)(blk - pair * chunks);
    const long b = pair / (T - 1), t = pair - b * (T - 1) + 1;
    const long cur = (b * T + t) * n, prev = cur - n;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < TM_STEPS; ++k) {
        const long e0 = (long)chunk * TM_CHUNK + ((long)k * TM_THREADS + threadIdx.x) * 4;
        if (e0 >= n) break;        float xc[4], xp[4], yc[4], yp[4];
        load4<TX, VEC>(x + cur, e0, n, clamp, xc);
        load4<TX, VEC>(x + prev, e0, n, clamp, xp);
        load4<TY, VEC>(y + cur, e0, n, clamp, yc);
        load4<TY, VEC>(y + prev, e0, n, clamp, yp);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float d = (yc[i] - yp[i]) - (xc[i] - xp[i]);      // values past n are 0 in all four: d = 0
            acc = fmaf(d, d, acc);
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < TM_THREADS / 64; ++w) s += wsum[w];
        part[blk] = s;
    }
}

// one wave per pair: lane l sums chunks l, l + 64, ... in order, then the butterfly (a fixed order: bitwise reproducible)
__global__ __launch_bounds__(64) void tmse_fold_kernel(const float* __restrict__ part, float* __restrict__ tmse, int chunks, float inv_n)
{
    const long p = blockIdx.x;
    float s = 0.f;
    for (int c = threadIdx.x; c < chunks; c += 64) s += part[p * chunks + c];
    s = wave_sum(s);
    if (threadIdx.x == 0) tmse[p] = s * inv_n;
}

template <typename TX, typename TY>
void tmse_launch(const void* x, const void* y, float* part, int T, long n, long pairs, int chunks, int clamp, bool vec, hipStream_t s)
{
    const dim3 grid((unsigned)(pairs * chunks));
    if (vec)
        hipLaunchKernelGGL((tmse_part_kernel<TX, TY, true>), grid, dim3(TM_THREADS), 0, s, (const TX*)x, (const TY*)y, part, T, n, chunks, clamp);
    else
        hipLaunchKernelGGL((tmse_part_kernel<TX, TY, false>), grid, dim3(TM_THREADS), 0, s, (const TX*)x, (const TY*)y, part, T, n, chunks,
                           clamp);
}

}  // namespace

extern "C" int vvae_temporal_mse_supported(int H, int W, int C, int x_dtype, int y_dtype)
{
    return dtype_pair_ok(x_dtype, y_dtype) && H > 0 && W > 0 && C >= 1 && C <= 4 && (long)H * W * C <= TM_MAX_FRAME;
}

extern "C" size_t vvae_temporal_mse_part_floats(int B, int T, int H, int W, int C)
{
    if (B <= 0 || T < 2 || !vvae_temporal_mse_supported(H, W, C, VVAE_DT_F32, VVAE_DT_F32)) return 0;
    const long n = (long)H * W * C;
    return (size_t)((long)B * (T - 1) * ((n + TM_CHUNK - 1) / TM_CHUNK));
}

extern "C" int vvae_temporal_mse_fwd(const void* x, int x_dtype, const void* y, int y_dtype, float* tmse, float* part, int B, int T, int H, int W,
                                     int C, int clamp, void* stream)
{
    if (!x || !y || B <= 0 || T <= 0 || !vvae_temporal_mse_supported(H, W, C, x_dtype, y_dtype) ||
        (uintptr_t)x % (x_dtype == VVAE_DT_F32 ? 4 : 2) || (uintptr_t)y % (y_dtype == VVAE_DT_F32 ? 4 : 2))
        return VVAE_ERR_BAD_ARG;
    if (T == 1) return 0;                                      // no pairs: nothing to write
    if (!tmse || !part || (uintptr_t)tmse % 4 || (uintptr_t)part % 4) return VVAE_ERR_BAD_ARG;
    const long n = (long)H * W * C;
    const int chunks = (int)((n + TM_CHUNK - 1) / TM_CHUNK);
    const long pairs = (long)B * (T - 1);
    if (pairs * chunks > 0x7fffffffL) return VVAE_ERR_BAD_ARG;
    const bool vec = n % 4 == 0 && (uintptr_t)x % (x_dtype == VVAE_DT_F32 ? 16 : 8) == 0 && (uintptr_t)y % (y_dtype == VVAE_DT_F32 ? 16 : 8) == 0;
    hipStream_t s = (hipStream_t)stream;
    dispatch_dtype_pair(x_dtype, y_dtype, [&](auto tx, auto ty) {
        tmse_launch<typename decltype(tx)::type, typename decltype(ty)::type>(x, y, part, T, n, pairs, chunks, clamp, vec, s);
    });
    VVAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(tmse_fold_kernel, dim3((unsigned)pairs), dim3(64), 0, s, (const float*)part, tmse, chunks, (float)(1.0 / (double)n));
    VVAE_LAUNCH_CHECK();
    return 0;
}
