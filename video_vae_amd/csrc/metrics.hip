// Reconstruction metrics per frame: MSE, PSNR and SSIM (Wang et al. 2004) of x (the clip) against y (its reconstruction), both
// channels-last (B, T, H, W, C) fp32 or bf16 with independent dtypes, converted to fp32 and (clamp) clamped to [0, 1].
//
//   mse[f]  = mean over H W C of (x - y)^2;  psnr[f] = 10 log10(1 / max(mse, 1e-10))
//   ssim[f] = mean over the valid region (rows and columns 5 .. n - 6) and the channels of
//             S = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sx + sy + C2)),  C1 = 0.01^2, C2 = 0.03^2,
//             m = g * x, sx = g * x^2 - mx^2, sxy = g * (x y) - mx my, g the normalised 11-tap Gaussian (sigma 1.5) applied separably
//   masked frames (mask == 0): 0 everywhere, the frame is never read.
//
// metrics_fwd_kernel: one workgroup per (band of rows, frame).  Each thread owns 4 consecutive elements of a flat row of W C values
// (one 16-B fp32 / 8-B bf16 load per operand and row when the row is aligned) and marches down the band with the last 11 rows of x
// and y in a register ring (the loop is unrolled by 11, so every ring slot is a compile-time register).  Per output row it forms the
// vertically filtered mx, my, x^2, y^2, xy and writes them channel-planar to LDS; after a barrier a thread per (channel, 4 columns)
// runs the horizontal 11 taps from 5 aligned 16-B LDS reads per quantity and sums S over its valid columns.  The squared error of
// each of the band's own rows is summed in the same pass; the 5 halo rows above and below a band are re-read (from cache).
// Reductions are deterministic: per-thread sums, a wave butterfly, a fixed-order sum over the waves, one partial pair per
// (frame, band); metrics_fold_kernel sums the bands of a frame in order.  No atomics, no memset.
//
// Wide frames (W C > 2048, vvae_recon_metrics_wide_*): the same kernel with STRIP = true and a third grid dimension of column strips.
// Strip s owns the SSIM columns [c0, c1) = [5 + s SW, min(5 + (s + 1) SW, W - 5)) and reads the frame columns [c0 - 5, c1 + 5); the
// strips' MSE columns are [c0, c1) widened to 0 on the first strip and to W on the last.  So the SSIM columns partition 5 .. W - 6 and
// the MSE columns 0 .. W - 1.  One partial pair per (frame, strip, band); the fold sums a frame's strips and bands in that order.
#include <type_traits>

#include "common.hpp"

namespace {

constexpr int RM_MAX_THREADS = 512;
constexpr int RM_MAX_ROW = 2048;             // W C: 4 elements per thread
constexpr int RM_MIN_BAND = 16;              // rows per band at least (halo overhead 10 / band rows)
constexpr int RM_TARGET_WGS = 1024;          // bands are split until the grid has about this many workgroups
constexpr int RM_MAX_WIDE_W = 8192;          // widest frame of the strip path

struct RmDims {
    int H, W, C, L, P, bands, R, clamp;
    float g[11];
};
// the strip path's dimensions (L is then the row pitch); the kernels without strips take RmDims alone
struct RmWideDims : RmDims {
    int SW, strips;                          // SSIM columns per strip, number of strips
};
template <bool STRIP> using RmDimsOf = typename std::conditional<STRIP, RmWideDims, RmDims>::type;

__device__ __forceinline__ float rm_prep(float v, int clamp) { return clamp ? fminf(fmaxf(v, 0.f), 1.f) : v; }

template <typename T, bool VEC>
__device__ __forceinline__ void rm_load(const T* __restrict__ row, int e0, int L, int clamp, float (&v)[4])
{
    if (VEC) {
        if (e0 < L) VecIO<T, 4>::load(row + e0, v);
        else v[0] = v[1] = v[2] = v[3] = 0.f;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = e0 + i < L ? ldf(row + e0 + i) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = rm_prep(v[i], clamp);
}

// a strip's row: the wide load only where all 4 elements lie in the strip (its width need not be a multiple of 4)
template <typename T, bool VEC, bool STRIP>
__device__ __forceinline__ void rm_row(const T* __restrict__ row, int e0, int L, int clamp, float (&v)[4])
{
    if constexpr (STRIP) {
        if (VEC && e0 + 4 <= L) {
            VecIO<T, 4>::load(row + e0, v);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = rm_prep(v[i], clamp);
        } else {
            rm_load<T, false>(row, e0, L, clamp, v);
        }
    } else {
        rm_load<T, VEC>(row, e0, L, clamp, v);
    }
}

// LDS: 5 planes (mx, my, x^2, y^2, xy) of C rows of P floats (column j at j + 8; the margins stay 0) | red[16]
template <typename TX, typename TY, bool VEC, bool STRIP>
__global__ __launch_bounds__(RM_MAX_THREADS) void metrics_fwd_kernel(const TX* __restrict__ x, const TY* __restrict__ y,
                                                                     const float* __restrict__ mask, float* __restrict__ part, RmDimsOf<STRIP> d)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int band = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    // STRIP: the strip's columns [col0, col0 + W) of the frame, a row of L values; the row pitch is d.L
    int strip = 0, col0 = 0, W = d.W, L = d.L;
    float* out = part + ((long)f * d.bands + band) * 2;
    if constexpr (STRIP) {
        strip = blockIdx.z;
        col0 = strip * d.SW;
        W = min(col0 + d.SW + 10, d.W) - col0;
        L = W * d.C;
        out = part + (((long)f * d.strips + strip) * d.bands + band) * 2;
    }
    if (mask[f] == 0.f) {                    // padding: never read
        if (tid == 0) { out[0] = 0.f; out[1] = 0.f; }
        return;
    }
    const int CP = d.C * d.P;
    float* red = lds + 5 * CP;
    for (int i = tid; i < 5 * CP; i += blockDim.x) lds[i] = 0.f;

    // rows: the band owns [r0, r1) for the squared error and the output rows [o0, o1) of SSIM, which read [o0 - 5, o1 + 5)
    const int r0 = band * d.R, r1 = min(r0 + d.R, d.H);
    const int o0 = max(r0, 5), o1 = min(r1, d.H - 5);
    const bool any = o0 < o1;
    const int a = any ? o0 - 5 : r0, e = any ? o1 + 5 : r1;

    // vertical pass: elements e0 .. e0 + 3 of the flat row; their LDS slots c P + j + 8
    const int e0 = tid * 4;
    int wofs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int el = e0 + i, j = el / d.C;
        wofs[i] = el < L ? (el - j * d.C) * d.P + j + 8 : -1;
    }
    // STRIP: the squared error counts the strip's own columns only
    bool mse_col[4] = {true, true, true, true};
    if constexpr (STRIP) {
        const int mlo = strip == 0 ? 0 : 5, mhi = strip == d.strips - 1 ? W : W - 5;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = (e0 + i) / d.C;
            mse_col[i] = j >= mlo && j < mhi;
        }
    }
    // horizontal pass: channel hc, output columns j0 .. j0 + 3
    const int ng = (W + 3) / 4, hc = tid / ng, j0 = (tid - hc * ng) * 4;
    const bool hact = hc < d.C && j0 + 3 >= 5 && j0 <= W - 6;
    const float* hrow = lds + hc * d.P + j0;

    const long fbase = (long)f * d.H * d.L;
    const TX* xf = x + fbase + (long)col0 * d.C;
    const TY* yf = y + fbase + (long)col0 * d.C;
    float g[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) g[k] = d.g[k];
    const float C1 = 1e-4f, C2 = 9e-4f;

    float xr[11][4], yr[11][4], nx[4], ny[4];
    float se = 0.f, ss = 0.f;
    rm_row<TX, VEC, STRIP>(xf + (long)a * d.L, e0, L, d.clamp, nx);
    rm_row<TY, VEC, STRIP>(yf + (long)a * d.L, e0, L, d.clamp, ny);
    __syncthreads();                         // LDS zeroed

    for (int base = a; base < e; base += 11) {
#pragma unroll
        for (int s = 0; s < 11; ++s) {
            const int r = base + s;
            if (r >= e) break;
#pragma unroll
            for (int i = 0; i < 4; ++i) { xr[s][i] = nx[i]; yr[s][i] = ny[i]; }
            if (r + 1 < e) {                 // the next row is in flight while this one is filtered
                rm_row<TX, VEC, STRIP>(xf + (long)(r + 1) * d.L, e0, L, d.clamp, nx);
                rm_row<TY, VEC, STRIP>(yf + (long)(r + 1) * d.L, e0, L, d.clamp, ny);
            }
            if (r >= r0 && r < r1) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float dd = xr[s][i] - yr[s][i];
                    if (mse_col[i]) se = fmaf(dd, dd, se);
                }
            }
            if (!any || r < a + 10) continue;
            // output row r - 5 from rows r - 10 .. r, i.e. ring slots (s + 1 + k) % 11
            float mx[4] = {0.f, 0.f, 0.f, 0.f}, my[4] = {0.f, 0.f, 0.f, 0.f}, xx[4] = {0.f, 0.f, 0.f, 0.f}, yy[4] = {0.f, 0.f, 0.f, 0.f},
                  xy[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const int q = (s + 1 + k) % 11;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float gx = g[k] * xr[q][i], gy = g[k] * yr[q][i];
                    mx[i] += gx;
                    my[i] += gy;
                    xx[i] = fmaf(gx, xr[q][i], xx[i]);
                    yy[i] = fmaf(gy, yr[q][i], yy[i]);
                    xy[i] = fmaf(gx, yr[q][i], xy[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (wofs[i] >= 0) {
                    lds[wofs[i]] = mx[i];
                    lds[CP + wofs[i]] = my[i];
                    lds[2 * CP + wofs[i]] = xx[i];
                    lds[3 * CP + wofs[i]] = yy[i];
                    lds[4 * CP + wofs[i]] = xy[i];
                }
            __syncthreads();
            if (hact) {
                float h[5][4];
#pragma unroll
                for (int p = 0; p < 5; ++p) {
                    float w[20];
#pragma unroll
                    for (int v = 0; v < 5; ++v) {
                        const float4 t = *reinterpret_cast<const float4*>(hrow + p * CP + 4 * v);
                        w[4 * v] = t.x; w[4 * v + 1] = t.y; w[4 * v + 2] = t.z; w[4 * v + 3] = t.w;
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {    // column j0 + i: taps j0 + i - 5 .. j0 + i + 5 at w[i + 3 .. i + 13]
                        float acc = 0.f;
#pragma unroll
                        for (int k = 0; k < 11; ++k) acc = fmaf(g[k], w[i + 3 + k], acc);
                        h[p][i] = acc;
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float ux = h[0][i], uy = h[1][i];
                    const float vx = h[2][i] - ux * ux, vy = h[3][i] - uy * uy, vxy = h[4][i] - ux * uy;
                    const float num = (2.f * ux * uy + C1) * (2.f * vxy + C2);
                    const float den = (ux * ux + uy * uy + C1) * (vx + vy + C2);
                    const int j = j0 + i;
                    ss += (j >= 5 && j <= W - 6) ? num / den : 0.f;
                }
            }
            __syncthreads();                 // the LDS row is rewritten by the next output row
        }
    }

    // deterministic workgroup reduction: wave butterflies, then the waves in order
    se = wave_sum(se);
    ss = wave_sum(ss);
    const int wave = tid >> 6, nw = (blockDim.x + 63) >> 6;
    if ((tid & 63) == 0) { red[2 * wave] = se; red[2 * wave + 1] = ss; }
    __syncthreads();
    if (tid == 0) {
        float a0 = 0.f, a1 = 0.f;
        for (int w = 0; w < nw; ++w) { a0 += red[2 * w]; a1 += red[2 * w + 1]; }
        out[0] = a0;
        out[1] = a1;
    }
}

// one thread per frame: the bands in order -> mse, psnr, ssim (0 on masked frames)
__global__ void metrics_fold_kernel(const float* __restrict__ part, const float* __restrict__ mask, float* __restrict__ mse,
                                    float* __restrict__ psnr, float* __restrict__ ssim, int F, int bands, double n, double nv)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    if (mask[f] == 0.f) { mse[f] = 0.f; psnr[f] = 0.f; ssim[f] = 0.f; return; }
    float se = 0.f, ss = 0.f;
    for (int b = 0; b < bands; ++b) { se += part[((long)f * bands + b) * 2]; ss += part[((long)f * bands + b) * 2 + 1]; }
    const double m = (double)se / n;
    mse[f] = (float)m;
    psnr[f] = (float)(10.0 * log10(1.0 / fmax(m, 1e-10)));
    ssim[f] = (float)((double)ss / nv);
}

// bands of rows until the grid has about RM_TARGET_WGS workgroups of `groups` per band, the Gaussian taps, the threads for rows of
// wmax columns
bool rm_bands_taps(int H, int C, long groups, int wmax, RmDims& d, int& threads)
{
    int bands = (int)((RM_TARGET_WGS + groups - 1) / groups);
    const int most = (H + RM_MIN_BAND - 1) / RM_MIN_BAND;
    if (bands > most) bands = most;
    if (bands < 1) bands = 1;
    d.R = (H + bands - 1) / bands;
    d.bands = (H + d.R - 1) / d.R;
    d.clamp = 0;
    double g[11], sum = 0.0;
    for (int k = 0; k < 11; ++k) { g[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5)); sum += g[k]; }
    for (int k = 0; k < 11; ++k) d.g[k] = (float)(g[k] / sum);
    const int need = max((wmax * C + 3) / 4, C * ((wmax + 3) / 4));
    threads = (need + 63) / 64 * 64;
    return threads <= RM_MAX_THREADS;
}

bool rm_dims(int B, int T, int H, int W, int C, RmDims& d, int& threads)
{
    if (B <= 0 || T <= 0 || H < 11 || W < 11 || C < 1 || C > 4 || (long)W * C > RM_MAX_ROW || (long)B * T > 65535) return false;
    d.H = H; d.W = W; d.C = C; d.L = W * C;
    d.P = (W + 3) / 4 * 4 + 16;
    return rm_bands_taps(H, C, (long)B * T, W, d, threads);
}

// wide frames: strips of at most RM_MAX_ROW values and RM_MAX_THREADS threads, halo included; SW C % 4 == 0 keeps every strip 16-B aligned
bool rm_wide_dims(int B, int T, int H, int W, int C, RmWideDims& d, int& threads)
{
    if (B <= 0 || T <= 0 || H < 11 || W < 11 || W > RM_MAX_WIDE_W || C < 1 || C > 4 || (long)B * T > 65535) return false;
    int sw = (RM_MAX_ROW / C - 10) / 4 * 4;
    while (C * ((sw + 10 + 3) / 4) > RM_MAX_THREADS) sw -= 4;
    d.SW = sw;
    d.strips = (W - 10 + sw - 1) / sw;
    const int wmax = min(sw + 10, W);
    d.H = H; d.W = W; d.C = C; d.L = W * C;
    d.P = (wmax + 3) / 4 * 4 + 16;
    return rm_bands_taps(H, C, (long)B * T * d.strips, wmax, d, threads);
}

template <typename TX, typename TY, bool STRIP>
void rm_launch(bool vec, dim3 grid, int threads, size_t lds, hipStream_t s, const void* x, const void* y, const float* mask, float* part,
               const RmDimsOf<STRIP>& d)
{
    if (vec)
        hipLaunchKernelGGL((metrics_fwd_kernel<TX, TY, true, STRIP>), grid, dim3(threads), lds, s, (const TX*)x, (const TY*)y, mask, part, d);
    else
        hipLaunchKernelGGL((metrics_fwd_kernel<TX, TY, false, STRIP>), grid, dim3(threads), lds, s, (const TX*)x, (const TY*)y, mask, part, d);
}

}  // namespace

extern "C" int vvae_recon_metrics_supported(int H, int W, int C, int x_dtype, int y_dtype)
{
    RmDims d; int threads;
    return (x_dtype == VVAE_DT_F32 || x_dtype == VVAE_DT_BF16) && (y_dtype == VVAE_DT_F32 || y_dtype == VVAE_DT_BF16) &&
           rm_dims(1, 1, H, W, C, d, threads);
}

extern "C" size_t vvae_recon_metrics_part_floats(int B, int T, int H, int W, int C)
{
    RmDims d; int threads;
    if (!rm_dims(B, T, H, W, C, d, threads)) return 0;
    return (size_t)B * T * d.bands * 2;
}

// x, y (B, T, H, W, C) contiguous, dtypes VVAE_DT_F32 / VVAE_DT_BF16 each; mask fp32 (B T), nonzero = valid frame; part: scratch of
// vvae_recon_metrics_part_floats floats (every word written before it is read) -> mse, psnr, ssim fp32 (B T).  clamp: clamp to [0, 1].
extern "C" int vvae_recon_metrics_fwd(const void* x, int x_dtype, const void* y, int y_dtype, const float* mask, float* mse, float* psnr,
                                      float* ssim, float* part, int B, int T, int H, int W, int C, int clamp, void* stream)
{
    RmDims d; int threads;
    if (!x || !y || !mask || !mse || !psnr || !ssim || !part || !vvae_recon_metrics_supported(H, W, C, x_dtype, y_dtype) ||
        !rm_dims(B, T, H, W, C, d, threads))
        return VVAE_ERR_BAD_ARG;
    const int ex = x_dtype == VVAE_DT_F32 ? 4 : 2, ey = y_dtype == VVAE_DT_F32 ? 4 : 2;
    if ((uintptr_t)x % ex || (uintptr_t)y % ey || ((uintptr_t)mask | (uintptr_t)mse | (uintptr_t)psnr | (uintptr_t)ssim | (uintptr_t)part) % 4)
        return VVAE_ERR_BAD_ARG;
    d.clamp = clamp ? 1 : 0;
    // one wide load per operand, row and thread when every row starts on a 4-element boundary
    const bool vec = d.L % 4 == 0 && (uintptr_t)x % (4 * ex) == 0 && (uintptr_t)y % (4 * ey) == 0;
    const int F = B * T;
    const size_t lds = ((size_t)5 * d.C * d.P + 16) * 4;
    const dim3 grid(d.bands, F);
    hipStream_t s = (hipStream_t)stream;
    if (x_dtype == VVAE_DT_F32 && y_dtype == VVAE_DT_F32) rm_launch<float, float, false>(vec, grid, threads, lds, s, x, y, mask, part, d);
    else if (x_dtype == VVAE_DT_F32) rm_launch<float, bf16_t, false>(vec, grid, threads, lds, s, x, y, mask, part, d);
    else if (y_dtype == VVAE_DT_F32) rm_launch<bf16_t, float, false>(vec, grid, threads, lds, s, x, y, mask, part, d);
    else rm_launch<bf16_t, bf16_t, false>(vec, grid, threads, lds, s, x, y, mask, part, d);
    VVAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(metrics_fold_kernel, dim3((F + 255) / 256), dim3(256), 0, s, part, mask, mse, psnr, ssim, F, d.bands,
                       (double)H * W * C, (double)(H - 10) * (W - 10) * C);
    VVAE_LAUNCH_CHECK();
    return 0;
}

extern "C" int vvae_recon_metrics_wide_supported(int H, int W, int C, int x_dtype, int y_dtype)
{
    RmWideDims d; int threads;
    return (x_dtype == VVAE_DT_F32 || x_dtype == VVAE_DT_BF16) && (y_dtype == VVAE_DT_F32 || y_dtype == VVAE_DT_BF16) &&
           rm_wide_dims(1, 1, H, W, C, d, threads);
}

extern "C" size_t vvae_recon_metrics_wide_part_floats(int B, int T, int H, int W, int C)
{
    RmWideDims d; int threads;
    if (rm_dims(B, T, H, W, C, d, threads)) return vvae_recon_metrics_part_floats(B, T, H, W, C);
    if (!rm_wide_dims(B, T, H, W, C, d, threads)) return 0;
    return (size_t)B * T * d.strips * d.bands * 2;
}

// vvae_recon_metrics_fwd for 11 <= W <= 8192: a shape that entry takes runs it (bitwise its results); wider rows run the strip path.
extern "C" int vvae_recon_metrics_wide_fwd(const void* x, int x_dtype, const void* y, int y_dtype, const float* mask, float* mse, float* psnr,
                                           float* ssim, float* part, int B, int T, int H, int W, int C, int clamp, void* stream)
{
    RmWideDims d; int threads;
    if (vvae_recon_metrics_supported(H, W, C, x_dtype, y_dtype) && rm_dims(B, T, H, W, C, d, threads))
        return vvae_recon_metrics_fwd(x, x_dtype, y, y_dtype, mask, mse, psnr, ssim, part, B, T, H, W, C, clamp, stream);
    if (!x || !y || !mask || !mse || !psnr || !ssim || !part || !vvae_recon_metrics_wide_supported(H, W, C, x_dtype, y_dtype) ||
        !rm_wide_dims(B, T, H, W, C, d, threads))
        return VVAE_ERR_BAD_ARG;
    const int ex = x_dtype == VVAE_DT_F32 ? 4 : 2, ey = y_dtype == VVAE_DT_F32 ? 4 : 2;
    if ((uintptr_t)x % ex || (uintptr_t)y % ey || ((uintptr_t)mask | (uintptr_t)mse | (uintptr_t)psnr | (uintptr_t)ssim | (uintptr_t)part) % 4)
        return VVAE_ERR_BAD_ARG;
    d.clamp = clamp ? 1 : 0;
    // every strip starts on a 4-element boundary (SW C % 4 == 0), so one alignment test covers them all
    const bool vec = d.L % 4 == 0 && (uintptr_t)x % (4 * ex) == 0 && (uintptr_t)y % (4 * ey) == 0;
    const int F = B * T;
    const size_t lds = ((size_t)5 * d.C * d.P + 16) * 4;
    const dim3 grid(d.bands, F, d.strips);
    hipStream_t s = (hipStream_t)stream;
    if (x_dtype == VVAE_DT_F32 && y_dtype == VVAE_DT_F32) rm_launch<float, float, true>(vec, grid, threads, lds, s, x, y, mask, part, d);
    else if (x_dtype == VVAE_DT_F32) rm_launch<float, bf16_t, true>(vec, grid, threads, lds, s, x, y, mask, part, d);
    else if (y_dtype == VVAE_DT_F32) rm_launch<bf16_t, float, true>(vec, grid, threads, lds, s, x, y, mask, part, d);
    else rm_launch<bf16_t, bf16_t, true>(vec, grid, threads, lds, s, x, y, mask, part, d);
    VVAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(metrics_fold_kernel, dim3((F + 255) / 256), dim3(256), 0, s, part, mask, mse, psnr, ssim, F, d.strips * d.bands,
                       (double)H * W * C, (double)(H - 10) * (W - 10) * C);
    VVAE_LAUNCH_CHECK();
    return 0;
}
