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
//
// MS-SSIM (Wang, Simoncelli, Bovik 2003; vvae_ms_ssim_*, the definition is metrics.py's): M <= 5 levels, level j + 1 the 2 x 2 means of
// level j (an odd trailing row or column dropped), both operands kept as fp32 pyramid levels in the caller's workspace.
//   metrics_fwd_kernel with MS = true (both strip forms): no squared error; per position CS = (2 sxy + C2) / (sx + sy + C2) and
//     S = (2 mx my + C1) / (mx^2 + my^2 + C1) CS, summed per channel.  A horizontal-pass thread owns one channel (hc), so the fixed
//     order is: every thread's (S, CS) sums go to LDS (the planes are free after the last row), then thread c < C adds the threads
//     c ng .. (c + 1) ng - 1 of its channel in ascending order.  One (S, CS) pair per (frame, strip, band, channel).  Bands go down to
//     4 rows (16 in the single-scale form): the small levels cannot fill the chip, so a workgroup's own rows + 10 are what they cost.
//   ms_pool_kernel: one launch per level transition, both operands: v' = ((v00 + v01) + (v10 + v11)) 0.25 in fp32, contraction off.
//     Level 0 reads the caller's tensors (and clamps them), later levels the fp32 pyramid.  A thread owns 4 output pixels (C 16-B
//     stores from 16-B loads of 8 input pixels of two rows) where every row of both levels starts on 16 bytes, one output element
//     otherwise.  Frames on grid.y with a stride loop; masked frames are skipped, their pyramid slots never written or read.
//   ms_fold_kernel: one thread per frame; per level and channel the (strip, band) partials in that order in fp32, divided by the
//     level's valid positions in double; then mean over c of prod_j max(term_j[c], 0)^w_j in double (CS below the last level, S there).
// 2 M launches (M moment passes, M - 1 pools, the fold); every workspace word is written before it is read; no atomics, no memset.
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
// MS: the multi-scale form (file header): S and CS per channel, C pairs per (frame, strip, band), nothing for a masked frame
template <typename TX, typename TY, bool VEC, bool STRIP, bool MS = false>
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
    if constexpr (MS) {
        out = part + (((long)f * gridDim.z + strip) * d.bands + band) * 2 * d.C;     // gridDim.z = the strips (1 without them)
        if (mask[f] == 0.f) return;          // padding: never read, and the fold never reads its partials
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
    if constexpr (STRIP && !MS) {
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
    [[maybe_unused]] float cs = 0.f;         // MS: the sum of CS beside the sum of S
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
            if constexpr (!MS) {
                if (r >= r0 && r < r1) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float dd = xr[s][i] - yr[s][i];
                        if (mse_col[i]) se = fmaf(dd, dd, se);
                    }
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
                    const int j = j0 + i;
                    if constexpr (MS) {
                        const float cst = (2.f * vxy + C2) / (vx + vy + C2);
                        const float lum = (2.f * ux * uy + C1) / (ux * ux + uy * uy + C1);
                        const bool in = j >= 5 && j <= W - 6;
                        cs += in ? cst : 0.f;
                        ss += in ? lum * cst : 0.f;
                    } else {
                        const float num = (2.f * ux * uy + C1) * (2.f * vxy + C2);
                        const float den = (ux * ux + uy * uy + C1) * (vx + vy + C2);
                        ss += (j >= 5 && j <= W - 6) ? num / den : 0.f;
                    }
                }
            }
            __syncthreads();                 // the LDS row is rewritten by the next output row
        }
    }

    if constexpr (MS) {
        // per channel, in a fixed order: the planes are free (the loop ends on a barrier), every thread parks its sums there and
        // thread c adds the ng horizontal-pass threads of channel c in ascending order
        const int nt = blockDim.x;
        lds[tid] = ss;
        lds[nt + tid] = cs;
        __syncthreads();
        if (tid < d.C) {
            float a0 = 0.f, a1 = 0.f;
            for (int t = tid * ng; t < (tid + 1) * ng; ++t) { a0 += lds[t]; a1 += lds[nt + t]; }
            out[2 * tid] = a0;
            out[2 * tid + 1] = a1;
        }
        return;
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

template <typename TX, typename TY, bool STRIP, bool MS = false>
void rm_launch(bool vec, dim3 grid, int threads, size_t lds, hipStream_t s, const void* x, const void* y, const float* mask, float* part,
               const RmDimsOf<STRIP>& d)
{
    if (vec)
        hipLaunchKernelGGL((metrics_fwd_kernel<TX, TY, true, STRIP, MS>), grid, dim3(threads), lds, s, (const TX*)x, (const TY*)y, mask, part, d);
    else
        hipLaunchKernelGGL((metrics_fwd_kernel<TX, TY, false, STRIP, MS>), grid, dim3(threads), lds, s, (const TX*)x, (const TY*)y, mask, part, d);
}

// ---- MS-SSIM: the pyramid, the fold over levels, the plan of a call (file header) -------------------------------------------------
constexpr int MS_MAX_SCALES = 5;
constexpr int MS_MIN_BAND = 4;               // rows per band at least: the small levels leave the chip idle, and a workgroup's time is its
                                             // rows + 10 halo rows at about a microsecond each, so shorter bands finish sooner

// the bands of an MS-SSIM level: as rm_bands_taps, down to MS_MIN_BAND rows
void ms_bands(RmDims& d, long groups)
{
    int bands = (int)((RM_TARGET_WGS + groups - 1) / groups);
    const int most = (d.H + MS_MIN_BAND - 1) / MS_MIN_BAND;
    if (bands > most) bands = most;
    if (bands < 1) bands = 1;
    d.R = (d.H + bands - 1) / bands;
    d.bands = (d.H + d.R - 1) / d.R;
}

struct MsPoolDims {
    int H, W, C, Ho, Wo, F, clamp;           // frames of H x W x C -> Ho x Wo x C = H / 2 x W / 2 x C
};

// 8 CV consecutive values (8 pixels of a row) by 16-B loads
template <typename T, int CV>
__device__ __forceinline__ void ms_load_px8(const T* __restrict__ p, int clamp, float (&v)[8 * CV])
{
    constexpr int N = VecWidth<T>::value;
#pragma unroll
    for (int q = 0; q < 8 * CV / N; ++q) {
        float t[N];
        VecIO<T, N>::load(p + q * N, t);
#pragma unroll
        for (int i = 0; i < N; ++i) v[q * N + i] = rm_prep(t[i], clamp);
    }
}

// 4 output pixels of one operand from 8 pixels of the rows r0 and r1: C 16-B stores
template <typename T, int CV>
__device__ __forceinline__ void ms_pool_group(const T* __restrict__ r0, const T* __restrict__ r1, float* __restrict__ o, int clamp)
{
#pragma clang fp contract(off)
    float a[8 * CV], b[8 * CV];
    ms_load_px8<T, CV>(r0, clamp, a);
    ms_load_px8<T, CV>(r1, clamp, b);
#pragma unroll
    for (int q = 0; q < CV; ++q) {
        float w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = 4 * q + i, k = e / CV, c = e - k * CV, s = 2 * k * CV + c;
            w[i] = ((a[s] + a[s + CV]) + (b[s] + b[s + CV])) * 0.25f;
        }
        VecIO<float, 4>::store(o + 4 * q, w);
    }
}

// one output element: v points at the input element (2 i, 2 k, c); its row pitch is L
template <typename T>
__device__ __forceinline__ float ms_pool_at(const T* __restrict__ v, int C, int L, int clamp)
{
#pragma clang fp contract(off)
    const float v00 = rm_prep(ldf(v), clamp), v01 = rm_prep(ldf(v + C), clamp);
    const float v10 = rm_prep(ldf(v + L), clamp), v11 = rm_prep(ldf(v + L + C), clamp);
    return ((v00 + v01) + (v10 + v11)) * 0.25f;
}

// CV = C in 1 .. 4: the 16-B form, a thread per (output row, group of 4 output pixels); a row's last group of fewer than 4 pixels
// goes element by element.  CV = 0: a thread per output element, any C.  grid (units / 256, frames with a stride loop).
template <typename TX, typename TY, int CV>
__global__ __launch_bounds__(256) void ms_pool_kernel(const TX* __restrict__ x, const TY* __restrict__ y, const float* __restrict__ mask,
                                                      float* __restrict__ ox, float* __restrict__ oy, MsPoolDims d)
{
    const int L = d.W * d.C, Lo = d.Wo * d.C;
    const long fin = (long)d.H * L, fout = (long)d.Ho * Lo;
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (CV > 0) {
        const int G = (d.Wo + 3) / 4;
        if (u >= (long)d.Ho * G) return;
        const int i = (int)(u / G), g = (int)(u - (long)i * G);
        const int np = min(4, d.Wo - 4 * g);
        const long in0 = (long)(2 * i) * L + 8 * g * CV, o0 = (long)i * Lo + 4 * g * CV;
        for (int f = blockIdx.y; f < d.F; f += gridDim.y) {
            if (mask[f] == 0.f) continue;    // padding: never read, its slot never written
            const TX* xf = x + f * fin + in0;
            const TY* yf = y + f * fin + in0;
            float* oxf = ox + f * fout + o0;
            float* oyf = oy + f * fout + o0;
            if (np == 4) {
                ms_pool_group<TX, CV>(xf, xf + L, oxf, d.clamp);
                ms_pool_group<TY, CV>(yf, yf + L, oyf, d.clamp);
            } else {
                for (int e = 0; e < np * CV; ++e) {
                    const int k = e / CV, s = e + k * CV;
                    oxf[e] = ms_pool_at(xf + s, CV, L, d.clamp);
                    oyf[e] = ms_pool_at(yf + s, CV, L, d.clamp);
                }
            }
        }
    } else {
        if (u >= fout) return;
        const long i = u / Lo;
        const int e = (int)(u - i * Lo), k = e / d.C;
        const long in0 = 2 * i * L + e + k * d.C;
        for (int f = blockIdx.y; f < d.F; f += gridDim.y) {
            if (mask[f] == 0.f) continue;
            ox[f * fout + u] = ms_pool_at(x + f * fin + in0, d.C, L, d.clamp);
            oy[f * fout + u] = ms_pool_at(y + f * fin + in0, d.C, L, d.clamp);
        }
    }
}

struct MsFoldDims {
    long off[MS_MAX_SCALES];                 // a level's partials in the workspace: (frame, strip band, channel, {S, CS})
    int nsb[MS_MAX_SCALES];                  // strips x bands of the level
    double nv[MS_MAX_SCALES], w[MS_MAX_SCALES];      // valid positions per channel, weight
    int M, C;
};

// one thread per frame: per channel the levels' terms (CS below the last level, S there), each the (strip, band) partials in order
// over the level's valid positions -> ms_ssim = mean over c of prod_j max(term, 0)^w_j; terms (F, M, C) when non-NULL
__global__ void ms_fold_kernel(const float* __restrict__ ws, const float* __restrict__ mask, float* __restrict__ ms, float* __restrict__ terms,
                               int F, MsFoldDims d)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    if (mask[f] == 0.f) {
        ms[f] = 0.f;
        if (terms)
            for (int i = 0; i < d.M * d.C; ++i) terms[(long)f * d.M * d.C + i] = 0.f;
        return;
    }
    double acc = 0.0;
    for (int c = 0; c < d.C; ++c) {
        double prod = 1.0;
        for (int j = 0; j < d.M; ++j) {
            const float* p = ws + d.off[j] + ((long)f * d.nsb[j] * d.C + c) * 2 + (j == d.M - 1 ? 0 : 1);
            // ascending (strip, band) order; 8 loads in flight at a time (the partials are cache-resident: latency is what this pays for)
            const long st = (long)d.C * 2;
            const int nsb = d.nsb[j];
            float s = 0.f;
            int b = 0;
            for (; b + 8 <= nsb; b += 8) {
                float v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = p[(b + i) * st];
#pragma unroll
                for (int i = 0; i < 8; ++i) s += v[i];
            }
            for (; b < nsb; ++b) s += p[b * st];
            const double t = (double)s / d.nv[j];
            if (terms) terms[((long)f * d.M + j) * d.C + c] = (float)t;
            prod *= pow(fmax(t, 0.0), d.w[j]);
        }
        acc += prod;
    }
    ms[f] = (float)(acc / d.C);
}

struct MsLevel {
    RmWideDims d;                            // the moment pass of the level (strips = 1, SW = 0 without strips)
    int threads, H, W;
    bool strip;
    size_t pyr, pyr_n;                       // levels >= 1: x at ws + pyr, y at ws + pyr + pyr_n (pyr_n a multiple of 4)
    size_t part;                             // the level's partials at ws + part
};
struct MsPlan {
    MsLevel lv[MS_MAX_SCALES];
    size_t total;
};

bool ms_plan(int B, int T, int H, int W, int C, int M, MsPlan& p)
{
    if (B <= 0 || T <= 0 || (long)B * T > 65535 || C < 1 || C > 4 || M < 1 || M > MS_MAX_SCALES || H < 11 || W < 11 || W > RM_MAX_WIDE_W ||
        (min(H, W) >> (M - 1)) < 11)
        return false;
    const size_t F = (size_t)B * T;
    size_t off = 0;
    for (int j = 0; j < M; ++j) {
        MsLevel& l = p.lv[j];
        l.H = H >> j; l.W = W >> j;
        l.strip = !rm_dims(B, T, l.H, l.W, C, l.d, l.threads);
        if (l.strip) {
            if (!rm_wide_dims(B, T, l.H, l.W, C, l.d, l.threads)) return false;
        } else {
            l.d.SW = 0; l.d.strips = 1;
        }
        ms_bands(l.d, (long)F * l.d.strips);
        if ((size_t)2 * l.threads > (size_t)5 * C * l.d.P + 16) return false;      // the per-channel sums park in the planes
        l.pyr = off; l.pyr_n = 0;
        if (j > 0) {
            l.pyr_n = (F * l.H * l.W * C + 3) / 4 * 4;
            off += 2 * l.pyr_n;
        }
    }
    for (int j = 0; j < M; ++j) {
        p.lv[j].part = off;
        off += (F * p.lv[j].d.strips * p.lv[j].d.bands * C * 2 + 3) / 4 * 4;
    }
    p.total = off;
    return true;
}

inline bool ms_al16(const void* p) { return (uintptr_t)p % 16 == 0; }

// one level: its moment pass and, when `ox` is given, the pool to the next level
template <typename TX, typename TY>
int ms_level_launch(const MsLevel& l, int F, int C, hipStream_t s, const void* x, const void* y, const float* mask, float* part, int clamp,
                    float* ox, float* oy)
{
    const int ex = sizeof(TX), ey = sizeof(TY);
    RmWideDims d = l.d;
    d.clamp = clamp;
    const bool vec = d.L % 4 == 0 && (uintptr_t)x % (4 * ex) == 0 && (uintptr_t)y % (4 * ey) == 0;
    const size_t lds = ((size_t)5 * d.C * d.P + 16) * 4;
    if (l.strip) rm_launch<TX, TY, true, true>(vec, dim3(d.bands, F, d.strips), l.threads, lds, s, x, y, mask, part, d);
    else rm_launch<TX, TY, false, true>(vec, dim3(d.bands, F), l.threads, lds, s, x, y, mask, part, d);
    VVAE_LAUNCH_CHECK();
    if (!ox) return 0;
    MsPoolDims pd;
    pd.H = l.H; pd.W = l.W; pd.C = C; pd.Ho = l.H / 2; pd.Wo = l.W / 2; pd.F = F; pd.clamp = clamp;
    const long L = (long)l.W * C, Lo = (long)pd.Wo * C;
    // 16-B accesses: every row of both operands and of both outputs starts on 16 bytes
    const bool pvec = L * ex % 16 == 0 && L * ey % 16 == 0 && Lo % 4 == 0 && ms_al16(x) && ms_al16(y) && ms_al16(ox) && ms_al16(oy);
    const long units = pvec ? (long)pd.Ho * ((pd.Wo + 3) / 4) : (long)pd.Ho * Lo;
    const long gx = (units + 255) / 256;
    long gy = 8192 / gx;
    if (gy < 1) gy = 1;
    if (gy > F) gy = F;
    const dim3 grid((unsigned)gx, (unsigned)gy);
#define MS_POOL(CV) hipLaunchKernelGGL((ms_pool_kernel<TX, TY, CV>), grid, dim3(256), 0, s, (const TX*)x, (const TY*)y, mask, ox, oy, pd)
    switch (pvec ? C : 0) {
    case 1: MS_POOL(1); break;
    case 2: MS_POOL(2); break;
    case 3: MS_POOL(3); break;
    case 4: MS_POOL(4); break;
    default: MS_POOL(0); break;
    }
#undef MS_POOL
    VVAE_LAUNCH_CHECK();
    return 0;
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

extern "C" int vvae_ms_ssim_supported(int H, int W, int C, int scales, int x_dtype, int y_dtype)
{
    MsPlan p;
    return (x_dtype == VVAE_DT_F32 || x_dtype == VVAE_DT_BF16) && (y_dtype == VVAE_DT_F32 || y_dtype == VVAE_DT_BF16) &&
           ms_plan(1, 1, H, W, C, scales, p);
}

extern "C" size_t vvae_ms_ssim_ws_floats(int B, int T, int H, int W, int C, int scales)
{
    MsPlan p;
    return ms_plan(B, T, H, W, C, scales, p) ? p.total : 0;
}

// x, y (B, T, H, W, C) contiguous, dtypes VVAE_DT_F32 / VVAE_DT_BF16 each; mask fp32 (B T), nonzero = valid frame; ws: scratch of
// vvae_ms_ssim_ws_floats floats (the fp32 pyramid of both operands, then every level's partials; every word written before it is
// read) -> ms_ssim fp32 (B T), terms fp32 (B T, scales, C) or NULL.  w0 .. w4: the weights, those past `scales` ignored.
extern "C" int vvae_ms_ssim_fwd(const void* x, int x_dtype, const void* y, int y_dtype, const float* mask, float* ms_ssim, float* terms,
                                float* ws, int B, int T, int H, int W, int C, int scales, double w0, double w1, double w2, double w3,
                                double w4, int clamp, void* stream)
{
    MsPlan p;
    if (!x || !y || !mask || !ms_ssim || !ws || !vvae_ms_ssim_supported(H, W, C, scales, x_dtype, y_dtype) ||
        !ms_plan(B, T, H, W, C, scales, p))
        return VVAE_ERR_BAD_ARG;
    const int ex = x_dtype == VVAE_DT_F32 ? 4 : 2, ey = y_dtype == VVAE_DT_F32 ? 4 : 2;
    if ((uintptr_t)x % ex || (uintptr_t)y % ey || ((uintptr_t)mask | (uintptr_t)ms_ssim | (uintptr_t)terms | (uintptr_t)ws) % 4)
        return VVAE_ERR_BAD_ARG;
    const double w[MS_MAX_SCALES] = {w0, w1, w2, w3, w4};
    for (int j = 0; j < scales; ++j)
        if (!(w[j] >= 0.0) || w[j] > 1e300) return VVAE_ERR_BAD_ARG;
    const int F = B * T;
    hipStream_t s = (hipStream_t)stream;
    MsFoldDims fd;
    fd.M = scales; fd.C = C;
    for (int j = 0; j < MS_MAX_SCALES; ++j) { fd.off[j] = 0; fd.nsb[j] = 0; fd.nv[j] = 1.0; fd.w[j] = 0.0; }
    for (int j = 0; j < scales; ++j) {
        const MsLevel& l = p.lv[j];
        fd.off[j] = (long)l.part;
        fd.nsb[j] = l.d.strips * l.d.bands;
        fd.nv[j] = (double)(l.H - 10) * (l.W - 10);
        fd.w[j] = w[j];
        float* ox = j + 1 < scales ? ws + p.lv[j + 1].pyr : nullptr;
        float* oy = ox ? ox + p.lv[j + 1].pyr_n : nullptr;
        int rc;
        if (j > 0) {
            const float* lx = ws + l.pyr;
            rc = ms_level_launch<float, float>(l, F, C, s, lx, lx + l.pyr_n, mask, ws + l.part, 0, ox, oy);
        } else if (x_dtype == VVAE_DT_F32 && y_dtype == VVAE_DT_F32) {
            rc = ms_level_launch<float, float>(l, F, C, s, x, y, mask, ws + l.part, clamp ? 1 : 0, ox, oy);
        } else if (x_dtype == VVAE_DT_F32) {
            rc = ms_level_launch<float, bf16_t>(l, F, C, s, x, y, mask, ws + l.part, clamp ? 1 : 0, ox, oy);
        } else if (y_dtype == VVAE_DT_F32) {
            rc = ms_level_launch<bf16_t, float>(l, F, C, s, x, y, mask, ws + l.part, clamp ? 1 : 0, ox, oy);
        } else {
            rc = ms_level_launch<bf16_t, bf16_t>(l, F, C, s, x, y, mask, ws + l.part, clamp ? 1 : 0, ox, oy);
        }
        if (rc) return rc;
    }
    hipLaunchKernelGGL(ms_fold_kernel, dim3((F + 255) / 256), dim3(256), 0, s, ws, mask, ms_ssim, terms, F, fd);
    VVAE_LAUNCH_CHECK();
    return 0;
}
