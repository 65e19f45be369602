// Scene-cut detection (video_vae_amd/scenes.py): per-frame colour histograms of a uint8 RGB clip (L, H, W, 3) and the correlation of
// consecutive histograms, the two quantities the change-point rule of scenes.change_indices reads.
//
//   space 0 (HSV): OpenCV's 8-bit RGB -> HSV (hsv_shift 12, the rounded sdiv / hdiv tables), then a 2-D (H, S) histogram of n x n bins,
//                  bin = hbin[h] n + sbin[s];
//   space 1 (gray): OpenCV's 8-bit RGB -> gray, Y = (4899 R + 9617 G + 1868 B + 8192) >> 14, bin = gbin[Y].
//
// All four 256-entry tables (sdiv, hdiv and the two bin tables, or the gray bin table) come from the caller, so no floating-point
// binning happens here.  Counts are exact integers:
//   scene_hist_part_kernel: one workgroup per (frame, chunk); a frame of n pixels is ceil(n / SH_CHUNK) chunks of equal size (a multiple
//     of 4 pixels, the last one shorter), so no workgroup is left nearly empty; an LDS histogram of the chunk, updated with LDS
//     integer adds that stay inside the workgroup.  Each thread keeps a run (bin, count) in registers and adds it only when the bin
//     changes, so a solid-colour frame costs one LDS add per thread and chunk instead of one per pixel.  The chunk's counts are
//     written to part (or straight to counts when a frame is one chunk).
//   scene_hist_fold_kernel: counts[f][b] = sum over the chunks of part, one thread per (frame, bin).
//   scene_corr_kernel: one workgroup per pair of consecutive frames; s1, s2, s11, s22, s12 as exact 64-bit integer sums, then
//     cv2.HISTCMP_CORREL in float64 in one thread.
// No global atomics, no float atomics, no fill launch: counts and correlations are bitwise reproducible.
#include "common.hpp"

#include <cfloat>

namespace {

constexpr int SH_THREADS = 256;
constexpr int SH_UNROLL = 4;                                   // 4-pixel groups loaded before any is binned
constexpr int SH_STEPS = 128;                                  // 4-pixel groups per thread and chunk
constexpr int SH_CHUNK = SH_THREADS * SH_STEPS * 4;            // most pixels of a frame per workgroup (131072)
constexpr int SH_MAX_BINS = 4096;
constexpr int SH_MAX_W = 8192;
constexpr int SH_MAX_H = 16384;

// tabs: space 0: [sdiv | hdiv | hbin | sbin], space 1: [gbin], 256 int32 each
template <int SPACE>
__device__ __forceinline__ int sh_bin(unsigned r, unsigned g, unsigned b, const int* __restrict__ t, int n)
{
    if (SPACE == 1) return t[(r * 4899u + g * 9617u + b * 1868u + 8192u) >> 14];
    const int ir = (int)r, ig = (int)g, ib = (int)b;
    const int v = max(max(ir, ig), ib);
    const int diff = v - min(min(ir, ig), ib);
    const int s = (diff * t[v] + 2048) >> 12;
    int h = v == ir ? ig - ib : v == ig ? ib - ir + 2 * diff : ir - ig + 4 * diff;
    h = (h * t[256 + diff] + 2048) >> 12;                      // arithmetic shift of a signed value
    h += h < 0 ? 180 : 0;
    return t[512 + h] * n + t[768 + s];
}

// bytes q = 0 .. 11 of three little-endian words
__device__ __forceinline__ unsigned sh_byte(const unsigned (&w)[3], int q) { return (w[q >> 2] >> ((q & 3) * 8)) & 0xffu; }

__device__ __forceinline__ void sh_push(int bin, int& cur, unsigned& run, unsigned* __restrict__ hist)
{
    if (bin != cur) {
        if (run) atomicAdd(hist + cur, run);
        cur = bin;
        run = 0;
    }
    ++run;
}

// blockIdx.x = frame chunks + chunk, the chunk = pixels [chunk cpx, min((chunk + 1) cpx, n)); out = part + blockIdx.x bins (or counts +
// frame bins when chunks == 1: the same index)
// VEC: n % 4 == 0 and the clip 4-byte aligned: a 4-pixel group is three aligned words
template <int SPACE, bool VEC>
__global__ __launch_bounds__(SH_THREADS) void scene_hist_part_kernel(const uint8_t* __restrict__ clip, const int* __restrict__ tabs,
                                                                     unsigned* __restrict__ out, long n, int chunks, long cpx, int hn,
                                                                     int bins)
{
    __shared__ unsigned hist[SH_MAX_BINS];
    __shared__ int tab[1024];
    const int ntab = SPACE == 1 ? 256 : 1024;
    for (int i = threadIdx.x; i < ntab; i += SH_THREADS) tab[i] = tabs[i];
    for (int i = threadIdx.x; i < bins; i += SH_THREADS) hist[i] = 0u;
    __syncthreads();
    const long blk = blockIdx.x;
    const long f = blk / chunks;
    const long p0 = (blk - f * chunks) * cpx;
    const long p1 = min(p0 + cpx, n);
    const uint8_t* src = clip + f * n * 3;
    int cur = 0;
    unsigned run = 0;
    if (VEC) {
        const unsigned* wsrc = reinterpret_cast<const unsigned*>(src);
        for (long g0 = p0 / 4 + threadIdx.x; g0 < p1 / 4; g0 += (long)SH_THREADS * SH_UNROLL) {
            unsigned w[SH_UNROLL][3];
#pragma unroll
            for (int u = 0; u < SH_UNROLL; ++u) {
                const long g = g0 + (long)u * SH_THREADS;
                if (g < p1 / 4) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) w[u][k] = wsrc[g * 3 + k];
                }
            }
#pragma unroll
            for (int u = 0; u < SH_UNROLL; ++u) {
                if (g0 + (long)u * SH_THREADS < p1 / 4) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        sh_push(sh_bin<SPACE>(sh_byte(w[u], 3 * q), sh_byte(w[u], 3 * q + 1), sh_byte(w[u], 3 * q + 2), tab, hn),
                                cur, run, hist);
                }
            }
        }
    } else {
        for (long p = p0 + threadIdx.x; p < p1; p += SH_THREADS)
            sh_push(sh_bin<SPACE>(src[p * 3], src[p * 3 + 1], src[p * 3 + 2], tab, hn), cur, run, hist);
    }
    if (run) atomicAdd(hist + cur, run);
    __syncthreads();
    unsigned* dst = out + blk * bins;
    for (int i = threadIdx.x; i < bins; i += SH_THREADS) dst[i] = hist[i];
}

// blockIdx.x = frame ceil(bins / 256) + j: counts[frame][j 256 + tid] = sum over chunks c (ascending) of part[frame chunks + c][...]
__global__ __launch_bounds__(SH_THREADS) void scene_hist_fold_kernel(const unsigned* __restrict__ part, unsigned* __restrict__ counts,
                                                                     int chunks, int bins)
{
    const int per = (bins + SH_THREADS - 1) / SH_THREADS;
    const long f = blockIdx.x / per;
    const int b = (int)(blockIdx.x - f * per) * SH_THREADS + threadIdx.x;
    if (b >= bins) return;
    const unsigned* src = part + f * chunks * (long)bins + b;
    unsigned s = 0u;
    for (int c = 0; c < chunks; ++c) s += src[(long)c * bins];
    counts[f * bins + b] = s;
}

// one workgroup per pair (f, f + 1): corr[f] = HISTCMP_CORREL(counts[f], counts[f + 1]) over `bins` bins
__global__ __launch_bounds__(SH_THREADS) void scene_corr_kernel(const unsigned* __restrict__ counts, double* __restrict__ corr, int bins)
{
#pragma clang fp contract(off)
    __shared__ unsigned long long red[5][SH_THREADS];
    const long f = blockIdx.x;
    const unsigned* a = counts + f * bins;
    const unsigned* b = a + bins;
    unsigned long long s1 = 0, s2 = 0, s11 = 0, s22 = 0, s12 = 0;
    for (int i = threadIdx.x; i < bins; i += SH_THREADS) {
        const unsigned long long x = a[i], y = b[i];
        s1 += x;
        s2 += y;
        s11 += x * x;
        s22 += y * y;
        s12 += x * y;
    }
    red[0][threadIdx.x] = s1;
    red[1][threadIdx.x] = s2;
    red[2][threadIdx.x] = s11;
    red[3][threadIdx.x] = s22;
    red[4][threadIdx.x] = s12;
    __syncthreads();
    for (int h = SH_THREADS / 2; h > 0; h >>= 1) {             // integer sums: exact in any order
        if ((int)threadIdx.x < h) {
#pragma unroll
            for (int k = 0; k < 5; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double d1 = (double)red[0][0], d2 = (double)red[1][0], d11 = (double)red[2][0], d22 = (double)red[3][0];
        const double d12 = (double)red[4][0];
        const double scale = 1.0 / (double)bins;
        const double num = d12 - d1 * d2 * scale;
        const double denom2 = (d11 - d1 * d1 * scale) * (d22 - d2 * d2 * scale);
        corr[f] = fabs(denom2) > DBL_EPSILON ? num / sqrt(denom2) : 1.0;
    }
}

int sh_bins(int hist_size, int space) { return space == 0 ? hist_size * hist_size : hist_size; }

template <int SPACE>
void sh_part_launch(const uint8_t* clip, const int* tabs, unsigned* out, long n, int chunks, long cpx, int hn, int bins, long blocks,
                    bool vec, hipStream_t s)
{
    if (vec)
        hipLaunchKernelGGL((scene_hist_part_kernel<SPACE, true>), dim3((unsigned)blocks), dim3(SH_THREADS), 0, s, clip, tabs, out, n, chunks,
                           cpx, hn, bins);
    else
        hipLaunchKernelGGL((scene_hist_part_kernel<SPACE, false>), dim3((unsigned)blocks), dim3(SH_THREADS), 0, s, clip, tabs, out, n, chunks,
                           cpx, hn, bins);
}

}  // namespace

extern "C" int vvae_scene_hist_supported(int H, int W, int hist_size, int space)
{
    const bool sz = space == 0 ? hist_size >= 1 && hist_size <= 64 : space == 1 && hist_size >= 1 && hist_size <= 256;
    return sz && H >= 1 && W >= 1 && H <= SH_MAX_H && W <= SH_MAX_W;
}

extern "C" size_t vvae_scene_hist_part_bytes(int L, int H, int W, int hist_size, int space)
{
    if (L <= 0 || !vvae_scene_hist_supported(H, W, hist_size, space)) return 0;
    const long chunks = ceil_div((long)H * W, SH_CHUNK);
    if (chunks == 1) return 0;                                 // one chunk per frame: its counts are the frame's
    return (size_t)L * chunks * sh_bins(hist_size, space) * sizeof(unsigned);
}

extern "C" int vvae_scene_hist_fwd(const void* clip, const int* tabs, unsigned* counts, double* corr, void* part, int L, int H, int W,
                                   int hist_size, int space, void* stream)
{
    if (!clip || !tabs || !counts || L <= 0 || !vvae_scene_hist_supported(H, W, hist_size, space) || (uintptr_t)tabs % 4 ||
        (uintptr_t)counts % 4)
        return VVAE_ERR_BAD_ARG;
    if (L > 1 && (!corr || (uintptr_t)corr % 8)) return VVAE_ERR_BAD_ARG;
    const long n = (long)H * W;
    const int chunks = ceil_div(n, SH_CHUNK);
    const int bins = sh_bins(hist_size, space);
    if (chunks > 1 && (!part || (uintptr_t)part % 4)) return VVAE_ERR_BAD_ARG;
    const long blocks = (long)L * chunks;
    const long fold_blocks = (long)L * ceil_div(bins, SH_THREADS);
    if (blocks > 0x7fffffffL || fold_blocks > 0x7fffffffL) return VVAE_ERR_BAD_ARG;
    const long cpx = ((n + chunks - 1) / chunks + 3) / 4 * 4;    // <= SH_CHUNK; chunks - 1 of them cover fewer than n pixels
    const bool vec = n % 4 == 0 && (uintptr_t)clip % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
    unsigned* out = chunks == 1 ? counts : (unsigned*)part;
    if (space == 0) sh_part_launch<0>((const uint8_t*)clip, tabs, out, n, chunks, cpx, hist_size, bins, blocks, vec, s);
    else sh_part_launch<1>((const uint8_t*)clip, tabs, out, n, chunks, cpx, hist_size, bins, blocks, vec, s);
    VVAE_LAUNCH_CHECK();
    if (chunks > 1) {
        hipLaunchKernelGGL(scene_hist_fold_kernel, dim3((unsigned)fold_blocks), dim3(SH_THREADS), 0, s, (const unsigned*)part, counts, chunks,
                           bins);
        VVAE_LAUNCH_CHECK();
    }
    if (L > 1) {
        hipLaunchKernelGGL(scene_corr_kernel, dim3((unsigned)(L - 1)), dim3(SH_THREADS), 0, s, (const unsigned*)counts, corr, bins);
        VVAE_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int vvae_scene_hist_corr(const unsigned* counts, double* corr, int L, int bins, void* stream)
{
    if (!counts || !corr || L < 2 || bins < 1 || bins > SH_MAX_BINS || (uintptr_t)counts % 4 || (uintptr_t)corr % 8) return VVAE_ERR_BAD_ARG;
    hipLaunchKernelGGL(scene_corr_kernel, dim3((unsigned)(L - 1)), dim3(SH_THREADS), 0, (hipStream_t)stream, counts, corr, bins);
    VVAE_LAUNCH_CHECK();
    return 0;
}
