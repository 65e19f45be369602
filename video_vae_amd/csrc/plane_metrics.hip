// Plane-wise metrics of two sets of 8-bit Y'CbCr planes (video_vae_amd/plane_metrics.py states the definition): per frame the exact
// integer squared error of the Y, U and V planes and metrics.py's SSIM of the Y plane taken as a one-channel frame y / 255.
//
// Operands are views, as vvae_yuv_to_rgb_u8 takes them: three byte pointers and two frame strides per operand, rows dense inside a frame,
// any base alignment -- the planes of frame records uploaded as they lie in a .y4m file.  A thread reads 4 consecutive bytes of a row as
// one dword where the address lies on a dword, as two 16-bit words where it lies on a word, else as bytes, per operand; a group that
// crosses the end of the row (or of the chunk) reads its own bytes only.  No byte outside the planes is ever read.
//
// plane_metrics_y_kernel: blockIdx.x = (strip, band), blockIdx.y = frame (grid-stride over frames).  A workgroup spans PM_SPAN columns
// (4 per thread); wider frames run in column strips: strip s owns the SSIM columns [5 + s SW, min(5 + (s + 1) SW, W - 5)) and reads the
// frame columns [s SW, s SW + SW + 10) (SW a multiple of 4, at most PM_STRIP).  Its squared-error columns are the same ones, widened to
// 0 on the first strip and to W on the last, so the strips partition both.  The thread marches down its band with the last 11 rows of
// both operands in a register ring, PACKED (4 pixels per VGPR: 22 registers).  Per output row it unpacks them (v_cvt_f32_ubyte0..3) and
// forms, for the rows k and 10 - k that share a tap, x + x', x^2 + x'^2, x y + x' y' (and the same for y) in fp32 -- integers up to
// 130 050, exact -- and from them the vertically filtered mx, my, x^2, y^2, xy in DOUBLE, which go to LDS; after a barrier it runs the
// horizontal 11 taps in double from 10 aligned 16-B LDS reads per quantity.  Why double: the variances are differences of numbers up to
// 65 025 that must be right to about 1e-3 (C2 255^2 = 58.5) -- about 30 bits; with fp32 sums two constant planes are off by up to 7e-4
// in S, the same at every position.  Values stay 0 .. 255, C1 and C2 are scaled by 255^2, which leaves S unchanged; S itself is formed
// and summed in fp32.  The squared error of the band's own rows comes from the same packed words, in integers: a thread sums at most
// 4 columns x 8192 rows = 32 768 samples, and a uint32 holds 66 051 of the worst case 255^2.  The 5 halo rows above and below a band
// are re-read (from cache).
// plane_metrics_c_kernel: the chroma planes are dense runs of CH CW bytes; blockIdx.x = (plane, chunk of PM_CCHUNK bytes), a thread sums
// PM_CCHUNK / 256 = 64 samples in a uint32.
// Reductions: per-thread sums, a wave butterfly (64-bit for the integers), the waves in order, one partial per (frame, strip, band) and
// per (frame, plane, chunk); plane_metrics_fold_kernel: one wave per frame, lane l takes the partials l, l + 64, ... in order, then the
// butterfly.  No atomics, no memset, no allocation; every workspace word that is read was written by the launch before; bitwise
// reproducible; three launches for any n (two for mono); safe inside a captured hipGraph.
#include "ssim_window.hpp"

namespace {

constexpr int PM_THREADS = 256;
constexpr int PM_SPAN = 1024;                // columns one workgroup spans: 4 per thread
constexpr int PM_STRIP = 1012;               // SSIM columns per strip at most: a multiple of 4, PM_STRIP + 10 <= PM_SPAN
constexpr int PM_P = PM_SPAN + 16;           // an LDS plane: column j at j + 8, the margins stay 0
constexpr int PM_MIN_BAND = 16;              // rows per band at least (halo overhead 10 / band rows)
constexpr int PM_TARGET_WGS = 2048;          // bands are split until the grid has about this many workgroups
constexpr int PM_MIN_SIDE = 11;
constexpr int PM_MAX_SIDE = 8192;
constexpr int PM_CCHUNK = 16384;             // chroma bytes per workgroup: 64 per thread
constexpr int PM_MAX_GRID_Y = 65535;

enum { CH_420 = 0, CH_444 = 1, CH_MONO = 2 };

struct PmYPart {
    unsigned long long se;
    float ss;
    float unused;
};

struct PmDims {
    int n, H, W, bands, R, strips, SW;
    long ays, bys;                           // frame strides of the Y planes in bytes
    double g[11];
};

// the first nb (<= 4; none when nb <= 0) bytes at p packed into a word, byte i at bits 8 i, the others 0
__device__ __forceinline__ uint32_t pm_load4(const uint8_t* p, int nb)
{
    if (nb >= 4) {
        const unsigned m = (unsigned)((uintptr_t)p & 3);
        if (m == 0) return *reinterpret_cast<const uint32_t*>(p);
        if (m == 2)
            return (uint32_t)*reinterpret_cast<const uint16_t*>(p) | ((uint32_t)*reinterpret_cast<const uint16_t*>(p + 2) << 16);
    }
    uint32_t w = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < nb) w |= (uint32_t)p[i] << (8 * i);
    return w;
}

__device__ __forceinline__ float pm_px(uint32_t w, int i) { return (float)((w >> (8 * i)) & 255u); }

// the sum over the 4 bytes of (a - b)^2 where keep[i]
__device__ __forceinline__ uint32_t pm_se4(uint32_t a, uint32_t b, const bool (&keep)[4])
{
    uint32_t s = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int d = (int)((a >> (8 * i)) & 255u) - (int)((b >> (8 * i)) & 255u);
        s += keep[i] ? (uint32_t)(d * d) : 0u;
    }
    return s;
}

__device__ __forceinline__ unsigned long long pm_wave_sum(unsigned long long v)
{
#define PM_STEP(O)                                                                                           \
    {                                                                                                        \
        const unsigned lo = xor_lane_u32<O>((unsigned)v), hi = xor_lane_u32<O>((unsigned)(v >> 32));         \
        v += ((unsigned long long)hi << 32) | lo;                                                            \
    }
    PM_STEP(32) PM_STEP(16) PM_STEP(8) PM_STEP(4) PM_STEP(2) PM_STEP(1)
#undef PM_STEP
    return v;
}

__global__ __launch_bounds__(PM_THREADS) void plane_metrics_y_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                     PmYPart* __restrict__ part, PmDims d)
{
    __shared__ __attribute__((aligned(16))) double lds[5 * PM_P];
    __shared__ unsigned long long red_se[PM_THREADS / 64];
    __shared__ float red_ss[PM_THREADS / 64];
    const int tid = threadIdx.x;
    const int strip = blockIdx.x / d.bands, band = blockIdx.x - strip * d.bands;
    const int col0 = strip * d.SW;
    const int W = min(col0 + d.SW + 10, d.W) - col0;                   // the strip's columns [col0, col0 + W) of the frame
    for (int i = tid; i < 5 * PM_P; i += blockDim.x) lds[i] = 0.0;

    const auto [r0, r1, ra, re, any] = ssim_rows(band, d.R, d.H);

    // the thread's columns e0 .. e0 + 3 of the strip: nb of them exist; the horizontal pass owns the same four as output columns
    const int e0 = tid * 4;
    const int nb = min(4, W - e0);
    const int mlo = strip == 0 ? 0 : 5, mhi = strip == d.strips - 1 ? W : W - 5;
    bool se_col[4], lds_col[4], ss_col[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = e0 + i;
        se_col[i] = j >= mlo && j < mhi;
        lds_col[i] = j < W;
        ss_col[i] = j >= 5 && j <= W - 6;
    }
    const bool hact = e0 + 3 >= 5 && e0 <= W - 6;
    const double* hrow = lds + e0;
    double g[6];                                                       // the taps are symmetric: g[k] = g[10 - k]
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = d.g[k];
    const double C1 = 6.5025, C2 = 58.5225;                            // 0.01^2 and 0.03^2 times 255^2
    __syncthreads();                                                   // LDS zeroed

    for (int f = blockIdx.y; f < d.n; f += gridDim.y) {
        const uint8_t* af = a + (long)f * d.ays + col0 + e0;
        const uint8_t* bf = b + (long)f * d.bys + col0 + e0;
        uint32_t xr[11], yr[11];
        uint32_t se = 0u;
        float ss = 0.f;
        uint32_t nx = pm_load4(af + (long)ra * d.W, nb), ny = pm_load4(bf + (long)ra * d.W, nb);
        for (int base = ra; base < re; base += 11) {
#pragma unroll
            for (int s = 0; s < 11; ++s) {
                const int r = base + s;
                if (r >= re) break;
                xr[s] = nx;
                yr[s] = ny;
                if (r + 1 < re) {                                      // the next row is in flight while this one is filtered
                    nx = pm_load4(af + (long)(r + 1) * d.W, nb);
                    ny = pm_load4(bf + (long)(r + 1) * d.W, nb);
                }
                if (r >= r0 && r < r1) se += pm_se4(xr[s], yr[s], se_col);
                if (!any || r < ra + 10) continue;
                // output row r - 5 from rows r - 10 .. r, i.e. ring slots (s + 1 + k) % 11
                // two pixels at a time, in both passes: 5 x 2 double sums are 20 registers
#pragma unroll
                for (int i0 = 0; i0 < 4; i0 += 2) {
                    double mx[2], my[2], xx[2], yy[2], xy[2];
                    {
                        const int q = (s + 6) % 11;                    // the centre row
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            const float x = pm_px(xr[q], i0 + i), y = pm_px(yr[q], i0 + i);
                            mx[i] = g[5] * (double)x;
                            my[i] = g[5] * (double)y;
                            xx[i] = g[5] * (double)(x * x);
                            yy[i] = g[5] * (double)(y * y);
                            xy[i] = g[5] * (double)(x * y);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < 5; ++k) {
                        const int qa = (s + 1 + k) % 11, qb = (s + 11 - k) % 11;   // the rows r - 10 + k and r - k share the tap g[k]
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            const float xa = pm_px(xr[qa], i0 + i), ya = pm_px(yr[qa], i0 + i);
                            const float xb = pm_px(xr[qb], i0 + i), yb = pm_px(yr[qb], i0 + i);
                            mx[i] = fma(g[k], (double)(xa + xb), mx[i]);
                            my[i] = fma(g[k], (double)(ya + yb), my[i]);
                            xx[i] = fma(g[k], (double)fmaf(xa, xa, xb * xb), xx[i]);
                            yy[i] = fma(g[k], (double)fmaf(ya, ya, yb * yb), yy[i]);
                            xy[i] = fma(g[k], (double)fmaf(xa, ya, xb * yb), xy[i]);
                        }
                    }
                    if (lds_col[i0]) {                                 // 16-B stores; a column past the strip's end is written too:
                        double* o = lds + e0 + i0 + 8;                 // it is 0 (pm_load4), like the margin it lies in
                        *reinterpret_cast<double2*>(o) = make_double2(mx[0], mx[1]);
                        *reinterpret_cast<double2*>(o + PM_P) = make_double2(my[0], my[1]);
                        *reinterpret_cast<double2*>(o + 2 * PM_P) = make_double2(xx[0], xx[1]);
                        *reinterpret_cast<double2*>(o + 3 * PM_P) = make_double2(yy[0], yy[1]);
                        *reinterpret_cast<double2*>(o + 4 * PM_P) = make_double2(xy[0], xy[1]);
                    }
                }
                __syncthreads();
                if (hact) {
#pragma unroll
                    for (int i0 = 0; i0 < 4; i0 += 2) {
                        double h[5][2];
#pragma unroll
                        for (int p = 0; p < 5; ++p) {
                            double w[12];                              // columns e0 + i0 - 5 .. e0 + i0 + 6 at LDS slots e0 + i0 + 3 ..
#pragma unroll
                            for (int v = 0; v < 12; ++v) w[v] = hrow[p * PM_P + i0 + 3 + v];
#pragma unroll
                            for (int i = 0; i < 2; ++i) {              // column e0 + i0 + i: its taps at w[i .. i + 10]
                                double acc = g[5] * w[i + 5];
#pragma unroll
                                for (int k = 0; k < 5; ++k) acc = fma(g[k], w[i + k] + w[i + 10 - k], acc);
                                h[p][i] = acc;
                            }
                        }
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            const double ux = h[0][i], uy = h[1][i];
                            const double vx = h[2][i] - ux * ux, vy = h[3][i] - uy * uy, vxy = h[4][i] - ux * uy;
                            const float num = (float)((2.0 * ux * uy + C1) * (2.0 * vxy + C2));
                            const float den = (float)((ux * ux + uy * uy + C1) * (vx + vy + C2));
                            ss += ss_col[i0 + i] ? num / den : 0.f;
                        }
                    }
                }
                __syncthreads();                                       // the LDS row is rewritten by the next output row
            }
        }
        // deterministic workgroup reduction: wave butterflies, then the waves in order
        const unsigned long long se64 = pm_wave_sum((unsigned long long)se);
        ss = wave_sum(ss);
        const int wave = tid >> 6, nw = (blockDim.x + 63) >> 6;
        if ((tid & 63) == 0) { red_se[wave] = se64; red_ss[wave] = ss; }
        __syncthreads();
        if (tid == 0) {
            unsigned long long t0 = 0ull;
            float t1 = 0.f;
            for (int w = 0; w < nw; ++w) { t0 += red_se[w]; t1 += red_ss[w]; }
            PmYPart o;
            o.se = t0; o.ss = t1; o.unused = 0.f;
            part[((long)f * d.strips + strip) * d.bands + band] = o;
        }
        __syncthreads();                                               // red is rewritten by the next frame
    }
}

// blockIdx.x = plane (0 = U, 1 = V) x chunks + chunk, blockIdx.y = frame (grid-stride); part (n, 2, chunks)
__global__ __launch_bounds__(PM_THREADS) void plane_metrics_c_kernel(const uint8_t* __restrict__ au, const uint8_t* __restrict__ av,
                                                                     const uint8_t* __restrict__ bu, const uint8_t* __restrict__ bv,
                                                                     long acs, long bcs, unsigned long long* __restrict__ part, int n,
                                                                     long plane, int chunks)
{
    __shared__ unsigned long long red[PM_THREADS / 64];
    const int tid = threadIdx.x;
    const int pl = blockIdx.x / chunks, chunk = blockIdx.x - pl * chunks;
    const uint8_t* pa = pl ? av : au;
    const uint8_t* pb = pl ? bv : bu;
    const long o0 = (long)chunk * PM_CCHUNK, o1 = o0 + PM_CCHUNK < plane ? o0 + PM_CCHUNK : plane;
    const bool all[4] = {true, true, true, true};
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint8_t* fa = pa + (long)f * acs;
        const uint8_t* fb = pb + (long)f * bcs;
        uint32_t se = 0u;                                              // at most PM_CCHUNK / PM_THREADS = 64 samples
        for (long o = o0 + 4 * tid; o < o1; o += 4 * PM_THREADS) {
            const int nb = o1 - o < 4 ? (int)(o1 - o) : 4;
            se += pm_se4(pm_load4(fa + o, nb), pm_load4(fb + o, nb), all);
        }
        const unsigned long long s = pm_wave_sum((unsigned long long)se);
        if ((tid & 63) == 0) red[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) part[((long)f * 2 + pl) * chunks + chunk] = ((red[0] + red[1]) + red[2]) + red[3];
        __syncthreads();
    }
}

// one wave per frame: lane l takes the partials l, l + 64, ... in ascending order, then the butterfly
__global__ __launch_bounds__(PM_THREADS) void plane_metrics_fold_kernel(const PmYPart* __restrict__ ypart,
                                                                        const unsigned long long* __restrict__ cpart,
                                                                        long long* __restrict__ sse, float* __restrict__ ssim_y, int n, int nsb,
                                                                        int chunks, double nv)
{
    const long f = (long)blockIdx.x * (PM_THREADS / 64) + (threadIdx.x >> 6);
    if (f >= n) return;                                                // whole waves leave together
    const int lane = threadIdx.x & 63;
    unsigned long long se = 0ull, su = 0ull, sv = 0ull;
    float ss = 0.f;
    for (int i = lane; i < nsb; i += 64) {
        const PmYPart p = ypart[f * nsb + i];
        se += p.se;
        ss += p.ss;
    }
    for (int i = lane; i < chunks; i += 64) {
        su += cpart[(f * 2) * chunks + i];
        sv += cpart[(f * 2 + 1) * chunks + i];
    }
    se = pm_wave_sum(se);
    su = pm_wave_sum(su);
    sv = pm_wave_sum(sv);
    ss = wave_sum(ss);
    if (lane == 0) {
        sse[f * 3] = (long long)se;
        sse[f * 3 + 1] = (long long)su;
        sse[f * 3 + 2] = (long long)sv;
        ssim_y[f] = (float)((double)ss / nv);
    }
}

bool pm_dims(int n, int H, int W, int chroma, PmDims& d, int& threads, long& cplane, int& chunks)
{
    if (n < 1 || H < PM_MIN_SIDE || W < PM_MIN_SIDE || H > PM_MAX_SIDE || W > PM_MAX_SIDE || chroma < CH_420 || chroma > CH_MONO) return false;
    d.n = n; d.H = H; d.W = W;
    d.strips = (W - 10 + PM_STRIP - 1) / PM_STRIP;
    d.SW = ((W - 10 + d.strips - 1) / d.strips + 3) / 4 * 4;           // the strips share the columns evenly; <= PM_STRIP, a multiple of 4
    d.strips = (W - 10 + d.SW - 1) / d.SW;
    ssim_bands(H, (long)n * d.strips, PM_TARGET_WGS, PM_MIN_BAND, d.R, d.bands);
    ssim_taps(d.g);
    const int wmax = min(d.SW + 10, W);
    threads = ((wmax + 3) / 4 + 63) / 64 * 64;
    cplane = chroma == CH_420 ? (long)((H + 1) / 2) * ((W + 1) / 2) : chroma == CH_444 ? (long)H * W : 0;
    chunks = (int)((cplane + PM_CCHUNK - 1) / PM_CCHUNK);
    return threads <= PM_THREADS;
}

}  // namespace

extern "C" int vvae_plane_metrics_supported(int H, int W, int chroma)
{
    PmDims d; int threads, chunks; long cplane;
    return pm_dims(1, H, W, chroma, d, threads, cplane, chunks) ? 1 : 0;
}

// bytes of the workspace: the Y partials (n, strips, bands) of 16 bytes, then the chroma partials (n, 2, chunks) of 8; 0 for a shape
// the kernels do not take
extern "C" size_t vvae_plane_metrics_ws_bytes(int n, int H, int W, int chroma)
{
    PmDims d; int threads, chunks; long cplane;
    if (!pm_dims(n, H, W, chroma, d, threads, cplane, chunks)) return 0;
    return (size_t)n * d.strips * d.bands * sizeof(PmYPart) + (size_t)n * 2 * chunks * sizeof(unsigned long long);
}

// Planes of the reference (a) and the test (b): y (n, H, W), u and v (n, CH, CW) uint8, rows dense inside a frame, frame f of a plane at
// base + f stride bytes (any alignment; u and v of an operand share a stride; not read for mono) -> sse int64 (n, 3): the sums of
// (a - b)^2 over the Y, U and V planes (0 for the chroma of mono); ssim_y fp32 (n).  ws: vvae_plane_metrics_ws_bytes bytes, 8-byte aligned.
extern "C" int vvae_plane_metrics_u8(const uint8_t* ay, const uint8_t* au, const uint8_t* av, long a_y_stride, long a_c_stride,
                                     const uint8_t* by, const uint8_t* bu, const uint8_t* bv, long b_y_stride, long b_c_stride,
                                     long long* sse, float* ssim_y, void* ws, int n, int H, int W, int chroma, void* stream)
{
    PmDims d; int threads, chunks; long cplane;
    if (!ay || !by || !sse || !ssim_y || !ws || !pm_dims(n, H, W, chroma, d, threads, cplane, chunks) ||
        (chroma != CH_MONO && (!au || !av || !bu || !bv)) || a_y_stride < 0 || a_c_stride < 0 || b_y_stride < 0 || b_c_stride < 0 ||
        (uintptr_t)sse % 8 || (uintptr_t)ssim_y % 4 || (uintptr_t)ws % 8)
        return VVAE_ERR_BAD_ARG;
    d.ays = a_y_stride; d.bys = b_y_stride;
    hipStream_t s = (hipStream_t)stream;
    PmYPart* ypart = (PmYPart*)ws;
    unsigned long long* cpart = (unsigned long long*)(ypart + (size_t)n * d.strips * d.bands);
    const unsigned gy = (unsigned)(n < PM_MAX_GRID_Y ? n : PM_MAX_GRID_Y);
    hipLaunchKernelGGL(plane_metrics_y_kernel, dim3((unsigned)(d.strips * d.bands), gy), dim3(threads), 0, s, ay, by, ypart, d);
    VVAE_LAUNCH_CHECK();
    if (chunks > 0) {
        hipLaunchKernelGGL(plane_metrics_c_kernel, dim3((unsigned)(2 * chunks), gy), dim3(PM_THREADS), 0, s, au, av, bu, bv, a_c_stride,
                           b_c_stride, cpart, n, cplane, chunks);
        VVAE_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(plane_metrics_fold_kernel, dim3((unsigned)ceil_div(n, PM_THREADS / 64)), dim3(PM_THREADS), 0, s, ypart, cpart, sse,
                       ssim_y, n, d.strips * d.bands, chunks, (double)(H - 10) * (W - 10));
    VVAE_LAUNCH_CHECK();
    return 0;
}
