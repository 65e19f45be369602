// Reconstruction metrics per frame: MSE, PSNR and SSIM (Wang et al. 2004) of x (the clip) against y (its reconstruction), both
// channels-last (B, T, H, W, C) fp32 or bf16 with independent dtypes, converted to fp32 and (clamp) clamped to [0, 1].
//
//   mse[f]  = mean over H W C of (x - y)^2;  psnr[f] = 10 log10(1 / max(mse, 1e-10))
//   ssim[f] = mean over the valid region (rows and columns 5 .. n - 6) and the channels of
//             S = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sx + sy + C2)),  C1 = 0.01^2, C2 = 0.03^2,
//             m = g * x, sx = g * x^2 - mx^2, sxy = g * (x y) - mx my, g the normalised 11-tap Gaussian (sigma 1.5) applied separably
//   masked frames (mask == 0): 0 everywhere, the frame is never read.
//
// metrics_fwd_kernel: one workgroup per (band of rows, frame, strip of columns).  Strip s owns the SSIM columns
// [c0, c1) = [5 + s SW, min(5 + (s + 1) SW, W - 5)) and reads the frame columns [c0 - 5, c1 + 5); its MSE columns are [c0, c1) widened
// to 0 on the first strip and to W on the last.  So the SSIM columns partition 5 .. W - 6 and the MSE columns 0 .. W - 1.  A row of at
// most 2048 values that 512 threads cover is one strip (SW = W: every shape vvae_recon_metrics_* takes); wider rows, up to W = 8192
// (vvae_recon_metrics_wide_*), are cut into strips that fit both, halo included (rm_plan).  One plan, one launch path and one kernel
// body serve both; the kernel keeps the compile-time flag STRIP (more than one strip), because the selects that choose a strip's
// columns, though they change no bit of a one-strip call, were measured to cost it 1.5 % (the VALU bounds this kernel).
// Each thread owns 4 consecutive elements of the strip's flat row of values (one 16-B fp32 / 8-B bf16 load per operand and row where
// the rows are aligned and all 4 lie in the strip) and marches down the band with the last 11 rows of x and y in a register ring (the
// loop is unrolled by 11, so every ring slot is a compile-time register).  Per output row it forms the vertically filtered mx, my,
// x^2, y^2, xy and writes them channel-planar to LDS; after a barrier a thread per (channel, 4 columns) runs the horizontal 11 taps
// from 5 aligned 16-B LDS reads per quantity and sums S over its valid columns.  The squared error of each of the band's own rows is
// summed in the same pass; the 5 halo rows above and below a band are re-read (from cache).
// Reductions are deterministic: per-thread sums, a wave butterfly, a fixed-order sum over the waves, one partial pair per
// (frame, strip, band); metrics_fold_kernel sums a frame's strips and bands in that order.  No atomics, no memset.
//
// MS-SSIM (Wang, Simoncelli, Bovik 2003; vvae_ms_ssim_*, the definition is metrics.py's): M <= 5 levels, level j + 1 the 2 x 2 means of
// level j (an odd trailing row or column dropped), both operands kept as fp32 pyramid levels in the caller's workspace.
//   metrics_fwd_kernel with MS = true: no squared error; per position CS = (2 sxy + C2) / (sx + sy + C2) and
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
//
// SSIM loss (vvae_ssim_loss_*, the definition is metrics.ssim_grad_reference): ssim[f] as above and its gradient with respect to y, for
// the one-strip shapes; frame (b, t) of y is compared with frame (b / video_div, t) of x.
//   metrics_fwd_kernel with LOSS = true: the single-scale one-strip pass, the same plan and fold, so ssim[f] has recon_metrics' bits; the
//     horizontal-pass thread also stores, for its channel and 4 columns, A = dS/dmy, Bm = dS/d(g * y^2), Cm = dS/d(g * x y) (zeros at
//     the columns outside 5 .. W - 6 of a group it owns) as three 16-B stores into the caller's workspace: per frame, map and channel
//     H - 10 rows of Wp = W rounded up to 4 floats, column j of the frame at j.  Column groups wholly outside the valid columns are
//     neither written nor read.  The instantiations without LOSS compile to the instructions they had before the flag existed.
//   ssim_bwd_kernel: dy(q) = gout[f] / (C (H - 10)(W - 10)) [ (G^T A)(q) + 2 y(q) (G^T Bm)(q) + x(q) (G^T Cm)(q) ] in gather form, the
//     forward's bands: every element of dy written exactly once (zeros on masked frames, where gout[f] == 0, and under clamp where y lies
//     strictly outside [0, 1]), no atomics, no memset, a fixed summation order.
#include "ssim_window.hpp"

namespace {

constexpr int RM_MAX_THREADS = 512;
constexpr int RM_MAX_ROW = 2048;             // values of a strip's row, halo included: 4 elements per thread
constexpr int RM_MIN_BAND = 16;              // rows per band at least (halo overhead 10 / band rows)
constexpr int RM_TARGET_WGS = 1024;          // bands are split until the grid has about this many workgroups
constexpr int RM_MAX_WIDE_W = 8192;          // widest frame

struct RmDims {
    int H, W, C, L, P, bands, R, clamp;      // L = W C, the row pitch
    int SW, strips;                          // SSIM columns per strip (W: one strip spans the row), number of strips
    float g[11];
};
// the training form's extras (SSIM loss): the maps (frame, {A, Bm, Cm}, channel, Hv = H - 10 rows, Wp = W rounded up to 4 floats; column j
// of the frame at j), the frames per sample and the pair doubling
struct RmMaps {
    float* maps;
    int T, video_div, Hv, Wp;
};

// a row of a strip: the wide load only where all 4 elements lie in the strip (its width need not be a multiple of 4)
template <typename T, bool VEC, bool STRIP>
__device__ __forceinline__ void rm_row(const T* __restrict__ row, int e0, int L, int clamp, float (&v)[4])
{
    if constexpr (STRIP) {
        if (VEC && e0 + 4 <= L) {
            VecIO<T, 4>::load(row + e0, v);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = clamp01(v[i], clamp);
        } else {
            load4<T, false>(row, e0, L, clamp, v);
        }
    } else {
        load4<T, VEC>(row, e0, L, clamp, v);
    }
}

// LDS: 5 planes (mx, my, x^2, y^2, xy) of C rows of P floats (column j at j + 8; the margins stay 0) | red[16]
// STRIP: more than one strip (file header); off: the one strip at column 0, without the selects that choose a strip's columns
// MS: the multi-scale form (file header): S and CS per channel, C pairs per (frame, strip, band), nothing for a masked frame
// LOSS: the training form (file header, SSIM loss): the one-strip single-scale pass that also stores the maps A, Bm, Cm of every valid
//       position to lm.maps, and reads frame (b, t) of y against frame (b / video_div, t) of x
template <typename TX, typename TY, bool VEC, bool STRIP, bool MS = false, bool LOSS = false>
__global__ __launch_bounds__(RM_MAX_THREADS) void metrics_fwd_kernel(const TX* __restrict__ x, const TY* __restrict__ y,
                                                                     const float* __restrict__ mask, float* __restrict__ part, RmDims d,
                                                                     RmMaps lm)
{
    static_assert(!LOSS || (!STRIP && !MS), "the maps are stored by the one-strip single-scale pass");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int band = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    // the strip's columns [col0, col0 + W) of the frame, a row of L values; the row pitch is d.L
    int strip = 0, col0 = 0, W = d.W, L = d.L;
    if constexpr (STRIP) {
        strip = blockIdx.z;
        col0 = strip * d.SW;
        W = min(col0 + d.SW + 10, d.W) - col0;
        L = W * d.C;
    }
    float* out = part + (((long)f * d.strips + strip) * d.bands + band) * 2 * (MS ? d.C : 1);
    if (mask[f] == 0.f) {                    // padding: never read; MS: and the fold never reads its partials
        if (!MS && tid == 0) { out[0] = 0.f; out[1] = 0.f; }
        return;
    }
    const int CP = d.C * d.P;
    float* red = lds + 5 * CP;
    for (int i = tid; i < 5 * CP; i += blockDim.x) lds[i] = 0.f;

    const auto [r0, r1, a, e, any] = ssim_rows(band, d.R, d.H);

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
    long xbase = fbase;
    if constexpr (LOSS) xbase = ((long)(f / lm.T / lm.video_div) * lm.T + f % lm.T) * d.H * d.L;
    const TX* xf = x + xbase + (long)col0 * d.C;
    const TY* yf = y + fbase + (long)col0 * d.C;
    // LOSS: the maps of channel hc, columns j0 .. j0 + 3: three planes of Hv rows of Wp floats, a plane stride apart
    [[maybe_unused]] float* mrow = nullptr;
    if constexpr (LOSS) mrow = lm.maps + ((long)f * 3 * d.C + hc) * lm.Hv * lm.Wp + j0;
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
                [[maybe_unused]] float ma[4], mb[4], mc[4];
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
                        if constexpr (LOSS) {
                            // dS/dmy, dS/d(g * y^2), dS/d(g * x y) with 1 / b2 - 1 / b1 = (b1 - b2) / (b1 b2); 0 outside the valid columns.
                            // The factors are restated here, not named above: naming them in the lines every instantiation shares
                            // took those from 163 to 203 VGPRs (occupancy 3 -> 2) for the same expression tree.
                            const float a1 = 2.f * ux * uy + C1, a2 = 2.f * vxy + C2;
                            const float b1 = ux * ux + uy * uy + C1, b2 = vx + vy + C2;
                            const bool in = j >= 5 && j <= W - 6;
                            const float sv = num / den, inv = 1.f / den;
                            ma[i] = in ? 2.f * (ux * (a2 - a1) + uy * sv * (b1 - b2)) * inv : 0.f;
                            mb[i] = in ? -(sv * b1) * inv : 0.f;
                            mc[i] = in ? 2.f * a1 * inv : 0.f;
                        }
                    }
                }
                if constexpr (LOSS) {                // output row r - 5 is row r - 10 of the valid region
                    float* o = mrow + (long)(r - 10) * lm.Wp;
                    const long ps = (long)d.C * lm.Hv * lm.Wp;
                    VecIO<float, 4>::store(o, ma);
                    VecIO<float, 4>::store(o + ps, mb);
                    VecIO<float, 4>::store(o + 2 * ps, mc);
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

// one thread per frame: the bands in order -> mse, psnr (both or neither), ssim (0 on masked frames)
__global__ void metrics_fold_kernel(const float* __restrict__ part, const float* __restrict__ mask, float* __restrict__ mse,
                                    float* __restrict__ psnr, float* __restrict__ ssim, int F, int bands, double n, double nv)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    if (mask[f] == 0.f) {
        if (mse) { mse[f] = 0.f; psnr[f] = 0.f; }
        ssim[f] = 0.f;
        return;
    }
    float se = 0.f, ss = 0.f;
    for (int b = 0; b < bands; ++b) { se += part[((long)f * bands + b) * 2]; ss += part[((long)f * bands + b) * 2 + 1]; }
    if (mse) {                                   // NULL (with psnr): the SSIM loss wants neither
        const double m = (double)se / n;
        mse[f] = (float)m;
        psnr[f] = (float)(10.0 * log10(1.0 / fmax(m, 1e-10)));
    }
    ssim[f] = (float)((double)ss / nv);
}

// the threads for rows of w columns: 4 flat elements each in the vertical pass, a (channel, 4 columns) each in the horizontal pass
int rm_threads(int w, int C)
{
    const int need = max((w * C + 3) / 4, C * ((w + 3) / 4));
    return (need + 63) / 64 * 64;
}

// The plan of a moment pass.  One strip spanning the row (SW = W) where the row fits RM_MAX_ROW values and RM_MAX_THREADS threads;
// else strips that fit both, halo included, SW C % 4 == 0 keeping every strip 16-B aligned.  The one-strip test comes first: strips of
// SW + 10 columns alone would cut rows that fit whole (C = 1, W = 2048: SW = 2036).  Bands of at least min_band rows.
bool rm_plan(int B, int T, int H, int W, int C, int min_band, RmDims& d, int& threads)
{
    if (B <= 0 || T <= 0 || H < 11 || W < 11 || W > RM_MAX_WIDE_W || C < 1 || C > 4 || (long)B * T > 65535) return false;
    int sw = W;
    if (W * C > RM_MAX_ROW || rm_threads(W, C) > RM_MAX_THREADS) {
        sw = (RM_MAX_ROW / C - 10) / 4 * 4;
        while (C * ((sw + 10 + 3) / 4) > RM_MAX_THREADS) sw -= 4;
    }
    const int wmax = min(sw + 10, W);
    d.H = H; d.W = W; d.C = C; d.L = W * C;
    d.SW = sw;
    d.strips = (W - 10 + sw - 1) / sw;
    d.P = (wmax + 3) / 4 * 4 + 16;
    d.clamp = 0;
    threads = rm_threads(wmax, C);
    ssim_bands(H, (long)B * T * d.strips, RM_TARGET_WGS, min_band, d.R, d.bands);
    double g[11];
    ssim_taps(g);
    for (int k = 0; k < 11; ++k) d.g[k] = (float)g[k];
    return true;
}

// one moment pass over F frames; the 16-B loads where every row of both operands starts on a 4-element boundary (every strip does
// then: SW C % 4 == 0)
template <typename TX, typename TY, bool MS, bool LOSS = false>
void rm_launch(RmDims d, int threads, int F, int clamp, hipStream_t s, const void* x, const void* y, const float* mask, float* part,
               RmMaps lm = RmMaps{nullptr, 1, 1, 0, 0})
{
    d.clamp = clamp ? 1 : 0;
    const bool vec = d.L % 4 == 0 && (uintptr_t)x % (4 * sizeof(TX)) == 0 && (uintptr_t)y % (4 * sizeof(TY)) == 0;
    const size_t lds = ((size_t)5 * d.C * d.P + 16) * 4;
    const dim3 grid(d.bands, F, d.strips);
#define RM_LAUNCH(VEC, STRIP, LS) \
    hipLaunchKernelGGL((metrics_fwd_kernel<TX, TY, VEC, STRIP, MS, LS>), grid, dim3(threads), lds, s, (const TX*)x, (const TY*)y, mask, part, \
                       d, lm)
    if constexpr (LOSS) { if (vec) RM_LAUNCH(true, false, true); else RM_LAUNCH(false, false, true); }      // one strip (sl_plan)
    else if (d.strips > 1) { if (vec) RM_LAUNCH(true, true, false); else RM_LAUNCH(false, true, false); }
    else { if (vec) RM_LAUNCH(true, false, false); else RM_LAUNCH(false, false, false); }
#undef RM_LAUNCH
}

// ---- SSIM loss: the plan and the backward pass (file header) ---------------------------------------------------------------------------
struct SbDims {
    int H, W, C, L, P, bands, R, clamp;      // as RmDims (the forward's plan: the same bands)
    int T, video_div, Hv, Wp;                // as RmMaps
    float inv_n;                             // 1 / (C (H - 10) (W - 10))
    float g[11];
};

// The plan of an SSIM-loss call: the moment pass's plan where it is one strip.  maps_n: floats of the three maps; total: with the forward's
// partial sums behind them.
struct SlPlan {
    RmDims d;
    int threads, Hv, Wp;
    size_t maps_n, total;
};
bool sl_plan(int B, int T, int H, int W, int C, SlPlan& p)
{
    if (!rm_plan(B, T, H, W, C, RM_MIN_BAND, p.d, p.threads) || p.d.strips != 1) return false;
    p.Hv = H - 10;
    p.Wp = (W + 3) / 4 * 4;
    p.maps_n = (size_t)B * T * 3 * C * p.Hv * p.Wp;
    p.total = p.maps_n + ((size_t)B * T * p.d.bands * 2 + 3) / 4 * 4;
    return true;
}

// 4 values to elements e0 .. e0 + 3 of a row of L: one 16-B fp32 / 8-B bf16 store (VEC: L % 4 == 0 and the rows aligned for it), or
// element by element
template <typename T, bool VEC>
__device__ __forceinline__ void store4(T* __restrict__ row, int e0, int L, const float (&v)[4])
{
    if (VEC) {
        if (e0 < L) VecIO<T, 4>::store(row + e0, v);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (e0 + i < L) stf(row + e0 + i, v[i]);
    }
}

// d ssim[f] / d y in gather form: one workgroup per (band of rows, frame) writes every element of its rows of dy exactly once.
// A thread has two roles.  Planar (channel hc, columns j0 .. j0 + 3, the forward's horizontal-pass role): it marches down the band with
// the last 11 rows of the three maps in a register ring (zeros outside the valid region, which are not read: rows outside 5 .. H - 6,
// and the column groups the forward did not write), forms the vertical 11 taps of output row r - 5 and writes them to the LDS planes;
// after a barrier it runs the horizontal 11 taps from 5 aligned 16-B LDS reads per map and parks the three results in a second set of
// planes.  Flat (elements e0 .. e0 + 3 of the row, the forward's vertical-pass role): after a second barrier it reads its elements'
// three results, combines them with x and y (loaded before the barriers) and stores the row's 4 elements.  Two barriers per row: the
// vertical planes are rewritten after the second one, the parked results after the next row's first.
// LDS: 3 vertical planes | 3 result planes, each C rows of P floats (column j at j + 8; the margins stay 0)
template <typename TX, typename TY, bool VEC>
__global__ __launch_bounds__(RM_MAX_THREADS) void ssim_bwd_kernel(const TX* __restrict__ x, const TY* __restrict__ y,
                                                                  const float* __restrict__ mask, const float* __restrict__ gout,
                                                                  const float* __restrict__ maps, TY* __restrict__ dy, SbDims d)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int band = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const int W = d.W, L = d.L, CP = d.C * d.P;
    const int r0 = band * d.R, r1 = min(r0 + d.R, d.H);
    const int e0 = tid * 4;
    TY* dyf = dy + (long)f * d.H * L;
    const float gf = mask[f] == 0.f ? 0.f : gout[f];
    if (gf == 0.f) {                         // padding, or an upstream gradient of 0: zeros, nothing read
        const float z[4] = {0.f, 0.f, 0.f, 0.f};
        for (int r = r0; r < r1; ++r) store4<TY, VEC>(dyf + (long)r * L, e0, L, z);
        return;
    }
    const float scale = gf * d.inv_n;
    for (int i = tid; i < 6 * CP; i += blockDim.x) lds[i] = 0.f;

    // planar role
    const int ng = (W + 3) / 4, hc = tid / ng, j0 = (tid - hc * ng) * 4;
    const bool pact = hc < d.C;
    const bool vact = pact && j0 + 3 >= 5 && j0 <= W - 6;        // the column groups the forward wrote
    const long ps = (long)d.C * d.Hv * d.Wp;
    const float* mf = maps + ((long)f * 3 * d.C + hc) * d.Hv * d.Wp + j0;
    float* vrow = lds + hc * d.P + j0;
    // flat role: the LDS slots of its elements' results
    int hofs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int el = e0 + i, j = el / d.C;
        hofs[i] = el < L ? 3 * CP + (el - j * d.C) * d.P + j + 8 : 3 * CP;
    }
    const long xbase = ((long)(f / d.T / d.video_div) * d.T + f % d.T) * d.H * L;
    const TX* xf = x + xbase;
    const TY* yf = y + (long)f * d.H * L;
    float g[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) g[k] = d.g[k];

    // row r of the maps in frame coordinates: zeros outside the valid rows and for a group the forward did not write
    auto map_row = [&](int r, float (&m)[3][4]) {
        if (vact && r >= 5 && r < d.H - 5) {
#pragma unroll
            for (int p = 0; p < 3; ++p) VecIO<float, 4>::load(mf + p * ps + (long)(r - 5) * d.Wp, m[p]);
        } else {
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int i = 0; i < 4; ++i) m[p][i] = 0.f;
        }
    };

    const int a = r0 - 5, e = r1 + 5;        // output row r - 5 from the map rows r - 10 .. r
    float mr[11][3][4], nm[3][4];
    map_row(a, nm);
    __syncthreads();                         // LDS zeroed

    for (int base = a; base < e; base += 11) {
#pragma unroll
        for (int s = 0; s < 11; ++s) {
            const int r = base + s;
            if (r >= e) break;
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int i = 0; i < 4; ++i) mr[s][p][i] = nm[p][i];
            if (r + 1 < e) map_row(r + 1, nm);
            if (r < a + 10) continue;
            const long ro = (long)(r - 5) * L;
            float xv[4], yv[4];              // in flight across the two barriers
            load4<TX, VEC>(xf + ro, e0, L, 0, xv);
            load4<TY, VEC>(yf + ro, e0, L, 0, yv);
            if (vact) {
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int k = 0; k < 11; ++k) {
                        const int q = (s + 1 + k) % 11;
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[i] = fmaf(g[k], mr[q][p][i], v[i]);
                    }
                    VecIO<float, 4>::store(vrow + p * CP + 8, v);
                }
            }
            __syncthreads();
            if (pact) {
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    float w[20], h[4];
#pragma unroll
                    for (int v = 0; v < 5; ++v) {
                        const float4 t = *reinterpret_cast<const float4*>(vrow + p * CP + 4 * v);
                        w[4 * v] = t.x; w[4 * v + 1] = t.y; w[4 * v + 2] = t.z; w[4 * v + 3] = t.w;
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {    // column j0 + i: taps j0 + i - 5 .. j0 + i + 5 at w[i + 3 .. i + 13]
                        float acc = 0.f;
#pragma unroll
                        for (int k = 0; k < 11; ++k) acc = fmaf(g[k], w[i + 3 + k], acc);
                        h[i] = acc;
                    }
                    VecIO<float, 4>::store(vrow + (3 + p) * CP + 8, h);
                }
            }
            __syncthreads();
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float ha = lds[hofs[i]], hb = lds[hofs[i] + CP], hm = lds[hofs[i] + 2 * CP];
                const float xc = clamp01(xv[i], d.clamp), yc = clamp01(yv[i], d.clamp);
                const float t = scale * (ha + 2.f * yc * hb + xc * hm);
                // clamp: no gradient where y lies strictly outside [0, 1]
                o[i] = (d.clamp && (yv[i] < 0.f || yv[i] > 1.f)) ? 0.f : t;
            }
            store4<TY, VEC>(dyf + ro, e0, L, o);
        }
    }
}

// ---- MS-SSIM: the pyramid, the fold over levels, the plan of a call (file header) -------------------------------------------------
constexpr int MS_MAX_SCALES = 5;
constexpr int MS_MIN_BAND = 4;               // rows per band at least: the small levels leave the chip idle, and a workgroup's time is its
                                             // rows + 10 halo rows at about a microsecond each, so shorter bands finish sooner

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
        for (int i = 0; i < N; ++i) v[q * N + i] = clamp01(t[i], clamp);
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
    const float v00 = clamp01(ldf(v), clamp), v01 = clamp01(ldf(v + C), clamp);
    const float v10 = clamp01(ldf(v + L), clamp), v11 = clamp01(ldf(v + L + C), clamp);
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
    RmDims d;                                // the moment pass of the level
    int threads, H, W;
    size_t pyr, pyr_n;                     // levels >= 1: x at ws + pyr, y at ws + pyr + pyr_n (pyr_n a multiple of 4)
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
        if (!rm_plan(B, T, l.H, l.W, C, MS_MIN_BAND, l.d, l.threads)) return false;
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
    rm_launch<TX, TY, true>(l.d, l.threads, F, clamp, s, x, y, mask, part);
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

extern "C" int vvae_recon_metrics_wide_supported(int H, int W, int C, int x_dtype, int y_dtype)
{
    RmDims d; int threads;
    return dtype_pair_ok(x_dtype, y_dtype) && rm_plan(1, 1, H, W, C, RM_MIN_BAND, d, threads);
}

extern "C" size_t vvae_recon_metrics_wide_part_floats(int B, int T, int H, int W, int C)
{
    RmDims d; int threads;
    if (!rm_plan(B, T, H, W, C, RM_MIN_BAND, d, threads)) return 0;
    return (size_t)B * T * d.strips * d.bands * 2;
}

// x, y (B, T, H, W, C) contiguous, 11 <= W <= 8192, dtypes VVAE_DT_F32 / VVAE_DT_BF16 each; mask fp32 (B T), nonzero = valid frame;
// part: scratch of vvae_recon_metrics_wide_part_floats floats (every word written before it is read) -> mse, psnr, ssim fp32 (B T).
// clamp: clamp to [0, 1].
extern "C" int vvae_recon_metrics_wide_fwd(const void* x, int x_dtype, const void* y, int y_dtype, const float* mask, float* mse, float* psnr,
                                           float* ssim, float* part, int B, int T, int H, int W, int C, int clamp, void* stream)
{
    RmDims d; int threads;
    if (!x || !y || !mask || !mse || !psnr || !ssim || !part || !dtype_pair_ok(x_dtype, y_dtype) ||
        !rm_plan(B, T, H, W, C, RM_MIN_BAND, d, threads))
        return VVAE_ERR_BAD_ARG;
    const int ex = x_dtype == VVAE_DT_F32 ? 4 : 2, ey = y_dtype == VVAE_DT_F32 ? 4 : 2;
    if ((uintptr_t)x % ex || (uintptr_t)y % ey || ((uintptr_t)mask | (uintptr_t)mse | (uintptr_t)psnr | (uintptr_t)ssim | (uintptr_t)part) % 4)
        return VVAE_ERR_BAD_ARG;
    const int F = B * T;
    hipStream_t s = (hipStream_t)stream;
    dispatch_dtype_pair(x_dtype, y_dtype, [&](auto tx, auto ty) {
        rm_launch<typename decltype(tx)::type, typename decltype(ty)::type, false>(d, threads, F, clamp, s, x, y, mask, part);
    });
    VVAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(metrics_fold_kernel, dim3((F + 255) / 256), dim3(256), 0, s, part, mask, mse, psnr, ssim, F, d.strips * d.bands,
                       (double)H * W * C, (double)(H - 10) * (W - 10) * C);
    VVAE_LAUNCH_CHECK();
    return 0;
}

// The entries for rows of one strip (W C <= 2048 and at most 512 threads): the wide entries on the shapes they plan one strip for.
extern "C" int vvae_recon_metrics_supported(int H, int W, int C, int x_dtype, int y_dtype)
{
    RmDims d; int threads;
    return dtype_pair_ok(x_dtype, y_dtype) && rm_plan(1, 1, H, W, C, RM_MIN_BAND, d, threads) && d.strips == 1;
}

extern "C" size_t vvae_recon_metrics_part_floats(int B, int T, int H, int W, int C)
{
    return vvae_recon_metrics_supported(H, W, C, VVAE_DT_F32, VVAE_DT_F32) ? vvae_recon_metrics_wide_part_floats(B, T, H, W, C) : 0;
}

extern "C" int vvae_recon_metrics_fwd(const void* x, int x_dtype, const void* y, int y_dtype, const float* mask, float* mse, float* psnr,
                                      float* ssim, float* part, int B, int T, int H, int W, int C, int clamp, void* stream)
{
    if (!vvae_recon_metrics_supported(H, W, C, x_dtype, y_dtype)) return VVAE_ERR_BAD_ARG;
    return vvae_recon_metrics_wide_fwd(x, x_dtype, y, y_dtype, mask, mse, psnr, ssim, part, B, T, H, W, C, clamp, stream);
}

extern "C" int vvae_ms_ssim_supported(int H, int W, int C, int scales, int x_dtype, int y_dtype)
{
    MsPlan p;
    return dtype_pair_ok(x_dtype, y_dtype) && ms_plan(1, 1, H, W, C, scales, p);
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
        // level 0 reads the caller's tensors, later levels the fp32 pyramid
        const float* lx = ws + l.pyr;
        const int rc = dispatch_dtype_pair(j ? VVAE_DT_F32 : x_dtype, j ? VVAE_DT_F32 : y_dtype, [&](auto tx, auto ty) {
            return ms_level_launch<typename decltype(tx)::type, typename decltype(ty)::type>(
                l, F, C, s, j ? lx : x, j ? lx + l.pyr_n : y, mask, ws + l.part, j == 0 && clamp, ox, oy);
        });
        if (rc) return rc;
    }
    hipLaunchKernelGGL(ms_fold_kernel, dim3((F + 255) / 256), dim3(256), 0, s, ws, mask, ms_ssim, terms, F, fd);
    VVAE_LAUNCH_CHECK();
    return 0;
}

// ---- SSIM loss (include/vvae_hip.h states the entries) -----------------------------------------------------------------------------
extern "C" int vvae_ssim_loss_supported(int H, int W, int C, int x_dtype, int y_dtype)
{
    SlPlan p;
    return dtype_pair_ok(x_dtype, y_dtype) && sl_plan(1, 1, H, W, C, p);
}

extern "C" size_t vvae_ssim_loss_ws_floats(int B, int T, int H, int W, int C)
{
    SlPlan p;
    return sl_plan(B, T, H, W, C, p) ? p.total : 0;
}

extern "C" int vvae_ssim_loss_band_rows(int B, int T, int H, int W, int C)
{
    SlPlan p;
    return sl_plan(B, T, H, W, C, p) ? p.d.R : 0;
}

namespace {

inline bool sl_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

// what both passes check: the plan, the pair doubling, the pointers' alignment -> 0 or VVAE_ERR_BAD_ARG
int sl_check(const void* x, int x_dtype, const void* y, int y_dtype, const float* mask, const float* ws, int B, int T, int H, int W, int C,
             int video_div, SlPlan& p)
{
    if (!x || !y || !mask || !ws || !dtype_pair_ok(x_dtype, y_dtype) || !sl_plan(B, T, H, W, C, p) || video_div < 1 || B % video_div)
        return VVAE_ERR_BAD_ARG;
    const int ex = x_dtype == VVAE_DT_F32 ? 4 : 2, ey = y_dtype == VVAE_DT_F32 ? 4 : 2;
    if ((uintptr_t)x % ex || (uintptr_t)y % ey || (uintptr_t)mask % 4 || (uintptr_t)ws % 16) return VVAE_ERR_BAD_ARG;
    return 0;
}

}  // namespace

extern "C" int vvae_ssim_loss_fwd(const void* x, int x_dtype, const void* y, int y_dtype, const float* mask, float* ssim, float* ws, int B,
                                  int T, int H, int W, int C, int video_div, int clamp, void* stream)
{
    SlPlan p;
    if (sl_check(x, x_dtype, y, y_dtype, mask, ws, B, T, H, W, C, video_div, p) || !ssim || (uintptr_t)ssim % 4) return VVAE_ERR_BAD_ARG;
    const int F = B * T;
    const int ex = x_dtype == VVAE_DT_F32 ? 4 : 2, ey = y_dtype == VVAE_DT_F32 ? 4 : 2;
    const size_t nx = (size_t)F / video_div * H * W * C * ex, ny = (size_t)F * H * W * C * ey;
    if (sl_overlap(ws, p.total * 4, x, nx) || sl_overlap(ws, p.total * 4, y, ny) || sl_overlap(ws, p.total * 4, mask, (size_t)F * 4) ||
        sl_overlap(ws, p.total * 4, ssim, (size_t)F * 4) || sl_overlap(ssim, (size_t)F * 4, x, nx) || sl_overlap(ssim, (size_t)F * 4, y, ny) ||
        sl_overlap(ssim, (size_t)F * 4, mask, (size_t)F * 4))
        return VVAE_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    float* part = ws + p.maps_n;
    const RmMaps lm{ws, T, video_div, p.Hv, p.Wp};
    dispatch_dtype_pair(x_dtype, y_dtype, [&](auto tx, auto ty) {
        rm_launch<typename decltype(tx)::type, typename decltype(ty)::type, false, true>(p.d, p.threads, F, clamp, s, x, y, mask, part, lm);
    });
    VVAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(metrics_fold_kernel, dim3((F + 255) / 256), dim3(256), 0, s, part, mask, (float*)nullptr, (float*)nullptr, ssim, F,
                       p.d.bands, (double)H * W * C, (double)(H - 10) * (W - 10) * C);
    VVAE_LAUNCH_CHECK();
    return 0;
}

extern "C" int vvae_ssim_loss_bwd(const void* x, int x_dtype, const void* y, int y_dtype, const float* mask, const float* gout,
                                  const float* ws, void* dy, int B, int T, int H, int W, int C, int video_div, int clamp, void* stream)
{
    SlPlan p;
    if (sl_check(x, x_dtype, y, y_dtype, mask, ws, B, T, H, W, C, video_div, p) || !gout || (uintptr_t)gout % 4 || !dy) return VVAE_ERR_BAD_ARG;
    const int F = B * T;
    const int ex = x_dtype == VVAE_DT_F32 ? 4 : 2, ey = y_dtype == VVAE_DT_F32 ? 4 : 2;
    if ((uintptr_t)dy % ey) return VVAE_ERR_BAD_ARG;
    const size_t nx = (size_t)F / video_div * H * W * C * ex, ny = (size_t)F * H * W * C * ey;
    // dy is written while the operands of other rows are still read: it may overlap none of them
    if (sl_overlap(dy, ny, x, nx) || sl_overlap(dy, ny, y, ny) || sl_overlap(dy, ny, ws, p.maps_n * 4) ||
        sl_overlap(dy, ny, mask, (size_t)F * 4) || sl_overlap(dy, ny, gout, (size_t)F * 4))
        return VVAE_ERR_BAD_ARG;
    SbDims d;
    d.H = H; d.W = W; d.C = C; d.L = p.d.L; d.P = p.d.P; d.bands = p.d.bands; d.R = p.d.R; d.clamp = clamp ? 1 : 0;
    d.T = T; d.video_div = video_div; d.Hv = p.Hv; d.Wp = p.Wp;
    d.inv_n = (float)(1.0 / ((double)C * (H - 10) * (W - 10)));
    for (int k = 0; k < 11; ++k) d.g[k] = p.d.g[k];
    const size_t lds = (size_t)6 * C * d.P * 4;
    const dim3 grid(d.bands, F);
    hipStream_t s = (hipStream_t)stream;
    dispatch_dtype_pair(x_dtype, y_dtype, [&](auto tx, auto ty) {
        using TX = typename decltype(tx)::type;
        using TY = typename decltype(ty)::type;
        const bool vec = d.L % 4 == 0 && (uintptr_t)x % (4 * sizeof(TX)) == 0 && (uintptr_t)y % (4 * sizeof(TY)) == 0 &&
                         (uintptr_t)dy % (4 * sizeof(TY)) == 0;
        if (vec)
            hipLaunchKernelGGL((ssim_bwd_kernel<TX, TY, true>), grid, dim3(p.threads), lds, s, (const TX*)x, (const TY*)y, mask, gout, ws,
                               (TY*)dy, d);
        else
            hipLaunchKernelGGL((ssim_bwd_kernel<TX, TY, false>), grid, dim3(p.threads), lds, s, (const TX*)x, (const TY*)y, mask, gout, ws,
                               (TY*)dy, d);
    });
    VVAE_LAUNCH_CHECK();
    return 0;
}
