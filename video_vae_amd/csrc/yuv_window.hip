// The training loader's front end on Y'CbCr planes: window -> RGB -> bilinear resize -> / 255 -> fp32 or bf16, one launch.
// video_vae_amd/y4m.py states the window and its to-RGB arithmetic (Y4MClip.window, window_to_rgb_reference), video_vae_amd/data.py the
// resize (resize_reference_u8); this file computes their composition divided by 255, bit for bit: what vvae_yuv_to_rgb_u8 on the whole
// planes, the crop, vvae_crop_resize_norm give, without the RGB intermediate.
//
// Operands.  y (n, H, W): the luma crop.  4:2:0: u, v (n, H / 2 + 3, W / 2 + 3): the crop's chroma neighbourhood, gathered with the frame's
// edge clamp by the host, so nothing is clamped here and only the crop's parities are needed; 4:4:4: u, v (n, H, W); mono: none.
// clip_params int32 (ceil(n / frames_per_clip), 4) = (top & 1, left & 1, full_range, 0): frame f reads row f / frames_per_clip.
// With (py, px) the parities, luma pixel (y, x) of the crop sits at frame-parity position Y = py + y, X = px + x; its chroma rows are
// r0 = (Y >> 1) + 1 and r0 + 1 (Y odd) or r0 - 1 (Y even), weights (3, 1); columns, centre siting: the same with X; mpeg2:
// c0 = (X >> 1) + 1, c1 = c0 + 1, weights (4, 0) for even X and (2, 2) for odd X.  U16 = sum wv wh U[r][c]; 4:4:4: 16 U; mono: 2048.  Then
// the integer matrix of yuv.hip gives the tap's bytes R, G, B.
//
// Resize (resize.hip's rule, the window as the whole frame).  The taps of an output pixel are x0, x1 = x0 + (0 | 1) and y0, y1 =
// y0 + (0 | 1): a 2 x 2 block of adjacent luma pixels, whose chroma lies in 3 rows x 3 columns of the window.  A tap whose weight is
// exactly 0 is not formed (0 * s = +0 for every byte s, and t + 0 = t): the bottom row when a1 = 0, the right column of a copy.
//
// yuv_window_kernel<CHROMA, SITING, XM, Out>: a workgroup is 4 waves; lane l of wave w owns OPX consecutive output pixels (from
// (blockIdx.x 64 + l) OPX) of the output rows blockIdx.y YW_ROWS + 2 w and + 2 w + 1; blockIdx.z = frame, grid-stride.  XM is the column
// geometry, the only thing that fixes which source columns a thread reads:
//   XM_COPY (out_w == W): OPX = 4 pixels = one span of 4 luma columns at 4 k, no right tap (8 pixels per thread left half of each wave
//     idle at 256 columns and took 176 VGPRs: 54.6 us against 26.0 us for a 4 x 16 x 256² batch);
//   XM_HALF (W == 2 out_w): OPX = 4 pixels = one span of 8 luma columns at 8 k, taps (2 i, 2 i + 1): every source pixel is converted once;
//   XM_ANY: OPX = 4 pixels, each its own span of 2 luma columns at x0 (taps repeat between neighbours and are converted again).
// A span of L luma columns at X needs the L / 2 + 2 chroma columns from (px + X) >> 1.  Per output row a thread reads the 2 luma rows
// and the (up to) 3 chroma rows of both planes over its span -- dwords from the first dword boundary inside a run of 4, 6 or 8 bytes where
// the whole run exists, bytes around them and elsewhere (window rows are odd-sized, so most chroma rows start off a dword) -- folds the
// chroma rows with the row weights (uniform over the wave), takes the column taps, converts and blends.  Matrix and range are values, not
// template axes: both ranges' coefficients of the matrix are kernel arguments and the clip's row picks one.
// Every output element is written once, by one thread; nothing outside dst is touched, no byte outside the planes read: no atomics, no
// memset, no workspace, no LDS, no cross-lane operation; bitwise reproducible; safe inside a captured hipGraph.
#include "common.hpp"

#pragma clang fp contract(off)

#include "resize_common.hpp"
#include "yuv_common.hpp"

extern "C" int vvae_yuv_window_supported(int H, int W, int chroma, int out_h, int out_w);

namespace {

constexpr int YW_LANES = 64;                 // threads across a row: one wave
constexpr int YW_WAVES = 4;
constexpr int YW_WROWS = 2;                  // output rows per wave
constexpr int YW_ROWS = YW_WAVES * YW_WROWS; // output rows per workgroup
constexpr int YW_MAX_SIDE = 16384;
constexpr int YW_MAX_GRID_Z = 65535;

enum { XM_ANY = 0, XM_COPY = 1, XM_HALF = 2 };

constexpr int YW_OPX = 4;                   // output pixels of a row per thread

struct WinDims {
    int H, W, CH, CW, out_h, out_w, frames_per_clip;
    float sy, sx;                            // float(H) / float(out_h), float(W) / float(out_w)
    YuvInv k[2];                             // the matrix in its limited and its full range
};

// o[i] = p[min(i, nv - 1)], i < N (nv >= 1): dword loads from the first dword boundary inside the run where all N bytes exist
template <int N>
__device__ __forceinline__ void load_run(const uint8_t* p, int nv, int (&o)[N])
{
    const int s = (int)((0u - (unsigned)(uintptr_t)p) & 3u);      // bytes before the boundary
    bool wide = false;
#pragma unroll
    for (int ss = 0; ss < 4 && ss + 4 <= N; ++ss) {
        if (s == ss && nv >= N) {
            wide = true;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                if (i >= ss && (i - ss) % 4 == 0 && i + 4 <= N) {
                    const uint32_t w = *reinterpret_cast<const uint32_t*>(p + i);
#pragma unroll
                    for (int b = 0; b < 4; ++b) o[i + b] = (int)((w >> (8 * b)) & 255u);
                } else if (i < ss || i >= ss + ((N - ss) / 4) * 4) {
                    o[i] = (int)p[i];
                }
            }
        }
    }
    if (!wide) {
#pragma unroll
        for (int i = 0; i < N; ++i) o[i] = (int)p[min(i, nv - 1)];
    }
}

// The chroma, at 4 extra bits, of luma column par + i (i static, par 0 | 1) of a span whose row-folded chroma columns are t[]
template <int SITING, int NC>
__device__ __forceinline__ int chroma_tap(const int (&t)[NC], int i, int par)
{
    int r[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int X = i + q, a = (X >> 1) + 1;                      // X <= L = 2 NC - 4: a <= NC - 1, and a <= NC - 2 when X is odd
        if (SITING == SITE_CENTRE) r[q] = 3 * t[a] + t[(X & 1) ? a + 1 : a - 1];
        else r[q] = (X & 1) ? 2 * t[a] + 2 * t[a + 1] : 4 * t[a];
    }
    return par ? r[1] : r[0];
}

// One luma row of one span: L luma columns at X of luma row `row`, the chroma rows cu, cv[3][NC] with the row's weights wr[3]
// -> S[i][c], the bytes R, G, B of the L pixels as fp32
template <int CHROMA, int SITING, int L>
__device__ __forceinline__ void convert_row(const uint8_t* fy, const uint8_t* fu, const uint8_t* fv, const WinDims& d, const YuvInv& k,
                                            int row, int X, int par, const int (&cu)[3][L / 2 + 2], const int (&cv)[3][L / 2 + 2],
                                            const int (&wr)[3], float (&S)[L][3])
{
    constexpr int NC = L / 2 + 2;
    int Y[L], U16[L], V16[L];
    const long o = (long)row * d.W + X;
    load_run<L>(fy + o, d.W - X, Y);
    if (CHROMA == CH_420) {
        int tu[NC], tv[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            tu[c] = wr[0] * cu[0][c] + wr[1] * cu[1][c] + wr[2] * cu[2][c];
            tv[c] = wr[0] * cv[0][c] + wr[1] * cv[1][c] + wr[2] * cv[2][c];
        }
#pragma unroll
        for (int i = 0; i < L; ++i) {
            U16[i] = chroma_tap<SITING, NC>(tu, i, par);
            V16[i] = chroma_tap<SITING, NC>(tv, i, par);
        }
    } else if (CHROMA == CH_444) {
        load_run<L>(fu + o, d.W - X, U16);
        load_run<L>(fv + o, d.W - X, V16);
#pragma unroll
        for (int i = 0; i < L; ++i) {
            U16[i] *= 16;
            V16[i] *= 16;
        }
    } else {
#pragma unroll
        for (int i = 0; i < L; ++i) U16[i] = V16[i] = 2048;
    }
#pragma unroll
    for (int i = 0; i < L; ++i) {
        const int l = 16 * k.cy * (Y[i] - k.off), u = U16[i] - 2048, v = V16[i] - 2048;
        S[i][0] = (float)clip255((l + k.crv * v + (1 << 17)) >> 18);
        S[i][1] = (float)clip255((l + k.cgu * u + k.cgv * v + (1 << 17)) >> 18);
        S[i][2] = (float)clip255((l + k.cbu * u + (1 << 17)) >> 18);
    }
}

template <int CHROMA, int SITING, int XM, typename Out>
__global__ __launch_bounds__(YW_LANES * YW_WAVES) void yuv_window_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ up,
                                                                        const uint8_t* __restrict__ vp, const int* __restrict__ params,
                                                                        typename Out::T* __restrict__ dst, int n, WinDims d)
{
    constexpr int OPX = YW_OPX;
    constexpr int L = XM == XM_ANY ? 2 : XM == XM_COPY ? 4 : 8;    // luma columns of a span
    constexpr int NS = XM == XM_ANY ? OPX : 1;                     // spans per thread
    constexpr int NC = L / 2 + 2;
    const int lane = threadIdx.x & (YW_LANES - 1), wave = threadIdx.x / YW_LANES;
    const int j0 = (blockIdx.x * YW_LANES + lane) * OPX;
    if (j0 >= d.out_w) return;
    const int nbp = min(OPX, d.out_w - j0);                        // output pixels of the row this thread owns
    int sx0[NS], dx[OPX];
    float b0[OPX], b1[OPX];
#pragma unroll
    for (int i = 0; i < OPX; ++i) {
        int x0, x1;
        rz_axis(min(j0 + i, d.out_w - 1), d.sx, d.W, x0, x1, b0[i], b1[i]);
        dx[i] = x1 - x0;
        if (XM == XM_ANY) sx0[i] = x0;
    }
    if (XM == XM_COPY) sx0[0] = j0;
    if (XM == XM_HALF) sx0[0] = 2 * j0;
    const int r_lo = blockIdx.y * YW_ROWS + wave * YW_WROWS, r_hi = min(r_lo + YW_WROWS, d.out_h);
    const long lplane = (long)d.H * d.W, cplane = (long)d.CH * d.CW;
    const int Lrow = d.out_w * 3;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const int* cp = params + 4 * (f / d.frames_per_clip);
        const int py = cp[0] & 1, px = cp[1] & 1;
        const YuvInv k = cp[2] ? d.k[1] : d.k[0];
        const uint8_t* fy = yp + (long)f * lplane;
        const uint8_t* fu = up + (long)f * cplane;
        const uint8_t* fv = vp + (long)f * cplane;
        typename Out::T* fdst = dst + (long)f * d.out_h * Lrow;
        for (int y = r_lo; y < r_hi; ++y) {
            int y0, y1;
            float a0, a1;
            rz_axis(y, d.sy, d.H, y0, y1, a0, a1);
            const bool two = a1 != 0.f;                            // is the bottom row blended in at all?
            const int RB = (py + y0) >> 1;                         // the first of the (up to) 3 chroma rows of the two luma rows
            int wr[2][3];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int Y = py + (t ? y1 : y0), ra = (Y >> 1) + 1 - RB, rb = (Y & 1) ? ra + 1 : ra - 1;
#pragma unroll
                for (int r = 0; r < 3; ++r) wr[t][r] = (r == ra ? 3 : 0) + (r == rb ? 1 : 0);
            }
            float top[OPX][3], bot[OPX][3];
#pragma unroll
            for (int sp = 0; sp < NS; ++sp) {
                const int X = sx0[sp], par = (px + X) & 1, CBX = (px + X) >> 1;
                int cu[3][NC], cv[3][NC];
                if (CHROMA == CH_420) {
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        if (wr[0][r] != 0 || (two && wr[1][r] != 0)) {
                            const long o = (long)min(RB + r, d.CH - 1) * d.CW + CBX;
                            load_run<NC>(fu + o, d.CW - CBX, cu[r]);
                            load_run<NC>(fv + o, d.CW - CBX, cv[r]);
                        } else {
#pragma unroll
                            for (int c = 0; c < NC; ++c) cu[r][c] = cv[r][c] = 0;
                        }
                    }
                }
                float S[2][L][3];
                convert_row<CHROMA, SITING, L>(fy, fu, fv, d, k, y0, X, par, cu, cv, wr[0], S[0]);
                if (two) convert_row<CHROMA, SITING, L>(fy, fu, fv, d, k, y1, X, par, cu, cv, wr[1], S[1]);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    if (t == 1 && !two) break;
#pragma unroll
                    for (int i = 0; i < (XM == XM_ANY ? 1 : OPX); ++i) {
                        const int op = XM == XM_ANY ? sp : i;     // the output pixel
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            float s0, s1;
                            if (XM == XM_COPY) s0 = s1 = S[t][i][c];
                            else if (XM == XM_HALF) s0 = S[t][2 * i][c], s1 = S[t][2 * i + 1][c];
                            else s0 = S[t][0][c], s1 = dx[op] ? S[t][1][c] : S[t][0][c];
                            const float h = (b0[op] * s0) + (b1[op] * s1);
                            if (t == 0) top[op][c] = h;
                            else bot[op][c] = h;
                        }
                    }
                }
            }
            typename Out::T* o = fdst + (long)y * Lrow + (long)j0 * 3;
#pragma unroll
            for (int g = 0; g < OPX * 3 / 4; ++g) {
                float q[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int el = 4 * g + e, op = el / 3, c = el % 3;
                    const float v = (a0 * top[op][c]) + (a1 * (two ? bot[op][c] : top[op][c]));
                    q[e] = fminf(fmaxf(rintf(v), 0.f), 255.f);
                }
                Out::store(o + 4 * g, q, nbp * 3 - 4 * g);
            }
        }
    }
}

int window_xm(int W, int out_w) { return out_w == W ? XM_COPY : W == 2 * out_w ? XM_HALF : XM_ANY; }

template <int CHROMA, int SITING, typename Out>
void launch_xm(int xm, dim3 grid, hipStream_t s, const uint8_t* y, const uint8_t* u, const uint8_t* v, const int* params,
               typename Out::T* dst, int n, const WinDims& d)
{
    const dim3 block(YW_LANES * YW_WAVES);
    if (xm == XM_COPY) hipLaunchKernelGGL((yuv_window_kernel<CHROMA, SITING, XM_COPY, Out>), grid, block, 0, s, y, u, v, params, dst, n, d);
    else if (xm == XM_HALF) hipLaunchKernelGGL((yuv_window_kernel<CHROMA, SITING, XM_HALF, Out>), grid, block, 0, s, y, u, v, params, dst, n, d);
    else hipLaunchKernelGGL((yuv_window_kernel<CHROMA, SITING, XM_ANY, Out>), grid, block, 0, s, y, u, v, params, dst, n, d);
}

template <typename Out>
int launch_window(const uint8_t* y, const uint8_t* u, const uint8_t* v, const int* params, typename Out::T* dst, int n, int frames_per_clip,
                  int H, int W, int chroma, int siting, int matrix, int out_h, int out_w, void* stream)
{
    if (!y || !params || !dst || n < 1 || frames_per_clip < 1 || !vvae_yuv_window_supported(H, W, chroma, out_h, out_w) ||
        (chroma != CH_MONO && (!u || !v)) || siting < SITE_CENTRE || siting > SITE_MPEG2 || matrix < 0 || matrix > 1)
        return VVAE_ERR_BAD_ARG;
    WinDims d{H, W, 0, 0, out_h, out_w, frames_per_clip, (float)H / (float)out_h, (float)W / (float)out_w,
              {INV[matrix * 2], INV[matrix * 2 + 1]}};
    if (chroma == CH_420) d.CH = H / 2 + 3, d.CW = W / 2 + 3;
    if (chroma == CH_444) d.CH = H, d.CW = W;
    const int xm = window_xm(W, out_w);
    const dim3 grid((unsigned)ceil_div(out_w, YW_LANES * YW_OPX), (unsigned)ceil_div(out_h, YW_ROWS),
                    (unsigned)(n < YW_MAX_GRID_Z ? n : YW_MAX_GRID_Z));
    hipStream_t s = (hipStream_t)stream;
    if (chroma == CH_420 && siting == SITE_CENTRE) launch_xm<CH_420, SITE_CENTRE, Out>(xm, grid, s, y, u, v, params, dst, n, d);
    else if (chroma == CH_420) launch_xm<CH_420, SITE_MPEG2, Out>(xm, grid, s, y, u, v, params, dst, n, d);
    else if (chroma == CH_444) launch_xm<CH_444, SITE_CENTRE, Out>(xm, grid, s, y, u, v, params, dst, n, d);
    else launch_xm<CH_MONO, SITE_CENTRE, Out>(xm, grid, s, y, u, v, params, dst, n, d);
    VVAE_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int vvae_yuv_window_supported(int H, int W, int chroma, int out_h, int out_w)
{
    return H >= 1 && W >= 1 && H <= YW_MAX_SIDE && W <= YW_MAX_SIDE && out_h >= 1 && out_w >= 1 && out_h <= YW_MAX_SIDE &&
           out_w <= YW_MAX_SIDE && chroma >= CH_420 && chroma <= CH_MONO;
}

// The output pixels of a row that one workgroup spans.
extern "C" int vvae_yuv_window_span(void) { return YW_LANES * YW_OPX; }

// Windows y (n, H, W), u, v (the window's chroma planes) uint8, all dense; clip_params int32 (ceil(n / frames_per_clip), 4) on the device
// -> dst (n, out_h, out_w, 3), fp32 or bf16 (dst_is_bf16 != 0), contiguous.  One launch for any n.
extern "C" int vvae_yuv_window_resize_norm(const uint8_t* y, const uint8_t* u, const uint8_t* v, const int* clip_params, void* dst,
                                           int dst_is_bf16, int n, int frames_per_clip, int H, int W, int chroma, int siting, int matrix,
                                           int out_h, int out_w, void* stream)
{
    if (dst_is_bf16)
        return launch_window<OutBF16>(y, u, v, clip_params, (bf16_t*)dst, n, frames_per_clip, H, W, chroma, siting, matrix, out_h, out_w, stream);
    return launch_window<OutF32>(y, u, v, clip_params, (float*)dst, n, frames_per_clip, H, W, chroma, siting, matrix, out_h, out_w, stream);
}
