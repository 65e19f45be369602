// Colour conversion between 8-bit Y'CbCr planes (YUV4MPEG2 clips) and interleaved RGB on the device.  video_vae_amd/y4m.py states the
// arithmetic (yuv_to_rgb_reference / rgb_to_yuv_reference); this file computes it the same way, byte for byte.  Everything is int32,
// >> an arithmetic shift.  A matrix is bt601 (0) or bt709 (1), a range limited (off = 16) or full (off = 0); the tables below hold the
// coefficients times 2^14.
//
// To RGB.  The chroma of luma pixel (y, x) is taken at 4 extra bits.  4:2:0: U16 = sum wv[i] wh[j] U[r_i][c_j] (likewise V16); rows
// r0 = y >> 1, r1 = r0 + 1 when y is odd, else r0 - 1, clamped to 0 .. CH - 1, wv = (3, 1); columns, centre siting: the same rule with x
// and CW; columns, mpeg2 siting: c0 = x >> 1, c1 = min(c0 + 1, CW - 1), wh = (4, 0) for even x and (2, 2) for odd x.  4:4:4: U16 = 16 U.
// mono: U16 = V16 = 2048.  With u = U16 - 2048, v = V16 - 2048, l = 16 cy (Y - off):
//   R = clip((l + crv v + 2^17) >> 18), G = clip((l + cgu u + cgv v + 2^17) >> 18), B = clip((l + cbu u + 2^17) >> 18).
// From RGB (4:2:0 centre siting and 4:4:4).  Y = clip((ry R + gy G + by B + (off << 14) + 2^13) >> 14); with a the sum of
// ru R + gu G + bu B over the pixel's 2 x 2 block (an index past the right or bottom edge reads the edge pixel again),
// U = clip((a + (128 << 16) + 2^15) >> 16), likewise V; 4:4:4 counts the one pixel four times.
//
// yuv_to_rgb_kernel<CHROMA, SITING>: blockIdx.x = piece of 2048 pixels of a row, blockIdx.y = band of YUV_ROWS rows, blockIdx.z = frame
// (grid-stride over frames).  A thread owns 8 consecutive pixels (x0 = 8 k) of the two rows 2 p and 2 p + 1, which share the chroma row
// p; the row above it serves the even row, the row below it the odd one.  The 4:2:0 column taps of the 8 pixels lie in the six chroma
// columns k2 - 1 .. k2 + 4 (k2 = x0 / 2, clamped to the plane), which are formed once; which two of them a pixel reads, and with which
// weights, depends on the pixel's place in the eight and the siting only.  Per row pair the thread reads the three chroma rows of both
// planes -- the four inner columns as one dword where they lie on a dword and inside the row, else as bytes, the two outer ones as
// bytes (planes of a file record start anywhere) -- and per row its 8 luma bytes as two dwords where aligned, and writes its 24 output
// bytes as six dwords where they lie on a dword, else as bytes.  Plain stores: the kernel's bytes are the next kernel's input on the same
// device, and write-through stores narrower than 16 bytes are one fabric write each.
// rgb_to_yuv_kernel<CHROMA>: blockIdx.x = piece of 1024 blocks (2048 pixels) of a row pair, blockIdx.y = band of YUV_BROWS row pairs,
// blockIdx.z = frame (grid-stride).  A thread owns 4 consecutive 2 x 2 blocks: 8 pixels of two rows, read as 6 dwords per row where they
// lie on a dword and inside the row; it writes 8 luma bytes per row (two dwords where aligned) and 4 bytes of U and of V (4:4:4: 8 per
// row).  Every output byte is written exactly once: no atomics, no memset, no workspace, no LDS, no cross-lane operation; bitwise
// reproducible; safe inside a captured hipGraph.
#include "common.hpp"
#include "yuv_common.hpp"

namespace {

constexpr int YUV_THREADS = 256;
constexpr int YUV_PX = 8;                    // to RGB: pixels of a row per thread
constexpr int YUV_ROWS = 8;                  // to RGB: rows per workgroup, as pairs
constexpr int YUV_BLK = 4;                   // from RGB: 2 x 2 blocks per thread
constexpr int YUV_BROWS = 4;                 // from RGB: row pairs per workgroup
constexpr int YUV_MAX_SIDE = 16384;
constexpr int YUV_MAX_GRID_Z = 65535;

struct YuvFwd { int ry, gy, by, ru, gu, bu, rv, gv, bv, off; };
const YuvFwd FWD[4] = {{4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170, 16}, {4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332, 0},
                       {2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660, 16}, {3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751, 0}};

// the first nb of the 4 bytes packed in w to p (none when nb <= 0)
__device__ __forceinline__ void store4(uint8_t* p, uint32_t w, int nb)
{
    if (nb >= 4 && ((uintptr_t)p & 3) == 0) *reinterpret_cast<uint32_t*>(p) = w;
    else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < nb) p[i] = (uint8_t)(w >> (8 * i));
    }
}

// the six chroma columns col[0 .. 5] = k2 - 1 .. k2 + 4 (clamped) of a chroma row: the inner four as a dword where they exist and align
__device__ __forceinline__ void load_cols(const uint8_t* row, const int (&col)[6], int k2, int CW, int (&c)[6])
{
    c[0] = (int)row[col[0]];
    if (k2 + 4 <= CW) load4(row + k2, 4, &c[1]);
    else {
#pragma unroll
        for (int j = 1; j < 5; ++j) c[j] = (int)row[col[j]];
    }
    c[5] = (int)row[col[5]];
}

template <int CHROMA, int SITING>
__global__ __launch_bounds__(YUV_THREADS) void yuv_to_rgb_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ up,
                                                                 const uint8_t* __restrict__ vp, long ys, long cs,
                                                                 uint8_t* __restrict__ rgb, int n, int H, int W, YuvInv k)
{
    const int x0 = (blockIdx.x * YUV_THREADS + threadIdx.x) * YUV_PX;
    if (x0 >= W) return;
    const int nb = min(YUV_PX, W - x0);                            // pixels of a row this thread owns
    const int CW = (W + 1) >> 1, CH = (H + 1) >> 1;
    const int k2 = x0 >> 1;
    int col[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) col[j] = min(max(k2 - 1 + j, 0), CW - 1);
    const int p_lo = blockIdx.y * (YUV_ROWS / 2), p_hi = min(p_lo + YUV_ROWS / 2, CH);
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const uint8_t* fy = yp + (long)f * ys;
        const uint8_t* fu = up + (long)f * cs;
        const uint8_t* fv = vp + (long)f * cs;
        uint8_t* fo = rgb + (long)f * H * W * 3;
        for (int p = p_lo; p < p_hi; ++p) {
            int cu[3][6], cv[3][6];                                // 4:2:0: the chroma rows above p, p, below p at the six columns
            if (CHROMA == CH_420) {
                const int rows[3] = {max(p - 1, 0), p, min(p + 1, CH - 1)};
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    load_cols(fu + (long)rows[r] * CW, col, k2, CW, cu[r]);
                    load_cols(fv + (long)rows[r] * CW, col, k2, CW, cv[r]);
                }
            }
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const int y = 2 * p + rr;
                if (y >= H) break;
                int Y[8], U16[8], V16[8];
                const long o = (long)y * W + x0;
                load4(fy + o, nb, &Y[0]);
                load4(fy + o + 4, nb - 4, &Y[4]);
                if (CHROMA == CH_420) {
                    int tu[6], tv[6];                              // the rows folded: 3 U[r0][c] + U[r1][c] at the six columns
#pragma unroll
                    for (int j = 0; j < 6; ++j) {
                        tu[j] = 3 * cu[1][j] + cu[2 * rr][j];
                        tv[j] = 3 * cv[1][j] + cv[2 * rr][j];
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int a = 1 + (i >> 1);                // the pixel's own column, then its neighbour, and their weights
                        const int b = SITING == SITE_CENTRE ? ((i & 1) ? a + 1 : a - 1) : a + 1;
                        const int wa = SITING == SITE_CENTRE ? 3 : ((i & 1) ? 2 : 4), wb = 4 - wa;
                        U16[i] = wa * tu[a] + wb * tu[b];
                        V16[i] = wa * tv[a] + wb * tv[b];
                    }
                } else if (CHROMA == CH_444) {
                    load4(fu + o, nb, &U16[0]);
                    load4(fu + o + 4, nb - 4, &U16[4]);
                    load4(fv + o, nb, &V16[0]);
                    load4(fv + o + 4, nb - 4, &V16[4]);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        U16[i] *= 16;
                        V16[i] *= 16;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i) U16[i] = V16[i] = 2048;
                }
                uint32_t w[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int l = 16 * k.cy * (Y[i] - k.off), u = U16[i] - 2048, v = V16[i] - 2048;
                    const int c[3] = {clip255((l + k.crv * v + (1 << 17)) >> 18), clip255((l + k.cgu * u + k.cgv * v + (1 << 17)) >> 18),
                                      clip255((l + k.cbu * u + (1 << 17)) >> 18)};
#pragma unroll
                    for (int j = 0; j < 3; ++j) w[(3 * i + j) >> 2] |= (uint32_t)c[j] << (8 * ((3 * i + j) & 3));
                }
                uint8_t* dst = fo + o * 3;
                if (nb == YUV_PX && ((uintptr_t)dst & 3) == 0) {
#pragma unroll
                    for (int j = 0; j < 6; ++j) reinterpret_cast<uint32_t*>(dst)[j] = w[j];
                } else {
#pragma unroll
                    for (int j = 0; j < 24; ++j)
                        if (j < 3 * nb) dst[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
                }
            }
        }
    }
}

template <int CHROMA>
__global__ __launch_bounds__(YUV_THREADS) void rgb_to_yuv_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ yp,
                                                                 uint8_t* __restrict__ up, uint8_t* __restrict__ vp, int n, int H, int W,
                                                                 YuvFwd k)
{
    const int b0 = (blockIdx.x * YUV_THREADS + threadIdx.x) * YUV_BLK;     // the thread's first block column
    const int x0 = 2 * b0;
    if (x0 >= W) return;
    const int npx = min(2 * YUV_BLK, W - x0);                              // pixels of a row this thread owns
    const int CW = (W + 1) >> 1, CH = (H + 1) >> 1;
    const int nbk = min(YUV_BLK, CW - b0);                                 // blocks of a row pair this thread owns
    const int p_lo = blockIdx.y * YUV_BROWS, p_hi = min(p_lo + YUV_BROWS, CH);
    const long cplane = CHROMA == CH_444 ? (long)H * W : (long)CH * CW;
    const int bias = (128 << 16) + (1 << 15);
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const uint8_t* fi = rgb + (long)f * H * W * 3;
        uint8_t* fy = yp + (long)f * H * W;
        uint8_t* fu = up + (long)f * cplane;
        uint8_t* fv = vp + (long)f * cplane;
        for (int p = p_lo; p < p_hi; ++p) {
            int au[YUV_BLK] = {0, 0, 0, 0}, av[YUV_BLK] = {0, 0, 0, 0};
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const int yy = 2 * p + rr, yr = min(yy, H - 1);            // past the bottom edge: the edge row again
                const uint8_t* src = fi + ((long)yr * W + x0) * 3;
                int c[2 * YUV_BLK][3];
                if (npx == 2 * YUV_BLK && ((uintptr_t)src & 3) == 0) {
#pragma unroll
                    for (int j = 0; j < 6; ++j) {
                        const uint32_t w = reinterpret_cast<const uint32_t*>(src)[j];
#pragma unroll
                        for (int b = 0; b < 4; ++b) c[(4 * j + b) / 3][(4 * j + b) % 3] = (int)((w >> (8 * b)) & 255u);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 2 * YUV_BLK; ++i) {
                        const int xi = min(i, npx - 1);                    // past the right edge: the edge pixel again
#pragma unroll
                        for (int j = 0; j < 3; ++j) c[i][j] = (int)src[3 * xi + j];
                    }
                }
                uint32_t wy[2] = {0u, 0u}, wu[2] = {0u, 0u}, wv[2] = {0u, 0u};
#pragma unroll
                for (int i = 0; i < 2 * YUV_BLK; ++i) {
                    const int R = c[i][0], G = c[i][1], B = c[i][2];
                    const int luma = clip255((k.ry * R + k.gy * G + k.by * B + (k.off << 14) + (1 << 13)) >> 14);
                    const int cu = k.ru * R + k.gu * G + k.bu * B, cv = k.rv * R + k.gv * G + k.bv * B;
                    wy[i >> 2] |= (uint32_t)luma << (8 * (i & 3));
                    if (CHROMA == CH_444) {
                        wu[i >> 2] |= (uint32_t)clip255((4 * cu + bias) >> 16) << (8 * (i & 3));
                        wv[i >> 2] |= (uint32_t)clip255((4 * cv + bias) >> 16) << (8 * (i & 3));
                    } else {
                        au[i >> 1] += cu;
                        av[i >> 1] += cv;
                    }
                }
                if (yy < H) {
                    const long o = (long)yy * W + x0;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int nbj = min(4, npx - 4 * j);               // <= 0: nothing of this dword exists
                        store4(fy + o + 4 * j, wy[j], nbj);
                        if (CHROMA == CH_444) {
                            store4(fu + o + 4 * j, wu[j], nbj);
                            store4(fv + o + 4 * j, wv[j], nbj);
                        }
                    }
                }
            }
            if (CHROMA == CH_420) {
                uint32_t wu = 0u, wv = 0u;
#pragma unroll
                for (int i = 0; i < YUV_BLK; ++i) {
                    wu |= (uint32_t)clip255((au[i] + bias) >> 16) << (8 * i);
                    wv |= (uint32_t)clip255((av[i] + bias) >> 16) << (8 * i);
                }
                store4(fu + (long)p * CW + b0, wu, nbk);
                store4(fv + (long)p * CW + b0, wv, nbk);
            }
        }
    }
}

}  // namespace

extern "C" int vvae_yuv_supported(int H, int W, int chroma)
{
    return H >= 1 && W >= 1 && H <= YUV_MAX_SIDE && W <= YUV_MAX_SIDE && chroma >= CH_420 && chroma <= CH_MONO;
}

// Planes y (n, H, W), u and v (n, CH, CW) uint8, rows dense inside a frame, frame f of a plane at base + f stride bytes (any alignment:
// the planes of frame records uploaded as they lie in a file) -> rgb uint8 (n, H, W, 3) contiguous.  One launch for any n.
extern "C" int vvae_yuv_to_rgb_u8(const uint8_t* y, const uint8_t* u, const uint8_t* v, long y_frame_stride, long c_frame_stride,
                                  uint8_t* rgb, int n, int H, int W, int chroma, int siting, int matrix, int full_range, void* stream)
{
    if (!y || !rgb || n < 1 || !vvae_yuv_supported(H, W, chroma) || (chroma != CH_MONO && (!u || !v)) || siting < SITE_CENTRE ||
        siting > SITE_MPEG2 || matrix < 0 || matrix > 1 || y_frame_stride < 0 || c_frame_stride < 0)
        return VVAE_ERR_BAD_ARG;
    const YuvInv k = INV[matrix * 2 + (full_range ? 1 : 0)];
    const dim3 grid((unsigned)ceil_div(W, YUV_THREADS * YUV_PX), (unsigned)ceil_div(H, YUV_ROWS),
                    (unsigned)(n < YUV_MAX_GRID_Z ? n : YUV_MAX_GRID_Z));
    const dim3 block(YUV_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (chroma == CH_420 && siting == SITE_CENTRE)
        hipLaunchKernelGGL((yuv_to_rgb_kernel<CH_420, SITE_CENTRE>), grid, block, 0, s, y, u, v, y_frame_stride, c_frame_stride, rgb, n, H, W, k);
    else if (chroma == CH_420)
        hipLaunchKernelGGL((yuv_to_rgb_kernel<CH_420, SITE_MPEG2>), grid, block, 0, s, y, u, v, y_frame_stride, c_frame_stride, rgb, n, H, W, k);
    else if (chroma == CH_444)
        hipLaunchKernelGGL((yuv_to_rgb_kernel<CH_444, SITE_CENTRE>), grid, block, 0, s, y, u, v, y_frame_stride, c_frame_stride, rgb, n, H, W, k);
    else
        hipLaunchKernelGGL((yuv_to_rgb_kernel<CH_MONO, SITE_CENTRE>), grid, block, 0, s, y, u, v, y_frame_stride, c_frame_stride, rgb, n, H, W, k);
    VVAE_LAUNCH_CHECK();
    return 0;
}

// rgb uint8 (n, H, W, 3) contiguous -> planes y (n, H, W), u and v (n, CH, CW) uint8 contiguous, 4:2:0 (centre siting) or 4:4:4.  One
// launch for any n.
extern "C" int vvae_rgb_to_yuv(const uint8_t* rgb, uint8_t* y, uint8_t* u, uint8_t* v, int n, int H, int W, int chroma, int matrix,
                               int full_range, void* stream)
{
    if (!rgb || !y || !u || !v || n < 1 || !vvae_yuv_supported(H, W, chroma) || chroma == CH_MONO || matrix < 0 || matrix > 1)
        return VVAE_ERR_BAD_ARG;
    const YuvFwd k = FWD[matrix * 2 + (full_range ? 1 : 0)];
    const int CW = (W + 1) / 2, CH = (H + 1) / 2;
    const dim3 grid((unsigned)ceil_div(CW, YUV_THREADS * YUV_BLK), (unsigned)ceil_div(CH, YUV_BROWS),
                    (unsigned)(n < YUV_MAX_GRID_Z ? n : YUV_MAX_GRID_Z));
    const dim3 block(YUV_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (chroma == CH_420) hipLaunchKernelGGL((rgb_to_yuv_kernel<CH_420>), grid, block, 0, s, rgb, y, u, v, n, H, W, k);
    else hipLaunchKernelGGL((rgb_to_yuv_kernel<CH_444>), grid, block, 0, s, rgb, y, u, v, n, H, W, k);
    VVAE_LAUNCH_CHECK();
    return 0;
}
