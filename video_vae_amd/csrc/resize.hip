// Crop + bilinear resize of uint8 frames on the device (video_vae_amd/data.py: resize_reference_u8 states the arithmetic; this file computes
// it the same way, byte for byte): src (n, H, W, C) -> the crop [top, top + crop_h) x [left, left + crop_w) of every frame resized to
// dst (n, out_h, out_w, C), half-pixel centres, the edge taps clamped -- what torch's bilinear interpolate (align_corners = False) on the
// cropped fp32 planes, rounded to nearest even and clamped to 0 .. 255, gives on the host.
//
// Per axis with input extent I (the crop's) and output extent O, all fp32, round to nearest, nothing fused:
//   scale = float(I) / float(O) (an IEEE division, done once on the host by the launcher);
//   src = scale * (float(d) + 0.5f) - 0.5f, 0 when negative;  i0 = min((int)src, I - 1), i1 = i0 + (i0 < I - 1);
//   l1 = src - float(i0), l0 = 1.0f - l1.
// Per pixel and channel, rows (y0, y1, a0, a1), columns (x0, x1, b0, b1), s the source bytes as fp32:
//   v = (a0 * ((b0 * s[y0][x0]) + (b1 * s[y0][x1]))) + (a1 * ((b0 * s[y1][x0]) + (b1 * s[y1][x1]))), every product and sum rounded on
//   its own; out = v rounded to nearest even, clamped to 0 .. 255.  Equal extents give l1 = 0: an exact copy, no special case.
//
// FMA contraction is switched OFF for this whole file (the pragma below): hipcc would otherwise fuse a * b + c on the device, which
// rounds once instead of twice and changes bytes.  (The __fmul_rn / __fadd_rn intrinsics are plain operators in this HIP and would not
// stop it.)
//
// crop_resize_kernel<C, Out>: blockIdx.x = 1024-element piece of the flat out_w C output row, blockIdx.y = band of RZ_ROWS output rows,
// blockIdx.z = frame (grid-stride over frames).  A thread owns 4 consecutive elements of the output row; its column taps (x0 C + c,
// x1 C + c, b0, b1 per element) are formed once and reused over the band's rows and the frames; per row it reads 16 source bytes and
// writes its 4 elements as one vector store (element stores where they are not aligned to the vector in memory or run past the row:
// out_w C not a multiple of 4).  Every output element is written once: no atomics, no memset, no workspace; bitwise reproducible; safe
// inside a captured hipGraph.
//
// Out is the output policy, the only thing the three entry points differ in; the tap arithmetic above it exists once.  With q the
// rounded, clamped value (an integer 0 .. 255 held in fp32):
//   OutByte: the byte q, 4 of them in one dword                                  (vvae_crop_resize_u8);
//   OutF32:  q / 255.0f, an IEEE fp32 division (hipcc's default division is correctly rounded), 4 in one 16-byte store;
//   OutBF16: that quotient rounded to nearest even to bf16, 4 in one 8-byte store (vvae_crop_resize_norm: the training loader's
//            u8.float() / 255 -> compute dtype, fused behind the resize).
#include "common.hpp"

#pragma clang fp contract(off)

#include "resize_common.hpp"

namespace {

constexpr int RZ_THREADS = 256;
constexpr int RZ_ROWS = 8;                   // output rows per workgroup
constexpr int RZ_MAX_SIDE = 16384;           // every extent, source and output
constexpr int RZ_MAX_GRID_Z = 65535;

struct ResizeDims {
    int H, W, top, left, crop_h, crop_w, out_h, out_w;
    float sy, sx;                            // float(crop_h) / float(out_h), float(crop_w) / float(out_w)
};

template <int C, typename Out>
__global__ __launch_bounds__(RZ_THREADS) void crop_resize_kernel(const uint8_t* __restrict__ src, typename Out::T* __restrict__ dst, int n,
                                                                 ResizeDims d)
{
    const int L = d.out_w * C;                                     // elements of an output row
    const int e0 = (blockIdx.x * RZ_THREADS + threadIdx.x) * 4;
    if (e0 >= L) return;
    const int nb = min(4, L - e0);                                 // elements of the row this thread owns
    int o0[4], o1[4];
    float b0[4], b1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int el = min(e0 + i, L - 1), j = el / C, c = el - j * C;
        int x0, x1;
        rz_axis(j, d.sx, d.crop_w, x0, x1, b0[i], b1[i]);
        o0[i] = x0 * C + c;
        o1[i] = x1 * C + c;
    }
    const int r0 = blockIdx.y * RZ_ROWS, r1 = min(r0 + RZ_ROWS, d.out_h);
    const long pitch = (long)d.W * C;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const uint8_t* fsrc = src + ((long)f * d.H + d.top) * pitch + (long)d.left * C;
        typename Out::T* fdst = dst + (long)f * d.out_h * L;
        for (int y = r0; y < r1; ++y) {
            int y0, y1;
            float a0, a1;
            rz_axis(y, d.sy, d.crop_h, y0, y1, a0, a1);
            const uint8_t* p0 = fsrc + y0 * pitch;
            const uint8_t* p1 = fsrc + y1 * pitch;
            float s[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s[i][0] = (float)p0[o0[i]];
                s[i][1] = (float)p0[o1[i]];
                s[i][2] = (float)p1[o0[i]];
                s[i][3] = (float)p1[o1[i]];
            }
            float q[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float t = (b0[i] * s[i][0]) + (b1[i] * s[i][1]);
                const float b = (b0[i] * s[i][2]) + (b1[i] * s[i][3]);
                const float v = (a0 * t) + (a1 * b);
                q[i] = fminf(fmaxf(rintf(v), 0.f), 255.f);
            }
            Out::store(fdst + (long)y * L + e0, q, nb);
        }
    }
}

}  // namespace

extern "C" int vvae_crop_resize_supported(int H, int W, int C, int crop_h, int crop_w, int out_h, int out_w)
{
    return H >= 1 && W >= 1 && H <= RZ_MAX_SIDE && W <= RZ_MAX_SIDE && C >= 1 && C <= 4 && crop_h >= 1 && crop_w >= 1 && crop_h <= H &&
           crop_w <= W && out_h >= 1 && out_w >= 1 && out_h <= RZ_MAX_SIDE && out_w <= RZ_MAX_SIDE;
}

namespace {

// The argument rules of every entry point and the one launch: 0, VVAE_ERR_BAD_ARG (nothing launched) or a hipError_t.
template <typename Out>
int launch_crop_resize(const uint8_t* src, typename Out::T* dst, int n, int H, int W, int C, int top, int left, int crop_h, int crop_w,
                       int out_h, int out_w, void* stream)
{
    if (!src || !dst || n < 1 || !vvae_crop_resize_supported(H, W, C, crop_h, crop_w, out_h, out_w) || top < 0 || left < 0 ||
        top > H - crop_h || left > W - crop_w)
        return VVAE_ERR_BAD_ARG;
    ResizeDims d{H, W, top, left, crop_h, crop_w, out_h, out_w, (float)crop_h / (float)out_h, (float)crop_w / (float)out_w};
    const dim3 grid((unsigned)ceil_div((long)out_w * C, RZ_THREADS * 4), (unsigned)ceil_div(out_h, RZ_ROWS),
                    (unsigned)(n < RZ_MAX_GRID_Z ? n : RZ_MAX_GRID_Z));
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
    case 1: hipLaunchKernelGGL((crop_resize_kernel<1, Out>), grid, dim3(RZ_THREADS), 0, s, src, dst, n, d); break;
    case 2: hipLaunchKernelGGL((crop_resize_kernel<2, Out>), grid, dim3(RZ_THREADS), 0, s, src, dst, n, d); break;
    case 3: hipLaunchKernelGGL((crop_resize_kernel<3, Out>), grid, dim3(RZ_THREADS), 0, s, src, dst, n, d); break;
    default: hipLaunchKernelGGL((crop_resize_kernel<4, Out>), grid, dim3(RZ_THREADS), 0, s, src, dst, n, d); break;
    }
    VVAE_LAUNCH_CHECK();
    return 0;
}

}  // namespace

// src uint8 (n, H, W, C) contiguous -> dst uint8 (n, out_h, out_w, C) contiguous: the crop at (top, left) of crop_h x crop_w, resized.
// One launch for any n.
extern "C" int vvae_crop_resize_u8(const uint8_t* src, uint8_t* dst, int n, int H, int W, int C, int top, int left, int crop_h, int crop_w,
                                   int out_h, int out_w, void* stream)
{
    return launch_crop_resize<OutByte>(src, dst, n, H, W, C, top, left, crop_h, crop_w, out_h, out_w, stream);
}

// The same crop and resize with every byte q written as q / 255.0f: dst fp32, or bf16 when dst_is_bf16 != 0, (n, out_h, out_w, C)
// contiguous.  One launch for any n.
extern "C" int vvae_crop_resize_norm(const uint8_t* src, void* dst, int dst_is_bf16, int n, int H, int W, int C, int top, int left,
                                     int crop_h, int crop_w, int out_h, int out_w, void* stream)
{
    if (dst_is_bf16) return launch_crop_resize<OutBF16>(src, (bf16_t*)dst, n, H, W, C, top, left, crop_h, crop_w, out_h, out_w, stream);
    return launch_crop_resize<OutF32>(src, (float*)dst, n, H, W, C, top, left, crop_h, crop_w, out_h, out_w, stream);
}
