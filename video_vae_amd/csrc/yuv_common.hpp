// What the Y'CbCr kernels share (yuv.hip, yuv_window.hip): the codes of the C ABI, the to-RGB coefficients and the byte loads.
#pragma once
#include "common.hpp"

namespace {

enum { CH_420 = 0, CH_444 = 1, CH_MONO = 2 };
enum { SITE_CENTRE = 0, SITE_MPEG2 = 1 };

struct YuvInv { int cy, crv, cgu, cgv, cbu, off; };

// [matrix * 2 + full_range]
const YuvInv INV[4] = {{19077, 26149, -6419, -13320, 33050, 16}, {16384, 22970, -5638, -11700, 29032, 0},
                       {19077, 29372, -3494, -8731, 34610, 16}, {16384, 25802, -3069, -7670, 30402, 0}};

__device__ __forceinline__ int clip255(int v) { return min(max(v, 0), 255); }

// the first nb (<= 4; none when nb <= 0) bytes at p, the last of them again in the places after it: one dword when all four exist and p
// lies on a dword
__device__ __forceinline__ void load4(const uint8_t* p, int nb, int* b)
{
    if (nb >= 4 && ((uintptr_t)p & 3) == 0) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = (int)((w >> (8 * i)) & 255u);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = nb > 0 ? (int)p[min(i, nb - 1)] : 0;
    }
}

}  // namespace
