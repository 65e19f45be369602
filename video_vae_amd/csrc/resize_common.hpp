// What the resizing kernels share (resize.hip, yuv_window.hip): the tap rule of an axis and the output policies.  Include it behind
// "#pragma clang fp contract(off)": nothing here may be fused.
#pragma once
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

// output index d of an axis with input extent I: taps i0, i1 and their weights l0, l1
__device__ __forceinline__ void rz_axis(int d, float scale, int I, int& i0, int& i1, float& l0, float& l1)
{
    float src = scale * ((float)d + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    i0 = min((int)src, I - 1);
    i1 = i0 + (i0 < I - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.0f - l1;
}

// Output policies: T is the element type; store() writes the first nb of the thread's 4 values q (integers 0 .. 255 in fp32) at o.
struct OutByte {
    typedef uint8_t T;
    static __device__ __forceinline__ void store(T* o, const float (&q)[4], int nb)
    {
        uint32_t w = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) w |= (uint32_t)q[i] << (8 * i);
        if (nb == 4 && ((uintptr_t)o & 3) == 0) *reinterpret_cast<uint32_t*>(o) = w;
        else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < nb) o[i] = (uint8_t)(w >> (8 * i));
        }
    }
};

struct OutF32 {
    typedef float T;
    static __device__ __forceinline__ void store(T* o, const float (&q)[4], int nb)
    {
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = q[i] / 255.0f;
        // a native vector type: a float4 struct store is taken apart and put together again as 12 + 4 bytes around the branch
        if (nb == 4 && ((uintptr_t)o & 15) == 0) *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
        else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < nb) o[i] = v[i];
        }
    }
};

struct OutBF16 {
    typedef bf16_t T;
    static __device__ __forceinline__ void store(T* o, const float (&q)[4], int nb)
    {
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = q[i] / 255.0f;
        if (nb == 4 && ((uintptr_t)o & 7) == 0) VecIO<bf16_t, 4>::store(o, v);
        else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < nb) o[i] = f2bf(v[i]);
        }
    }
};

}  // namespace
