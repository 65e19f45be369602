// Latent quantiser (video_vae_amd/quant.py: quantise_reference / dequantise_reference state the arithmetic; this file computes it the same
// way, bit for bit): latent (frames, hw, ld) bf16 or fp32 -> codes int8 (frames, hw, ld), step fp32 (frames, ld), counts uint32
// (frames, 256), and optionally the dequantised values written back over the latent.
//
// Uniform, symmetric, scalar, one step per (frame, channel).  With bits in 2 .. 8, qmax = 2^(bits - 1) - 1, per frame and channel c:
//   amax[c] = max_i |x[i, c]| (exact: the integer maximum of the bit patterns of |x|, which order as the values do; a NaN or an
//             infinity anywhere in the channel gives a pattern >= 0x7f800000);
//   dead    = amax not finite, or amax < 1e-30f (zero included): step[c] = 0, every code 0;
//   inv[c]  = float(qmax) / amax[c], step[c] = amax[c] / float(qmax): two IEEE divisions per channel, none per element;
//   q[i, c] = clamp(rint(x[i, c] * inv[c]), -qmax, qmax), ties to even;  xq[i, c] = float(q[i, c]) * step[c], rounded to the latent's
//             dtype where it is written back.
// FMA contraction is OFF for this whole file (the pragma below), as in resize.hip: every product is rounded on its own.
//
// latent_quantise_kernel<T, CACHED>: one workgroup of 256 threads per frame.  A thread owns groups of 8 consecutive elements (16 bytes of
// bf16, two 16-byte loads of fp32; ld is a multiple of 8, so a group lies in one token and its channels are c0 .. c0 + 7), group g =
// tid + 256 i.  CACHED (at most 12 groups per thread: the production frame 256 x 96 is exactly 12): the frame is loaded once and stays
// in registers between the max pass and the quantise pass; otherwise the second pass reads the frame again (still in L2).  The channel
// maxima and the histogram are LDS integer atomics that stay inside the workgroup; a thread adds a run of equal codes at once
// (scenes.hip's trick), so a flat frame costs one LDS add per thread.  A frame whose keep flag is zero is not read: its latent stays as
// it is, its codes, steps and counts are written as zeros.  Every output element is written by every launch: no global atomics, no
// float atomics, no memset, no workspace; bitwise reproducible; safe inside a captured hipGraph.
//
// latent_fake_quant_kernel is its out-of-place form for the train step; latent_rate_kernel / latent_rate_grad_kernel (quant.py:
// rate_reference) price the unrounded codes under a 256-entry cost table and give the gradient of that price, on the same front end.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int LQ_THREADS = 256;
constexpr int LQ_GROUP = 8;                  // elements per thread and step
constexpr int LQ_CACHED = 12;                // groups per thread that stay in registers (96 elements)
constexpr int LQ_MAX_LD = 1024;
constexpr long LQ_MAX_FRAME = 1L << 30;      // elements per frame

__device__ __forceinline__ void lq_load(const bf16_t* p, float (&x)[LQ_GROUP]) { VecIO<bf16_t, 8>::load(p, x); }
__device__ __forceinline__ void lq_load(const float* p, float (&x)[LQ_GROUP])
{
    float a[4], b[4];
    VecIO<float, 4>::load(p, a);
    VecIO<float, 4>::load(p + 4, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        x[j] = a[j];
        x[4 + j] = b[j];
    }
}
__device__ __forceinline__ void lq_store(bf16_t* p, const float (&x)[LQ_GROUP]) { VecIO<bf16_t, 8>::store(p, x); }
__device__ __forceinline__ void lq_store(float* p, const float (&x)[LQ_GROUP])
{
    const float a[4] = {x[0], x[1], x[2], x[3]}, b[4] = {x[4], x[5], x[6], x[7]};
    VecIO<float, 4>::store(p, a);
    VecIO<float, 4>::store(p + 4, b);
}

__device__ __forceinline__ void lq_max(const float (&x)[LQ_GROUP], unsigned* __restrict__ amax)
{
#pragma unroll
    for (int j = 0; j < LQ_GROUP; ++j) atomicMax(amax + j, __float_as_uint(x[j]) & 0x7fffffffu);
}

// one element: its code q = clamp(rint(x inv), -qmax, qmax) (0 in a dead channel), x replaced by float(q) * step -- through the integer, so
// a code 0 gives +0.0 and never -0.0 -- and the histogram run it extends or ends
__device__ __forceinline__ int lq_code(float& x, float inv, float st, float qmax, int& cur, unsigned& run, unsigned* __restrict__ hist)
{
    float r = fminf(fmaxf(rintf(x * inv), -qmax), qmax);
    r = st == 0.f ? 0.f : r;                                       // a dead channel: x * 0 may be NaN
    const int q = (int)r;
    x = (float)q * st;
    const int bin = q + 128;
    if (bin != cur) {
        if (run) atomicAdd(hist + cur, run);
        cur = bin;
        run = 0;
    }
    ++run;
    return q;
}

// one group: its 8 codes (stored as two words), the histogram runs, and the dequantised values over the latent when asked for
template <typename T>
__device__ __forceinline__ void lq_quantise(float (&x)[LQ_GROUP], const float* __restrict__ inv, const float* __restrict__ step, float qmax,
                                            int8_t* __restrict__ codes, T* __restrict__ latent, bool dequantise, int& cur, unsigned& run,
                                            unsigned* __restrict__ hist)
{
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < LQ_GROUP; ++j) {
        const int q = lq_code(x[j], inv[j], step[j], qmax, cur, run, hist);
        w[j >> 2] |= ((uint32_t)q & 0xffu) << (8 * (j & 3));
    }
    *reinterpret_cast<uint2*>(codes) = make_uint2(w[0], w[1]);
    if (dequantise) lq_store(latent, x);
}

// blockIdx.x = frame; groups = hw ld / 8
template <typename T, bool CACHED>
__global__ __launch_bounds__(LQ_THREADS) void latent_quantise_kernel(T* __restrict__ latent, const float* __restrict__ keep,
                                                                     int8_t* __restrict__ codes, float* __restrict__ step,
                                                                     unsigned* __restrict__ counts, int groups, int ld, int iqmax,
                                                                     int dequantise)
{
    __shared__ unsigned amax[LQ_MAX_LD];
    __shared__ float s_inv[LQ_MAX_LD];
    __shared__ float s_step[LQ_MAX_LD];
    __shared__ unsigned hist[256];
    const long f = blockIdx.x;
    const int tid = threadIdx.x;
    const long n = (long)groups * LQ_GROUP;
    int8_t* fcodes = codes + f * n;
    float* fstep = step + f * ld;
    unsigned* fcounts = counts + f * 256;
    if (!(keep[f] != 0.f)) {                                       // dropped or padding: the latent is not touched (uniform branch)
        for (int g = tid; g < groups; g += LQ_THREADS) *reinterpret_cast<uint2*>(fcodes + (long)g * LQ_GROUP) = make_uint2(0u, 0u);
        for (int c = tid; c < ld; c += LQ_THREADS) fstep[c] = 0.f;
        fcounts[tid] = 0u;
        return;
    }
    for (int c = tid; c < ld; c += LQ_THREADS) amax[c] = 0u;
    hist[tid] = 0u;
    __syncthreads();
    T* src = latent + f * n;
    float x[CACHED ? LQ_CACHED : 1][LQ_GROUP];
    if (CACHED) {
#pragma unroll
        for (int i = 0; i < LQ_CACHED; ++i) {
            const int g = tid + i * LQ_THREADS;
            if (g < groups) {
                lq_load(src + (long)g * LQ_GROUP, x[i]);
                lq_max(x[i], amax + (int)(((long)g * LQ_GROUP) % ld));
            }
        }
    } else {
        for (int g = tid; g < groups; g += LQ_THREADS) {
            lq_load(src + (long)g * LQ_GROUP, x[0]);
            lq_max(x[0], amax + (int)(((long)g * LQ_GROUP) % ld));
        }
    }
    __syncthreads();
    const float qmax = (float)iqmax;
    for (int c = tid; c < ld; c += LQ_THREADS) {
        const unsigned bits = amax[c];
        const float a = __uint_as_float(bits);
        const bool dead = bits >= 0x7f800000u || a < 1e-30f;
        const float iv = dead ? 0.f : qmax / a;                    // IEEE divisions (hipcc's default fp32 division is correctly rounded)
        const float st = dead ? 0.f : a / qmax;
        s_inv[c] = iv;
        s_step[c] = st;
        fstep[c] = st;
    }
    __syncthreads();
    int cur = 128;
    unsigned run = 0;
    if (CACHED) {
#pragma unroll
        for (int i = 0; i < LQ_CACHED; ++i) {
            const int g = tid + i * LQ_THREADS;
            if (g < groups) {
                const long e = (long)g * LQ_GROUP;
                const int c0 = (int)(e % ld);
                lq_quantise<T>(x[i], s_inv + c0, s_step + c0, qmax, fcodes + e, src + e, dequantise != 0, cur, run, hist);
            }
        }
    } else {
        for (int g = tid; g < groups; g += LQ_THREADS) {
            const long e = (long)g * LQ_GROUP;
            const int c0 = (int)(e % ld);
            lq_load(src + e, x[0]);
            lq_quantise<T>(x[0], s_inv + c0, s_step + c0, qmax, fcodes + e, src + e, dequantise != 0, cur, run, hist);
        }
    }
    if (run) atomicAdd(hist + cur, run);
    __syncthreads();
    fcounts[tid] = hist[tid];
}

template <typename T>
void lq_launch(void* latent, const float* keep, int8_t* codes, float* step, unsigned* counts, int frames, int groups, int ld, int qmax,
               int dequantise, hipStream_t s)
{
    if (groups <= LQ_CACHED * LQ_THREADS)
        hipLaunchKernelGGL((latent_quantise_kernel<T, true>), dim3((unsigned)frames), dim3(LQ_THREADS), 0, s, (T*)latent, keep, codes, step,
                           counts, groups, ld, qmax, dequantise);
    else
        hipLaunchKernelGGL((latent_quantise_kernel<T, false>), dim3((unsigned)frames), dim3(LQ_THREADS), 0, s, (T*)latent, keep, codes, step,
                           counts, groups, ld, qmax, dequantise);
}

// ---- the training form (quantisation-aware training): dst = the dequantised src on kept frames, src itself on the others ----
// one group: x becomes float(q) * step (lq_code); no code is stored
__device__ __forceinline__ void lq_fake(float (&x)[LQ_GROUP], const float* __restrict__ inv, const float* __restrict__ step, float qmax, int& cur,
                                        unsigned& run, unsigned* __restrict__ hist)
{
#pragma unroll
    for (int j = 0; j < LQ_GROUP; ++j) lq_code(x[j], inv[j], step[j], qmax, cur, run, hist);
}

// blockIdx.x = frame; groups = hw ld / 8.  Out of place: src is only read, every element of dst is written (a dropped frame as 16-byte
// words, so its bits pass whatever they encode).  counts may be null: then no histogram leaves the workgroup.
template <typename T, bool CACHED>
__global__ __launch_bounds__(LQ_THREADS) void latent_fake_quant_kernel(const T* __restrict__ src, T* __restrict__ dst,
                                                                       const float* __restrict__ keep, unsigned* __restrict__ counts,
                                                                       int groups, int ld, int iqmax)
{
    __shared__ unsigned amax[LQ_MAX_LD];
    __shared__ float s_inv[LQ_MAX_LD];
    __shared__ float s_step[LQ_MAX_LD];
    __shared__ unsigned hist[256];
    const long f = blockIdx.x;
    const int tid = threadIdx.x;
    const long n = (long)groups * LQ_GROUP;
    const T* fsrc = src + f * n;
    T* fdst = dst + f * n;
    if (!(keep[f] != 0.f)) {                                       // dropped or padding: copied through (uniform branch)
        const uint4* s4 = reinterpret_cast<const uint4*>(fsrc);
        uint4* d4 = reinterpret_cast<uint4*>(fdst);
        const long words = n * (long)sizeof(T) / 16;
        for (long w = tid; w < words; w += LQ_THREADS) d4[w] = s4[w];
        if (counts) counts[f * 256 + tid] = 0u;
        return;
    }
    for (int c = tid; c < ld; c += LQ_THREADS) amax[c] = 0u;
    hist[tid] = 0u;
    __syncthreads();
    float x[CACHED ? LQ_CACHED : 1][LQ_GROUP];
    if (CACHED) {
#pragma unroll
        for (int i = 0; i < LQ_CACHED; ++i) {
            const int g = tid + i * LQ_THREADS;
            if (g < groups) {
                lq_load(fsrc + (long)g * LQ_GROUP, x[i]);
                lq_max(x[i], amax + (int)(((long)g * LQ_GROUP) % ld));
            }
        }
    } else {
        for (int g = tid; g < groups; g += LQ_THREADS) {
            lq_load(fsrc + (long)g * LQ_GROUP, x[0]);
            lq_max(x[0], amax + (int)(((long)g * LQ_GROUP) % ld));
        }
    }
    __syncthreads();
    const float qmax = (float)iqmax;
    for (int c = tid; c < ld; c += LQ_THREADS) {
        const unsigned bits = amax[c];
        const float a = __uint_as_float(bits);
        const bool dead = bits >= 0x7f800000u || a < 1e-30f;
        s_inv[c] = dead ? 0.f : qmax / a;                          // the two IEEE divisions of latent_quantise_kernel
        s_step[c] = dead ? 0.f : a / qmax;
    }
    __syncthreads();
    int cur = 128;
    unsigned run = 0;
    if (CACHED) {
#pragma unroll
        for (int i = 0; i < LQ_CACHED; ++i) {
            const int g = tid + i * LQ_THREADS;
            if (g < groups) {
                const long e = (long)g * LQ_GROUP;
                const int c0 = (int)(e % ld);
                lq_fake(x[i], s_inv + c0, s_step + c0, qmax, cur, run, hist);
                lq_store(fdst + e, x[i]);
            }
        }
    } else {
        for (int g = tid; g < groups; g += LQ_THREADS) {
            const long e = (long)g * LQ_GROUP;
            const int c0 = (int)(e % ld);
            lq_load(fsrc + e, x[0]);
            lq_fake(x[0], s_inv + c0, s_step + c0, qmax, cur, run, hist);
            lq_store(fdst + e, x[0]);
        }
    }
    if (!counts) return;
    if (run) atomicAdd(hist + cur, run);
    __syncthreads();
    counts[f * 256 + tid] = hist[tid];
}

template <typename T>
void lq_fake_launch(const void* src, void* dst, const float* keep, unsigned* counts, int frames, int groups, int ld, int qmax, hipStream_t s)
{
    if (groups <= LQ_CACHED * LQ_THREADS)
        hipLaunchKernelGGL((latent_fake_quant_kernel<T, true>), dim3((unsigned)frames), dim3(LQ_THREADS), 0, s, (const T*)src, (T*)dst, keep,
                           counts, groups, ld, qmax);
    else
        hipLaunchKernelGGL((latent_fake_quant_kernel<T, false>), dim3((unsigned)frames), dim3(LQ_THREADS), 0, s, (const T*)src, (T*)dst, keep,
                           counts, groups, ld, qmax);
}

// ---- the rate term (quant.py: rate_reference states the arithmetic): the relaxed cost in bits of a frame's codes, and its gradient ----
// The front end both rate kernels share, which is latent_fake_quant_kernel's: the channel maxima by LDS integer atomicMax (the frame stays in
// registers when CACHED), then inv[c] = qmax / amax[c] (0 in a dead channel).  On return amax[c] holds the dead flag (1: dead) and the
// workgroup has been synchronised.
template <typename T, bool CACHED>
__device__ __forceinline__ void lr_scales(const T* __restrict__ fsrc, int groups, int ld, float qmax, float (&x)[CACHED ? LQ_CACHED : 1][LQ_GROUP],
                                          unsigned* __restrict__ amax, float* __restrict__ s_inv)
{
    const int tid = threadIdx.x;
    for (int c = tid; c < ld; c += LQ_THREADS) amax[c] = 0u;
    __syncthreads();
    if (CACHED) {
#pragma unroll
        for (int i = 0; i < LQ_CACHED; ++i) {
            const int g = tid + i * LQ_THREADS;
            if (g < groups) {
                lq_load(fsrc + (long)g * LQ_GROUP, x[i]);
                lq_max(x[i], amax + (int)(((long)g * LQ_GROUP) % ld));
            }
        }
    } else {
        for (int g = tid; g < groups; g += LQ_THREADS) {
            lq_load(fsrc + (long)g * LQ_GROUP, x[0]);
            lq_max(x[0], amax + (int)(((long)g * LQ_GROUP) % ld));
        }
    }
    __syncthreads();
    for (int c = tid; c < ld; c += LQ_THREADS) {
        const unsigned bits = amax[c];
        const float a = __uint_as_float(bits);
        const bool dead = bits >= 0x7f800000u || a < 1e-30f;
        s_inv[c] = dead ? 0.f : qmax / a;                          // the IEEE division of latent_quantise_kernel
        amax[c] = dead ? 1u : 0u;
    }
    __syncthreads();
}

// one element: v = x inv, k = clamp(floor(v), -qmax, qmax - 1), d = C[k + 129] - C[k + 128], term = C[k + 128] + (v - k) d; cost is the whole
// 256-entry table, so the two reads lie in 128 - qmax .. 128 + qmax whatever x holds.  A dead channel: term 0 (d is not used by the callers).
__device__ __forceinline__ float lr_term(float x, float inv, bool dead, float qmax, const float* __restrict__ cost, float& d)
{
    const float v = dead ? 0.f : x * inv;                          // x * 0 may be NaN
    const float kf = fminf(fmaxf(floorf(v), -qmax), qmax - 1.f);
    const int k = (int)kf;
    const float lo = cost[k + 128];
    d = cost[k + 129] - lo;
    const float t = v - kf;
    return dead ? 0.f : lo + t * d;
}

// blockIdx.x = frame; groups = hw ld / 8.  rate[f] = the sum of the frame's terms: a thread adds its own in the order it owns them, then
// wave_sum and four LDS words in a fixed order.  A dropped frame is not read: rate[f] = 0.
template <typename T, bool CACHED>
__global__ __launch_bounds__(LQ_THREADS) void latent_rate_kernel(const T* __restrict__ src, const float* __restrict__ keep,
                                                                 const float* __restrict__ cost256, float* __restrict__ rate, int groups, int ld,
                                                                 int iqmax)
{
    __shared__ unsigned amax[LQ_MAX_LD];
    __shared__ float s_inv[LQ_MAX_LD];
    __shared__ float cost[256];
    __shared__ float red[LQ_THREADS / 64];
    const long f = blockIdx.x;
    const int tid = threadIdx.x;
    if (!(keep[f] != 0.f)) {                                       // dropped or padding (uniform branch)
        if (tid == 0) rate[f] = 0.f;
        return;
    }
    const T* fsrc = src + f * (long)groups * LQ_GROUP;
    const float qmax = (float)iqmax;
    cost[tid] = cost256[tid];                                      // visible after the barriers of lr_scales
    float x[CACHED ? LQ_CACHED : 1][LQ_GROUP];
    lr_scales<T, CACHED>(fsrc, groups, ld, qmax, x, amax, s_inv);
    float sum = 0.f, d;
    if (CACHED) {
#pragma unroll
        for (int i = 0; i < LQ_CACHED; ++i) {
            const int g = tid + i * LQ_THREADS;
            if (g < groups) {
                const int c0 = (int)(((long)g * LQ_GROUP) % ld);
#pragma unroll
                for (int j = 0; j < LQ_GROUP; ++j) sum += lr_term(x[i][j], s_inv[c0 + j], amax[c0 + j] != 0u, qmax, cost, d);
            }
        }
    } else {
        for (int g = tid; g < groups; g += LQ_THREADS) {
            const long e = (long)g * LQ_GROUP;
            const int c0 = (int)(e % ld);
            lq_load(fsrc + e, x[0]);
#pragma unroll
            for (int j = 0; j < LQ_GROUP; ++j) sum += lr_term(x[0][j], s_inv[c0 + j], amax[c0 + j] != 0u, qmax, cost, d);
        }
    }
    sum = wave_sum(sum);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) rate[f] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one group of the gradient: grad = T(g * slope), slope = d inv (0 in a dead channel)
template <typename T>
__device__ __forceinline__ void lr_grad(float (&x)[LQ_GROUP], const float* __restrict__ inv, const unsigned* __restrict__ dead, float qmax,
                                        const float* __restrict__ cost, float g, T* __restrict__ dst)
{
#pragma unroll
    for (int j = 0; j < LQ_GROUP; ++j) {
        float d;
        const bool dd = dead[j] != 0u;
        lr_term(x[j], inv[j], dd, qmax, cost, d);
        const float slope = dd ? 0.f : d * inv[j];
        x[j] = g * slope;
    }
    lq_store(dst, x);
}

// blockIdx.x = frame.  grad[f, i, c] = T(gr[f] * slope); a dropped frame, or one whose gr[f] is zero, is written as zero words and src is
// not read.  Every element of grad is written.
template <typename T, bool CACHED>
__global__ __launch_bounds__(LQ_THREADS) void latent_rate_grad_kernel(const T* __restrict__ src, const float* __restrict__ keep,
                                                                      const float* __restrict__ cost256, const float* __restrict__ gr,
                                                                      T* __restrict__ grad, int groups, int ld, int iqmax)
{
    __shared__ unsigned amax[LQ_MAX_LD];
    __shared__ float s_inv[LQ_MAX_LD];
    __shared__ float cost[256];
    const long f = blockIdx.x;
    const int tid = threadIdx.x;
    const long n = (long)groups * LQ_GROUP;
    T* fdst = grad + f * n;
    const float g = gr[f];
    if (!(keep[f] != 0.f) || g == 0.f) {                           // uniform branch
        uint4* d4 = reinterpret_cast<uint4*>(fdst);
        const long words = n * (long)sizeof(T) / 16;
        for (long w = tid; w < words; w += LQ_THREADS) d4[w] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const T* fsrc = src + f * n;
    const float qmax = (float)iqmax;
    cost[tid] = cost256[tid];
    float x[CACHED ? LQ_CACHED : 1][LQ_GROUP];
    lr_scales<T, CACHED>(fsrc, groups, ld, qmax, x, amax, s_inv);
    if (CACHED) {
#pragma unroll
        for (int i = 0; i < LQ_CACHED; ++i) {
            const int gi = tid + i * LQ_THREADS;
            if (gi < groups) {
                const long e = (long)gi * LQ_GROUP;
                const int c0 = (int)(e % ld);
                lr_grad<T>(x[i], s_inv + c0, amax + c0, qmax, cost, g, fdst + e);
            }
        }
    } else {
        for (int gi = tid; gi < groups; gi += LQ_THREADS) {
            const long e = (long)gi * LQ_GROUP;
            const int c0 = (int)(e % ld);
            lq_load(fsrc + e, x[0]);
            lr_grad<T>(x[0], s_inv + c0, amax + c0, qmax, cost, g, fdst + e);
        }
    }
}

template <typename T>
void lr_launch(const void* x, const float* keep, const float* cost, float* rate, int frames, int groups, int ld, int qmax, hipStream_t s)
{
    if (groups <= LQ_CACHED * LQ_THREADS)
        hipLaunchKernelGGL((latent_rate_kernel<T, true>), dim3((unsigned)frames), dim3(LQ_THREADS), 0, s, (const T*)x, keep, cost, rate, groups, ld,
                           qmax);
    else
        hipLaunchKernelGGL((latent_rate_kernel<T, false>), dim3((unsigned)frames), dim3(LQ_THREADS), 0, s, (const T*)x, keep, cost, rate, groups,
                           ld, qmax);
}

template <typename T>
void lr_grad_launch(const void* x, const float* keep, const float* cost, const float* g, void* grad, int frames, int groups, int ld, int qmax,
                    hipStream_t s)
{
    if (groups <= LQ_CACHED * LQ_THREADS)
        hipLaunchKernelGGL((latent_rate_grad_kernel<T, true>), dim3((unsigned)frames), dim3(LQ_THREADS), 0, s, (const T*)x, keep, cost, g,
                           (T*)grad, groups, ld, qmax);
    else
        hipLaunchKernelGGL((latent_rate_grad_kernel<T, false>), dim3((unsigned)frames), dim3(LQ_THREADS), 0, s, (const T*)x, keep, cost, g,
                           (T*)grad, groups, ld, qmax);
}

}  // namespace

extern "C" int vvae_latent_quantise_supported(int hw, int ld, int dtype)
{
    return (dtype == VVAE_DT_F32 || dtype == VVAE_DT_BF16) && hw >= 1 && ld >= LQ_GROUP && ld <= LQ_MAX_LD && ld % LQ_GROUP == 0 &&
           (long)hw * ld <= LQ_MAX_FRAME;
}

// latent (frames, hw, ld) contiguous, 16-byte aligned; keep fp32 (frames,); codes int8 (frames, hw, ld), 8-byte aligned; step fp32
// (frames, ld); counts uint32 (frames, 256).  dequantise != 0: the kept frames of latent are overwritten with float(q) * step.
extern "C" int vvae_latent_quantise(void* latent, int dtype, const float* keep, int8_t* codes, float* step, unsigned* counts, int frames,
                                    int hw, int ld, int bits, int dequantise, void* stream)
{
    if (!latent || !keep || !codes || !step || !counts || frames < 1 || bits < 2 || bits > 8 || !vvae_latent_quantise_supported(hw, ld, dtype) ||
        (uintptr_t)latent % 16 || (uintptr_t)codes % 8 || (uintptr_t)keep % 4 || (uintptr_t)step % 4 || (uintptr_t)counts % 4)
        return VVAE_ERR_BAD_ARG;
    const int groups = (int)((long)hw * ld / LQ_GROUP);
    const int qmax = (1 << (bits - 1)) - 1;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == VVAE_DT_BF16) lq_launch<bf16_t>(latent, keep, codes, step, counts, frames, groups, ld, qmax, dequantise, s);
    else lq_launch<float>(latent, keep, codes, step, counts, frames, groups, ld, qmax, dequantise, s);
    VVAE_LAUNCH_CHECK();
    return 0;
}

// The quantiser inside the train step: dst (frames, hw, ld) = float(q) * step of src on the frames whose keep flag is nonzero, src's own
// bits on the others.  src and dst contiguous, 16-byte aligned, and disjoint (autograd keeps src); counts uint32 (frames, 256) or null.
// No codes and no steps leave the kernel.  The shapes are those of vvae_latent_quantise_supported.
extern "C" int vvae_latent_fake_quant(const void* src, void* dst, int dtype, const float* keep, unsigned* counts_or_null, int frames, int hw,
                                      int ld, int bits, void* stream)
{
    if (!src || !dst || !keep || frames < 1 || bits < 2 || bits > 8 || !vvae_latent_quantise_supported(hw, ld, dtype) || (uintptr_t)src % 16 ||
        (uintptr_t)dst % 16 || (uintptr_t)keep % 4 || (uintptr_t)counts_or_null % 4)
        return VVAE_ERR_BAD_ARG;
    const uintptr_t bytes = (uintptr_t)frames * hw * ld * (dtype == VVAE_DT_BF16 ? 2 : 4);
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
    if (a < b + bytes && b < a + bytes) return VVAE_ERR_BAD_ARG;   // src == dst or overlapping: the op is out of place
    const int groups = (int)((long)hw * ld / LQ_GROUP);
    const int qmax = (1 << (bits - 1)) - 1;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == VVAE_DT_BF16) lq_fake_launch<bf16_t>(src, dst, keep, counts_or_null, frames, groups, ld, qmax, s);
    else lq_fake_launch<float>(src, dst, keep, counts_or_null, frames, groups, ld, qmax, s);
    VVAE_LAUNCH_CHECK();
    return 0;
}

// The rate term of quantisation-aware training (quant.rate_reference is the definition): rate[f] = sum over the frame of the cost table
// cost256, interpolated linearly at the unrounded code x inv; 0 for a frame whose keep flag is zero.  x (frames, hw, ld) contiguous, 16-byte
// aligned, only read; keep, rate fp32 (frames,); cost256 fp32 (256,).  The shapes are those of vvae_latent_quantise_supported.
extern "C" int vvae_latent_rate(const void* x, int dtype, const float* keep, const float* cost256, float* rate, int frames, int hw, int ld,
                                int bits, void* stream)
{
    if (!x || !keep || !cost256 || !rate || frames < 1 || bits < 2 || bits > 8 || !vvae_latent_quantise_supported(hw, ld, dtype) ||
        (uintptr_t)x % 16 || (uintptr_t)keep % 4 || (uintptr_t)cost256 % 4 || (uintptr_t)rate % 4)
        return VVAE_ERR_BAD_ARG;
    const int groups = (int)((long)hw * ld / LQ_GROUP);
    const int qmax = (1 << (bits - 1)) - 1;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == VVAE_DT_BF16) lr_launch<bf16_t>(x, keep, cost256, rate, frames, groups, ld, qmax, s);
    else lr_launch<float>(x, keep, cost256, rate, frames, groups, ld, qmax, s);
    VVAE_LAUNCH_CHECK();
    return 0;
}

// Its gradient: grad[f, i, c] = g[f] * slope rounded to the dtype, slope = (C[k + 129] - C[k + 128]) inv[c] (amax and the table are
// constants); zero words for a frame whose keep flag or g[f] is zero.  grad (frames, hw, ld) of x's dtype, 16-byte aligned, disjoint from x
// (overlapping buffers: VVAE_ERR_BAD_ARG); g fp32 (frames,).  Every element of grad is written.
extern "C" int vvae_latent_rate_grad(const void* x, int dtype, const float* keep, const float* cost256, const float* g, void* grad, int frames,
                                     int hw, int ld, int bits, void* stream)
{
    if (!x || !keep || !cost256 || !g || !grad || frames < 1 || bits < 2 || bits > 8 || !vvae_latent_quantise_supported(hw, ld, dtype) ||
        (uintptr_t)x % 16 || (uintptr_t)grad % 16 || (uintptr_t)keep % 4 || (uintptr_t)cost256 % 4 || (uintptr_t)g % 4)
        return VVAE_ERR_BAD_ARG;
    const uintptr_t bytes = (uintptr_t)frames * hw * ld * (dtype == VVAE_DT_BF16 ? 2 : 4);
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)grad;
    if (a < b + bytes && b < a + bytes) return VVAE_ERR_BAD_ARG;   // the gradient is written out of place
    const int groups = (int)((long)hw * ld / LQ_GROUP);
    const int qmax = (1 << (bits - 1)) - 1;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == VVAE_DT_BF16) lr_grad_launch<bf16_t>(x, keep, cost256, g, grad, frames, groups, ld, qmax, s);
    else lr_grad_launch<float>(x, keep, cost256, g, grad, frames, groups, ld, qmax, s);
    VVAE_LAUNCH_CHECK();
    return 0;
}
