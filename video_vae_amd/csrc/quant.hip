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
// Four kernels <T, CACHED>, one workgroup of 256 threads per frame each, on one front end (lq_scales) and one frame loop (lq_groups).  A
// thread owns groups of 8 consecutive elements (16 bytes of bf16, two 16-byte loads of fp32; ld is a multiple of 8, so a group lies in
// one token and its channels are c0 .. c0 + 7), group g = tid + 256 i.  CACHED (at most 12 groups per thread: the production frame
// 256 x 96 is exactly 12): the frame is loaded once and stays in registers between the max pass and the second pass; otherwise the second
// pass reads the frame again (still in L2).  The channel maxima and the histogram are LDS integer atomics that stay inside the workgroup;
// a thread adds a run of equal codes at once (scenes.hip's trick), so a flat frame costs one LDS add per thread.
//   latent_quantise_kernel    codes, steps and counts for inference.  A frame whose keep flag is zero is not read: its latent stays as it
//                             is, its codes, steps and counts are written as zeros.
//   latent_fake_quant_kernel  its out-of-place form for the train step: no codes and no steps leave the kernel.
//   latent_rate_kernel, latent_rate_grad_kernel (quant.py: rate_reference)  price the unrounded codes under a 256-entry cost table and
//                             give the gradient of that price.
// Every output element is written by every launch: no global atomics, no float atomics, no memset, no workspace; bitwise reproducible;
// safe inside a captured hipGraph.
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

// The frame loop: a thread's groups in the order it owns them, each handed to f(x, e, c0) with x its 8 values, e its first element and
// c0 = e % ld its first channel.  CACHED: unrolled over the LQ_CACHED groups in registers, which the FIRST pass loads and the later ones
// find there; otherwise strided, and every pass loads the group into x[0].
template <bool CACHED, bool FIRST, typename T, typename F>
__device__ __forceinline__ void lq_groups(const T* fsrc, int groups, int ld, float (&x)[CACHED ? LQ_CACHED : 1][LQ_GROUP], F f)
{
    const int tid = threadIdx.x;
    if (CACHED) {
#pragma unroll
        for (int i = 0; i < LQ_CACHED; ++i) {
            const int g = tid + i * LQ_THREADS;
            if (g < groups) {
                const long e = (long)g * LQ_GROUP;
                if (FIRST) lq_load(fsrc + e, x[i]);
                f(x[i], e, (int)(e % ld));
            }
        }
    } else {
        for (int g = tid; g < groups; g += LQ_THREADS) {
            const long e = (long)g * LQ_GROUP;
            lq_load(fsrc + e, x[0]);
            f(x[0], e, (int)(e % ld));
        }
    }
}

// What a kernel wants of the front end beside s_inv: nothing (the rate kernels, which find the dead flag in amax), the steps in s_step and a
// cleared hist (the training form), or these and the global step row fstep (inference).  A template argument and not a null pointer: a
// test of an LDS or of a computed global pointer against null stays in the machine code.
enum LqWant { LQ_INV, LQ_STEP, LQ_STEP_ROW };

// The front end of all four kernels: amax (and hist) cleared, the channel maxima by LDS integer atomicMax over the FIRST pass of the frame
// loop, then per channel the dead rule and s_inv[c] = qmax / amax[c], step[c] = amax[c] / qmax (both 0 in a dead channel): the step of
// the file format is defined HERE, for what training sees and for what infer writes alike.  LQ_INV: no step is formed, and on return
// amax[c] holds the dead flag (1: dead).  The workgroup has been synchronised on return.
template <typename T, bool CACHED, LqWant WANT>
__device__ __forceinline__ void lq_scales(const T* fsrc, int groups, int ld, float qmax, float (&x)[CACHED ? LQ_CACHED : 1][LQ_GROUP],
                                          unsigned* __restrict__ amax, float* __restrict__ s_inv, float* __restrict__ s_step,
                                          float* __restrict__ fstep, unsigned* __restrict__ hist)
{
    const int tid = threadIdx.x;
    for (int c = tid; c < ld; c += LQ_THREADS) amax[c] = 0u;
    if (WANT != LQ_INV) hist[tid] = 0u;
    __syncthreads();
    lq_groups<CACHED, true>(fsrc, groups, ld, x, [&](const float (&v)[LQ_GROUP], long, int c0) {
#pragma unroll
        for (int j = 0; j < LQ_GROUP; ++j) atomicMax(amax + c0 + j, __float_as_uint(v[j]) & 0x7fffffffu);
    });
    __syncthreads();
    for (int c = tid; c < ld; c += LQ_THREADS) {
        const unsigned bits = amax[c];
        const float a = __uint_as_float(bits);
        const bool dead = bits >= 0x7f800000u || a < 1e-30f;
        s_inv[c] = dead ? 0.f : qmax / a;                          // IEEE divisions (hipcc's default fp32 division is correctly rounded)
        if (WANT == LQ_INV) {
            amax[c] = dead ? 1u : 0u;
        } else {
            const float st = dead ? 0.f : a / qmax;
            s_step[c] = st;
            if (WANT == LQ_STEP_ROW) fstep[c] = st;
        }
    }
    __syncthreads();
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

// blockIdx.x = frame; groups = hw ld / 8.  The kept frames' 8 codes per group are stored as two words, and the dequantised values over the
// latent when asked for.
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
    T* src = latent + f * n;
    const float qmax = (float)iqmax;
    float x[CACHED ? LQ_CACHED : 1][LQ_GROUP];
    lq_scales<T, CACHED, LQ_STEP_ROW>(src, groups, ld, qmax, x, amax, s_inv, s_step, fstep, hist);
    const bool deq = dequantise != 0;                              // formed once: a test of the int inside the loop compiles to other code
    int cur = 128;
    unsigned run = 0;
    lq_groups<CACHED, false>(src, groups, ld, x, [&](float (&v)[LQ_GROUP], long e, int c0) {
        uint32_t w[2] = {0u, 0u};
#pragma unroll
        for (int j = 0; j < LQ_GROUP; ++j) {
            const int q = lq_code(v[j], s_inv[c0 + j], s_step[c0 + j], qmax, cur, run, hist);
            w[j >> 2] |= ((uint32_t)q & 0xffu) << (8 * (j & 3));
        }
        *reinterpret_cast<uint2*>(fcodes + e) = make_uint2(w[0], w[1]);
        if (deq) lq_store(src + e, v);
    });
    if (run) atomicAdd(hist + cur, run);
    __syncthreads();
    fcounts[tid] = hist[tid];
}

// The training form (quantisation-aware training): dst = the dequantised src on kept frames, src itself on the others.  Out of place: src
// is only read, every element of dst is written (a dropped frame as 16-byte words, so its bits pass whatever they encode).  counts may be
// null: then no histogram leaves the workgroup.
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
    const float qmax = (float)iqmax;
    float x[CACHED ? LQ_CACHED : 1][LQ_GROUP];
    lq_scales<T, CACHED, LQ_STEP>(fsrc, groups, ld, qmax, x, amax, s_inv, s_step, nullptr, hist);
    int cur = 128;
    unsigned run = 0;
    lq_groups<CACHED, false>(fsrc, groups, ld, x, [&](float (&v)[LQ_GROUP], long e, int c0) {
#pragma unroll
        for (int j = 0; j < LQ_GROUP; ++j) lq_code(v[j], s_inv[c0 + j], s_step[c0 + j], qmax, cur, run, hist);
        lq_store(fdst + e, v);
    });
    if (!counts) return;
    if (run) atomicAdd(hist + cur, run);
    __syncthreads();
    counts[f * 256 + tid] = hist[tid];
}

// ---- the rate term (quant.py: rate_reference states the arithmetic): the relaxed cost in bits of a frame's codes, and its gradient ----
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
    cost[tid] = cost256[tid];                                      // visible after the barriers of lq_scales
    float x[CACHED ? LQ_CACHED : 1][LQ_GROUP];
    lq_scales<T, CACHED, LQ_INV>(fsrc, groups, ld, qmax, x, amax, s_inv, nullptr, nullptr, nullptr);
    float sum = 0.f;
    lq_groups<CACHED, false>(fsrc, groups, ld, x, [&](const float (&v)[LQ_GROUP], long, int c0) {
        float d;
#pragma unroll
        for (int j = 0; j < LQ_GROUP; ++j) sum += lr_term(v[j], s_inv[c0 + j], amax[c0 + j] != 0u, qmax, cost, d);
    });
    sum = wave_sum(sum);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) rate[f] = (red[0] + red[1]) + (red[2] + red[3]);
}

// blockIdx.x = frame.  grad[f, i, c] = T(gr[f] * slope), slope = d inv (0 in a dead channel); a dropped frame, or one whose gr[f] is zero,
// is written as zero words and src is not read.  Every element of grad is written.
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
    lq_scales<T, CACHED, LQ_INV>(fsrc, groups, ld, qmax, x, amax, s_inv, nullptr, nullptr, nullptr);
    lq_groups<CACHED, false>(fsrc, groups, ld, x, [&](float (&v)[LQ_GROUP], long e, int c0) {
#pragma unroll
        for (int j = 0; j < LQ_GROUP; ++j) {
            float d;
            const bool dead = amax[c0 + j] != 0u;
            lr_term(v[j], s_inv[c0 + j], dead, qmax, cost, d);
            v[j] = g * (dead ? 0.f : d * s_inv[c0 + j]);
        }
        lq_store(fdst + e, v);
    });
}

bool lq_shape_ok(int hw, int ld, int dtype)
{
    return (dtype == VVAE_DT_F32 || dtype == VVAE_DT_BF16) && hw >= 1 && ld >= LQ_GROUP && ld <= LQ_MAX_LD && ld % LQ_GROUP == 0 &&
           (long)hw * ld <= LQ_MAX_FRAME;
}

// What the four entries check and derive alike: frames >= 1, bits in 2 .. 8 and a shape the kernels take, or ok is false; then
// groups = hw ld / 8 and qmax = 2^(bits - 1) - 1.
struct LqArgs {
    bool ok;
    int groups, qmax;
};
LqArgs lq_args(int dtype, int frames, int hw, int ld, int bits)
{
    if (frames < 1 || bits < 2 || bits > 8 || !lq_shape_ok(hw, ld, dtype)) return {false, 0, 0};
    return {true, (int)((long)hw * ld / LQ_GROUP), (1 << (bits - 1)) - 1};
}

// a pointer that is given and a multiple of `to` bytes
bool lq_aligned(const void* p, unsigned to) { return p && (uintptr_t)p % to == 0; }

// two (frames, hw, ld) buffers of dtype that share no byte: the out-of-place entries refuse a == b and every overlap
bool lq_disjoint(const void* pa, const void* pb, int dtype, int frames, int hw, int ld)
{
    const uintptr_t bytes = (uintptr_t)frames * hw * ld * (dtype == VVAE_DT_BF16 ? 2 : 4);
    const uintptr_t a = (uintptr_t)pa, b = (uintptr_t)pb;
    return !(a < b + bytes && b < a + bytes);
}

}  // namespace

// The one launch: KERNEL<T, CACHED> with T from dtype (the arguments name it) and CACHED from the frame's size, one workgroup per frame on
// `stream`.  It reads the entry's dtype, frames, stream and its LqArgs a.
#define LQ_LAUNCH(KERNEL, ...)                                                                                                    \
    do {                                                                                                                          \
        const dim3 grid((unsigned)frames), block(LQ_THREADS);                                                                     \
        hipStream_t s = (hipStream_t)stream;                                                                                      \
        const bool cached = a.groups <= LQ_CACHED * LQ_THREADS;                                                                   \
        if (dtype == VVAE_DT_BF16) {                                                                                              \
            typedef bf16_t T;                                                                                                     \
            if (cached) hipLaunchKernelGGL((KERNEL<T, true>), grid, block, 0, s, __VA_ARGS__);                                    \
            else hipLaunchKernelGGL((KERNEL<T, false>), grid, block, 0, s, __VA_ARGS__);                                          \
        } else {                                                                                                                  \
            typedef float T;                                                                                                      \
            if (cached) hipLaunchKernelGGL((KERNEL<T, true>), grid, block, 0, s, __VA_ARGS__);                                    \
            else hipLaunchKernelGGL((KERNEL<T, false>), grid, block, 0, s, __VA_ARGS__);                                          \
        }                                                                                                                         \
    } while (0)

extern "C" int vvae_latent_quantise_supported(int hw, int ld, int dtype) { return lq_shape_ok(hw, ld, dtype); }

// latent (frames, hw, ld) contiguous, 16-byte aligned; keep fp32 (frames,); codes int8 (frames, hw, ld), 8-byte aligned; step fp32
// (frames, ld); counts uint32 (frames, 256).  dequantise != 0: the kept frames of latent are overwritten with float(q) * step.
extern "C" int vvae_latent_quantise(void* latent, int dtype, const float* keep, int8_t* codes, float* step, unsigned* counts, int frames,
                                    int hw, int ld, int bits, int dequantise, void* stream)
{
    const LqArgs a = lq_args(dtype, frames, hw, ld, bits);
    if (!a.ok || !lq_aligned(latent, 16) || !lq_aligned(codes, 8) || !lq_aligned(keep, 4) || !lq_aligned(step, 4) || !lq_aligned(counts, 4))
        return VVAE_ERR_BAD_ARG;
    LQ_LAUNCH(latent_quantise_kernel, (T*)latent, keep, codes, step, counts, a.groups, ld, a.qmax, dequantise);
    VVAE_LAUNCH_CHECK();
    return 0;
}

// The quantiser inside the train step: dst (frames, hw, ld) = float(q) * step of src on the frames whose keep flag is nonzero, src's own
// bits on the others.  src and dst contiguous, 16-byte aligned, and disjoint (autograd keeps src); counts uint32 (frames, 256) or null.
// No codes and no steps leave the kernel.  The shapes are those of vvae_latent_quantise_supported.
extern "C" int vvae_latent_fake_quant(const void* src, void* dst, int dtype, const float* keep, unsigned* counts_or_null, int frames, int hw,
                                      int ld, int bits, void* stream)
{
    const LqArgs a = lq_args(dtype, frames, hw, ld, bits);
    if (!a.ok || !lq_aligned(src, 16) || !lq_aligned(dst, 16) || !lq_aligned(keep, 4) || (counts_or_null && !lq_aligned(counts_or_null, 4)) ||
        !lq_disjoint(src, dst, dtype, frames, hw, ld))
        return VVAE_ERR_BAD_ARG;
    LQ_LAUNCH(latent_fake_quant_kernel, (const T*)src, (T*)dst, keep, counts_or_null, a.groups, ld, a.qmax);
    VVAE_LAUNCH_CHECK();
    return 0;
}

// The rate term of quantisation-aware training (quant.rate_reference is the definition): rate[f] = sum over the frame of the cost table
// cost256, interpolated linearly at the unrounded code x inv; 0 for a frame whose keep flag is zero.  x (frames, hw, ld) contiguous, 16-byte
// aligned, only read; keep, rate fp32 (frames,); cost256 fp32 (256,).  The shapes are those of vvae_latent_quantise_supported.
extern "C" int vvae_latent_rate(const void* x, int dtype, const float* keep, const float* cost256, float* rate, int frames, int hw, int ld,
                                int bits, void* stream)
{
    const LqArgs a = lq_args(dtype, frames, hw, ld, bits);
    if (!a.ok || !lq_aligned(x, 16) || !lq_aligned(keep, 4) || !lq_aligned(cost256, 4) || !lq_aligned(rate, 4)) return VVAE_ERR_BAD_ARG;
    LQ_LAUNCH(latent_rate_kernel, (const T*)x, keep, cost256, rate, a.groups, ld, a.qmax);
    VVAE_LAUNCH_CHECK();
    return 0;
}

// Its gradient: grad[f, i, c] = g[f] * slope rounded to the dtype, slope = (C[k + 129] - C[k + 128]) inv[c] (amax and the table are
// constants); zero words for a frame whose keep flag or g[f] is zero.  grad (frames, hw, ld) of x's dtype, 16-byte aligned, disjoint from x
// (overlapping buffers: VVAE_ERR_BAD_ARG); g fp32 (frames,).  Every element of grad is written.
extern "C" int vvae_latent_rate_grad(const void* x, int dtype, const float* keep, const float* cost256, const float* g, void* grad, int frames,
                                     int hw, int ld, int bits, void* stream)
{
    const LqArgs a = lq_args(dtype, frames, hw, ld, bits);
    if (!a.ok || !lq_aligned(x, 16) || !lq_aligned(grad, 16) || !lq_aligned(keep, 4) || !lq_aligned(cost256, 4) || !lq_aligned(g, 4) ||
        !lq_disjoint(x, grad, dtype, frames, hw, ld))
        return VVAE_ERR_BAD_ARG;
    LQ_LAUNCH(latent_rate_grad_kernel, (const T*)x, keep, cost256, g, (T*)grad, a.groups, ld, a.qmax);
    VVAE_LAUNCH_CHECK();
    return 0;
}
