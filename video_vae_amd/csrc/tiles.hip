// Spatial tiling of frames larger than the model's square: the gather of overlapping S x S tiles out of uint8 frames, and the weighted
// blend of reconstructed tiles back into frames (video_vae_amd/tiling.py states the grid and the weights; this file computes them
// the same way).
//
// Grid, per axis of length L with tile side S and n tiles: start_i = i (L - S) / (n - 1) (integer division; 0 when n == 1).  Tile i
// covers [start_i, start_i + S); positions past L (L < S) are edge-replicated by the gather and never read by the blend.  Weight of tile
// i at in-tile position p: 1, times min(1, (p + 0.5) / r) with r = end_{i-1} - start_i when that overlap is positive, times
// min(1, (S - p - 0.5) / r) with r = end_i - start_{i+1} likewise.  2D weight = w_y w_x; output = sum_k w_k tile_k / sum_k w_k over the
// covering tiles in ascending k = ty nx + tx.
//
// tile_gather_kernel: each thread writes 4 consecutive fp32 of a tile row (S C values) with one 16-B store.  Inside the frame a tile row
// is a contiguous byte run, read as one (aligned) or two dwords per thread; edge tiles clamp every source index.  Bytes are converted
// through a 256-entry table in LDS (the caller's exact u8 -> fp32 values).
// tile_blend_kernel: each thread owns 4 consecutive values of an output row (W C values) and loops over its covering tiles in fixed
// order with fp32 accumulation; every output word is written once, no atomics, no memset.
//
// Temporal windows (WindowPlan in tiling.py): the same grid arithmetic on the time axis, a clip of L frames in windows of F frames that
// overlap by at least o_t (L <= F: one window at 0).  Weight of (window w, tile (ty, tx)) at in-window frame q and in-tile (py, px):
// (w_t(w, q) w_y(ty, py)) w_x(tx, px), products in that order; out = sum weight tile / sum weight over the covering (w, ty, tx) in
// ascending order, fp32.  With w_t = 1 (a frame one window covers) the products and sums are exactly tile_blend_kernel's.
// window_blend_kernel: one workgroup per (output row (f, y), 1024 values of it).  The temporal and vertical cover of the row and the
// weights w_t w_y of its (window, ty) pairs are formed once per workgroup into LDS; each thread owns 4 consecutive values of the row,
// finds their horizontal cover and weights once, and sums the pairs in order.  Every word of frames [f_lo, f_hi) is written once.
#include "common.hpp"

namespace {

constexpr int TG_THREADS = 256;
constexpr int TG_QUADS = 4;                  // quads (4 output floats) per thread in the gather
constexpr int TB_THREADS = 256;
constexpr int TILE_MAX_SIDE = 16384;         // frame height and width
constexpr int WB_THREADS = 256;
constexpr int WB_MAXC = 4;                   // windows / tiles covering one position of an axis, at most (checked on the host)

struct TileDims {
    int N, T, H, W, C, S, ny, nx;
};

// 32-bit unsigned arithmetic: L <= TILE_MAX_SIDE keeps i (L - S) and p (n - 1) below 2^28 (a 64-bit division costs ~10x more)
__host__ __device__ __forceinline__ int tile_start(int i, int L, int S, int n)
{
    return n > 1 ? (int)((unsigned)(i * (L - S)) / (unsigned)(n - 1)) : 0;
}

// tiles [lo, hi] on one axis that cover position p (0 <= p < L)
__device__ __forceinline__ void tile_cover(int p, int L, int S, int n, int& lo, int& hi)
{
    int i = n > 1 ? min(n - 1, (int)((unsigned)(p * (n - 1)) / (unsigned)(L - S))) : 0;     // start_i <= p
    while (i + 1 < n && tile_start(i + 1, L, S, n) <= p) ++i;
    hi = i;
    while (i > 0 && tile_start(i - 1, L, S, n) + S > p) --i;
    lo = i;
}

__device__ __forceinline__ float tile_weight(int i, int q, int L, int S, int n)
{
    const int s = tile_start(i, L, S, n);
    float w = 1.f;
    if (i > 0) {
        const int r = tile_start(i - 1, L, S, n) + S - s;
        if (r > 0) w *= fminf(1.f, ((float)q + 0.5f) / (float)r);
    }
    if (i < n - 1) {
        const int r = s + S - tile_start(i + 1, L, S, n);
        if (r > 0) w *= fminf(1.f, ((float)(S - q) - 0.5f) / (float)r);
    }
    return w;
}

// src uint8 (N, T, H, W, C); dst fp32 (count, T, S, S, C), tile j of dst = flat tile first + j (flat = n ny nx + ty nx + tx)
__global__ __launch_bounds__(TG_THREADS) void tile_gather_kernel(const uint8_t* __restrict__ src, const float* __restrict__ lut,
                                                                 float* __restrict__ dst, TileDims d, int first, long quads, long src_bytes)
{
    __shared__ float tab[256];
    tab[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int rq = d.S * d.C / 4;                                  // quads per tile row
    const int K = d.ny * d.nx;
    for (int u = 0; u < TG_QUADS; ++u) {
        const long q = ((long)blockIdx.x * TG_QUADS + u) * TG_THREADS + threadIdx.x;
        if (q >= quads) return;
        const long row = q / rq;
        const int e = (int)(q - row * rq) * 4;
        const int r = (int)(row % d.S);
        const long tt = row / d.S;
        const int t = (int)(tt % d.T);
        const int flat = first + (int)(tt / d.T);
        const int n = flat / K, k = flat - n * K, ty = k / d.nx, tx = k - ty * d.nx;
        const int y0 = tile_start(ty, d.H, d.S, d.ny), x0 = tile_start(tx, d.W, d.S, d.nx);
        const int ys = min(y0 + r, d.H - 1);
        const long base = (((long)n * d.T + t) * d.H + ys) * d.W * d.C;
        uint32_t b4;
        if (x0 + d.S <= d.W) {                                     // the whole tile row lies in the frame: one contiguous run
            const long a = base + (long)x0 * d.C + e;
            const long al = a & ~3L;
            const int sh = (int)(a - al) * 8;
            const uint32_t lo = *reinterpret_cast<const uint32_t*>(src + al);
            if (sh == 0) b4 = lo;
            else if (al + 8 <= src_bytes) {
                const uint32_t hi = *reinterpret_cast<const uint32_t*>(src + al + 4);
                b4 = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
            } else {
                b4 = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) b4 |= (uint32_t)src[a + i] << (8 * i);
            }
        } else {                                                   // edge tile: clamp every column
            b4 = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int el = e + i, j = el / d.C, c = el - j * d.C;
                b4 |= (uint32_t)src[base + (long)min(x0 + j, d.W - 1) * d.C + c] << (8 * i);
            }
        }
        const float v[4] = {tab[b4 & 255], tab[(b4 >> 8) & 255], tab[(b4 >> 16) & 255], tab[b4 >> 24]};
        VecIO<float, 4>::store(dst + q * 4, v);
    }
}

// tiles (N ny nx, T, S, S, C) fp32 / bf16 -> out fp32 (N, T, H, W, C)
template <typename TT>
__global__ __launch_bounds__(TB_THREADS) void tile_blend_kernel(const TT* __restrict__ tiles, float* __restrict__ out, TileDims d, long quads,
                                                                int vec_store)
{
    const long q = (long)blockIdx.x * TB_THREADS + threadIdx.x;
    if (q >= quads) return;
    const int L = d.W * d.C, rq = (L + 3) / 4;
    const long row = q / rq;
    const int e0 = (int)(q - row * rq) * 4;
    const int y = (int)(row % d.H);
    const long nt = row / d.H;
    const int t = (int)(nt % d.T), n = (int)(nt / d.T);
    int ylo, yhi;
    tile_cover(y, d.H, d.S, d.ny, ylo, yhi);
    const long tstride = (long)d.T * d.S * d.S * d.C;              // one tile
    const TT* tbase = tiles + ((long)n * d.ny * d.nx) * tstride + (long)t * d.S * d.S * d.C;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int el = e0 + i;
        v[i] = 0.f;
        if (el >= L) continue;
        const int x = el / d.C, c = el - x * d.C;
        int xlo, xhi;
        tile_cover(x, d.W, d.S, d.nx, xlo, xhi);
        float num = 0.f, den = 0.f;
        for (int ty = ylo; ty <= yhi; ++ty) {
            const int py = y - tile_start(ty, d.H, d.S, d.ny);
            const float wy = tile_weight(ty, py, d.H, d.S, d.ny);
            for (int tx = xlo; tx <= xhi; ++tx) {
                const int px = x - tile_start(tx, d.W, d.S, d.nx);
                const float w = wy * tile_weight(tx, px, d.W, d.S, d.nx);
                const float s = ldf(tbase + (long)(ty * d.nx + tx) * tstride + ((long)py * d.S + px) * d.C + c);
                num = fmaf(w, s, num);
                den += w;
            }
        }
        v[i] = num / den;
    }
    float* o = out + row * L + e0;
    if (vec_store) VecIO<float, 4>::store(o, v);
    else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (e0 + i < L) o[i] = v[i];
    }
}

struct WinDims {
    int L, F, nw, ring, f_lo;                // clip length, window length, windows, ring slots, first output frame
    int H, W, C, S, ny, nx;
};

// tiles (ring, ny nx, F, S, S, C) fp32 / bf16, window w in slot w % ring -> out fp32 (L, H, W, C), rows of frames [f_lo, f_hi)
template <typename TT>
__global__ __launch_bounds__(WB_THREADS) void window_blend_kernel(const TT* __restrict__ tiles, float* __restrict__ out, WinDims d,
                                                                  int vec_store)
{
    __shared__ long poff[WB_MAXC * WB_MAXC];                       // (window, ty) pair: element offset of its tile row (tx = 0)
    __shared__ float pw[WB_MAXC * WB_MAXC];                        // its weight w_t w_y
    __shared__ int npair;
    const long row = blockIdx.x;                                   // (f - f_lo) H + y
    const int f = d.f_lo + (int)(row / d.H), y = (int)(row % d.H);
    const long tstride = (long)d.F * d.S * d.S * d.C;              // one tile
    if (threadIdx.x < WB_MAXC * WB_MAXC) {
        int wlo, whi, ylo, yhi;
        tile_cover(f, d.L, d.F, d.nw, wlo, whi);
        tile_cover(y, d.H, d.S, d.ny, ylo, yhi);
        const int a = threadIdx.x / WB_MAXC, b = threadIdx.x % WB_MAXC, nyc = yhi - ylo + 1;
        if (threadIdx.x == 0) npair = (whi - wlo + 1) * nyc;
        if (wlo + a <= whi && ylo + b <= yhi) {
            const int w = wlo + a, ty = ylo + b;
            const int q = f - tile_start(w, d.L, d.F, d.nw), py = y - tile_start(ty, d.H, d.S, d.ny);
            const float wt = tile_weight(w, q, d.L, d.F, d.nw);
            pw[a * nyc + b] = wt * tile_weight(ty, py, d.H, d.S, d.ny);
            poff[a * nyc + b] = ((long)(w % d.ring) * d.ny * d.nx + (long)ty * d.nx) * tstride + ((long)q * d.S + py) * d.S * d.C;
        }
    }
    __syncthreads();
    const int L = d.W * d.C;
    const int e0 = (blockIdx.y * WB_THREADS + threadIdx.x) * 4;
    if (e0 >= L) return;
    const int np = npair;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int el = e0 + i;
        v[i] = 0.f;
        if (el >= L) continue;
        const int x = el / d.C, c = el - x * d.C;
        int xlo, xhi;
        tile_cover(x, d.W, d.S, d.nx, xlo, xhi);
        float wx[WB_MAXC];
        long xo[WB_MAXC];
#pragma unroll
        for (int j = 0; j < WB_MAXC; ++j) {
            const int tx = min(xlo + j, xhi);
            const int px = x - tile_start(tx, d.W, d.S, d.nx);
            wx[j] = tile_weight(tx, px, d.W, d.S, d.nx);
            xo[j] = (long)tx * tstride + (long)px * d.C + c;
        }
        float num = 0.f, den = 0.f;
        for (int p = 0; p < np; ++p) {
            const float wp = pw[p];
            const TT* base = tiles + poff[p];
#pragma unroll
            for (int j = 0; j < WB_MAXC; ++j) {
                if (xlo + j > xhi) break;
                const float w = wp * wx[j];
                const float s = ldf(base + xo[j]);
                num = fmaf(w, s, num);
                den += w;
            }
        }
        v[i] = num / den;
    }
    float* o = out + ((long)f * d.H + y) * L + e0;
    if (vec_store) VecIO<float, 4>::store(o, v);
    else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (e0 + i < L) o[i] = v[i];
    }
}

// the most tiles covering one position of an axis (starts ascending: count the starts in [start_i, start_i + S))
int axis_max_cover(int L, int S, int n)
{
    int best = 1;
    for (int i = 0, j = 0; i < n; ++i) {
        const int s = tile_start(i, L, S, n);
        if (j < i) j = i;
        while (j + 1 < n && tile_start(j + 1, L, S, n) < s + S) ++j;
        best = best > j - i + 1 ? best : j - i + 1;
    }
    return best;
}

int tiles_per_axis(int L, int S, int o)
{
    return L <= S ? 1 : (L - o + (S - o) - 1) / (S - o);
}

bool tile_dims(int N, int T, int H, int W, int C, int S, int overlap, int ny, int nx, TileDims& d)
{
    if (N <= 0 || T <= 0 || H <= 0 || W <= 0 || H > TILE_MAX_SIDE || W > TILE_MAX_SIDE || C < 1 || C > 4 || S <= 0 || overlap < 0 || overlap > S / 2) return false;
    if (ny != tiles_per_axis(H, S, overlap) || nx != tiles_per_axis(W, S, overlap)) return false;
    if ((long)N * ny * nx > (1L << 30) || (long)N * T * H > (1L << 40)) return false;
    d.N = N; d.T = T; d.H = H; d.W = W; d.C = C; d.S = S; d.ny = ny; d.nx = nx;
    return true;
}

}  // namespace

extern "C" int vvae_tile_gather_supported(int H, int W, int C, int S, int overlap)
{
    TileDims d;
    return (S * C) % 4 == 0 &&
           tile_dims(1, 1, H, W, C, S, overlap, tiles_per_axis(H, S, overlap), tiles_per_axis(W, S, overlap), d);
}

// src uint8 (N, T, H, W, C) contiguous; lut fp32 [256] (the value of each byte); dst fp32 (count, T, S, S, C), 16-B aligned: the tiles
// first .. first + count - 1 of the flat (window, ty, tx) order.
extern "C" int vvae_tile_gather_u8(const void* src, const float* lut, float* dst, int N, int T, int H, int W, int C, int S, int overlap,
                                   int ny, int nx, int first, int count, void* stream)
{
    TileDims d;
    if (!src || !lut || !dst || !vvae_tile_gather_supported(H, W, C, S, overlap) || !tile_dims(N, T, H, W, C, S, overlap, ny, nx, d) ||
        first < 0 || count <= 0 || (long)first + count > (long)N * ny * nx || (uintptr_t)dst % 16 || (uintptr_t)lut % 4)
        return VVAE_ERR_BAD_ARG;
    const long quads = (long)count * T * S * S * C / 4;
    const long per = (long)TG_THREADS * TG_QUADS;
    const long blocks = (quads + per - 1) / per;
    if (blocks > 0x7fffffffL) return VVAE_ERR_BAD_ARG;
    hipLaunchKernelGGL(tile_gather_kernel, dim3((unsigned)blocks), dim3(TG_THREADS), 0, (hipStream_t)stream, (const uint8_t*)src, lut, dst, d,
                       first, quads, (long)N * T * H * W * C);
    VVAE_LAUNCH_CHECK();
    return 0;
}

extern "C" int vvae_tile_blend_supported(int H, int W, int C, int S, int overlap, int dtype)
{
    TileDims d;
    return (dtype == VVAE_DT_F32 || dtype == VVAE_DT_BF16) &&
           tile_dims(1, 1, H, W, C, S, overlap, tiles_per_axis(H, S, overlap), tiles_per_axis(W, S, overlap), d);
}

// tiles (N ny nx, T, S, S, C) contiguous, dtype VVAE_DT_F32 / VVAE_DT_BF16 -> out fp32 (N, T, H, W, C) contiguous, every word written.
extern "C" int vvae_tile_blend(const void* tiles, int dtype, float* out, int N, int T, int H, int W, int C, int S, int overlap, int ny, int nx,
                               void* stream)
{
    TileDims d;
    if (!tiles || !out || !vvae_tile_blend_supported(H, W, C, S, overlap, dtype) || !tile_dims(N, T, H, W, C, S, overlap, ny, nx, d) ||
        (uintptr_t)tiles % (dtype == VVAE_DT_F32 ? 4 : 2) || (uintptr_t)out % 4)
        return VVAE_ERR_BAD_ARG;
    const int L = W * C;
    const long quads = (long)N * T * H * ((L + 3) / 4);
    const long blocks = (quads + TB_THREADS - 1) / TB_THREADS;
    if (blocks > 0x7fffffffL) return VVAE_ERR_BAD_ARG;
    const int vec = L % 4 == 0 && (uintptr_t)out % 16 == 0;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == VVAE_DT_F32)
        hipLaunchKernelGGL(tile_blend_kernel<float>, dim3((unsigned)blocks), dim3(TB_THREADS), 0, s, (const float*)tiles, out, d, quads, vec);
    else
        hipLaunchKernelGGL(tile_blend_kernel<bf16_t>, dim3((unsigned)blocks), dim3(TB_THREADS), 0, s, (const bf16_t*)tiles, out, d, quads, vec);
    VVAE_LAUNCH_CHECK();
    return 0;
}

extern "C" int vvae_window_blend_supported(int L, int frames, int t_overlap, int H, int W, int C, int S, int overlap, int dtype)
{
    TileDims d;
    if (L <= 0 || frames <= 0 || t_overlap < 0 || t_overlap > frames / 2 || L > TILE_MAX_SIDE ||
        !vvae_tile_blend_supported(H, W, C, S, overlap, dtype) ||
        !tile_dims(1, frames, H, W, C, S, overlap, tiles_per_axis(H, S, overlap), tiles_per_axis(W, S, overlap), d))
        return 0;
    return axis_max_cover(L, frames, tiles_per_axis(L, frames, t_overlap)) <= WB_MAXC &&
           axis_max_cover(H, S, d.ny) <= WB_MAXC && axis_max_cover(W, S, d.nx) <= WB_MAXC;
}

// tiles (ring, ny nx, frames, S, S, C) contiguous, dtype VVAE_DT_F32 / VVAE_DT_BF16, window w in slot w % ring -> out fp32 (L, H, W, C)
// contiguous, frames [f_lo, f_hi) written (every word), no other word touched.  The windows covering [f_lo, f_hi) must fit the ring.
extern "C" int vvae_window_blend(const void* tiles, int dtype, int ring, float* out, int L, int frames, int t_overlap, int n_windows, int f_lo,
                                 int f_hi, int H, int W, int C, int S, int overlap, int ny, int nx, void* stream)
{
    TileDims td;
    if (!tiles || !out || ring < 1 || !vvae_window_blend_supported(L, frames, t_overlap, H, W, C, S, overlap, dtype) ||
        !tile_dims(1, frames, H, W, C, S, overlap, ny, nx, td) || n_windows != tiles_per_axis(L, frames, t_overlap) ||
        f_lo < 0 || f_lo >= f_hi || f_hi > L || (uintptr_t)tiles % (dtype == VVAE_DT_F32 ? 4 : 2) || (uintptr_t)out % 4)
        return VVAE_ERR_BAD_ARG;
    // windows covering [f_lo, f_hi): start < f_hi and start + frames > f_lo; they must be at most `ring` consecutive ones
    int wlo = n_windows, whi = -1;
    for (int w = 0; w < n_windows; ++w) {
        const int s = tile_start(w, L, frames, n_windows);
        if (s < f_hi && s + frames > f_lo) { wlo = wlo < w ? wlo : w; whi = w; }
    }
    if (whi < wlo || whi - wlo + 1 > ring) return VVAE_ERR_BAD_ARG;
    if ((long)ring * ny * nx * frames * S > (1L << 40)) return VVAE_ERR_BAD_ARG;
    const int rowlen = W * C;
    const long rows = (long)(f_hi - f_lo) * H;
    const int chunks = (rowlen + 4 * WB_THREADS - 1) / (4 * WB_THREADS);
    if (rows > 0x7fffffffL) return VVAE_ERR_BAD_ARG;
    WinDims d{L, frames, n_windows, ring, f_lo, H, W, C, S, ny, nx};
    const int vec = rowlen % 4 == 0 && (uintptr_t)out % 16 == 0;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == VVAE_DT_F32)
        hipLaunchKernelGGL(window_blend_kernel<float>, dim3((unsigned)rows, (unsigned)chunks), dim3(WB_THREADS), 0, s, (const float*)tiles, out,
                           d, vec);
    else
        hipLaunchKernelGGL(window_blend_kernel<bf16_t>, dim3((unsigned)rows, (unsigned)chunks), dim3(WB_THREADS), 0, s, (const bf16_t*)tiles,
                           out, d, vec);
    VVAE_LAUNCH_CHECK();
    return 0;
}
