// Interleaved rANS over the quantiser's codes (video_vae_amd/entropy.py: encode_reference / decode_reference state the format; this file
// computes it the same way, word for word): 32-bit states, 16-bit renormalisation words, probability scale M = 2^12, lower bound
// L = 2^16, 64 lanes.  Symbol i of a frame (s = code + qmax, row-major) belongs to lane i mod 64 and step i div 64.
//
// One wavefront (one 64-thread workgroup) per frame, grid = frames.  A lane is one rANS state; the only traffic between lanes is where a
// word goes: per step a ballot of the lanes that renormalise, and the count of set bits below the lane (v_mbcnt) as the lane's place
// among them.
//   encode: steps from the last to the first; the emitted words are written from the END of the frame's region of ceil(n / 64) 64 words
//           (the most a frame can emit: at most one word per symbol) backwards, so the stream ends up contiguous, in the order the decoder
//           reads it (steps ascending, lanes ascending), in the last n_words entries of the region.  The symbols do not depend on the
//           states, so they are loaded a block of steps ahead of the dependent chain, the next block while this one is coded.
//   decode: steps ascending; the stream is staged through an LDS ring a chunk ahead of the read position (the position depends on the
//           states, a global load per step would put memory latency into the chain); every global read is bounded to the frame's
//           [offset, offset + n_words), itself cut to the words array; past the end a read yields 0.
// freq / cum live in LDS as one dword per symbol (cum << 16 | freq), the prefix sum built once per launch; decode expands them into the
// 4096-entry slot table, one dword per slot holding the symbol, its frequency and slot - cum, so a step costs one table read.  x / freq is hipcc's 32-bit unsigned division (exact).  freq << 20 is 2^32 when one symbol owns the table: that comparison is
// made in 64 bits.  Every output element is written by every launch (the unused head of a frame's word region excepted: it is not part
// of the stream): no global atomics, no float atomics, no memset, no workspace; bitwise reproducible; safe inside a captured hipGraph.
#include "common.hpp"

namespace {

constexpr int RANS_LANES = 64;
constexpr int RANS_SCALE_BITS = 12;
constexpr unsigned RANS_M = 1u << RANS_SCALE_BITS;
constexpr unsigned RANS_L = 1u << 16;
constexpr int RANS_TAB = 256;                 // table entries in LDS (4 per lane; at most 255 symbols)
constexpr int RANS_AHEAD = 8;                 // encode: steps whose symbols are loaded before the chain needs them
constexpr int RANS_RING = 2048;               // decode: words of the LDS ring
constexpr int RANS_CHUNK = 1024;              // decode: words per refill (16 per lane); RING >= CHUNK + 64
constexpr long RANS_MAX_FRAME = 1L << 30;     // symbols per frame

// the number of set bits of a ballot below this lane
__device__ __forceinline__ unsigned rans_rank(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// tab[s] = cum[s] << 16 | freq[s] for s < 256 (freq 0 past nsym): lane l owns symbols 4 l .. 4 l + 3; the exclusive prefix over the lanes'
// sums goes through ``part`` (64 dwords of LDS, broadcast reads: no LDS-crossbar shuffle, once per launch).  Ends with the table visible.
__device__ __forceinline__ void rans_build_table(const uint16_t* __restrict__ freq, int nsym, unsigned* __restrict__ tab,
                                                 unsigned* __restrict__ part, int lane)
{
    unsigned f[4], tot = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int s = lane * 4 + j;
        f[j] = s < nsym ? (unsigned)freq[s] : 0u;
        tot += f[j];
    }
    part[lane] = tot;
    __syncthreads();
    unsigned c = 0u;
#pragma unroll 8
    for (int k = 0; k < RANS_LANES; ++k) {
        const unsigned v = part[k];
        c += k < lane ? v : 0u;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        tab[lane * 4 + j] = ((c < 0xffffu ? c : 0xffffu) << 16) | f[j];          // a table that sums to M never saturates
        c += f[j];
    }
    __syncthreads();
}

// the codes of steps t0 - 1 .. t0 - RANS_AHEAD of this lane.  No branch around a load: an index before the frame's first step or past its
// last symbol is clamped into the frame instead (such a step is idle or never runs), so the loads issue back to back.
__device__ __forceinline__ void rans_load_symbols(const int8_t* __restrict__ src, long n, int t0, int lane, int (&sym)[RANS_AHEAD])
{
#pragma unroll
    for (int j = 0; j < RANS_AHEAD; ++j) {
        const int t = t0 - 1 - j;
        long i = (long)(t < 0 ? 0 : t) * RANS_LANES + lane;
        i = i < n ? i : n - 1;
        sym[j] = (int)src[i];
    }
}

// blockIdx.x = frame; n = hw ld symbols, steps = ceil(n / 64); words (frames, steps 64)
__global__ __launch_bounds__(RANS_LANES) void rans_encode_kernel(const int8_t* __restrict__ codes, const float* __restrict__ keep,
                                                                 const uint16_t* __restrict__ freq, uint16_t* __restrict__ words,
                                                                 int* __restrict__ n_words, unsigned* __restrict__ state, long n, int steps,
                                                                 int nsym, int qmax)
{
    __shared__ unsigned tab[RANS_TAB];
    __shared__ unsigned part[RANS_LANES];
    const long fr = blockIdx.x;
    const int lane = threadIdx.x;
    if (!(keep[fr] != 0.f)) {                                      // dropped or padding: not read (uniform branch)
        state[fr * RANS_LANES + lane] = RANS_L;
        if (lane == 0) n_words[fr] = 0;
        return;
    }
    rans_build_table(freq, nsym, tab, part, lane);
    const int8_t* src = codes + fr * n;
    const long cap = (long)steps * RANS_LANES;
    uint16_t* end = words + fr * cap + cap;                        // one past the frame's region
    unsigned x = RANS_L;
    unsigned written = 0u;                                         // <= cap <= 2^30
    int sym[RANS_AHEAD];
    rans_load_symbols(src, n, steps, lane, sym);
    for (int t0 = steps; t0 > 0; t0 -= RANS_AHEAD) {
        unsigned ent[RANS_AHEAD];
#pragma unroll
        for (int j = 0; j < RANS_AHEAD; ++j) {
            const int s = sym[j] + qmax;
            ent[j] = tab[s < 0 ? 0 : (s >= nsym ? nsym - 1 : s)];   // a code beyond +-qmax (outside the contract) stays inside the table
        }
        rans_load_symbols(src, n, t0 - RANS_AHEAD, lane, sym);     // the next block's codes travel while this block's chain runs
#pragma unroll
        for (int j = 0; j < RANS_AHEAD; ++j) {
            const int t = t0 - 1 - j;
            if (t < 0) break;                                      // uniform
            const bool active = (long)t * RANS_LANES + lane < n;
            const unsigned e = ent[j];
            const unsigned f = e & 0xffffu, c = e >> 16;
            const bool emit = active && (unsigned long long)x >= ((unsigned long long)f << 20);
            const unsigned long long m = __ballot(emit);
            const unsigned cnt = (unsigned)__popcll(m);
            if (emit) {
                end[-(long)(written + cnt) + (long)rans_rank(m)] = (uint16_t)x;       // written + cnt <= 64 (steps - t) <= cap
                x >>= 16;
            }
            written += cnt;
            if (active) {
                const unsigned fd = f ? f : 1u;                    // a symbol outside the table's support (outside the contract)
                const unsigned q = x / fd;
                x = (q << RANS_SCALE_BITS) + (x - q * fd) + c;
            }
        }
    }
    state[fr * RANS_LANES + lane] = x;
    if (lane == 0) n_words[fr] = (int)written;
}

// blockIdx.x = frame; frame fr's stream is words[offsets[fr] .. offsets[fr] + n_words[fr]), cut to [0, total)
__global__ __launch_bounds__(RANS_LANES) void rans_decode_kernel(const uint16_t* __restrict__ words, long total, const long* __restrict__ offsets,
                                                                 const int* __restrict__ n_words, const unsigned* __restrict__ state,
                                                                 const uint16_t* __restrict__ freq, int8_t* __restrict__ codes,
                                                                 int* __restrict__ ok, long n, int steps, int nsym, int qmax)
{
    __shared__ unsigned tab[RANS_TAB];
    __shared__ unsigned part[RANS_LANES];
    __shared__ unsigned slot_tab[RANS_M];                          // slot -> (freq - 1) << 20 | (slot - cum) << 8 | symbol: one read per step
    __shared__ uint16_t ring[RANS_RING];
    const long fr = blockIdx.x;
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < (int)RANS_M / RANS_LANES; ++k) slot_tab[lane + k * RANS_LANES] = 0u;          // a table that sums to less than M
    rans_build_table(freq, nsym, tab, part, lane);
    for (int s = 0; s < nsym; ++s) {                               // at most nsym + 64 stores per lane over the whole loop
        const unsigned e = tab[s];
        const unsigned f = e & 0xffffu, c = e >> 16;
        for (unsigned k = lane; k < f; k += RANS_LANES)            // k = slot - cum < freq <= 4096 for a table that sums to M
            if (c + k < RANS_M) slot_tab[c + k] = ((f - 1u) << 20) | ((k & 0xfffu) << 8) | (unsigned)s;
    }
    __syncthreads();
    long off = offsets[fr];
    long cnt = n_words[fr];
    const bool fits = off >= 0 && cnt >= 0 && off <= total && cnt <= total - off;
    off = off < 0 ? 0 : (off > total ? total : off);
    cnt = cnt < 0 ? 0 : (cnt > total - off ? total - off : cnt);
    const uint16_t* w = words + off;
    int8_t* dst = codes + fr * n;
    unsigned x = state[fr * RANS_LANES + lane];
    long pos = 0, hi = 0;                                          // words consumed; words staged (the ring holds [pos, hi))
    for (int t = 0; t < steps; ++t) {
        if (pos + RANS_LANES > hi) {                               // uniform: hi - pos < 64, so the refill overwrites no live word
            if (hi < cnt) {                                        // uniform.  No branch around a load, so the 16 issue back to back: the
                uint16_t v[RANS_CHUNK / RANS_LANES];               // index is clamped to the stream's last word, never outside [off, off + cnt)
#pragma unroll
                for (int j = 0; j < RANS_CHUNK / RANS_LANES; ++j) {
                    const long r = hi + j * RANS_LANES + lane;
                    v[j] = w[r < cnt ? r : cnt - 1];
                }
#pragma unroll
                for (int j = 0; j < RANS_CHUNK / RANS_LANES; ++j) {
                    const long r = hi + j * RANS_LANES + lane;
                    ring[r & (RANS_RING - 1)] = r < cnt ? v[j] : (uint16_t)0;
                }
            } else {                                               // past the stream: zeros
#pragma unroll
                for (int j = 0; j < RANS_CHUNK / RANS_LANES; ++j) ring[(hi + j * RANS_LANES + lane) & (RANS_RING - 1)] = (uint16_t)0;
            }
            hi += RANS_CHUNK;
            __syncthreads();
        }
        const long i = (long)t * RANS_LANES + lane;
        const bool active = i < n;
        const unsigned e = slot_tab[x & (RANS_M - 1)];
        if (active) {
            dst[i] = (int8_t)((int)(e & 0xffu) - qmax);
            x = ((e >> 20) + 1u) * (x >> RANS_SCALE_BITS) + ((e >> 8) & 0xfffu);
        }
        const bool need = active && x < RANS_L;
        const unsigned long long m = __ballot(need);
        if (need) x = (x << 16) | (unsigned)ring[(pos + (long)rans_rank(m)) & (RANS_RING - 1)];      // pos + rank < pos + 64 <= hi
        pos += __popcll(m);
    }
    const unsigned long long off_l = __ballot(x != RANS_L);
    if (lane == 0) ok[fr] = (fits && off_l == 0ull && pos == cnt) ? 1 : 0;
}

}  // namespace

extern "C" int vvae_rans_supported(int hw, int ld, int bits)
{
    return bits >= 2 && bits <= 8 && hw >= 1 && ld >= 1 && (long)hw * ld <= RANS_MAX_FRAME;
}

// codes int8 (frames, hw, ld); keep fp32 (frames,); freq uint16 (2 qmax + 1,) summing to 4096, positive on every code that occurs in a
// kept frame; words uint16 (frames, ceil(hw ld / 64) 64); n_words int32 (frames,); state uint32 (frames, 64).
extern "C" int vvae_rans_encode(const int8_t* codes, const float* keep, const uint16_t* freq, uint16_t* words, int* n_words, uint32_t* state,
                                int frames, int hw, int ld, int bits, void* stream)
{
    if (!codes || !keep || !freq || !words || !n_words || !state || frames < 1 || !vvae_rans_supported(hw, ld, bits) ||
        (uintptr_t)keep % 4 || (uintptr_t)freq % 2 || (uintptr_t)words % 2 || (uintptr_t)n_words % 4 || (uintptr_t)state % 4)
        return VVAE_ERR_BAD_ARG;
    const long n = (long)hw * ld;
    const int steps = (int)((n + RANS_LANES - 1) / RANS_LANES);
    const int qmax = (1 << (bits - 1)) - 1;
    hipLaunchKernelGGL(rans_encode_kernel, dim3((unsigned)frames), dim3(RANS_LANES), 0, (hipStream_t)stream, codes, keep, freq, words, n_words,
                       state, n, steps, 2 * qmax + 1, qmax);
    VVAE_LAUNCH_CHECK();
    return 0;
}

// words uint16 (total_words,); offsets int64 (frames,), n_words int32 (frames,): frame f's stream is words[offsets[f] .. + n_words[f]);
// state uint32 (frames, 64); freq as above -> codes int8 (frames, hw, ld), ok int32 (frames,): 1 when the frame's stream lies inside
// words, every one of its words was consumed and every lane ended at L.
extern "C" int vvae_rans_decode(const uint16_t* words, long total_words, const long* offsets, const int* n_words, const uint32_t* state,
                                const uint16_t* freq, int8_t* codes, int* ok, int frames, int hw, int ld, int bits, void* stream)
{
    if ((!words && total_words > 0) || total_words < 0 || !offsets || !n_words || !state || !freq || !codes || !ok || frames < 1 ||
        !vvae_rans_supported(hw, ld, bits) || (uintptr_t)words % 2 || (uintptr_t)offsets % 8 || (uintptr_t)n_words % 4 || (uintptr_t)state % 4 ||
        (uintptr_t)freq % 2 || (uintptr_t)ok % 4)
        return VVAE_ERR_BAD_ARG;
    const long n = (long)hw * ld;
    const int steps = (int)((n + RANS_LANES - 1) / RANS_LANES);
    const int qmax = (1 << (bits - 1)) - 1;
    hipLaunchKernelGGL(rans_decode_kernel, dim3((unsigned)frames), dim3(RANS_LANES), 0, (hipStream_t)stream, words, total_words, offsets, n_words,
                       state, freq, codes, ok, n, steps, 2 * qmax + 1, qmax);
    VVAE_LAUNCH_CHECK();
    return 0;
}
