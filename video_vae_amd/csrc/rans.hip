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

// ---------------------------------------------------------------------------------------------------------------- the context coder
// entropy.py: encode_context_reference / decode_context_reference.  Everything above stays; the table of a symbol is chosen by the energy
// E = sum_c |code| of the token grid_w places before its own: context 0 when there is none, else 1 + (E > thr0) + (E > thr1).  Four tables
// tab[ctx][s] in LDS, the energies of the frame's tokens in LDS (hw <= RANS_CTX_MAX_HW).  The context of a lane's symbol depends on its
// index and on E only, never on the state: it is read ahead of the dependent chain.  (grid_w - 1) ld >= 63 puts every symbol of the token
// above into an earlier step than any symbol of this one, so the decoder's E[tok - grid_w] is complete before the step that reads it.
constexpr int RANS_CTX = 4;
constexpr int RANS_CTX_MAX_HW = 4096;         // tokens per frame: the energies are 16 KB of LDS
constexpr int RANS_COUNT_THREADS = 256;

// the four tables, one after the other (rans_build_table ends with a barrier, so ``part`` is free again)
__device__ __forceinline__ void rans_build_tables(const uint16_t* __restrict__ freq4, int nsym, unsigned* __restrict__ tab,
                                                  unsigned* __restrict__ part, int lane)
{
    for (int k = 0; k < RANS_CTX; ++k) rans_build_table(freq4 + k * nsym, nsym, tab + k * RANS_TAB, part, lane);
}

// sum of |code| over the bytes of a load unit
__device__ __forceinline__ int rans_abs_sum(int8_t v) { return v < 0 ? -(int)v : (int)v; }
__device__ __forceinline__ int rans_abs_sum(unsigned w)
{
    int e = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) e += rans_abs_sum((int8_t)(w >> (8 * b)));
    return e;
}
__device__ __forceinline__ int rans_abs_sum(uint4 w) { return rans_abs_sum(w.x) + rans_abs_sum(w.y) + rans_abs_sum(w.z) + rans_abs_sum(w.w); }

// sum of |code| over a token's row of ``units`` load units, 8 loads in flight: no branch around a load, an index past the row is clamped
// into it and its value dropped
template <typename U> __device__ __forceinline__ int rans_row_energy(const U* __restrict__ row, int units)
{
    int e = 0;
    for (int c0 = 0; c0 < units; c0 += 8) {
        U v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = row[c0 + j < units ? c0 + j : units - 1];
#pragma unroll
        for (int j = 0; j < 8; ++j) e += c0 + j < units ? rans_abs_sum(v[j]) : 0;
    }
    return e;
}

// E[tok] = sum of |code| over the token's ld channels, a token per thread: plain stores, no atomics.  Rows of 16-byte or 4-byte units
// where ld and the frame's address allow it.  Ends with E visible to the workgroup.
__device__ __forceinline__ void rans_token_energy(const int8_t* __restrict__ src, int hw, int ld, int* __restrict__ E, int tid, int threads)
{
    const int unit = (ld % 16 == 0 && (uintptr_t)src % 16 == 0) ? 16 : (ld % 4 == 0 && (uintptr_t)src % 4 == 0) ? 4 : 1;      // uniform
    for (int tok = tid; tok < hw; tok += threads) {
        const int8_t* row = src + (long)tok * ld;
        E[tok] = unit == 16 ? rans_row_energy(reinterpret_cast<const uint4*>(row), ld / 16)
                 : unit == 4 ? rans_row_energy(reinterpret_cast<const unsigned*>(row), ld / 4) : rans_row_energy(row, ld);
    }
    __syncthreads();
}

// the context of a symbol of token ``tok`` from the energies ``e_above`` = E[clamp(tok - grid_w)]
__device__ __forceinline__ int rans_context(int tok, int grid_w, int e_above, int thr0, int thr1)
{
    return tok < grid_w ? 0 : 1 + (e_above > thr0 ? 1 : 0) + (e_above > thr1 ? 1 : 0);
}
__device__ __forceinline__ int rans_above(int tok, int grid_w, int hw)
{
    const int up = tok - grid_w;
    return up < 0 ? 0 : (up >= hw ? hw - 1 : up);                          // always inside E; a token without one above never uses it
}

// C[tok] = the table offset (context * RANS_TAB) of the symbols of token tok, once per token instead of once per symbol; E complete and
// visible on entry, C visible on return
__device__ __forceinline__ void rans_token_offsets(const int* __restrict__ E, uint16_t* __restrict__ C, int hw, int grid_w, int thr0, int thr1,
                                                   int tid, int threads)
{
    for (int tok = tid; tok < hw; tok += threads)
        C[tok] = (uint16_t)(rans_context(tok, grid_w, E[rans_above(tok, grid_w, hw)], thr0, thr1) * RANS_TAB);
    __syncthreads();
}

// blockIdx.x = frame; counts int32 (frames, 4, 256): counts[f][ctx][code + 128] over the frame's symbols
__global__ __launch_bounds__(RANS_COUNT_THREADS) void rans_context_counts_kernel(const int8_t* __restrict__ codes, const float* __restrict__ keep,
                                                                                 int* __restrict__ counts, int hw, int ld, int grid_w, int thr0,
                                                                                 int thr1)
{
    __shared__ int E[RANS_CTX_MAX_HW];
    __shared__ uint16_t C[RANS_CTX_MAX_HW];
    __shared__ int hist[RANS_CTX * 256];
    const long fr = blockIdx.x;
    const int tid = threadIdx.x;
    int* dst = counts + fr * (RANS_CTX * 256);
    if (!(keep[fr] != 0.f)) {                                      // dropped or padding: not read (uniform branch)
        for (int k = tid; k < RANS_CTX * 256; k += RANS_COUNT_THREADS) dst[k] = 0;
        return;
    }
    for (int k = tid; k < RANS_CTX * 256; k += RANS_COUNT_THREADS) hist[k] = 0;
    const int n = hw * ld;                                         // <= 2^30
    const int8_t* src = codes + fr * (long)n;
    rans_token_energy(src, hw, ld, E, tid, RANS_COUNT_THREADS);    // its barrier covers the zeroed histogram too
    rans_token_offsets(E, C, hw, grid_w, thr0, thr1, tid, RANS_COUNT_THREADS);
    static_assert(RANS_TAB == 256, "a table offset is a histogram offset");
    for (int i = tid; i < n; i += RANS_COUNT_THREADS) atomicAdd(&hist[(int)C[i / ld] + (int)src[i] + 128], 1);
    __syncthreads();
    for (int k = tid; k < RANS_CTX * 256; k += RANS_COUNT_THREADS) dst[k] = hist[k];
}

// A lane's place in the frame as (token, channel) of its symbol, moved a step (64 symbols) at a time: no division per symbol.
struct RansCursor {
    int tok, ch;
};
__device__ __forceinline__ void rans_cursor_back(RansCursor& c, int ld, int q64, int r64)
{
    c.tok -= q64;
    c.ch -= r64;
    if (c.ch < 0) {
        c.ch += ld;
        c.tok -= 1;
    }
}
__device__ __forceinline__ void rans_cursor_forth(RansCursor& c, int ld, int q64, int r64)
{
    c.tok += q64;
    c.ch += r64;
    if (c.ch >= ld) {
        c.ch -= ld;
        c.tok += 1;
    }
}

// rans_load_symbols with the table offsets of the same steps; ``cur`` is at step t0 - 1 on entry and at step t0 - 1 - RANS_AHEAD on
// return.  A token outside the frame (a step that is idle or never runs) is clamped into it.
__device__ __forceinline__ void rans_load_symbols_ctx(const int8_t* __restrict__ src, long n, int t0, int lane, const uint16_t* __restrict__ C,
                                                      RansCursor& cur, int hw, int ld, int q64, int r64, int (&sym)[RANS_AHEAD],
                                                      int (&toff)[RANS_AHEAD])
{
    rans_load_symbols(src, n, t0, lane, sym);
#pragma unroll
    for (int j = 0; j < RANS_AHEAD; ++j) {
        toff[j] = (int)C[cur.tok < 0 ? 0 : (cur.tok >= hw ? hw - 1 : cur.tok)];
        rans_cursor_back(cur, ld, q64, r64);
    }
}

// rans_encode_kernel with tab[ctx][s]; blockIdx.x = frame
__global__ __launch_bounds__(RANS_LANES) void rans_encode_ctx_kernel(const int8_t* __restrict__ codes, const float* __restrict__ keep,
                                                                     const uint16_t* __restrict__ freq4, uint16_t* __restrict__ words,
                                                                     int* __restrict__ n_words, unsigned* __restrict__ state, int hw, int ld,
                                                                     int steps, int nsym, int qmax, int grid_w, int thr0, int thr1)
{
    __shared__ unsigned tab[RANS_CTX * RANS_TAB];
    __shared__ unsigned part[RANS_LANES];
    __shared__ int E[RANS_CTX_MAX_HW];
    __shared__ uint16_t C[RANS_CTX_MAX_HW];
    const long fr = blockIdx.x;
    const int lane = threadIdx.x;
    if (!(keep[fr] != 0.f)) {                                      // dropped or padding: not read (uniform branch)
        state[fr * RANS_LANES + lane] = RANS_L;
        if (lane == 0) n_words[fr] = 0;
        return;
    }
    rans_build_tables(freq4, nsym, tab, part, lane);
    const long n = (long)hw * ld;
    const int8_t* src = codes + fr * n;
    rans_token_energy(src, hw, ld, E, lane, RANS_LANES);           // one more read of the frame
    rans_token_offsets(E, C, hw, grid_w, thr0, thr1, lane, RANS_LANES);
    const long cap = (long)steps * RANS_LANES;
    uint16_t* end = words + fr * cap + cap;                        // one past the frame's region
    const int q64 = RANS_LANES / ld, r64 = RANS_LANES % ld;
    const int i_last = (steps - 1) * RANS_LANES + lane;            // < 2^30 + 64
    RansCursor cur = {i_last / ld, i_last % ld};
    unsigned x = RANS_L;
    unsigned written = 0u;                                         // <= cap <= 2^30
    int sym[RANS_AHEAD], toff[RANS_AHEAD];
    rans_load_symbols_ctx(src, n, steps, lane, C, cur, hw, ld, q64, r64, sym, toff);
    for (int t0 = steps; t0 > 0; t0 -= RANS_AHEAD) {
        unsigned ent[RANS_AHEAD];
#pragma unroll
        for (int j = 0; j < RANS_AHEAD; ++j) {
            const int s = sym[j] + qmax;
            ent[j] = tab[toff[j] + (s < 0 ? 0 : (s >= nsym ? nsym - 1 : s))];     // a code beyond +-qmax (outside the contract) stays inside its table
        }
        rans_load_symbols_ctx(src, n, t0 - RANS_AHEAD, lane, C, cur, hw, ld, q64, r64, sym, toff);
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
                const unsigned fd = f ? f : 1u;                    // a symbol outside its table's support (outside the contract)
                const unsigned q = x / fd;
                x = (q << RANS_SCALE_BITS) + (x - q * fd) + c;
            }
        }
    }
    state[fr * RANS_LANES + lane] = x;
    if (lane == 0) n_words[fr] = (int)written;
}

// rans_decode_kernel with a slot table per context.  FULL: four tables of 4096 dwords (64 KB, one read per step as in the static kernel) in
// dynamic LDS; else one byte per slot (the symbol, 16 KB) and a second read of tab[ctx][s].  The energies grow in LDS as the steps proceed
// (integer atomic adds of the decoded magnitudes: several lanes of a step share a token; spreading a token's sum over 8 addresses to
// thin the queue on one was measured slower, 170 against 160 us, for the 8 reads it costs).  One wavefront: its LDS operations execute in
// program order, so the adds of step t are in E before the read for step t + 1, which is issued right behind them and ahead of the
// state-dependent part of the step.
template <bool FULL>
__global__ __launch_bounds__(RANS_LANES) void rans_decode_ctx_kernel(const uint16_t* __restrict__ words, long total, const long* __restrict__ offsets,
                                                                     const int* __restrict__ n_words, const unsigned* __restrict__ state,
                                                                     const uint16_t* __restrict__ freq4, int8_t* __restrict__ codes,
                                                                     int* __restrict__ ok, int hw, int ld, int steps, int nsym, int qmax,
                                                                     int grid_w, int thr0, int thr1)
{
    extern __shared__ unsigned slot_full[];                        // FULL: RANS_CTX * RANS_M dwords
    __shared__ uint8_t slot_sym[FULL ? 4 : RANS_CTX * RANS_M];
    __shared__ unsigned tab[RANS_CTX * RANS_TAB];
    __shared__ unsigned part[RANS_LANES];
    __shared__ uint16_t ring[RANS_RING];
    __shared__ int E[RANS_CTX_MAX_HW];
    const long fr = blockIdx.x;
    const int lane = threadIdx.x;
    for (int k = lane; k < (int)(RANS_CTX * RANS_M); k += RANS_LANES) {           // a table that sums to less than M
        if constexpr (FULL) slot_full[k] = 0u;
        else slot_sym[k] = (uint8_t)0;
    }
    for (int k = lane; k < hw; k += RANS_LANES) E[k] = 0;
    rans_build_tables(freq4, nsym, tab, part, lane);
    for (int g = 0; g < RANS_CTX; ++g)
        for (int s = 0; s < nsym; ++s) {
            const unsigned e = tab[g * RANS_TAB + s];
            const unsigned f = e & 0xffffu, c = e >> 16;
            for (unsigned k = lane; k < f; k += RANS_LANES)        // k = slot - cum < freq <= 4096 for a table that sums to M
                if (c + k < RANS_M) {
                    if constexpr (FULL) slot_full[g * RANS_M + c + k] = ((f - 1u) << 20) | ((k & 0xfffu) << 8) | (unsigned)s;
                    else slot_sym[g * RANS_M + c + k] = (uint8_t)s;
                }
        }
    __syncthreads();
    const long n = (long)hw * ld;
    long off = offsets[fr];
    long cnt = n_words[fr];
    const bool fits = off >= 0 && cnt >= 0 && off <= total && cnt <= total - off;
    off = off < 0 ? 0 : (off > total ? total : off);
    cnt = cnt < 0 ? 0 : (cnt > total - off ? total - off : cnt);
    const uint16_t* w = words + off;
    int8_t* dst = codes + fr * n;
    unsigned x = state[fr * RANS_LANES + lane];
    const int q64 = RANS_LANES / ld, r64 = RANS_LANES % ld;
    RansCursor cur = {lane / ld, lane % ld};
    int ctx = rans_context(cur.tok, grid_w, 0, thr0, thr1);        // step 0: E is all zeros, and row 0 has context 0 anyway
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
        const unsigned slot = x & (RANS_M - 1);
        unsigned s, f, d;                                          // the symbol, its frequency, slot - cum
        if constexpr (FULL) {
            const unsigned e = slot_full[ctx * (int)RANS_M + slot];
            s = e & 0xffu, f = (e >> 20) + 1u, d = (e >> 8) & 0xfffu;
        } else {
            s = slot_sym[ctx * (int)RANS_M + slot];
            const unsigned e = tab[ctx * RANS_TAB + s];
            f = e & 0xffffu, d = slot - (e >> 16);
        }
        const int q = (int)s - qmax;
        if (active && q != 0)                                      // cur.tok < hw on an active lane
            __hip_atomic_fetch_add(&E[cur.tok], q < 0 ? -q : q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        rans_cursor_forth(cur, ld, q64, r64);                      // the next step's context: behind this step's adds, not behind x
        ctx = rans_context(cur.tok, grid_w,
                           __hip_atomic_load(&E[rans_above(cur.tok, grid_w, hw)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP), thr0, thr1);
        if (active) {
            dst[i] = (int8_t)q;
            x = f * (x >> RANS_SCALE_BITS) + d;
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

extern "C" int vvae_rans_context_supported(int hw, int ld, int bits, int grid_w)
{
    return vvae_rans_supported(hw, ld, bits) && hw <= RANS_CTX_MAX_HW && grid_w >= 1 && (long)(grid_w - 1) * ld >= RANS_LANES - 1;
}

// codes int8 (frames, hw, ld); keep fp32 (frames,) -> counts int32 (frames, 4, 256): counts[f][ctx][code + 128]; zeros for a dropped frame
extern "C" int vvae_rans_context_counts(const int8_t* codes, const float* keep, int* counts, int frames, int hw, int ld, int bits, int grid_w,
                                        int thr0, int thr1, void* stream)
{
    if (!codes || !keep || !counts || frames < 1 || !vvae_rans_context_supported(hw, ld, bits, grid_w) || (uintptr_t)keep % 4 ||
        (uintptr_t)counts % 4)
        return VVAE_ERR_BAD_ARG;
    hipLaunchKernelGGL(rans_context_counts_kernel, dim3((unsigned)frames), dim3(RANS_COUNT_THREADS), 0, (hipStream_t)stream, codes, keep, counts,
                       hw, ld, grid_w, thr0, thr1);
    VVAE_LAUNCH_CHECK();
    return 0;
}

// vvae_rans_encode with freq4 uint16 (4, 2 qmax + 1), every row summing to 4096 and positive on every code that occurs in its context
extern "C" int vvae_rans_encode_ctx(const int8_t* codes, const float* keep, const uint16_t* freq4, uint16_t* words, int* n_words,
                                    uint32_t* state, int frames, int hw, int ld, int bits, int grid_w, int thr0, int thr1, void* stream)
{
    if (!codes || !keep || !freq4 || !words || !n_words || !state || frames < 1 || !vvae_rans_context_supported(hw, ld, bits, grid_w) ||
        (uintptr_t)keep % 4 || (uintptr_t)freq4 % 2 || (uintptr_t)words % 2 || (uintptr_t)n_words % 4 || (uintptr_t)state % 4)
        return VVAE_ERR_BAD_ARG;
    const long n = (long)hw * ld;
    const int steps = (int)((n + RANS_LANES - 1) / RANS_LANES);
    const int qmax = (1 << (bits - 1)) - 1;
    hipLaunchKernelGGL(rans_encode_ctx_kernel, dim3((unsigned)frames), dim3(RANS_LANES), 0, (hipStream_t)stream, codes, keep, freq4, words,
                       n_words, state, hw, ld, steps, 2 * qmax + 1, qmax, grid_w, thr0, thr1);
    VVAE_LAUNCH_CHECK();
    return 0;
}

// vvae_rans_decode with freq4; slot_form 0: a byte per slot and a second table read (41 KB of LDS a wave), 1: four full slot tables in 64 KB
// of dynamic LDS (89 KB a wave, one per CU), -1: the full tables while every frame gets a CU of its own, where the shorter chain wins (160
// against 175 us at 16 and 64 production frames), the compact ones beyond, where three waves share a CU (382 against 640 us at 1024)
extern "C" int vvae_rans_decode_ctx(const uint16_t* words, long total_words, const long* offsets, const int* n_words, const uint32_t* state,
                                    const uint16_t* freq4, int8_t* codes, int* ok, int frames, int hw, int ld, int bits, int grid_w, int thr0,
                                    int thr1, int slot_form, void* stream)
{
    if ((!words && total_words > 0) || total_words < 0 || !offsets || !n_words || !state || !freq4 || !codes || !ok || frames < 1 ||
        !vvae_rans_context_supported(hw, ld, bits, grid_w) || (uintptr_t)words % 2 || (uintptr_t)offsets % 8 || (uintptr_t)n_words % 4 ||
        (uintptr_t)state % 4 || (uintptr_t)freq4 % 2 || (uintptr_t)ok % 4 || slot_form < -1 || slot_form > 1)
        return VVAE_ERR_BAD_ARG;
    if (slot_form < 0) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
        slot_form = frames <= cus ? 1 : 0;
    }
    const long n = (long)hw * ld;
    const int steps = (int)((n + RANS_LANES - 1) / RANS_LANES);
    const int qmax = (1 << (bits - 1)) - 1;
    if (slot_form == 1) {
        constexpr size_t dyn = (size_t)RANS_CTX * RANS_M * sizeof(unsigned);
        static const hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void*>(&rans_decode_ctx_kernel<true>),
                                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);       // once
        if (raised != hipSuccess) return (int)raised;
        hipLaunchKernelGGL(rans_decode_ctx_kernel<true>, dim3((unsigned)frames), dim3(RANS_LANES), dyn, (hipStream_t)stream, words, total_words,
                           offsets, n_words, state, freq4, codes, ok, hw, ld, steps, 2 * qmax + 1, qmax, grid_w, thr0, thr1);
    } else {
        hipLaunchKernelGGL(rans_decode_ctx_kernel<false>, dim3((unsigned)frames), dim3(RANS_LANES), 0, (hipStream_t)stream, words, total_words,
                           offsets, n_words, state, freq4, codes, ok, hw, ld, steps, 2 * qmax + 1, qmax, grid_w, thr0, thr1);
    }
    VVAE_LAUNCH_CHECK();
    return 0;
}
