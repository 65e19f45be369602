// Interleaved rANS over the quantiser's codes, static, context-adaptive and temporal (video_vae_amd/entropy.py states the format; this file computes
// it the same way, word for word).
//
// The format: 32-bit states, 16-bit renormalisation words, probability scale M = 2^12, lower bound L = 2^16, 64 lanes.  Symbol i of a frame
// (s = code + qmax, row-major) belongs to lane i mod 64 and step i div 64.  One wavefront (one 64-thread workgroup) per frame, grid = frames.
// A lane is one rANS state; the only traffic between lanes is where a word goes: per step a ballot of the lanes that renormalise, and the
// count of set bits below the lane (v_mbcnt) as the lane's place among them.
//   encode: steps from the last to the first; the emitted words are written from the END of the frame's region of ceil(n / 64) 64 words
//           (the most a frame can emit: at most one word per symbol) backwards, so the stream ends up contiguous, in the order the decoder
//           reads it (steps ascending, lanes ascending), in the last n_words entries of the region.  The symbols do not depend on the
//           states, so they are loaded a block of steps ahead of the dependent chain, the next block while this one is coded.
//   decode: steps ascending; the stream is staged through an LDS ring a chunk ahead of the read position (the position depends on the
//           states, a global load per step would put memory latency into the chain); every global read is bounded to the frame's
//           [offset, offset + n_words), itself cut to the words array; past the end a read yields 0.
// freq / cum live in LDS as one dword per symbol (cum << 16 | freq), the prefix sum built once per launch; decode expands them into a
// 4096-entry slot table, one dword per slot holding the symbol, its frequency and slot - cum, so a step costs one table read.  x / freq is
// hipcc's 32-bit unsigned division (exact).  freq << 20 is 2^32 when one symbol owns the table: that comparison is made in 64 bits.  Every
// output element is written by every launch (the unused head of a frame's word region excepted: it is not part of the stream): no global
// atomics, no float atomics, no memset, no workspace; bitwise reproducible; safe inside a captured hipGraph.
//
// Each piece of that is written once, as a helper, inside one body per direction: rans_encode_frame<MODEL> and rans_decode_frame<FORM>; the
// __global__ entry points only name the form.  The static coder is the context coder with one table; the context coder (entropy.py:
// encode_context_reference / decode_context_reference) differs in these points and no others:
//   * the table of a symbol is chosen by the energy E = sum_c |code| of the token grid_w places before its own: context 0 when there is
//     none, else 1 + (E > thr0) + (E > thr1).  Four tables tab[ctx][s] and the energies of the frame's tokens (hw <= RANS_CTX_MAX_HW) in LDS;
//   * a lane keeps a cursor (token, channel) of its symbol, moved a step at a time: the context depends on the symbol's index and on E
//     only, never on the state, so it is read ahead of the dependent chain;
//   * encode knows every E before it starts (one more read of the frame); decode grows E as the steps proceed.  (grid_w - 1) ld >= 63 puts
//     every symbol of the token above into an earlier step than any symbol of this one, so E[tok - grid_w] is complete when it is read;
//   * decode has two slot forms: four full slot tables in 64 KB of dynamic LDS (one read per step, as the static kernel), or one byte per
//     slot (the symbol, 16 KB) and a second read of tab[ctx][s].
// The temporal coder (entropy.py: encode_temporal_reference / decode_temporal_reference) differs from the static one in these points:
//   * nine tables; a frame that starts a chain uses table 0, a chained frame the table 1 + #{k : q_prev > thr[k]} of the code at the same
//     index of the frame before it, through a 256-entry class table in LDS.  The same index is the same lane and step, and the table is
//     known before the frame starts: no energies, no cursor, no condition on the token grid;
//   * encode stays one wavefront per frame (it knows every code) and loads the predecessor's code beside the symbol's own;
//   * decode is one wavefront per CHAIN, its frames in order, each lane reading back the code it stored itself a frame earlier; the
//     tables are built once per chain; compact slots only (nine full tables would be 144 KB of LDS).
#include <initializer_list>
#include <type_traits>
#include <utility>

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
constexpr int RANS_CTX = 4;                   // the tables of the context coder
constexpr int RANS_CTX_MAX_HW = 4096;         // tokens per frame: the energies are 16 KB of LDS
constexpr int RANS_COUNT_THREADS = 256;
constexpr int RANS_TMP = 9;                   // the tables of the temporal coder: chain starts, and 8 classes of the previous frame's code
constexpr int RANS_TMP_THR = RANS_TMP - 2;    // the thresholds between the classes

// which model chooses a symbol's table
enum RansModel { RANS_ONE, RANS_SPATIAL, RANS_TEMPORAL };

// a frame as the kernels see it; the static coder leaves the context members at 0
struct RansFrame {
    long n;                                   // hw ld symbols
    int steps, nsym, qmax;                    // ceil(n / 64); 2 qmax + 1
    int hw, ld, grid_w, thr0, thr1;
};

// the temporal coder's part of a launch (null and zeros in the others): ``prev`` (frames,) the frame an encoder-side frame is coded
// against or -1; ``start`` (chains + 1,) the decoder's chains, chain c = frames start[c] .. start[c + 1] - 1
struct RansThr {
    int v[RANS_TMP_THR];
};
struct RansChains {
    const int* prev;
    const int* start;
    int frames;
    RansThr thr;
};

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

// the K tables, one after the other (rans_build_table ends with a barrier, so ``part`` is free again)
template <int K>
__device__ __forceinline__ void rans_build_tables(const uint16_t* __restrict__ freq, int nsym, unsigned* __restrict__ tab,
                                                  unsigned* __restrict__ part, int lane)
{
    for (int k = 0; k < K; ++k) rans_build_table(freq + k * nsym, nsym, tab + k * RANS_TAB, part, lane);
}

// -------------------------------------------------------------------------------------------- contexts: energies, offsets, the cursor
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

// ------------------------------------------------------------------------------------------- temporal contexts: classes, predecessors
// cls[b] = the table of a symbol whose predecessor (the previous frame's code at the same token and channel) is b - 128:
// 1 + #{k : code > thr[k]}, once per launch instead of seven comparisons per symbol.  Ends with cls visible.
__device__ __forceinline__ void rans_build_classes(const RansThr& thr, uint8_t* __restrict__ cls, int tid, int threads)
{
    for (int b = tid; b < 256; b += threads) {
        int c = 1;
#pragma unroll
        for (int k = 0; k < RANS_TMP_THR; ++k) c += b - 128 > thr.v[k] ? 1 : 0;
        cls[b] = (uint8_t)c;
    }
    __syncthreads();
}

// the frame that frame fr is coded against, or -1 (uniform); an index that names no frame counts as none, so no read leaves the codes
__device__ __forceinline__ long rans_prev(const int* __restrict__ prev, long fr, int frames)
{
    const int p = prev[fr];
    return p >= 0 && p < frames ? (long)p : -1L;
}

// byte b of a load unit as a code
__device__ __forceinline__ int rans_code(int8_t v, int) { return (int)v; }
__device__ __forceinline__ int rans_code(unsigned w, int b) { return (int)(int8_t)(w >> (8 * b)); }
__device__ __forceinline__ int rans_code(uint4 w, int b) { return rans_code(b < 4 ? w.x : (b < 8 ? w.y : (b < 12 ? w.z : w.w)), b & 3); }

// hist[table * 256 + code + 128] += 1 over the frame's n symbols, a load unit of the frame and of its predecessor per thread and turn.
// Quantised latents repeat (zeros above all): a run of equal (table, code) inside a unit is one integer LDS add of its length.
template <typename U>
__device__ __forceinline__ void rans_count_runs(const int8_t* __restrict__ src, const int8_t* __restrict__ psrc, bool chained, int n,
                                                const uint8_t* __restrict__ cls, int* __restrict__ hist, int tid)
{
    constexpr int B = (int)sizeof(U);
    const U* a = reinterpret_cast<const U*>(src);
    const U* p = reinterpret_cast<const U*>(psrc);
    for (int u = tid; u < n / B; u += RANS_COUNT_THREADS) {
        const U va = a[u], vp = p[u];
        int key = 0, run = 0;
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const int k = (chained ? (int)cls[rans_code(vp, b) + 128] : 0) * 256 + rans_code(va, b) + 128;
            if (k != key && run) {
                atomicAdd(&hist[key], run);
                run = 0;
            }
            key = k;
            ++run;
        }
        atomicAdd(&hist[key], run);
    }
}

// blockIdx.x = frame; counts int32 (frames, 9, 256): counts[f][table][code + 128] over the frame's symbols
__global__ __launch_bounds__(RANS_COUNT_THREADS) void rans_temporal_counts_kernel(const int8_t* __restrict__ codes, const float* __restrict__ keep,
                                                                                  int* __restrict__ counts, int n, RansChains ch)
{
    __shared__ uint8_t cls[256];
    __shared__ int hist[RANS_TMP * 256];
    const long fr = blockIdx.x;
    const int tid = threadIdx.x;
    int* dst = counts + fr * (RANS_TMP * 256);
    if (!(keep[fr] != 0.f)) {                                      // dropped or padding: not read (uniform branch)
        for (int k = tid; k < RANS_TMP * 256; k += RANS_COUNT_THREADS) dst[k] = 0;
        return;
    }
    for (int k = tid; k < RANS_TMP * 256; k += RANS_COUNT_THREADS) hist[k] = 0;
    rans_build_classes(ch.thr, cls, tid, RANS_COUNT_THREADS);      // its barrier covers the zeroed histogram too
    const long pf = rans_prev(ch.prev, fr, ch.frames);
    const bool chained = pf >= 0;
    const int8_t* src = codes + fr * (long)n;                      // n <= 2^30
    const int8_t* psrc = codes + (chained ? pf : fr) * (long)n;    // a chain start reads itself and drops what it read: no branch at the loads
    const uintptr_t both = (uintptr_t)src | (uintptr_t)psrc | (uintptr_t)n;            // uniform
    if (both % 16 == 0) rans_count_runs<uint4>(src, psrc, chained, n, cls, hist, tid);
    else if (both % 4 == 0) rans_count_runs<unsigned>(src, psrc, chained, n, cls, hist, tid);
    else rans_count_runs<int8_t>(src, psrc, chained, n, cls, hist, tid);
    __syncthreads();
    for (int k = tid; k < RANS_TMP * 256; k += RANS_COUNT_THREADS) dst[k] = hist[k];
}

// ------------------------------------------------------------------------------------------------------------------------------- encode
// a dropped or padding frame is not read: no word, every state L.  True when the frame was one (uniform).
__device__ __forceinline__ bool rans_dropped(const float* __restrict__ keep, long fr, int* __restrict__ n_words, unsigned* __restrict__ state,
                                             int lane)
{
    if (keep[fr] != 0.f) return false;
    state[fr * RANS_LANES + lane] = RANS_L;
    if (lane == 0) n_words[fr] = 0;
    return true;
}

// one symbol per active lane with the table entry ``e`` = cum << 16 | freq: the lanes that renormalise store their low words, ranked by
// lane, in front of the ``written`` words that end at ``end``; then the state takes the symbol
__device__ __forceinline__ void rans_encode_step(unsigned& x, unsigned& written, unsigned e, bool active, uint16_t* __restrict__ end)
{
    const unsigned f = e & 0xffffu, c = e >> 16;
    const bool emit = active && (unsigned long long)x >= ((unsigned long long)f << 20);
    const unsigned long long m = __ballot(emit);
    const unsigned cnt = (unsigned)__popcll(m);
    if (emit) {
        end[-(long)(written + cnt) + (long)rans_rank(m)] = (uint16_t)x;       // written + cnt <= 64 (steps done) <= the frame's region
        x >>= 16;
    }
    written += cnt;
    if (active) {
        const unsigned fd = f ? f : 1u;                    // a symbol outside its table's support (outside the contract)
        const unsigned q = x / fd;
        x = (q << RANS_SCALE_BITS) + (x - q * fd) + c;
    }
}

// the table offsets of the steps whose codes rans_load_symbols loads; ``cur`` is at the first of them on entry and RANS_AHEAD steps
// further back on return.  A token outside the frame (a step that is idle or never runs) is clamped into it.
__device__ __forceinline__ void rans_load_offsets(const uint16_t* __restrict__ C, RansCursor& cur, const RansFrame& fm, int q64, int r64,
                                                  int (&toff)[RANS_AHEAD])
{
#pragma unroll
    for (int j = 0; j < RANS_AHEAD; ++j) {
        toff[j] = (int)C[cur.tok < 0 ? 0 : (cur.tok >= fm.hw ? fm.hw - 1 : cur.tok)];
        rans_cursor_back(cur, fm.ld, q64, r64);
    }
}

// blockIdx.x = frame; words (frames, steps 64).  An array that a model does not use (E and C in the static kernel) takes no LDS there.
// RANS_TEMPORAL: the encoder knows every code, so its frames stay independent; the predecessor's code is loaded with the symbol's own, as
// far ahead of the chain, and chooses the table through cls.  A chain start loads its own codes in their place (no branch at the loads)
// and drops them.
template <int MODEL>
__device__ __forceinline__ void rans_encode_frame(const int8_t* __restrict__ codes, const float* __restrict__ keep,
                                                  const uint16_t* __restrict__ freq, uint16_t* __restrict__ words, int* __restrict__ n_words,
                                                  unsigned* __restrict__ state, const RansFrame& fm, const RansChains& ch)
{
    constexpr bool CTX = MODEL == RANS_SPATIAL, TMP = MODEL == RANS_TEMPORAL;
    constexpr int K = CTX ? RANS_CTX : (TMP ? RANS_TMP : 1);
    __shared__ unsigned tab[K * RANS_TAB];
    __shared__ unsigned part[RANS_LANES];
    __shared__ int E[CTX ? RANS_CTX_MAX_HW : 1];
    __shared__ uint16_t C[CTX ? RANS_CTX_MAX_HW : 1];
    __shared__ uint8_t cls[TMP ? 256 : 1];
    const long fr = blockIdx.x;
    const int lane = threadIdx.x;
    if (rans_dropped(keep, fr, n_words, state, lane)) return;
    rans_build_tables<K>(freq, fm.nsym, tab, part, lane);
    const int8_t* src = codes + fr * fm.n;
    const long cap = (long)fm.steps * RANS_LANES;
    uint16_t* end = words + fr * cap + cap;                        // one past the frame's region
    unsigned x = RANS_L;
    unsigned written = 0u;                                         // <= cap <= 2^30
    int sym[RANS_AHEAD], toff[RANS_AHEAD];
    [[maybe_unused]] int q64 = 0, r64 = 0;
    [[maybe_unused]] RansCursor cur = {0, 0};
    [[maybe_unused]] int before[RANS_AHEAD];                       // the predecessor's codes of the steps of sym
    [[maybe_unused]] const int8_t* psrc = src;
    [[maybe_unused]] bool chained = false;
    if constexpr (TMP) {
        rans_build_classes(ch.thr, cls, lane, RANS_LANES);
        const long pf = rans_prev(ch.prev, fr, ch.frames);
        chained = pf >= 0;                                         // uniform
        psrc = codes + (chained ? pf : fr) * fm.n;
    }
    if constexpr (CTX) {
        rans_token_energy(src, fm.hw, fm.ld, E, lane, RANS_LANES);         // one more read of the frame
        rans_token_offsets(E, C, fm.hw, fm.grid_w, fm.thr0, fm.thr1, lane, RANS_LANES);
        q64 = RANS_LANES / fm.ld, r64 = RANS_LANES % fm.ld;
        const int i_last = (fm.steps - 1) * RANS_LANES + lane;             // < 2^30 + 64
        cur = {i_last / fm.ld, i_last % fm.ld};
    }
    rans_load_symbols(src, fm.n, fm.steps, lane, sym);
    if constexpr (CTX) rans_load_offsets(C, cur, fm, q64, r64, toff);
    if constexpr (TMP) rans_load_symbols(psrc, fm.n, fm.steps, lane, before);
    for (int t0 = fm.steps; t0 > 0; t0 -= RANS_AHEAD) {
        unsigned ent[RANS_AHEAD];
#pragma unroll
        for (int j = 0; j < RANS_AHEAD; ++j) {
            const int s = sym[j] + fm.qmax;
            int at = s < 0 ? 0 : (s >= fm.nsym ? fm.nsym - 1 : s);         // a code beyond +-qmax (outside the contract) stays inside its table
            if constexpr (CTX) at += toff[j];
            if constexpr (TMP) at += chained ? (int)cls[before[j] + 128] * RANS_TAB : 0;
            ent[j] = tab[at];
        }
        rans_load_symbols(src, fm.n, t0 - RANS_AHEAD, lane, sym);  // the next block's codes travel while this block's chain runs
        if constexpr (CTX) rans_load_offsets(C, cur, fm, q64, r64, toff);
        if constexpr (TMP) rans_load_symbols(psrc, fm.n, t0 - RANS_AHEAD, lane, before);
#pragma unroll
        for (int j = 0; j < RANS_AHEAD; ++j) {
            const int t = t0 - 1 - j;
            if (t < 0) break;                                      // uniform
            rans_encode_step(x, written, ent[j], (long)t * RANS_LANES + lane < fm.n, end);
        }
    }
    state[fr * RANS_LANES + lane] = x;
    if (lane == 0) n_words[fr] = (int)written;
}

// n = hw ld symbols, steps = ceil(n / 64)
__global__ __launch_bounds__(RANS_LANES) void rans_encode_kernel(const int8_t* __restrict__ codes, const float* __restrict__ keep,
                                                                 const uint16_t* __restrict__ freq, uint16_t* __restrict__ words,
                                                                 int* __restrict__ n_words, unsigned* __restrict__ state, long n, int steps,
                                                                 int nsym, int qmax)
{
    rans_encode_frame<RANS_ONE>(codes, keep, freq, words, n_words, state, RansFrame{n, steps, nsym, qmax, 0, 0, 0, 0, 0}, RansChains{});
}

__global__ __launch_bounds__(RANS_LANES) void rans_encode_ctx_kernel(const int8_t* __restrict__ codes, const float* __restrict__ keep,
                                                                     const uint16_t* __restrict__ freq4, uint16_t* __restrict__ words,
                                                                     int* __restrict__ n_words, unsigned* __restrict__ state, int hw, int ld,
                                                                     int steps, int nsym, int qmax, int grid_w, int thr0, int thr1)
{
    rans_encode_frame<RANS_SPATIAL>(codes, keep, freq4, words, n_words, state,
                                    RansFrame{(long)hw * ld, steps, nsym, qmax, hw, ld, grid_w, thr0, thr1}, RansChains{});
}

// freq9 (9, nsym); ch.prev (frames,) and ch.thr
__global__ __launch_bounds__(RANS_LANES) void rans_encode_temporal_kernel(const int8_t* __restrict__ codes, const float* __restrict__ keep,
                                                                          const uint16_t* __restrict__ freq9, uint16_t* __restrict__ words,
                                                                          int* __restrict__ n_words, unsigned* __restrict__ state, long n,
                                                                          int steps, int nsym, int qmax, RansChains ch)
{
    rans_encode_frame<RANS_TEMPORAL>(codes, keep, freq9, words, n_words, state, RansFrame{n, steps, nsym, qmax, 0, 0, 0, 0, 0}, ch);
}

// ------------------------------------------------------------------------------------------------------------------------------- decode
enum RansForm { RANS_STATIC, RANS_CTX_COMPACT, RANS_CTX_FULL, RANS_TMP_COMPACT };
template <int FORM> constexpr bool RANS_COMPACT = FORM == RANS_CTX_COMPACT || FORM == RANS_TMP_COMPACT;
// a slot table entry: a byte (the symbol) in the compact forms, else a dword (freq - 1) << 20 | (slot - cum) << 8 | symbol
template <int FORM> using RansSlot = std::conditional_t<RANS_COMPACT<FORM>, uint8_t, unsigned>;

// slots[g][slot] for the K tables tab[g] (cum << 16 | freq per symbol), over slots that were zeroed before the tables were built (a table
// that sums to less than M leaves some untouched); ends with the slots visible
template <int K, typename S>
__device__ __forceinline__ void rans_expand_slots(const unsigned* __restrict__ tab, int nsym, S* __restrict__ slots, int lane)
{
    for (int g = 0; g < K; ++g)
        for (int s = 0; s < nsym; ++s) {                           // at most nsym + 64 stores per lane and table over the whole loop
            const unsigned e = tab[g * RANS_TAB + s];
            const unsigned f = e & 0xffffu, c = e >> 16;
            for (unsigned k = lane; k < f; k += RANS_LANES)        // k = slot - cum < freq <= 4096 for a table that sums to M
                if (c + k < RANS_M) {
                    if constexpr (sizeof(S) == 1) slots[g * RANS_M + c + k] = (S)s;
                    else slots[g * RANS_M + c + k] = ((f - 1u) << 20) | ((k & 0xfffu) << 8) | (unsigned)s;
                }
        }
    __syncthreads();
}

// the symbol of ``slot`` in table ``ctx``, and in ``e`` the entry that holds its frequency and cum: one read (the slot's dword), or in the
// compact form two (the slot's byte, then tab[ctx][s])
template <int FORM>
__device__ __forceinline__ unsigned rans_slot_lookup(const RansSlot<FORM>* __restrict__ slots, const unsigned* __restrict__ tab, int ctx,
                                                     unsigned slot, unsigned& e)
{
    if constexpr (RANS_COMPACT<FORM>) {
        const unsigned s = slots[ctx * (int)RANS_M + slot];
        e = tab[ctx * RANS_TAB + s];
        return s;
    } else {
        e = slots[ctx * (int)RANS_M + slot];
        return e & 0xffu;
    }
}

// the state after it gave up the symbol of ``slot`` with the entry ``e``: freq (x >> 12) + slot - cum
template <int FORM> __device__ __forceinline__ unsigned rans_decode_step(unsigned x, unsigned slot, unsigned e)
{
    if constexpr (RANS_COMPACT<FORM>) return (e & 0xffffu) * (x >> RANS_SCALE_BITS) + slot - (e >> 16);
    else return ((e >> 20) + 1u) * (x >> RANS_SCALE_BITS) + ((e >> 8) & 0xfffu);
}

// a frame's stream w[0 .. cnt): words[off .. off + cnt) cut to [0, total); fits: it needed no cutting
struct RansStream {
    const uint16_t* w;
    long cnt;
    bool fits;
};
__device__ __forceinline__ RansStream rans_stream(const uint16_t* __restrict__ words, long total, long off, long cnt)
{
    const bool fits = off >= 0 && cnt >= 0 && off <= total && cnt <= total - off;
    off = off < 0 ? 0 : (off > total ? total : off);
    cnt = cnt < 0 ? 0 : (cnt > total - off ? total - off : cnt);
    return {words + off, cnt, fits};
}

// before a step: the ring holds the stream's words [pos, hi); with fewer than 64 of them left (a step takes at most 64) the next chunk
// is staged, zeros past the stream's end.  FORM (here and in rans_renorm_read) only gives every kernel an instantiation of its own:
// inlined from one shared by the three kernels, the same instructions are scheduled into 2 VGPRs more in each (tools/kres.sh).  ``ring``
// is taken as the LDS array itself for the same reason.
template <int FORM, typename Ring>
__device__ __forceinline__ void rans_ring_refill(const RansStream& st, long pos, long& hi, Ring& ring, int lane)
{
    if (pos + RANS_LANES > hi) {                               // uniform: hi - pos < 64, so the refill overwrites no live word
    if (hi < st.cnt) {                                         // uniform.  No branch around a load, so the 16 issue back to back: the
        uint16_t v[RANS_CHUNK / RANS_LANES];                   // index is clamped to the stream's last word, never outside [off, off + cnt)
#pragma unroll
        for (int j = 0; j < RANS_CHUNK / RANS_LANES; ++j) {
            const long r = hi + j * RANS_LANES + lane;
            v[j] = st.w[r < st.cnt ? r : st.cnt - 1];
        }
#pragma unroll
        for (int j = 0; j < RANS_CHUNK / RANS_LANES; ++j) {
            const long r = hi + j * RANS_LANES + lane;
            ring[r & (RANS_RING - 1)] = r < st.cnt ? v[j] : (uint16_t)0;
        }
    } else {                                                   // past the stream: zeros
#pragma unroll
        for (int j = 0; j < RANS_CHUNK / RANS_LANES; ++j) ring[(hi + j * RANS_LANES + lane) & (RANS_RING - 1)] = (uint16_t)0;
    }
    hi += RANS_CHUNK;
    __syncthreads();
    }
}

// the active lanes below L take consecutive words from ``pos`` in ascending lane order
template <int FORM, typename Ring>
__device__ __forceinline__ void rans_renorm_read(unsigned& x, bool active, const Ring& ring, long& pos)
{
    const bool need = active && x < RANS_L;
    const unsigned long long m = __ballot(need);
    if (need) x = (x << 16) | (unsigned)ring[(pos + (long)rans_rank(m)) & (RANS_RING - 1)];      // pos + rank < pos + 64 <= hi
    pos += __popcll(m);
}

// ok: the stream lay inside the words, every word of it was consumed and every lane is back at L
__device__ __forceinline__ void rans_verdict(unsigned x, const RansStream& st, long pos, int* __restrict__ ok, long fr, int lane)
{
    const unsigned long long off_l = __ballot(x != RANS_L);
    if (lane == 0) ok[fr] = (st.fits && off_l == 0ull && pos == st.cnt) ? 1 : 0;
}

// blockIdx.x = frame; frame fr's stream is words[offsets[fr] .. offsets[fr] + n_words[fr]), cut to [0, total).  The slot tables of
// RANS_CTX_FULL are 64 KB of dynamic LDS, and an array that a form does not use (E in the static kernel) takes no LDS.  With a context form the
// energies grow in LDS as the steps proceed (integer atomic adds of the decoded magnitudes: several lanes of a step share a token;
// spreading a token's sum over 8 addresses to thin the queue on one was measured slower, 170 against 160 us, for the 8 reads it costs).
// One wavefront: its LDS operations execute in program order, so the adds of step t are in E before the read for step t + 1, which is
// issued right behind them and ahead of the state-dependent part of the step.
//
// RANS_TMP_COMPACT (the temporal coder): blockIdx.x = chain, and the wave decodes the chain's frames in order.  The table of a symbol comes
// from the code at the same index of the frame before, through cls; that code is the byte THIS lane stored at the same step of the
// previous frame (equal index: equal lane, equal step), and a thread's load of an address follows its own earlier store to it in program
// order, so no barrier, fence or cross-lane visibility is needed (a lane past the frame's last symbol reads a clamped index, another
// lane's byte, and drops it).  The byte does not depend on the state: it is loaded RANS_AHEAD steps ahead of its use and handed down a
// register queue.  Tables, slots and cls are built once per chain; the ring, the bounds and the verdict are per frame, as everywhere.
template <int FORM>
__device__ __forceinline__ void rans_decode_frame(const uint16_t* __restrict__ words, long total, const long* __restrict__ offsets,
                                                  const int* __restrict__ n_words, const unsigned* __restrict__ state,
                                                  const uint16_t* __restrict__ freq, int8_t* __restrict__ codes, int* __restrict__ ok,
                                                  const RansFrame& fm, const RansChains& ch)
{
    constexpr bool CTX = FORM == RANS_CTX_COMPACT || FORM == RANS_CTX_FULL, TMP = FORM == RANS_TMP_COMPACT;
    constexpr int K = CTX ? RANS_CTX : (TMP ? RANS_TMP : 1);
    extern __shared__ unsigned slot_full[];                        // RANS_CTX_FULL: K RANS_M dwords
    __shared__ RansSlot<FORM> slot_tab[FORM == RANS_CTX_FULL ? 1 : K * RANS_M];
    __shared__ unsigned tab[K * RANS_TAB];
    __shared__ unsigned part[RANS_LANES];
    __shared__ uint16_t ring[RANS_RING];
    __shared__ int E[CTX ? RANS_CTX_MAX_HW : 1];
    __shared__ uint8_t cls[TMP ? 256 : 1];
    RansSlot<FORM>* slots = slot_tab;
    if constexpr (FORM == RANS_CTX_FULL) slots = slot_full;
    long fr = blockIdx.x;
    const int lane = threadIdx.x;
#pragma unroll 64
    for (int k = 0; k < K * (int)RANS_M / RANS_LANES; ++k) slots[lane + k * RANS_LANES] = 0;          // under the latency of the table's loads
    if constexpr (CTX)
        for (int k = lane; k < fm.hw; k += RANS_LANES) E[k] = 0;
    rans_build_tables<K>(freq, fm.nsym, tab, part, lane);
    rans_expand_slots<K>(tab, fm.nsym, slots, lane);
    [[maybe_unused]] long last = 0;
    [[maybe_unused]] bool chained = false;                         // uniform: false on the chain's first frame
    if constexpr (TMP) {
        rans_build_classes(ch.thr, cls, lane, RANS_LANES);
        const long a = ch.start[fr], b = ch.start[fr + 1];         // cut to the frames: no access leaves them whatever start holds
        fr = a < 0 ? 0 : (a > ch.frames ? ch.frames : a);
        last = b < 0 ? 0 : (b > ch.frames ? ch.frames : b);
        if (fr >= last) return;
    }
    do {
    const RansStream st = rans_stream(words, total, offsets[fr], n_words[fr]);
    int8_t* dst = codes + fr * fm.n;
    unsigned x = state[fr * RANS_LANES + lane];
    [[maybe_unused]] int q64 = 0, r64 = 0;
    [[maybe_unused]] RansCursor cur = {0, 0};
    int ctx = 0;                                                   // the static coder's only table
    if constexpr (CTX) {
        q64 = RANS_LANES / fm.ld, r64 = RANS_LANES % fm.ld;
        cur = {lane / fm.ld, lane % fm.ld};
        ctx = rans_context(cur.tok, fm.grid_w, 0, fm.thr0, fm.thr1);       // step 0: E is all zeros, and row 0 has context 0 anyway
    }
    [[maybe_unused]] int before[RANS_AHEAD] = {};                  // the previous frame's codes of the next block of steps, last step first
    [[maybe_unused]] const int8_t* psrc = dst - (chained ? fm.n : 0);
    if constexpr (TMP)
        if (chained) rans_load_symbols(psrc, fm.n, RANS_AHEAD, lane, before);
    long pos = 0, hi = 0;                                          // words consumed; words staged (the ring holds [pos, hi))
    auto step = [&](int t) {
        rans_ring_refill<FORM>(st, pos, hi, ring, lane);
        const long i = (long)t * RANS_LANES + lane;
        const bool active = i < fm.n;
        const unsigned slot = x & (RANS_M - 1);
        unsigned e;
        const int q = (int)rans_slot_lookup<FORM>(slots, tab, ctx, slot, e) - fm.qmax;             // the code
        if constexpr (CTX) {
            if (active && q != 0)                                  // cur.tok < hw on an active lane
                __hip_atomic_fetch_add(&E[cur.tok], q < 0 ? -q : q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            rans_cursor_forth(cur, fm.ld, q64, r64);               // the next step's context: behind this step's adds, not behind x
            ctx = rans_context(cur.tok, fm.grid_w,
                               __hip_atomic_load(&E[rans_above(cur.tok, fm.grid_w, fm.hw)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP),
                               fm.thr0, fm.thr1);
        }
        if (active) {
            dst[i] = (int8_t)q;                                    // ahead of the state's arithmetic: the step waits for this store
            x = rans_decode_step<FORM>(x, slot, e);
        }
        rans_renorm_read<FORM>(x, active, ring, pos);
    };
    if constexpr (TMP) {                                           // a block of steps at a time, as the encoder: the block's tables from the
        for (int t0 = 0; t0 < fm.steps; t0 += RANS_AHEAD) {        // codes loaded a block ago, then the next block's loads, then its chain
            int row[RANS_AHEAD];
#pragma unroll
            for (int j = 0; j < RANS_AHEAD; ++j) row[j] = chained ? (int)cls[before[RANS_AHEAD - 1 - j] + 128] : 0;
            if (chained) rans_load_symbols(psrc, fm.n, t0 + 2 * RANS_AHEAD, lane, before);
#pragma unroll
            for (int j = 0; j < RANS_AHEAD; ++j) {
                if (t0 + j >= fm.steps) break;                     // uniform
                ctx = row[j];
                step(t0 + j);
            }
        }
    } else {
        for (int t = 0; t < fm.steps; ++t) step(t);
    }
    rans_verdict(x, st, pos, ok, fr, lane);
    ++fr;
    chained = true;
    } while (TMP && fr < last);                                    // the other forms: one frame
}

__global__ __launch_bounds__(RANS_LANES) void rans_decode_kernel(const uint16_t* __restrict__ words, long total, const long* __restrict__ offsets,
                                                                 const int* __restrict__ n_words, const unsigned* __restrict__ state,
                                                                 const uint16_t* __restrict__ freq, int8_t* __restrict__ codes,
                                                                 int* __restrict__ ok, long n, int steps, int nsym, int qmax)
{
    rans_decode_frame<RANS_STATIC>(words, total, offsets, n_words, state, freq, codes, ok, RansFrame{n, steps, nsym, qmax, 0, 0, 0, 0, 0},
                                   RansChains{});
}

// FULL: four slot tables of 4096 dwords (64 KB) in dynamic LDS; else a byte per slot (16 KB)
template <bool FULL>
__global__ __launch_bounds__(RANS_LANES) void rans_decode_ctx_kernel(const uint16_t* __restrict__ words, long total, const long* __restrict__ offsets,
                                                                     const int* __restrict__ n_words, const unsigned* __restrict__ state,
                                                                     const uint16_t* __restrict__ freq4, int8_t* __restrict__ codes,
                                                                     int* __restrict__ ok, int hw, int ld, int steps, int nsym, int qmax,
                                                                     int grid_w, int thr0, int thr1)
{
    rans_decode_frame<FULL ? RANS_CTX_FULL : RANS_CTX_COMPACT>(words, total, offsets, n_words, state, freq4, codes, ok,
                                                               RansFrame{(long)hw * ld, steps, nsym, qmax, hw, ld, grid_w, thr0, thr1},
                                                               RansChains{});
}

// blockIdx.x = chain; ch.start (chains + 1,), ch.frames and ch.thr
__global__ __launch_bounds__(RANS_LANES) void rans_decode_temporal_kernel(const uint16_t* __restrict__ words, long total,
                                                                          const long* __restrict__ offsets, const int* __restrict__ n_words,
                                                                          const unsigned* __restrict__ state, const uint16_t* __restrict__ freq9,
                                                                          int8_t* __restrict__ codes, int* __restrict__ ok, long n, int steps,
                                                                          int nsym, int qmax, RansChains ch)
{
    rans_decode_frame<RANS_TMP_COMPACT>(words, total, offsets, n_words, state, freq9, codes, ok, RansFrame{n, steps, nsym, qmax, 0, 0, 0, 0, 0}, ch);
}

}  // namespace

// ----------------------------------------------------------------------------------------------------------------------------- launchers
extern "C" int vvae_rans_supported(int hw, int ld, int bits)
{
    return bits >= 2 && bits <= 8 && hw >= 1 && ld >= 1 && (long)hw * ld <= RANS_MAX_FRAME;
}

extern "C" int vvae_rans_context_supported(int hw, int ld, int bits, int grid_w)
{
    return vvae_rans_supported(hw, ld, bits) && hw <= RANS_CTX_MAX_HW && grid_w >= 1 && (long)(grid_w - 1) * ld >= RANS_LANES - 1;
}

namespace {

// frames of hw x ld at ``bits`` (laid out grid_w wide with CTX) as the kernels take them, or false: no frame, an unsupported one, or a
// pointer of ``ptrs`` (address, alignment) that is missing or misaligned
template <bool CTX>
bool rans_frame(int frames, int hw, int ld, int bits, int grid_w, int thr0, int thr1, std::initializer_list<std::pair<const void*, int>> ptrs,
                RansFrame& fm)
{
    if (frames < 1 || !(CTX ? vvae_rans_context_supported(hw, ld, bits, grid_w) : vvae_rans_supported(hw, ld, bits))) return false;
    for (const auto& p : ptrs)
        if (!p.first || (uintptr_t)p.first % p.second) return false;
    const long n = (long)hw * ld;
    const int qmax = (1 << (bits - 1)) - 1;
    fm = {n, (int)((n + RANS_LANES - 1) / RANS_LANES), 2 * qmax + 1, qmax, hw, ld, grid_w, thr0, thr1};
    return true;
}

// the words of a decoder: none at all need no address
bool rans_words(const uint16_t* words, long total_words) { return total_words >= 0 && (words || total_words == 0) && (uintptr_t)words % 2 == 0; }

}  // namespace

// codes int8 (frames, hw, ld); keep fp32 (frames,); freq uint16 (2 qmax + 1,) summing to 4096, positive on every code that occurs in a
// kept frame; words uint16 (frames, ceil(hw ld / 64) 64); n_words int32 (frames,); state uint32 (frames, 64).
extern "C" int vvae_rans_encode(const int8_t* codes, const float* keep, const uint16_t* freq, uint16_t* words, int* n_words, uint32_t* state,
                                int frames, int hw, int ld, int bits, void* stream)
{
    RansFrame fm;
    if (!rans_frame<false>(frames, hw, ld, bits, 0, 0, 0, {{codes, 1}, {keep, 4}, {freq, 2}, {words, 2}, {n_words, 4}, {state, 4}}, fm))
        return VVAE_ERR_BAD_ARG;
    hipLaunchKernelGGL(rans_encode_kernel, dim3((unsigned)frames), dim3(RANS_LANES), 0, (hipStream_t)stream, codes, keep, freq, words, n_words,
                       state, fm.n, fm.steps, fm.nsym, fm.qmax);
    VVAE_LAUNCH_CHECK();
    return 0;
}

// vvae_rans_encode with freq4 uint16 (4, 2 qmax + 1), every row summing to 4096 and positive on every code that occurs in its context
extern "C" int vvae_rans_encode_ctx(const int8_t* codes, const float* keep, const uint16_t* freq4, uint16_t* words, int* n_words,
                                    uint32_t* state, int frames, int hw, int ld, int bits, int grid_w, int thr0, int thr1, void* stream)
{
    RansFrame fm;
    if (!rans_frame<true>(frames, hw, ld, bits, grid_w, thr0, thr1, {{codes, 1}, {keep, 4}, {freq4, 2}, {words, 2}, {n_words, 4}, {state, 4}}, fm))
        return VVAE_ERR_BAD_ARG;
    hipLaunchKernelGGL(rans_encode_ctx_kernel, dim3((unsigned)frames), dim3(RANS_LANES), 0, (hipStream_t)stream, codes, keep, freq4, words,
                       n_words, state, hw, ld, fm.steps, fm.nsym, fm.qmax, grid_w, thr0, thr1);
    VVAE_LAUNCH_CHECK();
    return 0;
}

// words uint16 (total_words,); offsets int64 (frames,), n_words int32 (frames,): frame f's stream is words[offsets[f] .. + n_words[f]);
// state uint32 (frames, 64); freq as above -> codes int8 (frames, hw, ld), ok int32 (frames,): 1 when the frame's stream lies inside
// words, every one of its words was consumed and every lane ended at L.
extern "C" int vvae_rans_decode(const uint16_t* words, long total_words, const long* offsets, const int* n_words, const uint32_t* state,
                                const uint16_t* freq, int8_t* codes, int* ok, int frames, int hw, int ld, int bits, void* stream)
{
    RansFrame fm;
    if (!rans_words(words, total_words) ||
        !rans_frame<false>(frames, hw, ld, bits, 0, 0, 0, {{offsets, 8}, {n_words, 4}, {state, 4}, {freq, 2}, {codes, 1}, {ok, 4}}, fm))
        return VVAE_ERR_BAD_ARG;
    hipLaunchKernelGGL(rans_decode_kernel, dim3((unsigned)frames), dim3(RANS_LANES), 0, (hipStream_t)stream, words, total_words, offsets, n_words,
                       state, freq, codes, ok, fm.n, fm.steps, fm.nsym, fm.qmax);
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
    RansFrame fm;
    if (!rans_words(words, total_words) || slot_form < -1 || slot_form > 1 ||
        !rans_frame<true>(frames, hw, ld, bits, grid_w, thr0, thr1, {{offsets, 8}, {n_words, 4}, {state, 4}, {freq4, 2}, {codes, 1}, {ok, 4}}, fm))
        return VVAE_ERR_BAD_ARG;
    if (slot_form < 0) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
        slot_form = frames <= cus ? 1 : 0;
    }
    if (slot_form == 1) {
        constexpr size_t dyn = (size_t)RANS_CTX * RANS_M * sizeof(unsigned);
        static const hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void*>(&rans_decode_ctx_kernel<true>),
                                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);       // once
        if (raised != hipSuccess) return (int)raised;
        hipLaunchKernelGGL(rans_decode_ctx_kernel<true>, dim3((unsigned)frames), dim3(RANS_LANES), dyn, (hipStream_t)stream, words, total_words,
                           offsets, n_words, state, freq4, codes, ok, hw, ld, fm.steps, fm.nsym, fm.qmax, grid_w, thr0, thr1);
    } else {
        hipLaunchKernelGGL(rans_decode_ctx_kernel<false>, dim3((unsigned)frames), dim3(RANS_LANES), 0, (hipStream_t)stream, words, total_words,
                           offsets, n_words, state, freq4, codes, ok, hw, ld, fm.steps, fm.nsym, fm.qmax, grid_w, thr0, thr1);
    }
    VVAE_LAUNCH_CHECK();
    return 0;
}

// codes int8 (frames, hw, ld); keep fp32 (frames,) -> counts int32 (frames, 4, 256): counts[f][ctx][code + 128]; zeros for a dropped frame
extern "C" int vvae_rans_context_counts(const int8_t* codes, const float* keep, int* counts, int frames, int hw, int ld, int bits, int grid_w,
                                        int thr0, int thr1, void* stream)
{
    RansFrame fm;
    if (!rans_frame<true>(frames, hw, ld, bits, grid_w, thr0, thr1, {{codes, 1}, {keep, 4}, {counts, 4}}, fm)) return VVAE_ERR_BAD_ARG;
    hipLaunchKernelGGL(rans_context_counts_kernel, dim3((unsigned)frames), dim3(RANS_COUNT_THREADS), 0, (hipStream_t)stream, codes, keep, counts,
                       hw, ld, grid_w, thr0, thr1);
    VVAE_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------- the temporal coder
extern "C" int vvae_rans_temporal_supported(int hw, int ld, int bits) { return vvae_rans_supported(hw, ld, bits); }

namespace {

// thr: 7 ascending integers on the HOST (kernel arguments, fixed in a captured graph)
bool rans_chains(const int* prev, const int* start, int frames, const int* thr, RansChains& ch)
{
    if (!thr) return false;
    ch = RansChains{prev, start, frames, {}};
    for (int k = 0; k < RANS_TMP_THR; ++k) {
        if (k && thr[k] < thr[k - 1]) return false;
        ch.thr.v[k] = thr[k];
    }
    return true;
}

}  // namespace

// codes int8 (frames, hw, ld); keep fp32 (frames,); prev int32 (frames,): the frame a kept frame is coded against (its table rows come
// from that frame's codes) or -1 for one that starts a chain -> counts int32 (frames, 9, 256): counts[f][row][code + 128]; zeros for a
// dropped frame, which is not read
extern "C" int vvae_rans_temporal_counts(const int8_t* codes, const float* keep, const int* prev, int* counts, int frames, int hw, int ld,
                                         int bits, const int* thr, void* stream)
{
    RansFrame fm;
    RansChains ch;
    if (!rans_frame<false>(frames, hw, ld, bits, 0, 0, 0, {{codes, 1}, {keep, 4}, {prev, 4}, {counts, 4}}, fm) ||
        !rans_chains(prev, nullptr, frames, thr, ch))
        return VVAE_ERR_BAD_ARG;
    hipLaunchKernelGGL(rans_temporal_counts_kernel, dim3((unsigned)frames), dim3(RANS_COUNT_THREADS), 0, (hipStream_t)stream, codes, keep, counts,
                       (int)fm.n, ch);
    VVAE_LAUNCH_CHECK();
    return 0;
}

// vvae_rans_encode with freq9 uint16 (9, 2 qmax + 1), every row summing to 4096 and positive on every code that occurs in it, and prev, thr
// as above.  One wavefront per frame: the encoder knows all codes, so chained frames are coded independently.
extern "C" int vvae_rans_encode_temporal(const int8_t* codes, const float* keep, const int* prev, const uint16_t* freq9, uint16_t* words,
                                         int* n_words, uint32_t* state, int frames, int hw, int ld, int bits, const int* thr, void* stream)
{
    RansFrame fm;
    RansChains ch;
    if (!rans_frame<false>(frames, hw, ld, bits, 0, 0, 0, {{codes, 1}, {keep, 4}, {prev, 4}, {freq9, 2}, {words, 2}, {n_words, 4}, {state, 4}},
                           fm) ||
        !rans_chains(prev, nullptr, frames, thr, ch))
        return VVAE_ERR_BAD_ARG;
    hipLaunchKernelGGL(rans_encode_temporal_kernel, dim3((unsigned)frames), dim3(RANS_LANES), 0, (hipStream_t)stream, codes, keep, freq9, words,
                       n_words, state, fm.n, fm.steps, fm.nsym, fm.qmax, ch);
    VVAE_LAUNCH_CHECK();
    return 0;
}

// vvae_rans_decode with freq9 and chain_start int32 (chains + 1,) on the device: chain c holds the frames chain_start[c] ..
// chain_start[c + 1] - 1, and the chains partition 0 .. frames - 1 (then every code and every ok is written).  One wavefront per chain,
// which decodes its frames in order; ok is one flag per frame, and a frame behind an invalid one is decoded from what that one produced.
// The slot tables are the compact form (a byte per slot, 36 KB, and a second read of tab[row][s]; 50 KB of LDS a wave).
extern "C" int vvae_rans_decode_temporal(const uint16_t* words, long total_words, const long* offsets, const int* n_words, const uint32_t* state,
                                         const uint16_t* freq9, int8_t* codes, int* ok, const int* chain_start, int chains, int frames, int hw,
                                         int ld, int bits, const int* thr, void* stream)
{
    RansFrame fm;
    RansChains ch;
    if (!rans_words(words, total_words) || chains < 1 || chains > frames ||
        !rans_frame<false>(frames, hw, ld, bits, 0, 0, 0, {{offsets, 8}, {n_words, 4}, {state, 4}, {freq9, 2}, {codes, 1}, {ok, 4}, {chain_start, 4}},
                           fm) ||
        !rans_chains(nullptr, chain_start, frames, thr, ch))
        return VVAE_ERR_BAD_ARG;
    hipLaunchKernelGGL(rans_decode_temporal_kernel, dim3((unsigned)chains), dim3(RANS_LANES), 0, (hipStream_t)stream, words, total_words, offsets,
                       n_words, state, freq9, codes, ok, fm.n, fm.steps, fm.nsym, fm.qmax, ch);
    VVAE_LAUNCH_CHECK();
    return 0;
}
