"""The entropy coder of the quantised latents: interleaved rANS, one static table per latent file.

Fixed parameters: 32-bit states, 16-bit renormalisation words, probability scale ``M = 2^12``, state lower bound ``L = 2^16``, 64 lanes
(one wavefront).  For one frame of codes ``q`` (hw, ld) int8 at ``bits`` in 2 .. 8, ``qmax = 2^(bits - 1) - 1``:

  * symbols ``s = q + qmax`` in 0 .. 2 qmax; the frame is flattened row-major to ``n = hw ld`` symbols; symbol ``i`` belongs to lane
    ``i mod 64`` and step ``i div 64``; a lane with ``i >= n`` in the last step is idle for that step;
  * the table ``freq`` uint16 (2 qmax + 1,) sums to exactly ``M`` (``normalise_counts``), ``cum`` is its exclusive prefix sum; it is stored
    with the stream, so a decoder never derives it again;
  * encode: every lane starts at ``x = L``; steps run from the last to the first; an active lane with ``x >= freq[s] << 20`` (a 64-bit
    comparison: ``freq[s] << 20`` is 2^32 when one symbol owns the table) emits ``x & 0xffff`` and shifts ``x >>= 16``, at most once per
    symbol; then ``x = ((x // f) << 12) + (x % f) + cum[s]``;
  * the frame's stream is the emitted words in the order the DECODER consumes them: steps ascending, within a step lanes ascending (the
    encoder produces exactly the reverse); the 64 final states are stored as uint32;
  * decode: from the stored states, for each step in ascending order ``slot = x & 4095``, ``s`` the symbol with ``cum[s] <= slot <
    cum[s] + freq[s]``, ``x = freq[s] (x >> 12) + slot - cum[s]``; then the active lanes with ``x < L`` take consecutive words in ascending
    lane order, ``x = (x << 16) | w``;
  * a valid stream ends with every word consumed and every lane back at ``L``; anything else raises ValueError.  A read past the frame's
    words yields 0 and never indexes outside it.

``encode_reference`` / ``decode_reference`` below are the definition (numpy, vectorised over lanes and frames); ``ops.rans_encode`` /
``ops.rans_decode`` (csrc/rans.hip) equal them on every word, count and state.
"""
from typing import NamedTuple

import numpy as np

from .quant import qmax_of

SCALE_BITS = 12
M = 1 << SCALE_BITS
L = 1 << 16
LANES = 64
STATE_BITS = LANES * 32 + 32          # a frame's states and its word count


class CodedFrames(NamedTuple):
    """Coded frames.  On the host (the definition, the latent files): ``words`` uint16 (total,), the frames' streams concatenated;
    ``n_words`` int64 (frames,); ``state`` uint32 (frames, 64).  ``ops.rans_encode`` returns GPU tensors in the capacity layout instead:
    ``words`` (frames, capacity) with frame f's stream in its last ``n_words[f]`` entries (``gather_streams`` brings them here)."""
    words: object
    n_words: object
    state: object


def table_size(bits):
    return 2 * qmax_of(bits) + 1


def capacity(n):
    """The most words a frame of ``n`` symbols can emit: one per symbol slot, ceil(n / 64) * 64."""
    return (int(n) + LANES - 1) // LANES * LANES


def normalise_counts(counts, bits):
    """The frequency table uint16 (2 qmax + 1,) of a code histogram ``counts`` (256,) or (frames, 256) (pooled; counts[q + 128], what
    the quantiser returns): with N the number of codes, ``max(1, c M // N)`` on every present symbol and 0 elsewhere, then the difference
    to M is added to or taken from the currently largest entry one unit at a time, never below 1; the lowest index wins ties.  Integer
    arithmetic only.  An empty histogram, or a code beyond +-qmax, raises ValueError."""
    qmax = qmax_of(bits)
    c = np.asarray(counts).astype(np.int64).reshape(-1, 256).sum(axis=0)
    if (c < 0).any():
        raise ValueError("normalise_counts: negative counts")
    inside = c[128 - qmax:128 + qmax + 1]
    n = int(inside.sum())
    if int(c.sum()) != n:
        raise ValueError(f"normalise_counts: codes beyond +-{qmax} in a histogram for {int(bits)} bits")
    if n == 0:
        raise ValueError("normalise_counts: an empty histogram has no table")
    freq = np.where(inside > 0, np.maximum(1, inside * M // n), 0).astype(np.int64)
    diff = M - int(freq.sum())
    while diff != 0:
        i = int(np.argmax(freq))                           # the first of the largest
        step = 1 if diff > 0 else -1
        if freq[i] + step < 1:
            raise ValueError("normalise_counts: cannot reach the scale")      # more symbols than M: impossible for 8 bits
        freq[i] += step
        diff -= step
    return freq.astype(np.uint16)


def _table(freq, bits):
    """(freq int64, cum int64 exclusive prefix, slot -> symbol int64 (M,)) of a stored table, checked."""
    f = np.asarray(freq)
    if f.ndim != 1 or f.shape[0] != table_size(bits) or f.dtype.kind not in "ui":
        raise ValueError(f"rANS table {f.dtype} {f.shape}: integers ({table_size(bits)},) expected for {int(bits)} bits")
    f = f.astype(np.int64)
    if (f < 0).any() or int(f.sum()) != M:
        raise ValueError(f"rANS table sums to {int(f.sum())}, not {M}")
    cum = np.concatenate([[0], np.cumsum(f)[:-1]]).astype(np.int64)
    return f, cum, np.repeat(np.arange(f.shape[0], dtype=np.int64), f)


def encode_reference(codes, freq, bits):
    """codes int8 (frames, hw, ld) (or one frame (hw, ld)) -> CodedFrames on the host.  A code outside the table's support raises."""
    qmax = qmax_of(bits)
    f, cum, _ = _table(freq, bits)
    q = np.asarray(codes)
    if q.ndim == 2:
        q = q[None]
    if q.ndim != 3 or q.dtype != np.int8:
        raise ValueError(f"codes {q.dtype} {q.shape}: int8 (frames, hw, ld) expected")
    frames, n = q.shape[0], q.shape[1] * q.shape[2]
    sym = q.reshape(frames, n).astype(np.int64) + qmax
    if sym.size and (sym.min() < 0 or sym.max() >= f.shape[0] or (f[sym] == 0).any()):
        raise ValueError("encode_reference: a code outside the table's support")
    steps = capacity(n) // LANES
    pad = np.zeros((frames, steps * LANES), dtype=np.int64)
    pad[:, :n] = sym
    pad = pad.reshape(frames, steps, LANES)
    active = (np.arange(steps * LANES) < n).reshape(steps, LANES)
    x = np.full((frames, LANES), L, dtype=np.uint64)
    emitted = np.zeros((frames, steps, LANES), dtype=np.uint16)
    flag = np.zeros((frames, steps, LANES), dtype=bool)
    for t in range(steps - 1, -1, -1):
        act = active[t][None]
        fs = np.where(act, f[pad[:, t]], 1).astype(np.uint64)                # an idle lane divides by 1 and keeps its state
        cs = cum[pad[:, t]].astype(np.uint64)
        emit = act & (x >= (fs << np.uint64(20)))          # 64 bits: fs << 20 may be 2^32
        emitted[:, t] = np.where(emit, x & np.uint64(0xffff), 0).astype(np.uint16)
        flag[:, t] = emit
        x = np.where(emit, x >> np.uint64(16), x)
        x = np.where(act, ((x // fs) << np.uint64(SCALE_BITS)) + (x % fs) + cs, x)
    n_words = flag.reshape(frames, steps * LANES).sum(axis=1).astype(np.int64)
    return CodedFrames(emitted[flag], n_words, x.astype(np.uint32))       # boolean indexing: frames, steps, lanes ascending


def _check_coded(coded):
    words, n_words, state = np.asarray(coded.words), np.asarray(coded.n_words), np.asarray(coded.state)
    if words.dtype != np.uint16 or words.ndim != 1 or n_words.ndim != 1 or n_words.dtype.kind not in "ui" or \
            state.dtype != np.uint32 or state.shape != (n_words.shape[0], LANES):
        raise ValueError(f"coded frames: words {words.dtype} {words.shape}, n_words {n_words.dtype} {n_words.shape}, state {state.dtype} "
                         f"{state.shape}: uint16 (total,), integers (frames,), uint32 (frames, {LANES}) expected")
    n_words = n_words.astype(np.int64)
    if (n_words < 0).any() or int(n_words.sum()) != words.shape[0]:
        raise ValueError(f"coded frames: {words.shape[0]} words for frames of {n_words.tolist()} words")
    return words, n_words, state


def decode_reference(coded, freq, bits, hw, ld):
    """CodedFrames on the host -> codes int8 (frames, hw, ld).  A frame that does not end with every word consumed and every lane at L
    raises ValueError naming it ("frame f", counted among the coded frames)."""
    qmax = qmax_of(bits)
    f, cum, slot_sym = _table(freq, bits)
    words, n_words, state = _check_coded(coded)
    frames, n = n_words.shape[0], int(hw) * int(ld)
    if n < 1:
        raise ValueError(f"frames of {hw} x {ld}")
    if (n_words > capacity(n)).any():
        raise ValueError(f"coded frames: more than {capacity(n)} words for a frame of {n} symbols")
    steps = capacity(n) // LANES
    width = max(int(n_words.max()) if frames else 0, 1)
    offsets = np.concatenate([[0], np.cumsum(n_words)[:-1]]).astype(np.int64) if frames else np.zeros(0, dtype=np.int64)
    padded = np.zeros((frames, width), dtype=np.int64)     # every frame's words in a row of its own, zeros behind them
    cols = np.arange(width)[None]
    have = cols < n_words[:, None]
    padded[have] = words[(offsets[:, None] + cols)[have]]
    active = (np.arange(steps * LANES) < n).reshape(steps, LANES)
    x = state.astype(np.int64)
    pos = np.zeros(frames, dtype=np.int64)
    out = np.zeros((frames, steps, LANES), dtype=np.int64)
    rows = np.arange(frames)[:, None]
    for t in range(steps):
        act = active[t][None]
        slot = x & (M - 1)
        s = slot_sym[slot]
        out[:, t] = s
        x = np.where(act, f[s] * (x >> SCALE_BITS) + slot - cum[s], x)
        need = act & (x < L)
        idx = pos[:, None] + np.cumsum(need, axis=1) - need
        w = np.where(idx < n_words[:, None], padded[rows, np.minimum(idx, width - 1)], 0)
        x = np.where(need, (x << 16) | w, x)
        pos += need.sum(axis=1)
    bad = np.nonzero((pos != n_words) | (x != L).any(axis=1))[0]
    if bad.size:
        b = int(bad[0])
        raise ValueError(f"rANS stream of frame {b} is not valid: {int(pos[b])} of {int(n_words[b])} words consumed, "
                         f"{int((x[b] != L).sum())} lanes not back at {L}")
    return (out.reshape(frames, steps * LANES)[:, :n] - qmax).astype(np.int8).reshape(frames, int(hw), int(ld))


def coded_bits(coded, freq):
    """The size in bits of coded frames with their table: 16 per word, 64 states of 32 bits and a 32-bit word count per frame, 16 per
    table entry."""
    words, n_words, _ = _check_coded(coded)
    return 16 * int(words.shape[0]) + int(n_words.shape[0]) * STATE_BITS + 16 * int(np.asarray(freq).shape[0])


def gather_streams(words, n_words, state, keep=None):
    """The capacity layout of ``ops.rans_encode`` (words (frames, capacity), frame f's stream in its last n_words[f] entries; tensors or
    arrays) -> CodedFrames on the host, of the frames whose ``keep`` flag is nonzero (all without it), in their order."""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    w, nw, st = host(words), host(n_words).astype(np.int64).reshape(-1), host(state)
    w = w.view(np.uint16) if w.dtype == np.int16 else w
    st = st.view(np.uint32) if st.dtype == np.int32 else st
    w, st = w.reshape(nw.shape[0], -1), st.reshape(nw.shape[0], LANES)
    k = np.ones(nw.shape[0], dtype=bool) if keep is None else host(keep).reshape(-1) != 0
    cap = w.shape[1]
    if (nw < 0).any() or (nw > cap).any():
        raise ValueError(f"word counts outside 0 .. {cap}")
    mask = (np.arange(cap)[None] >= cap - nw[:, None]) & k[:, None]
    return CodedFrames(np.ascontiguousarray(w[mask]), nw[k], np.ascontiguousarray(st[k]))
