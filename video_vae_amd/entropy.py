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
``ops.rans_decode`` (csrc/rans.hip) equal them on every word, count and state.  Each recurrence is written once, in ``_encode`` and
``_decode_steps``, over tables of shape (K, 2 qmax + 1) and a table row per symbol: the static coder is K = 1 with row 0 everywhere.

The context coder (``encode_context_reference`` / ``decode_context_reference``; ``ops.rans_encode_context`` / ``ops.rans_decode_context``)
keeps all of the above and chooses the table of a symbol by the activity of the token ABOVE its own.  With ``grid_w`` the number of
token columns of the frame (token j sits in row ``j div grid_w``):

  * token energy ``E[j] = sum_c |q[j, c]|``, an integer;
  * every symbol of token j has the context ``0`` when ``j < grid_w`` (no token above), else ``1 + (E[j - grid_w] > thr0) +
    (E[j - grid_w] > thr1)``: ``K = 4`` contexts;
  * the thresholds ``(thr0, thr1)`` are integers stored with the stream (``context_thresholds``: the energies ``E[j]``, ``j < hw - grid_w``,
    of all coded frames pooled and sorted ascending, ``thr0 = pool[n // 3]``, ``thr1 = pool[2 n // 3]``; an empty pool gives 0, 0);
  * the table ``freq`` is uint16 (4, 2 qmax + 1), every row summing to ``M``: row k is ``normalise_counts`` of the symbols whose context
    is k, and a context without a symbol gets the pooled (static) table (``normalise_context_counts``); a symbol uses ``freq[ctx]`` /
    ``cum[ctx]`` in the recurrences above, and nothing else changes;
  * support: ``grid_w >= 1`` and ``(grid_w - 1) ld >= 63``.  Why: the last symbol of token ``j - grid_w`` has the index
    ``a = (j - grid_w + 1) ld - 1``, the first symbol of token j the index ``b = j ld``, and ``b - a = (grid_w - 1) ld + 1 >= 64``, so
    ``a div 64 < b div 64``: every symbol of the token above was decoded in an earlier step than any symbol of token j, and the decoder
    knows a step's contexts before the step.  ``hw`` need not be a multiple of ``grid_w``.

The temporal coder (``encode_temporal_reference`` / ``decode_temporal_reference``; ``ops.rans_encode_temporal`` /
``ops.rans_decode_temporal``) keeps all of the static coder (states, words, ``M``, ``L``, lanes, symbol order, stream order, the validity
rule, the read past the end) and chooses the table of a symbol by the code at the same place of the coded frame before it:

  * chains: the frames come in file order with one flag each, ``chain`` uint8: 1 when the frame is coded against the coded frame
    directly before it, 0 when it starts a chain; ``chain[0]`` is 0.  ``chain_flags(keep, period)`` makes them from a keep array
    (..., T): the last axis is time, every index of the leading axes a sequence of its own; a kept frame starts a chain when it is the
    first kept frame of its sequence or its chain already holds ``period`` frames;
  * classes: seven integer thresholds ``thr[0] <= ... <= thr[6]`` stored with the stream (``temporal_thresholds``: the codes of every
    frame that is the predecessor of a chained frame, pooled and sorted ascending, ``thr[k] = pool[(k + 1) n // 8]``; an empty pool gives
    zeros).  Only the pool's histogram matters: with C the inclusive prefix sum of its 256 bins, ``pool[i]`` is the least code q with
    ``C[q + 128] > i`` (``temporal_thresholds_of_counts``, from the quantiser's per-frame counts);
  * contexts: ``K = 9`` tables.  Every symbol of a frame that starts a chain uses row 0; symbol (j, c) of a chained frame uses row
    ``1 + #{k : q_prev[j, c] > thr[k]}`` with ``q_prev`` the predecessor's code at the same token and channel -- the same flat index, so
    the same lane and the same step.  A frame's rows are known before the frame starts: no support condition on the token grid;
  * the table ``freq`` is uint16 (9, 2 qmax + 1), every row summing to ``M``: row k is ``normalise_counts`` of the symbols of row k, and a
    row without a symbol gets the pooled table (``temporal_counts``, ``normalise_temporal_counts``).  With nine equal rows the stream is
    the static coder's, word for word, for any ``chain``;
  * decode goes by chain depth: every frame that starts a chain, then every frame at depth 1 with the rows its decoded predecessor
    gives, and so on.  A frame behind an invalid frame of its chain is decoded from whatever that frame produced; the ValueError names
    the first invalid frame in file order.
"""
from typing import NamedTuple

import numpy as np

from .quant import qmax_of

SCALE_BITS = 12
M = 1 << SCALE_BITS
L = 1 << 16
LANES = 64
STATE_BITS = LANES * 32 + 32          # a frame's states and its word count
CONTEXTS = 4                          # the tables of the context coder
CONTEXT_BITS = 3 * 32                 # grid_w and the two thresholds of a context stream
TEMPORAL_CLASSES = 8                  # the quantile classes of the previous frame's code
TEMPORAL_TABLES = 1 + TEMPORAL_CLASSES                     # row 0: the frames that start a chain
TEMPORAL_BITS = (TEMPORAL_CLASSES - 1) * 32                # the thresholds of a temporal stream (and a chain bit per frame)


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


def _table(freq, bits, contexts=None):
    """(freq int64 (K, nsym), cum int64 (K, nsym) exclusive prefix, slot -> symbol int64 (K, M)) of a stored table, every row checked:
    one table (nsym,) (K = 1), or with ``contexts`` the context coder's (contexts, nsym)."""
    f = np.asarray(freq)
    if contexts is not None and (f.ndim != 2 or f.shape[0] != contexts):
        raise ValueError(f"rANS context tables {f.dtype} {f.shape}: integers ({contexts}, {table_size(bits)}) expected")
    rows = []
    for r in (f[None] if contexts is None else f):
        if r.ndim != 1 or r.shape[0] != table_size(bits) or r.dtype.kind not in "ui":
            raise ValueError(f"rANS table {r.dtype} {r.shape}: integers ({table_size(bits)},) expected for {int(bits)} bits")
        r = r.astype(np.int64)
        if (r < 0).any() or int(r.sum()) != M:
            raise ValueError(f"rANS table sums to {int(r.sum())}, not {M}")
        rows.append((r, np.concatenate([[0], np.cumsum(r)[:-1]]).astype(np.int64), np.repeat(np.arange(r.shape[0], dtype=np.int64), r)))
    return tuple(np.stack([r[i] for r in rows]) for i in range(3))


def _frames_of(codes):
    q = np.asarray(codes)
    if q.ndim == 2:
        q = q[None]
    if q.ndim != 3 or q.dtype != np.int8:
        raise ValueError(f"codes {q.dtype} {q.shape}: int8 (frames, hw, ld) expected")
    return q


def _encode(q, tables, ctx, bits, refusal):
    """The encoder of both coders: codes ``q`` int8 (frames, hw, ld), ``tables`` of ``_table`` with K rows, ``ctx`` int64 (frames, n) the
    row of every symbol (all 0: the static coder) -> CodedFrames on the host."""
    f, cum, _ = tables
    frames, n = q.shape[0], q.shape[1] * q.shape[2]
    sym = q.reshape(frames, n).astype(np.int64) + qmax_of(bits)
    if sym.size and (sym.min() < 0 or sym.max() >= f.shape[1] or (f[ctx, sym] == 0).any()):
        raise ValueError(refusal)
    steps = capacity(n) // LANES
    fpad = np.ones((frames, steps * LANES), dtype=np.uint64)              # an idle lane divides by 1 and keeps its state
    cpad = np.zeros((frames, steps * LANES), dtype=np.uint64)
    fpad[:, :n] = f[ctx, sym]
    cpad[:, :n] = cum[ctx, sym]
    fpad, cpad = fpad.reshape(frames, steps, LANES), cpad.reshape(frames, steps, LANES)
    active = (np.arange(steps * LANES) < n).reshape(steps, LANES)
    x = np.full((frames, LANES), L, dtype=np.uint64)
    emitted = np.zeros((frames, steps, LANES), dtype=np.uint16)
    flag = np.zeros((frames, steps, LANES), dtype=bool)
    for t in range(steps - 1, -1, -1):
        act = active[t][None]
        fs, cs = fpad[:, t], cpad[:, t]
        emit = act & (x >= (fs << np.uint64(20)))          # 64 bits: fs << 20 may be 2^32
        emitted[:, t] = np.where(emit, x & np.uint64(0xffff), 0).astype(np.uint16)
        flag[:, t] = emit
        x = np.where(emit, x >> np.uint64(16), x)
        x = np.where(act, ((x // fs) << np.uint64(SCALE_BITS)) + (x % fs) + cs, x)
    n_words = flag.reshape(frames, steps * LANES).sum(axis=1).astype(np.int64)
    return CodedFrames(emitted[flag], n_words, x.astype(np.uint32))       # boolean indexing: frames, steps, lanes ascending


def encode_reference(codes, freq, bits):
    """codes int8 (frames, hw, ld) (or one frame (hw, ld)) -> CodedFrames on the host.  A code outside the table's support raises."""
    tables = _table(freq, bits)
    q = _frames_of(codes)
    ctx = np.zeros((q.shape[0], q.shape[1] * q.shape[2]), dtype=np.int64)
    return _encode(q, tables, ctx, bits, "encode_reference: a code outside the table's support")


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


def _stream_rows(coded, hw, ld):
    """CodedFrames on the host, checked for frames of ``hw`` x ``ld`` -> (every frame's words in a row of its own, zeros behind them,
    int64 (frames, width); n_words int64 (frames,); state int64 (frames, 64))."""
    words, n_words, state = _check_coded(coded)
    frames, n = n_words.shape[0], int(hw) * int(ld)
    if n < 1:
        raise ValueError(f"frames of {int(hw)} x {int(ld)}")
    if (n_words > capacity(n)).any():
        raise ValueError(f"coded frames: more than {capacity(n)} words for a frame of {n} symbols")
    width = max(int(n_words.max()) if frames else 0, 1)
    offsets = np.concatenate([[0], np.cumsum(n_words)[:-1]]).astype(np.int64) if frames else np.zeros(0, dtype=np.int64)
    padded = np.zeros((frames, width), dtype=np.int64)
    cols = np.arange(width)[None]
    have = cols < n_words[:, None]
    padded[have] = words[(offsets[:, None] + cols)[have]]
    return padded, n_words, state.astype(np.int64)


def _decode_steps(padded, n_words, state, tables, bits, hw, ld, grid_w=None, thr=None, rows=None):
    """The decoder's recurrence over the frames of ``_stream_rows`` -> (codes int8 (frames, hw, ld), words consumed int64 (frames,), final
    states int64 (frames, 64)); the caller judges them (``_verdict``).  The table row of a symbol: with ``grid_w`` (the context coder) the
    energies of the decoded tokens are accumulated as the steps proceed and choose it; with ``rows`` int64 (frames, n) (the temporal
    coder: known before the frame starts) it is given; else row 0."""
    qmax = qmax_of(bits)
    f, cum, slot_sym = tables
    hw, ld = int(hw), int(ld)
    frames, n, width = n_words.shape[0], hw * ld, padded.shape[1]
    if grid_w is not None:
        g = int(grid_w)
        thr0, thr1 = _check_context(hw, ld, bits, g, thr)
    steps = capacity(n) // LANES
    index = np.arange(steps * LANES).reshape(steps, LANES)
    active = index < n
    token = np.minimum(index // ld, hw - 1)                # an idle lane's token is never used
    x = state
    pos = np.zeros(frames, dtype=np.int64)
    out = np.zeros((frames, steps, LANES), dtype=np.int64)
    energy = np.zeros((frames, hw), dtype=np.int64)
    frame = np.arange(frames)[:, None]
    ctx = np.zeros((frames, LANES), dtype=np.int64)
    if rows is not None:
        given = np.zeros((frames, steps * LANES), dtype=np.int64)          # an idle lane reads row 0 and keeps its state
        given[:, :n] = rows
        given = given.reshape(frames, steps, LANES)
    for t in range(steps):
        act = active[t][None]
        if grid_w is not None:
            above = energy[:, np.maximum(token[t] - g, 0)]
            ctx = np.where((token[t] >= g)[None], 1 + (above > thr0) + (above > thr1), 0)
        elif rows is not None:
            ctx = given[:, t]
        slot = x & (M - 1)
        s = slot_sym[ctx, slot]
        out[:, t] = s
        if grid_w is not None:
            np.add.at(energy, (np.broadcast_to(frame, s.shape), np.broadcast_to(token[t][None], s.shape)), np.where(act, np.abs(s - qmax), 0))
        x = np.where(act, f[ctx, s] * (x >> SCALE_BITS) + slot - cum[ctx, s], x)
        need = act & (x < L)
        idx = pos[:, None] + np.cumsum(need, axis=1) - need
        w = np.where(idx < n_words[:, None], padded[frame, np.minimum(idx, width - 1)], 0)
        x = np.where(need, (x << 16) | w, x)
        pos = pos + need.sum(axis=1)
    return (out.reshape(frames, steps * LANES)[:, :n] - qmax).astype(np.int8).reshape(frames, hw, ld), pos, x


def _verdict(pos, n_words, x):
    """A valid frame consumed every word and brought every lane back to L; the first that did not raises ValueError naming it."""
    bad = np.nonzero((pos != n_words) | (x != L).any(axis=1))[0]
    if bad.size:
        b = int(bad[0])
        raise ValueError(f"rANS stream of frame {b} is not valid: {int(pos[b])} of {int(n_words[b])} words consumed, "
                         f"{int((x[b] != L).sum())} lanes not back at {L}")


def _decode(coded, tables, bits, hw, ld, grid_w=None, thr=None):
    """The decoder of the static and the context coder: CodedFrames on the host and ``tables`` of ``_table`` -> codes int8 (frames, hw,
    ld).  Frames are independent: all of them take every step together."""
    padded, n_words, state = _stream_rows(coded, hw, ld)
    codes, pos, x = _decode_steps(padded, n_words, state, tables, bits, hw, ld, grid_w, thr)
    _verdict(pos, n_words, x)
    return codes


def decode_reference(coded, freq, bits, hw, ld):
    """CodedFrames on the host -> codes int8 (frames, hw, ld).  A frame that does not end with every word consumed and every lane at L
    raises ValueError naming it ("frame f", counted among the coded frames)."""
    return _decode(coded, _table(freq, bits), bits, hw, ld)


def coded_bits(coded, freq):
    """The size in bits of coded frames with their table: 16 per word, 64 states of 32 bits and a 32-bit word count per frame, 16 per
    table entry; a context stream (``freq`` (4, 2 qmax + 1)) pays for its four tables and 3 x 32 bits for grid_w and the thresholds; a
    temporal stream (``freq`` (9, 2 qmax + 1)) for its nine tables, 7 x 32 bits for the thresholds and one chain bit per frame."""
    words, n_words, _ = _check_coded(coded)
    f = np.asarray(freq)
    frames = int(n_words.shape[0])
    model = 0 if f.ndim != 2 else (TEMPORAL_BITS + frames if f.shape[0] == TEMPORAL_TABLES else CONTEXT_BITS)
    return 16 * int(words.shape[0]) + frames * STATE_BITS + 16 * int(f.size) + model


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


# ------------------------------------------------------------------------------------------------------------- the context coder
def context_supported(hw, ld, bits, grid_w):
    """Does the context coder's format take frames of ``hw`` x ``ld`` at ``bits`` laid out ``grid_w`` tokens wide (the module docstring's
    support condition)?"""
    return 2 <= int(bits) <= 8 and int(hw) >= 1 and int(ld) >= 1 and int(grid_w) >= 1 and (int(grid_w) - 1) * int(ld) >= LANES - 1


def _check_context(hw, ld, bits, grid_w, thr):
    if not context_supported(hw, ld, bits, grid_w):
        raise ValueError(f"context coder: frames of {hw} x {ld} at {bits} bits, {grid_w} tokens wide: grid_w >= 1 and (grid_w - 1) ld >= "
                         f"{LANES - 1} expected")
    t = np.asarray(thr)
    if t.shape != (2,) or t.dtype.kind not in "ui":
        raise ValueError(f"context coder: thresholds {t.dtype} {t.shape}: two integers expected")
    return int(t[0]), int(t[1])


def token_energy(codes):
    """codes int8 (..., hw, ld) -> int64 (..., hw): ``sum_c |q[j, c]|``."""
    q = np.asarray(codes)
    if q.dtype != np.int8 or q.ndim < 2:
        raise ValueError(f"codes {q.dtype} {q.shape}: int8 (..., hw, ld) expected")
    return np.abs(q.astype(np.int64)).sum(axis=-1)


def context_thresholds(energy, grid_w):
    """(thr0, thr1) of the coded frames' token energies (frames, hw) (or one frame (hw,)): the energies of the tokens that have a token
    below them (j < hw - grid_w), pooled and sorted ascending, at a third and at two thirds; (0, 0) for an empty pool."""
    e = np.asarray(energy).astype(np.int64)
    e = e.reshape(-1, e.shape[-1]) if e.ndim else e.reshape(0, 0)
    pool = np.sort(e[:, :max(e.shape[1] - int(grid_w), 0)].reshape(-1))
    n = pool.shape[0]
    return (int(pool[n // 3]), int(pool[2 * n // 3])) if n else (0, 0)


def token_contexts(energy, grid_w, thr):
    """The context 0 .. 3 of every token: energy int (..., hw) -> int64 (..., hw)."""
    e = np.asarray(energy).astype(np.int64)
    g = int(grid_w)
    if g < 1:
        raise ValueError(f"grid_w {g}")
    ctx = np.zeros(e.shape, dtype=np.int64)
    if e.shape[-1] > g:
        above = e[..., :e.shape[-1] - g]
        ctx[..., g:] = 1 + (above > int(thr[0])) + (above > int(thr[1]))
    return ctx


def context_counts(codes, grid_w, thr):
    """codes int8 (frames, hw, ld) (or one frame) -> int64 (frames, 4, 256): counts[f, ctx, q + 128], the quantiser's histogram layout
    split by context."""
    q = np.asarray(codes)
    if q.ndim == 2:
        q = q[None]
    if q.ndim != 3 or q.dtype != np.int8:
        raise ValueError(f"codes {q.dtype} {q.shape}: int8 (frames, hw, ld) expected")
    ctx = token_contexts(token_energy(q), grid_w, thr)
    out = np.zeros((q.shape[0], CONTEXTS, 256), dtype=np.int64)
    frame = np.broadcast_to(np.arange(q.shape[0])[:, None, None], q.shape)
    np.add.at(out, (frame, np.broadcast_to(ctx[:, :, None], q.shape), q.astype(np.int64) + 128), 1)
    return out


def normalise_context_counts(counts, bits):
    """The tables uint16 (4, 2 qmax + 1) of context histograms (4, 256) or (frames, 4, 256) (pooled): row k is ``normalise_counts`` of
    context k; a context without a symbol gets the table of all contexts pooled.  No symbol at all raises ValueError."""
    return _normalise_rows(counts, bits, CONTEXTS)


def _normalise_rows(counts, bits, contexts):
    c = np.asarray(counts).astype(np.int64).reshape(-1, contexts, 256).sum(axis=0)
    pooled = normalise_counts(c.sum(axis=0), bits)
    return np.stack([normalise_counts(c[k], bits) if c[k].sum() else pooled for k in range(contexts)])


def encode_context_reference(codes, freq4, bits, grid_w, thr):
    """codes int8 (frames, hw, ld) (or one frame (hw, ld)) -> CodedFrames on the host, every symbol coded with the table of its context.
    A code outside its table's support raises."""
    tables = _table(freq4, bits, CONTEXTS)
    q = _frames_of(codes)
    thr = _check_context(q.shape[1], q.shape[2], bits, grid_w, thr)
    ctx = np.repeat(token_contexts(token_energy(q), grid_w, thr), q.shape[2], axis=1)
    return _encode(q, tables, ctx, bits, "encode_context_reference: a code outside its table's support")


def decode_context_reference(coded, freq4, bits, hw, ld, grid_w, thr):
    """CodedFrames on the host -> codes int8 (frames, hw, ld).  The energies of the decoded tokens are accumulated as the steps proceed; a
    step's contexts come from tokens that earlier steps completed (the support condition).  A frame that does not end with every word
    consumed and every lane at L raises ValueError naming it ("frame f", counted among the coded frames)."""
    return _decode(coded, _table(freq4, bits, CONTEXTS), bits, hw, ld, grid_w, thr)


# ------------------------------------------------------------------------------------------------------------ the temporal coder
class TemporalModel(NamedTuple):
    """What a temporal stream stores beside its tables: ``thr`` int64 (7,) and ``chain`` uint8 (coded frames,)."""
    thr: object
    chain: object


def chain_flags(keep, period):
    """The chain flags uint8 of the kept frames of ``keep`` (..., T) (tensor or array, nonzero = kept; the last axis is time, every index
    of the leading axes a sequence of its own), in row-major order: 0 on the first kept frame of a sequence and on every kept frame whose
    chain already holds ``period`` frames, 1 elsewhere.  Dropped frames do not break a chain."""
    period = int(period)
    if period < 1:
        raise ValueError(f"chain period {period}: at least 1 expected")
    k = (keep.detach().cpu().numpy() if hasattr(keep, "detach") else np.asarray(keep)) != 0
    if k.ndim < 1:
        raise ValueError("chain_flags: keep (..., T) expected")
    k = k.reshape(-1, k.shape[-1])
    rank = np.cumsum(k, axis=1) - 1                        # a kept frame's place among the kept frames of its sequence
    return (rank[k] % period != 0).astype(np.uint8)


def _check_chain(chain, frames):
    """The chain flags of ``frames`` coded frames as a bool array; a chain cannot start behind nothing."""
    c = np.asarray(chain)
    if c.ndim != 1 or c.shape[0] != int(frames) or c.dtype.kind not in "uib":
        raise ValueError(f"temporal coder: chain flags {c.dtype} {c.shape}: one integer per coded frame ({int(frames)},) expected")
    if c.size and (int(c[0]) != 0 or int(c.min()) < 0 or int(c.max()) > 1):
        raise ValueError("temporal coder: chain flags must be 0 or 1 and the first frame starts a chain")
    return c != 0


def _check_thresholds(thr):
    t = np.asarray(thr)
    if t.shape != (TEMPORAL_CLASSES - 1,) or t.dtype.kind not in "ui":
        raise ValueError(f"temporal coder: thresholds {t.dtype} {t.shape}: {TEMPORAL_CLASSES - 1} integers expected")
    t = t.astype(np.int64)
    if (np.diff(t) < 0).any() or int(t.min()) < -(1 << 31) or int(t.max()) >= 1 << 31:
        raise ValueError(f"temporal coder: thresholds {t.tolist()} must ascend and fit 32 bits")
    return t


def chain_starts(chain):
    """int32 (chains + 1,): chain c holds the coded frames chain_starts[c] .. chain_starts[c + 1] - 1 (a chain's frames are contiguous)."""
    c = _check_chain(chain, np.asarray(chain).shape[0])
    return np.concatenate([np.nonzero(~c)[0], [c.shape[0]]]).astype(np.int32)


def chain_prev(keep, chain):
    """int32, one per frame of ``keep`` (any shape, row-major): the flat index of the frame a kept, chained frame is coded against (the
    kept frame directly before it), -1 for a frame that starts a chain or is dropped."""
    k = ((keep.detach().cpu().numpy() if hasattr(keep, "detach") else np.asarray(keep)) != 0).reshape(-1)
    at = np.nonzero(k)[0]
    c = _check_chain(chain, at.shape[0])
    prev = np.full(k.shape[0], -1, dtype=np.int32)
    prev[at[c]] = at[np.nonzero(c)[0] - 1]
    return prev


def temporal_thresholds(codes, chain):
    """thr int64 (7,) of the coded frames ``codes`` int8 (frames, hw, ld): the codes of every frame that is the predecessor of a chained
    frame, pooled and sorted ascending, ``thr[k] = pool[(k + 1) n // 8]``; zeros for an empty pool.  The definition;
    ``temporal_thresholds_of_counts`` computes the same from the frames' histograms."""
    q = _frames_of(codes)
    c = _check_chain(chain, q.shape[0])
    pool = np.sort(q[np.nonzero(c)[0] - 1].reshape(-1).astype(np.int64))
    n = pool.shape[0]
    return pool[(np.arange(1, TEMPORAL_CLASSES) * n) // TEMPORAL_CLASSES] if n else np.zeros(TEMPORAL_CLASSES - 1, dtype=np.int64)


def temporal_thresholds_of_counts(counts, chain):
    """``temporal_thresholds`` from the frames' code histograms ``counts`` (frames, 256) (counts[f, q + 128], what the quantiser returns
    per frame): only the pool's histogram matters.  With C its inclusive prefix sum, pool[i] is the least code q with C[q + 128] > i."""
    h = np.asarray(counts).astype(np.int64)
    if h.ndim != 2 or h.shape[1] != 256:
        raise ValueError(f"code histograms {h.shape}: (frames, 256) expected")
    c = _check_chain(chain, h.shape[0])
    cum = np.cumsum(h[np.nonzero(c)[0] - 1].sum(axis=0))
    n = int(cum[-1])
    if n == 0:
        return np.zeros(TEMPORAL_CLASSES - 1, dtype=np.int64)
    return np.searchsorted(cum, (np.arange(1, TEMPORAL_CLASSES) * n) // TEMPORAL_CLASSES, side="right").astype(np.int64) - 128


def temporal_contexts(codes, chain, thr):
    """The table row 0 .. 8 of every symbol: codes int8 (frames, hw, ld) -> int64 (frames, hw ld).  0 in a frame that starts a chain; in a
    chained frame ``1 + #{k : q_prev > thr[k]}`` with q_prev the previous frame's code at the same token and channel."""
    q = _frames_of(codes)
    c = _check_chain(chain, q.shape[0])
    t = _check_thresholds(thr)
    flat = q.reshape(q.shape[0], -1).astype(np.int64)
    ctx = np.zeros(flat.shape, dtype=np.int64)
    at = np.nonzero(c)[0]
    ctx[at] = 1 + (flat[at - 1][:, :, None] > t).sum(axis=2)
    return ctx


def temporal_counts(codes, chain, thr):
    """codes int8 (frames, hw, ld) -> int64 (frames, 9, 256): counts[f, row, q + 128], the quantiser's histogram layout split by row."""
    q = _frames_of(codes)
    ctx = temporal_contexts(q, chain, thr)
    out = np.zeros((q.shape[0], TEMPORAL_TABLES, 256), dtype=np.int64)
    np.add.at(out, (np.broadcast_to(np.arange(q.shape[0])[:, None], ctx.shape), ctx, q.reshape(ctx.shape).astype(np.int64) + 128), 1)
    return out


def normalise_temporal_counts(counts, bits):
    """The tables uint16 (9, 2 qmax + 1) of row histograms (9, 256) or (frames, 9, 256) (pooled), as ``normalise_context_counts``: a row
    without a symbol gets the table of all rows pooled.  No symbol at all raises ValueError."""
    return _normalise_rows(counts, bits, TEMPORAL_TABLES)


def encode_temporal_reference(codes, freq9, bits, chain, thr):
    """codes int8 (frames, hw, ld) in file order -> CodedFrames on the host, every symbol coded with the table of its row
    (``temporal_contexts``).  The encoder knows all codes, so its frames are independent.  A code outside its table's support raises."""
    tables = _table(freq9, bits, TEMPORAL_TABLES)
    q = _frames_of(codes)
    return _encode(q, tables, temporal_contexts(q, chain, thr), bits, "encode_temporal_reference: a code outside its table's support")


def decode_temporal_reference(coded, freq9, bits, hw, ld, chain, thr):
    """CodedFrames on the host -> codes int8 (frames, hw, ld), by chain depth: every frame that starts a chain, then every frame at depth
    1 with the rows its decoded predecessor gives, and so on.  A frame behind an invalid frame of its chain is decoded from whatever that
    frame produced; the ValueError names the first invalid frame in file order ("frame f", counted among the coded frames)."""
    tables = _table(freq9, bits, TEMPORAL_TABLES)
    padded, n_words, state = _stream_rows(coded, hw, ld)
    frames = n_words.shape[0]
    c = _check_chain(chain, frames)
    t = _check_thresholds(thr)
    depth = np.arange(frames) - np.maximum.accumulate(np.where(c, 0, np.arange(frames))) if frames else np.zeros(0, dtype=np.int64)
    codes = np.zeros((frames, int(hw), int(ld)), dtype=np.int8)
    pos, x = np.zeros(frames, dtype=np.int64), state.copy()
    for d in range(int(depth.max()) + 1 if frames else 0):
        at = np.nonzero(depth == d)[0]
        before = codes[at - 1].reshape(at.shape[0], -1).astype(np.int64)
        rows = 1 + (before[:, :, None] > t).sum(axis=2) if d else np.zeros(before.shape, dtype=np.int64)
        codes[at], pos[at], x[at] = _decode_steps(padded[at], n_words[at], state[at], tables, bits, hw, ld, rows=rows)
    _verdict(pos, n_words, x)
    return codes
