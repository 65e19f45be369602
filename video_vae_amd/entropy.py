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
``_decode``, over tables of shape (K, 2 qmax + 1) and a table row per symbol: the static coder is K = 1 with row 0 everywhere.

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


def _decode(coded, tables, bits, hw, ld, grid_w=None, thr=None):
    """The decoder of both coders: CodedFrames on the host and ``tables`` of ``_table`` -> codes int8 (frames, hw, ld).  With ``grid_w``
    (the context coder) the energies of the decoded tokens are accumulated as the steps proceed and choose the row of every symbol;
    without it every symbol uses row 0."""
    qmax = qmax_of(bits)
    f, cum, slot_sym = tables
    words, n_words, state = _check_coded(coded)
    hw, ld = int(hw), int(ld)
    frames, n = n_words.shape[0], hw * ld
    if n < 1:
        raise ValueError(f"frames of {hw} x {ld}")
    if grid_w is not None:
        g = int(grid_w)
        thr0, thr1 = _check_context(hw, ld, bits, g, thr)
    if (n_words > capacity(n)).any():
        raise ValueError(f"coded frames: more than {capacity(n)} words for a frame of {n} symbols")
    steps = capacity(n) // LANES
    width = max(int(n_words.max()) if frames else 0, 1)
    offsets = np.concatenate([[0], np.cumsum(n_words)[:-1]]).astype(np.int64) if frames else np.zeros(0, dtype=np.int64)
    padded = np.zeros((frames, width), dtype=np.int64)     # every frame's words in a row of its own, zeros behind them
    cols = np.arange(width)[None]
    have = cols < n_words[:, None]
    padded[have] = words[(offsets[:, None] + cols)[have]]
    index = np.arange(steps * LANES).reshape(steps, LANES)
    active = index < n
    token = np.minimum(index // ld, hw - 1)                # an idle lane's token is never used
    x = state.astype(np.int64)
    pos = np.zeros(frames, dtype=np.int64)
    out = np.zeros((frames, steps, LANES), dtype=np.int64)
    energy = np.zeros((frames, hw), dtype=np.int64)
    rows = np.arange(frames)[:, None]
    ctx = np.zeros((frames, LANES), dtype=np.int64)
    for t in range(steps):
        act = active[t][None]
        if grid_w is not None:
            above = energy[:, np.maximum(token[t] - g, 0)]
            ctx = np.where((token[t] >= g)[None], 1 + (above > thr0) + (above > thr1), 0)
        slot = x & (M - 1)
        s = slot_sym[ctx, slot]
        out[:, t] = s
        if grid_w is not None:
            np.add.at(energy, (np.broadcast_to(rows, s.shape), np.broadcast_to(token[t][None], s.shape)), np.where(act, np.abs(s - qmax), 0))
        x = np.where(act, f[ctx, s] * (x >> SCALE_BITS) + slot - cum[ctx, s], x)
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
    return (out.reshape(frames, steps * LANES)[:, :n] - qmax).astype(np.int8).reshape(frames, hw, ld)


def decode_reference(coded, freq, bits, hw, ld):
    """CodedFrames on the host -> codes int8 (frames, hw, ld).  A frame that does not end with every word consumed and every lane at L
    raises ValueError naming it ("frame f", counted among the coded frames)."""
    return _decode(coded, _table(freq, bits), bits, hw, ld)


def coded_bits(coded, freq):
    """The size in bits of coded frames with their table: 16 per word, 64 states of 32 bits and a 32-bit word count per frame, 16 per
    table entry; a context stream (``freq`` (4, 2 qmax + 1)) pays for its four tables and 3 x 32 bits for grid_w and the thresholds."""
    words, n_words, _ = _check_coded(coded)
    f = np.asarray(freq)
    return 16 * int(words.shape[0]) + int(n_words.shape[0]) * STATE_BITS + 16 * int(f.size) + (CONTEXT_BITS if f.ndim == 2 else 0)


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
    c = np.asarray(counts).astype(np.int64).reshape(-1, CONTEXTS, 256).sum(axis=0)
    pooled = normalise_counts(c.sum(axis=0), bits)
    return np.stack([normalise_counts(c[k], bits) if c[k].sum() else pooled for k in range(CONTEXTS)])


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
