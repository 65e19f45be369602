"""The latent files of ``infer encode``: one ``.npz`` per clip, in three formats (plain, tiled, windowed) that differ in their header
keys and in the shape of ``selection``.

Every format stores the means of the kept frames only, in the row-major order of its selection: ``mean`` float32 (lossless from bf16),
or with ``quant`` the ``mean_q`` int8 codes, ``mean_step`` and ``quant_bits`` of quant.py, or with ``entropy`` too those codes range-coded (entropy.py):
``mean_ans`` / ``ans_words`` / ``ans_state`` / ``ans_freq`` / ``ans_shape`` in place of ``mean_q`` (the context coder: ``ans_freq`` (4, nsym) and
``ans_ctx`` int64 [grid_w, thr0, thr1] behind ``ans_shape``; the temporal coder: ``ans_freq`` (9, nsym), ``ans_tthr`` int64 (7,) and ``ans_chain`` uint8
(kept,) behind ``ans_shape``); ``selection`` uint8; ``log_variance`` of the kept frames when given.  Unpacking gives the dense compressed representation float32, shaped like the selection + (hw, ld): the stored
means on the kept frames, the fill token on the others (VideoVAE's latent gate with z = mean).  ``np.savez`` writes the members in the
order of the dict, so the key order of the packers is part of the format.
"""
import os

import numpy as np
import torch

from .entropy import (CONTEXTS, TEMPORAL_TABLES, CodedFrames, LANES, TemporalModel, _check_chain, _check_coded, _check_context,
                      _check_thresholds, _table, decode_context_reference, decode_reference, decode_temporal_reference)
from .quant import dequantise_reference, qmax_of
from .tiling import ScenePlan, TileGrid, WindowPlan


def _mean_arrays(mean, sel, quant, entropy=None):
    """The arrays that hold the kept means: ``mean`` float32, or with ``quant = (codes, step, bits)`` (dense, shaped like mean and like
    mean without its token axis) ``mean_q`` int8 (kept, hw, ld), ``mean_step`` float32 (kept, ld) and ``quant_bits``, rows in mean's order.
    ``entropy = (CodedFrames, freq)`` (with ``quant``; the coded KEPT frames on the host, in the rows' order, and their table): in place
    of ``mean_q``, ``mean_ans`` uint16 (the streams concatenated), ``ans_words`` uint32 (kept,), ``ans_state`` uint32 (kept, 64),
    ``ans_freq`` uint16 and ``ans_shape`` int64 [hw, ld].  ``entropy = (CodedFrames, freq4, (grid_w, thr0, thr1))``: the context coder's
    stream; ``ans_freq`` is (4, nsym) and ``ans_ctx`` int64 [grid_w, thr0, thr1] follows ``ans_shape``.  ``entropy = (CodedFrames, freq9,
    entropy.TemporalModel(thr, chain))``: the temporal coder's stream; ``ans_freq`` is (9, nsym), and ``ans_tthr`` int64 (7,) and ``ans_chain``
    uint8 (kept,) follow ``ans_shape``."""
    if entropy is not None and quant is None:
        raise ValueError("entropy-coded latents need quant: the coder codes the quantiser's codes")
    if quant is None:
        return {"mean": torch.as_tensor(mean).detach().float().cpu().numpy()[sel]}
    codes, step, bits = quant
    qmax_of(bits)
    codes = torch.as_tensor(codes).detach().cpu().numpy()
    step = torch.as_tensor(step).detach().float().cpu().numpy()
    if codes.dtype != np.int8 or codes.shape[:sel.ndim] != sel.shape or codes.ndim != sel.ndim + 2:
        raise ValueError(f"quantised codes {codes.dtype} {codes.shape}: int8 {sel.shape} + (hw, ld) expected")
    if step.shape != sel.shape + codes.shape[-1:]:
        raise ValueError(f"quantiser steps {step.shape}: {sel.shape + codes.shape[-1:]} expected")
    rest = {"mean_step": step[sel].astype(np.float32), "quant_bits": np.int64(bits)}
    if entropy is None:
        return {"mean_q": codes[sel], **rest}
    coded, freq = entropy[:2]
    words, n_words, state = _check_coded(coded)
    context = {}
    if len(entropy) == 3 and isinstance(entropy[2], TemporalModel):
        _table(freq, bits, TEMPORAL_TABLES)
        context["ans_tthr"] = _check_thresholds(entropy[2].thr)
        context["ans_chain"] = _check_chain(entropy[2].chain, n_words.shape[0]).astype(np.uint8)
    elif len(entropy) == 3:
        ctx = np.array([int(v) for v in entropy[2]], dtype=np.int64)
        _table(freq, bits, CONTEXTS)
        _check_context(codes.shape[-2], codes.shape[-1], bits, ctx[0], ctx[1:])
        context["ans_ctx"] = ctx
    else:
        _table(freq, bits)
    if n_words.shape[0] != int(sel.sum()):
        raise ValueError(f"entropy-coded latents: {n_words.shape[0]} coded frames for {int(sel.sum())} kept frames")
    return {"mean_ans": words, "ans_words": n_words.astype(np.uint32), "ans_state": state, "ans_freq": np.asarray(freq).astype(np.uint16),
            "ans_shape": np.array(codes.shape[-2:], dtype=np.int64), **context, **rest}


def coded_members(arrays):
    """(CodedFrames on the host, freq, bits, hw, ld) of a latent file with ``mean_ans``, its members checked for type and shape; a file
    of the context coder (``ans_ctx``): (CodedFrames, freq4, bits, hw, ld, grid_w, (thr0, thr1)); a file of the temporal coder
    (``ans_chain``): (CodedFrames, freq9, bits, hw, ld, entropy.TemporalModel), its chain flags checked against its frames."""
    shape = np.asarray(arrays["ans_shape"]).reshape(-1)
    state = np.asarray(arrays["ans_state"])
    if shape.shape[0] != 2 or int(shape.min()) < 1 or state.dtype != np.uint32:
        raise ValueError(f"entropy-coded latent file: ans_shape {shape.tolist()}, ans_state {state.dtype}")
    coded = CodedFrames(np.asarray(arrays["mean_ans"]), np.asarray(arrays["ans_words"]).astype(np.int64), state.reshape(-1, LANES))
    _check_coded(coded)
    bits = int(arrays["quant_bits"])
    freq = np.asarray(arrays["ans_freq"])
    if "ans_chain" in arrays:
        _table(freq, bits, TEMPORAL_TABLES)
        try:
            model = TemporalModel(_check_thresholds(np.asarray(arrays["ans_tthr"]).reshape(-1)),
                                  _check_chain(np.asarray(arrays["ans_chain"]), coded.n_words.shape[0]).astype(np.uint8))
        except ValueError as e:
            raise ValueError(f"entropy-coded latent file: {e}") from None
        return coded, freq, bits, int(shape[0]), int(shape[1]), model
    if "ans_ctx" in arrays:
        ctx = np.asarray(arrays["ans_ctx"]).reshape(-1)
        if ctx.shape[0] != 3 or ctx.dtype.kind not in "ui":
            raise ValueError(f"entropy-coded latent file: ans_ctx {ctx.dtype} {ctx.tolist()}")
        _table(freq, bits, CONTEXTS)
        thr = _check_context(int(shape[0]), int(shape[1]), bits, int(ctx[0]), ctx[1:])
        return coded, freq, bits, int(shape[0]), int(shape[1]), int(ctx[0]), thr
    _table(freq, bits)
    return coded, freq, bits, int(shape[0]), int(shape[1])


def _stored_mean(arrays):
    """The kept means of a latent file as float32 (kept, hw, ld): its ``mean``, or its ``mean_q`` / ``mean_step`` dequantised; a file with
    ``mean_ans`` (and no ``mean_q`` handed over in its place) is decoded on the host (entropy.decode_reference, with ``ans_ctx``
    entropy.decode_context_reference, with ``ans_chain`` entropy.decode_temporal_reference), and a stream that fails the end check raises ValueError naming the file's frame."""
    if "mean_q" not in arrays and "mean_ans" in arrays:
        coded, freq, bits, hw, ld, *context = coded_members(arrays)
        try:
            if context and isinstance(context[0], TemporalModel):
                arrays = dict(arrays, mean_q=decode_temporal_reference(coded, freq, bits, hw, ld, context[0].chain, context[0].thr))
            elif context:
                arrays = dict(arrays, mean_q=decode_context_reference(coded, freq, bits, hw, ld, context[0], np.array(context[1])))
            else:
                arrays = dict(arrays, mean_q=decode_reference(coded, freq, bits, hw, ld))
        except ValueError as e:
            raise ValueError(f"entropy-coded latent file: {e} (counted among the file's kept frames)") from None
    if "mean_q" not in arrays:
        return np.asarray(arrays["mean"], dtype=np.float32)
    q, step = np.asarray(arrays["mean_q"]), np.asarray(arrays["mean_step"], dtype=np.float32)
    if q.dtype != np.int8 or q.ndim != 3 or step.shape != (q.shape[0], q.shape[2]):
        raise ValueError(f"quantised latent file: mean_q {q.dtype} {q.shape} with mean_step {step.shape}")
    qmax = qmax_of(int(arrays["quant_bits"]))
    if q.size and int(np.abs(q.astype(np.int16)).max()) > qmax:
        raise ValueError(f"quantised latent file: codes beyond +-{qmax} for quant_bits {int(arrays['quant_bits'])}")
    return dequantise_reference(q, step)


def save_latents(path, arrays):
    """Write a clip's arrays: quantised files deflated (``np.savez_compressed``), the others (entropy-coded ones too: they are coded
    already) as before (``np.savez``) -> bytes written."""
    (np.savez_compressed if "mean_q" in arrays else np.savez)(path, **arrays)
    return os.path.getsize(path)


def _kept(selection):
    """A selection of any rank (tensor or array, nonzero = kept) as a fresh bool array."""
    return np.asarray(torch.as_tensor(selection).detach().float().cpu().numpy() != 0)


def _pack(sel, mean, log_variance, quant, header, footer, entropy=None):
    """``header``, the kept means (``_mean_arrays``), ``selection`` uint8, ``footer``, the kept ``log_variance`` when given, in that key
    order; ``sel`` bool of any rank, mean / log_variance (and quant's codes) shaped sel.shape + (hw, ld); ``entropy``: ``_mean_arrays``."""
    out = {**header, **_mean_arrays(mean, sel, quant, entropy), "selection": sel.astype(np.uint8), **footer}
    if log_variance is not None:
        out["log_variance"] = torch.as_tensor(log_variance).detach().float().cpu().numpy()[sel]
    return out


def _unpack(arrays, fill_token, shape, error):
    """(dense float32 ``shape`` + (hw, ld), selection uint8 ``shape``) of a file's arrays.  A selection of another shape or a number
    of stored means that is not the number of kept frames raises ValueError(``error``), a format template that may name ``{sel}`` (the
    file's selection shape), ``{means}`` and ``{kept}``."""
    sel = np.asarray(arrays["selection"]).astype(np.uint8)
    mean = _stored_mean(arrays)
    means, kept = mean.shape[0] if mean.ndim else 0, int(sel.sum())
    if sel.shape != shape or mean.ndim != 3 or means != kept:
        raise ValueError(error.format(sel=sel.shape, means=means, kept=kept))
    fill = torch.as_tensor(fill_token).detach().float().cpu().numpy().reshape(-1)
    comp = np.broadcast_to(fill, shape + mean.shape[1:]).copy()
    comp[sel != 0] = mean
    return comp, sel


def pack_latents(mean, selection, log_variance=None, quant=None, entropy=None):
    """One clip's latents -> the arrays of its ``.npz``: ``mean`` (kept frames only, float32: lossless from bf16), ``selection`` uint8
    (n_frames,), ``n_frames``; ``log_variance`` of the kept frames when given.  mean / log_variance (n_frames, hw, ld), selection (n_frames,).
    ``quant = (codes (n_frames, hw, ld), step (n_frames, ld), bits)``: ``mean_q`` / ``mean_step`` / ``quant_bits`` in place of ``mean``.
    ``entropy = (entropy.CodedFrames of the kept frames, freq)`` beside ``quant``: ``mean_ans`` / ``ans_*`` in place of ``mean_q``;
    ``entropy = (CodedFrames, freq4, (grid_w, thr0, thr1))``: the context coder's stream, with ``ans_ctx``;
    ``entropy = (CodedFrames, freq9, entropy.TemporalModel(thr, chain))``: the temporal coder's, with ``ans_tthr`` and ``ans_chain``."""
    sel = _kept(selection)
    return _pack(sel, mean, log_variance, quant, {}, {"n_frames": np.int64(sel.shape[0])}, entropy)


def unpack_latents(arrays, fill_token):
    """The dense compressed representation (n_frames, hw, ld) float32 of a packed clip: its means on the kept frames, the fill token
    on the dropped ones -> (comp, selection uint8 (n_frames,))."""
    n = int(arrays["n_frames"])
    return _unpack(arrays, fill_token, (n,),
                   f"latent file: {n} frames, {{sel[0]}} selections, {{means}} kept means for {{kept}} kept frames")


def pack_latents_tiled(mean, selection, grid, log_variance=None, quant=None, entropy=None):
    """One tiled clip's latents -> the arrays of its ``.npz``: ``tile_grid`` int64 [H, W, S, overlap, ny, nx], ``selection`` uint8
    (ny nx, n_frames), ``mean`` float32 (sum of kept, hw, ld) tile-major then frame order, ``n_frames``; ``log_variance`` likewise when
    given.  mean / log_variance (ny nx, n_frames, hw, ld), selection (ny nx, n_frames).  ``quant = (codes, step, bits)`` shaped like mean
    (step without the token axis): ``mean_q`` / ``mean_step`` / ``quant_bits`` in place of ``mean``; ``entropy`` as in ``pack_latents``."""
    sel = _kept(selection)
    if sel.ndim != 2 or sel.shape[0] != grid.tiles:
        raise ValueError(f"selection {sel.shape}: expected ({grid.tiles}, n_frames)")
    return _pack(sel, mean, log_variance, quant, {"tile_grid": grid.as_array()}, {"n_frames": np.int64(sel.shape[1])}, entropy)


def unpack_latents_tiled(arrays, fill_token):
    """The dense compressed representation (ny nx, n_frames, hw, ld) float32 of a packed tiled clip (means on kept frames, the fill
    token elsewhere) -> (comp, selection uint8 (ny nx, n_frames), TileGrid)."""
    grid = TileGrid.from_array(arrays["tile_grid"])
    n = int(arrays["n_frames"])
    error = f"tiled latent file: {grid.tiles} tiles x {n} frames, selection {{sel}}, {{means}} kept means for {{kept}} kept frames"
    return _unpack(arrays, fill_token, (grid.tiles, n), error) + (grid,)


def pack_latents_windows(mean, selection, grid, plan, log_variance=None, quant=None, entropy=None):
    """One clip's latents in overlapping windows -> the arrays of its ``.npz``: ``tile_grid`` int64 [H, W, S, overlap, ny, nx] (1 x 1 for
    the untiled centre square), ``window_starts`` int64 (windows,), ``temporal_overlap``, ``window`` (frames per window), ``n_frames``,
    ``selection`` uint8 (windows, ny nx, F') with F' = min(window, n_frames), ``mean`` float32 (sum of kept, hw, ld) in window, tile, frame
    order; ``log_variance`` likewise when given.  mean / log_variance (windows, ny nx, F', hw, ld), selection (windows, ny nx, F').  A
    ``ScenePlan`` adds ``scene_cuts`` int64 and stores the padded frames of a short scene's window as not kept.  ``quant = (codes, step,
    bits)`` shaped like mean (step without the token axis): ``mean_q`` / ``mean_step`` / ``quant_bits`` in place of ``mean``; ``entropy`` as
    in ``pack_latents`` (its frames are those kept after the padding was dropped)."""
    fw = min(plan.frames, plan.length)
    sel = _kept(selection)
    if sel.shape != (plan.windows, grid.tiles, fw):
        raise ValueError(f"selection {sel.shape}: expected ({plan.windows}, {grid.tiles}, {fw})")
    footer = {}
    if isinstance(plan, ScenePlan):                    # the padding of a short scene's window is not kept
        for w, c in enumerate(plan.counts):
            sel[w, :, c:] = False
        footer["scene_cuts"] = plan.cuts_array()
    header = {"tile_grid": grid.as_array(), "window_starts": plan.starts_array(), "temporal_overlap": np.int64(plan.overlap),
              "window": np.int64(plan.frames), "n_frames": np.int64(plan.length)}
    return _pack(sel, mean, log_variance, quant, header, footer, entropy)


def unpack_latents_windows(arrays, fill_token):
    """The dense compressed representation (windows, ny nx, F', hw, ld) float32 of a packed windowed clip (means on kept frames, the fill
    token elsewhere) -> (comp, selection uint8 (windows, ny nx, F'), TileGrid, WindowPlan, or ScenePlan when the file has
    ``scene_cuts``).  A file whose starts, selection or means do not fit its plan raises ValueError."""
    grid = TileGrid.from_array(arrays["tile_grid"])
    if "scene_cuts" in arrays:
        plan = ScenePlan(int(arrays["n_frames"]), int(arrays["window"]), int(arrays["temporal_overlap"]),
                         np.asarray(arrays["scene_cuts"]).reshape(-1).tolist())
    else:
        plan = WindowPlan(int(arrays["n_frames"]), int(arrays["window"]), int(arrays["temporal_overlap"]))
    starts = np.asarray(arrays["window_starts"]).reshape(-1)
    if starts.tolist() != plan.starts:
        raise ValueError(f"windowed latent file: window starts {starts.tolist()}, {plan!r} has {plan.starts}")
    shape = (plan.windows, grid.tiles, min(plan.frames, plan.length))
    error = f"windowed latent file: selection {{sel}} for {shape}, {{means}} kept means for {{kept}} kept frames"
    return _unpack(arrays, fill_token, shape, error) + (grid, plan)
