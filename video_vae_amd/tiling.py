"""Spatial tiling: encode, decode, reconstruct and evaluate frames of any size with a model trained on one square frame.

Each frame is cut into overlapping ``tile x tile`` tiles (the model's frame side), the tiles run through the existing replayed graphs as
batch entries, and the reconstructed tiles are blended back with weights that ramp across the overlaps.

Grid (``TileGrid``), per axis of length L with tile side S and requested overlap o (0 <= o <= S // 2):
  * n = 1 if L <= S, otherwise ceil((L - o) / (S - o)) (the fewest tiles whose neighbours overlap by at least o);
  * start_i = (i (L - S)) // (n - 1) for n > 1, 0 for n == 1; tile i covers [start_i, start_i + S) = [start_i, end_i).
  * Tiles are ordered row-major over (ty, tx): tile k = ty nx + tx of a window.  When L < S the gather replicates the edge (source index
    min(p, L - 1)); the blend reads only in-frame positions.
Blend weight of tile i at in-tile position p, per axis: 1, times min(1, (p + 0.5) / r) with r = end_{i-1} - start_i when i > 0 and r > 0,
times min(1, (S - p - 0.5) / r) with r = end_i - start_{i+1} when i < n - 1 and r > 0.  2D weight = w_y w_x; output pixel =
sum_k w_k tile_k / sum_k w_k over the covering tiles in ascending k.  Where exactly two tiles overlap this is a partition of unity.

Temporal windows (``WindowPlan``): the time axis on the same grid, a clip of L frames in windows of F frames (``--frames``) that overlap
by at least o_t (0 <= o_t <= F // 2): window starts ``axis_starts(L, F, o_t)``, temporal weights ``axis_weights(L, F, o_t)``.  L <= F: one
window at 0, zero-padded and masked past L.  L > F: every window is full (no padded tail); neighbours may overlap by more than o_t and a
frame may lie in three windows.  o_t = 0 on a multiple of F gives hard cuts (``infer.windows``).  Blend weight of window w, tile (ty, tx)
at in-window frame q and in-tile (py, px): (w_t(w, q) w_y(ty, py)) w_x(tx, px); output = sum weight tile / sum weight over the covering
(w, ty, tx) in ascending order.  A frame one window covers has w_t = 1: exactly the tile blend of that window.

GPU tensors run the HIP kernels (``ops.tile_gather`` / ``ops.tile_blend`` / ``ops.window_blend``, csrc/tiles.hip); CPU tensors a composed
path (the blends in float64).  ``TiledInference`` runs ``infer.GraphedInference`` over chunks of tiles; ``ClipInference`` runs a whole clip
through a ``WindowPlan`` x ``TileGrid`` the same way.

Scenes (``ScenePlan``): a clip cut at scene changes (scenes.py) is one ``WindowPlan`` per scene [c_i, c_{i+1}); no window reads a frame of
another scene and no blend crosses a cut.  ``ClipInference(..)(clip, cuts=...)`` runs the windows of all scenes in one flat order.
"""
import copy
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from .metrics import FrameMetrics, frame_metrics_wide

TILED_MODES = ("reconstruct", "evaluate", "encode", "decode")


def axis_tiles(length, tile, overlap):
    """Number of tiles on an axis of ``length`` (module docstring)."""
    if length <= tile:
        return 1
    return math.ceil((length - overlap) / (tile - overlap))


def axis_starts(length, tile, overlap):
    """The tile starts on one axis: [start_0, ..., start_{n-1}]."""
    n = axis_tiles(length, tile, overlap)
    if n == 1:
        return [0]
    return [(i * (length - tile)) // (n - 1) for i in range(n)]


def axis_weights(length, tile, overlap):
    """float64 (n, tile): the blend weight of each tile of the axis at each in-tile position (positions past ``length`` included)."""
    st = axis_starts(length, tile, overlap)
    n = len(st)
    p = np.arange(tile, dtype=np.float64)
    w = np.ones((n, tile), dtype=np.float64)
    for i in range(n):
        if i > 0:
            r = st[i - 1] + tile - st[i]
            if r > 0:
                w[i] *= np.minimum(1.0, (p + 0.5) / r)
        if i < n - 1:
            r = st[i] + tile - st[i + 1]
            if r > 0:
                w[i] *= np.minimum(1.0, (tile - p - 0.5) / r)
    return w


class TileGrid:
    """The tiles of a ``height x width`` frame: ``ny x nx`` tiles of side ``tile`` whose neighbours overlap by at least ``overlap``.

    ``ys`` / ``xs``: the tile starts per axis; ``weights_y`` (ny, tile) / ``weights_x`` (nx, tile): the per-axis blend weights, float64;
    ``weight(ty, tx)``: the 2D weight (tile, tile) of one tile."""

    def __init__(self, height, width, tile, overlap):
        height, width, tile, overlap = int(height), int(width), int(tile), int(overlap)
        if height < 1 or width < 1 or tile < 1:
            raise ValueError(f"grid of {height}x{width} with tile {tile}: sizes must be positive")
        if not 0 <= overlap <= tile // 2:
            raise ValueError(f"overlap {overlap}: 0 <= overlap <= tile // 2 = {tile // 2}")
        self.height, self.width, self.tile, self.overlap = height, width, tile, overlap
        self.ys, self.xs = axis_starts(height, tile, overlap), axis_starts(width, tile, overlap)
        self.ny, self.nx = len(self.ys), len(self.xs)
        self.weights_y, self.weights_x = axis_weights(height, tile, overlap), axis_weights(width, tile, overlap)

    @property
    def tiles(self):
        """Tiles per window (ny nx)."""
        return self.ny * self.nx

    def origin(self, k):
        """(y0, x0) of tile k = ty nx + tx."""
        ty, tx = divmod(k, self.nx)
        return self.ys[ty], self.xs[tx]

    def weight(self, ty, tx):
        return self.weights_y[ty][:, None] * self.weights_x[tx][None, :]

    def pixel_ratio(self):
        """Tile pixels the model sees per frame pixel: ny nx tile^2 / (height width)."""
        return self.tiles * self.tile * self.tile / (self.height * self.width)

    def as_array(self):
        """int64 [H, W, S, overlap, ny, nx] (what a tiled latent file stores)."""
        return np.array([self.height, self.width, self.tile, self.overlap, self.ny, self.nx], dtype=np.int64)

    @classmethod
    def from_array(cls, a):
        h, w, s, o, ny, nx = (int(v) for v in np.asarray(a).reshape(-1))
        g = cls(h, w, s, o)
        if (g.ny, g.nx) != (ny, nx):
            raise ValueError(f"tile grid {list(np.asarray(a))}: {h}x{w} with tile {s}, overlap {o} has {g.ny}x{g.nx} tiles")
        return g

    def __eq__(self, other):
        return isinstance(other, TileGrid) and (self.height, self.width, self.tile, self.overlap) == (
            other.height, other.width, other.tile, other.overlap)

    def __repr__(self):
        return f"TileGrid({self.height}, {self.width}, tile={self.tile}, overlap={self.overlap}: {self.ny}x{self.nx})"


def gather_tiles(frames, grid, first=0, count=None, out=None):
    """uint8 frames (N, T, H, W, C) -> fp32 tiles (count, T, S, S, C): tiles ``first .. first + count - 1`` of the flat (window, ty, tx)
    order, each value ``u8.float() / 255`` (bitwise, on the GPU), edges replicated.  GPU tensors: ``ops.tile_gather`` into ``out`` when
    given (written in place, may hold more than ``count`` tiles); CPU tensors: indexing."""
    n = frames.shape[0]
    total = n * grid.tiles
    count = total - first if count is None else count
    if first < 0 or count < 1 or first + count > total:
        raise ValueError(f"tiles {first} .. {first + count - 1} of {total}")
    if frames.is_cuda:
        from . import ops
        if out is None:
            out = torch.empty((count,) + tuple(frames.shape[1:2]) + (grid.tile, grid.tile, frames.shape[4]), dtype=torch.float32,
                              device=frames.device)
        return ops.tile_gather(frames, grid, first, count, out)
    s = grid.tile
    tiles = []
    for q in range(first, first + count):
        w, k = divmod(q, grid.tiles)
        y0, x0 = grid.origin(k)
        yi = torch.clamp(torch.arange(y0, y0 + s), max=grid.height - 1)
        xi = torch.clamp(torch.arange(x0, x0 + s), max=grid.width - 1)
        tiles.append(frames[w][:, yi][:, :, xi].float() / 255)
    res = torch.stack(tiles)
    if out is not None:
        out[:count].copy_(res)
        return out
    return res


def blend_tiles(tiles, grid):
    """Tiles (N ny nx, T, S, S, C) -> frames (N, T, H, W, C): the weighted blend of the module docstring.  GPU tensors (fp32 / bf16):
    ``ops.tile_blend``, fp32 out; CPU tensors: composed in float64, float64 out."""
    if tiles.is_cuda:
        from . import ops
        return ops.tile_blend(tiles, grid)
    nk, t, s, _, c = tiles.shape
    k_per = grid.tiles
    n = nk // k_per
    h, w = grid.height, grid.width
    x = tiles.to(torch.float64).reshape(n, k_per, t, s, s, c)
    num = torch.zeros((n, t, h, w, c), dtype=torch.float64)
    den = torch.zeros((h, w), dtype=torch.float64)
    for k in range(k_per):
        ty, tx = divmod(k, grid.nx)
        y0, x0 = grid.ys[ty], grid.xs[tx]
        hh, ww = min(s, h - y0), min(s, w - x0)
        wk = torch.from_numpy(grid.weight(ty, tx)[:hh, :ww])
        num[:, :, y0:y0 + hh, x0:x0 + ww] += wk[None, None, :, :, None] * x[:, k, :, :hh, :ww]
        den[y0:y0 + hh, x0:x0 + ww] += wk
    return num / den[None, None, :, :, None]


def window_runs(first, count, k_per):
    """Tiles first .. first + count - 1 of the flat (window, k) order as runs of one window: (offset j in the chunk, window w, first tile
    k of the run, tiles m in it)."""
    j = 0
    while j < count:
        w, k = divmod(first + j, k_per)
        m = min(count - j, k_per - k)
        yield j, w, k, m
        j += m


class TiledOutput(NamedTuple):
    """What ``TiledInference`` returns; fields a mode does not produce are None.
    frames: stitched fp32 (N, T, H, W, C) ("reconstruct", "evaluate", "decode"); selection: (N, ny nx, T) fp32 frame gate per tile (not
    "decode"); metrics: ``FrameMetrics`` (N, T) of the stitched frames against frames / 255 ("evaluate"); mean, log_variance:
    (N, ny nx, T, hw, ld) ("encode"; log_variance when asked for)."""
    frames: Optional[torch.Tensor]
    selection: Optional[torch.Tensor]
    metrics: Optional[FrameMetrics]
    mean: Optional[torch.Tensor]
    log_variance: Optional[torch.Tensor]


class TiledInference:
    """``infer.GraphedInference`` at (batch, frames) with frame_shape (S, S, C), replayed over the tiles of a ``TileGrid``.

    ``__call__(inputs, mask)``: ``inputs`` = uint8 frames (N, T, H, W, C) on the GPU ("reconstruct", "evaluate", "encode"), or the
    compressed representation (N, ny nx, T, hw, ld) ("decode"); ``mask`` (N, T), shared by every tile of a window.  The tiles run in flat
    (window, ty, tx) order, ``batch`` per replay, gathered straight into the graph's static input; a short last chunk is filled with
    copies of its last tile (their outputs are dropped).  A window's tiles are kept until it is complete, then blended.  "evaluate" adds
    ``frame_metrics_wide`` of the stitched frames against frames / 255.  Returns a fresh ``TiledOutput``.
    ``with_grid(grid)``: the same captured graph on another grid of the same tile side."""

    def __init__(self, model, weights, grid, batch, frames, mode, rngs=None, want_log_variance=False, warmup=2):
        from .infer import GraphedInference
        if mode not in TILED_MODES:
            raise ValueError(f"mode {mode!r}: one of {TILED_MODES}")
        enc = model.encoder
        p = enc.patch_embedding.patch_size
        side = math.isqrt(enc.selection_layer2.kernel.shape[0]) * p
        if grid.tile != side:
            raise ValueError(f"tile {grid.tile}: the model's frame side is {side}")
        self.grid, self.batch, self.frames, self.mode = grid, int(batch), int(frames), mode
        self.channels = enc.last_dim // (p * p)
        self.want_log_variance = bool(want_log_variance)
        gmode = "reconstruct" if mode == "evaluate" else mode
        self.runner = GraphedInference(model, weights, batch, frames, gmode, rngs=rngs, want_log_variance=want_log_variance,
                                       warmup=warmup, frame_shape=(side, side, self.channels), with_selection=True)

    def with_grid(self, grid):
        if grid.tile != self.grid.tile:
            raise ValueError(f"tile {grid.tile}: this runner's tile is {self.grid.tile}")
        other = copy.copy(self)
        other.grid = grid
        return other

    def _load(self, inputs, first, count):
        """Tiles first .. first + count - 1 (and copies of the last up to the batch) into the graph's static input."""
        r, b = self.runner, self.batch
        if self.mode == "decode":
            src = inputs.reshape((-1,) + tuple(inputs.shape[2:]))
            r.input[:count].copy_(src[first:first + count])
            if count < b:
                r.input[count:].copy_(src[first + count - 1].expand((b - count,) + tuple(src.shape[1:])))
            return
        gather_tiles(inputs, self.grid, first, count, out=r.input)
        for j in range(count, b):
            gather_tiles(inputs, self.grid, first + count - 1, 1, out=r.input[j:j + 1])

    def _replay(self, mask, load, place):
        """The chunk loop of both runners, over the windows of ``mask`` (N, T): per chunk of ``batch`` tiles of the flat (window, k)
        order, ``load(first, count)`` fills the graph's static input, every slot gets the mask row of its window (the copies filling a
        short last chunk that of the last tile), the graph is replayed and the selection copied out.  "encode" collects mean /
        log_variance; the other modes hand every run of one window to ``place(recon, j, w, k, m)`` (``window_runs``).
        -> (selection, mean, log_variance), None where the mode has none."""
        b, t, k_per = self.batch, self.frames, self.grid.tiles
        n = mask.shape[0]
        total = n * k_per
        dev = self.runner.input.device
        sel = None if self.mode == "decode" else torch.empty((n, k_per, t), dtype=torch.float32, device=dev)
        mean = logvar = None
        for first in range(0, total, b):
            count = min(b, total - first)
            load(first, count)
            wins = [min(first + j, first + count - 1) // k_per for j in range(b)]
            res = self.runner(None, mask.index_select(0, torch.tensor(wins, device=dev)))
            if self.mode == "encode":
                if mean is None:
                    mean = torch.empty((n, k_per, t) + tuple(res.mean.shape[2:]), dtype=res.mean.dtype, device=dev)
                    if self.want_log_variance:
                        logvar = torch.empty_like(mean)
                mean.view((total,) + tuple(mean.shape[2:]))[first:first + count].copy_(res.mean[:count])
                if self.want_log_variance:
                    logvar.view((total,) + tuple(mean.shape[2:]))[first:first + count].copy_(res.log_variance[:count])
                sel.view(total, t)[first:first + count].copy_(res.selection[:count])
                continue
            recon = res
            if self.mode != "decode":
                recon, selection = res
                sel.view(total, t)[first:first + count].copy_(selection[:count])
            for j, w, k, m in window_runs(first, count, k_per):
                place(recon, j, w, k, m)
        return sel, mean, logvar

    @torch.no_grad()
    def __call__(self, inputs, mask):
        from . import ops
        g, t = self.grid, self.frames
        n = inputs.shape[0]
        k_per = g.tiles
        dev = self.runner.input.device
        if self.mode == "decode":
            if tuple(inputs.shape[1:3]) != (k_per, t):
                raise ValueError(f"decode inputs {tuple(inputs.shape)}: expected (N, {k_per}, {t}, hw, ld)")
        elif inputs.dtype != torch.uint8 or tuple(inputs.shape[1:]) != (t, g.height, g.width, self.channels):
            raise ValueError(f"inputs {inputs.dtype} {tuple(inputs.shape)}: expected uint8 (N, {t}, {g.height}, {g.width}, {self.channels})")
        mask = mask.to(device=dev, dtype=torch.float32).reshape(n, t)
        frames = None
        if self.mode != "encode":
            frames = torch.empty((n, t, g.height, g.width, self.channels), dtype=torch.float32, device=dev)
        pending = {}

        def place(recon, j, w, k, m):                         # a window's tiles are kept until it is complete, then blended
            if w not in pending:
                pending[w] = torch.empty((k_per,) + tuple(recon.shape[1:]), dtype=recon.dtype, device=dev)
            pending[w][k:k + m].copy_(recon[j:j + m])
            if k + m == k_per:
                ops.tile_blend(pending.pop(w), g, out=frames[w:w + 1])

        sel, mean, logvar = self._replay(mask, lambda first, count: self._load(inputs, first, count), place)
        fm = None
        if self.mode == "evaluate":
            fm = frame_metrics_wide(inputs.float() / 255.0, frames, mask)
        return TiledOutput(frames, sel, fm, mean, logvar)


class WindowPlan:
    """The windows of a clip of ``length`` frames: ``frames`` frames each, neighbours overlapping by at least ``overlap`` (module docstring).

    ``starts``: the window starts; ``weights`` (windows, frames): the temporal blend weights, float64; ``counts``: real frames per window
    (``frames`` each when length > frames, else [length])."""

    def __init__(self, length, frames, overlap):
        length, frames, overlap = int(length), int(frames), int(overlap)
        if length < 1 or frames < 1:
            raise ValueError(f"{length} frames in windows of {frames}: sizes must be positive")
        if not 0 <= overlap <= frames // 2:
            raise ValueError(f"temporal overlap {overlap}: 0 <= overlap <= frames // 2 = {frames // 2}")
        self.length, self.frames, self.overlap = length, frames, overlap
        self.starts = axis_starts(length, frames, overlap)
        self.weights = axis_weights(length, frames, overlap)
        self.windows = len(self.starts)
        self.counts = [min(frames, length - st) for st in self.starts]

    def mask(self):
        """float32 (windows, frames): 1 on real frames, 0 on the padding of a clip shorter than a window."""
        m = np.zeros((self.windows, self.frames), dtype=np.float32)
        for w, c in enumerate(self.counts):
            m[w, :c] = 1.0
        return m

    def covering(self, f):
        """The windows that hold frame ``f``, ascending."""
        return [w for w, st in enumerate(self.starts) if st <= f < st + self.frames]

    def final(self, w):
        """Frames below this index are final once windows 0 .. w are: the next window's start, or the clip length."""
        return self.starts[w + 1] if w + 1 < self.windows else self.length

    def ring(self):
        """Windows whose tiles must be held at once when each final range is blended as soon as its last window is done."""
        best, lo = 1, 0
        for w in range(self.windows):
            first = self.starts[w] if w else 0
            while self.starts[lo] + self.frames <= first:
                lo += 1
            best = max(best, w - lo + 1)
        return best

    def stored_ratio(self):
        """Real window frames the model runs per clip frame: sum(counts) / length (1.0 for hard cuts)."""
        return sum(self.counts) / self.length

    def starts_array(self):
        return np.array(self.starts, dtype=np.int64)

    def __eq__(self, other):
        return isinstance(other, WindowPlan) and (self.length, self.frames, self.overlap) == (other.length, other.frames, other.overlap)

    def __repr__(self):
        return f"WindowPlan({self.length}, frames={self.frames}, overlap={self.overlap}: starts {self.starts})"


def check_cuts(cuts, length):
    """``cuts`` as a list of ints after checking that they are strictly increasing frame indices in 1 .. length - 1."""
    c = [int(v) for v in cuts]
    if any(v != w for v, w in zip(c, cuts)):
        raise ValueError(f"scene cuts {list(cuts)}: integers expected")
    if any(v < 1 or v >= length for v in c) or any(a >= b for a, b in zip(c, c[1:])):
        raise ValueError(f"scene cuts {c}: strictly increasing frame indices in 1 .. {length - 1} expected")
    return c


class ScenePlan:
    """The windows of a clip of ``length`` frames cut into scenes at ``cuts``: one ``WindowPlan(end - start, frames, overlap)`` per scene
    [start, end), so that no window spans a cut and no blend crosses one.  A scene shorter than ``frames`` is one window, zero-padded and
    masked past the scene's end.

    The attributes of a ``WindowPlan`` over all windows in scene order, with global window starts: ``length``, ``frames``, ``overlap``,
    ``starts``, ``counts``, ``weights`` (windows, frames), ``windows``, ``mask()``, ``covering(f)`` (only windows of f's scene),
    ``ring()`` (the largest scene ring), ``stored_ratio()``, ``starts_array()``; plus ``cuts``, ``scenes`` [(start, end)], ``plans``
    (the per-scene ``WindowPlan``), ``first`` (each scene's first window) and ``scene(w)`` -> (scene index, window index in the scene).
    With ``cuts=[]`` the starts, counts and weights are the ``WindowPlan``'s."""

    def __init__(self, length, frames, overlap, cuts):
        length, frames, overlap = int(length), int(frames), int(overlap)
        WindowPlan(length, frames, overlap)                                  # validates the sizes and the overlap
        self.length, self.frames, self.overlap = length, frames, overlap
        self.cuts = check_cuts(cuts, length)
        b = [0] + self.cuts + [length]
        self.scenes = [(b[i], b[i + 1]) for i in range(len(b) - 1)]
        self.plans = [WindowPlan(e - a, frames, overlap) for a, e in self.scenes]
        self.first, self.starts, self.counts, self._owner = [], [], [], []
        for i, ((a, _), p) in enumerate(zip(self.scenes, self.plans)):
            self.first.append(len(self.starts))
            self.starts += [a + st for st in p.starts]
            self.counts += p.counts
            self._owner += [(i, w) for w in range(p.windows)]
        self.windows = len(self.starts)
        self.weights = np.concatenate([p.weights for p in self.plans])

    def scene(self, w):
        """(scene index, window index within the scene) of window ``w``."""
        return self._owner[w]

    def scene_of_frame(self, f):
        return int(np.searchsorted(self.cuts, f, side="right"))

    def mask(self):
        return np.concatenate([p.mask() for p in self.plans])

    def covering(self, f):
        i = self.scene_of_frame(f)
        return [self.first[i] + w for w in self.plans[i].covering(f - self.scenes[i][0])]

    def ring(self):
        return max(p.ring() for p in self.plans)

    def stored_ratio(self):
        return sum(self.counts) / self.length

    def starts_array(self):
        return np.array(self.starts, dtype=np.int64)

    def cuts_array(self):
        return np.array(self.cuts, dtype=np.int64)

    def __eq__(self, other):
        return isinstance(other, ScenePlan) and (self.length, self.frames, self.overlap, self.cuts) == (
            other.length, other.frames, other.overlap, other.cuts)

    def __repr__(self):
        return f"ScenePlan({self.length}, frames={self.frames}, overlap={self.overlap}, cuts={self.cuts}: starts {self.starts})"


def blend_windows(tiles, plan, grid, f_lo=0, f_hi=None, out=None, ring=None):
    """Tiles (windows, ny nx, F, S, S, C) of a clip's windows -> the clip (L, H, W, C): the weighted blend of the module docstring.

    GPU tensors (fp32 / bf16): ``ops.window_blend`` of frames ``f_lo .. f_hi - 1`` into ``out`` (a fresh fp32 clip when None; only that
    range is written), ``tiles`` may be a ring of slots (window w in slot w % ring).  CPU tensors: composed in float64 over every window,
    float64 out, the whole clip.  A ``ScenePlan`` blends each scene on its own ``WindowPlan`` into its slice of the clip (the whole clip,
    every window's tiles given)."""
    if isinstance(plan, ScenePlan):
        if f_lo != 0 or f_hi not in (None, plan.length) or ring is not None:
            raise ValueError("blend_windows on a ScenePlan: the whole clip only")
        if tiles.shape[0] != plan.windows:
            raise ValueError(f"tiles {tuple(tiles.shape)}: expected {plan.windows} windows")
        parts = []
        for i, ((a, e), p) in enumerate(zip(plan.scenes, plan.plans)):
            w0 = plan.first[i]
            if tiles.is_cuda:
                if out is None:
                    out = torch.empty((plan.length, grid.height, grid.width, tiles.shape[-1]), dtype=torch.float32, device=tiles.device)
                blend_windows(tiles[w0:w0 + p.windows], p, grid, out=out[a:e])
            else:
                parts.append(blend_windows(tiles[w0:w0 + p.windows], p, grid))
        return out if tiles.is_cuda else torch.cat(parts)
    f_hi = plan.length if f_hi is None else f_hi
    if tiles.is_cuda:
        from . import ops
        if out is None:
            out = torch.empty((plan.length, grid.height, grid.width, tiles.shape[-1]), dtype=torch.float32, device=tiles.device)
        return ops.window_blend(tiles, plan, grid, f_lo, f_hi, out, ring)
    nw, k_per, f, s, _, c = tiles.shape
    if (nw, k_per, f) != (plan.windows, grid.tiles, plan.frames):
        raise ValueError(f"tiles {tuple(tiles.shape)}: expected ({plan.windows}, {grid.tiles}, {plan.frames}, S, S, C)")
    h, w = grid.height, grid.width
    x = tiles.to(torch.float64)
    num = torch.zeros((plan.length, h, w, c), dtype=torch.float64)
    den = torch.zeros((plan.length, h, w), dtype=torch.float64)
    for win, (st, cnt) in enumerate(zip(plan.starts, plan.counts)):
        wt = torch.from_numpy(plan.weights[win][:cnt])
        for k in range(k_per):
            ty, tx = divmod(k, grid.nx)
            y0, x0 = grid.ys[ty], grid.xs[tx]
            hh, ww = min(s, h - y0), min(s, w - x0)
            wk = wt[:, None, None] * torch.from_numpy(grid.weight(ty, tx)[:hh, :ww])[None]
            num[st:st + cnt, y0:y0 + hh, x0:x0 + ww] += wk[..., None] * x[win, k, :cnt, :hh, :ww]
            den[st:st + cnt, y0:y0 + hh, x0:x0 + ww] += wk
    return num / den[..., None]


class ClipOutput(NamedTuple):
    """What ``ClipInference`` returns; fields a mode does not produce are None.
    frames: the stitched clip fp32 (L, H, W, C) ("reconstruct", "evaluate", "decode"); selection: (windows, ny nx, F) fp32 frame gate per
    window and tile (not "decode"); metrics: ``FrameMetrics`` (1, L) of the clip against frames / 255 ("evaluate"); mean, log_variance:
    (windows, ny nx, F, hw, ld) ("encode"; log_variance when asked for); plan: the ``WindowPlan`` (the ``ScenePlan`` with cuts)."""
    frames: Optional[torch.Tensor]
    selection: Optional[torch.Tensor]
    metrics: Optional[FrameMetrics]
    mean: Optional[torch.Tensor]
    log_variance: Optional[torch.Tensor]
    plan: WindowPlan


class ClipInference(TiledInference):
    """A whole clip through a ``WindowPlan`` (``frames``, ``temporal_overlap``) x ``TileGrid``, on the replayed graph of ``TiledInference``
    (the untiled centre square is the 1 x 1 grid ``TileGrid(size, size, size, 0)``).

    ``__call__(inputs, length=None)``: ``inputs`` = the uint8 clip (L, H, W, C) on the GPU ("reconstruct", "evaluate", "encode"), or the
    compressed representation (windows, ny nx, F, hw, ld) of a clip of ``length`` frames ("decode").  The tiles run in flat (window, ty,
    tx) order, ``batch`` per replay, gathered straight from the clip into the graph's static input (a clip shorter than a window is
    zero-padded); a short last chunk is filled with copies of its last tile.  A window's tiles are held in a ring of
    ``WindowPlan.ring()`` slots until every frame they cover is final; each final frame range is blended with one ``ops.window_blend``.
    "evaluate" adds ``frame_metrics_wide`` of the stitched clip against frames / 255.  Returns a fresh ``ClipOutput``."""

    def __init__(self, model, weights, grid, batch, frames, temporal_overlap, mode, rngs=None, want_log_variance=False, warmup=2):
        super().__init__(model, weights, grid, batch, frames, mode, rngs=rngs, want_log_variance=want_log_variance, warmup=warmup)
        self.temporal_overlap = int(temporal_overlap)
        if not 0 <= self.temporal_overlap <= self.frames // 2:
            raise ValueError(f"temporal overlap {temporal_overlap}: 0 <= overlap <= frames // 2 = {self.frames // 2}")

    def with_grid(self, grid, temporal_overlap=None):
        """The same captured graph on another grid of the same tile side (and another temporal overlap when given)."""
        other = super().with_grid(grid)
        if temporal_overlap is not None:
            WindowPlan(self.frames, self.frames, temporal_overlap)          # validates the overlap
            other.temporal_overlap = int(temporal_overlap)
        return other

    def plan(self, length, cuts=None):
        """The clip's ``WindowPlan``, or its ``ScenePlan`` when ``cuts`` is given."""
        if cuts is not None:
            return ScenePlan(length, self.frames, self.temporal_overlap, cuts)
        return WindowPlan(length, self.frames, self.temporal_overlap)

    def _load_clip(self, clip, plan, first, count, padded):
        """Tiles first .. first + count - 1 of the flat (window, k) order, gathered from their windows of ``clip`` (``padded``: window ->
        its zero-padded frames, for the windows shorter than ``frames``), then copies of the last up to the batch."""
        r, f = self.runner, self.frames
        for j, w, k, m in window_runs(first, count, self.grid.tiles):
            st = plan.starts[w]
            src = padded[w] if w in padded else clip[st:st + f]
            gather_tiles(src[None], self.grid, k, m, out=r.input[j:j + m])
        if count < self.batch:
            r.input[count:].copy_(r.input[count - 1:count].expand((self.batch - count,) + tuple(r.input.shape[1:])))

    @torch.no_grad()
    def __call__(self, inputs, length=None, cuts=None):
        """``cuts`` (sorted frame indices 1 .. L - 1, or None): run the clip through a ``ScenePlan`` -- the windows of every scene in one
        flat order, each scene blended into its own slice of the clip on its own ``WindowPlan`` (ring slots numbered per scene).  A short
        scene's window is zero-padded and masked, never filled with frames of the next scene."""
        from . import ops
        g, t = self.grid, self.frames
        k_per = g.tiles
        dev = self.runner.input.device
        if self.mode == "decode":
            if length is None:
                raise ValueError("decode needs the clip length")
            plan = self.plan(length, cuts)
            if tuple(inputs.shape[:3]) != (plan.windows, k_per, t):
                raise ValueError(f"decode inputs {tuple(inputs.shape)}: expected ({plan.windows}, {k_per}, {t}, hw, ld)")
            load = lambda first, count: self._load(inputs, first, count)
        else:
            if inputs.dtype != torch.uint8 or inputs.dim() != 4 or tuple(inputs.shape[1:]) != (g.height, g.width, self.channels):
                raise ValueError(f"inputs {inputs.dtype} {tuple(inputs.shape)}: expected uint8 (L, {g.height}, {g.width}, {self.channels})")
            plan = self.plan(inputs.shape[0], cuts)
            clip = inputs.contiguous()
            # the short windows (a clip or a scene shorter than a window), zero-padded
            padded = {w: torch.cat([clip[st:st + c], clip.new_zeros((t - c,) + tuple(clip.shape[1:]))])
                      for w, (st, c) in enumerate(zip(plan.starts, plan.counts)) if c < t}
            load = lambda first, count: self._load_clip(clip, plan, first, count, padded)
        frames = ring = None
        if self.mode != "encode":
            frames = torch.empty((plan.length, g.height, g.width, self.channels), dtype=torch.float32, device=dev)
        slots = plan.ring()

        def place(recon, j, w, k, m):
            nonlocal ring
            if ring is None:
                ring = torch.empty((slots, k_per) + tuple(recon.shape[1:]), dtype=recon.dtype, device=dev)
            if cuts is None:
                sp, lw, dst = plan, w, frames
            else:                                             # the scene's own plan, window index and slice of the clip
                si, lw = plan.scene(w)
                sp, (a, e) = plan.plans[si], plan.scenes[si]
                dst = frames[a:e]
            ring[lw % slots, k:k + m].copy_(recon[j:j + m])
            if k + m == k_per:                                # window w is complete: the frames below the next start are final
                f_lo = sp.starts[lw] if lw else 0
                ops.window_blend(ring, sp, g, f_lo, sp.final(lw), dst, slots)

        sel, mean, logvar = self._replay(torch.from_numpy(plan.mask()).to(dev), load, place)
        fm = None
        if self.mode == "evaluate":
            fm = frame_metrics_wide(inputs.float()[None] / 255.0, frames[None], torch.ones((1, plan.length), device=dev))
        return ClipOutput(frames, sel, fm, mean, logvar, plan)
