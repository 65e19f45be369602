"""Host input pipeline: clips on disk -> cropped / resized / padded batches -> pinned host memory -> HBM on a side stream.

Counterpart of the reference's grain + OpenCV loader (train/dataloader.py:95-390, per-rank variant
claude_distributed/dataloader.py:340-373) for one node of MI355X GPUs.  Same batch contract
(train/dataloader.py:387-390):

    {"video": float32 (B, T, H, W, 3) in [0, 1], "mask": float32 (B, T) with 1 = real frame, 0 = padding}

and the same per-clip recipe (train/dataloader.py:148-240): a random temporal window of at most ``max_frames`` frames, ONE random
spatial crop for all frames of the clip (frames smaller than the crop are scaled up first), an optional resize to
``resize``, pixel values / 255, zero padding up to ``max_frames``, mask over the real frames; a clip that cannot be
read yields zeros with an all-ones mask, as the reference does.  Per-rank sharding is the reference's: every rank
shuffles the whole file list with ``seed + rank`` (claude_distributed/dataloader.py:363).

What is different, and why.  At ~1.6 k frames/s per GPU (13 k on a node) the reference's float32 host batches would
be 50 MB per step per GPU across PCIe; here the worker processes hand over **uint8** frames (12.6 MB per C3 batch),
the batch is staged in pinned memory, copied on a side HIP stream while the previous step computes (double
buffered) and converted to the contract's float32 / 255 (or straight to the compute dtype) on the GPU:
``u8.float() / 255`` there is the same IEEE division the reference does on the host, so the values are
bit-identical.  Decoding: frame containers ``.npy`` / ``.npz`` (uint8 (T, H, W, 3)) and YUV4MPEG2 clips ``.y4m`` (y4m.py: the planes are
converted to RGB on the host here unless ``device_yuv=True``, on the device in infer) are read natively; compressed video
files (.mp4 ...) are read through OpenCV when ``cv2`` is importable (it is not in this image: such files are then
reported as unreadable, i.e. the reference's zero-clip fallback).

Device resize (``device_resize=True`` in the loader, ``resize=(h, w)`` in DevicePrefetcher): the workers stop after the crop, the
crop-sized uint8 batch crosses PCIe and one HIP launch (csrc/resize.hip, ops.crop_resize_norm) resizes it, divides by 255 and writes the
compute dtype: the reference's 512-crop, 256-resize recipe without the host's interpolate, the same values bit for bit.

Device conversion of .y4m clips (``device_yuv=True`` in the loader, ``yuv={...}`` in DevicePrefetcher): the workers do no colour arithmetic
either.  They copy the plane bytes of the chosen window and crop out of the memory-mapped file (y4m.Y4MClip.window: 1.5 bytes per pixel at
4:2:0 instead of 3), the plane batch crosses PCIe as it is and one HIP launch (csrc/yuv_window.hip, ops.yuv_window_resize_norm) converts,
resizes, divides by 255 and writes the compute dtype: the host path's values bit for bit, from the same files with the same seed.
"""
import os
import sys
import queue
import threading

import numpy as np
import torch
import torch.nn.functional as F

VIDEO_EXT = (".mp4", ".avi", ".mov", ".mkv", ".webm")
ARRAY_EXT = (".npy", ".npz")
Y4M_EXT = (".y4m",)


def list_video_files(base_dir):
    """All clips under ``base_dir/videos{i}`` for i in 0..99 (train/dataloader.py:96-112); ``base_dir`` itself is scanned too
    when it has no such sub-directory, so a flat folder of clips works."""
    paths = []
    dirs = [os.path.join(base_dir, f"videos{i}") for i in range(100)]
    dirs = [d for d in dirs if os.path.isdir(d)] or [base_dir]
    for d in dirs:
        for name in sorted(os.listdir(d)):
            if name.endswith(VIDEO_EXT + ARRAY_EXT + Y4M_EXT):
                paths.append(os.path.join(d, name))
    return paths


def get_random_crop_params(h, w, crop_size, rng):
    """(new_h, new_w, start_h, start_w): frames smaller than the crop are scaled up first (train/dataloader.py:115-130)."""
    if h < crop_size or w < crop_size:
        scale = max(crop_size / h, crop_size / w)
        h, w = int(h * scale), int(w * scale)
    return h, w, int(rng.integers(0, h - crop_size + 1)), int(rng.integers(0, w - crop_size + 1))


def _resize_u8(frames, h, w):
    """(T, H0, W0, 3) uint8 -> (T, h, w, 3) uint8, bilinear with half-pixel centres (cv2.resize's default INTER_LINEAR)."""
    if frames.shape[1] == h and frames.shape[2] == w:
        return frames
    t = torch.from_numpy(np.array(frames)).permute(0, 3, 1, 2).float()      # copy: memory-mapped sources are read-only
    t = F.interpolate(t, size=(h, w), mode="bilinear", align_corners=False)
    return t.round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()


def _resize_taps(i_ext, o_ext):
    """One axis of resize_reference_u8, input extent ``i_ext`` -> output extent ``o_ext``: (i0, i1 int64, l0, l1 float32), each (o_ext,)."""
    half = np.float32(0.5)
    scale = np.float32(i_ext) / np.float32(o_ext)
    src = scale * (np.arange(o_ext, dtype=np.float32) + half) - half
    src = np.where(src < 0, np.float32(0), src).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), i_ext - 1)
    i1 = i0 + (i0 < i_ext - 1)
    l1 = src - i0.astype(np.float32)
    return i0, i1, np.float32(1) - l1, l1


def resize_reference_u8(frames, h, w):
    """(T, H0, W0, C) uint8 -> (T, h, w, C) uint8: the bytes of ``_resize_u8``, written out.  It is the specification of the device resize
    (csrc/resize.hip, ops.crop_resize_u8) and the tests' CPU reference; no framework interpolation is called.

    Per axis with input extent I and output extent O, in float32, every operation rounded to nearest on its own (numpy fuses nothing):
    scale = float32(I) / float32(O); src = scale * (d + 0.5) - 0.5, 0 when negative; i0 = min(int(src), I - 1), i1 = i0 + (i0 < I - 1);
    l1 = src - i0, l0 = 1 - l1.  With rows (y0, y1, a0, a1) and columns (x0, x1, b0, b1):
    v = a0 * (b0 * s[y0, x0] + b1 * s[y0, x1]) + a1 * (b0 * s[y1, x0] + b1 * s[y1, x1]); the result is v rounded to nearest even and
    clamped to 0 .. 255.  Equal extents give l1 = 0, an exact copy."""
    frames = np.asarray(frames)
    if frames.ndim != 4 or frames.dtype != np.uint8:
        raise ValueError(f"resize_reference_u8: expected uint8 (T, H, W, C), got {frames.dtype} {frames.shape}")
    y0, y1, a0, a1 = _resize_taps(frames.shape[1], h)
    x0, x1, b0, b1 = _resize_taps(frames.shape[2], w)
    tap = lambda y, x: frames[:, y[:, None], x[None, :]].astype(np.float32)          # (T, h, w, C)
    a0, a1 = a0[None, :, None, None], a1[None, :, None, None]
    b0, b1 = b0[None, None, :, None], b1[None, None, :, None]
    top = b0 * tap(y0, x0) + b1 * tap(y0, x1)
    bot = b0 * tap(y1, x0) + b1 * tap(y1, x1)
    v = a0 * top + a1 * bot
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def centre_square_crop(h, w):
    """(top, left, side) of the centred square of an h x w frame: side min(h, w) (infer.centre_square's crop)."""
    s = min(h, w)
    return (h - s) // 2, (w - s) // 2, s


def device_centre_square(frames, size, out=None):
    """uint8 (T, H, W, C) on a GPU -> uint8 (T, size, size, C) there: infer.centre_square's crop and resize, its bytes, in one kernel
    launch (ops.crop_resize_u8)."""
    from . import ops
    top, left, s = centre_square_crop(frames.shape[1], frames.shape[2])
    return ops.crop_resize_u8(frames, top, left, s, s, size, size, out=out)


UPLOAD_RUN_BYTES = 1 << 30


def y4m_device_runs(clip, device, run_bytes=UPLOAD_RUN_BYTES, out=None):
    """A y4m.Y4MClip -> (a, b, uint8 RGB (b - a, H, W, 3) on ``device``) for consecutive runs of frames covering the clip: the frame
    records of a run (at most about ``run_bytes``, at least one frame) are uploaded exactly as they lie in the file, FRAME lines included,
    and converted there in one launch (ops.yuv_to_rgb_u8 on views of the upload): 1.5 bytes per pixel over PCIe for 4:2:0 instead of 3, no
    host conversion, the bytes of ``clip[a:b]``.  ``out``: a uint8 (T, H, W, 3) tensor on the device whose frames [a, b) take the runs."""
    from . import ops
    _, h, w, _ = clip.shape
    ch, cw = clip.header.chroma_shape
    for a, b in clip.runs(0, clip.shape[0], run_bytes):
        rec, line, stride = clip.records(a, b)
        buf = torch.from_numpy(np.array(rec)).to(device)           # copy: the memory map is read-only
        view = lambda off, r, c: buf.as_strided((b - a, r, c), (stride, c, 1), off)
        y = view(line, h, w)
        u = v = None
        if clip.chroma != "mono":
            u, v = view(line + h * w, ch, cw), view(line + h * w + ch * cw, ch, cw)
        yield a, b, ops.yuv_to_rgb_u8(y, u, v, clip.chroma, clip.siting, clip.matrix, clip.full, out=None if out is None else out[a:b])


def upload_rgb(clip, device, run_bytes=UPLOAD_RUN_BYTES):
    """A clip uint8 (T, H, W, 3) -> the same frames on ``device``: a host array is copied; a y4m.Y4MClip is uploaded as planes, run by run,
    and converted there (y4m_device_runs)."""
    from .y4m import Y4MClip
    if not isinstance(clip, Y4MClip):
        return torch.from_numpy(np.ascontiguousarray(clip)).to(device)
    out = torch.empty(clip.shape, dtype=torch.uint8, device=device)
    for _ in y4m_device_runs(clip, device, run_bytes, out=out):
        pass
    return out


def upload_centre_square(clip, size, device, run_bytes=UPLOAD_RUN_BYTES):
    """A host clip uint8 (T, H, W, C) -> its device_centre_square (T, size, size, C) on ``device``, uploaded in runs of frames of at most
    about ``run_bytes`` each (at least one frame) and resized run by run into one result, so a long clip never sits on the device whole.
    A y4m.Y4MClip is uploaded as runs of raw frame records and converted to RGB on the device before the resize (y4m_device_runs)."""
    from .y4m import Y4MClip
    t, h, w, c = clip.shape
    out = torch.empty((t, size, size, c), dtype=torch.uint8, device=device)
    if isinstance(clip, Y4MClip):
        for a, b, rgb in y4m_device_runs(clip, device, run_bytes):
            device_centre_square(rgb, size, out=out[a:b])
        return out
    per = max(1, int(run_bytes) // max(1, h * w * c))
    for a in range(0, t, per):
        run = torch.from_numpy(np.ascontiguousarray(clip[a:a + per])).to(device)
        device_centre_square(run, size, out=out[a:a + per])
    return out


def open_y4m(path, y4m=None):
    """The y4m.Y4MClip of a .y4m file; ``y4m``: {"matrix": ..., "range": ...} (y4m.Y4MClip's defaults where absent)."""
    from .y4m import Y4MClip
    return Y4MClip(path, **{k: v for k, v in (y4m or {}).items() if k in ("matrix", "range")})


def _read_frames(path, start, count, y4m=None):
    """Frames [start, start + count) of a clip as uint8 (T, H, W, 3) RGB, and the clip's total frame count.  A .y4m clip is converted
    on the host (y4m.yuv_to_rgb_reference), the requested frames only; ``y4m``: its matrix and range (open_y4m)."""
    if path.endswith(".npy"):
        arr = np.load(path, mmap_mode="r")
    elif path.endswith(Y4M_EXT):
        arr = open_y4m(path, y4m)
    elif path.endswith(".npz"):
        with np.load(path) as z:
            arr = z[z.files[0]]
    else:
        try:
            import cv2
        except ImportError as e:
            raise ValueError(f"{path}: compressed video needs OpenCV, which is not installed ({e})")
        cap = cv2.VideoCapture(path)
        if not cap.isOpened():
            raise ValueError(f"Could not open video: {path}")
        total = int(cap.get(cv2.CAP_PROP_FRAME_COUNT))
        start = start(total) if callable(start) else start
        frames, idx = [], 0
        while len(frames) < count:
            ok, frame = cap.read()
            if not ok:
                break
            if idx >= start:
                frames.append(cv2.cvtColor(frame, cv2.COLOR_BGR2RGB))
            idx += 1
        cap.release()
        if not frames:
            raise ValueError(f"No frames loaded from video: {path}")
        return np.stack(frames, 0), total
    if arr.ndim != 4 or arr.shape[-1] != 3 or arr.dtype != np.uint8:
        raise ValueError(f"{path}: expected uint8 (T, H, W, 3), got {arr.dtype} {arr.shape}")
    total = arr.shape[0]
    start = start(total) if callable(start) else start
    return np.asarray(arr[start:start + count]), total


def load_video_u8(path, max_frames, resize, crop_size, rng, device_resize=False, y4m=None):
    """One clip as (uint8 (max_frames, H, W, 3), float32 mask (max_frames,)); the recipe of train/dataloader.py:148-240.
    ``device_resize``: the final resize to ``resize`` is left to the device (DevicePrefetcher(resize=...)) and the clip comes back at
    crop_size x crop_size; everything before it, the draws from ``rng`` and the upscale of clips smaller than the crop included, is the
    same, so one rng picks the same window and crop in both modes.  ``y4m``: the matrix and range of .y4m clips (open_y4m)."""
    try:
        frames, _total = _read_frames(path, lambda total: int(rng.integers(0, max(total - max_frames, 0) + 1)), max_frames, y4m)
        if frames.shape[0] == 0:
            raise ValueError(f"No frames loaded from video: {path}")
        h, w = frames.shape[1:3]
        th, tw, sh, sw = get_random_crop_params(h, w, crop_size, rng)
        frames = _resize_u8(frames, th, tw)[:, sh:sh + crop_size, sw:sw + crop_size]
        if resize is not None and not device_resize:
            frames = _resize_u8(frames, resize[0], resize[1])
        n = frames.shape[0]
        out = np.zeros((max_frames,) + frames.shape[1:], dtype=np.uint8)
        out[:n] = frames
        mask = np.zeros((max_frames,), dtype=np.float32)
        mask[:n] = 1.0
        return out, mask
    except Exception as e:                                     # unreadable clip: zeros + all-ones mask, like the reference (:235-239)
        print(e, path)
        h, w = resize if resize is not None and not device_resize else (crop_size, crop_size)
        return np.zeros((max_frames, h, w, 3), dtype=np.uint8), np.ones((max_frames,), dtype=np.float32)


def _y4m_full(y4m):
    """The fallback's range: full only when ``y4m`` forces it (a clip that cannot be read has no header to ask)."""
    return (y4m or {}).get("range", "header") == "full"


def load_video_planes(path, max_frames, crop_size, rng, y4m=None, form=None):
    """One .y4m clip as plane bytes, no colour arithmetic: (y uint8 (max_frames, crop_size, crop_size), u, v uint8 (max_frames,) +
    y4m.window_chroma_shape (None for mono), params int32 (4,) = (top & 1, left & 1, full range, 0), float32 mask (max_frames,)):
    y4m.Y4MClip.window of the window and crop that load_video_u8 picks -- the same draws from ``rng`` in the same order, so one seed picks
    the same frames in every mode.  ``form`` = (chroma, siting) of the dataset (default: the clip's own).  Frames behind a short clip hold
    the padding value (y4m.pad_luma, y4m.PAD_CHROMA: RGB zero exactly); a clip that cannot be read -- a corrupt or truncated file, one
    whose form is not the dataset's or that is smaller than the crop -- yields padding-value planes with an all-ones mask (with no
    ``form`` to shape them by, the error is raised instead)."""
    from . import y4m as Y
    full = _y4m_full(y4m)
    try:
        clip = open_y4m(path, y4m)
        if form is None:
            form = (clip.chroma, clip.siting)
        if (clip.chroma, clip.siting) != tuple(form):
            raise ValueError(f"{path}: chroma form {(clip.chroma, clip.siting)} is not the dataset's {tuple(form)}")
        total, h, w, _ = clip.shape
        start = int(rng.integers(0, max(total - max_frames, 0) + 1))
        n = min(max_frames, total - start)
        if n <= 0:
            raise ValueError(f"No frames loaded from video: {path}")
        if h < crop_size or w < crop_size:
            raise ValueError(f"{path}: frames of {h}x{w} are smaller than the crop {crop_size}: the upscale is the host path's")
        _, _, top, left = get_random_crop_params(h, w, crop_size, rng)
        wy, wu, wv = clip.window(start, start + n, top, left, crop_size, crop_size)
        full = clip.full
        params = np.array([top & 1, left & 1, int(full), 0], dtype=np.int32)
        mask = np.zeros((max_frames,), dtype=np.float32)
        mask[:n] = 1.0
    except Exception as e:                                     # unreadable clip: RGB zeros + all-ones mask, as load_video_u8
        print(e, path)
        if form is None:
            raise
        n, wy, wu, wv = 0, None, None, None
        params = np.array([0, 0, int(full), 0], dtype=np.int32)
        mask = np.ones((max_frames,), dtype=np.float32)
    chroma = form[0]
    y = np.full((max_frames, crop_size, crop_size), Y.pad_luma(full), dtype=np.uint8)
    u = v = None
    if chroma != "mono":
        u, v = (np.full((max_frames,) + Y.window_chroma_shape(crop_size, crop_size, chroma), Y.PAD_CHROMA, dtype=np.uint8) for _ in range(2))
    if n:
        y[:n] = wy
        if u is not None:
            u[:n], v[:n] = wu, wv
    return y, u, v, params, mask


def load_video(path, max_frames=None, resize=None, crop_size=512, rng=None):
    """The reference's signature and return types: (float32 (T, H, W, 3) in [0, 1], float32 mask (T,))."""
    rng = rng if rng is not None else np.random.default_rng()
    v, m = load_video_u8(path, max_frames, resize, crop_size, rng)
    return v.astype(np.float32) / 255.0, m


class VideoDataSource:
    """Random-access source of clip paths (train/dataloader.py:243-256)."""

    def __init__(self, base_dir):
        self.video_paths = list_video_files(base_dir)
        print(f"Found {len(self.video_paths)} videos", file=sys.stderr)      # the reference prints this (train/dataloader.py:268); stderr keeps stdout for results

    def __len__(self):
        return len(self.video_paths)

    def __getitem__(self, idx):
        return self.video_paths[idx]


class _ClipDataset(torch.utils.data.Dataset):
    def __init__(self, source, max_frames, resize, crop_size, seed, device_resize=False, y4m=None, yuv_form=None):
        self.source, self.max_frames, self.resize, self.crop_size, self.seed = source, max_frames, resize, crop_size, seed
        self.device_resize, self.y4m, self.yuv_form = device_resize, y4m, yuv_form

    def __len__(self):
        return len(self.source)

    def __getitem__(self, item):
        epoch, idx = item
        rng = np.random.default_rng([self.seed, epoch, idx])  # crop / window depend on (seed, epoch, clip), not on the worker
        if self.yuv_form is not None:                         # device_yuv: plane bytes, (y, u, v, params, mask) with u, v None for mono
            return tuple(None if a is None else torch.from_numpy(a)
                         for a in load_video_planes(self.source[idx], self.max_frames, self.crop_size, rng, self.y4m, self.yuv_form))
        v, m = load_video_u8(self.source[idx], self.max_frames, self.resize, self.crop_size, rng, self.device_resize, self.y4m)
        return torch.from_numpy(v), torch.from_numpy(m)


class _EpochSampler(torch.utils.data.Sampler):
    """Shuffled clip indices, reshuffled every epoch from (seed, epoch); ``num_epochs=None`` streams forever (the
    claude_distributed loader has no epoch limit, the training loop caps the steps)."""

    def __init__(self, n, shuffle, seed, num_epochs):
        self.n, self.shuffle, self.seed, self.num_epochs = n, shuffle, seed, num_epochs

    def __iter__(self):
        epoch = 0
        while self.num_epochs is None or epoch < self.num_epochs:
            order = np.random.default_rng([self.seed, epoch]).permutation(self.n) if self.shuffle else np.arange(self.n)
            for i in order:
                yield (epoch, int(i))
            epoch += 1

    def __len__(self):
        return self.n * (self.num_epochs or 1)


def _collate(items):
    return {"video": torch.stack([v for v, _ in items]), "mask": torch.stack([m for _, m in items])}


def _collate_planes(items):
    names = ("y", "u", "v", "params", "mask")
    return {k: torch.stack([it[i] for it in items]) for i, k in enumerate(names) if items[0][i] is not None}


def _check_device_yuv(source, crop_size):
    """The refusals of ``device_yuv=True``, each naming the first offending file -> the dataset's (chroma, siting)."""
    from .y4m import read_header
    form = first = None
    for i in range(len(source)):
        path = source[i]
        if not path.endswith(Y4M_EXT):
            raise ValueError(f"device_yuv=True: {path} is not a .y4m clip (every clip of the folder must be one)")
        try:
            h = read_header(path)
        except (OSError, ValueError):
            continue                                           # unreadable: the zero-clip fallback at load time, as on the host path
        if form is None:
            form, first = (h.chroma, h.siting), path
        elif (h.chroma, h.siting) != form:
            raise ValueError(f"device_yuv=True: {path} is {h.chroma} ({h.siting} siting) but {first} is {form[0]} ({form[1]} siting): "
                             "one chroma form per dataset")
        if h.height < crop_size or h.width < crop_size:
            raise ValueError(f"device_yuv=True: {path} has frames of {h.height}x{h.width}, below the crop {crop_size}: the upscale of "
                             "small clips is the host path's")
    if form is None:
        raise ValueError(f"device_yuv=True: no readable .y4m header among the {len(source)} clips ({source[0]} ...)")
    return form


class BatchedDataLoader:
    """Iterable of host batches.  ``as_uint8=False`` (default) yields the reference's contract -- numpy float32 video in [0, 1] and
    float32 mask; ``as_uint8=True`` yields pinned uint8 torch tensors for DevicePrefetcher (4x fewer bytes over PCIe).
    ``device_resize=True`` (with ``as_uint8``) yields them at crop_size x crop_size: the resize is DevicePrefetcher(resize=...)'s.
    ``device_yuv=True`` (with ``as_uint8``; a folder of .y4m clips of one chroma form, none smaller than the crop) yields plane bytes
    {"y", "u", "v", "params", "mask"} (load_video_planes; no u, v for mono) for DevicePrefetcher(yuv=self.yuv, resize=...); ``yuv`` holds
    the dataset's {"chroma", "siting", "matrix"}.  ``y4m``: {"matrix", "range"} of .y4m clips, in every mode (open_y4m)."""

    def __init__(self, source, batch_size, max_frames, resize, crop_size, shuffle, seed, num_workers, prefetch_size, drop_remainder,
                 num_epochs, as_uint8, device_resize=False, device_yuv=False, y4m=None):
        if max_frames is None or (resize is None and crop_size is None):
            raise ValueError("batching needs max_frames and a fixed frame size (resize or crop_size)")
        if device_resize and not as_uint8:
            raise ValueError("device_resize=True needs as_uint8=True: the float32 contract batch has no device end to resize it")
        if device_yuv and not as_uint8:
            raise ValueError("device_yuv=True needs as_uint8=True: the float32 contract batch has no device end to convert it")
        self.as_uint8, self.yuv = as_uint8, None
        form = None
        if device_yuv:
            if crop_size is None:
                raise ValueError("device_yuv=True needs crop_size: the workers cut the crop out of the planes")
            form = _check_device_yuv(source, crop_size)
            self.yuv = {"chroma": form[0], "siting": form[1], "matrix": (y4m or {}).get("matrix", "bt601")}
        ds = _ClipDataset(source, max_frames, resize, crop_size, seed, device_resize, y4m, form)
        kw = {}
        if num_workers > 0:
            kw = dict(prefetch_factor=max(1, prefetch_size // max(1, num_workers)), persistent_workers=False)
        self.loader = torch.utils.data.DataLoader(ds, batch_size=batch_size, sampler=_EpochSampler(len(source), shuffle, seed, num_epochs),
                                                  num_workers=num_workers, collate_fn=_collate_planes if device_yuv else _collate,
                                                  drop_last=drop_remainder, pin_memory=as_uint8 and torch.cuda.is_available(), **kw)

    def __iter__(self):
        for b in self.loader:
            if self.as_uint8:
                yield b
            else:
                yield {"video": b["video"].numpy().astype(np.float32) / 255.0, "mask": b["mask"].numpy()}


def create_batched_dataloader(base_dir, batch_size=1, max_frames=None, resize=None, crop_size=512, shuffle=True, seed=42,
                              num_workers=4, prefetch_size=16, drop_remainder=False, rank=0, num_epochs=1, as_uint8=False,
                              device_resize=False, device_yuv=False, y4m=None):
    """The reference's factory (train/dataloader.py:334-390; per-rank form claude_distributed/dataloader.py:340-373):
    ``batch_size`` is the LOCAL batch of this rank, every rank shuffles the whole list with ``seed + rank``.
    ``num_epochs=None`` streams forever (the distributed variant).  ``device_resize``, ``device_yuv``, ``y4m``: BatchedDataLoader."""
    source = VideoDataSource(base_dir)
    if len(source) == 0:
        raise ValueError(f"no clips under {base_dir}")
    return BatchedDataLoader(source, batch_size, max_frames, resize, crop_size, shuffle, seed + rank, num_workers, prefetch_size,
                             drop_remainder, num_epochs, as_uint8, device_resize, device_yuv, y4m)


def apply_crop(frame, crop_size, crop_params):
    """One frame (H, W, 3) uint8 through the pre-computed crop of get_random_crop_params (train/dataloader.py:133-145)."""
    th, tw, sh, sw = crop_params
    if frame.shape[:2] != (th, tw):
        frame = _resize_u8(frame[None], th, tw)[0]
    return frame[sh:sh + crop_size, sw:sw + crop_size]


def _identity(item):
    return item


class _ClipIterator:
    """Unbatched clips, the reference's create_dataloader (train/dataloader.py:293-331): dicts with 'video' (T, H, W, 3) float32 in
    [0, 1] and 'mask' (T,)."""

    def __init__(self, source, max_frames, resize, crop_size, shuffle, seed, num_workers, prefetch_size):
        ds = _ClipDataset(source, max_frames, resize, crop_size, seed)
        kw = dict(prefetch_factor=max(1, prefetch_size), persistent_workers=False) if num_workers > 0 else {}
        self.loader = torch.utils.data.DataLoader(ds, batch_size=None, sampler=_EpochSampler(len(source), shuffle, seed, 1),
                                                  num_workers=num_workers, collate_fn=_identity, **kw)

    def __iter__(self):
        for v, m in self.loader:
            yield {"video": np.asarray(v).astype(np.float32) / 255.0, "mask": np.asarray(m)}


def create_dataloader(base_dir, batch_size=1, max_frames=None, resize=None, crop_size=512, shuffle=True, seed=42, num_workers=4,
                      prefetch_size=2):
    """train/dataloader.py:293-331: one clip per item (``batch_size`` is accepted and ignored there too: batching is
    create_batched_dataloader's)."""
    source = VideoDataSource(base_dir)
    if len(source) == 0:
        raise ValueError(f"no clips under {base_dir}")
    if max_frames is None:
        raise ValueError("create_dataloader needs max_frames (frame containers are read by range)")
    return _ClipIterator(source, max_frames, resize, crop_size, shuffle, seed, num_workers, prefetch_size)


def batch_to_video(batch, output_path, fps=30.0, use_mask=True, sample_idx=0, crf=18, preset="medium", y4m=None):
    """Write one sample of a batch as a video (train/dataloader.py:10-93): clip to [0, 1], scale to uint8, drop padded frames when
    ``use_mask``, H.264 through an ffmpeg pipe.  ``output_path`` ending in .npy / .npz writes the uint8 (T, H, W, 3) frame container
    the loader reads natively instead (no ffmpeg needed); ending in .y4m a YUV4MPEG2 clip (y4m.write on the host: no GPU, no ffmpeg;
    ``y4m``: its {"chroma", "matrix", "full"}, y4m.write's defaults where absent; ``fps`` may then be (n, d))."""
    import shutil
    import subprocess
    video, mask = batch["video"], batch["mask"]
    if isinstance(video, torch.Tensor):
        video = video.detach().float().cpu().numpy()
    if isinstance(mask, torch.Tensor):
        mask = mask.detach().float().cpu().numpy()
    video = np.clip(np.asarray(video, dtype=np.float32), 0, 1)
    mask = np.asarray(mask)
    if video.ndim == 5:
        video, mask = video[sample_idx], mask[sample_idx]
    video = (video * 255).astype(np.uint8)
    if use_mask:
        video = video[mask > 0.5]
    if len(video) == 0:
        raise ValueError("No frames to write (all frames are padded)")
    t, h, w, _ = video.shape
    if output_path.endswith(".npy"):
        np.save(output_path, video)
    elif output_path.endswith(".npz"):
        np.savez(output_path, frames=video)
    elif output_path.endswith(Y4M_EXT):
        from .y4m import write
        write(output_path, video, fps=fps, **{k: v for k, v in (y4m or {}).items() if k in ("chroma", "matrix", "full")})
    else:
        if not shutil.which("ffmpeg"):
            raise RuntimeError("ffmpeg not found on PATH.")
        cmd = ["ffmpeg", "-y", "-f", "rawvideo", "-pix_fmt", "rgb24", "-s", f"{w}x{h}", "-r", str(fps), "-i", "pipe:0", "-vcodec", "libx264",
               "-pix_fmt", "yuv420p", "-crf", str(crf), "-preset", preset, output_path]
        proc = subprocess.Popen(cmd, stdin=subprocess.PIPE)
        try:
            for frame in video:
                proc.stdin.write(frame.tobytes())
        finally:
            proc.stdin.close()
            proc.wait()
            if proc.returncode != 0:
                raise RuntimeError("ffmpeg failed.")
    print(f"Saved video to {output_path} ({len(video)} frames, {w}x{h}, {fps} fps)", file=sys.stderr)


class DevicePrefetcher:
    """Host batches -> device batches, one step ahead, on a side stream.

    A background thread pulls the next host batch (the worker processes decode, crop and resize), stages it in one of two
    pinned buffers and issues the H2D copy plus the uint8 -> [0, 1] conversion on ``self.stream``; ``__next__`` makes the
    caller's current stream wait on that stream's event and hands over device tensors that stay valid until the
    batch after next is requested (two device slots).  Yields {"video": ``dtype`` (B, T, H, W, 3) in [0, 1], "mask": float32 (B, T)}.

    ``resize=(h, w)`` (batches of a loader with ``device_resize=True``): the uint8 batch (B, T, H0, W0, 3) is resized to (B, T, h, w, 3),
    divided by 255 and written in ``dtype`` by ONE kernel launch on the side stream (ops.crop_resize_norm over all B T frames, the whole
    frame as the crop) instead of the three framework launches: the values of the host resize followed by the conversion, bit for bit.

    ``yuv={"chroma", "siting", "matrix"}`` with ``resize=(h, w)`` (batches of a loader with ``device_yuv=True``, whose ``yuv`` attribute is
    this dict): the planes and params are uploaded as they are and ONE launch on the side stream (ops.yuv_window_resize_norm) converts them
    to RGB, resizes, divides by 255 and writes ``dtype``: the host loader's batch, bit for bit.
    """

    def __init__(self, batches, device, dtype=torch.float32, depth=2, resize=None, yuv=None):
        if yuv is not None and resize is None:
            raise ValueError("DevicePrefetcher(yuv=...) needs resize=(h, w): the one launch converts and resizes")
        self.device, self.dtype, self.resize, self.yuv = device, dtype, resize, yuv
        self.stream = torch.cuda.Stream(device=device)
        self.div255 = torch.full((), 255.0, dtype=torch.float32, device=device)
        self.q = queue.Queue(maxsize=depth)
        self.slots, self.slot = [None] * (depth + 1), 0
        self.err = None
        self.thread = threading.Thread(target=self._run, args=(iter(batches),), daemon=True)
        self.thread.start()

    def _planes_to_device(self, b):
        if "y" not in b or "params" not in b or (self.yuv["chroma"] != "mono" and ("u" not in b or "v" not in b)):
            raise ValueError(f"DevicePrefetcher(yuv=...) takes plane batches (y, u, v, params, mask: a loader with device_yuv=True); "
                             f"got {sorted(b)}")
        from . import ops
        host = {k: (t if t.is_pinned() else t.pin_memory()) for k, t in b.items()}
        with torch.cuda.stream(self.stream):
            d = {k: t.to(self.device, non_blocking=True) for k, t in host.items()}
            b_, t_, h0, w0 = d["y"].shape
            flat = lambda t: t.reshape((b_ * t_,) + tuple(t.shape[2:]))
            mono = self.yuv["chroma"] == "mono"
            # the uploads were allocated on self.stream and are freed to it: their memory is handed out again only behind this launch
            dv = ops.yuv_window_resize_norm(flat(d["y"]), None if mono else flat(d["u"]), None if mono else flat(d["v"]), d["params"], t_,
                                            self.yuv["chroma"], self.yuv["siting"], self.yuv["matrix"], self.resize[0], self.resize[1],
                                            dtype=self.dtype).view(b_, t_, self.resize[0], self.resize[1], 3)
            dm = d["mask"].float()
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return {"video": dv, "mask": dm}, ev, host

    def _to_device(self, b):
        if self.yuv is not None:
            return self._planes_to_device(b)
        video, mask = b["video"], b["mask"]
        if isinstance(video, np.ndarray):                          # contract-shaped float32 host batch
            video, mask = torch.from_numpy(video), torch.from_numpy(mask)
        if not video.is_pinned():
            video = video.pin_memory()
        with torch.cuda.stream(self.stream):
            dv = video.to(self.device, non_blocking=True)
            dm = mask.to(self.device, non_blocking=True).float()
            if self.resize is not None:
                if dv.dtype != torch.uint8 or dv.dim() != 5:
                    raise ValueError(f"DevicePrefetcher(resize=...) takes uint8 (B, T, H, W, 3) batches; got {dv.dtype} {tuple(dv.shape)}")
                from . import ops
                b_, t_, h0, w0, c = dv.shape
                # dv was allocated on self.stream and is freed to it: the allocator hands its memory out again only behind this launch
                dv = ops.crop_resize_norm(dv.reshape(b_ * t_, h0, w0, c), 0, 0, h0, w0, self.resize[0], self.resize[1],
                                          dtype=self.dtype).view(b_, t_, self.resize[0], self.resize[1], c)
            elif dv.dtype == torch.uint8:
                # the reference's astype(float32) / 255.0, done after the copy.  The divisor is a device TENSOR on purpose: with a
                # Python scalar the framework multiplies by the rounded reciprocal, which is 1 ulp off a true division for some k
                dv = torch.div(dv.float(), self.div255).to(self.dtype)
            else:
                dv = dv.to(self.dtype)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return {"video": dv, "mask": dm}, ev, video

    def _run(self, it):
        try:
            torch.cuda.set_device(self.device)
            for b in it:
                self.q.put(self._to_device(b))
        except Exception as e:                                     # surfaced by __next__
            self.err = e
        self.q.put(None)

    def __iter__(self):
        return self

    def __next__(self):
        item = self.q.get()
        if item is None:
            if self.err is not None:
                raise self.err
            raise StopIteration
        batch, ev, host = item
        torch.cuda.current_stream(self.device).wait_event(ev)
        for t in batch.values():
            t.record_stream(torch.cuda.current_stream(self.device))
        self.slots[self.slot] = (batch, host)                      # keeps the pinned source alive until its copy has surely run
        self.slot = (self.slot + 1) % len(self.slots)
        return batch


def write_synthetic_clips(base_dir, n_clips, frames, height, width, seed=0, ext=".npy"):
    """A folder of random uint8 clips (.npy, (frames, height, width, 3)) in the reference's directory layout: test / bench data
    (there is no network for a real dataset).  ``ext=".y4m"``: the same frames written as 4:2:0 YUV4MPEG2 clips (y4m.write)."""
    d = os.path.join(base_dir, "videos0")
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    for i in range(n_clips):
        t = frames if i % 3 else max(1, frames - frames // 4)      # every third clip is short: exercises padding + mask
        clip = rng.integers(0, 256, size=(t, height, width, 3), dtype=np.uint8)
        if ext == ".y4m":
            from .y4m import write
            write(os.path.join(d, f"clip{i:04d}.y4m"), clip)
        else:
            np.save(os.path.join(d, f"clip{i:04d}.npy"), clip)
    return d
