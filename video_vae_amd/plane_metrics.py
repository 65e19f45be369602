"""Plane-wise metrics of 8-bit Y'CbCr planes: PSNR-Y, PSNR-U, PSNR-V, the sample-pooled PSNR-YUV and SSIM-Y, the numbers the codec world
quotes beside a bit rate.  This module is the specification of csrc/plane_metrics.hip (ops.plane_metrics_u8).

Operands are two sets of uint8 planes of one shape, the reference first and the test second: ``y`` (n, H, W), ``u`` and ``v`` (n, CH, CW)
with y4m.chroma_shape's CH and CW for "420" and "444"; for "mono" ``u`` and ``v`` are None.

  * ``sse[f, p]`` int64: the sum over plane p (0 = Y, 1 = U, 2 = V) of frame f of (a - b)^2, exact.  ``samples[p]`` int64: the samples
    of plane p of one frame.  A mono clip has sse[:, 1:] = 0 and samples[1:] = 0.
  * ``mse[f, p]`` = sse / samples_p / 255^2 in float64: the data range is 1, as everywhere in metrics.py.
  * ``psnr[f, p]`` = 10 log10(1 / max(mse, 1e-10)): metrics.py's rule, identical planes give 100 dB, never inf.  A plane with 0 samples
    reports 0 (mse and psnr).
  * ``psnr_yuv[f]``: the same formula applied to (sse_y + sse_u + sse_v) / (n_y + n_u + n_v) / 255^2: pooled over the samples, what
    ffmpeg's psnr filter calls "average"; at 4:2:0 the 4 : 1 : 1 weighting.
  * ``ssim_y[f]``: metrics.py's SSIM of the Y plane taken as a one-channel frame y / 255 (11-tap Gaussian, sigma 1.5, valid positions
    only, C1 = 0.01^2, C2 = 0.03^2).  float64 on the host route, fp32 from the kernel.

``mse`` and ``psnr`` are formed in float64 from the exact integers on both routes.  Supported: 11 <= H, W <= 8192, chroma "420" | "444" |
"mono", any n >= 1; anything else is a ValueError naming the limits.  There is no mask: callers slice the real frames (planes are views).
"""
from typing import NamedTuple

import numpy as np
import torch

from . import y4m
from .metrics import WIN

MIN_SIDE, MAX_SIDE = WIN, 8192
CHROMAS = y4m.CHROMAS
KEYS = ("psnr_y", "psnr_u", "psnr_v", "psnr_yuv", "ssim_y", "mse_y")


class PlaneMetrics(NamedTuple):
    """Per-frame plane metrics: ``sse`` int64 (n, 3), ``samples`` int64 (3,), ``mse`` and ``psnr`` float64 (n, 3), ``psnr_yuv`` float64
    (n,), ``ssim_y`` (n,) float64 (host) or fp32 (kernel); numpy arrays from arrays and CPU tensors, tensors on the device from GPU tensors."""
    sse: object
    samples: object
    mse: object
    psnr: object
    psnr_yuv: object
    ssim_y: object


def _limits():
    return f"{MIN_SIDE} <= H, W <= {MAX_SIDE}, chroma one of {CHROMAS}, uint8 planes y (n, H, W), u and v (n, CH, CW), n >= 1"


def check_planes(ref, test, chroma):
    """ValueError unless ``ref`` and ``test`` are (y, u, v) of uint8 planes of one supported shape in the ``chroma`` form -> (n, H, W).
    Shapes and dtypes only: nothing is read."""
    if chroma not in CHROMAS:
        raise ValueError(f"plane_metrics: chroma {chroma!r} ({_limits()})")
    if len(ref) != 3 or len(test) != 3:
        raise ValueError(f"plane_metrics: each operand is (y, u, v) ({_limits()})")
    u8 = lambda p: str(p.dtype) in ("uint8", "torch.uint8")
    y = ref[0]
    if len(y.shape) != 3 or not u8(y):
        raise ValueError(f"plane_metrics: y is {y.dtype} {tuple(y.shape)} ({_limits()})")
    n, h, w = (int(s) for s in y.shape)
    if n < 1 or not (MIN_SIDE <= h <= MAX_SIDE and MIN_SIDE <= w <= MAX_SIDE):
        raise ValueError(f"plane_metrics: {n} frames of {h}x{w} ({_limits()})")
    cshape = (n,) + y4m.chroma_shape(h, w, chroma)
    for name, (py, pu, pv) in (("reference", ref), ("test", test)):
        if tuple(py.shape) != (n, h, w) or not u8(py):
            raise ValueError(f"plane_metrics: the {name}'s y is {py.dtype} {tuple(py.shape)}, expected uint8 {(n, h, w)} ({_limits()})")
        if chroma == "mono":
            continue
        for what, p in (("u", pu), ("v", pv)):
            if p is None or tuple(p.shape) != cshape or not u8(p):
                got = "None" if p is None else f"{p.dtype} {tuple(p.shape)}"
                raise ValueError(f"plane_metrics: the {name}'s {what} is {got}, expected uint8 {cshape} for {chroma} frames of {h}x{w} "
                                 f"({_limits()})")
    return n, h, w


def samples_of(h, w, chroma):
    """int64 (3,): the samples of the Y, U and V planes of one h x w frame (0 for the chroma of mono)."""
    ch, cw = y4m.chroma_shape(h, w, chroma)
    return np.array([h * w, ch * cw, ch * cw], dtype=np.int64)


def _derive(sse, samples):
    """float64 (mse (n, 3), psnr (n, 3), psnr_yuv (n,)) of exact int64 ``sse`` (n, 3) and ``samples`` (3,), numpy."""
    sse, samples = np.asarray(sse, dtype=np.int64), np.asarray(samples, dtype=np.int64)
    has = samples > 0
    mse = np.where(has, sse.astype(np.float64) / np.maximum(samples, 1).astype(np.float64) / 255.0 ** 2, 0.0)
    psnr = np.where(has, 10.0 * np.log10(1.0 / np.maximum(mse, 1e-10)), 0.0)
    pooled = sse.sum(axis=1).astype(np.float64) / float(samples.sum()) / 255.0 ** 2
    return mse, psnr, 10.0 * np.log10(1.0 / np.maximum(pooled, 1e-10))


def _np(p):
    return p.numpy() if torch.is_tensor(p) else np.asarray(p)


def plane_metrics_reference(ref, test, chroma="420"):
    """The definition on the host -> ``PlaneMetrics`` of numpy arrays: the squared errors in int64, SSIM-Y in float64
    (metrics._frame_metrics_composed's arithmetic on y / 255 as a one-channel frame, kept in float64; a few frames at a time)."""
    n, h, w = check_planes(ref, test, chroma)
    sse = np.zeros((n, 3), dtype=np.int64)
    ssim = np.empty((n,), dtype=np.float64)
    per = max(1, (1 << 20) // (h * w))                                 # frames at a time: the float64 planes stay small
    for s in range(0, n, per):
        for p in range(1 if chroma == "mono" else 3):
            d = _np(ref[p])[s:s + per].astype(np.int64) - _np(test[p])[s:s + per].astype(np.int64)
            sse[s:s + per, p] = (d * d).reshape(d.shape[0], -1).sum(axis=1)
        x = torch.from_numpy(np.array(_np(ref[0])[s:s + per])).to(torch.float64) / 255.0
        y = torch.from_numpy(np.array(_np(test[0])[s:s + per])).to(torch.float64) / 255.0
        ssim[s:s + per] = _ssim_f64(x, y)
    samples = samples_of(h, w, chroma)
    return PlaneMetrics(sse, samples, *_derive(sse, samples), ssim)


def _ssim_f64(x, y):
    """metrics.py's SSIM of (t, h, w) float64 one-channel frames in [0, 1], kept in float64 -> numpy (t,)."""
    import torch.nn.functional as F
    from .metrics import C1, C2, gaussian_window
    t, h, w = x.shape
    xp, yp = x.reshape(t, 1, h, w), y.reshape(t, 1, h, w)
    g = gaussian_window(torch.float64)
    q = torch.cat([xp, yp, xp * xp, yp * yp, xp * yp], dim=1)
    q = F.conv2d(q, g.view(1, 1, WIN, 1).expand(5, 1, WIN, 1), groups=5)
    q = F.conv2d(q, g.view(1, 1, 1, WIN).expand(5, 1, 1, WIN), groups=5)
    ux, uy, uxx, uyy, uxy = q.unbind(1)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    s = (2 * ux * uy + C1) * (2 * vxy + C2) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return s.reshape(t, -1).mean(dim=1).numpy()


def plane_metrics(ref, test, chroma="420"):
    """``PlaneMetrics`` of the test's planes against the reference's (module docstring).  GPU tensors run the HIP kernel
    (ops.plane_metrics_u8: exact integer sums and fp32 SSIM-Y from one pass over the bytes; the planes may be views of uploaded frame
    records) and give tensors on the device; CPU tensors and numpy arrays run ``plane_metrics_reference``."""
    n, h, w = check_planes(ref, test, chroma)
    if not (torch.is_tensor(ref[0]) and ref[0].is_cuda):
        return plane_metrics_reference(ref, test, chroma)
    from . import ops
    sse, ssim = ops.plane_metrics_u8(ref, test, chroma)
    dev = sse.device
    samples = torch.from_numpy(samples_of(h, w, chroma)).to(dev)
    has = samples > 0
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    mse = torch.where(has, sse.double() / samples.clamp_min(1).double() / 255.0 ** 2, zero)
    psnr = torch.where(has, 10.0 * torch.log10(1.0 / mse.clamp_min(1e-10)), zero)
    pooled = sse.sum(dim=1).double() / float(samples.sum()) / 255.0 ** 2
    return PlaneMetrics(sse, samples, mse, psnr, 10.0 * torch.log10(1.0 / pooled.clamp_min(1e-10)), ssim)


def summarize_planes(pm):
    """Per-clip means over the frames (the project's convention: the mean of per-frame values) -> {"frames", "psnr_y", "psnr_u",
    "psnr_v", "psnr_yuv", "ssim_y", "mse_y"} of Python numbers."""
    host = lambda v: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)).astype(np.float64)
    psnr, mse = host(pm.psnr), host(pm.mse)
    return {"frames": int(psnr.shape[0]), "psnr_y": float(psnr[:, 0].mean()), "psnr_u": float(psnr[:, 1].mean()),
            "psnr_v": float(psnr[:, 2].mean()), "psnr_yuv": float(host(pm.psnr_yuv).mean()), "ssim_y": float(host(pm.ssim_y).mean()),
            "mse_y": float(mse[:, 0].mean())}


def per_frame_planes(pm):
    """The per-frame lists of a ``PlaneMetrics`` and its integer ``sse`` rows, as eval's and compare's --per-frame JSON stores them."""
    host = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    psnr, mse = host(pm.psnr).astype(np.float64), host(pm.mse).astype(np.float64)
    return {"psnr_y": psnr[:, 0].tolist(), "psnr_u": psnr[:, 1].tolist(), "psnr_v": psnr[:, 2].tolist(),
            "psnr_yuv": host(pm.psnr_yuv).astype(np.float64).tolist(), "ssim_y": host(pm.ssim_y).astype(np.float64).tolist(),
            "mse_y": mse[:, 0].tolist(), "sse": [[int(v) for v in row] for row in host(pm.sse)]}


def concat_planes(parts):
    """Several ``PlaneMetrics`` of one frame shape (runs of one clip) -> one, on the host."""
    host = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    cat = lambda k: np.concatenate([host(getattr(p, k)) for p in parts])
    return PlaneMetrics(cat("sse"), host(parts[0].samples), cat("mse"), cat("psnr"), cat("psnr_yuv"), cat("ssim_y").astype(np.float64))
