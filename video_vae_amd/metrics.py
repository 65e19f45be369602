"""Reconstruction metrics: per-frame MSE, PSNR and SSIM of a clip against its reconstruction, honouring the (b, t) frame mask.

Definition (what ``vvae_recon_metrics_fwd`` computes and ``tests/test_metrics_host.py`` pins against a float64 numpy restatement):

  * ``video``, ``recon`` (B, T, H, W, C), fp32 or bf16 each, are converted to fp32 and, with ``clamp=True`` (default), clamped to [0, 1]
    (what ``data.batch_to_video`` writes out).  C is 1..4, H and W are at least 11.
  * ``mse[b, t]`` = mean over H W C of (x - y)^2;  ``psnr[b, t]`` = 10 log10(1 / max(mse, 1e-10)), so at most 100 dB.
  * ``ssim[b, t]`` (Wang et al. 2004) per channel, averaged over the channels: an 11-tap Gaussian window, sigma 1.5, normalised to sum 1,
    applied separably over rows and columns at the valid positions only (rows and columns 5 .. n - 6);  mx = g * x, sx = g * x^2 - mx^2,
    sxy = g * (x y) - mx my (likewise for y);  S = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sx + sy + C2)), C1 = 0.01^2,
    C2 = 0.03^2;  the frame's value is the mean of S over the valid region and the channels.  This is
    ``skimage.metrics.structural_similarity(x, y, data_range=1, channel_axis=-1, gaussian_weights=True, sigma=1.5,
    use_sample_covariance=False)``.
  * Frames the mask marks 0 get mse = psnr = ssim = 0 (never NaN) and are never read on the GPU.  Clip values are means over the valid
    frames; a clip without one reports 0 with a frame count of 0.  ``kept_fraction[b]`` = sum(selection mask) / sum(mask) (rl flavour).

Temporal consistency (``temporal_mse``, the HIP kernel ``ops.temporal_mse`` on GPU tensors): for consecutive frames t - 1, t of a clip
``x`` and its reconstruction ``y``, both converted to fp32 and clamped to [0, 1], ``tmse[b, t - 1]`` = mean over H W C of
((y_t - y_{t-1}) - (x_t - x_{t-1}))^2: zero where the reconstruction changes from frame to frame exactly as the clip does, large where it
flickers (a seam between windows that per-frame metrics cannot see).  A clip of one frame has no pairs.

Multi-scale SSIM (``ms_ssim(video, recon, mask, clamp=True, weights=MS_SSIM_WEIGHTS)`` -> fp32 (B, T); Wang, Simoncelli, Bovik 2003;
``MS_SSIM_WEIGHTS`` = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)).  ``weights`` is any tuple of 1 to 5 non-negative floats; its length
is the number of scales M, and it is used as given, without renormalising.

  1. x and y are converted to fp32 and, with ``clamp``, clamped to [0, 1]: level 0.
  2. Level j + 1 from level j, both operands: H' = H // 2, W' = W // 2 (an odd trailing row or column is dropped),
     v'[i, k, c] = ((v[2i, 2k, c] + v[2i, 2k+1, c]) + (v[2i+1, 2k, c] + v[2i+1, 2k+1, c])) * 0.25, kept in fp32.  This is
     ``F.avg_pool2d(., 2)``; it differs from pytorch-msssim only on odd extents, where that package zero-pads.
  3. At every level, per channel c, with the window and moments above (11 taps, sigma 1.5, valid positions only, C1, C2):
     CS = (2 sxy + C2) / (sx + sy + C2), S = (2 mx my + C1) / (mx^2 + my^2 + C1) CS; cs_j[c] and ssim_j[c] are the means of CS and S
     over the valid positions of channel c.
  4. ms_ssim = mean over c of ( prod_{j < M-1} max(cs_j[c], 0)^{w_j} * max(ssim_{M-1}[c], 0)^{w_{M-1}} ), powers and product in
     float64: the per-channel product followed by the channel mean, as pytorch-msssim and ``tf.image.ssim_multiscale`` do.
  5. A masked frame gives 0 and is never read.

Supported: 1 <= C <= 4, 1 <= M <= 5, min(H, W) >> (M - 1) >= 11 (176 at five scales), W <= 8192, B T <= 65535; anything else is a
ValueError naming the smallest frame the chosen M takes.  ``return_terms=True`` also returns ``terms`` fp32 (B, T, M, C), 0 on masked
frames: the unclamped cs_j[c] for j < M - 1 and the unclamped ssim_{M-1}[c].  GPU tensors run ``ops.ms_ssim`` (per level a per-channel
moment pass of the SSIM kernel and a 2 x 2 pool, then one fold), CPU tensors the composed path (the pyramid in fp32, the rest float64).

SSIM as a training loss: ``ssim_grad_reference(video, recon, mask, gout, clamp=True, video_div=1)`` states the per-frame SSIM above and its
gradient with respect to ``recon`` in closed form (float64, no autograd); ``ops.ssim_frames`` is the differentiable operator (HIP forward and
backward on GPU tensors, ``ssim_frames_composed`` through framework autograd on CPU tensors) and ``loss.add_ssim_term`` the loss term.

GPU tensors run the HIP kernel (``ops.recon_metrics``: one pass over both operands plus a fold over the bands; a shape it does not take
raises ``VvaeError``).  CPU tensors run the same definition composed from framework ops in float64.  ``frame_metrics_wide`` takes frames
up to 8192 wide (a row of more than 2048 values runs in column strips on the GPU).
"""
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2
WIN, SIGMA = 11, 1.5


class FrameMetrics(NamedTuple):
    """Per-frame metrics, each (B, T) fp32; 0 on masked frames."""
    mse: torch.Tensor
    psnr: torch.Tensor
    ssim: torch.Tensor


class ClipMetrics(NamedTuple):
    """Per-clip means over the valid frames, each (B,) fp32 (0 for a clip without a valid frame); ``frames`` (B,) int64 valid-frame
    counts; ``kept_fraction`` (B,) fp32 when a selection was given, else None."""
    mse: torch.Tensor
    psnr: torch.Tensor
    ssim: torch.Tensor
    frames: torch.Tensor
    kept_fraction: Optional[torch.Tensor]


def gaussian_window(dtype=torch.float64):
    """The 11 normalised Gaussian taps (sigma 1.5)."""
    k = torch.arange(WIN, dtype=torch.float64) - WIN // 2
    g = torch.exp(-k * k / (2 * SIGMA * SIGMA))
    return (g / g.sum()).to(dtype)


def _check(video, recon, mask):
    if video.dim() != 5 or recon.shape != video.shape:
        raise ValueError(f"video and recon must be (B, T, H, W, C) of one shape; got {tuple(video.shape)} and {tuple(recon.shape)}")
    b, t, h, w, c = video.shape
    if h < WIN or w < WIN:
        raise ValueError(f"frames of {h}x{w}: SSIM's {WIN}-tap window needs H and W >= {WIN}")
    if not 1 <= c <= 4:
        raise ValueError(f"{c} channels: 1 to 4 are supported")
    if tuple(mask.shape) != (b, t):
        raise ValueError(f"mask of shape {tuple(mask.shape)}, expected {(b, t)}")
    if recon.device != video.device or mask.device != video.device:
        raise ValueError("video, recon and mask must be on one device")


def _frame_metrics_composed(video, recon, mask, clamp):
    """The definition from framework ops in float64 (CPU tensors)."""
    b, t, h, w, c = video.shape
    x, y = video.to(torch.float64), recon.to(torch.float64)
    if clamp:
        x, y = x.clamp(0, 1), y.clamp(0, 1)
    mse = ((x - y) ** 2).mean(dim=(2, 3, 4))
    psnr = 10 * torch.log10(1 / mse.clamp_min(1e-10))
    planes = lambda v: v.permute(0, 1, 4, 2, 3).reshape(b * t * c, 1, h, w)
    xp, yp = planes(x), planes(y)
    g = gaussian_window(torch.float64)
    q = torch.cat([xp, yp, xp * xp, yp * yp, xp * yp], dim=1)                    # (n, 5, h, w)
    q = F.conv2d(q, g.view(1, 1, WIN, 1).expand(5, 1, WIN, 1), groups=5)         # rows
    q = F.conv2d(q, g.view(1, 1, 1, WIN).expand(5, 1, 1, WIN), groups=5)         # columns
    ux, uy, uxx, uyy, uxy = q.unbind(1)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    s = (2 * ux * uy + C1) * (2 * vxy + C2) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    ssim = s.reshape(b, t, -1).mean(dim=2)
    valid = mask != 0
    zero = torch.zeros((), dtype=torch.float64)
    return FrameMetrics(*(torch.where(valid, v, zero).to(torch.float32) for v in (mse, psnr, ssim)))


def frame_metrics(video, recon, mask, clamp=True):
    """Per-frame MSE, PSNR (dB) and SSIM of ``recon`` against ``video`` (module docstring) -> ``FrameMetrics``, each (B, T) fp32.

    video, recon (B, T, H, W, C) fp32 or bf16 (independently); mask (B, T), nonzero = valid frame.  GPU tensors run the HIP kernel, CPU
    tensors the composed path; the outputs are fresh tensors."""
    _check(video, recon, mask)
    if video.is_cuda:
        from . import ops
        return FrameMetrics(*ops.recon_metrics(video, recon, mask, clamp))
    return _frame_metrics_composed(video, recon, mask.to(torch.float32), clamp)


def _ssim_operands(video, recon, mask, video_div):
    """float64 x (the clip, each sample repeated ``video_div`` times), y, the (B, T) validity -> (x, y, valid); masked frames are replaced
    by zeros (they are never read)."""
    as_f64 = lambda v: (v if torch.is_tensor(v) else torch.as_tensor(v)).to(torch.float64)
    x, y = as_f64(video), as_f64(recon)
    if x.dim() != 5 or y.dim() != 5 or video_div < 1 or x.shape[0] * video_div != y.shape[0] or x.shape[1:] != y.shape[1:]:
        raise ValueError(f"video {tuple(x.shape)} and recon {tuple(y.shape)}: (B / {video_div}, T, H, W, C) and (B, T, H, W, C)")
    if video_div > 1:
        x = x.repeat_interleave(video_div, dim=0)
    _check(x, y, torch.as_tensor(mask))
    valid = torch.as_tensor(mask).to(y.device) != 0
    keep = valid.view(*valid.shape, 1, 1, 1)
    zero = torch.zeros((), dtype=torch.float64, device=y.device)
    return torch.where(keep, x, zero), torch.where(keep, y, zero), valid


def _ssim_moments(x, y):
    """float64 (B, T, H, W, C) -> mx, my, g * x^2, g * y^2, g * x y at the valid positions, each (B T C, 1, H - 10, W - 10)."""
    b, t, h, w, c = y.shape
    planes = lambda v: v.permute(0, 1, 4, 2, 3).reshape(b * t * c, 1, h, w)
    xp, yp = planes(x), planes(y)
    g = gaussian_window(torch.float64).to(y.device)
    q = torch.cat([xp, yp, xp * xp, yp * yp, xp * yp], dim=1)
    q = F.conv2d(q, g.view(1, 1, WIN, 1).expand(5, 1, WIN, 1), groups=5)
    q = F.conv2d(q, g.view(1, 1, 1, WIN).expand(5, 1, 1, WIN), groups=5)
    return [v.unsqueeze(1) for v in q.unbind(1)]


def ssim_frames_composed(video, recon, mask, clamp=True, video_div=1):
    """Per-frame SSIM (module docstring) of ``recon`` (B, T, H, W, C) against sample i // video_div of ``video``, composed from framework
    ops in float64 -> fp32 (B, T), 0 on masked frames; differentiable with respect to ``recon`` through framework autograd (what
    ``ops.ssim_frames`` runs for CPU tensors, and what ``ssim_grad_reference`` is tested against)."""
    x, y, valid = _ssim_operands(video, recon, mask, video_div)
    if clamp:
        x, y = x.clamp(0, 1), y.clamp(0, 1)
    ux, uy, uxx, uyy, uxy = _ssim_moments(x, y)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    s = (2 * ux * uy + C1) * (2 * vxy + C2) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    ssim = s.reshape(y.shape[0], y.shape[1], -1).mean(dim=2)
    return torch.where(valid, ssim, torch.zeros((), dtype=torch.float64, device=y.device)).to(torch.float32)


def ssim_grad_reference(video, recon, mask, gout, clamp=True, video_div=1):
    """The SSIM loss's specification: per-frame SSIM and its gradient with respect to ``recon`` in closed form, float64, no autograd.

    video (B / video_div, T, H, W, C), recon (B, T, H, W, C), numpy or torch; sample i of recon is compared with sample i // video_div of
    video (the rl flavour's pair doubling, as in ``ops.masked_mse_mae``); mask (B, T), nonzero = valid frame; gout (B, T) the upstream
    gradient per frame.  -> (ssim (B, T), drecon (B, T, H, W, C)), float64 torch tensors.

    Per channel, at every valid position p (rows and columns 5 .. n - 6), with the window and moments of the module docstring and
    a1 = 2 mx my + C1, a2 = 2 sxy + C2, b1 = mx^2 + my^2 + C1, b2 = sx + sy + C2, S = a1 a2 / (b1 b2):
      A  = dS/dmy        = 2 mx (a2 - a1) / (b1 b2) + 2 my S (1 / b2 - 1 / b1)
      Bm = dS/d(g * y^2) = -S / b2
      Cm = dS/d(g * x y) = 2 a1 / (b1 b2)
      drecon(q) = gout[f] / (C (H - 10)(W - 10)) [ (G^T A)(q) + 2 y(q) (G^T Bm)(q) + x(q) (G^T Cm)(q) ]
    where G^T is the transposed separable window: the 11 taps applied along rows and columns to the map zero-extended by 5 on every side,
    so the result has the frame's H x W positions.  ``clamp``: x and y are clamped to [0, 1] first and the gradient is 0 where y lies
    strictly outside [0, 1] (it passes at exactly 0 and 1, as ``torch.clamp``'s does).  Masked frames: ssim 0, gradient 0, never read."""
    with torch.no_grad():
        x, y, valid = _ssim_operands(video, recon, mask, video_div)
        b, t, h, w, c = y.shape
        go = torch.as_tensor(gout).to(torch.float64).to(y.device).reshape(b, t)
        inside = (y >= 0) & (y <= 1)
        if clamp:
            x, y = x.clamp(0, 1), y.clamp(0, 1)
        mx, my, uxx, uyy, uxy = _ssim_moments(x, y)
        sx, sy, sxy = uxx - mx * mx, uyy - my * my, uxy - mx * my
        a1, a2, b1, b2 = 2 * mx * my + C1, 2 * sxy + C2, mx * mx + my * my + C1, sx + sy + C2
        s = a1 * a2 / (b1 * b2)
        map_a = 2 * mx * (a2 - a1) / (b1 * b2) + 2 * my * s * (1 / b2 - 1 / b1)
        map_b = -s / b2
        map_c = 2 * a1 / (b1 * b2)
        g = gaussian_window(torch.float64).to(y.device)

        def transposed(m):                                # zero-extended by 5, then the 11 taps: H x W positions
            m = F.conv2d(m, g.view(1, 1, WIN, 1), padding=(WIN - 1, 0))
            m = F.conv2d(m, g.view(1, 1, 1, WIN), padding=(0, WIN - 1))
            return m.reshape(b, t, c, h, w).permute(0, 1, 3, 4, 2)

        scale = go / (c * (h - 10) * (w - 10))
        d = (transposed(map_a) + 2 * y * transposed(map_b) + x * transposed(map_c)) * scale.view(b, t, 1, 1, 1)
        zero = torch.zeros((), dtype=torch.float64, device=y.device)
        if clamp:
            d = torch.where(inside, d, zero)
        d = torch.where(valid.view(b, t, 1, 1, 1), d, zero)
        ssim = torch.where(valid, s.reshape(b, t, -1).mean(dim=2), zero)
        return ssim, d


MAX_WIDE_W = 8192


def frame_metrics_wide(video, recon, mask, clamp=True):
    """``frame_metrics`` for frames of any width 11 <= W <= 8192 (C <= 4): the same definition and outputs.  GPU tensors run the kernel's
    column-strip path (``ops.recon_metrics_wide``) where a row holds more than 2048 values, and exactly ``frame_metrics``' launches (bitwise
    its results) for every shape that takes; CPU tensors the composed path."""
    _check(video, recon, mask)
    if video.shape[3] > MAX_WIDE_W:
        raise ValueError(f"frames {video.shape[3]} wide: at most {MAX_WIDE_W}")
    if video.is_cuda:
        from . import ops
        return FrameMetrics(*ops.recon_metrics_wide(video, recon, mask, clamp))
    return _frame_metrics_composed(video, recon, mask.to(torch.float32), clamp)


MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MS_SSIM_MAX_SCALES = 5


def ms_ssim_min_side(scales):
    """The smallest frame side ``scales`` levels take: the last level must still hold the 11-tap window (176 at five scales)."""
    return WIN << (scales - 1)


def ms_ssim_check(h, w, c, scales, frames=1):
    """ValueError unless ``frames`` frames of h x w x c can be measured at ``scales`` levels (module docstring, MS-SSIM)."""
    if not 1 <= scales <= MS_SSIM_MAX_SCALES:
        raise ValueError(f"ms_ssim at {scales} scales: 1 to {MS_SSIM_MAX_SCALES} are supported")
    side = ms_ssim_min_side(scales)
    note = f"{scales} scales take frames of {side}x{side} and larger"
    if min(h, w) >> (scales - 1) < WIN:
        raise ValueError(f"ms_ssim: frames of {h}x{w} are too small: {note} (the last level must hold the {WIN}-tap window)")
    if not 1 <= c <= 4:
        raise ValueError(f"ms_ssim: {c} channels: 1 to 4 are supported ({note})")
    if w > MAX_WIDE_W:
        raise ValueError(f"ms_ssim: frames {w} wide: at most {MAX_WIDE_W} ({note})")
    if frames > 65535:
        raise ValueError(f"ms_ssim: {frames} frames in one call: at most 65535 ({note})")


def pool2x2(v):
    """The next pyramid level of fp32 ``v`` (..., H, W, C) -> (..., H // 2, W // 2, C): the 2 x 2 means in the definition's order,
    ((v00 + v01) + (v10 + v11)) * 0.25 in fp32; an odd trailing row or column is dropped."""
    h2, w2 = v.shape[-3] // 2 * 2, v.shape[-2] // 2 * 2
    v = v[..., :h2, :w2, :]
    top = v[..., 0::2, 0::2, :] + v[..., 0::2, 1::2, :]
    bot = v[..., 1::2, 0::2, :] + v[..., 1::2, 1::2, :]
    return (top + bot) * 0.25


def _level_terms(x, y):
    """One level, fp32 (n, h, w, c) -> the means of CS and of S over the valid positions, float64 (n, c) each."""
    n, h, w, c = x.shape
    planes = lambda v: v.to(torch.float64).permute(0, 3, 1, 2).reshape(n * c, 1, h, w)
    xp, yp = planes(x), planes(y)
    g = gaussian_window(torch.float64)
    q = torch.cat([xp, yp, xp * xp, yp * yp, xp * yp], dim=1)
    q = F.conv2d(q, g.view(1, 1, WIN, 1).expand(5, 1, WIN, 1), groups=5)
    q = F.conv2d(q, g.view(1, 1, 1, WIN).expand(5, 1, 1, WIN), groups=5)
    ux, uy, uxx, uyy, uxy = q.unbind(1)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    cs = (2 * vxy + C2) / (vx + vy + C2)
    s = (2 * ux * uy + C1) / (ux * ux + uy * uy + C1) * cs
    return cs.reshape(n, c, -1).mean(dim=2), s.reshape(n, c, -1).mean(dim=2)


def _ms_ssim_composed(video, recon, mask, clamp, weights):
    """The definition from framework ops (CPU tensors): the pyramid in fp32, everything else in float64 -> (ms_ssim, terms)."""
    b, t, h, w, c = video.shape
    m = len(weights)
    x, y = video.to(torch.float32).reshape(b * t, h, w, c), recon.to(torch.float32).reshape(b * t, h, w, c)
    if clamp:
        x, y = x.clamp(0, 1), y.clamp(0, 1)
    terms = []
    for j in range(m):
        both = [_level_terms(x[i:i + 8], y[i:i + 8]) for i in range(0, b * t, 8)]  # 8 frames at a time: the float64 planes stay small
        terms.append(torch.cat([s if j == m - 1 else cs for cs, s in both]))
        if j < m - 1:
            x, y = pool2x2(x), pool2x2(y)
    terms = torch.stack(terms, dim=1)                                            # (n, m, c) float64
    wts = torch.tensor(weights, dtype=torch.float64).view(1, m, 1)
    ms = (terms.clamp_min(0) ** wts).prod(dim=1).mean(dim=1)
    valid = mask.reshape(b * t) != 0
    zero = torch.zeros((), dtype=torch.float64)
    ms = torch.where(valid, ms, zero).to(torch.float32).reshape(b, t)
    terms = torch.where(valid.view(-1, 1, 1), terms, zero).to(torch.float32).reshape(b, t, m, c)
    return ms, terms


def ms_ssim(video, recon, mask, clamp=True, weights=MS_SSIM_WEIGHTS, return_terms=False):
    """Per-frame multi-scale SSIM of ``recon`` against ``video`` (module docstring) -> fp32 (B, T), 0 on masked frames; with
    ``return_terms`` also ``terms`` fp32 (B, T, M, C): the unclamped cs_j[c] of the levels below the last and ssim_{M-1}[c].

    video, recon (B, T, H, W, C) fp32 or bf16 (independently); mask (B, T), nonzero = valid frame; ``weights``: 1 to 5 non-negative
    floats, one per scale, used as given.  A shape outside the supported ones is a ValueError naming the smallest frame the scales
    take.  GPU tensors run the HIP kernels (``ops.ms_ssim``), CPU tensors the composed path; the outputs are fresh tensors."""
    weights = tuple(float(v) for v in weights)
    if not 1 <= len(weights) <= MS_SSIM_MAX_SCALES:
        raise ValueError(f"ms_ssim: {len(weights)} weights: one per scale, 1 to {MS_SSIM_MAX_SCALES}")
    if any(not 0.0 <= v < float("inf") for v in weights):
        raise ValueError(f"ms_ssim: weights {weights} must be non-negative and finite")
    if video.dim() != 5 or recon.shape != video.shape:
        raise ValueError(f"video and recon must be (B, T, H, W, C) of one shape; got {tuple(video.shape)} and {tuple(recon.shape)}")
    b, t, h, w, c = video.shape
    ms_ssim_check(h, w, c, len(weights), b * t)
    _check(video, recon, mask)
    if video.is_cuda:
        from . import ops
        ms, terms = ops.ms_ssim(video, recon, mask, clamp, weights, return_terms)
    else:
        ms, terms = _ms_ssim_composed(video, recon, mask.to(torch.float32), clamp, weights)
    return (ms, terms) if return_terms else ms


def summarize(fm, mask, selection=None):
    """Clip means of per-frame metrics over the valid frames -> ``ClipMetrics`` (see there).  ``selection`` (B, T): the frame gate
    (rl flavour), giving ``kept_fraction``."""
    valid = (mask.reshape(fm.mse.shape) != 0).to(torch.float32)
    n = valid.sum(dim=1)
    den = n.clamp_min(1)
    means = [(v * valid).sum(dim=1) / den for v in fm]
    kept = None
    if selection is not None:
        kept = (selection.reshape(valid.shape).to(torch.float32) * valid).sum(dim=1) / den
    return ClipMetrics(*means, n.to(torch.int64), kept)


def clip_metrics(video, recon, mask, selection=None, clamp=True):
    """Per-clip means of ``frame_metrics`` over the valid frames, the valid-frame counts and, when ``selection`` is given, the kept
    fraction sum(selection mask) / sum(mask) -> ``ClipMetrics``."""
    return summarize(frame_metrics(video, recon, mask, clamp), mask, selection)


def _temporal_mse_composed(video, recon, clamp):
    x, y = video.to(torch.float64), recon.to(torch.float64)
    if clamp:
        x, y = x.clamp(0, 1), y.clamp(0, 1)
    d = (y[:, 1:] - y[:, :-1]) - (x[:, 1:] - x[:, :-1])
    return (d * d).mean(dim=(2, 3, 4)).to(torch.float32)


def temporal_mse(video, recon, clamp=True):
    """Temporal-difference error of each pair of consecutive frames (module docstring) -> fp32 (B, T - 1) (empty for T = 1).

    video, recon (B, T, H, W, C) fp32 or bf16 (independently), C 1..4.  GPU tensors run the HIP kernel, CPU tensors the definition in
    float64 (rounded to fp32 at the end)."""
    if video.dim() != 5 or recon.shape != video.shape:
        raise ValueError(f"video and recon must be (B, T, H, W, C) of one shape; got {tuple(video.shape)} and {tuple(recon.shape)}")
    if not 1 <= video.shape[4] <= 4:
        raise ValueError(f"{video.shape[4]} channels: 1 to 4 are supported")
    if recon.device != video.device:
        raise ValueError("video and recon must be on one device")
    if video.is_cuda:
        from . import ops
        return ops.temporal_mse(video, recon, clamp)
    return _temporal_mse_composed(video, recon, clamp)


def temporal_summary(tmse, window):
    """One clip's pair values ``tmse`` (n - 1,) -> {"tmse", "tmse_seam", "tmse_inner", "pairs", "seam_pairs"}: the means over all pairs,
    over the pairs whose later frame index is a positive multiple of ``window`` (the seams of hard cuts), and over the others; each 0
    where it has no pair."""
    v = [float(a) for a in (tmse.tolist() if hasattr(tmse, "tolist") else tmse)]
    seam = [a for t, a in enumerate(v, start=1) if t % window == 0]
    inner = [a for t, a in enumerate(v, start=1) if t % window != 0]
    mean = lambda a: sum(a) / len(a) if a else 0.0
    return {"tmse": mean(v), "tmse_seam": mean(seam), "tmse_inner": mean(inner), "pairs": len(v), "seam_pairs": len(seam)}


def temporal_summary_scenes(tmse, window, cuts):
    """``temporal_summary`` of a clip cut into scenes at ``cuts``: adds "tmse_scene" / "scene_pairs", the mean over the pairs whose later
    frame is a cut (a change of content, not an error of the model); "tmse_seam" / "seam_pairs" and "tmse_inner" then cover the
    remaining pairs (later frame a positive multiple of ``window``, or not)."""
    v = [float(a) for a in (tmse.tolist() if hasattr(tmse, "tolist") else tmse)]
    cut = set(int(c) for c in cuts)
    scene = [a for t, a in enumerate(v, start=1) if t in cut]
    seam = [a for t, a in enumerate(v, start=1) if t not in cut and t % window == 0]
    inner = [a for t, a in enumerate(v, start=1) if t not in cut and t % window != 0]
    mean = lambda a: sum(a) / len(a) if a else 0.0
    return {"tmse": mean(v), "tmse_seam": mean(seam), "tmse_inner": mean(inner), "pairs": len(v), "seam_pairs": len(seam),
            "tmse_scene": mean(scene), "scene_pairs": len(scene)}
