"""Scene-cut detection: the frames of a clip where a new shot starts, from per-frame colour histograms.

The rule is the reference's data preparation (``hist_diff_indices_pil``), restated exactly:
  * per frame, a histogram of its pixels in one of two spaces:
      - "hsv": OpenCV's 8-bit ``COLOR_RGB2HSV`` (hsv_shift 12): v = max(r, g, b), diff = v - min(r, g, b),
        s = (diff sdiv[v] + 2048) >> 12, h = g - b (v == r) | b - r + 2 diff (v == g) | r - g + 4 diff, h = (h hdiv[diff] + 2048) >> 12
        (arithmetic shift), h += 180 if h < 0, with sdiv[i] = round((255 << 12) / i), hdiv[i] = round((180 << 12) / (6 i)), both 0 at 0;
        then the 2-D (H, S) histogram of ``cv2.calcHist([hsv], [0, 1], None, [n, n], [0, 180, 0, 256])``: n x n bins, H bin
        floor(j (n / 180.0)), S bin floor(j (n / 256.0)) (float64, OpenCV's order: the scale first; clamped to n - 1);
      - "gray": OpenCV's 8-bit ``COLOR_RGB2GRAY``, Y = (4899 R + 9617 G + 1868 B + 8192) >> 14, n bins, bin floor(Y (n / 256.0));
  * the correlation of consecutive histograms, ``cv2.HISTCMP_CORREL`` on the raw counts (s12 - s1 s2 / N over sqrt((s11 - s1^2 / N)
    (s22 - s2^2 / N)), N = bins, the sums exact integers converted to float64; 1.0 when |denominator| <= DBL_EPSILON).  The reference
    L2-normalises each histogram first; the correlation does not change under scaling, so that step is dropped;
  * ``change_indices``: acc += 1 - corr; frame i is a cut when acc > 1 - similarity, and acc restarts at 0.

GPU tensors run the HIP kernels (``ops.scene_hist`` / ``ops.scene_corr``, csrc/scenes.hip); CPU tensors a composed numpy path, which is
the definition the tests hold the kernels to.  ``change_indices`` is L - 1 scalar steps and runs on the host.
"""
import math
import sys

import numpy as np
import torch

SPACES = ("hsv", "gray")
HSV_SHIFT = 12


def _check(hist_size, space):
    if space not in SPACES:
        raise ValueError(f"space {space!r}: one of {SPACES}")
    top = 64 if space == "hsv" else 256
    if not 1 <= int(hist_size) <= top:
        raise ValueError(f"hist_size {hist_size}: 1 .. {top} for {space}")


def hsv_divisors():
    """(sdiv, hdiv) int64 (256,): OpenCV's rounded 8-bit RGB -> HSV divisor tables (entry 0 = 0; no entry has a .5 tie)."""
    sdiv, hdiv = np.zeros(256, dtype=np.int64), np.zeros(256, dtype=np.int64)
    for i in range(1, 256):
        sdiv[i] = round((255 << HSV_SHIFT) / i)
        hdiv[i] = round((180 << HSV_SHIFT) / (6 * i))
    return sdiv, hdiv


def bin_table(n, span):
    """int64 (256,): the bin of each 8-bit value j over [0, span) in n bins, as cv2.calcHist's uniform ranges: floor(j * (n / span)) in
    float64, clamped to n - 1."""
    a = n / float(span)
    return np.array([min(math.floor(j * a), n - 1) for j in range(256)], dtype=np.int64)


def tables(hist_size, space):
    """The int32 tables the kernel reads: "hsv" [sdiv | hdiv | H bins | S bins] (1024,), "gray" [Y bins] (256,)."""
    _check(hist_size, space)
    if space == "gray":
        return bin_table(hist_size, 256).astype(np.int32)
    sdiv, hdiv = hsv_divisors()
    return np.concatenate([sdiv, hdiv, bin_table(hist_size, 180), bin_table(hist_size, 256)]).astype(np.int32)


def rgb_to_hsv(rgb):
    """uint8 (..., 3) RGB -> (h, s, v) int64 arrays of the leading shape: OpenCV's 8-bit COLOR_RGB2HSV (module docstring)."""
    x = np.asarray(rgb).astype(np.int64)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    sdiv, hdiv = hsv_divisors()
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    s = (diff * sdiv[v] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    h = h + np.where(h < 0, 180, 0)
    return h, s, v


def rgb_to_gray(rgb):
    """uint8 (..., 3) RGB -> int64 Y of the leading shape: OpenCV's 8-bit COLOR_RGB2GRAY."""
    x = np.asarray(rgb).astype(np.int64)
    return (4899 * x[..., 0] + 9617 * x[..., 1] + 1868 * x[..., 2] + 8192) >> 14


def _bins(clip, hist_size, space):
    """int64 (L, H W): every pixel's bin."""
    x = np.asarray(clip).reshape(clip.shape[0], -1, 3)
    if space == "gray":
        return bin_table(hist_size, 256)[rgb_to_gray(x)]
    h, s, _ = rgb_to_hsv(x)
    return bin_table(hist_size, 180)[h] * hist_size + bin_table(hist_size, 256)[s]


def frame_histograms(clip, hist_size=64, space="hsv"):
    """uint8 RGB clip (L, H, W, 3) -> int32 (L, bins) exact pixel counts per frame, bins = hist_size^2 ("hsv") or hist_size ("gray")."""
    _check(hist_size, space)
    if clip.dim() != 4 or clip.shape[3] != 3 or clip.dtype != torch.uint8:
        raise ValueError(f"clip must be uint8 (L, H, W, 3); got {clip.dtype} {tuple(clip.shape)}")
    if clip.is_cuda:
        from . import ops
        return ops.scene_hist(clip, hist_size, space)[0]
    bins = hist_size * hist_size if space == "hsv" else hist_size
    idx = _bins(clip.numpy(), hist_size, space)
    flat = idx + (np.arange(idx.shape[0], dtype=np.int64) * bins)[:, None]
    counts = np.bincount(flat.reshape(-1), minlength=idx.shape[0] * bins).reshape(idx.shape[0], bins)
    return torch.from_numpy(counts.astype(np.int32))


def correl(a, b):
    """cv2.HISTCMP_CORREL of two integer count vectors, in float64 from exact integer sums (module docstring)."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    s1, s2 = float(int(a.sum())), float(int(b.sum()))
    s11, s22, s12 = float(int((a * a).sum())), float(int((b * b).sum())), float(int((a * b).sum()))
    scale = 1.0 / a.shape[0]
    num = s12 - s1 * s2 * scale
    denom2 = (s11 - s1 * s1 * scale) * (s22 - s2 * s2 * scale)
    return num / math.sqrt(denom2) if abs(denom2) > sys.float_info.epsilon else 1.0


def histogram_correlation(counts):
    """int32 counts (L, bins) -> float64 (L - 1,): the correlation of each frame's histogram with the next one's."""
    if counts.dim() != 2:
        raise ValueError(f"counts must be (L, bins); got {tuple(counts.shape)}")
    if counts.is_cuda:
        from . import ops
        return ops.scene_corr(counts)
    c = counts.numpy()
    return torch.tensor([correl(c[i], c[i + 1]) for i in range(c.shape[0] - 1)], dtype=torch.float64)


def change_indices(corr, similarity=0.85):
    """The reference's change-point rule over consecutive-frame correlations ``corr`` (L - 1 values): frame i (1 .. L - 1) is a cut when
    the accumulated 1 - corr since the last cut exceeds 1 - similarity."""
    acc, cuts = 0.0, []
    thresh = 1 - similarity
    for i, sim in enumerate((float(v) for v in np.asarray(torch.as_tensor(corr).cpu()).reshape(-1)), start=1):
        acc += 1 - sim
        if acc > thresh:
            cuts.append(i)
            acc = 0.0
    return cuts


def scene_cuts(clip, hist_size=64, similarity=0.85, space="hsv"):
    """uint8 RGB clip (L, H, W, 3) -> the sorted frame indices (1 .. L - 1) that start a new scene."""
    _check(hist_size, space)
    if clip.is_cuda:
        from . import ops
        if clip.dtype != torch.uint8 or clip.dim() != 4 or clip.shape[3] != 3:
            raise ValueError(f"clip must be uint8 (L, H, W, 3); got {clip.dtype} {tuple(clip.shape)}")
        corr = ops.scene_hist(clip, hist_size, space)[1]
    else:
        corr = histogram_correlation(frame_histograms(clip, hist_size, space))
    return change_indices(corr.cpu(), similarity)


def scene_ranges(cuts, length):
    """[[start, end), ...] of the scenes a clip of ``length`` frames splits into at ``cuts``."""
    b = [0] + [int(c) for c in cuts] + [int(length)]
    return [[b[i], b[i + 1]] for i in range(len(b) - 1)]
