"""The latent quantiser and the rate of a quantised clip.

One quantiser, uniform, symmetric and scalar, with one step per (kept frame, latent channel) -- so its definition does not depend on
batches, windows, tiles or scenes.  For a frame's latent ``x`` (hw, ld) and ``bits`` in 2 .. 8, ``qmax = 2^(bits - 1) - 1``, all in
float32 with every operation rounded on its own:

  * ``amax[c] = max_i |x[i, c]|``;
  * a channel is dead when ``amax[c]`` is 0, not finite or below 1e-30: ``step[c] = 0`` and every code 0;
  * otherwise ``inv[c] = float32(qmax) / amax[c]``, ``step[c] = amax[c] / float32(qmax)``,
    ``q[i, c] = clamp(rint(x[i, c] * inv[c]), -qmax, qmax)`` (ties to even), stored as int8;
  * dequantised ``xq[i, c] = float32(q[i, c]) * step[c]``; ``|xq - x| <= 0.5 step (1 + 2^-10)``.

``quantise_reference`` / ``dequantise_reference`` below are the definition; ``ops.latent_quantise`` (csrc/quant.hip) equals them on every
bit.  ``fake_quant_reference`` is what the decoder sees under quantisation-aware training (``ops.latent_fake_quant``).
``rate_cost_reference`` / ``rate_reference`` define the rate term of that training (``ops.latent_rate``): the bits a zeroth-order coder
would spend, as a piecewise-linear function of the unrounded codes.  ``rate_summary`` turns the code histograms of a clip into bits and
bits per pixel.
"""
from typing import NamedTuple

import numpy as np

BITS_MIN, BITS_MAX = 2, 8
DEAD_BELOW = np.float32(1e-30)


class QuantisedLatents(NamedTuple):
    """What ``ops.latent_quantise`` returns."""
    codes: object            # int8 (..., hw, ld)
    step: object             # float32 (..., ld)
    counts: object           # int32 (..., 256): counts[..., q + 128] = elements of the frame with code q


def qmax_of(bits):
    bits = int(bits)
    if not BITS_MIN <= bits <= BITS_MAX:
        raise ValueError(f"quantiser bits {bits}: {BITS_MIN} .. {BITS_MAX}")
    return (1 << (bits - 1)) - 1


def _scales_reference(x, qmax):
    """x float32 (frames, hw, ld) -> (amax, dead, inv, step), (frames, ld) each: the per-channel rules above, under the caller's errstate."""
    amax = np.abs(x).max(axis=1) if x.shape[0] else np.zeros((0, x.shape[2]), dtype=np.float32)
    dead = ~np.isfinite(amax) | (amax < DEAD_BELOW)
    safe = np.where(dead, np.float32(1), amax).astype(np.float32)
    inv = np.where(dead, np.float32(0), qmax / safe).astype(np.float32)
    step = np.where(dead, np.float32(0), safe / qmax).astype(np.float32)
    return amax, dead, inv, step


def quantise_reference(mean, bits):
    """``mean`` (frames, hw, ld) (or one frame (hw, ld)) -> (codes int8 of that shape, step float32 (frames, ld)).  Plain numpy float32."""
    qmax = np.float32(qmax_of(bits))
    x = np.asarray(mean, dtype=np.float32)
    single = x.ndim == 2
    if single:
        x = x[None]
    if x.ndim != 3:
        raise ValueError(f"mean {x.shape}: (frames, hw, ld) expected")
    with np.errstate(all="ignore"):
        _, dead, inv, step = _scales_reference(x, qmax)
        r = np.clip(np.rint((x * inv[:, None, :]).astype(np.float32)), -qmax, qmax)
        r = np.where(dead[:, None, :], np.float32(0), r)
    codes = r.astype(np.int8)
    return (codes[0] if single else codes), step


def dequantise_reference(codes, step):
    """codes int8 (frames, hw, ld), step float32 (frames, ld) -> float32 (frames, hw, ld): float32(q) * step."""
    q = np.asarray(codes)
    s = np.asarray(step, dtype=np.float32)
    if q.ndim != 3 or s.shape != (q.shape[0], q.shape[2]):
        raise ValueError(f"codes {q.shape} with step {s.shape}: (frames, hw, ld) and (frames, ld) expected")
    return (q.astype(np.float32) * s[:, None, :]).astype(np.float32)


def _round_to_bf16(x):
    """float32 -> the nearest bfloat16 (ties to even), held in float32; a NaN stays a NaN."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)).astype(np.uint32)
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    return np.where(nan, u | np.uint32(0x00400000), r).astype(np.uint32).view(np.float32)


def fake_quant_reference(x, keep, bits, dtype="float32"):
    """What the decoder is trained on under quantisation-aware training (ops.latent_fake_quant, csrc/quant.hip: equal on every bit).
    ``x`` float32 (frames, hw, ld), ``keep`` (frames,), ``dtype`` float32 or bfloat16 (a name, a numpy or a torch dtype) -> float32
    (frames, hw, ld) holding values of ``dtype``: a frame whose ``keep`` flag is nonzero becomes
    ``dequantise_reference(*quantise_reference(x, bits))`` rounded once to ``dtype``; every other frame is ``x`` unchanged, bit for bit,
    NaN payloads included.

    The value goes through the INTEGER code: ``float32(int8 q) * step``.  A code 0 therefore dequantises to +0.0 and never to -0.0,
    whatever the sign of ``x``.  A restatement as ``rint(x * inv) * step`` without the integer conversion keeps the sign of a value that
    rounds to zero and differs from this definition in the sign of zero."""
    name = getattr(dtype, "__name__", None) or str(dtype).replace("torch.", "")
    if name not in ("float32", "bfloat16"):
        raise ValueError(f"fake_quant_reference: dtype {dtype}: float32 or bfloat16")
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 3:
        raise ValueError(f"x {x.shape}: (frames, hw, ld) expected")
    k = np.asarray(keep).reshape(-1) != 0
    if k.shape[0] != x.shape[0]:
        raise ValueError(f"keep holds {k.shape[0]} flags for {x.shape[0]} frames")
    out = x.copy()
    if k.any():
        xq = dequantise_reference(*quantise_reference(x[k], bits))
        out[k] = _round_to_bf16(xq) if name == "bfloat16" else xq
    else:
        qmax_of(bits)
    return out


RATE_ALPHA = 0.5


def rate_cost_reference(counts, bits, alpha=RATE_ALPHA):
    """The price in bits of each code under the batch's own pooled histogram (the table ``ops.latent_rate`` interpolates):
    ``counts`` (..., 256) pooled to n[256], N = sum n, A = 2 qmax + 1; for s in 128 - qmax .. 128 + qmax
    ``C[s] = log2(N + A alpha) - log2(n[s] + alpha)`` (additive smoothing: the prices are those of a distribution that sums to one over
    the alphabet), 0 elsewhere -> float32 (256,).  float32 with every operation rounded on its own (the counts are pooled as integers);
    an empty histogram gives the constant table log2(A alpha) - log2(alpha)."""
    qmax = qmax_of(bits)
    n = np.asarray(counts).astype(np.int64).reshape(-1, 256).sum(axis=0)
    nf = n.astype(np.float32)
    a = np.float32(alpha)
    total = np.float32(np.float32(n.sum()) + np.float32(np.float32(2 * qmax + 1) * a))
    cost = (np.log2(total) - np.log2((nf + a).astype(np.float32))).astype(np.float32)
    s = np.arange(256)
    return np.where(np.abs(s - 128) <= qmax, cost, np.float32(0)).astype(np.float32)


def rate_reference(x, keep, bits, cost):
    """The relaxed code cost of a latent (ops.latent_rate, csrc/quant.hip): ``x`` float32 (frames, hw, ld), ``keep`` (frames,), ``cost``
    float32 (256,) (rate_cost_reference) -> (terms, slope), float32 (frames, hw, ld) each.  With amax, dead and inv exactly those of
    quantise_reference, for a kept frame and a live channel c, every operation rounded on its own:
      v = x inv[c];  k = clamp(floor(v), -qmax, qmax - 1);  t = v - k;  d = C[k + 129] - C[k + 128];
      term = C[k + 128] + t d;  slope = d inv[c].
    (t is exact for v >= 0 and v <= -1; in -1 < v < 0 it is 1 + v rounded once.)  A dead channel gives term 0 and slope 0, a frame whose
    keep flag is zero gives zeros.  The rate of a frame is the sum of its terms: the
    piecewise-linear interpolation of the cost table at the UNROUNDED code, which equals C[q + 128] wherever v is the integer q.
    ``slope`` is d term / d x with amax (hence inv) and the table held constant: both are stop-gradient, the rate's gradient moves a
    value towards the cheaper neighbouring code and neither rescales its channel nor reprices the codes."""
    iq = qmax_of(bits)
    qmax = np.float32(iq)
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 3:
        raise ValueError(f"x {x.shape}: (frames, hw, ld) expected")
    kept = np.asarray(keep).reshape(-1) != 0
    if kept.shape[0] != x.shape[0]:
        raise ValueError(f"keep holds {kept.shape[0]} flags for {x.shape[0]} frames")
    c = np.asarray(cost, dtype=np.float32).reshape(-1)
    if c.shape[0] != 256:
        raise ValueError(f"cost {np.shape(cost)}: 256 entries expected")
    with np.errstate(all="ignore"):
        _, dead, inv, _ = _scales_reference(x, qmax)
        v = (x * inv[:, None, :]).astype(np.float32)
        v = np.where(dead[:, None, :], np.float32(0), v)              # x * 0 may be NaN in a dead channel
        kf = np.clip(np.floor(v), -qmax, qmax - np.float32(1)).astype(np.float32)
        t = (v - kf).astype(np.float32)
        k = kf.astype(np.int64)
        lo = c[k + 128]
        d = (c[k + 129] - lo).astype(np.float32)
        terms = (lo + (t * d).astype(np.float32)).astype(np.float32)
        slope = (d * inv[:, None, :]).astype(np.float32)
    off = dead[:, None, :] | ~kept[:, None, None]
    zero = np.float32(0)
    return np.where(off, zero, terms).astype(np.float32), np.where(off, zero, slope).astype(np.float32)


def code_counts(codes):
    """int64 (256,): the pooled histogram of int8 codes, counts[q + 128] (what the kernel's per-frame counts sum to)."""
    return np.bincount(np.asarray(codes).astype(np.int64).reshape(-1) + 128, minlength=256).astype(np.int64)


def entropy_bits(counts):
    """The zeroth-order entropy in bits per symbol of a histogram (0 log 0 = 0; an empty histogram gives 0)."""
    c = np.asarray(counts, dtype=np.float64).reshape(-1)
    n = c.sum()
    if n <= 0:
        return 0.0
    p = c[c > 0] / n
    return float(max(0.0, -(p * np.log2(p)).sum()))


def rate_summary(counts, selection, n_frames, height, width, ld, bits, coded=None, coded_context=None, coded_temporal=None):
    """The rate of one clip from ONE pooled histogram: ``counts`` (256,) or (frames, 256) (summed) over all kept frames and channels,
    ``selection`` the stored frame gate (any shape; its nonzero entries are the kept frames).  With N = the number of codes,
    p = counts / N and pixels = n_frames height width:
      bits_raw = N bits;  bits_entropy = N H(p);  bits_side = kept ld 32 + n_frames (the steps, one selection bit per frame);
      bpp_raw = (bits_raw + bits_side) / pixels;  bpp_entropy = (bits_entropy + bits_side) / pixels.
    Also ``codes`` = N, ``kept`` and ``pixels``, so that dataset figures can be formed as ratios of sums (``rate_dataset``).  ``coded``
    (entropy.coded_bits of the clip's range-coded stream) adds bits_coded = coded + bits_side and bpp_coded = bits_coded / pixels;
    ``coded_context`` (the same of the context coder's stream) adds bits_coded_context / bpp_coded_context likewise, and
    ``coded_temporal`` (of the temporal coder's) bits_coded_temporal / bpp_coded_temporal."""
    qmax_of(bits)
    c = np.asarray(counts, dtype=np.int64)
    c = c.reshape(-1, 256).sum(axis=0)
    n = int(c.sum())
    kept = int(np.count_nonzero(np.asarray(selection)))
    pixels = int(n_frames) * int(height) * int(width)
    bits_raw = n * int(bits)
    bits_entropy = n * entropy_bits(c)
    bits_side = kept * int(ld) * 32 + int(n_frames)
    out = {"codes": n, "kept": kept, "pixels": pixels, "bits_raw": bits_raw, "bits_entropy": bits_entropy, "bits_side": bits_side,
           "bpp_raw": (bits_raw + bits_side) / pixels, "bpp_entropy": (bits_entropy + bits_side) / pixels}
    if coded is not None:
        out["bits_coded"] = int(coded) + bits_side
        out["bpp_coded"] = out["bits_coded"] / pixels
    if coded_context is not None:
        out["bits_coded_context"] = int(coded_context) + bits_side
        out["bpp_coded_context"] = out["bits_coded_context"] / pixels
    if coded_temporal is not None:
        out["bits_coded_temporal"] = int(coded_temporal) + bits_side
        out["bpp_coded_temporal"] = out["bits_coded_temporal"] / pixels
    return out


def rate_dataset(summaries):
    """Dataset figures of several clips' ``rate_summary``: ratios of sums, not means of ratios."""
    s = list(summaries)
    tot = {k: sum(r[k] for r in s) for k in ("codes", "kept", "pixels", "bits_raw", "bits_entropy", "bits_side")}
    pixels = tot["pixels"]
    tot["bpp_raw"] = (tot["bits_raw"] + tot["bits_side"]) / pixels if pixels else 0.0
    tot["bpp_entropy"] = (tot["bits_entropy"] + tot["bits_side"]) / pixels if pixels else 0.0
    if s and all("bits_coded" in r for r in s):            # every clip was range-coded: bits_coded holds its side bits already
        tot["bits_coded"] = sum(r["bits_coded"] for r in s)
        tot["bpp_coded"] = tot["bits_coded"] / pixels if pixels else 0.0
    if s and all("bits_coded_context" in r for r in s):
        tot["bits_coded_context"] = sum(r["bits_coded_context"] for r in s)
        tot["bpp_coded_context"] = tot["bits_coded_context"] / pixels if pixels else 0.0
    if s and all("bits_coded_temporal" in r for r in s):
        tot["bits_coded_temporal"] = sum(r["bits_coded_temporal"] for r in s)
        tot["bpp_coded_temporal"] = tot["bits_coded_temporal"] / pixels if pixels else 0.0
    return tot
