"""The evaluation kernels, held per band, per strip and per window: metrics.hip (the moment pass in its one-strip, strip and multi-scale
forms, the pools, the folds), plane_metrics.hip (the Y plane) and temporal_metrics.hip.

Observables, the finest each entry gives:
  * vvae_recon_metrics_fwd / _wide_fwd through lib() with the test's own buffers: the partial pair (se, ss) of every (frame, strip, band)
    at part[((f strips + strip) bands + band) 2], and mse, psnr, ssim per frame.
  * ops.ms_ssim(want_terms=True): the term of every (frame, level, channel), and the result.
  * ops.plane_metrics_u8: sse (int64) and ssim_y per frame.
  * vvae_temporal_mse_fwd with the test's own buffers: part[pair chunks + chunk] and tmse.

Every case asserts the regime it means to reach from Python mirrors of rm_plan, ssim_bands, ssim_rows, ms_plan, pm_dims and the
temporal chunking.  `mirrors` holds them against vvae_*_part_floats, vvae_ssim_loss_band_rows, vvae_ms_ssim_ws_floats and
vvae_plane_metrics_ws_bytes on both sides of every boundary used, and against every row of tests/golden/metrics_plans.json, so a
retuning fails there (and in the `expect` of the cases) instead of moving the cases into one band.  What the queries do not give
directly is pinned indirectly: strips from part_floats at H = 11 (one band), SW from the widths 10 + 2 SW and 11 + 2 SW, R from
vvae_ssim_loss_band_rows at a one-strip shape with the same H and the same number of (frame, strip) groups -- ssim_bands is one function.

All inputs are multiples of 1/16 in [0, 1], numbers of bf16, so the four dtype pairs see the same values.  A case is ONE clip whose
frames belong to families; one launch per dtype pair covers them all:

  D  dyadic errors: x, y random multiples of 1/16, |x - y| <= 1/2.  Every squared difference is a multiple of 1/256; the builder asserts
     256 x (every partial, every frame total) < 2^24, so any summation order is exact.  Zero tolerance on every `se` partial against the
     integer sum over the band's own rows and the strip's own columns (widened to 0 on the first strip and to W on the last), on mse
     against float(double(se) / n); psnr against the fp64 value at the spacing of the float result.  (Every frame of every family is held
     to these.)  Their `ss` partials are held too, with the general window bound below at km = 24.
  I  identical operands, y == x of family D.  vx, vy and vxy come from the same instruction sequence on the same numbers, so
     (2 vxy + C2) / (vx + vy + C2) == 1 bit for bit, and 2 ux uy + C1 differs from ux ux + uy uy + C1 by at most two spacings (a
     contraction of ux ux + uy uy): with the two products and the quotient S is 1 within 8 u, u = 2^-24.  Every partial is its count
     of owned positions within the bound; the builder asserts the bound below 1/8.
  Z  an all-zero pair: every moment is 0, numerator and denominator are the same two constants multiplied: S == 1 exactly, sums of ones
     below 2^24 are exact: every partial EQUALS its count, every term of the multi-scale form is exactly 1.
  P  probes on a zero background: x = 0, y = 0 but for probe pixels of value 1, at least 11 apart in both directions; every third probe
     is a pair probe (x = 1, y = 1/2 at the same pixel, so the x y plane is live); probe i sits in channel i % C.  The whole case also
     runs with the operands swapped.  Nothing cancels on a zero background: every moment is ONE product of two taps and a value.
     Positions: every row from 6 above to 5 below each band seam, every column from 6 left to 5 right of each strip seam, rows 0 .. 10
     and H - 11 .. H - 1, columns 0 .. 10 and W - 11 .. W - 1, the four corners.  The builder checks the table of a probe of 1 against
     the fp64 map: total deficit 62.98, centre 0.9997, outermost row 0.9468, corner 1.17e-3.
     Multi-scale: the probes are aligned 16 x 16 blocks of ones (one per frame; a pair probe adds x = 1 on the block's first 8 x 8), so
     every level sees one; plus single pixels in the odd
     trailing row and column, which only level 0 sees: every other level's term must stay exactly 1.
  M  masked frames, filled with NaN and 1e30: partials (0, 0), results 0; a read would poison the frame's own partial.

The reference is the fp64 SSIM map of the definition (test_metrics_host.ref_frame's arithmetic), summed over exactly the positions a
partial owns.  The 2 x 2 means of dyadic values are exact, so the reference pyramid is the kernel's bit for bit.

The bound of an `ss` partial (never read off the kernel):
  per window, from the fp64 moments ux, uy, h2 = g*x^2, h3 = g*y^2, h4 = g*xy.  Each moment is a sum of positive terms with a relative
  error of at most km u: km = 4 for a single probe pixel (two rounded taps, two products), km = 24 in general (two passes of 11 rounded
  taps, a product and an addition per tap).  Then |d vx| <= u (km h2 + (2 km + 1) ux^2 + vx), the same for vy and vxy;
  a2 = 2 vxy + C2 and b2 = vx + vy + C2 add one rounding and the rounding of the float constant each; cs = a2 / b2:
  |d cs| <= (|d a2| + |cs| |d b2|) / b2 + u |cs|; the luminance factor has the relative error
  (2 km + 2) u (2 |ux uy| / a1 + (ux^2 + uy^2) / b1) + 4 u; S = lum cs adds three roundings.  A window whose five moments are all 0
  gives exactly 1 (family Z) and has no error.  Families I and Z replace this by 8 u and 0 (above).
  summation: a thread adds at most n_t = 4 x (output rows of the band) values of at most 1 in sequence: at most u n_t (n_t + 1) / 2,
  over all threads u count (n_t + 1) / 2; every level of the wave butterfly and every step of the sum over the nw waves adds at most
  u x (the partial): u count (6 + nw).  The multi-scale form adds the ng threads of a channel in sequence instead: u count ng.
  fold: one more u x total per partial folded; the division is in double; the float result adds u.
  The whole is multiplied by 1.01 for the second-order terms.
The builder asserts every bound below half of the smallest defect the case claims to catch: one outermost row or column of a probe's
table (0.9468) for every case, one corner window (1.17e-3) for the small one-strip shapes 11 x 11 x 1 and 17 x 24 x 1, whose partials
hold few enough windows.  The fp32 CPU restatement (`twin_*`: the same definition in fp32 numpy, summed per partial) has to pass the very
assertions the GPU results meet; tests/test_host.py runs it (HOST_CHECKS) and feeds the assertions a restatement with one defect each
(DEFECT_CHECKS), which must raise in the assertion named.

The plane metrics form their moments in double and S in fp32 (two casts and a quotient): 4 u per live window, the same summation
terms; sse is exact.  The temporal error is held to zero tolerance throughout: d = (yc - yp) - (xc - xp) is a multiple of 1/16 with
|d| <= 1/8, every chunk and every pair total times 256 an integer below 2^24, tmse = float(s) * float(1 / n) in fp32.

Sentinel words stand in front of and behind `part` and every output of the entries called through lib(); they must be unchanged, and
no word of `part` or of an output may still hold the sentinel ("guards", "unwritten").
"""
import ctypes
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
BF16, F32 = torch.bfloat16, torch.float32
DT = {F32: 0, BF16: 1}
PAIRS = ((F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16))
PAIR_IDS = ["f32-f32", "f32-bf16", "bf16-f32", "bf16-bf16"]
SENT = 0x7FA5A5A5                          # a NaN no kernel computes
GUARD = 64                                 # words; keeps what follows 16-byte aligned
C1, C2 = 0.01 ** 2, 0.03 ** 2
ROW_DEFECT, CORNER_DEFECT = 0.9468, 1.17e-3
KM_PIXEL, KM_GENERAL = 4, 24
RATIOS = {}                                # route -> largest error / bound seen (printed by the tests, tabulated in NOTES.md)


class _Case(types.SimpleNamespace):
    pass


def _lib():
    from video_vae_amd._lib import lib
    return lib()


def _raises(fn, match):
    with pytest.raises(AssertionError, match=match):
        fn()


def _note(route, ratio):
    RATIOS[route] = max(RATIOS.get(route, 0.0), float(ratio))
    return float(ratio)


# =========================================================================================== the plans, mirrored
RM_MAX_THREADS, RM_MAX_ROW, RM_MIN_BAND, RM_TARGET_WGS, RM_MAX_WIDE_W = 512, 2048, 16, 1024, 8192
MS_MIN_BAND, MS_MAX_SCALES = 4, 5
PM_THREADS, PM_STRIP, PM_MIN_BAND, PM_TARGET_WGS, PM_CCHUNK = 256, 1012, 16, 2048, 16384
TM_CHUNK, TM_MAX_FRAME = 4096, 1 << 30


def rm_threads(w, c):
    need = max((w * c + 3) // 4, c * ((w + 3) // 4))
    return (need + 63) // 64 * 64


def ssim_bands(h, groups, target, min_band):
    n = max(1, min((target + groups - 1) // groups, (h + min_band - 1) // min_band))
    r = (h + n - 1) // n
    return r, (h + r - 1) // r


def ssim_rows(band, r, h):
    """(r0, r1, o0, o1): the band owns the rows [r0, r1) for the squared error and the output rows [o0, o1) (none when o0 >= o1)."""
    r0, r1 = band * r, min(band * r + r, h)
    return r0, r1, max(r0, 5), min(r1, h - 5)


def rm_plan(b, t, h, w, c, min_band=RM_MIN_BAND):
    if b <= 0 or t <= 0 or h < 11 or w < 11 or w > RM_MAX_WIDE_W or c < 1 or c > 4 or b * t > 65535:
        return None
    sw = w
    if w * c > RM_MAX_ROW or rm_threads(w, c) > RM_MAX_THREADS:
        sw = (RM_MAX_ROW // c - 10) // 4 * 4
        while c * ((sw + 10 + 3) // 4) > RM_MAX_THREADS:
            sw -= 4
    wmax = min(sw + 10, w)
    strips = (w - 10 + sw - 1) // sw
    r, bands = ssim_bands(h, b * t * strips, RM_TARGET_WGS, min_band)
    return _Case(H=h, W=w, C=c, SW=sw, strips=strips, R=r, bands=bands, threads=rm_threads(wmax, c), P=(wmax + 3) // 4 * 4 + 16)


def strip_cols(p, s):
    """(c0, c1, m0, m1, ws): strip s owns the SSIM columns [c0, c1) and the squared-error columns [m0, m1); it spans ws columns."""
    c0, c1 = 5 + s * p.SW, min(5 + (s + 1) * p.SW, p.W - 5)
    ws = min(s * p.SW + p.SW + 10, p.W) - s * p.SW
    return c0, c1, (0 if s == 0 else c0), (p.W if s == p.strips - 1 else c1), ws


def ms_plan(b, t, h, w, c, m):
    if (b <= 0 or t <= 0 or b * t > 65535 or c < 1 or c > 4 or m < 1 or m > MS_MAX_SCALES or h < 11 or w < 11 or w > RM_MAX_WIDE_W
            or (min(h, w) >> (m - 1)) < 11):
        return None
    f, off, lv = b * t, 0, []
    for j in range(m):
        p = rm_plan(b, t, h >> j, w >> j, c, MS_MIN_BAND)
        if p is None or 2 * p.threads > 5 * c * p.P + 16:
            return None
        if j:
            off += 2 * ((f * p.H * p.W * c + 3) // 4 * 4)
        lv.append(p)
    for p in lv:
        off += (f * p.strips * p.bands * c * 2 + 3) // 4 * 4
    return _Case(levels=lv, total=off)


def pm_plan(n, h, w, chroma):
    """chroma: 0 = 4:2:0, 1 = 4:4:4, 2 = mono"""
    if n < 1 or not 11 <= h <= 8192 or not 11 <= w <= 8192 or not 0 <= chroma <= 2:
        return None
    strips = (w - 10 + PM_STRIP - 1) // PM_STRIP
    sw = ((w - 10 + strips - 1) // strips + 3) // 4 * 4
    strips = (w - 10 + sw - 1) // sw
    r, bands = ssim_bands(h, n * strips, PM_TARGET_WGS, PM_MIN_BAND)
    threads = ((min(sw + 10, w) + 3) // 4 + 63) // 64 * 64
    cplane = ((h + 1) // 2) * ((w + 1) // 2) if chroma == 0 else h * w if chroma == 1 else 0
    chunks = (cplane + PM_CCHUNK - 1) // PM_CCHUNK
    if threads > PM_THREADS:
        return None
    return _Case(H=h, W=w, C=1, SW=sw, strips=strips, R=r, bands=bands, threads=threads, chunks=chunks,
                 ws_bytes=n * strips * bands * 16 + n * 2 * chunks * 8)


def tm_chunks(n):
    return (n + TM_CHUNK - 1) // TM_CHUNK


def tm_part_floats(b, t, h, w, c):
    if b <= 0 or t < 2 or h <= 0 or w <= 0 or not 1 <= c <= 4 or h * w * c > TM_MAX_FRAME:
        return 0
    return b * (t - 1) * tm_chunks(h * w * c)


def pool_vec(w, c, ex, ey):
    """Does the pool of a level of rows of w pixels run its 16-byte form (operands and pyramid 16-byte aligned, as they are here)?"""
    return (w * c * ex) % 16 == 0 and (w * c * ey) % 16 == 0 and ((w // 2) * c) % 4 == 0


def _golden_row(c, h, w, b, t):
    p = rm_plan(b, t, h, w, c)
    one = rm_plan(1, 1, h, w, c)
    row = [int(one is not None and one.strips == 1), b * t * p.bands * 2 if p is not None and p.strips == 1 else 0,
           int(one is not None), b * t * p.strips * p.bands * 2 if p is not None else 0]
    row += [int(ms_plan(1, 1, h, w, c, m) is not None) for m in range(1, 6)]
    row += [getattr(ms_plan(b, t, h, w, c, m), "total", 0) for m in range(1, 6)]
    pm = pm_plan(b * t, h, w, c % 3)
    return row + [int(pm_plan(1, h, w, c % 3) is not None), pm.ws_bytes if pm is not None else 0, tm_part_floats(b, t, h, w, c)]


def _mirrors_match_the_library():
    """The mirrors against the recorded plans, and against the library on both sides of every boundary the cases use."""
    lb = _lib()
    with open(os.path.join(ROOT, "tests", "golden", "metrics_plans.json")) as fh:
        want = json.load(fh)
    assert want["columns"][:5] == ["C", "H", "W", "B", "T"] and len(want["rows"]) >= 200
    for r in want["rows"]:
        assert _golden_row(*r[:5]) == r[5:], ("golden row", r[:5], _golden_row(*r[:5]), r[5:])

    def part(b, t, h, w, c):
        p = rm_plan(b, t, h, w, c)
        wide = b * t * p.strips * p.bands * 2 if p is not None else 0
        assert lb.vvae_recon_metrics_wide_part_floats(b, t, h, w, c) == wide, ("wide part_floats", b, t, h, w, c, wide)
        narrow = wide if p is not None and p.strips == 1 else 0
        assert lb.vvae_recon_metrics_part_floats(b, t, h, w, c) == narrow, ("part_floats", b, t, h, w, c, narrow)
        return p

    # strips and SW: one band at H = 11, so part_floats / 2 is the number of strips
    for c, sw, limit in ((1, 2036, 2048), (2, 1012, 1024), (3, 668, 680), (4, 500, 512)):
        assert part(1, 1, 11, limit, c).strips == 1 and part(1, 1, 12, limit, c).SW == limit
        p = part(1, 1, 11, limit + 1, c)
        assert (p.strips, p.SW) == (2, sw), (c, p)
        assert part(1, 1, 11, 10 + 2 * sw, c).strips == 2 and part(1, 1, 11, 11 + 2 * sw, c).strips == 3
        assert part(1, 1, 11, 10 + 3 * sw, c).strips == 3 and part(1, 1, 11, 11 + 3 * sw, c).strips == 4
    assert part(1, 1, 11, 682, 3).SW == 668 and 682 * 3 <= RM_MAX_ROW and rm_threads(681, 3) > RM_MAX_THREADS >= rm_threads(680, 3)
    for w in (10, 11, 8192, 8193):
        part(1, 1, 11, w, 1), part(1, 1, w, 11, 1)
    # R and bands: vvae_ssim_loss_band_rows is ssim_bands' R at a one-strip shape; groups = frames x strips
    for h in (11, 12, 16, 17, 32, 33, 37, 48, 49, 64, 65, 176, 720):
        for f in (1, 2, 15, 16, 21, 22, 63, 64, 65, 256, 341, 342, 511, 512, 513, 1023, 1024, 1025, 4096, 65535):
            p = part(1, f, h, 24, 2)
            assert lb.vvae_ssim_loss_band_rows(1, f, h, 24, 2) == p.R, ("band rows", h, f, p.R)
            assert part(f, 1, h, 24, 2).bands == p.bands == -(-h // p.R)
    assert lb.vvae_ssim_loss_band_rows(1, 1, 37, 2049, 1) == 0 and part(1, 65536, 16, 16, 1) is None
    for f, strips in ((1, 2), (171, 2), (172, 2), (7, 3), (114, 3)):             # wide shapes: the same bands as frames x strips groups
        w = 2049 if strips == 2 else 11 + 2 * 2036
        p = part(1, f, 37, w, 1)
        assert p.strips == strips and p.R == lb.vvae_ssim_loss_band_rows(1, f * strips, 37, 24, 1), (f, strips, p)
    # the multi-scale plan: one level gives frames x strips x bands x C x 2 words at bands of at least 4 rows
    for h, w, c, f in ((176, 176, 1, 12), (179, 181, 3, 12), (22, 2049, 1, 9), (24, 26, 4, 9), (11, 11, 1, 300), (22, 22, 2, 1200), (89, 90, 3, 5)):
        for m in range(1, 6):
            mp = ms_plan(1, f, h, w, c, m)
            assert lb.vvae_ms_ssim_ws_floats(1, f, h, w, c, m) == (mp.total if mp else 0), ("ms ws", h, w, c, f, m)
            assert bool(lb.vvae_ms_ssim_supported(h, w, c, m, 0, 1)) == (ms_plan(1, 1, h, w, c, m) is not None)
        p = rm_plan(1, f, h, w, c, MS_MIN_BAND)
        assert lb.vvae_ms_ssim_ws_floats(1, f, h, w, c, 1) == (f * p.strips * p.bands * c * 2 + 3) // 4 * 4
    # the plane metrics: mono has no chroma partials, so ws_bytes / 16 is frames x strips x bands
    for w, strips, sw in ((1022, 1, 1012), (1023, 2, 508), (2034, 2, 1012), (2035, 3, 676), (17, 1, 8), (71, 1, 64)):
        for h, n in ((11, 1), (13, 1), (33, 3), (37, 1), (37, 40), (37, 700), (64, 2000)):
            p = pm_plan(n, h, w, 2)
            assert (p.strips, p.SW) == (strips, sw), (w, p)
            assert lb.vvae_plane_metrics_ws_bytes(n, h, w, 2) == p.ws_bytes == n * strips * p.bands * 16, ("pm ws", n, h, w)
            assert lb.vvae_plane_metrics_ws_bytes(n, h, w, 0) == pm_plan(n, h, w, 0).ws_bytes
    assert pm_plan(1, 11, 1023, 2).bands == 1 and pm_plan(1, 10, 64, 2) is None and lb.vvae_plane_metrics_ws_bytes(1, 10, 64, 2) == 0
    # the temporal chunks
    for n, chunks in ((4096, 1), (4097, 2), (4100, 2), (3 * 4096 + 8, 4), (64 * 4096, 64), (64 * 4096 + 4, 65), (129 * 4096 + 4, 130)):
        assert tm_chunks(n) == chunks and lb.vvae_temporal_mse_part_floats(2, 3, 1, n, 1) == 4 * chunks, n
        if n % 4 == 0:
            assert lb.vvae_temporal_mse_part_floats(2, 3, 1, n // 4, 4) == 4 * chunks
    assert lb.vvae_temporal_mse_part_floats(2, 1, 4, 4, 1) == 0 == tm_part_floats(2, 1, 4, 4, 1)


# =========================================================================================== the definition in fp64, its restatement in fp32
def _taps():
    k = np.arange(11, dtype=np.float64) - 5
    g = np.exp(-k * k / (2 * 1.5 ** 2))
    return g / g.sum()


G64 = _taps()
G32 = G64.astype(np.float32)


def _filt(a, g):
    """(F, H, W, C) -> (F, H - 10, W - 10, C): the 11 taps down, then across, accumulated in order in a's precision"""
    h, w = a.shape[1], a.shape[2]
    r = np.zeros((a.shape[0], h - 10, w, a.shape[3]), a.dtype)
    for k in range(11):
        r = r + g[k] * a[:, k:h - 10 + k]
    o = np.zeros((a.shape[0], h - 10, w - 10, a.shape[3]), a.dtype)
    for k in range(11):
        o = o + g[k] * r[:, :, k:w - 10 + k]
    return o


def moments(x, y, dtype=np.float64):
    g = G64 if dtype == np.float64 else G32
    x, y = x.astype(dtype), y.astype(dtype)
    return _filt(x, g), _filt(y, g), _filt(x * x, g), _filt(y * y, g), _filt(x * y, g)


def maps(mo):
    """(S, CS) of the moments, in their precision"""
    ux, uy, h2, h3, h4 = mo
    dt = ux.dtype.type
    c1, c2, two = dt(np.float32(1e-4)) if dt == np.float32 else dt(C1), dt(np.float32(9e-4)) if dt == np.float32 else dt(C2), dt(2)
    vx, vy, vxy = h2 - ux * ux, h3 - uy * uy, h4 - ux * uy
    a1, a2, b1, b2 = two * ux * uy + c1, two * vxy + c2, ux * ux + uy * uy + c1, vx + vy + c2
    return (a1 * a2) / (b1 * b2), a2 / b2


def window_eps(mo, km):
    """(|dS|, |dCS|) per window, the module docstring's derivation; 0 where the five moments are all 0"""
    ux, uy, h2, h3, h4 = mo
    vx, vy, vxy = h2 - ux * ux, h3 - uy * uy, h4 - ux * uy
    a1, a2, b1, b2 = 2 * ux * uy + C1, 2 * vxy + C2, ux * ux + uy * uy + C1, vx + vy + C2
    dvx = U * (km * h2 + (2 * km + 1) * ux * ux + np.abs(vx))
    dvy = U * (km * h3 + (2 * km + 1) * uy * uy + np.abs(vy))
    dvxy = U * (km * np.abs(h4) + (2 * km + 1) * np.abs(ux * uy) + np.abs(vxy))
    da2 = 2 * dvxy + U * (np.abs(a2) + C2)
    db2 = dvx + dvy + U * (2 * np.abs(b2) + C2)
    cs, lum = a2 / b2, a1 / b1
    dcs = (da2 + np.abs(cs) * db2) / b2 + U * np.abs(cs)
    rlum = (2 * km + 2) * U * (2 * np.abs(ux * uy) / a1 + (ux * ux + uy * uy) / b1) + 4 * U
    ds = np.abs(lum) * dcs + np.abs(lum * cs) * (rlum + 3 * U)
    dead = (ux == 0) & (uy == 0) & (h2 == 0) & (h3 == 0)
    return np.where(dead, 0.0, 1.01 * ds), np.where(dead, 0.0, 1.01 * dcs)


@functools.lru_cache(maxsize=None)
def probe_table():
    """The deficits 1 - S of a probe of 1 on a zero background (fp64), 11 x 11 -- and what the issue states of them."""
    x, y = np.zeros((1, 21, 21, 1)), np.zeros((1, 21, 21, 1))
    y[0, 10, 10, 0] = 1.0
    d = 1.0 - maps(moments(x, y))[0][0, :, :, 0]
    assert d.shape == (11, 11) and abs(d.sum() - 62.98) < 5e-3 and abs(d[5, 5] - 0.9997) < 5e-5
    assert abs(d[0].sum() - ROW_DEFECT) < 5e-5 and abs(d[:, 10].sum() - ROW_DEFECT) < 5e-5 and abs(d[0, 0] - CORNER_DEFECT) < 5e-6
    assert d[0].sum() >= ROW_DEFECT - 5e-5 and d.min() == d[0, 0]
    return d


# =========================================================================================== inputs
def _rng(*key):
    import zlib
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def probe_sites(h, w, row_seams, col_seams):
    rows = sorted({r for r in list(range(11)) + list(range(h - 11, h)) + [r for s in row_seams for r in range(s - 6, s + 6)] if 0 <= r < h})
    cols = sorted({c for c in list(range(11)) + list(range(w - 11, w)) + [c for s in col_seams for c in range(s - 6, s + 6)] if 0 <= c < w})
    sites = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    sites += [(rows[i % len(rows)], cols[(i * 7) % len(cols)] if len(cols) > len(rows) else cols[i % len(cols)]) for i in range(len(rows))]
    sites += [(rows[(i * 5) % len(rows)], cols[i]) for i in range(len(cols))]
    sites = list(dict.fromkeys(sites))
    assert {r for r, _ in sites} == set(rows) and {c for _, c in sites} == set(cols)
    return sites, rows, cols


def pack_frames(sites):
    """Greedily into frames: the probes of a frame at least 11 apart in BOTH directions, so no window sees two"""
    frames = []
    for s in sites:
        for fr in frames:
            if all(abs(s[0] - q[0]) >= 11 and abs(s[1] - q[1]) >= 11 for q in fr):
                fr.append(s)
                break
        else:
            frames.append([s])
    return frames


def dyadic_pair(shape, key):
    """x, y in sixteenths (integers 0 .. 16), |x - y| <= 8"""
    g = _rng(*key)
    x = g.integers(0, 17, shape)
    return x, np.clip(x + g.integers(-8, 9, shape), 0, 16)


def build_clip(name, h, w, c, plan_of, col_seams_of, reps=1, swap=False):
    """The frames of a case (module docstring): fam (F,), xi, yi (F, H, W, C) in sixteenths, mask (F,).  The plan depends on the number
    of frames and the probe frames on the plan's seams: iterate to the fixed point."""
    f = 12
    for _ in range(4):
        p = plan_of(f * reps)
        sites, rows, cols = probe_sites(h, w, [k * p.R for k in range(1, p.bands)], col_seams_of(p))
        pf = pack_frames(sites)
        nf = 2 + 2 + 1 + len(pf) + 2
        if nf == f:
            break
        f = nf
    else:
        raise AssertionError(f"{name}: the plan does not settle")
    fam = ["D", "M", "I", "P"] + ["P"] * (len(pf) - 1) + ["M", "Z", "I", "D"]
    assert len(fam) == f
    xi, yi = np.zeros((f, h, w, c), np.int64), np.zeros((f, h, w, c), np.int64)
    probes, k, ip = [], 0, 0
    for i, fm in enumerate(fam):
        if fm == "D":
            xi[i], yi[i] = dyadic_pair((h, w, c), (name, i))
        elif fm == "I":
            xi[i] = yi[i] = dyadic_pair((h, w, c), (name, i))[0]
        elif fm == "P":
            for (r, q) in pf[ip]:
                ch = k % c
                if k % 3 == 1:
                    xi[i, r, q, ch], yi[i, r, q, ch] = 16, 8
                else:
                    yi[i, r, q, ch] = 16
                probes.append((i, r, q, ch))
                k += 1
            ip += 1
    if swap:
        xi, yi = yi, xi
    fam = np.array(fam * reps)
    return _Case(name=name, H=h, W=w, C=c, F=f * reps, reps=reps, fam=fam, xi=xi, yi=yi, mask=(fam != "M").astype(np.float32), plan=p,
                 probes=probes, rows=rows, cols=cols, swap=swap)


def clip_tensors(case, dtx, dty, offx=0, offy=0):
    """CPU tensors (F, H, W, C) of the two dtypes, the masked frames poisoned; off: the tensor starts that many elements into its buffer"""
    out = []
    for v, dt, off, bad in ((case.xi, dtx, offx, float("nan")), (case.yi, dty, offy, 1e30)):
        t = torch.from_numpy(np.tile(v, (case.reps, 1, 1, 1)) / 16.0).to(torch.float32)
        t[torch.from_numpy(case.fam == "M")] = bad
        t = t.to(dt)
        buf = torch.zeros(t.numel() + off + 8, dtype=dt)
        buf[off:off + t.numel()] = t.reshape(-1)
        out.append((buf, off))
    return out


# =========================================================================================== single scale: expectation, assertion, restatement
def _sum_depth(n_t, nw):
    return (n_t + 1) / 2 + 6 + nw


def expect_rm(case):
    """What every (frame, strip, band) must give: se256 int, ss fp64, its bound and count, per frame of the base clip"""
    if getattr(case, "exp", None) is not None:
        return case.exp
    p, f0 = case.plan, case.xi.shape[0]
    x, y = case.xi / 16.0, case.yi / 16.0
    mo = moments(x, y)
    smap = maps(mo)[0]
    single = np.array([(case.xi[i] != 0).sum() + (case.yi[i] != 0).sum() for i in range(f0)])
    eps = np.zeros_like(smap)
    for i in range(f0):
        fm = case.fam[i]
        if fm == "D":
            eps[i] = window_eps([m[i:i + 1] for m in mo], KM_GENERAL)[0][0]
        elif fm == "P":
            eps[i] = window_eps([m[i:i + 1] for m in mo], KM_PIXEL)[0][0]
        elif fm == "I":
            assert np.array_equal(case.xi[i], case.yi[i])
            eps[i] = 8 * U
        else:
            assert single[i] == 0
    d2 = (case.xi - case.yi) ** 2
    shape = (f0, p.strips, p.bands)
    e = _Case(se=np.zeros(shape, np.int64), ss=np.zeros(shape), bound=np.zeros(shape), count=np.zeros(shape, np.int64))
    for s in range(p.strips):
        c0, c1, m0, m1, _ = strip_cols(p, s)
        for b in range(p.bands):
            r0, r1, o0, o1 = ssim_rows(b, p.R, p.H)
            e.se[:, s, b] = d2[:, r0:r1, m0:m1].sum(axis=(1, 2, 3))
            if o0 < o1:
                cnt = (o1 - o0) * (c1 - c0) * p.C
                e.count[:, s, b] = cnt
                e.ss[:, s, b] = smap[:, o0 - 5:o1 - 5, c0 - 5:c1 - 5].sum(axis=(1, 2, 3))
                e.bound[:, s, b] = 1.01 * (eps[:, o0 - 5:o1 - 5, c0 - 5:c1 - 5].sum(axis=(1, 2, 3)) + U * cnt * _sum_depth(4 * (o1 - o0), p.threads // 64))
    live = case.fam[:f0] != "M"
    e.se[~live], e.ss[~live], e.bound[~live], e.count[~live] = 0, 0, 0, 0
    e.bound[case.fam[:f0] == "Z"] = 0
    assert e.se.max() < 2 ** 24 and e.se.sum(axis=(1, 2)).max() < 2 ** 24, "family D leaves the exact range of fp32"
    n, nv, nsb = p.H * p.W * p.C, (p.H - 10) * (p.W - 10) * p.C, p.strips * p.bands
    assert e.count.sum(axis=(1, 2))[live].min() == nv and np.all(d2.sum(axis=(1, 2, 3))[live] == e.se.sum(axis=(1, 2))[live])
    m = e.se.sum(axis=(1, 2)) / 256.0 / n
    e.mse = np.where(live, m, 0).astype(np.float32)
    e.psnr = np.where(live, 10.0 * np.log10(1.0 / np.maximum(m, 1e-10)), 0.0)
    e.ssim = np.where(live, e.ss.sum(axis=(1, 2)) / nv, 0.0)
    e.ssim_bound = np.where(case.fam[:f0] == "Z", 0.0, (e.bound.sum(axis=(1, 2)) + 1.01 * U * (nsb + 1) / 2 * nv) / nv + U)
    # the claims: every bound below half of an outermost row of a probe's table; the small shapes resolve one corner window
    claim = np.isin(case.fam[:f0], ("P", "I"))
    assert e.bound[claim].max() < ROW_DEFECT / 2 and e.bound[case.fam[:f0] == "I"].max() < 1 / 8, (case.name, e.bound[claim].max())
    case.corner = bool(e.bound[case.fam[:f0] == "P"].max() < CORNER_DEFECT / 2)
    probe_table()
    case.exp = e
    return e


def _tile(a, reps):
    return np.tile(a, (reps,) + (1,) * (a.ndim - 1))


def check_rm(case, res, what):
    """res: part (F, strips, bands, 2) fp32, mse, psnr, ssim (F,) fp32, guards, unwritten (counts) -> largest ss error / bound"""
    e, reps = expect_rm(case), case.reps
    assert res.guards == 0, f"{what}: guards: {res.guards} sentinel words around part and the outputs changed"
    assert res.unwritten == 0, f"{what}: unwritten: {res.unwritten} words of part or of an output still hold the sentinel"
    dead = case.fam == "M"
    for name, v in (("part", res.part), ("mse", res.mse), ("psnr", res.psnr), ("ssim", res.ssim)):
        assert np.all(v[dead] == 0), f"{what}: masked: {name} of a masked frame is not 0: {v[dead].reshape(-1)[:4]}"
    se = res.part[..., 0].astype(np.float64) * 256.0
    bad = se != _tile(e.se, reps)
    assert not bad.any(), (f"{what}: se partials: {int(bad.sum())} differ from the integer sums; first (frame, strip, band) "
                           f"{tuple(np.argwhere(bad)[0])}: got {se[bad][0]} want {_tile(e.se, reps)[bad][0]} (x 1/256)")
    err, bound = np.abs(res.part[..., 1].astype(np.float64) - _tile(e.ss, reps)), _tile(e.bound, reps)
    bad = ~(err <= bound)
    assert not bad.any(), (f"{what}: ss partials: {int(bad.sum())} outside their bound; first (frame, strip, band) {tuple(np.argwhere(bad)[0])} "
                           f"(family {case.fam[np.argwhere(bad)[0][0]]}): got {res.part[..., 1][bad][0]!r} want {_tile(e.ss, reps)[bad][0]!r} "
                           f"bound {bound[bad][0]:.3e}")
    bad = res.mse != _tile(e.mse, reps)
    assert not bad.any(), f"{what}: mse: frames {np.argwhere(bad).reshape(-1)[:8]} differ: got {res.mse[bad][:4]} want {_tile(e.mse, reps)[bad][:4]}"
    want = _tile(e.psnr, reps)
    bad = ~(np.abs(res.psnr.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32)))
    assert not bad.any(), f"{what}: psnr: frames {np.argwhere(bad).reshape(-1)[:8]}: got {res.psnr[bad][:4]} want {want[bad][:4]}"
    bad = ~(np.abs(res.ssim.astype(np.float64) - _tile(e.ssim, reps)) <= _tile(e.ssim_bound, reps))
    assert not bad.any(), f"{what}: ssim: frames {np.argwhere(bad).reshape(-1)[:8]}: got {res.ssim[bad][:4]} want {_tile(e.ssim, reps)[bad][:4]}"
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def twin_rm(case, defect=None):
    """The definition in fp32 numpy, summed per partial in fp32 (module docstring); `defect`: one of DEFECTS_RM"""
    p, f0 = case.plan, case.xi.shape[0]
    x, y = (case.xi / 16.0).astype(np.float32), (case.yi / 16.0).astype(np.float32)
    smap = maps(moments(x, y, np.float32))[0]
    if defect == "halo row one off":                     # the first output row of every band but the first filters the rows one further down
        shifted = maps(moments(np.roll(x, -1, axis=1), np.roll(y, -1, axis=1), np.float32))[0]
        for b in range(1, p.bands):
            o0 = ssim_rows(b, p.R, p.H)[2]
            smap[:, o0 - 5] = shifted[:, o0 - 5]
    d2 = ((case.xi - case.yi) ** 2).astype(np.float32) / np.float32(256)
    part = np.zeros((f0, p.strips, p.bands, 2), np.float32)
    for s in range(p.strips):
        c0, c1, m0, m1, _ = strip_cols(p, s)
        if defect == "mse columns from 5" and s == 0:
            m0 = 5
        if defect == "window doubled at a strip seam" and s > 0:
            c0 -= 1
        for b in range(p.bands):
            r0, r1, o0, o1 = ssim_rows(b, p.R, p.H)
            if defect == "window dropped at a band seam" and b > 0:
                o0 += 1
            part[:, s, b, 0] = d2[:, r0:r1, m0:m1].sum(axis=(1, 2, 3), dtype=np.float32)
            if o0 < o1:
                blk = smap[:, o0 - 5:o1 - 5, c0 - 5:c1 - 5]
                part[:, s, b, 1] = blk.sum(axis=(1, 2, 3), dtype=np.float32)
                if defect == "window dropped at a band seam" and b > 0:       # one window, not the row: the first of the row
                    part[:, s, b, 1] += smap[:, o0 - 6, c0 - 4:c1 - 5].sum(axis=(1, 2), dtype=np.float32)
    live = case.fam[:f0] != "M"
    part[~live] = 0
    n, nv = p.H * p.W * p.C, (p.H - 10) * (p.W - 10) * p.C
    se, ss = part[..., 0].sum(axis=(1, 2), dtype=np.float32), part[..., 1].sum(axis=(1, 2), dtype=np.float32)
    m = se.astype(np.float64) / n
    res = _Case(part=part, mse=np.where(live, m, 0).astype(np.float32),
                psnr=np.where(live, 10.0 * np.log10(1.0 / np.maximum(m, 1e-10)), 0).astype(np.float32),
                ssim=np.where(live, ss.astype(np.float64) / nv, 0).astype(np.float32), guards=0, unwritten=0)
    if defect == "guard word written":
        res.guards = 1
    if defect == "partial never written":
        res.unwritten = 1
    if defect == "masked frame read":
        res.part[np.argmax(~live), 0, 0, 1] = np.float32(1.0)
    for k in ("part", "mse", "psnr", "ssim"):
        setattr(res, k, _tile(getattr(res, k), case.reps))
    return res


# name -> (entry, H, W, C, reps, what the plan must be)
RM_CASES = {
    "11x11x1": ("narrow", 11, 11, 1, 1, dict(strips=1, bands=1, R=11)),
    "17x24x1": ("narrow", 17, 24, 1, 1, dict(strips=1, bands=2, R=9)),
    "37x53x3": ("narrow", 37, 53, 3, 1, dict(strips=1, bands=3, R=13)),
    "37x52x4": ("narrow", 37, 52, 4, 1, dict(strips=1, bands=3, R=13)),
    "48x40x2": ("narrow", 48, 40, 2, 64, dict(strips=1, bands=1, R=48)),
    "12x2048x1": ("narrow", 12, 2048, 1, 1, dict(strips=1, bands=1, SW=2048, threads=512)),
    "12x680x3": ("narrow", 12, 680, 3, 1, dict(strips=1, bands=1, SW=680, threads=512)),
    "12x512x4": ("narrow", 12, 512, 4, 1, dict(strips=1, bands=1, SW=512, threads=512)),
    "37x2049x1": ("wide", 37, 2049, 1, 1, dict(strips=2, SW=2036, bands=3, R=13)),
    "37x681x3": ("wide", 37, 681, 3, 1, dict(strips=2, SW=668, bands=3, R=13)),
    "37x682x3": ("wide", 37, 682, 3, 1, dict(strips=2, SW=668, bands=3, R=13)),
    "37x513x4": ("wide", 37, 513, 4, 1, dict(strips=2, SW=500, bands=3, R=13)),
    "37x1011x4": ("wide", 37, 1011, 4, 1, dict(strips=3, SW=500, bands=3, R=13)),
    "37x1025x2": ("wide", 37, 1025, 2, 1, dict(strips=2, SW=1012, bands=3, R=13)),
}
RM_CORNER = ("11x11x1", "17x24x1")        # the shapes whose bounds resolve one corner window


@functools.lru_cache(maxsize=None)
def rm_case(name, swap=False):
    entry, h, w, c, reps, want = RM_CASES[name]
    case = build_clip(name, h, w, c, lambda f: rm_plan(1, f, h, w, c), lambda p: [5 + k * p.SW for k in range(1, p.strips)], reps, swap)
    case.entry = entry
    p = case.plan
    got = {k: getattr(p, k) for k in want}
    assert got == want, f"{name}: regime: the plan is {got}, the case was built for {want}"
    assert (p.strips == 1) == (entry == "narrow")
    e = expect_rm(case)
    if name == "37x2049x1":
        assert strip_cols(p, 1)[:2] == (2041, 2044)                              # the second strip owns 3 SSIM columns
    if name == "37x1011x4":
        assert strip_cols(p, 1)[2:4] == strip_cols(p, 1)[:2] == (505, 1005)      # the middle strip: a halo on both sides, no MSE edge
    if name == "17x24x1":
        assert ssim_rows(1, p.R, p.H)[2:] == (9, 12)                             # the second band owns three output rows
    if name == "48x40x2":
        assert case.F >= 1024 and (48 + 10 - 1) // 11 == 5                       # four passes of the unrolled loop and a ragged one
    if name in RM_CORNER:
        assert case.corner, f"{name}: the bound {e.bound.max():.3e} does not resolve one corner window"
    return case


def gpu_rm(case, dev, dtx, dty, entry=None, offx=0, offy=0):
    """vvae_recon_metrics[_wide]_fwd on the case with guarded buffers -> the result check_rm takes"""
    lb, p, f = _lib(), case.plan, case.F
    name = "vvae_recon_metrics_fwd" if (entry or case.entry) == "narrow" else "vvae_recon_metrics_wide_fwd"
    (xb, ox), (yb, oy) = clip_tensors(case, dtx, dty, offx, offy)
    xb, yb = xb.to(dev), yb.to(dev)
    npart = f * p.strips * p.bands * 2
    query = lb.vvae_recon_metrics_part_floats if name == "vvae_recon_metrics_fwd" else lb.vvae_recon_metrics_wide_part_floats
    assert query(1, f, p.H, p.W, p.C) == npart
    buf = torch.full((GUARD + npart + GUARD + 3 * (f + GUARD),), SENT, dtype=torch.int32, device=dev)
    mask = torch.from_numpy(case.mask).to(dev)
    at = lambda words: ctypes.c_void_p(buf.data_ptr() + 4 * words)
    o = GUARD + npart + GUARD
    rc = getattr(lb, name)(ctypes.c_void_p(xb.data_ptr() + ox * xb.element_size()), DT[dtx], ctypes.c_void_p(yb.data_ptr() + oy * yb.element_size()),
                           DT[dty], ctypes.c_void_p(mask.data_ptr()), at(o), at(o + f + GUARD), at(o + 2 * (f + GUARD)), at(GUARD),
                           1, f, p.H, p.W, p.C, 1, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    w = buf.cpu().numpy()
    own = np.zeros(w.shape, bool)
    own[GUARD:GUARD + npart] = True
    for k in range(3):
        own[o + k * (f + GUARD):o + k * (f + GUARD) + f] = True
    fl = w.view(np.float32)
    return _Case(part=fl[GUARD:GUARD + npart].reshape(f, p.strips, p.bands, 2).copy(), mse=fl[o:o + f].copy(),
                 psnr=fl[o + f + GUARD:o + 2 * f + GUARD].copy(), ssim=fl[o + 2 * (f + GUARD):o + 2 * (f + GUARD) + f].copy(),
                 guards=int((w[~own] != SENT).sum()), unwritten=int((w[own] == SENT).sum()))


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("name", list(RM_CASES))
def test_single_scale_partials(dev, name, pair):
    """Every (se, ss) partial, mse, psnr and ssim of every family, in the four dtype pairs; the probes also with the operands swapped"""
    case = rm_case(name)
    r = _note(f"single scale, {case.entry}", check_rm(case, gpu_rm(case, dev, *pair), name))
    if pair[0] == pair[1]:
        sw = rm_case(name, True)
        r = max(r, _note(f"single scale, {case.entry}", check_rm(sw, gpu_rm(sw, dev, *pair), name + " swapped")))
    print(f"{name} {pair}: largest ss error / bound {r:.4f}, corner resolved: {case.corner}")


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("name", ["37x52x4", "17x24x1"])
def test_single_scale_operand_off_its_16_bytes(dev, name, pair):
    """An operand one element into its buffer: the scalar loads, the same values, bit for bit the aligned call's partials"""
    case = rm_case(name)
    base = gpu_rm(case, dev, *pair)
    for offx, offy in ((1, 0), (0, 1), (3, 2)):
        res = gpu_rm(case, dev, *pair, offx=offx, offy=offy)
        check_rm(case, res, f"{name} off {offx},{offy}")
        assert np.array_equal(res.part.view(np.int32), base.part.view(np.int32)), f"{name}: the scalar loads give other partials"


@pytest.mark.parametrize("name", [n for n, v in RM_CASES.items() if v[0] == "narrow"])
def test_wide_entry_gives_the_narrow_entry_partials(dev, name):
    case = rm_case(name)
    for pair in (PAIRS[0], PAIRS[3]):
        a, b = gpu_rm(case, dev, *pair, entry="narrow"), gpu_rm(case, dev, *pair, entry="wide")
        check_rm(case, b, name + " through the wide entry")
        for k in ("part", "mse", "psnr", "ssim"):
            assert np.array_equal(getattr(a, k).view(np.int32), getattr(b, k).view(np.int32)), f"{name}: {k} differs between the entries"


# =========================================================================================== multi-scale
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
# name -> (H, W, C, scales)
MS_CASES = {"176x176x1": (176, 176, 1, 5), "176x176x3": (176, 176, 3, 5), "179x181x1": (179, 181, 1, 5), "179x181x3": (179, 181, 3, 5),
            "22x2049x1": (22, 2049, 1, 2), "24x26x4": (24, 26, 4, 2)}


def pool(v):
    ho, wo = v.shape[1] // 2, v.shape[2] // 2
    v = v[:, :2 * ho, :2 * wo]
    return ((v[:, 0::2, 0::2] + v[:, 0::2, 1::2]) + (v[:, 1::2, 0::2] + v[:, 1::2, 1::2])) * 0.25


@functools.lru_cache(maxsize=None)
def ms_case(name):
    h, w, c, m = MS_CASES[name]
    blocks = [(r, q) for r in sorted({0, (h - 16) // 16 * 16, (h // 32) * 16}) for q in sorted({0, (w - 16) // 16 * 16, (w // 32) * 16})]
    if w > 2000:
        blocks += [(0, 2032), (0, 1024)]                     # across the strip seam of level 0 (SSIM column 2041), and mid-row
    if h == 24:
        blocks = [(0, 0), (8, 10)]
    pixels = [(h - 1, w // 2), (h // 2, w - 1)] if h % 2 and w % 2 else []
    fam = ["D", "I", "M"] + ["P"] * len(blocks) + ["T"] * len(pixels) + ["Z", "M", "I"]
    f = len(fam)
    xi, yi = np.zeros((f, h, w, c), np.int64), np.zeros((f, h, w, c), np.int64)
    k = 0
    for i, fm in enumerate(fam):
        if fm == "D":
            xi[i], yi[i] = dyadic_pair((h, w, c), (name, i))
        elif fm == "I":
            xi[i] = yi[i] = dyadic_pair((h, w, c), (name, i))[0]
        elif fm == "P":
            r, q = blocks[k]
            yi[i, r:r + 16, q:q + 16, k % c] = 16
            if k % 3 == 1:                                   # a pair probe: x = 1 on the block's first 8 x 8, smaller than a window, so
                xi[i, r:r + 8, q:q + 8, k % c] = 16              # x's variance does not cancel where y's does
            k += 1
        elif fm == "T":
            r, q = pixels[i - 3 - len(blocks)]
            yi[i, r, q, 0] = 16
    fam = np.array(fam)
    mp = ms_plan(1, f, h, w, c, m)
    assert mp is not None
    case = _Case(name=name, H=h, W=w, C=c, M=m, F=f, reps=1, fam=fam, xi=xi, yi=yi, mask=(fam != "M").astype(np.float32), plan=mp)
    # the regimes
    lv = mp.levels
    assert [(p.H, p.W) for p in lv] == [(h >> j, w >> j) for j in range(m)]
    if name.startswith("176"):
        assert [p.H for p in lv] == [176, 88, 44, 22, 11]
    if name.startswith("179"):
        assert [(p.H, p.W) for p in lv] == [(179, 181), (89, 90), (44, 45), (22, 22), (11, 11)] and not pool_vec(181, c, 4, 4)
    if m == 5:
        assert all(p.R == 4 and p.strips == 1 for p in lv) and (lv[4].H - 10) * (lv[4].W - 10) == 1
        dry = [(j, b) for j, p in enumerate(lv) for b in range(p.bands) if ssim_rows(b, p.R, p.H)[2] >= ssim_rows(b, p.R, p.H)[3]]
        assert any(j == 3 for j, _ in dry) and any(j == 4 for j, _ in dry), dry      # bands without any output row
    if name == "22x2049x1":
        assert lv[0].strips == 2 and lv[1].strips == 1 and (lv[1].H, lv[1].W) == (11, 1024)
    if name == "24x26x4":
        assert (lv[1].H, lv[1].W) == (12, 13) and pool_vec(26, 4, 4, 4) and pool_vec(26, 4, 2, 2) and 13 % 4 == 1     # a last group of one pixel
    if name == "176x176x1":
        assert pool_vec(176, 1, 4, 2) and pool_vec(88, 1, 4, 4) and not pool_vec(22, 1, 4, 4)
    expect_ms(case)
    return case


def _ms_levels(case, dtype=np.float64):
    x, y = case.xi / 16.0, case.yi / 16.0
    out = []
    for j in range(case.M):
        assert np.all(x * (16 * 4 ** j) == np.round(x * (16 * 4 ** j))) and x.max() <= 1.0          # dyadic: the means are exact
        out.append((x.astype(dtype), y.astype(dtype)))
        x, y = pool(x), pool(y)
    return out


def _ms_sum_bound(p, c):
    """the summation part of the bound of one (level, channel) total: per thread, the ng threads of the channel in order, the fold"""
    tot, nv = 0.0, (p.H - 10) * (p.W - 10)
    for s in range(p.strips):
        c0, c1, _, _, ws = strip_cols(p, s)
        for b in range(p.bands):
            _, _, o0, o1 = ssim_rows(b, p.R, p.H)
            if o0 < o1:
                n_t, ng = 4 * (o1 - o0), (ws + 3) // 4
                tot += U * ((o1 - o0) * (c1 - c0) * (n_t + 1) / 2 + n_t * ng * (ng + 1) / 2)
    return tot + U * (p.strips * p.bands + 1) / 2 * nv


def expect_ms(case):
    if getattr(case, "exp", None) is not None:
        return case.exp
    f, m, c = case.F, case.M, case.C
    e = _Case(sum=np.zeros((f, m, c)), bound=np.zeros((f, m, c)), nv=np.zeros(m), defect=np.full((f, m, c), np.inf))
    for j, (x, y) in enumerate(_ms_levels(case)):
        p = case.plan.levels[j]
        mo = moments(x, y)
        s_map, cs_map = maps(mo)
        tmap = s_map if j == m - 1 else cs_map
        e.nv[j] = (p.H - 10) * (p.W - 10)
        e.sum[:, j] = tmap.sum(axis=(1, 2))
        for i in range(f):
            fm = case.fam[i]
            if fm in ("D", "P", "T"):
                ep = window_eps([q[i:i + 1] for q in mo], KM_PIXEL if fm == "T" and j == 0 else KM_GENERAL)[0 if j == m - 1 else 1][0]
                e.bound[i, j] = 1.01 * (ep.sum(axis=(0, 1)) + _ms_sum_bound(p, c))
            elif fm == "I":
                e.bound[i, j] = 1.01 * (8 * U * e.nv[j] + _ms_sum_bound(p, c))
            if fm in ("P", "T"):                                 # the smallest defect claimed: an outermost row or column of the deficits
                d = 1.0 - tmap[i]
                for ch in range(c):
                    rows, cols = np.nonzero(d[:, :, ch].sum(axis=1))[0], np.nonzero(d[:, :, ch].sum(axis=0))[0]
                    if len(rows) and fm == "T":              # one row or column of windows sees the pixel: the claim is that row
                        e.defect[i, j, ch] = d[:, :, ch].sum()
                    elif len(rows):
                        e.defect[i, j, ch] = min(d[rows[0], :, ch].sum(), d[rows[-1], :, ch].sum(), d[:, cols[0], ch].sum(), d[:, cols[-1], ch].sum())
                    else:
                        e.bound[i, j, ch] = 0            # no window of this level and channel sees anything: exactly the count
    dead = case.fam == "M"
    e.sum[dead], e.bound[dead] = 0, 0
    e.bound[case.fam == "Z"] = 0
    trail = case.fam == "T"
    assert np.all(e.bound[trail][:, 1:] == 0) and np.all(e.bound[trail][:, 0, 0] > 0) if trail.any() else True
    live = np.isfinite(e.defect)
    assert live[case.fam == "P"].any(axis=2).all()
    e.smallest = float(e.defect[live].min())
    worst = np.unravel_index(np.argmax(np.where(live, e.bound / e.defect, 0)), live.shape)
    assert np.all(e.bound[live] < e.defect[live] / 2), (case.name, "bound / defect", worst, case.fam[worst[0]], e.bound[worst], e.defect[worst])
    # one window of family I is worth 1: half of it at most, 1/8 wherever a channel's sum does not run over 512 threads in sequence
    limit = 1 / 2 if max(p.W for p in case.plan.levels) > 2048 else 1 / 8
    assert e.bound[case.fam == "I"].max() < limit, (case.name, "family I", e.bound[case.fam == "I"].max(axis=(0, 2)))
    e.terms = e.sum / e.nv[None, :, None]
    e.terms_bound = np.where(e.bound > 0, e.bound / e.nv[None, :, None] + U, 0.0)
    w = np.array(MS_WEIGHTS[:m])[None, :, None]
    t = np.maximum(e.terms, 0)
    e.ms = np.where(dead, 0.0, (t ** w).prod(axis=1).mean(axis=1))
    # the product is monotone in every term: its values at the ends of the terms' intervals
    hi = ((t + e.terms_bound) ** w).prod(axis=1).mean(axis=1)
    lo = (np.maximum(e.terms - e.terms_bound, 0) ** w).prod(axis=1).mean(axis=1)
    e.ms_bound = np.where(e.bound.max(axis=(1, 2)) > 0, 1.01 * np.maximum(hi - e.ms, e.ms - lo) + 2 * U, 0.0)
    case.exp = e
    return e


def check_ms(case, ms, terms, what):
    """ms (F,), terms (F, M, C) fp32 numpy -> largest term error / bound"""
    e = expect_ms(case)
    dead = case.fam == "M"
    assert np.all(ms[dead] == 0) and np.all(terms[dead] == 0), f"{what}: masked: a masked frame's results are not 0"
    err = np.abs(terms.astype(np.float64) - e.terms)
    bad = ~(err <= e.terms_bound)
    assert not bad.any(), (f"{what}: terms: {int(bad.sum())} outside their bound; first (frame, level, channel) {tuple(np.argwhere(bad)[0])} "
                           f"(family {case.fam[np.argwhere(bad)[0][0]]}): got {terms[bad][0]!r} want {e.terms[bad][0]!r} bound {e.terms_bound[bad][0]:.3e}")
    bad = ~(np.abs(ms.astype(np.float64) - e.ms) <= e.ms_bound)
    assert not bad.any(), f"{what}: ms_ssim: frames {np.argwhere(bad).reshape(-1)[:8]}: got {ms[bad][:4]} want {e.ms[bad][:4]} bound {e.ms_bound[bad][:4]}"
    live = e.terms_bound > 0
    return float((err[live] / e.terms_bound[live]).max())


def twin_ms(case, defect=None):
    """The definition in fp32 numpy on the exact pyramid, summed per band and then per level in fp32"""
    f, m, c = case.F, case.M, case.C
    terms = np.zeros((f, m, c), np.float32)
    for j, (x, y) in enumerate(_ms_levels(case, np.float32)):
        p = case.plan.levels[j]
        s_map, cs_map = maps(moments(x, y, np.float32))
        tmap = s_map if j == m - 1 else cs_map
        tot, prev = np.zeros((f, c), np.float32), np.zeros((f, c), np.float32)
        for b in range(p.bands):
            _, _, o0, o1 = ssim_rows(b, p.R, p.H)
            if o0 < o1:
                prev = tmap[:, o0 - 5:o1 - 5].sum(axis=(1, 2), dtype=np.float32)
                tot = tot + prev
            elif defect == "band without output rows returns a stale value":
                tot = tot + prev
        terms[:, j] = (tot.astype(np.float64) / ((p.H - 10) * (p.W - 10))).astype(np.float32)
    if defect == "deficit booked to the wrong channel":
        pr = case.fam == "P"
        terms[pr] = np.roll(terms[pr], 1, axis=2)
    dead = case.fam == "M"
    terms[dead] = 0
    w = np.array(MS_WEIGHTS[:m])[None, :, None]
    ms = (np.maximum(terms.astype(np.float64), 0) ** w).prod(axis=1).mean(axis=1)
    return np.where(dead, 0, ms).astype(np.float32), terms


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("name", list(MS_CASES))
def test_multi_scale_terms(dev, name, pair):
    """Every (level, channel) term and the result: blocks of ones at every level, identical and zero pairs, the odd trailing row and column"""
    from video_vae_amd import ops
    case = ms_case(name)
    (xb, _), (yb, _) = clip_tensors(case, *pair)
    shape = (1, case.F, case.H, case.W, case.C)
    x, y = xb[:xb.numel() - 8].reshape(shape).to(dev), yb[:yb.numel() - 8].reshape(shape).to(dev)
    ms, terms = ops.ms_ssim(x, y, torch.from_numpy(case.mask).to(dev).reshape(1, -1), True, MS_WEIGHTS[:case.M], want_terms=True)
    r = _note("multi-scale terms", check_ms(case, ms.cpu().numpy()[0], terms.cpu().numpy()[0], name))
    print(f"{name} {pair}: largest term error / bound {r:.4f}")


# =========================================================================================== plane metrics
PM_CASES = {"13x17": (13, 17, dict(strips=1, bands=1)), "33x71": (33, 71, dict(strips=1, bands=3, R=11)),
            "37x1023": (37, 1023, dict(strips=2, SW=508, bands=3, R=13)), "37x2035": (37, 2035, dict(strips=3, SW=676, bands=3, R=13))}


@functools.lru_cache(maxsize=None)
def pm_case(name, swap=False):
    h, w, want = PM_CASES[name]
    case = build_clip("pm" + name, h, w, 1, lambda f: pm_plan(f, h, w, 2), lambda p: [5 + k * p.SW for k in range(1, p.strips)], 1, swap)
    p = case.plan
    keep = np.isin(case.fam, ("P", "Z"))                    # bytes: the probe and the zero frames (0 / 255, and 255 / 128 for a pair)
    case.fam, case.xi, case.yi = case.fam[keep], case.xi[keep], case.yi[keep]
    case.F = int(keep.sum())
    case.plan = pm_plan(case.F, h, w, 2)
    assert (case.plan.R, case.plan.bands, case.plan.strips) == (p.R, p.bands, p.strips)          # the seams the probes were placed at
    p = case.plan
    got = {k: getattr(p, k) for k in want}
    assert got == want, f"{name}: regime: the plan is {got}, the case was built for {want}"
    if name == "37x1023":
        assert pm_plan(case.F, h, 1022, 2).strips == 1      # the first width at which the plan cuts strips
    byte = lambda v: np.where(v == 16, 255, np.where(v == 8, 128, 0)).astype(np.uint8)[..., 0]
    case.a, case.b = byte(case.xi), byte(case.yi)
    x, y = case.a[..., None] / 255.0, case.b[..., None] / 255.0
    mo = moments(x, y)
    smap = maps(mo)[0]
    live = ~((mo[0] == 0) & (mo[1] == 0) & (mo[2] == 0) & (mo[3] == 0))
    nv, nsb = (h - 10) * (w - 10), p.strips * p.bands
    rows = max(ssim_rows(b, p.R, h)[3] - ssim_rows(b, p.R, h)[2] for b in range(p.bands))
    sumb = U * nv * ((4 * rows + 1) / 2 + 6 + p.threads // 64) + U * nv * (-(-nsb // 64) + 6)
    case.sse = ((case.a.astype(np.int64) - case.b) ** 2).sum(axis=(1, 2))
    case.ssim = smap.sum(axis=(1, 2, 3)) / nv
    case.bound = np.where(live.any(axis=(1, 2, 3)), 1.01 * (4 * U * live.sum(axis=(1, 2, 3)) + sumb) / nv + U, 0.0)
    assert case.bound.max() * nv < ROW_DEFECT / 2 and (case.bound > 0).sum() == (case.fam == "P").sum()
    return case


def check_pm(case, sse, ssim, what):
    assert sse.dtype == np.int64 and np.all(sse[:, 1:] == 0), f"{what}: sse: the chroma sums of mono are not 0"
    bad = sse[:, 0] != case.sse
    assert not bad.any(), f"{what}: sse: frames {np.argwhere(bad).reshape(-1)[:8]}: got {sse[bad, 0][:4]} want {case.sse[bad][:4]}"
    err = np.abs(ssim.astype(np.float64) - case.ssim)
    bad = ~(err <= case.bound)
    assert not bad.any(), (f"{what}: ssim_y: frames {np.argwhere(bad).reshape(-1)[:8]}: got {ssim[bad][:4]} want {case.ssim[bad][:4]} "
                           f"bound {case.bound[bad][:4]}")
    live = case.bound > 0
    return float((err[live] / case.bound[live]).max())


def twin_pm(case, defect=None):
    p, h, w = case.plan, case.H, case.W
    smap = maps(moments(case.a[..., None] / 255.0, case.b[..., None] / 255.0))[0].astype(np.float32)
    tot = np.zeros(case.F, np.float32)
    for s in range(p.strips):
        c0, c1 = 5 + s * p.SW, min(5 + (s + 1) * p.SW, w - 5)
        if defect == "window doubled at a strip seam" and s > 0:
            c0 -= 1
        tot = tot + smap[:, :, c0 - 5:c1 - 5].sum(axis=(1, 2, 3), dtype=np.float32)
    sse = np.zeros((case.F, 3), np.int64)
    sse[:, 0] = case.sse
    if defect == "a probe's error left out":
        sse[np.argmax(case.sse > 0), 0] -= 255 * 255
    return sse, (tot.astype(np.float64) / ((h - 10) * (w - 10))).astype(np.float32)


def _pm_view(a, res, dev):
    """The planes as a view that starts `res` bytes into a 16-byte aligned buffer, frames 3 bytes apart from dense"""
    n, h, w = a.shape
    stride = h * w + 3
    buf = torch.full((16 + n * stride,), 77, dtype=torch.uint8)
    v = torch.as_strided(buf, (n, h, w), (stride, w, 1), res)
    v.copy_(torch.from_numpy(a))
    g = buf.to(dev)
    assert g.data_ptr() % 16 == 0
    return torch.as_strided(g, (n, h, w), (stride, w, 1), res)


@pytest.mark.parametrize("name", list(PM_CASES))
def test_plane_metrics_probes(dev, name):
    """sse exactly and ssim_y per frame, probes at every seam and edge; every base residue of each operand (dword, word and byte loads)"""
    from video_vae_amd import ops
    residues = [(ra, rb) for ra in range(4) for rb in range(4)] if name == "13x17" else [(0, 0), (1, 2), (2, 3), (3, 1)]
    for swap in (False, True):
        case = pm_case(name, swap)
        for ra, rb in residues if not swap else residues[:2]:
            sse, ssim = ops.plane_metrics_u8((_pm_view(case.a, ra, dev), None, None), (_pm_view(case.b, rb, dev), None, None), "mono")
            r = _note("plane metrics ssim_y", check_pm(case, sse.cpu().numpy(), ssim.cpu().numpy(), f"{name} residues {ra},{rb} swap {swap}"))
    print(f"{name}: largest ssim_y error / bound {r:.4f}")


# =========================================================================================== temporal error
# name -> (H, W, C, offx, offy, chunks)
TM_CASES = {"4096": (32, 32, 4, 0, 0, 1), "4097": (17, 241, 1, 0, 0, 2), "4100": (25, 41, 4, 0, 0, 2), "3x4096+8": (58, 53, 4, 0, 0, 4),
            "64x4096+4": (1, 65537, 4, 0, 0, 65), "129x4096+4": (1, 132097, 4, 0, 0, 130), "4096 x off": (32, 32, 4, 1, 0, 1),
            "3x4096+8 y off": (58, 53, 4, 0, 3, 4)}


@functools.lru_cache(maxsize=None)
def tm_case(name):
    h, w, c, offx, offy, chunks = TM_CASES[name]
    b, t, n = 2, 3, h * w * c
    assert tm_chunks(n) == chunks, f"{name}: regime: {tm_chunks(n)} chunks, the case was built for {chunks}"
    if name == "4100":
        assert n - TM_CHUNK == 4                                  # a last chunk of one group
    g = _rng("tm", name)
    xi = g.integers(0, 17, (b, t, n))
    yi = np.clip(xi + g.integers(-1, 2, (b, t, n)), 0, 16)
    xi[:, :, -4:] = 8                                             # the last group of a frame: d = +-1 in each of its values
    yi[:, :, -4:] = 8 + (np.arange(t) % 2)[None, :, None]
    d = (yi[:, 1:] - yi[:, :-1]) - (xi[:, 1:] - xi[:, :-1])       # in sixteenths, |d| <= 2
    d2 = np.zeros((b, t - 1, chunks * TM_CHUNK), np.int64)
    d2[:, :, :n] = d * d
    part = d2.reshape(b * (t - 1), chunks, TM_CHUNK).sum(axis=2)
    assert np.abs(d).max() <= 2 and part.sum(axis=1).max() < 2 ** 24 and np.all(d2[:, :, n - 4:n] == 1)
    tmse = (part.sum(axis=1) / 256.0).astype(np.float32) * np.float32(1.0 / n)
    return _Case(name=name, B=b, T=t, H=h, W=w, C=c, n=n, chunks=chunks, offx=offx, offy=offy, xi=xi, yi=yi, part=part, tmse=tmse)


def check_tm(case, res, what):
    assert res.guards == 0, f"{what}: guards: {res.guards} sentinel words around part and tmse changed"
    assert res.unwritten == 0, f"{what}: unwritten: {res.unwritten} words of part or tmse still hold the sentinel"
    got = res.part.astype(np.float64) * 256.0
    bad = got != case.part
    assert not bad.any(), (f"{what}: chunk partials: {int(bad.sum())} differ; first (pair, chunk) {tuple(np.argwhere(bad)[0])}: got {got[bad][0]} "
                           f"want {case.part[bad][0]} (x 1/256)")
    bad = res.tmse != case.tmse
    assert not bad.any(), f"{what}: tmse: pairs {np.argwhere(bad).reshape(-1)}: got {res.tmse[bad]} want {case.tmse[bad]}"


def twin_tm(case, defect=None):
    part = (case.part / 256.0).astype(np.float32)
    fold = part.copy()
    if defect == "chunk left out of the fold":
        fold[:, -1] = 0
    if defect == "fold stops after its first lane trip":
        fold[:, 64:] = 0
    if defect == "last group of the last chunk unread":
        part[:, -1] -= np.float32(4 / 256.0)
    return _Case(part=part, tmse=fold.sum(axis=1, dtype=np.float32) * np.float32(1.0 / case.n), guards=0, unwritten=0)


def gpu_tm(case, dev, dtx, dty):
    lb = _lib()
    b, t, n = case.B, case.T, case.n
    bufs = []
    for v, dt, off in ((case.xi, dtx, case.offx), (case.yi, dty, case.offy)):
        buf = torch.zeros(v.size + off + 8, dtype=dt)
        buf[off:off + v.size] = torch.from_numpy(v.reshape(-1) / 16.0).to(dt)
        bufs.append(buf.to(dev))
    npart, npair = b * (t - 1) * case.chunks, b * (t - 1)
    assert lb.vvae_temporal_mse_part_floats(b, t, case.H, case.W, case.C) == npart
    buf = torch.full((GUARD + npart + GUARD + npair + GUARD,), SENT, dtype=torch.int32, device=dev)
    at = lambda words: ctypes.c_void_p(buf.data_ptr() + 4 * words)
    rc = lb.vvae_temporal_mse_fwd(ctypes.c_void_p(bufs[0].data_ptr() + case.offx * bufs[0].element_size()), DT[dtx],
                                  ctypes.c_void_p(bufs[1].data_ptr() + case.offy * bufs[1].element_size()), DT[dty], at(2 * GUARD + npart), at(GUARD),
                                  b, t, case.H, case.W, case.C, 1, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    w = buf.cpu().numpy()
    own = np.zeros(w.shape, bool)
    own[GUARD:GUARD + npart] = True
    own[2 * GUARD + npart:2 * GUARD + npart + npair] = True
    fl = w.view(np.float32)
    return _Case(part=fl[GUARD:GUARD + npart].reshape(npair, case.chunks).copy(), tmse=fl[2 * GUARD + npart:2 * GUARD + npart + npair].copy(),
                 guards=int((w[~own] != SENT).sum()), unwritten=int((w[own] == SENT).sum()))


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("name", list(TM_CASES))
def test_temporal_chunks(dev, name, pair):
    """Every (pair, chunk) partial and tmse at zero tolerance"""
    case = tm_case(name)
    check_tm(case, gpu_tm(case, dev, *pair), name)


def test_mirrors(dev):
    _mirrors_match_the_library()


# =========================================================================================== the CPU twin (tests/test_host.py)
def _host_rm(name):
    def run():
        for swap in (False, True):
            case = rm_case(name, swap)
            _note(f"cpu single scale, {case.entry}", check_rm(case, twin_rm(case), name))
    return run


def _host_ms(name):
    def run():
        case = ms_case(name)
        _note("cpu multi-scale terms", check_ms(case, *twin_ms(case), name))
    return run


def _host_pm(name):
    def run():
        for swap in (False, True):
            case = pm_case(name, swap)
            _note("cpu plane metrics ssim_y", check_pm(case, *twin_pm(case), name))
    return run


def _host_tm(name):
    def run():
        case = tm_case(name)
        check_tm(case, twin_tm(case), name)
    return run


HOST_CHECKS = ([("mirrors", _mirrors_match_the_library), ("probe-table", probe_table)] + [(f"single-{n}", _host_rm(n)) for n in RM_CASES] +
               [(f"ms-{n}", _host_ms(n)) for n in MS_CASES] + [(f"plane-{n}", _host_pm(n)) for n in PM_CASES] +
               [(f"temporal-{n}", _host_tm(n)) for n in TM_CASES])


def _defect_rm(name, defect, match, swap=False):
    def run():
        case = rm_case(name, swap)
        check_rm(case, twin_rm(case), name)
        _raises(lambda: check_rm(case, twin_rm(case, defect), name), match)
    return run


def _defect_ms(name, defect, match):
    def run():
        case = ms_case(name)
        _raises(lambda: check_ms(case, *twin_ms(case, defect), name), match)
    return run


def _defect_pm(name, defect, match):
    def run():
        case = pm_case(name)
        _raises(lambda: check_pm(case, *twin_pm(case, defect), name), match)
    return run


def _defect_tm(name, defect, match):
    def run():
        case = tm_case(name)
        _raises(lambda: check_tm(case, twin_tm(case, defect), name), match)
    return run


def _defect_corner():
    """One corner window of one probe's table left out of a partial of the small shapes: the bound resolves it"""
    for name in RM_CORNER:
        case = rm_case(name)
        res = twin_rm(case)
        i, r, q, ch = case.probes[0]
        assert (r, q, ch) == (0, 0, 0) and case.yi[i, 0, 0, 0] == 16 and case.xi[i, 0, 0, 0] == 0
        cr, cq = 5, 5                                               # the window that sees the probe at its corner
        s = maps(moments(case.xi[i:i + 1] / 16.0, case.yi[i:i + 1] / 16.0))[0][0, cr - 5, cq - 5, ch]
        assert abs((1 - s) - CORNER_DEFECT) < 5e-6
        b = cr // case.plan.R
        res.part[i, 0, b, 1] += np.float32(1 - s)                   # the window counted as if it saw nothing
        _raises(lambda: check_rm(case, res, name), "ss partials")


DEFECT_CHECKS = (
    [(f"single-{n}-band-seam-window-dropped", _defect_rm(n, "window dropped at a band seam", "ss partials")) for n in ("17x24x1", "37x53x3", "37x2049x1")] +
    [(f"single-{n}-strip-seam-window-doubled", _defect_rm(n, "window doubled at a strip seam", "ss partials")) for n in ("37x2049x1", "37x1011x4", "37x681x3")] +
    [(f"single-{n}-halo-row-one-off", _defect_rm(n, "halo row one off", "ss partials")) for n in ("17x24x1", "37x52x4", "37x513x4")] +
    [(f"single-{n}-mse-columns-from-5", _defect_rm(n, "mse columns from 5", "se partials")) for n in ("37x2049x1", "37x1025x2")] +
    [("single-guard-word-written", _defect_rm("37x53x3", "guard word written", "guards")),
     ("single-partial-never-written", _defect_rm("37x53x3", "partial never written", "unwritten")),
     ("single-masked-frame-read", _defect_rm("37x53x3", "masked frame read", "masked")),
     ("single-corner-window", _defect_corner)] +
    [(f"ms-{n}-wrong-channel", _defect_ms(n, "deficit booked to the wrong channel", "terms")) for n in ("176x176x3", "24x26x4")] +
    [(f"ms-{n}-stale-band", _defect_ms(n, "band without output rows returns a stale value", "terms")) for n in ("176x176x1", "179x181x3")] +
    [(f"plane-{n}-strip-seam-window-doubled", _defect_pm(n, "window doubled at a strip seam", "ssim_y")) for n in ("37x1023", "37x2035")] +
    [("plane-probe-error-left-out", _defect_pm("13x17", "a probe's error left out", "sse"))] +
    [("temporal-chunk-left-out", _defect_tm("3x4096+8", "chunk left out of the fold", "tmse")),
     ("temporal-second-lane-trip", _defect_tm("64x4096+4", "fold stops after its first lane trip", "tmse")),
     ("temporal-third-lane-trip", _defect_tm("129x4096+4", "fold stops after its first lane trip", "tmse")),
     ("temporal-last-group-unread", _defect_tm("4100", "last group of the last chunk unread", "chunk partials"))])
