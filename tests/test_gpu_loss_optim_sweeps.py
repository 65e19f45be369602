"""The streaming kernels of csrc/loss_optim.hip past one chunk and one sweep: masked MSE / MAE, reparameterise + KL, the plain loss tail on
512 partial columns, and the optimizer entries on raw buffers, against fp64 and with families of inputs whose results are exact.

The other direct tests of these kernels stay inside their smallest launch: one chunk per sample (grid.x == 1, the fold of the partials
adds one term) and buffers of 4099 floats (five workgroups, no second sweep, no cap).  Here the shapes alone reach the other regimes (no
tuning hook is touched) and every case asserts the regime it means to be in -- chunks, the length of the last chunk, elements per
workgroup, the number of norm partials, sweeps per workgroup -- from Python mirrors of pick_epb, vvae_sqnorm_blocks and the n / 1024 + 1,
cap 4096 grid, which are themselves held against vvae_loss_part_floats and vvae_sqnorm_blocks.  A retuning then fails loudly.

Families of the loss kernels (LOSS_TABLE lists the rows and what each is there for):

  * D, dyadic, zero tolerance.  P (and for the KL, T) a power of two; the mask is 0/1 with len a power of two per sample, the frames of
    a sample not a prefix, one sample fully masked (where B > 1); video - recon in {-2 .. 2}; mean in {-2 .. 2}, logvar = 0, eps and dz
    small integers.  Every per-workgroup sum is an integer (or half of one) below 2^24, 1 / (len P) and 1 / (len M) are powers of two,
    so every partial, every per-sample value and every gradient is a number of its dtype: mse, mae, each partial column, kl, z, drecon,
    dmean and dlogvar must equal the fp64 value bit for bit.  gmse / gmae / gkl are signed powers of two chosen so that the gradients are
    numbers of the output dtype (the builder asserts it).  The KL half rests on the device's fast exponential returning exactly 1.0f at
    0, which test_fast_exp_of_zero_is_one asserts on its own first.
  * N, integer numerators at an odd P (625, 36000: bf16x8 and fp32x4 vectors straddle frame boundaries, 1 / (len P) is inexact).
    A partial column times len P (exact in fp64) against the integer chunk sum at a relative 2^-22: 1 / (len * (float)P) takes two
    roundings (the product is exact below 2^24, so really one), the product with the sum one more, 2^-24 each, and one bit of margin.
    The builder asserts that 2^-22 of the largest chunk sum is below 1/2, half of what one element with |e| = 1 moves it by.  The folded
    per-sample value against the integer total at 2^-22 + (chunks - 1) 2^-24: the bound of an fp32 sum of non-negative terms in ANY
    order (the fold is a lane-strided loop and a shuffle tree, far shallower).  The builder asserts that this is below half of the
    smallest sum of a chunk that lies wholly in unmasked frames -- the last, ragged one and one past the 64th among them -- so one chunk
    dropped or doubled by the fold is seen.  The KL numerators likewise: t / (len * (float)M) is one rounding (len M < 2^24 is exact),
    so 2^-23 per partial and 2^-23 + (chunks - 1) 2^-24 for kl.  drecon is held at Family G's bar.
  * G, Gaussian: the inputs and the bars of test_gpu_ops.py::test_masked_mse_mae / test_reparam_kl at the odd-P rows; the reference is
    oracle.loss in fp64 with gradients by autograd.

B = 1 rows have no second sample: no fully masked one, and no video_div = 2 (video would need half a sample).

Optimizer families (n1 = 2 * 2^20 + 4099: 1024 norm partials, three ragged sweeps of sqnorm_kernel, n % 4 = 3; n2 = 4 * 2^20 + 4099: the
Adam / fold / swap / cast grids at their 4096-workgroup cap, five ragged sweeps of the scalar kernels).  Buffers are n + 8 long and are
compared whole: nothing beyond n may change.

  * Norm partials: g (and acc) integers in {-2 .. 2}; each fp64 partial must equal the sum over exactly the quads the grid-stride loop
    hands that workgroup (from the mirror), bit for bit, and gnorm_sq_out of a following Adam step (the in-kernel fold of 1024 partials,
    four per thread) their integer sum.
  * Adam, step one, exact: count = 1, m = v = 0, b1 = 0.5, b2 = 0.75, eps = 0, lr = 2^-3, g (or g + acc) in {+-1, +-2, +-4}, p a
    multiple of 2^-3.  Then m / c1 = g clip and sqrt(v / c2) = |g clip| in fp32 (sqrt of a rounded square is exact), so
    p_new = p - lr sign(g) whatever the clip factor is: p, the bf16 shadow and (decay 0.5, dyadic ema) the average at zero tolerance.
    The builder repeats this in fp32 torch for the case's clip factor, and a host check for 1, 0.5, 1/3 and 1 / ||g||.
    m against 0.5 g clip64 at a relative 6 * 2^-24 and v against 0.25 (g clip64)^2 at 14 * 2^-24: clip is rounded twice (the cast of
    the fp64 root, the division), g clip once: 3 roundings for m; the square doubles them and rounds once more: 7 for v; each 2^-24,
    doubled.  A wrong index changes m by a factor of two at the least.
  * Adam, generic: three steps (plain entry, clip biting in the first and third) on Gaussian p and g with the default b1, b2, eps against
    an fp64 restatement of the kernel's formula.  The bar on p is 4 x the worst ratio of the fp32 CPU restatement's error to
    2^-24 (|p| + lr sum_k |update_k|); the margin is for fused multiply-adds and the host's powf.  Both ratios are printed (FIGURE).
  * vvae_grad_fold_f32 (overwrite / accumulate, aligned / one element off, integers, dst NaN-filled in overwrite mode),
    vvae_swap_refresh_f32 and vvae_cast_f32_to_bf16 (aligned / one off): bitwise against torch, guards on both sides untouched.

No check says "mostly": the share of elements exempted is zero everywhere.

Every builder validates its case on the CPU before a GPU result is looked at: representability, the "bound < half a defect"
conditions, and a CPU result in the case's dtype (the kernels' formulas in fp32 torch, chunk by chunk) passing the very assertions the
GPU result meets.  tests/test_host.py runs the builders without a GPU (HOST_CHECKS) and feeds the assertions CPU results with one defect
each (DEFECT_CHECKS): every one of them must raise.
"""
import ctypes
import functools
import math
import types
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import loss as OLoss
from util import assert_close, assert_close_scaled, assert_exact, assert_representable, ints, rnd

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
PART_REL, KL_PART_REL = 4 * U, 2 * U     # Family N: one partial column (see the module docstring)
ADAM_M_REL, ADAM_V_REL = 6 * U, 14 * U   # Adam, step one
GUARD = 8


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 31 - 1000)


def _q(x, dtype):
    return x.to(dtype).float()


def _cdiv(a, b):
    return -(-a // b)


def _lib():
    from video_vae_amd._lib import lib
    return lib()


def _within(got, want64, tol, what, name):
    """|got - want| <= tol element for element (tol a number or a tensor; 0 where no rounding is allowed); a NaN never passes.
    -> the largest error / bound."""
    assert tuple(got.shape) == tuple(want64.shape), (what, name, tuple(got.shape), tuple(want64.shape))
    err = (got.detach().double().cpu() - want64.double()).abs()
    tol = torch.as_tensor(tol, dtype=F64).expand(err.shape)
    bad = ~(err <= tol)
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err != 0, float("inf"), 0.0).double())
    worst = float(ratio.nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    nbad = int(bad.sum())
    if nbad:
        idx = bad.nonzero()
        i = tuple(idx[0].tolist())
        raise AssertionError(f"{what}: {name}: {nbad}/{bad.numel()} elements outside the bound, worst error / bound {worst:.3e}; first at {i}: "
                             f"got {float(got[i])!r} want {float(want64[i])!r} bound {float(tol[i]):.3e}; last at {tuple(idx[-1].tolist())}")
    return worst


def _exact(got, want64, what, name):
    assert_exact(got.detach().cpu(), want64, f"{what}: {name}")


def _finite(res, what):
    for name, x in res.items():
        bad = int((~torch.isfinite(x.double())).sum())
        assert bad == 0, f"{what}: {name}: {bad}/{x.numel()} elements are not finite"


def _figure(what, name, value):
    print(f"FIGURE {what}: {name}: error / bound = {value:.3e}")


# =========================================================================================== the dispatch, mirrored
SQN_MAX_BLOCKS, STREAM_MAX_BLOCKS = 1024, 4096


def pick_epb(m, b):
    """loss_optim.hip: elements per workgroup of the per-sample loss kernels (about 2048 workgroups in all, never less than 2048 elements)."""
    want = max(1, 2048 // max(b, 1))
    return _cdiv(_cdiv(m, want), 2048) * 2048


def loss_regime(b, t, p):
    """-> M, elements per workgroup, chunks per sample, length of the last chunk."""
    m = t * p
    epb = pick_epb(m, b)
    chunks = _cdiv(m, epb)
    return m, epb, chunks, m - (chunks - 1) * epb


def sqnorm_blocks(n):
    return min(n // 1024 + 1, SQN_MAX_BLOCKS) if n > 0 else 0


def stream_blocks(n):
    """The grid of the Adam, fold, swap and cast launches."""
    return min(n // 1024 + 1, STREAM_MAX_BLOCKS)


def sweeps(items, blocks):
    """Trips of the grid-stride loop of the workgroup that makes the most, over ``items`` elements or vectors."""
    return _cdiv(items, blocks * 256)


# B, T, P, then the regime the row is there for: elements per workgroup, chunks, length of the last chunk
LOSS_TABLE = [(2, 8, 625, 2048, 3, 904),           # P odd, M % 8 = 0: bf16x8 and fp32x4 vectors straddle frames
              (2, 5, 1024, 2048, 3, 1024),         # dyadic P, ragged last chunk
              (1, 4, 36000, 2048, 71, 640),        # more than 64 chunks: a second term in the fold's lane loop
              (1, 8, 16384, 2048, 64, 2048),       # exactly 64 chunks
              (64, 41, 2048, 4096, 21, 2048),      # several vector loads per thread, ragged, B = 64
              (4, 16, 65536, 2048, 512, 2048),     # 512 partial columns into the plain loss tail
              (4, 8, 262144, 4096, 512, 4096)]     # production: several vector loads per thread and 512 columns
SMALL_ROWS = [(4, 5, 1024, 2048, 3, 1024), (4, 8, 625, 2048, 3, 904), (4, 8, 1024, 2048, 4, 2048)]   # the defect checks'
_REGIMES = {row[:3]: row[3:] for row in LOSS_TABLE + SMALL_ROWS}
ROWS_D = [r[:3] for r in LOSS_TABLE if r[2] & (r[2] - 1) == 0]
ROWS_ODD = [r[:3] for r in LOSS_TABLE if r[2] & (r[2] - 1) != 0]
ROWS_D_KL = [r for r in ROWS_D if r[1] in (4, 8, 16)]
ROWS_TAIL = [(4, 16, 65536), (4, 8, 262144)]


def claimed_regime(b, t, p):
    """The regime of a row, asserted from the mirror and held against what the library reports."""
    m, epb, chunks, last = loss_regime(b, t, p)
    assert (epb, chunks, last) == _REGIMES[(b, t, p)], ((b, t, p), (epb, chunks, last), "pick_epb moved: re-derive the shapes")
    floats = _lib().vvae_loss_part_floats(b, m)
    assert floats == 2 * b * chunks, (floats, b, chunks, "the mirror of pick_epb no longer matches the library")
    return m, epb, chunks, last


def _mirrors_match_the_library():
    for b, t, p in sorted(_REGIMES):
        claimed_regime(b, t, p)
    for b in (1, 2, 3, 4, 7, 64, 100, 2048, 5000):
        for m in (1, 540, 576, 2047, 2048, 2049, 5000, 83968, 144000, 2 ** 21, 3 * 2 ** 24 + 5):
            assert _lib().vvae_loss_part_floats(b, m) == 2 * b * _cdiv(m, pick_epb(m, b)), (b, m)
    for n in (1, 1023, 1024, 4099, 1024 * 1023 - 1, 1024 * 1023, N1, N2, 2 ** 31 + 7):
        assert _lib().vvae_sqnorm_blocks(n) == sqnorm_blocks(n), n
    assert _lib().vvae_loss_part_floats(0, 5) == 0 and _lib().vvae_sqnorm_blocks(0) == 0


def _is_pow2(x):
    return x > 0 and math.frexp(float(x))[0] == 0.5


def pow2_mask(b, t, seed):
    """(b, t) of 0 / 1: len a power of two below t per sample, on seeded frames that include the last one (so that the ragged last chunk
    counts); the last sample fully masked (b > 1)."""
    g = torch.Generator().manual_seed(seed)
    pows = [l for l in (1, 2, 4, 8, 16, 32) if l < t]
    mask = torch.zeros(b, t)
    for i in range(b):
        if b > 1 and i == b - 1:
            continue
        ln = pows[int(torch.randint(0, len(pows), (1,), generator=g))]
        mask[i, t - 1] = 1.0
        mask[i, torch.randperm(t - 1, generator=g)[:ln - 1]] = 1.0
    lens = mask.sum(1)
    assert all(_is_pow2(l) or (b > 1 and i == b - 1 and l == 0) for i, l in enumerate(lens.tolist()))
    assert bool((mask[:, 1:] != mask[:, :-1]).any(1)[lens > 0].all()), "adjacent frames must differ"
    return mask


def signed_pow2(n, seed, lo, hi):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 2, (n,), generator=g).double().mul(2).sub(1) * 2.0 ** torch.randint(lo, hi + 1, (n,), generator=g).double()


def _chunked(x, chunks, epb):
    """(b, M) -> (b, chunks, epb), zero-padded: chunk c holds what workgroup c of a sample reads."""
    return F.pad(x, (0, chunks * epb - x.shape[1])).view(x.shape[0], chunks, epb)


def _fold_separates(num, fold_rel, live, chunks):
    """The bound of a folded value is below half of the smallest non-zero chunk sum of its sample, the last (ragged) chunk and, past 64
    chunks, every chunk of the fold's second lane trip are non-zero: one of them dropped or doubled is seen."""
    nz = num > 0
    assert bool(nz[live, -1].all()) and (chunks <= 64 or bool(nz[live, 64:].all()))
    smallest = torch.where(nz, num, torch.full_like(num, float("inf"))).min(1).values
    assert bool((fold_rel * num.sum(1) < 0.5 * smallest)[live].all()), "the fold bound no longer separates one chunk"


# =========================================================================================== masked MSE / MAE: cases
@functools.lru_cache(maxsize=2)
def mse_case(family, b, t, p, dtype, div):
    k = types.SimpleNamespace()
    k.family, k.b, k.t, k.p, k.dtype, k.div = family, b, t, p, dtype, div
    k.m, k.epb, k.chunks, k.last = claimed_regime(b, t, p)
    assert b % div == 0
    nv = b // div
    seed = _seed("mse", family, b, t, p, str(dtype), div)
    if family in ("D", "N"):
        assert _is_pow2(p) == (family == "D")
        k.mask = pow2_mask(b, t, seed)
        k.video = ints((nv, t, p), seed + 1, -3, 3)
        k.recon = k.video.repeat_interleave(div, 0) - ints((b, t, p), seed + 2, -2, 2)
        k.gm, k.ga = signed_pow2(b, seed + 3, -1, 2), signed_pow2(b, seed + 4, -1, 2)
    else:                                                                # test_gpu_ops.py::test_masked_mse_mae
        k.video = _q(torch.rand((nv, t, p), generator=torch.Generator().manual_seed(seed + 1)), dtype)
        k.recon = _q(k.video.repeat_interleave(div, 0) + 0.3 * rnd((b, t, p), seed + 2), dtype)
        k.mask = torch.ones(b, t)
        k.mask[0, 1] = 0
        if b > 1:
            k.mask[1, t // 2:] = 0
        k.gm, k.ga = rnd((b,), seed + 3).double(), rnd((b,), seed + 4).double()
    for x in (k.video, k.recon):
        assert bool((_q(x, dtype) == x).all())
    if div > 1 and nv > 1:
        assert not torch.equal(k.video[0], k.video[1])
    m64 = k.mask.double()
    k.len = m64.sum(1).clamp_min(1.0)
    k.dead = k.mask.sum(1) == 0
    e = ((k.video.repeat_interleave(div, 0).double() - k.recon.double()) * m64[:, :, None]).view(b, k.m)
    ec = _chunked(e, k.chunks, k.epb)
    k.num2, k.num1 = (ec * ec).sum(2), ec.abs().sum(2)                  # (b, chunks): the numerators, integers in D and N
    sc = 1.0 / (k.len * p)
    k.part2, k.part1 = k.num2 * sc[:, None], k.num1 * sc[:, None]
    k.mse, k.mae = k.num2.sum(1) * sc, k.num1.sum(1) * sc
    k.drecon = (-(2.0 * e * (k.gm * sc)[:, None] + e.sign() * (k.ga * sc)[:, None])).view(b, t, p)
    k.e = e.float()
    if family == "G":
        r64 = k.recon.double().view(b, t, 1, 1, p).requires_grad_(True)
        mse_o, mae_o = OLoss.masked_mse_mae(k.video.repeat_interleave(div, 0).double().view(b, t, 1, 1, p), r64, m64)
        ((mse_o * k.gm).sum() + (mae_o * k.ga).sum()).backward()
        for mine, oracle in ((k.mse, mse_o), (k.mae, mae_o), (k.drecon, r64.grad.view(b, t, p))):
            assert float((mine - oracle.detach()).abs().max()) <= 1e-12 * float(oracle.detach().abs().max())
        k.mse, k.mae, k.drecon = mse_o.detach(), mae_o.detach(), r64.grad.view(b, t, p)
    else:
        assert_representable(k.num2, F32, 4 * k.epb)
        assert_representable(k.num1, F32, 2 * k.epb)
        assert_representable(k.num2.sum(1), F32, 4 * k.m)
        assert int(k.dead.sum()) == (1 if b > 1 else 0)
    if family == "D":
        assert all(_is_pow2(x) for x in (k.len * p).tolist())
        for x in (k.part2, k.part1, k.mse, k.mae):
            assert bool((x.float().double() == x).all())
        assert bool((k.drecon.to(dtype).double() == k.drecon).all()), "drecon is no tensor of the output dtype: move gmse / gmae"
    if family == "N":
        k.fold_rel = PART_REL + (k.chunks - 1) * U
        assert PART_REL * float(k.num2.max()) < 0.5
        for num in (k.num2, k.num1):
            _fold_separates(num, k.fold_rel, ~k.dead, k.chunks)
    for partials in (False, True):
        check_mse(k, cpu_mse(k, partials), "cpu")
    return k


def cpu_mse(k, partials, defect=None):
    """masked_mse_mae_fwd_kernel / _bwd_kernel and sum_chunks2_kernel in fp32 torch on the CPU, chunk by chunk; with ``defect`` one of the
    mistakes such kernels make: "chunk-dropped" / "chunk-doubled" (the last chunk of the last live sample, in the fold), "tail-unread" (what
    the last trip of the last chunk's loop reads), "straddle-mask" (a vector takes its first element's frame for all lanes),
    "video-index" (sample b reads video b, the last one where there is no such video), "len-zero" (no max(len, 1))."""
    b, t, p, dt = k.b, k.t, k.p, k.dtype
    vi = torch.arange(b) // k.div
    if defect == "video-index":
        vi = torch.arange(b).clamp_max(b // k.div - 1)
    frame = torch.arange(k.m) // p
    if defect == "straddle-mask":
        vec = 8 if dt == BF16 else 4
        assert k.m % vec == 0 and p % vec != 0
        frame = (torch.arange(k.m) // vec * vec) // p
    mfull = k.mask[:, frame]
    e = (k.video[vi].view(b, k.m) - k.recon.view(b, k.m)) * mfull
    es = e.clone()
    if defect == "tail-unread":
        es[:, k.m - (k.last % 256 or 256):] = 0.0
    ec = _chunked(es, k.chunks, k.epb)
    ln = k.mask.sum(1)
    if defect != "len-zero":
        ln = ln.clamp_min(1.0)
    sc = 1.0 / (ln * torch.tensor(float(p), dtype=F32))
    part2, part1 = (ec * ec).sum(2) * sc[:, None], ec.abs().sum(2) * sc[:, None]
    res = {}
    if partials:
        res["part2"], res["part1"] = part2, part1
    else:
        w = torch.ones(b, k.chunks)
        if defect in ("chunk-dropped", "chunk-doubled"):
            w[int((~k.dead).nonzero()[-1]), -1] = 0.0 if defect == "chunk-dropped" else 2.0
        res["mse"], res["mae"] = (part2 * w).sum(1), (part1 * w).sum(1)
    g2, g1 = k.gm.float() * sc, k.ga.float() * sc
    res["drecon"] = (-mfull * (2.0 * e * g2[:, None] + e.sign() * g1[:, None])).view(b, t, p).to(dt)
    return res


def check_mse(k, res, route):
    """Every assertion of a case on {mse, mae (b) | part2, part1 (b, chunks); drecon (b, t, p)}; a route may return a part of them."""
    what = f"{route} {k.family} {k.dtype} (B {k.b}, T {k.t}, P {k.p}, video_div {k.div})"
    _finite(res, what)
    f32 = k.dtype == F32
    r = 1e-3 if f32 else 2e-2                                            # test_gpu_ops.py::test_masked_mse_mae
    lp = k.len * k.p
    for name, x in res.items():
        want = getattr(k, name)
        if k.family == "D":
            _exact(x, want, what, name)
        elif name == "drecon":
            assert_close_scaled(x, want, rel=r, what=f"{what}: drecon")
        elif k.family == "G":
            assert_close(x, want, rtol=r, atol=1e-6, what=f"{what}: {name}")
        elif name in ("part2", "part1"):
            num = k.num2 if name == "part2" else k.num1
            _figure(what, name, _within(x.double().cpu() * lp[:, None], num, PART_REL * num, what, name))
        else:
            tot = (k.num2 if name == "mse" else k.num1).sum(1)
            _figure(what, name, _within(x.double().cpu() * lp, tot, k.fold_rel * tot, what, name))
        if bool(k.dead.any()):
            assert float(x[k.dead].float().abs().max()) == 0.0, f"{what}: {name}: the fully masked sample is not all zero"


# =========================================================================================== reparameterise + KL: cases
KL_FORMS = ("joint", "z", "kl")


@functools.lru_cache(maxsize=2)
def kl_case(family, b, t, p, dtype, masked):
    k = types.SimpleNamespace()
    k.family, k.b, k.t, k.p, k.dtype, k.masked = family, b, t, p, dtype, masked
    k.m, k.epb, k.chunks, k.last = claimed_regime(b, t, p)
    seed = _seed("kl", family, b, t, p, str(dtype), masked)
    shape = (b, t, p)
    if family in ("D", "N"):
        assert (_is_pow2(p) and _is_pow2(t)) == (family == "D")
        k.mask = pow2_mask(b, t, seed) if masked else None
        k.mean, k.logvar = ints(shape, seed + 1, -2, 2), torch.zeros(shape)
        k.eps, k.dz = ints(shape, seed + 2, -3, 3), ints(shape, seed + 3, -2, 2)
    else:                                                                # test_gpu_ops.py::test_reparam_kl
        k.mean, k.logvar = _q(rnd(shape, seed + 1), dtype), _q(0.5 * rnd(shape, seed + 2) - 1, dtype)
        k.eps, k.dz = rnd(shape, seed + 3), rnd(shape, seed + 4)
        k.mask = None
        if masked:
            k.mask = torch.ones(b, t)
            k.mask[0, 1] = 0
            if b > 1:
                k.mask[1, t // 2:] = 0
    m64 = k.mask.double() if masked else torch.ones(b, t, dtype=F64)
    k.len = m64.sum(1).clamp_min(1.0)
    k.dead = m64.sum(1) == 0
    if family == "G":
        k.gkl = rnd((b,), seed + 5).double()
    else:                                                                # kscale = gkl / (len M) = +-2^-4: dz + kscale mu is a bf16 number
        k.gkl = signed_pow2(b, seed + 5, -4, -4) * k.len * k.m
    mo, lo = k.mean.double().requires_grad_(True), k.logvar.double().requires_grad_(True)
    zo = mo + k.eps.double() * torch.exp(lo / 2)
    klo = OLoss.kl_per_sample(mo.view(b, t, 1, p), lo.view(b, t, 1, p), m64)
    gz = torch.autograd.grad((zo * k.dz.double()).sum(), [mo, lo], retain_graph=True)
    gk = torch.autograd.grad((klo * k.gkl).sum(), [mo, lo])
    k.z, k.kl = zo.detach(), klo.detach()
    k.grads = {"z": gz, "kl": gk, "joint": (gz[0] + gk[0], gz[1] + gk[1])}
    terms = _chunked((0.5 * (torch.exp(k.logvar.double()) - 1 - k.logvar.double() + k.mean.double() ** 2) * m64[:, :, None]).view(b, k.m), k.chunks, k.epb)
    k.num = terms.sum(2)                                                 # (b, chunks): halves of integers in D and N
    assert float((k.num.sum(1) / (k.len * k.m) - k.kl).abs().max()) <= 1e-12 * float(k.kl.abs().max().clamp_min(1e-30))
    if family != "G":
        assert_representable(2 * k.num, F32, 4 * k.epb)
        assert_representable(2 * k.num.sum(1), F32, 4 * k.m)
        assert bool((k.z == (k.mean + k.eps).double()).all())
        assert int(k.dead.sum()) == (1 if masked and b > 1 else 0)
    if family == "D":
        assert all(_is_pow2(x) for x in (k.len * k.m).tolist())
        assert bool((k.kl.float().double() == k.kl).all())
        for form in KL_FORMS:
            for g in k.grads[form]:
                assert bool((g.to(dtype).double() == g).all()), f"{form}: a gradient is no tensor of the output dtype"
        assert bool((k.grads["z"][1] == 0.5 * k.dz.double() * k.eps.double()).all()) and float(k.grads["kl"][1].abs().max()) == 0.0
    if family == "N":
        k.fold_rel = KL_PART_REL + (k.chunks - 1) * U
        assert float(k.len.max()) * k.m < 2 ** 24                        # len * (float)M is exact
        _fold_separates(k.num, k.fold_rel, ~k.dead, k.chunks)
    for form in KL_FORMS:
        check_kl(k, cpu_kl(k, form), form, "cpu")
    return k


def cpu_kl(k, form, defect=None):
    """reparam_kl_fwd_kernel / _bwd_kernel and sum_chunks_kernel in fp32 torch on the CPU; ``defect``: "chunk-dropped" / "chunk-doubled" (the
    last chunk of the last live sample, in the fold), "len-zero" (no max(len, 1))."""
    b, t, p, dt = k.b, k.t, k.p, k.dtype
    mu, lv, res = k.mean, k.logvar, {}
    mask = k.mask if k.masked else torch.ones(b, t)
    ln = mask.sum(1)
    if defect != "len-zero":
        ln = ln.clamp_min(1.0)
    den = ln * torch.tensor(float(k.m), dtype=F32)
    dm, dl = torch.zeros_like(mu), torch.zeros_like(mu)
    if form != "kl":
        res["z"] = mu + k.eps * torch.exp(0.5 * lv)
        dm, dl = dm + k.dz, dl + k.dz * k.eps * 0.5 * torch.exp(0.5 * lv)
    if form != "z":
        terms = 0.5 * (torch.exp(lv) - 1.0 - lv + mu * mu) * mask[:, :, None]
        part = _chunked(terms.view(b, k.m), k.chunks, k.epb).sum(2) / den[:, None]
        w = torch.ones(b, k.chunks)
        if defect in ("chunk-dropped", "chunk-doubled"):
            w[int((~k.dead).nonzero()[-1]), -1] = 0.0 if defect == "chunk-dropped" else 2.0
        res["kl"] = (part * w).sum(1)
        ks = (k.gkl.float() / den)[:, None, None] * mask[:, :, None]
        dm, dl = dm + ks * mu, dl + ks * 0.5 * (torch.exp(lv) - 1.0)
    res["dmean"], res["dlogvar"] = dm.to(dt), dl.to(dt)
    return res


def check_kl(k, res, form, route):
    """Every assertion of a case on {z (b, t, p), kl (b); dmean, dlogvar (b, t, p)} of one entry point; a route may return a part of them."""
    what = f"{route} {form} {k.family} {k.dtype} (B {k.b}, T {k.t}, P {k.p}, {'masked' if k.masked else 'no mask'})"
    _finite(res, what)
    r = 1e-3 if k.dtype == F32 else 2e-2                                 # test_gpu_ops.py::test_reparam_kl
    for name, x in res.items():
        want = {"z": k.z, "kl": k.kl, "dmean": k.grads[form][0], "dlogvar": k.grads[form][1]}[name]
        if k.family == "D" or (k.family == "N" and name == "z"):
            _exact(x, want, what, name)
        elif name == "kl" and k.family == "N":
            tot = k.num.sum(1)
            _figure(what, name, _within(x.double().cpu() * (k.len * k.m), tot, k.fold_rel * tot, what, name))
        elif name == "z":
            assert_close(x, want, rtol=r, atol=1e-4, what=f"{what}: z")
        elif name == "kl":
            assert_close(x, want, rtol=r, atol=1e-5, what=f"{what}: kl")
        else:
            assert_close_scaled(x, want, rel=r, what=f"{what}: {name}")
        if bool(k.dead.any()) and name == "kl":
            assert float(x[k.dead].abs().max()) == 0.0, f"{what}: kl: the fully masked sample is not zero"


# =========================================================================================== the plain loss tail on 512 columns
TAIL_HPARAMS = {"max_compression_rate": 2, "magnify_negatives_rate": 4, "gamma1": 0.25, "gamma2": 0.5}
TAIL_KL_P = 64


@functools.lru_cache(maxsize=1)
def tail_case(b, t, p):
    """masked_mse_mae(partials=True) of a Family D case and kl_per_sample(...).unsqueeze(1) of a small one on the same mask into
    plain_loss_tail.  MSE and kl_loss are means of exact dyadics over B = 4 samples: exact.  The others against fp64."""
    k = types.SimpleNamespace()
    k.mse = mse_case("D", b, t, p, BF16, 1)
    k.b, k.t, k.mask = b, t, k.mse.mask
    assert k.mse.chunks == 512 and _is_pow2(b) and _is_pow2(t)
    seed = _seed("tail", b, t, p)
    k.mean = ints((b, t, TAIL_KL_P), seed, -2, 2)
    k.sel = ints((b, t, 1, 1), seed + 1, 0, 4) / 4.0
    hp, m64 = TAIL_HPARAMS, k.mask.double()
    lens, km = k.mse.len, t * TAIL_KL_P
    k.kl = (0.5 * k.mean.double() ** 2 * m64[:, :, None]).sum((1, 2)) / (lens * km)
    assert bool((k.kl.float().double() == k.kl).all()) and all(_is_pow2(x) for x in (lens * km).tolist())
    sel64 = k.sel.double().requires_grad_(True)
    density = (sel64.reshape(b, t) * m64).sum(1, keepdim=True) / lens[:, None]
    s_loss = torch.square(OLoss.magnify_negatives(density - 1 / hp["max_compression_rate"], hp["magnify_negatives_rate"])).mean()
    k.mse_mean, k.kl_mean = k.mse.mse.mean(), k.kl.mean()
    loss = k.mse_mean + hp["gamma1"] * s_loss + hp["gamma2"] * k.kl_mean
    loss.backward()
    k.out = torch.stack([loss.detach(), k.mse_mean, s_loss.detach(), k.kl_mean, density.detach().mean()])
    k.dsel = sel64.grad
    assert bool((k.out[[1, 3]].float().double() == k.out[[1, 3]]).all())
    sc = 1.0 / (lens * p)
    k.drecon = (-(2.0 * k.mse.e.double() * (sc / b)[:, None])).view(b, t, p)
    k.dmean = (hp["gamma2"] / b / (lens * km))[:, None, None] * m64[:, :, None] * k.mean.double()
    for x in (k.drecon, k.dmean):
        assert bool((x.to(BF16).double() == x).all())
    check_tail(k, cpu_tail(k), "cpu")
    return k


def cpu_tail(k):
    """loss_tail_plain_kernel in fp32 torch on the CPU, fed the CPU partials of the two cases."""
    b, t, hp = k.b, k.t, TAIL_HPARAMS
    part2 = cpu_mse(k.mse, True)["part2"]
    ln = k.mask.sum(1).clamp_min(1.0)
    kl = (0.5 * k.mean ** 2 * k.mask[:, :, None]).sum((1, 2)) / (ln * float(t * TAIL_KL_P))
    msum = part2.sum(1)
    density = (k.sel.reshape(b, t) * k.mask).sum(1) / ln
    d = density - 1.0 / hp["max_compression_rate"]
    slope = torch.where(d < 0, torch.tensor(float(hp["magnify_negatives_rate"])), torch.tensor(1.0))
    mm = d * slope
    a, q, kk, dn = msum.sum() / b, (mm * mm).sum() / b, kl.sum() / b, density.sum() / b
    out = torch.stack([a + hp["gamma1"] * q + hp["gamma2"] * kk, a, q, kk, dn])
    dsel = (hp["gamma1"] / b * 2.0 * mm * slope / ln)[:, None] * k.mask
    sc = 1.0 / (ln * float(k.mse.p))
    drecon = (-(2.0 * k.mse.e * (sc / b)[:, None])).view(k.mse.b, k.mse.t, k.mse.p).to(BF16)
    dmean = ((hp["gamma2"] / b / (ln * float(t * TAIL_KL_P)))[:, None, None] * k.mask[:, :, None] * k.mean).to(BF16)
    return {"out": out, "dsel": dsel.view(b, t, 1, 1), "drecon": drecon, "dmean": dmean, "dlogvar": torch.zeros_like(dmean)}


def check_tail(k, res, route):
    what = f"{route} plain loss tail (B {k.b}, T {k.t}, P {k.mse.p})"
    _finite(res, what)
    _exact(res["out"][[1, 3]], k.out[[1, 3]], what, "MSE, kl_loss")
    assert_close(res["out"], k.out, rtol=1e-5, atol=1e-6, what=f"{what}: out")      # test_plain_loss_tail_matches_the_framework_ops
    assert_close_scaled(res["dsel"], k.dsel, rel=1e-5, what=f"{what}: d selection")
    _exact(res["drecon"], k.drecon, what, "drecon")
    _exact(res["dmean"], k.dmean, what, "dmean")
    _exact(res["dlogvar"], torch.zeros_like(k.dmean), what, "dlogvar")


# =========================================================================================== optimizer streams: cases
N1, N2 = 2 * 1048576 + 4099, 4 * 1048576 + 4099


def sq_owner(n):
    """Which workgroup of sqnorm_kernel adds quad i (the n % 4 tail is workgroup 0's)."""
    return (torch.arange(n // 4) // 256) % sqnorm_blocks(n)


def _sq_parts(x, n, dtype):
    n4 = n // 4
    q = (x[:n4 * 4].to(dtype) ** 2).view(n4, 4).sum(1)
    part = torch.zeros(sqnorm_blocks(n), dtype=dtype).index_add_(0, sq_owner(n), q)
    part[0] += (x[n4 * 4:n].to(dtype) ** 2).sum()
    return part


@functools.lru_cache(maxsize=2)
def sq_case(n, acc):
    k = types.SimpleNamespace()
    k.n, k.acc, k.nparts = n, acc, sqnorm_blocks(n)
    seed = _seed("sq", n, acc)
    k.g = ints((n + GUARD,), seed, -2, 2)
    k.a = ints((n + GUARD,), seed + 1, -2, 2) if acc else None
    x = k.g + k.a if acc else k.g
    k.part = _sq_parts(x, n, F64)
    k.total = (x[:n].double() ** 2).sum()
    assert float(k.part.sum()) == float(k.total)
    k.sweeps = sweeps(n // 4, k.nparts)
    assert_representable(k.part, F32, 4 * 4 * 256 * k.sweeps + 4 * 3)
    check_sq(k, cpu_sq(k), "cpu")
    return k


def cpu_sq(k, defect=None):
    """sqnorm_kernel in fp32 torch on the CPU and the fold of its partials in adam_clip_kernel; ``defect``: "tail-out" (the n % 4 tail
    left out), "fold-256" (only the first 256 partials folded)."""
    x = k.g + k.a if k.acc else k.g
    n = k.n - k.n % 4 if defect == "tail-out" else k.n
    part = _sq_parts(x, n, F32).double()
    if defect == "tail-out":
        assert part.numel() == k.nparts
    return {"part": part, "gnorm_sq": (part[:256] if defect == "fold-256" else part).sum()}


def check_sq(k, res, route):
    what = f"{route} sqnorm (n {k.n}, {'g + acc' if k.acc else 'g'})"
    _finite(res, what)
    _exact(res["part"], k.part, what, "part")
    assert float(res["part"].sum()) == float(k.total), f"{what}: the partials do not add up to the sum of squares"
    _exact(res["gnorm_sq"].reshape(1), k.total.reshape(1), what, "gnorm_sq_out")


ADAM1 = dict(lr=2.0 ** -3, b1=0.5, b2=0.75, eps=0.0, decay=0.5)
ADAM_REGIMES = ("noclip", "bite", "loose")          # gnorm_part NULL and gscale 0.5; max_norm 1; max_norm 2^13 above ||g||


def _f(x):
    return torch.tensor(x, dtype=F32)


def clip_f32(tot, gscale, max_norm):
    """adam_clip_kernel's clip factor from the folded sum of squares (fp64), in fp32 as the kernel computes it."""
    gn = np.float32(gscale) * np.float32(np.sqrt(np.float64(tot)))
    return float(np.float32(gscale) * np.float32(max_norm) / gn) if gn >= np.float32(max_norm) else float(np.float32(gscale))


def adam_f32(p, g, m, v, clip, lr, b1, b2, eps, count, ema=None, decay=0.0):
    """The update of adam_clip_kernel in fp32 torch (every operation rounded, no fused multiply-add); c1, c2 as the launcher computes them."""
    one, b1, b2 = _f(1.0), _f(b1), _f(b2)
    c1, c2 = one - b1 ** _f(float(count)), one - b2 ** _f(float(count))
    gi = g * _f(clip)
    mi = b1 * m + (one - b1) * gi
    vi = b2 * v + (one - b2) * gi * gi
    pn = p - _f(lr) * (mi / c1) / (torch.sqrt(vi / c2) + _f(eps))
    en = _f(decay) * ema + (one - _f(decay)) * pn if ema is not None else None
    return pn, mi, vi, en


@functools.lru_cache(maxsize=1)
def adam1_case(n, ema, acc, regime):
    k = types.SimpleNamespace()
    k.n, k.ema, k.acc, k.regime = n, ema, acc, regime
    k.blocks, k.nparts = stream_blocks(n), sqnorm_blocks(n)
    k.sweeps = sweeps(n, k.blocks)
    seed = _seed("adam1", n, ema, acc, regime)
    nb = n + GUARD
    s = torch.tensor([1.0, 2.0, 4.0, -1.0, -2.0, -4.0])[ints((nb,), seed, 0, 5).long()]
    k.a = ints((nb,), seed + 1, -2, 2) if acc else None
    k.g = s - k.a if acc else s
    k.p0, k.e0 = ints((nb,), seed + 2, -64, 64) / 8.0, ints((nb,), seed + 3, -64, 64) / 8.0
    k.tot = float((s[:n].double() ** 2).sum())
    k.gscale, k.max_norm = (0.5, 1.0) if regime == "noclip" else (1.0, 1.0) if regime == "bite" else (1.0, 2.0 ** 13)
    norm = math.sqrt(k.tot)
    assert regime != "loose" or norm < k.max_norm
    k.clip64 = 0.5 if regime == "noclip" else 1.0 / norm if regime == "bite" else 1.0
    k.clip = clip_f32(k.tot, k.gscale, k.max_norm) if regime != "noclip" else 0.5
    assert abs(k.clip / k.clip64 - 1) <= 2 * U
    inside = torch.arange(nb) < n
    keep = lambda new, old: torch.where(inside, new, old)
    zero = torch.zeros(nb, dtype=F64)
    k.p = keep(k.p0 - ADAM1["lr"] * s.sign(), k.p0).double()
    k.sh = keep(k.p.float().bfloat16().double(), zero)
    k.e = keep(0.5 * k.e0 + 0.5 * k.p.float(), k.e0).double()
    for x in (k.p, k.e):
        assert bool((x.float().double() == x).all())
    k.mm, k.vv = keep(0.5 * s.double() * k.clip64, zero), keep(0.25 * (s.double() * k.clip64) ** 2, zero)
    assert bool((k.p != k.p0.double())[:n].all())                       # a stale element shows
    check_adam1(k, cpu_adam1(k), "cpu")
    return k


def cpu_adam1(k, defect=None, clip=None):
    """One launch of adam_clip_kernel on the case's buffers in fp32 torch; ``defect`` "sweep-skipped": the second sweep of the grid leaves
    p, m, v, the shadow and the average as they were."""
    n, nb = k.n, k.n + GUARD
    g = (k.g + k.a if k.acc else k.g)
    pn, mi, vi, en = adam_f32(k.p0, g, torch.zeros(nb), torch.zeros(nb), k.clip if clip is None else clip, ADAM1["lr"], ADAM1["b1"], ADAM1["b2"],
                              ADAM1["eps"], 1, k.e0, ADAM1["decay"])
    inside = torch.arange(nb) < n
    if defect == "sweep-skipped":
        assert k.sweeps > 2
        idx = torch.arange(nb)
        inside = inside & ~((idx >= k.blocks * 256) & (idx < 2 * k.blocks * 256))
    zero = torch.zeros(nb)
    res = {"p": torch.where(inside, pn, k.p0), "m": torch.where(inside, mi, zero), "v": torch.where(inside, vi, zero),
           "sh": torch.where(inside, pn, zero).bfloat16()}
    if k.ema:
        res["e"] = torch.where(inside, en, k.e0)
    if k.regime != "noclip":
        res["gnorm_sq"] = torch.tensor(k.tot, dtype=F64)
    return res


def check_adam1(k, res, route):
    """Whole buffers, guards included: p, the shadow and the average at zero tolerance; m and v at ADAM_M_REL / ADAM_V_REL."""
    what = f"{route} adam step one (n {k.n}, ema {k.ema}, acc {k.acc}, {k.regime})"
    _finite(res, what)
    _exact(res["p"], k.p, what, "p")
    _exact(res["sh"], k.sh, what, "shadow")
    if k.ema:
        _exact(res["e"], k.e, what, "ema")
    _within(res["m"], k.mm, ADAM_M_REL * k.mm.abs(), what, "m")
    _within(res["v"], k.vv, ADAM_V_REL * k.vv, what, "v")
    if "gnorm_sq" in res:
        assert float(res["gnorm_sq"]) == k.tot, f"{what}: gnorm_sq_out: {float(res['gnorm_sq'])!r} is not {k.tot!r}"


def _adam1_holds_for_any_clip():
    """p - lr sign(g) bit for bit in fp32 torch for clip factors 1, 0.5, 1/3 and 1 / ||g||, without underflow."""
    k = adam1_case(N1, True, False, "bite")
    for clip in (1.0, 0.5, float(np.float32(1.0) / np.float32(3.0)), k.clip):
        res = cpu_adam1(k, clip=clip)
        for name, want in (("p", k.p), ("sh", k.sh), ("e", k.e)):
            _exact(res[name], want, f"clip {clip!r}", name)
        assert float(res["v"][:k.n].min()) > 2.0 ** -100


ADAMG = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, steps=3, max_norm=(1.0, 1e9, 1.0))
ADAMG_MARGIN = 4.0


@functools.lru_cache(maxsize=1)
def adamg_case():
    """Three steps on n1 in fp64 (the reference) and in fp32 torch (which sets the bar, see the module docstring)."""
    k = types.SimpleNamespace()
    n, nb = N1, N1 + GUARD
    k.n = n
    k.p0 = rnd((nb,), _seed("adamg", "p"))
    k.gs = [rnd((nb,), _seed("adamg", "g", i)) for i in range(ADAMG["steps"])]
    lr, b1, b2, eps = (float(np.float32(ADAMG[x])) for x in ("lr", "b1", "b2", "eps"))
    p, m, v = k.p0.double(), torch.zeros(nb, dtype=F64), torch.zeros(nb, dtype=F64)
    p32, m32, v32 = k.p0.clone(), torch.zeros(nb), torch.zeros(nb)
    moved = torch.zeros(nb, dtype=F64)
    k.bites = []
    for i, g in enumerate(k.gs):
        mx = ADAMG["max_norm"][i]
        tot = float((g[:n].double() ** 2).sum())
        k.bites.append(math.sqrt(tot) >= mx)
        gi = g.double() * (mx / math.sqrt(tot) if k.bites[-1] else 1.0)
        m, v = b1 * m + (1 - b1) * gi, b2 * v + (1 - b2) * gi * gi
        upd = (m / (1 - b1 ** (i + 1))) / (torch.sqrt(v / (1 - b2 ** (i + 1))) + eps)
        p = p - lr * upd
        moved += lr * upd.abs()
        clip = clip_f32(float(_sq_parts(g, n, F32).double().sum()), 1.0, mx)
        p32, m32, v32, _ = adam_f32(p32, g, m32, v32, clip, ADAMG["lr"], ADAMG["b1"], ADAMG["b2"], ADAMG["eps"], i + 1)
    assert k.bites == [True, False, True]
    k.p, k.unit = p[:n], U * (p.abs() + moved)[:n]
    k.cpu_ratio = float(((p32[:n].double() - k.p).abs() / k.unit).max())
    assert 0.5 <= k.cpu_ratio < 1e4, k.cpu_ratio
    k.bar = ADAMG_MARGIN * k.cpu_ratio
    return k


def check_adamg(k, p, route):
    what = f"{route} adam, three generic steps (n {k.n})"
    _finite({"p": p}, what)
    ratio = _within(p[:k.n], k.p, k.bar * k.unit, what, "p")
    print(f"FIGURE {what}: worst |p - p64| / (2^-24 (|p| + lr sum |update|)): fp32 on the CPU {k.cpu_ratio:.3f}, here {k.bar * ratio:.3f}, bar {k.bar:.3f}")
    assert torch.equal(p[k.n:].cpu(), k.p0[k.n:]), f"{what}: the guard behind p changed"


FOLD_FORMS = [(ovw, off) for ovw in (True, False) for off in (0, 1)]


@functools.lru_cache(maxsize=1)
def fold_case(n, overwrite, off):
    """dst[off : off + n] (+)= src[off : off + n] inside buffers with GUARD elements on both sides."""
    k = types.SimpleNamespace()
    k.n, k.overwrite, k.off, k.lo = n, overwrite, off, GUARD + off
    nb = n + 2 * GUARD + 1
    seed = _seed("fold", n, overwrite, off)
    k.src, k.dst0 = ints((nb,), seed, -1000, 1000), ints((nb,), seed + 1, -1000, 1000)
    inside = (torch.arange(nb) >= k.lo) & (torch.arange(nb) < k.lo + n)
    k.dst = torch.where(inside, k.src if overwrite else k.dst0 + k.src, k.dst0).double()
    if overwrite:
        k.dst0 = torch.where(inside, torch.full((nb,), float("nan")), k.dst0)         # dst is never read
    k.blocks = stream_blocks(n)
    check_fold(k, cpu_fold(k), "cpu")
    return k


def cpu_fold(k, defect=None):
    """grad_fold_kernel on the CPU; ``defect`` "one-past": it also folds the element behind the last."""
    hi = k.lo + k.n + (1 if defect == "one-past" else 0)
    dst = k.dst0.clone()
    dst[k.lo:hi] = k.src[k.lo:hi] if k.overwrite else dst[k.lo:hi] + k.src[k.lo:hi]
    return dst


def check_fold(k, dst, route):
    _exact(dst, k.dst, f"{route} grad fold (n {k.n}, {'overwrite' if k.overwrite else 'accumulate'}, offset {k.off})", "dst and its guards")


# =========================================================================================== host and defect checks (tests/test_host.py)
def _mse_cases():
    out = []
    for fam, rows in (("D", ROWS_D), ("N", ROWS_ODD), ("G", ROWS_ODD)):
        for b, t, p in rows:
            for dt in (BF16, F32):
                for div in (1, 2):
                    if b % div == 0:
                        out.append((fam, b, t, p, dt, div))
    return out


def _kl_cases():
    return [(fam, b, t, p, dt, masked) for fam, rows in (("D", ROWS_D_KL), ("N", ROWS_ODD), ("G", ROWS_ODD)) for b, t, p in rows
            for dt in (BF16, F32) for masked in (True, False)]


ADAM1_CASES = [(n, ema, acc, regime) for n in (N1, N2) for ema in (False, True) for acc in (False, True) for regime in ADAM_REGIMES]


def _name(dt):
    return "bf16" if dt == BF16 else "fp32"


def _host_checks():
    cs = [("mirrors", _mirrors_match_the_library)]
    cs += [(f"mse-{f}-B{b}-T{t}-P{p}-{_name(dt)}-div{d}", functools.partial(mse_case, f, b, t, p, dt, d)) for f, b, t, p, dt, d in _mse_cases()]
    cs += [(f"kl-{f}-B{b}-T{t}-P{p}-{_name(dt)}-{'mask' if mk else 'nomask'}", functools.partial(kl_case, f, b, t, p, dt, mk))
           for f, b, t, p, dt, mk in _kl_cases()]
    cs += [(f"tail-B{b}-T{t}-P{p}", functools.partial(tail_case, b, t, p)) for b, t, p in ROWS_TAIL]
    cs += [(f"sqnorm-n{n}-{'acc' if acc else 'plain'}", functools.partial(sq_case, n, acc)) for n in (N1, N2) for acc in (False, True)]
    cs += [(f"adam1-n{n}-ema{int(e)}-acc{int(a)}-{r}", functools.partial(adam1_case, n, e, a, r)) for n, e, a, r in ADAM1_CASES]
    cs += [("adam1-any-clip", _adam1_holds_for_any_clip), ("adam-generic", adamg_case)]
    cs += [(f"fold-{'ovw' if o else 'acc'}-off{off}", functools.partial(fold_case, N2, o, off)) for o, off in FOLD_FORMS]
    return cs


def _raises(fn, match):
    with pytest.raises(AssertionError, match=match):
        fn()


def _mse_defect(fam, b, t, p, dt, div, partials, defect, name):
    k = mse_case(fam, b, t, p, dt, div)
    if defect is None:
        return check_mse(k, cpu_mse(k, partials), "cpu")
    _raises(lambda: check_mse(k, cpu_mse(k, partials, defect), "cpu"), rf"\): {name}: ")


def _kl_defect(fam, b, t, p, dt, defect, name):
    k = kl_case(fam, b, t, p, dt, True)
    _raises(lambda: check_kl(k, cpu_kl(k, "joint", defect), "joint", "cpu"), rf"\): {name}: ")


def _sq_defect(defect, name):
    k = sq_case(N1, False)
    assert k.nparts == 1024 and k.n % 4 == 3
    _raises(lambda: check_sq(k, cpu_sq(k, defect), "cpu"), rf"\): {name}")


def _adam_defect(ema, acc):
    k = adam1_case(N1, ema, acc, "bite")
    _raises(lambda: check_adam1(k, cpu_adam1(k, "sweep-skipped"), "cpu"), r"\): p: \d+/\d+ ")
    stale = dict(cpu_adam1(k), m=cpu_adam1(k, "sweep-skipped")["m"])       # m alone: its relative bound sees a stale stripe too
    _raises(lambda: check_adam1(k, stale, "cpu"), r"\): m: \d+/\d+ ")


def _fold_defect(overwrite, off):
    k = fold_case(4099, overwrite, off)
    _raises(lambda: check_fold(k, cpu_fold(k, "one-past"), "cpu"), r"dst and its guards: 1/\d+ ")


def _defect_checks():
    out = []
    for dt in (BF16, F32):
        d_, n_ = ("D", 4, 5, 1024, dt), ("N", 4, 8, 625, dt)
        nm = _name(dt)
        for fam, key in (("D", d_), ("N", n_)):
            for partials in (False, True):
                out.append((f"mse-{fam}-{nm}-{'partials' if partials else 'folded'}-clean", functools.partial(_mse_defect, *key, 2, partials, None, None)))
            out.append((f"mse-{fam}-{nm}-chunk-dropped", functools.partial(_mse_defect, *key, 1, False, "chunk-dropped", "mse")))
            out.append((f"mse-{fam}-{nm}-chunk-doubled", functools.partial(_mse_defect, *key, 1, False, "chunk-doubled", "mse")))
            out.append((f"mse-{fam}-{nm}-tail-unread-folded", functools.partial(_mse_defect, *key, 1, False, "tail-unread", "mse")))
            out.append((f"mse-{fam}-{nm}-tail-unread-partials", functools.partial(_mse_defect, *key, 1, True, "tail-unread", "part2")))
            out.append((f"mse-{fam}-{nm}-video-index", functools.partial(_mse_defect, *key, 2, True, "video-index", "part2")))
            out.append((f"mse-{fam}-{nm}-len-zero", functools.partial(_mse_defect, *key, 1, False, "len-zero", "mse")))
            kkey = ("D", 4, 8, 1024, dt) if fam == "D" else key
            out.append((f"kl-{fam}-{nm}-chunk-dropped", functools.partial(_kl_defect, *kkey, "chunk-dropped", "kl")))
            out.append((f"kl-{fam}-{nm}-chunk-doubled", functools.partial(_kl_defect, *kkey, "chunk-doubled", "kl")))
            out.append((f"kl-{fam}-{nm}-len-zero", functools.partial(_kl_defect, *kkey, "len-zero", "kl")))
        out.append((f"mse-N-{nm}-straddle-mask", functools.partial(_mse_defect, *n_, 1, True, "straddle-mask", "part2")))
    out.append(("sqnorm-fold-256", functools.partial(_sq_defect, "fold-256", "gnorm_sq_out")))
    out.append(("sqnorm-tail-out", functools.partial(_sq_defect, "tail-out", "part")))
    out += [(f"adam1-ema{int(e)}-acc{int(a)}-sweep-skipped", functools.partial(_adam_defect, e, a)) for e, a in ((False, False), (True, True))]
    out += [(f"fold-{'ovw' if o else 'acc'}-off{off}-one-past", functools.partial(_fold_defect, o, off)) for o, off in FOLD_FORMS]
    return out


HOST_CHECKS = _host_checks()
DEFECT_CHECKS = _defect_checks()


# =========================================================================================== GPU runners
def _ops():
    from video_vae_amd import ops
    return ops


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _poison(dev, nbytes):
    """Fill the allocator's free blocks of an output's size with NaN bit patterns: the ops allocate their own outputs, and a block that a
    run before this one left holding the right values would otherwise let an element no kernel wrote pass.  Best effort, no proof."""
    blocks = [torch.full((nbytes,), 0xff, dtype=torch.uint8, device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    del blocks


def _put(x, dev, dtype, off):
    """x on the device in ``dtype``; off > 0: as a contiguous view that starts ``off`` elements into its storage (not 16-byte aligned)."""
    if not off:
        out = x.to(dev, dtype)
        assert out.data_ptr() % 16 == 0
        return out
    buf = torch.zeros(x.numel() + 8, dtype=dtype, device=dev)
    view = buf[off:off + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def run_mse(k, dev, partials, off=0):
    ops = _ops()
    _poison(dev, k.b * k.m * (2 if k.dtype == BF16 else 4))
    video, recon = _put(k.video, dev, k.dtype, off), _put(k.recon, dev, k.dtype, off).requires_grad_(True)
    o2, o1 = ops.masked_mse_mae(video, recon, k.mask.to(dev), k.div, partials)
    gm, ga = k.gm.float().to(dev), k.ga.float().to(dev)
    if partials:
        assert tuple(o2.shape) == tuple(o1.shape) == (k.b, k.chunks)
        gm, ga = gm[:, None].expand(k.b, k.chunks), ga[:, None].expand(k.b, k.chunks)
    (dr,) = torch.autograd.grad([o2, o1], [recon], [gm, ga])
    torch.cuda.synchronize()
    names = ("part2", "part1") if partials else ("mse", "mae")
    return {names[0]: o2.detach().cpu(), names[1]: o1.detach().cpu(), "drecon": dr.cpu()}


def run_kl(k, dev, form):
    ops = _ops()
    _poison(dev, k.b * k.m * (2 if k.dtype == BF16 else 4))
    mean, logvar = k.mean.to(dev, k.dtype).requires_grad_(True), k.logvar.to(dev, k.dtype).requires_grad_(True)
    mask = k.mask.to(dev) if k.masked else None
    res, outs, gos = {}, [], []
    if form == "joint":
        res["z"], res["kl"] = ops.reparameterise_kl(mean, logvar, k.eps.to(dev), mask)
    elif form == "z":
        res["z"] = ops.reparameterise(mean, logvar, k.eps.to(dev))
    else:
        res["kl"] = ops.kl_per_sample(mean, logvar, mask)
    if "z" in res:
        outs.append(res["z"]); gos.append(k.dz.to(dev))
    if "kl" in res:
        outs.append(res["kl"]); gos.append(k.gkl.float().to(dev))
    res["dmean"], res["dlogvar"] = torch.autograd.grad(outs, [mean, logvar], gos)
    torch.cuda.synchronize()
    return {name: x.detach().cpu() for name, x in res.items()}


def run_tail(k, dev):
    ops = _ops()
    recon = k.mse.recon.to(dev, BF16).requires_grad_(True)
    mean = k.mean.to(dev, BF16).requires_grad_(True)
    logvar = torch.zeros_like(mean).requires_grad_(True)
    sel = k.sel.to(dev).requires_grad_(True)
    mask = k.mask.to(dev)
    mse_ps, _ = ops.masked_mse_mae(k.mse.video.to(dev, BF16), recon, mask, 1, True)
    kl_ps = ops.kl_per_sample(mean, logvar, mask).unsqueeze(1)
    assert tuple(mse_ps.shape) == (k.b, 512) and ops.plain_loss_tail_ok(mse_ps, kl_ps, sel, mask)
    loss, aux = ops.plain_loss_tail(mse_ps, kl_ps, sel, mask, TAIL_HPARAMS)
    loss.backward(gradient=ops.unit_grad(loss))
    torch.cuda.synchronize()
    out = torch.stack([loss.detach(), *aux]).cpu()
    return {"out": out, "dsel": sel.grad.cpu(), "drecon": recon.grad.cpu(), "dmean": mean.grad.cpu(), "dlogvar": logvar.grad.cpu()}


def _ok(code, what):
    assert code == 0, f"{what} returned {code}"


def run_sq(k, dev):
    """vvae_sqnorm_partials (acc given or NULL), then an Adam step on scratch parameters for the fold of the partials into gnorm_sq_out."""
    lib = _lib()
    g, a = k.g.to(dev), k.a.to(dev) if k.acc else None
    part = torch.full((SQN_MAX_BLOCKS + GUARD,), -1.0, dtype=F64, device=dev)
    _ok(lib.vvae_sqnorm_partials(_vp(g), _vp(a), k.n, _vp(part), _stream()), "vvae_sqnorm_partials")
    p, m, v = (torch.zeros(k.n, device=dev) for _ in range(3))
    out = torch.full((1 + GUARD,), -1.0, dtype=F64, device=dev)
    nparts = lib.vvae_sqnorm_blocks(k.n)
    _ok(lib.vvae_adam_clip_step(_vp(p), _vp(g), None, _vp(m), _vp(v), None, k.n, _vp(part), nparts, _vp(out), 1.0, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1,
                                None, 0.0, _stream()), "vvae_adam_clip_step")
    torch.cuda.synchronize()
    assert nparts == k.nparts and bool((part[nparts:] == -1.0).all()) and bool((out[1:] == -1.0).all()), "a guard changed"
    assert torch.equal(g.cpu(), k.g) and (not k.acc or torch.equal(a.cpu(), k.a)), "an input changed"
    return {"part": part[:nparts].cpu(), "gnorm_sq": out[0].cpu()}


def run_adam1(k, dev):
    lib = _lib()
    n, nb = k.n, k.n + GUARD
    p, g, e = k.p0.to(dev), k.g.to(dev), k.e0.to(dev)
    a = k.a.to(dev) if k.acc else None
    m, v = torch.zeros(nb, device=dev), torch.zeros(nb, device=dev)
    sh = torch.zeros(nb, dtype=BF16, device=dev)
    part, out, nparts = None, None, 0
    if k.regime != "noclip":
        nparts = lib.vvae_sqnorm_blocks(n)
        part = torch.empty((nparts,), dtype=F64, device=dev)
        out = torch.full((1,), -1.0, dtype=F64, device=dev)
        _ok(lib.vvae_sqnorm_partials(_vp(g), _vp(a), n, _vp(part), _stream()), "vvae_sqnorm_partials")
    h = ADAM1
    common = (n, _vp(part), nparts, _vp(out), k.gscale, k.max_norm, h["lr"], h["b1"], h["b2"], h["eps"], 1)
    _ok(lib.vvae_adam_clip_step(_vp(p), _vp(g), _vp(a), _vp(m), _vp(v), _vp(sh), *common, _vp(e) if k.ema else None, h["decay"] if k.ema else 0.0,
                                _stream()), "vvae_adam_clip_step")
    torch.cuda.synchronize()
    assert torch.equal(g.cpu(), k.g) and (not k.acc or torch.equal(a.cpu(), k.a)), "an input changed"
    res = {"p": p.cpu(), "m": m.cpu(), "v": v.cpu(), "sh": sh.cpu()}
    if k.ema:
        res["e"] = e.cpu()
    else:
        assert torch.equal(e.cpu(), k.e0)
    if out is not None:
        res["gnorm_sq"] = out[0].cpu()
    return res


def run_adamg(k, dev):
    lib = _lib()
    n, nb = k.n, k.n + GUARD
    p, m, v = k.p0.to(dev), torch.zeros(nb, device=dev), torch.zeros(nb, device=dev)
    sh = torch.zeros(nb, dtype=BF16, device=dev)
    nparts = lib.vvae_sqnorm_blocks(n)
    part = torch.empty((nparts,), dtype=F64, device=dev)
    h = ADAMG
    for i, g in enumerate(k.gs):
        g = g.to(dev)
        _ok(lib.vvae_sqnorm_partials(_vp(g), None, n, _vp(part), _stream()), "vvae_sqnorm_partials")
        _ok(lib.vvae_adam_clip_step(_vp(p), _vp(g), None, _vp(m), _vp(v), _vp(sh), n, _vp(part), nparts, None, 1.0, h["max_norm"][i], h["lr"], h["b1"],
                                    h["b2"], h["eps"], i + 1, None, 0.0, _stream()), "vvae_adam_clip_step")
    torch.cuda.synchronize()
    assert torch.equal(sh[:n], p[:n].bfloat16()) and float(sh[n:].float().abs().max()) == 0.0
    assert float(m[n:].abs().max()) == 0.0 and float(v[n:].abs().max()) == 0.0
    return p.cpu()


# =========================================================================================== GPU tests
def test_mirrors_match_the_library():
    _mirrors_match_the_library()


@pytest.mark.parametrize("family,b,t,p,dtype,div", _mse_cases(), ids=[f"{f}-B{b}-T{t}-P{p}-{_name(dt)}-div{d}" for f, b, t, p, dt, d in _mse_cases()])
def test_masked_mse_mae_past_one_chunk(dev, family, b, t, p, dtype, div):
    """ops.masked_mse_mae forward and backward, folded and as partial columns, at a row of LOSS_TABLE."""
    k = mse_case(family, b, t, p, dtype, div)
    assert (k.epb, k.chunks, k.last) == _REGIMES[(b, t, p)] and (k.chunks > 1 or k.epb > 2048)
    if p == 625:
        vec = 8 if dtype == BF16 else 4
        assert k.m % vec == 0 and p % vec != 0, "no vector straddles a frame boundary"
    for partials in (False, True):
        check_mse(k, run_mse(k, dev, partials), "partials" if partials else "folded")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
def test_masked_mse_mae_unaligned_operands(dev, dtype):
    """video and recon one element into their storage: the VEC = 1 kernels.  Bit for bit the aligned run, and the Family D reference."""
    k = mse_case("D", 2, 5, 1024, dtype, 1)
    assert k.chunks == 3 and k.last < k.epb
    for partials in (False, True):
        aligned, shifted = run_mse(k, dev, partials), run_mse(k, dev, partials, off=1)
        check_mse(k, shifted, "unaligned")
        for name in aligned:
            assert torch.equal(aligned[name], shifted[name]), name


def test_fast_exp_of_zero_is_one(dev):
    """What Family D of the KL kernels rests on: mean = 0, eps = 1, logvar = 0 must give z = 1.0 exactly."""
    ops = _ops()
    shape = (2, 4, 1024)
    for dtype in (BF16, F32):
        z = ops.reparameterise(torch.zeros(shape, dtype=dtype, device=dev), torch.zeros(shape, dtype=dtype, device=dev), torch.ones(shape, device=dev))
        off = (z.double() - 1.0).abs().max().item()
        assert off == 0.0, f"exp(0) on the device is 1 + {off!r}: Family D of the KL kernels does not hold as written"


@pytest.mark.parametrize("family,b,t,p,dtype,masked", _kl_cases(),
                         ids=[f"{f}-B{b}-T{t}-P{p}-{_name(dt)}-{'mask' if mk else 'nomask'}" for f, b, t, p, dt, mk in _kl_cases()])
def test_reparam_kl_past_one_chunk(dev, family, b, t, p, dtype, masked):
    """ops.reparameterise_kl, ops.reparameterise and ops.kl_per_sample, forward and backward, at a row of LOSS_TABLE."""
    k = kl_case(family, b, t, p, dtype, masked)
    assert (k.epb, k.chunks, k.last) == _REGIMES[(b, t, p)] and k.chunks > 1
    for form in KL_FORMS:
        check_kl(k, run_kl(k, dev, form), form, "gpu")


@pytest.mark.parametrize("b,t,p", ROWS_TAIL)
def test_plain_loss_tail_on_512_partial_columns(dev, b, t, p):
    k = tail_case(b, t, p)
    assert k.mse.chunks == 512 and 512 + 1 > 16 and b <= 64             # the whole-workgroup tree of loss_tail_plain_kernel
    check_tail(k, run_tail(k, dev), "gpu")


@pytest.mark.parametrize("acc", [False, True], ids=["g", "g+acc"])
@pytest.mark.parametrize("n", [N1, N2])
def test_sqnorm_partials_past_one_sweep(dev, n, acc):
    k = sq_case(n, acc)
    assert k.nparts == SQN_MAX_BLOCKS and k.sweeps == (3 if n == N1 else 5) and (n // 4) % (k.nparts * 256) != 0 and n % 4 == 3
    assert _cdiv(k.nparts, 256) == 4                                     # terms per thread in the fold of adam_clip_kernel
    check_sq(k, run_sq(k, dev), "gpu")


@pytest.mark.parametrize("n,ema,acc,regime", ADAM1_CASES, ids=[f"n{n}-ema{int(e)}-acc{int(a)}-{r}" for n, e, a, r in ADAM1_CASES])
def test_adam_step_one_is_exact(dev, n, ema, acc, regime):
    k = adam1_case(n, ema, acc, regime)
    assert (k.blocks, k.sweeps, k.nparts) == ((2053, 4, 1024) if n == N1 else (STREAM_MAX_BLOCKS, 5, 1024)) and n % (k.blocks * 256) != 0
    check_adam1(k, run_adam1(k, dev), "gpu")


def test_adam_generic_steps(dev):
    k = adamg_case()
    check_adamg(k, run_adamg(k, dev), "gpu")


@pytest.mark.parametrize("overwrite,off", FOLD_FORMS, ids=[f"{'ovw' if o else 'acc'}-off{off}" for o, off in FOLD_FORMS])
def test_grad_fold_at_the_grid_cap(dev, overwrite, off):
    k = fold_case(N2, overwrite, off)
    assert k.blocks == STREAM_MAX_BLOCKS and sweeps(k.n // 4 if off == 0 else k.n, k.blocks) == (2 if off == 0 else 5)
    dst, src = k.dst0.to(dev), k.src.to(dev)
    assert (dst[k.lo:].data_ptr() % 16 == 0) == (off == 0) and (src[k.lo:].data_ptr() % 16 == 0) == (off == 0)
    _ok(_lib().vvae_grad_fold_f32(_vp(dst[k.lo:]), _vp(src[k.lo:]), k.n, int(overwrite), _stream()), "vvae_grad_fold_f32")
    torch.cuda.synchronize()
    assert torch.equal(src.cpu(), k.src), "src changed"
    check_fold(k, dst.cpu(), "gpu")


@pytest.mark.parametrize("off", [0, 1])
def test_swap_refresh_and_cast_at_the_grid_cap(dev, off):
    """vvae_swap_refresh_f32 (with and without the shadow) and vvae_cast_f32_to_bf16 on n2, bitwise against torch, guards untouched."""
    n, lo = N2, GUARD + off
    nb = n + 2 * GUARD + 1
    assert stream_blocks(n) == STREAM_MAX_BLOCKS and sweeps(n, STREAM_MAX_BLOCKS) == 5
    a0, b0 = rnd((nb,), _seed("swap", "a", off)), rnd((nb,), _seed("swap", "b", off))
    inside = (torch.arange(nb) >= lo) & (torch.arange(nb) < lo + n)
    bits = lambda x: x.cpu().view(torch.int16)
    for with_shadow in (True, False):
        a, b = a0.to(dev), b0.to(dev)
        h = torch.full((nb,), 7.0, dtype=BF16, device=dev)
        assert (a[lo:].data_ptr() % 16 == 0) == (off == 0)
        _ok(_lib().vvae_swap_refresh_f32(_vp(a[lo:]), _vp(b[lo:]), _vp(h[lo:]) if with_shadow else None, n, _stream()), "vvae_swap_refresh_f32")
        torch.cuda.synchronize()
        assert torch.equal(a.cpu(), torch.where(inside, b0, a0)) and torch.equal(b.cpu(), torch.where(inside, a0, b0))
        want_h = torch.where(inside, b0.bfloat16(), torch.full((nb,), 7.0, dtype=BF16)) if with_shadow else torch.full((nb,), 7.0, dtype=BF16)
        assert torch.equal(bits(h), bits(want_h))
    x, y = a0.to(dev), torch.full((nb,), 7.0, dtype=BF16, device=dev)
    _ok(_lib().vvae_cast_f32_to_bf16(_vp(x[lo:]), _vp(y[lo:]), n, _stream()), "vvae_cast_f32_to_bf16")
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), a0)
    assert torch.equal(bits(y), bits(torch.where(inside, a0.bfloat16(), torch.full((nb,), 7.0, dtype=BF16))))


def test_optimizer_tail_bit_for_bit_with_the_parent(dev):
    """Every member of tests/golden/optim_parent_bits.json (make_optim_parent_bits.py: p, m, v, the bf16 shadow, the average, the fp64
    partials and gnorm_sq after each of three consecutive updates, all four (EMA, ACC) variants, the clip biting and not, at n = 4099 and
    N1; the fold and the swap at n = 4099, aligned and one element off), recorded on the GPU from the five-entry ABI before the norm and
    Adam entries were merged: same dtype, same shape, same bytes."""
    import importlib.util
    import json
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_optim_parent_bits", os.path.join(golden, "make_optim_parent_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.LENGTHS == (4099, N1) and stream_blocks(N1) > 1 and sweeps(N1, stream_blocks(N1)) > 1 and sweeps(N1 // 4, sqnorm_blocks(N1)) > 1
    got = mod.record(_lib(), dev)
    with open(os.path.join(golden, "optim_parent_bits.json")) as fh:
        want = json.load(fh)
    assert sorted(got) == sorted(want) and len(want) == 2 * 4 * 2 * 3 * 6 + 2 * 2 * 2 * 3 + 4 + 6, (len(got), len(want), sorted(set(got) ^ set(want))[:8])
    bad = [f"{m}: got {got[m]}, recorded {want[m]}" for m in sorted(want) if got[m] != want[m]]
    assert not bad, f"{len(bad)} of {len(want)} members differ from the parent's bits: " + "; ".join(bad[:4])
