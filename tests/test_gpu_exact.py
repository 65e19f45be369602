"""Exact-arithmetic parity of the matrix-core kernels: bit for bit against a CPU reference, at small AND at production extents.

Every kernel under test is a sum of products.  Fed small integers (activations and output gradients in {-2 ... 2}, weights in
{-1, 0, 1} thinned to about 432 non-zero terms per dot product, biases in {-3 ... 3}) every product is an integer and every partial sum
an integer below 2^24, so fp32 addition is exact and therefore associative: ANY correct kernel -- whatever its tiling, summation order,
split-K, slab fold or epilogue placement -- must return the bits of a high-precision CPU reference, and a wrong index or a dropped term
cannot hide under a tolerance.  The tolerance is zero and no output is exempted.

The references are plain torch on the CPU (F.conv3d / matmul on the integer data, fp64; at the production extents fp32, which is
itself exact under the same condition -- the host test checks fp32 == fp64 on the small sets).  Each reference is validated by
util.assert_representable BEFORE a GPU result is looked at; the same builders and validations run without a GPU in
tests/test_host.py (HOST_CHECKS below).

Left out on purpose: the * silu'(res) epilogue (EPI_MUL_DSILU) and silu(h) itself -- their factor goes through an approximate
reciprocal, which is not integer arithmetic (not tried on hardware with res = 0); silu(h) keeps its existing tolerance here, the saved
pre-activation h is exact.
"""
import contextlib
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from test_gpu_ops import DEEP_CASES, FAST_CASES, ROLL_CASES
from util import assert_exact, assert_representable, ints

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
TERMS = 432.0                # non-zero weight terms per dot product: max |y| stays near 100, far inside bf16's exact integers (256)


def _ops():
    from video_vae_amd import ops
    return ops


def density(k):
    return min(1.0, TERMS / k)


def _to(device, *ts):
    """References of the large cases are validated and compared where the result lives (``device``); None: they stay on the CPU."""
    return ts if device is None else tuple(t.to(device) for t in ts)


def _validate(case):
    """assert_representable on every reference of a built case."""
    for name, ref, dtype, bound in case.refs:
        try:
            assert_representable(ref, dtype, bound)
        except AssertionError as e:
            raise AssertionError(f"{case.name} / {name}: {e}") from None
    return case


# =========================================================================================== CPU: operands and references
def conv_refs(x, k, b, gy, dtype=F64):
    """SAME stride-1 NDHWC cross-correlation and its three gradients on the CPU: -> y (+ bias), dx, dw, db."""
    kt, kh, kw = k.shape[:3]
    xr = x.to(dtype).requires_grad_(True)
    kr = k.to(dtype).requires_grad_(True)
    y = F.conv3d(xr.permute(0, 4, 1, 2, 3), kr.permute(4, 3, 0, 1, 2), padding=(kt // 2, kh // 2, kw // 2)).permute(0, 2, 3, 4, 1)
    y.backward(gy.to(dtype))
    y = y.detach()
    if b is not None:
        y = y + b.to(dtype)
    return y, xr.grad, kr.grad, gy.to(dtype).sum((0, 1, 2, 3))


def _conv_seed(ci, co, kh, dims):
    n, t, h, w = dims
    return (ci * 131 + co * 17 + kh * 7 + n * 5 + t * 3 + h * 2 + w) % 100003


def conv_case(ci, co, kt, kh, kw, dims, gy_hi=2, dtype=F64, out_dtype=BF, device=None):
    """Integer operands of one conv layer + exact references.  Weight density from the longer of the forward / input-gradient dots."""
    n, t, h, w = dims
    s = _conv_seed(ci, co, kh, dims)
    taps = kt * kh * kw
    x = ints((n, t, h, w, ci), s + 1, -2, 2)
    k = ints((kt, kh, kw, ci, co), s + 2, -1, 1, density(taps * max(ci, co)))
    b = ints((co,), s + 3, -3, 3)
    gy = ints((n, t, h, w, co), s + 4, -gy_hi, gy_hi)
    y, dx, dw, db = _to(device, *conv_refs(x, k, b, gy, dtype))
    vox = n * t * h * w
    c = types.SimpleNamespace(name=f"conv {ci}->{co} k{kt}{kh}{kw} {dims}", x=x, k=k, b=b, gy=gy, y=y, dx=dx, dw=dw, db=db)
    c.refs = [("y", y, out_dtype, taps * ci * 2 + 3), ("dx", dx, out_dtype, taps * co * gy_hi),
              ("dw", dw, F32, vox * 2 * gy_hi), ("db", db, F32, vox * gy_hi)]
    return c


@functools.lru_cache(maxsize=None)
def small_conv_case(case):
    ci, co, kt, kh, kw, dims = case
    return _validate(conv_case(ci, co, kt, kh, kw, dims))


def _dedupe(seq):
    out = []
    for c in seq:
        if c not in out:
            out.append(c)
    return out


# every layer shape of the UNet (FAST_CASES) + the ragged and degenerate extents of the rolling and deep kernel tests
SMALL_CONV_CASES = _dedupe(list(FAST_CASES) + [(ci, co, 3, kh, kh, d) for ci, co, kh, d in ROLL_CASES]
                           + [(ci, co, 3, 3, 3, d) for ci, co, d in DEEP_CASES])

# production extents: B = 4 x 16 frames; resolution per level read off video_vae_amd/unet.py and model.py (base 16 features, 3 levels,
# 256^2 input: 16 @ 256^2, 32 @ 128^2, 64 @ 64^2, bottleneck 128 @ 32^2)
FULL_CONV_CASES = [(16, 16, 3, 256), (32, 16, 3, 256), (16, 16, 7, 256), (32, 32, 3, 128), (64, 32, 3, 128), (64, 64, 3, 64), (128, 128, 3, 32)]


def full_conv_case(ci, co, kh, hw, device=None):
    """fp32 references (exact: every partial sum is an integer below 2^24 -- checked); output gradients from {-1, 0, 1} so that the
    weight gradient's hard bound 2 V stays below 2^24 at V = 4 x 16 x 256^2."""
    return _validate(conv_case(ci, co, 3, kh, kh, (4, 16, hw, hw), gy_hi=1, dtype=F32, device=device))


PITCH_CASES = [(16, 16, 3, (2, 5, 20, 24)), (64, 64, 3, (1, 3, 9, 17)), (32, 16, 3, (1, 2, 3, 50)), (16, 16, 7, (1, 3, 20, 24))]

CAT2_CASES = [(16, 16, 16, (2, 5, 20, 36)), (16, 16, 32, (1, 4, 16, 32)), (16, 16, 16, (1, 3, 9, 21))]

GN_CASES = [(16, 16, (2, 5, 20, 24)), (16, 32, (1, 4, 9, 33)), (32, 16, (2, 3, 17, 16)), (32, 32, (1, 6, 18, 30)), (64, 32, (1, 2, 8, 16)),
            (32, 64, (2, 3, 12, 20)), (64, 64, (1, 5, 9, 17)), (64, 128, (1, 2, 8, 16)), (128, 128, (2, 3, 6, 16)), (128, 64, (1, 4, 10, 18))]


def gn_refs(case, groups):
    """Per (sample, group) sums and sums of squares of the integer conv output.  Every workgroup's partial is a sub-sum of
    non-negative squares, so the whole sum below 2^24 bounds each of them."""
    y = case.y.double()
    n, co = y.shape[0], y.shape[-1]
    yr = y.reshape(n, -1, groups, co // groups)
    s, ss = yr.sum((1, 3)), (yr * yr).sum((1, 3))
    return [("gn sums", s, F32, float(yr.abs().sum((1, 3)).max())), ("gn sums of squares", ss, F32, float(ss.max()))]


def _with_gn(c, name):
    g = types.SimpleNamespace(name=name, conv=c, groups=min(8, c.y.shape[-1]))
    g.refs = gn_refs(c, g.groups)
    g.sums, g.sumsq = g.refs[0][1], g.refs[1][1]
    return _validate(g)


def gn_case(ci, co, dims):
    c = small_conv_case((ci, co, 3, 3, 3, dims))
    return _with_gn(c, c.name + " GroupNorm partials")


def cat2_case(ca, cb, co, dims):
    c = small_conv_case((ca + cb, co, 3, 3, 3, dims))
    return _with_gn(c, c.name + " as two tensors")


MIXER_DIMS, MIXER_C, MIXER_PAD = (1, 5, 40, 52), 12, 4


@functools.lru_cache(maxsize=None)
def mixer_case():
    """3x7x7 patch mixer, 12 real channels zero-padded to 16: the reference is the conv over the 12 real channels."""
    c, pad, dims = MIXER_C, MIXER_PAD, MIXER_DIMS
    n, t, h, w = dims
    x12 = ints((n, t, h, w, c), 701, -2, 2)
    k12 = ints((3, 7, 7, c, c), 702, -1, 1, density(147 * c))
    b12 = ints((c,), 703, -3, 3)
    gy12 = ints((n, t, h, w, c), 704, -2, 2)
    y, dx, dw, db = conv_refs(x12, k12, b12, gy12)
    m = types.SimpleNamespace(name="patch mixer 12 of 16 channels")
    m.x, m.gy, m.b = F.pad(x12, (0, pad)), F.pad(gy12, (0, pad)), F.pad(b12, (0, pad))
    m.k = F.pad(k12, (0, pad, 0, pad))
    m.y, m.dx, m.db = F.pad(y, (0, pad)), F.pad(dx, (0, pad)), F.pad(db, (0, pad))
    m.dw = F.pad(dw, (0, pad, 0, pad))
    vox = n * t * h * w
    m.refs = [("y", m.y, BF, 147 * c * 2 + 3), ("dx", m.dx, BF, 147 * c * 2), ("dw", m.dw, F32, vox * 4), ("db", m.db, F32, vox * 2)]
    return _validate(m)


POINTWISE_SHAPES = [(1, 1, 1, 1), (1, 3, 9, 11), (2, 3, 9, 11), (1, 4, 64, 80)]        # V = 1, odd, even, many workgroups


@functools.lru_cache(maxsize=None)
def pointwise_case(cin, shape, dtype):
    n, t, h, w = shape
    s = cin * 1000 + n * t * h * w
    x = ints((n, t, h, w, cin), s + 1, -2, 2)
    k = ints((1, 1, 1, cin, 3), s + 2, -1, 1)
    b = ints((3,), s + 3, -3, 3)
    gy = ints((n, t, h, w, 3), s + 4, -2, 2)
    addend = ints((n, t, h, w, 3), s + 5, -2, 2)
    dother = ints((n, t, h, w, cin), s + 6, -2, 2)
    xd, kd, gd = x.double(), k.double()[0, 0, 0], gy.double()
    p = types.SimpleNamespace(name=f"pointwise {cin}->3 {shape} {dtype}", x=x, k=k, b=b, gy=gy, addend=addend, dother=dother)
    p.y = xd @ kd + b.double()
    p.y_add = p.y + addend.double()
    p.dx = gd @ kd.t()
    p.dx_add = p.dx + dother.double()
    p.dw = (xd.reshape(-1, cin).t() @ gd.reshape(-1, 3)).reshape(1, 1, 1, cin, 3)
    p.db = gd.sum((0, 1, 2, 3))
    vox = n * t * h * w
    p.refs = [("y", p.y, dtype, cin * 2 + 3), ("y + addend", p.y_add, dtype, cin * 2 + 5), ("dx", p.dx, dtype, 6), ("dx + other", p.dx_add, dtype, 8),
              ("dw", p.dw, F32, vox * 4), ("db", p.db, F32, vox * 2)]
    return _validate(p)


def convt_refs(x, k, b, gy, dtype=F64):
    """ConvTranspose (1,2,2) / stride (1,2,2) restated: out[2i + d] = x[i] . K[1 - d] per spatial axis, and its gradients."""
    x, k, gy = x.to(dtype), k.to(dtype), gy.to(dtype)
    n, t, h, w, ci = x.shape
    co = k.shape[-1]
    y = torch.zeros((n, t, 2 * h, 2 * w, co), dtype=dtype)
    dx = torch.zeros_like(x)
    dw = torch.zeros_like(k)
    for a in (0, 1):
        for c in (0, 1):
            kk = k[0, 1 - a, 1 - c]
            g = gy[:, :, a::2, c::2]
            y[:, :, a::2, c::2] = x @ kk
            dx += g @ kk.t()
            dw[0, 1 - a, 1 - c] = x.reshape(-1, ci).t() @ g.reshape(-1, co)
    return y + b.to(dtype), dx, dw, gy.sum((0, 1, 2, 3))


CONVT_SMALL = [(32, 16, (2, 3, 6, 10)), (64, 32, (1, 2, 5, 7)), (128, 64, (1, 2, 4, 8)), (32, 16, (1, 5, 32, 40)), (128, 64, (2, 4, 16, 16)),
               (64, 32, (1, 1, 1, 1))]
# each up-conv at its real input resolution (B = 4 x 16 frames): 128 -> 64 reads 32^2, 64 -> 32 reads 64^2, 32 -> 16 reads 128^2
CONVT_FULL = [(128, 64, (4, 16, 32, 32)), (64, 32, (4, 16, 64, 64)), (32, 16, (4, 16, 128, 128))]


def convt_case(ci, co, dims, gy_hi=2, dtype=F64, device=None):
    n, t, h, w = dims
    s = _conv_seed(ci, co, 2, dims)
    x = ints((n, t, h, w, ci), s + 1, -2, 2)
    k = ints((1, 2, 2, ci, co), s + 2, -1, 1)
    b = ints((co,), s + 3, -3, 3)
    gy = ints((n, t, 2 * h, 2 * w, co), s + 4, -gy_hi, gy_hi)
    y, dx, dw, db = _to(device, *convt_refs(x, k, b, gy, dtype))
    vox = n * t * h * w
    c = types.SimpleNamespace(name=f"convT {ci}->{co} {dims}", x=x, k=k, b=b, gy=gy, y=y, dx=dx, dw=dw, db=db)
    c.refs = [("y", y, BF, ci * 2 + 3), ("dx", dx, BF, 4 * co * gy_hi), ("dw", dw, F32, vox * 2 * gy_hi), ("db", db, F32, 4 * vox * gy_hi)]
    return _validate(c)


NT_SHAPES = [(256, 192, 64), (512, 768, 512), (256, 128, 128), (1024, 1536, 768), (256, 512, 192), (16384, 1536, 768), (16384, 2304, 256),
             (16384, 1024, 256), (8192, 3072, 128), (16384, 1536, 192)]                                  # test_gemm_nt_linear_forms
PP_SHAPES = [(16384, 1536, 768), (16384, 768, 1536), (16384, 512, 768), (16384, 768, 512), (512, 384, 128), (256, 1536, 192), (1024, 2048, 256),
             (768, 192, 832), (16384, 1536, 192)]                                                      # test_gemm_pp_matches_gemm_nt_bitwise_and_fp32
GEMM_SHAPES = _dedupe(NT_SHAPES + PP_SHAPES)


def gemm_nt_case(m, n, k, dtype=None, device=None):
    """A (pitched rows) in {-2 ... 2}, B^T in {-1, 0, 1} at ~432 terms per dot, bias in {-3 ... 3}, residual (pitched rows) in {-2 ... 2}.
    Reference in fp64; the 8192- and 16384-row products in fp32 (exact under the checked bound, and half the CPU time)."""
    dtype = dtype if dtype is not None else (F32 if m >= 8192 else F64)
    s = (m * 7 + n * 3 + k) % 100003
    g = types.SimpleNamespace(name=f"gemm_nt {m}x{n} K{k}")
    g.a_full = ints((m, k + 64), s + 1, -2, 2)
    g.b = ints((n, k), s + 2, -1, 1, density(k))
    g.bias = ints((n,), s + 3, -3, 3)
    g.res_full = ints((m, n + 64), s + 4, -2, 2)
    g.h0, bias, res = _to(device, g.a_full[:, :k].to(dtype) @ g.b.to(dtype).t(), g.bias.to(dtype), g.res_full[:, :n].to(dtype))
    g.h = g.h0 + bias
    g.hr = g.h + res
    g.refs = [("a b^T", g.h0, BF, 2 * k), ("+ bias", g.h, BF, 2 * k + 3), ("+ bias + res", g.hr, BF, 2 * k + 5)]
    return _validate(g)


TN_SHAPES = [(128, 128, 64), (256, 384, 1000), (768, 1536, 4096), (512, 128, 33), (256, 256, 32), (512, 768, 2080), (768, 512, 16384),
             (256, 512, 96), (768, 96, 16384), (96, 768, 16384), (96, 96, 500), (8, 200, 77), (136, 24, 64)]    # test_gemm_tn_weight_gradient
GROUPED_K = 1024
GROUPED_SHAPES = [(768, 1536), (512, 768), (1536, 768), (256, 256), (768, 768), (1536, 1536), (512, 512), (768, 512), (256, 1536), (1536, 256),
                  (1536, 1536)]                                                                         # test_gemm_tn_grouped_deferred


def gemm_tn_case(m, n, k, seed=0):
    """Dense operands in {-2 ... 2}: fp32 outputs are exact up to 2^24 and the hard bound is 4 K."""
    s = (m * 7 + n * 3 + k + seed) % 100003
    g = types.SimpleNamespace(name=f"gemm_tn {m}x{n} K{k}")
    g.a = ints((k, m), s + 1, -2, 2)
    g.b = ints((k, n), s + 2, -2, 2)
    g.c = g.a.double().t() @ g.b.double()
    g.db = g.b.double().sum(0)
    g.refs = [("dW", g.c, F32, 4 * k), ("db", g.db, F32, 2 * k)]
    return _validate(g)


LINRES_SHAPES = [(16384, 512, 768), (4096, 1536, 768), (256, 64, 64)]                                   # test_linear_residual_library_product


def linres_case(m, k, n, device=None):
    s = (m + k * 5 + n * 11) % 100003
    g = types.SimpleNamespace(name=f"linear_residual {m}x{n} K{k}")
    g.x_full = ints((m, k + 8), s + 1, -2, 2)
    g.w = ints((k, n), s + 2, -1, 1, density(k))
    g.b = ints((n,), s + 3, -3, 3)
    g.r_full = ints((m, n + 8), s + 4, -2, 2)
    g.plain, res = _to(device, g.x_full[:, :k].double() @ g.w.double() + g.b.double(), g.r_full[:, :n].double())
    g.y = g.plain + res
    g.refs = [("x W + b", g.plain, BF, 2 * k + 3), ("x W + b + res", g.y, BF, 2 * k + 5)]
    return _validate(g)


SUM_ROWS_SHAPES = [(1024, 2, 768), (8192, 128), (1000, 2, 64), (7, 12), (1, 4), (4096, 1536)]           # test_sum_rows
COLSUM_CASES = [(16384, 768, BF), (16384, 96, BF), (1000, 8, BF), (777, 20, F32), (4096, 2048, BF), (300, 7, BF), (64, 1, BF)]
FOLD_CASES = [(384, 1536, 768), (4096, 128, 64), (7, 12, 12)]                                           # rows, cols, n0 (the second: two-stage fold)


def colsum_ref(shape, seed, hi):
    g = types.SimpleNamespace(name=f"column sums {shape}")
    g.x = ints(shape, seed, -hi, hi)
    g.sum = g.x.double().sum(0)
    g.refs = [("column sums", g.sum, F32, shape[0] * hi)]
    return _validate(g)


def _host_checks():
    """(id, callable) for every parametrised input set of this module: builds the operands and the reference on the CPU and runs
    assert_representable on it.  tests/test_host.py runs them all without a GPU."""
    def small_conv(case):
        c = small_conv_case(case)
        y32, dx32, dw32, db32 = conv_refs(c.x, c.k, c.b, c.gy, F32)          # the fp32 CPU conv used at full size is exact, too
        for a, b_ in ((y32, c.y), (dx32, c.dx), (dw32, c.dw), (db32, c.db)):
            assert torch.equal(a.double(), b_)
    ch = [(f"conv-small-{c}", functools.partial(small_conv, c)) for c in SMALL_CONV_CASES]
    ch += [(f"conv-full-{c}", functools.partial(full_conv_case, *c)) for c in FULL_CONV_CASES]
    ch += [(f"conv-pitch-{c}", functools.partial(small_conv_case, (c[0], c[1], 3, c[2], c[2], c[3]))) for c in PITCH_CASES]
    ch += [(f"conv-cat2-{c}", functools.partial(cat2_case, *c)) for c in CAT2_CASES]
    ch += [(f"conv-gn-{c}", functools.partial(gn_case, *c)) for c in GN_CASES]
    ch += [("conv-mixer", mixer_case)]
    ch += [(f"pointwise-{cin}-{s}-{dt}", functools.partial(pointwise_case, cin, s, dt)) for cin in (16, 12) for s in POINTWISE_SHAPES for dt in (F32, BF)]
    ch += [(f"convt-{c}", functools.partial(convt_case, *c)) for c in CONVT_SMALL]
    ch += [(f"convt-full-{c}", functools.partial(convt_case, *c, gy_hi=1, dtype=F32)) for c in CONVT_FULL]
    def gemm_nt(c):
        g = gemm_nt_case(*c)
        if c[0] <= 1024:                                                     # the fp32 CPU product used for the tall shapes is exact, too
            assert torch.equal(gemm_nt_case(*c, dtype=F32).hr.double(), g.hr.double())
    ch += [(f"gemm-nt-{c}", functools.partial(gemm_nt, c)) for c in GEMM_SHAPES]
    ch += [(f"gemm-tn-{c}", functools.partial(gemm_tn_case, *c)) for c in TN_SHAPES]
    ch += [(f"gemm-tn-grouped-{i}-{c}", functools.partial(gemm_tn_case, c[0], c[1], GROUPED_K, i)) for i, c in enumerate(GROUPED_SHAPES)]
    ch += [(f"linear-residual-{c}", functools.partial(linres_case, *c)) for c in LINRES_SHAPES]
    ch += [(f"sum-rows-{c}", functools.partial(colsum_ref, c, 90, 3)) for c in SUM_ROWS_SHAPES]
    ch += [(f"colsum-{v}-{c}", functools.partial(colsum_ref, (v, c), v + c, 2)) for v, c, _ in COLSUM_CASES]
    ch += [(f"fold-{c}", functools.partial(colsum_ref, c[:2], 91, 3)) for c in FOLD_CASES]
    return ch


HOST_CHECKS = _host_checks()


# =========================================================================================== GPU tests
@contextlib.contextmanager
def kernel_form(roll=(1, 0), deep=1, generic=False, cob16=0):
    """Select a kernel form through the library's test hooks; the defaults are restored whatever happens."""
    from video_vae_amd._lib import lib
    ops = _ops()
    try:
        lib().vvae_conv3d_roll_config(*roll)
        lib().vvae_conv3d_deep_config(deep)
        lib().vvae_conv3d_wgrad_config(cob16, 0)
        if generic:
            ops.force_generic_conv(True)
        yield
    finally:
        ops.force_generic_conv(False)
        lib().vvae_conv3d_roll_config(1, 0)
        lib().vvae_conv3d_deep_config(1)
        lib().vvae_conv3d_wgrad_config(0, 0)


# form -> (hook settings, which of forward / dgrad / wgrad the hooks can change)
CONV_FORMS = {
    "default": (dict(), "fdw"),
    "per-frame": (dict(roll=(0, 0), deep=0), "fd"),
    "tchunk1": (dict(roll=(1, 1)), "fd"),
    "tchunk3": (dict(roll=(1, 3)), "fd"),
    "tchunk16": (dict(roll=(1, 16)), "fd"),
    "deep-off": (dict(deep=0), "fd"),
    "generic": (dict(generic=True), "fdw"),
    "wgrad-cob16": (dict(cob16=1), "w"),
}


def _run_conv(ops, c, dev, which, what):
    xg, kg, bg, gyg = c.x.to(dev, BF), c.k.to(dev), c.b.to(dev), c.gy.to(dev, BF)
    if "f" in which:
        assert_exact(ops.conv3d_fwd_raw(xg, kg, bg), c.y, f"{what}: y")
    if "d" in which:
        assert_exact(ops.conv3d_dgrad_raw(gyg, kg), c.dx, f"{what}: dx")
    if "w" in which:
        dw, db = ops.conv3d_wgrad_raw(xg, gyg, tuple(c.k.shape))
        assert_exact(dw, c.dw, f"{what}: dw")
        assert_exact(db, c.db, f"{what}: db")


@pytest.mark.parametrize("form", list(CONV_FORMS))
@pytest.mark.parametrize("case", SMALL_CONV_CASES)
def test_conv3d_kernel_forms_exact(dev, case, form):
    """Forward, input gradient, weight + bias gradient of every UNet layer shape (bf16 storage) on every kernel form the hooks reach
    -- per-frame, rolling with 0 / 1 / 3 / 16 frames per workgroup, deep on / off, the generic fp32-matrix-core path, 16 output
    channels per weight-gradient workgroup -- at ragged and degenerate extents (one frame, one row, 1 x 1, widths that are no tile
    multiple, N > 1): each equals the CPU fp64 reference bit for bit, hence they equal each other with no allowance."""
    ops = _ops()
    c = small_conv_case(case)
    hooks, which = CONV_FORMS[form]
    with kernel_form(**hooks):
        _run_conv(ops, c, dev, which, f"{c.name} [{form}]")


@pytest.mark.parametrize("ci,co,kh,hw", FULL_CONV_CASES)
def test_conv3d_production_extent_exact(dev, ci, co, kh, hw):
    """B = 4 x 16 frames at each level's real resolution, WHOLE tensors (no crops): the forward output, the input gradient and the
    weight / bias gradients against the CPU reference (fp32 on integer data: exact, see the module docstring), compared on the device.
    Seams between many tiles per axis, the persistent-grid tail of the weight-gradient slabs and large offsets exist only here."""
    ops = _ops()
    c = full_conv_case(ci, co, kh, hw, device=dev)
    try:
        _run_conv(ops, c, dev, "fdw", c.name)
    finally:
        del c
        torch.cuda.empty_cache()


@pytest.mark.parametrize("ci,co,kh,dims", PITCH_CASES)
def test_conv3d_channel_pitch_operands_exact(dev, ci, co, kh, dims):
    """Input and output as channel slices of wider buffers (row pitch > C): exact results inside the slice, the sentinel outside it
    untouched; the weight gradient from two pitched operands."""
    ops = _ops()
    c = small_conv_case((ci, co, 3, kh, kh, dims))
    n, t, h, w = dims
    sentinel = 77.0
    kg, bg = c.k.to(dev), c.b.to(dev)

    def wide(src, ch):                                        # src in channels [ch, 2 ch) of a 3 ch-wide buffer of other integers
        buf = ints((n, t, h, w, 3 * ch), 5, -2, 2).to(dev, BF)
        buf[..., ch:2 * ch] = src.to(dev, BF)
        return buf[..., ch:2 * ch]
    xs, gys = wide(c.x, ci), wide(c.gy, co)
    assert xs.stride(-2) == 3 * ci and not xs.is_contiguous()
    for name, fn, ref, cout in (("y", lambda o: ops.conv3d_fwd_raw(xs, kg, bg, out=o), c.y, co),
                                ("dx", lambda o: ops.conv3d_dgrad_raw(gys, kg, out=o), c.dx, ci)):
        out = torch.full((n, t, h, w, cout + 32), sentinel, dtype=BF, device=dev)
        fn(out[..., 16:16 + cout])
        assert_exact(out[..., 16:16 + cout], ref, f"{c.name}: pitched {name}")
        assert bool((out[..., :16] == sentinel).all()) and bool((out[..., 16 + cout:] == sentinel).all()), f"{name}: wrote outside its channel slice"
    dw, db = ops.conv3d_wgrad_raw(xs, gys, tuple(c.k.shape))
    assert_exact(dw, c.dw, f"{c.name}: pitched dw")
    assert_exact(db, c.db, f"{c.name}: pitched db")


def _gn_check(part, g, what):
    tot = part.double().sum(1)
    assert_exact(tot[..., 0], g.sums, f"{what}: group sums")
    assert_exact(tot[..., 1], g.sumsq, f"{what}: group sums of squares")


@pytest.mark.parametrize("ca,cb,co,dims", CAT2_CASES)
def test_conv3d_two_tensor_level_exact(dev, ca, cb, co, dims):
    """The decoder level whose input is held as two tensors: forward (with its GroupNorm partials), both input gradients, weight and
    bias gradients against the CPU conv of the concatenation; a pitched first operand too."""
    ops = _ops()
    g = cat2_case(ca, cb, co, dims)
    c = g.conv
    xa, xb = c.x[..., :ca].contiguous().to(dev, BF), c.x[..., ca:].contiguous().to(dev, BF)
    kg, bg, gyg = c.k.to(dev), c.b.to(dev), c.gy.to(dev, BF)
    assert ops.conv3d_cat2_ok(xa, xb, kg)
    assert_exact(ops.conv3d_cat2_fwd_raw(xa, xb, kg, bg), c.y, f"{g.name}: y")
    nblk = ops.conv3d_gn_blocks(torch.cat([xa, xb], -1), kg, g.groups)
    assert nblk > 0
    y, part = ops.conv3d_cat2_fwd_raw(xa, xb, kg, bg, g.groups, nblk)
    assert_exact(y, c.y, f"{g.name}: y (with partials)")
    _gn_check(part, g, g.name)
    dxa, dxb = ops.conv3d_cat2_dgrad_raw(gyg, kg, ca)
    assert_exact(dxa, c.dx[..., :ca], f"{g.name}: dxa")
    assert_exact(dxb, c.dx[..., ca:], f"{g.name}: dxb")
    dw, db = ops.conv3d_cat2_wgrad_raw(xa, xb, gyg, tuple(c.k.shape))
    assert_exact(dw, c.dw, f"{g.name}: dw")
    assert_exact(db, c.db, f"{g.name}: db")
    wide = torch.full((*dims, ca + 8), 2.0, dtype=BF, device=dev)
    wide[..., :ca] = xa
    assert_exact(ops.conv3d_cat2_fwd_raw(wide[..., :ca], xb, kg, bg), c.y, f"{g.name}: y, pitched first operand")


@pytest.mark.parametrize("ci,co,dims", GN_CASES)
def test_conv3d_gn_partials_exact(dev, ci, co, dims):
    """GroupNorm partial sums from the conv epilogue (rolling and deep kernels): the per-(sample, group) sums and sums of squares,
    folded in fp64, against the fp64 sums of the integer output.  The extents keep every sum of squares below 2^24 (checked on the
    reference), so both columns are tested on every shape."""
    ops = _ops()
    g = gn_case(ci, co, dims)
    c = g.conv
    xg, kg, bg = c.x.to(dev, BF), c.k.to(dev), c.b.to(dev)
    nblk = ops.conv3d_gn_blocks(xg, kg, g.groups)
    assert nblk > 0
    y, part = ops.conv3d_fwd_gn_raw(xg, kg, bg, g.groups, nblk)
    assert_exact(y, c.y, f"{g.name}: y")
    _gn_check(part, g, g.name)


def test_patch_mixer_real_channels_exact(dev):
    """The 3x7x7 mixer on 16-channel voxels of which 12 are real: told the real count (k_real) or not, packed per call or prepacked,
    forward and input gradient equal the fp64 conv over the 12 real channels and the padded channels come out exactly zero; likewise
    the weight and bias gradients of the padded launch."""
    ops = _ops()
    m = mixer_case()
    c = MIXER_C
    xg, kg, bg, gyg = m.x.to(dev, BF), m.k.to(dev), m.b.to(dev), m.gy.to(dev, BF)
    pack = ops.conv3d_prepack([kg], [(c, c)])[0]
    assert pack is not None
    for name, kw_f, kw_d in (("padded product", dict(), dict()), ("k_real", dict(k_real=c), dict(k_real=c)),
                             ("k_real, prepacked", dict(k_real=c, packed=pack.fwd), dict(k_real=c, packed=pack.dgrad))):
        y = ops.conv3d_fwd_raw(xg, kg, bg, **kw_f)
        dx = ops.conv3d_dgrad_raw(gyg, kg, **kw_d)
        assert_exact(y, m.y, f"mixer y [{name}]")
        assert_exact(dx, m.dx, f"mixer dx [{name}]")
        assert float(y[..., c:].float().abs().max()) == 0 and float(dx[..., c:].float().abs().max()) == 0
    with kernel_form(roll=(0, 0)):                             # the per-frame kernel ignores the hint: padded product
        assert_exact(ops.conv3d_fwd_raw(xg, kg, bg, k_real=c), m.y, "mixer y [per-frame]")
    dw, db = ops.conv3d_wgrad_raw(xg, gyg, tuple(m.k.shape))
    assert_exact(dw, m.dw, "mixer dw")
    assert_exact(db, m.db, "mixer db")
    assert float(dw[..., c:, :].abs().max()) == 0 and float(dw[..., c:].abs().max()) == 0 and float(db[c:].abs().max()) == 0


@pytest.mark.parametrize("shape", POINTWISE_SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("cin", [16, 12])
def test_conv_pointwise_exact(dev, cin, dtype, shape):
    """1x1x1 convs onto 3 channels (HBM-stream kernels), fp32 and bf16 storage: forward, input gradient, weight and bias gradients,
    the fused `addend + conv` forward and the `other gradient + dgrad` backward, at V = 1, odd V, and a V over many workgroups; the
    generic path on the same data."""
    ops = _ops()
    p = pointwise_case(cin, shape, dtype)
    xg, kg, bg, gyg = p.x.to(dev, dtype), p.k.to(dev), p.b.to(dev), p.gy.to(dev, dtype)
    for form, hooks in (("stream", dict()), ("generic", dict(generic=True))):
        with kernel_form(**hooks):
            assert_exact(ops.conv3d_fwd_raw(xg, kg, bg), p.y, f"{p.name} [{form}]: y")
            assert_exact(ops.conv3d_dgrad_raw(gyg, kg), p.dx, f"{p.name} [{form}]: dx")
            dw, db = ops.conv3d_wgrad_raw(xg, gyg, tuple(p.k.shape))
            assert_exact(dw, p.dw, f"{p.name} [{form}]: dw")
            assert_exact(db, p.db, f"{p.name} [{form}]: db")
    ag = p.addend.to(dev, dtype)
    assert ops.conv3d_pointwise_add_ok(xg, kg, ag) and ops.conv3d_pointwise_fork_ok(xg, kg)
    assert_exact(ops.conv3d_pointwise_add(xg, kg, bg, ag), p.y_add, f"{p.name}: addend + y")
    xr = xg.clone().requires_grad_(True)
    y, x_other = ops.conv3d_pointwise_fork(xr, kg, bg)
    assert_exact(y.detach(), p.y, f"{p.name}: fork y")
    torch.autograd.backward([y, x_other], [gyg, p.dother.to(dev, dtype)])
    assert_exact(xr.grad, p.dx_add, f"{p.name}: other gradient + dx")


def _run_convt(ops, c, dev, what, packed=False):
    xg, kg, bg, gyg = c.x.to(dev, BF), c.k.to(dev), c.b.to(dev), c.gy.to(dev, BF)
    pf = pd = None
    if packed:
        pack = ops.convt_prepack([kg])[0]
        assert pack is not None
        pf, pd = pack.fwd, pack.dgrad
    assert_exact(ops.convt_fwd_raw(xg, kg, bg, packed=pf), c.y, f"{what}: y")
    assert_exact(ops.convt_dgrad_raw(gyg, kg, packed=pd), c.dx, f"{what}: dx")
    if not packed:
        dw, db = ops.convt_wgrad_db_raw(xg, gyg, tuple(c.k.shape))
        assert_exact(dw, c.dw, f"{what}: dw")
        assert_exact(db, c.db, f"{what}: db")


@pytest.mark.parametrize("ci,co,dims", CONVT_SMALL)
def test_conv_transpose_exact(dev, ci, co, dims):
    """ConvTranspose (1,2,2): forward, input gradient, weight + bias gradient on the bf16 matrix-core path (weights packed per call and
    prepacked) and on the generic path, and into / out of channel slices of wider buffers, against the fp64 restatement
    out[2i + d] = x[i] . K[1 - d]."""
    from video_vae_amd._lib import lib
    ops = _ops()
    c = convt_case(ci, co, dims)
    assert lib().vvae_convt_bf16_supported(ci, co, ci, co) == 1
    _run_convt(ops, c, dev, f"{c.name} [fast]")
    _run_convt(ops, c, dev, f"{c.name} [prepacked]", packed=True)
    with kernel_form(generic=True):
        _run_convt(ops, c, dev, f"{c.name} [generic]")
    n, t, h, w = dims
    sentinel = 77.0
    xg, kg, bg, gyg = c.x.to(dev, BF), c.k.to(dev), c.b.to(dev), c.gy.to(dev, BF)
    buf = torch.full((n, t, 2 * h, 2 * w, 2 * co), sentinel, dtype=BF, device=dev)
    ops.convt_fwd_raw(xg, kg, bg, out=buf[..., :co])
    assert_exact(buf[..., :co], c.y, f"{c.name}: y into a channel slice")
    assert bool((buf[..., co:] == sentinel).all()), "y: wrote outside its channel slice"
    gwide = torch.full((n, t, 2 * h, 2 * w, 2 * co), 1.0, dtype=BF, device=dev)
    gwide[..., co:] = gyg
    buf = torch.full((n, t, h, w, 2 * ci), sentinel, dtype=BF, device=dev)
    ops.convt_dgrad_raw(gwide[..., co:], kg, out=buf[..., ci:])
    assert_exact(buf[..., ci:], c.dx, f"{c.name}: dx from / into channel slices")
    assert bool((buf[..., :ci] == sentinel).all()), "dx: wrote outside its channel slice"


@pytest.mark.parametrize("ci,co,dims", CONVT_FULL)
def test_conv_transpose_production_extent_exact(dev, ci, co, dims):
    """Each up-conv at its real resolution (B = 4 x 16 frames): whole outputs against the CPU restatement (fp32 on integer data: exact)."""
    ops = _ops()
    c = convt_case(ci, co, dims, gy_hi=1, dtype=F32, device=dev)
    try:
        _run_convt(ops, c, dev, c.name)
    finally:
        del c
        torch.cuda.empty_cache()


@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
def test_gemm_nt_forms_exact(dev, m, n, k):
    """C = epi(A B^T + bias) on both kernel forms (gemm_nt.hip, gemm_pp.hip) against fp64: no epilogue, bias, bias + residual, and the
    pre-activation h saved by the SiLU epilogue (silu(h) itself stays on its tolerance; the * silu'(res) epilogue is left out: not
    integer arithmetic).  A and the residual are pitched views.  Both forms must equal fp64, not merely each other."""
    ops = _ops()
    g = gemm_nt_case(m, n, k, device=dev)
    a = g.a_full.to(dev, BF)[:, :k]
    b, bias = g.b.to(dev, BF), g.bias.to(dev)
    res = g.res_full.to(dev, BF)[:, :n]
    forms = []
    if ops.gemm_nt_supported(a, b):
        forms.append("nt")
    if ops.lib().vvae_gemm_pp_supported(m, n, k, a.stride(0), b.stride(0), n) == 1:
        forms.append("pp")
    assert "nt" in forms, "every shape of the two source tests runs on gemm_nt.hip"
    assert "pp" in forms or (m, n, k) not in PP_SHAPES
    for form in forms:
        what = f"{g.name} [{form}]"
        assert_exact(ops.gemm_nt(a, b, form=form), g.h0, f"{what}: a b^T")
        assert_exact(ops.gemm_nt(a, b, bias, form=form), g.h, f"{what}: + bias")
        assert_exact(ops.gemm_nt(a, b, bias, res, ops.EPI_RES, form=form), g.hr, f"{what}: + bias + res")
        act, h = ops.gemm_nt(a, b, bias, None, ops.EPI_SILU, form=form)
        assert_exact(h, g.h, f"{what}: saved pre-activation")
        want = F.silu(h.float())                             # the existing bar (rtol = atol = 1e-2), evaluated on the device
        assert bool(((act.float() - want).abs() <= 1e-2 + 1e-2 * want.abs()).all()), f"{what}: silu"


@pytest.mark.parametrize("big", [True, False])
@pytest.mark.parametrize("m,n,k", TN_SHAPES)
def test_gemm_tn_exact(dev, m, n, k, big):
    """dW = X^T dY and db = colsum(dY) from the split-K kernels (256 x 256 tiles on / off, the 96-wide edge tiles, K = 33 / 77 / 500)
    against fp64: dense integer operands, fp32 outputs."""
    from video_vae_amd._lib import lib
    ops = _ops()
    g = gemm_tn_case(m, n, k)
    a, b = g.a.to(dev, BF), g.b.to(dev, BF)
    assert ops.gemm_tn_supported(a, b)
    lib().vvae_gemm_tn_use_big_tiles(1 if big else 0)
    try:
        c, db = ops.gemm_tn(a, b)
        c2, none = ops.gemm_tn(a, b, False)
    finally:
        lib().vvae_gemm_tn_use_big_tiles(1)
    assert_exact(c, g.c, f"{g.name}: dW")
    assert_exact(db, g.db, f"{g.name}: db")
    assert none is None
    assert_exact(c2, g.c, f"{g.name}: dW (no column sums)")


def test_gemm_tn_grouped_exact(dev):
    """Parked Linear weight gradients multiplied in one grouped launch (whole-K tiles) straight into the flat gradient slots, driven
    through _WgradQueue: every dW and db against fp64."""
    ops = _ops()
    cases = [gemm_tn_case(m, n, GROUPED_K, i) for i, (m, n) in enumerate(GROUPED_SHAPES)]
    marked = []
    opt = types.SimpleNamespace(mark_external=lambda p: marked.append(p))
    items = []
    for g in cases:
        m, n = g.c.shape
        kern = torch.nn.Parameter(torch.zeros(m, n, device=dev)); bias = torch.nn.Parameter(torch.zeros(n, device=dev))
        kern.gview = torch.full((m, n), 7.0, device=dev); bias.gview = torch.full((n,), 7.0, device=dev)
        items.append((g.a.to(dev, BF), g.b.to(dev, BF), kern, bias))
    assert sum((m // 256) * (n // 256) for m, n in GROUPED_SHAPES) >= ops.GROUP_MIN_TILES
    ops.WGRAD_QUEUE[0] = []
    try:
        for it in items:
            assert ops.wgrad_deferrable(*it)
    finally:
        ops.WGRAD_QUEUE[0] = None
    q = ops._WgradQueue(opt)
    for it in items:
        q.append(it)
    q.flush()
    for g, (_, _, kern, bias) in zip(cases, items):
        assert_exact(kern.gview, g.c, f"{g.name}: grouped dW")
        assert_exact(bias.gview, g.db, f"{g.name}: grouped db")
    assert len(marked) == 2 * len(items)


@pytest.mark.parametrize("m,k,n", LINRES_SHAPES)
def test_linear_residual_exact(dev, m, k, n):
    """y = x W + bias + res as one library product: a library GEMM on integer data is exact as well.  Both weight operand forms
    ((K, N) and its (N, K) transpose), with and without the residual, contiguous and pitched x / res rows."""
    ops = _ops()
    g = linres_case(m, k, n, device=dev)
    xf, rf = g.x_full.to(dev, BF), g.r_full.to(dev, BF)
    wg, bg = g.w.to(dev, BF), g.b.to(dev, BF)
    wt = wg.t().contiguous()
    for pitched in (False, True):
        xg = xf[:, :k] if pitched else xf[:, :k].contiguous()
        rg = rf[:, :n] if pitched else rf[:, :n].contiguous()
        assert ops.linear_residual_ok(xg, wg, bg, rg)
        for form, kw in (("w", dict()), ("w^T", dict(wt=wt))):
            what = f"{g.name} [{form}{', pitched' if pitched else ''}]"
            assert_exact(ops.linear_residual(xg, wg, bg, rg, **kw), g.y, f"{what}: x W + b + res")
            assert_exact(ops.linear_residual(xg, wg, bg, None, **kw), g.plain, f"{what}: x W + b")


@pytest.mark.parametrize("shape", SUM_ROWS_SHAPES)
def test_sum_rows_exact(dev, shape):
    ops = _ops()
    g = colsum_ref(shape, 90, 3)
    assert_exact(ops.sum_rows(g.x.to(dev)), g.sum, g.name)


@pytest.mark.parametrize("v,c,dt", COLSUM_CASES)
def test_colsum_exact(dev, v, c, dt):
    """vvae_colsum: vector form, column-group loop, scalar fallback (odd widths), a pitched slice."""
    ops = _ops()
    g = colsum_ref((v, c), v + c, 2)
    x = F.pad(g.x, (0, 8), value=1.0).to(dev, dt)[:, :c] if c % 8 == 0 else g.x.to(dev, dt)
    assert_exact(ops.colsum_raw(x), g.sum, g.name)


@pytest.mark.parametrize("rows,cols,n0", FOLD_CASES)
def test_fold_partials_exact(dev, rows, cols, n0):
    """ops.fold_partials: the immediate form, and parked in a _WgradQueue and folded by the grouped launch into the parameters' slots."""
    ops = _ops()
    g = colsum_ref((rows, cols), 91, 3)
    part = g.x.to(dev)
    s0, s1 = ops.fold_partials(part, None, None, n0)
    assert_exact(s0, g.sum[:n0], f"{g.name}: first parameter")
    assert_exact(s1, g.sum[n0:], f"{g.name}: second parameter")
    opt = types.SimpleNamespace(mark_external=lambda p: None)
    p0 = torch.nn.Parameter(torch.zeros(n0, device=dev)); p0.gview = torch.full((n0,), 7.0, device=dev)
    p1 = None
    if cols > n0:
        p1 = torch.nn.Parameter(torch.zeros(cols - n0, device=dev)); p1.gview = torch.full((cols - n0,), 7.0, device=dev)
    q = ops._WgradQueue(opt)
    ops.WGRAD_QUEUE[0] = q
    try:
        assert ops.fold_partials(part, p0, p1, n0) == (None, None)
    finally:
        ops.WGRAD_QUEUE[0] = None
    q.flush_folds()
    assert_exact(p0.gview, g.sum[:n0], f"{g.name}: parked fold, first parameter")
    if p1 is not None:
        assert_exact(p1.gview, g.sum[n0:], f"{g.name}: parked fold, second parameter")
