"""The SSIM distortion term on the GPU: vvae_ssim_loss_fwd / vvae_ssim_loss_bwd (csrc/metrics.hip) and ops.ssim_frames against
metrics.ssim_grad_reference and ops.recon_metrics, poisoned padding and guard words, the refusals, the op inside a captured graph, the ascent
the gradient is for, the eager and the graphed train step of both VideoVAE flavours, and ``train --ssim-weight``."""
import gc
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from video_vae_amd import metrics as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 32
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
PAIRS = [("fp32", "fp32"), ("fp32", "bf16"), ("bf16", "fp32"), ("bf16", "bf16")]
B, T = 2, 3
SENTINEL = -7.0
KINDS = ["random", "near", "flat", "ramp"]


def _band_height():
    """Two bands of the library's own plan plus 3 rows: a frame of 32 rows is cut into bands of R rows (two of them); H = 2 R + 3 is then
    three bands with an uneven last one.  From vvae_ssim_loss_band_rows, not a literal."""
    from video_vae_amd._lib import lib
    r = int(lib().vvae_ssim_loss_band_rows(B, T, 32, 20, 3))
    assert 0 < r < 32
    h = 2 * r + 3
    assert 0 < int(lib().vvae_ssim_loss_band_rows(B, T, h, 20, 3)) < h               # more than one band
    return h


def _shapes():
    # one valid position (1 and 3 channels); W C no multiple of 4 (the element-wise path) twice; 4 channels; several bands; the
    # production row; W C = 2048, the limit; one channel at an odd size
    return [(11, 11, 1), (11, 11, 3), (12, 13, 2), (13, 27, 3), (16, 16, 4), (_band_height(), 20, 3), (40, 256, 3), (11, 512, 4), (33, 70, 1)]


SHAPES = ["11x11x1", "11x11x3", "12x13x2", "13x27x3", "16x16x4", "bands", "40x256x3", "11x512x4", "33x70x1"]


def _shape(name):
    return _shapes()[SHAPES.index(name)]


def _bf16_valued(v):
    return v.to(torch.bfloat16).to(torch.float64)


_CASES = {}


def _case(name, kind, video_div, clamp=False):
    """bf16-valued float64 operands of one shape and input family, with one masked frame, an upstream gradient with a zero and negative
    entries, and the float64 reference: computed once, shared, never written."""
    key = (name, kind, video_div, clamp)
    if key not in _CASES:
        h, w, c = _shape(name)
        g = torch.Generator().manual_seed(1000 * SHAPES.index(name) + KINDS.index(kind))
        shape = (B, T, h, w, c)
        xs = (B // video_div, T, h, w, c)
        x = torch.rand(xs, generator=g, dtype=torch.float64)
        noise = torch.randn(shape, generator=g, dtype=torch.float64)
        if kind == "flat":
            x = torch.full(xs, 0.5, dtype=torch.float64)
        elif kind == "ramp":
            x = (torch.arange(w, dtype=torch.float64) / (w - 1)).view(1, 1, 1, w, 1).expand(xs).contiguous()
        xr = x.repeat_interleave(video_div, dim=0)
        y = {"random": torch.rand(shape, generator=g, dtype=torch.float64), "near": xr + 0.02 * noise, "flat": xr + 0.01 * noise,
             "ramp": 0.9 * xr + 0.03}[kind]
        if clamp:                                                # values below 0, above 1 and exactly 0 and 1
            y = y * 1.5 - 0.25
            flat = y.reshape(-1)
            flat[0::11] = 0.0
            flat[1::11] = 1.0
        x, y = _bf16_valued(x), _bf16_valued(y)
        mask = torch.tensor([[1.0, 1.0, 1.0], [1.0, 0.0, 2.0]])
        gout = torch.tensor([[1.0, -0.75, 0.0], [2.5, 3.0, -1.0]])
        ssim, d = M.ssim_grad_reference(x, y, mask, gout, clamp=clamp, video_div=video_div)
        _CASES[key] = (x, y, mask, gout, ssim, d)
    return _CASES[key]


def _restatement_fp32(x, y, mask, gout, clamp, video_div):
    """The definition (metrics.ssim_grad_reference) restated from framework ops in fp32 on the CPU: what fp32 arithmetic alone loses."""
    x, y = x.float().repeat_interleave(video_div, dim=0), y.float()
    b, t, h, w, c = y.shape
    inside = (y >= 0) & (y <= 1)
    if clamp:
        x, y = x.clamp(0, 1), y.clamp(0, 1)
    planes = lambda v: v.permute(0, 1, 4, 2, 3).reshape(b * t * c, 1, h, w)
    xp, yp = planes(x), planes(y)
    g = M.gaussian_window(torch.float32)
    q = torch.cat([xp, yp, xp * xp, yp * yp, xp * yp], dim=1)
    q = F.conv2d(q, g.view(1, 1, 11, 1).expand(5, 1, 11, 1), groups=5)
    q = F.conv2d(q, g.view(1, 1, 1, 11).expand(5, 1, 1, 11), groups=5)
    mx, my, uxx, uyy, uxy = [v.unsqueeze(1) for v in q.unbind(1)]
    sx, sy, sxy = uxx - mx * mx, uyy - my * my, uxy - mx * my
    a1, a2, b1, b2 = 2 * mx * my + M.C1, 2 * sxy + M.C2, mx * mx + my * my + M.C1, sx + sy + M.C2
    s = a1 * a2 / (b1 * b2)
    maps = [2 * mx * (a2 - a1) / (b1 * b2) + 2 * my * s * (1 / b2 - 1 / b1), -s / b2, 2 * a1 / (b1 * b2)]

    def transposed(m):
        m = F.conv2d(m, g.view(1, 1, 11, 1), padding=(10, 0))
        m = F.conv2d(m, g.view(1, 1, 1, 11), padding=(0, 10))
        return m.reshape(b, t, c, h, w).permute(0, 1, 3, 4, 2)
    ta, tb, tc = (transposed(m) for m in maps)
    d = (ta + 2 * y * tb + x * tc) * (gout.float() / (c * (h - 10) * (w - 10))).view(b, t, 1, 1, 1)
    if clamp:
        d = torch.where(inside, d, torch.zeros(()))
    return torch.where((mask != 0).view(b, t, 1, 1, 1), d, torch.zeros(()))


def _poisoned(x, y, mask, video_div, dev, dtx, dty):
    """The operands on the device with NaN in every masked frame of the reconstruction, and of the clip where every sample that reads the
    frame is masked."""
    xg, yg = x.clone(), y.clone()
    dead = mask == 0
    yg[dead] = float("nan")
    xg[dead.reshape(B // video_div, video_div, T).all(dim=1)] = float("nan")
    return xg.to(DTYPES[dtx]).to(dev), yg.to(DTYPES[dty]).to(dev)


# ---------------------------------------------------------------------------------------------------------------- forward values
@pytest.mark.parametrize("video_div", [1, 2])
@pytest.mark.parametrize("name", SHAPES)
def test_forward_values(dev, name, video_div):
    """video_div = 1: bitwise ops.recon_metrics' ssim; video_div = 2: bitwise the video_div = 1 call on repeat_interleave(2); both within
    1e-4 of float64 (the bar of tests/test_gpu_metrics.py).  All four dtype pairs, clamp on and off."""
    from video_vae_amd import ops
    x, y, mask, _, ssim64, _ = _case(name, "random", video_div)
    for dtx, dty in PAIRS:
        xg, yg = _poisoned(x, y, mask, video_div, dev, dtx, dty)
        mg = mask.to(dev)
        for clamp in (False, True):
            got = ops.ssim_frames(xg, yg, mg, video_div=video_div, clamp=clamp)
            assert got.dtype == torch.float32 and tuple(got.shape) == (B, T)
            wide = xg.repeat_interleave(video_div, dim=0)
            if video_div == 1:
                want = ops.recon_metrics(xg, yg, mg, clamp)[2]
            else:
                want = ops.ssim_frames(wide, yg, mg, video_div=1, clamp=clamp)
                assert torch.equal(want, ops.recon_metrics(wide, yg, mg, clamp)[2])
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (dtx, dty, clamp)
            err = float((got.cpu().double() - ssim64).abs().max())
            assert err <= 1e-4, (dtx, dty, clamp, err)
            assert float(got[1, 1]) == 0.0


# ---------------------------------------------------------------------------------------------------------------- the gradient
@pytest.mark.parametrize("video_div", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", SHAPES)
def test_gradient_against_the_reference(dev, name, kind, video_div):
    """Element-wise against metrics.ssim_grad_reference on the bf16-valued inputs.  random and near: within 1e-3 of the tensor's max-abs
    (the project's fp32 gradient bar).  flat and ramp (b2 -> C2 amplifies cancellation): within max(1e-3, 3 x the error of the fp32
    restatement of the same definition) of it.  A bf16 reconstruction adds 2^-8 |reference element| for its single output rounding.
    Masked frames and frames whose upstream gradient is 0: exactly 0."""
    from video_vae_amd import ops
    x, y, mask, gout, _, ref = _case(name, kind, video_div)
    scale = float(ref.abs().max())
    assert scale > 0
    bar = 1e-3
    if kind in ("flat", "ramp"):
        rest = float((_restatement_fp32(x, y, mask, gout, False, video_div).double() - ref).abs().max()) / scale
        bar = max(1e-3, 3 * rest)
    worst = {"fp32": 0.0, "bf16": 0.0}                      # by the reconstruction's (the gradient's) dtype
    for dtx, dty in PAIRS:
        xg, yg = _poisoned(x, y, mask, video_div, dev, dtx, dty)
        leaf = yg.clone().requires_grad_(True)
        out = ops.ssim_frames(xg, leaf, mask.to(dev), video_div=video_div, clamp=False)
        (grad,) = torch.autograd.grad(out, leaf, gout.to(dev))
        assert grad.dtype == DTYPES[dty] and grad.shape == leaf.shape
        got = grad.cpu().double()
        assert bool(torch.isfinite(got).all())
        assert not got[1, 1].any() and not got[0, 2].any()                     # a masked frame; an upstream gradient of 0
        tol = bar * scale + ((2.0 ** -8) * ref.abs() if dty == "bf16" else 0.0)
        err = (got - ref).abs()
        worst[dty] = max(worst[dty], float(err.max()) / scale)
        assert bool((err <= tol).all()), (dtx, dty, float(err.max()) / scale, bar)
    print(f"{name} {kind} div {video_div}: worst error fp32 {worst['fp32']:.2e}, bf16 {worst['bf16']:.2e} of the scale {scale:.3e} "
          f"(bar {bar:.2e}, bf16 + 2^-8 |element|)")


@pytest.mark.parametrize("name", ["12x13x2", "16x16x4", "40x256x3"])
def test_clamp_gates_the_gradient_in_the_right_places(dev, name):
    """clamp=True with y below 0, above 1 and exactly 0 and 1: zeros exactly where y lies strictly outside [0, 1], the reference elsewhere
    (it passes at exactly 0 and 1)."""
    from video_vae_amd import ops
    x, y, mask, gout, ssim64, ref = _case(name, "random", 1, clamp=True)
    live = (mask != 0).view(B, T, 1, 1, 1) & (gout != 0).view(B, T, 1, 1, 1)
    out_of_range = (y < 0) | (y > 1)
    edge = ((y == 0) | (y == 1)) & live
    assert bool(out_of_range.any()) and bool((y < 0).any()) and bool((y > 1).any()) and int(edge.sum()) > 0
    scale = float(ref.abs().max())
    for dtx, dty in PAIRS:
        xg, yg = _poisoned(x, y, mask, 1, dev, dtx, dty)
        leaf = yg.clone().requires_grad_(True)
        out = ops.ssim_frames(xg, leaf, mask.to(dev), clamp=True)
        (grad,) = torch.autograd.grad(out, leaf, gout.to(dev))
        got = grad.cpu().double()
        assert float((out.detach().cpu().double() - ssim64).abs().max()) <= 1e-4
        assert not got[out_of_range].any()
        zero_elsewhere = (got == 0) & ~out_of_range & live
        assert bool((ref[zero_elsewhere].abs() <= 1e-3 * scale).all())           # a zero inside the range only where the reference is ~0
        assert int((got[edge] != 0).sum()) >= int((ref[edge].abs() > 1e-3 * scale).sum())
        tol = 1e-3 * scale + ((2.0 ** -8) * ref.abs() if dty == "bf16" else 0.0)
        assert bool(((got - ref).abs() <= tol).all()), (dtx, dty)


# ---------------------------------------------------------------------------------------------------------------- poison, guards, NULL
def _entries():
    from video_vae_amd import ops
    from video_vae_amd._lib import lib
    fwd = lambda x, y, m, s, ws, b, t, h, w, c, div=1, clamp=0, dx=0, dy=0: lib().vvae_ssim_loss_fwd(
        ops._p(x), dx, ops._p(y), dy, ops._p(m), ops._p(s), ops._p(ws), b, t, h, w, c, div, clamp, ops._stream())
    bwd = lambda x, y, m, g, ws, d, b, t, h, w, c, div=1, clamp=0, dx=0, dy=0: lib().vvae_ssim_loss_bwd(
        ops._p(x), dx, ops._p(y), dy, ops._p(m), ops._p(g), ops._p(ws), ops._p(d), b, t, h, w, c, div, clamp, ops._stream())
    return fwd, bwd


@pytest.mark.parametrize("dty", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["13x27x3", "bands", "40x256x3"])
def test_poisoned_padding_and_guard_words(dev, name, dty):
    """NaN in every masked frame of both operands and a NaN-filled drecon: the outputs are finite, the masked frames' gradients exactly 0,
    and the guard words around drecon and around the workspace are untouched."""
    from video_vae_amd._lib import lib
    fwd, bwd = _entries()
    h, w, c = _shape(name)
    x, y, mask, gout, ssim64, ref = _case(name, "near", 1)
    xg, yg = _poisoned(x, y, mask, 1, dev, "bf16", dty)
    n = B * T * h * w * c
    nws = int(lib().vvae_ssim_loss_ws_floats(B, T, h, w, c))
    guard = 64
    wbuf = torch.full((nws + 2 * guard,), SENTINEL, device=dev)
    ws = wbuf[guard:guard + nws]
    dbuf = torch.full((n + 2 * guard,), float("nan"), device=dev).to(DTYPES[dty])
    dbuf[:guard] = SENTINEL
    dbuf[guard + n:] = SENTINEL
    dr = dbuf[guard:guard + n]
    ssim = torch.full((B, T), float("nan"), device=dev)
    mg, gg = mask.to(dev), gout.to(dev)
    code = 1 if dty == "bf16" else 0
    assert fwd(xg, yg, mg, ssim, ws, B, T, h, w, c, dx=1, dy=code) == 0
    assert bwd(xg, yg, mg, gg, ws, dr, B, T, h, w, c, dx=1, dy=code) == 0
    torch.cuda.synchronize()
    got = dr.view(B, T, h, w, c).cpu().double()
    assert bool(torch.isfinite(ssim).all()) and bool(torch.isfinite(got).all())
    assert float(ssim[1, 1]) == 0.0 and not got[1, 1].any() and not got[0, 2].any()
    assert bool((wbuf[:guard] == SENTINEL).all()) and bool((wbuf[guard + nws:] == SENTINEL).all())
    assert bool((dbuf[:guard] == SENTINEL).all()) and bool((dbuf[guard + n:] == SENTINEL).all())
    scale = float(ref.abs().max())
    tol = 1e-3 * scale + ((2.0 ** -8) * ref.abs() if dty == "bf16" else 0.0)
    assert bool(((got - ref).abs() <= tol).all())


def test_an_unused_output_gives_none_and_launches_nothing(dev):
    """gout = None (set_materialize_grads(False)): no launch with a NULL gout, the gradient is None."""
    from video_vae_amd import ops
    x, y, mask, _, _, _ = _case("13x27x3", "near", 1)
    xg, yg = x.float().to(dev), y.float().to(dev)
    leaf = yg.clone().requires_grad_(True)
    out = ops.ssim_frames(xg, leaf, mask.to(dev))
    other = (leaf * 2).sum()
    (g,) = torch.autograd.grad(other, leaf)                                     # the op's node is not on the path
    assert bool((g == 2).all())
    ctx = types.SimpleNamespace(saved_tensors=(xg, yg, mask.to(dev)))
    assert ops._SsimFrames.backward(ctx, None) == (None, None, None, None, None)
    del out
    fwd, bwd = _entries()
    h, w, c = _shape("13x27x3")
    from video_vae_amd._lib import lib
    ws = torch.empty(int(lib().vvae_ssim_loss_ws_floats(B, T, h, w, c)), device=dev)
    dr = torch.full_like(yg, SENTINEL)
    assert bwd(xg, yg, mask.to(dev), None, ws, dr, B, T, h, w, c) == 1001        # the C entry refuses a NULL gout
    torch.cuda.synchronize()
    assert bool((dr == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_before_any_launch(dev):
    from video_vae_amd import ops
    from video_vae_amd._lib import VvaeError, lib
    mk = lambda b, t, h, w, c: torch.zeros((b, t, h, w, c), dtype=torch.bfloat16, device=dev)
    ones = lambda b, t: torch.ones((b, t), device=dev)
    good_x, good_y, good_m = mk(2, 3, 13, 27, 3), mk(2, 3, 13, 27, 3), ones(2, 3)
    for bad in (lambda: ops.ssim_frames(mk(1, 1, 11, 513, 4), mk(1, 1, 11, 513, 4), ones(1, 1)),      # W C = 2052
                lambda: ops.ssim_frames(mk(1, 1, 10, 16, 3), mk(1, 1, 10, 16, 3), ones(1, 1)),        # H = 10
                lambda: ops.ssim_frames(mk(1, 1, 16, 10, 3), mk(1, 1, 16, 10, 3), ones(1, 1)),
                lambda: ops.ssim_frames(mk(1, 1, 16, 16, 5), mk(1, 1, 16, 16, 5), ones(1, 1)),        # C = 5
                lambda: ops.ssim_frames(mk(65536, 1, 11, 11, 1), mk(65536, 1, 11, 11, 1), ones(65536, 1)),    # B T = 65536
                lambda: ops.ssim_frames(good_x.cpu(), good_y, good_m), lambda: ops.ssim_frames(good_x, good_y.cpu(), good_m),
                lambda: ops.ssim_frames(good_x, good_y, good_m.cpu()), lambda: ops.ssim_frames(good_x.half(), good_y, good_m),
                lambda: ops.ssim_frames(good_x, good_y, good_m, video_div=3), lambda: ops.ssim_frames(good_x, good_y[:, :2], good_m)):
        with pytest.raises(VvaeError):
            bad()
    # the C entries: shapes they do not take, NULL and misaligned pointers, a drecon that overlaps an operand, the workspace, gout
    fwd, bwd = _entries()
    h, w, c = 13, 27, 3
    n = B * T * h * w * c
    nws = int(lib().vvae_ssim_loss_ws_floats(B, T, h, w, c))
    buf = torch.rand(n + 8, device=dev)
    x, y = torch.rand(n, device=dev), buf[:n]
    kept_y = y.clone()
    wbuf = torch.full((nws + 8,), SENTINEL, device=dev)
    ws = wbuf[:nws]
    ssim = torch.full((B, T), SENTINEL, device=dev)
    dr = torch.full((n,), SENTINEL, device=dev)
    mask, g = torch.ones(B, T, device=dev), torch.ones(B, T, device=dev)
    codes = [fwd(x, y, mask, ssim, ws, B, T, 10, w, c), fwd(x, y, mask, ssim, ws, B, T, h, 10, c), fwd(x, y, mask, ssim, ws, B, T, h, 513, 4),
             fwd(x, y, mask, ssim, ws, B, T, h, w, 5), fwd(x, y, mask, ssim, ws, 65536, 1, 11, 11, 1), fwd(x, y, mask, ssim, ws, B, T, h, w, c, div=0),
             fwd(x, y, mask, ssim, ws, B, T, h, w, c, div=4), fwd(None, y, mask, ssim, ws, B, T, h, w, c), fwd(x, None, mask, ssim, ws, B, T, h, w, c),
             fwd(x, y, None, ssim, ws, B, T, h, w, c), fwd(x, y, mask, None, ws, B, T, h, w, c), fwd(x, y, mask, ssim, None, B, T, h, w, c),
             fwd(x, y, mask, ssim, wbuf[1:nws + 1], B, T, h, w, c), fwd(x, y, mask, ssim, ws, B, T, h, w, c, dx=2),
             fwd(x, y, mask, ssim, y, B, T, h, w, c),
             bwd(x, y, mask, g, ws, dr, B, T, 10, w, c), bwd(x, y, mask, g, ws, dr, B, T, h, w, 5), bwd(x, y, mask, g, ws, dr, B, T, h, 513, 4),
             bwd(x, y, mask, g, ws, dr, 65536, 1, 11, 11, 1), bwd(x, y, mask, g, ws, None, B, T, h, w, c), bwd(x, y, mask, None, ws, dr, B, T, h, w, c),
             bwd(x, y, mask, g, None, dr, B, T, h, w, c), bwd(x, y, mask, g, ws, y, B, T, h, w, c), bwd(x, y, mask, g, ws, x, B, T, h, w, c),
             bwd(x, y, mask, g, ws, buf[4:n + 4], B, T, h, w, c), bwd(x, y, mask, g, ws, ws[:n], B, T, h, w, c),
             bwd(x, y, mask, g, ws, dr, B, T, h, w, c, dy=3)]
    assert codes == [1001] * len(codes), codes
    torch.cuda.synchronize()
    assert torch.equal(y, kept_y) and bool((ssim == SENTINEL).all()) and bool((dr == SENTINEL).all()) and bool((wbuf == SENTINEL).all())
    assert fwd(x, y, mask, ssim, ws, B, T, h, w, c) == 0 and bwd(x, y, mask, g, ws, dr, B, T, h, w, c) == 0      # well formed: taken
    torch.cuda.synchronize()
    assert not bool((ssim == SENTINEL).any()) and not bool((dr == SENTINEL).any()) and torch.equal(y, kept_y)
    assert bool((wbuf[nws:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------- captured
def test_captured_and_replayed_equals_eager(dev):
    """Forward and backward inside a captured graph, replayed with other contents in the static operands, mask and upstream gradient:
    bitwise the eager values and gradient; no memset node."""
    from video_vae_amd import ops
    from video_vae_amd.graph import graph_node_census
    sets = []
    for kind in ("near", "random"):
        x, y, mask, gout, _, _ = _case("40x256x3", kind, 2)
        sets.append((x.to(torch.bfloat16).to(dev), y.to(torch.bfloat16).to(dev), mask.to(dev), gout.to(dev)))
    sets[1] = (sets[1][0], sets[1][1], torch.tensor([[0.0, 1.0, 1.0], [1.0, 1.0, 1.0]], device=dev), sets[1][3].flip(0))

    def eager(i):
        x, y, mask, gout = sets[i]
        leaf = y.clone().requires_grad_(True)
        out = ops.ssim_frames(x, leaf, mask, video_div=2, clamp=False)
        (grad,) = torch.autograd.grad(out, leaf, gout)
        return out.detach(), grad
    sx, smask, sg = sets[0][0].clone(), sets[0][2].clone(), sets[0][3].clone()
    sy = sets[0][1].clone().requires_grad_(True)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        torch.autograd.grad(ops.ssim_frames(sx, sy, smask, video_div=2, clamp=False), sy, sg)
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = ops.ssim_frames(sx, sy, smask, video_div=2, clamp=False)
        (grad,) = torch.autograd.grad(out, sy, sg)
    census = graph_node_census(graph)
    assert census is not None and census.get("memset", 0) == 0 and census.get("kernel", 0) >= 3, census
    for i in (0, 1, 0):
        with torch.no_grad():
            sx.copy_(sets[i][0])
            sy.copy_(sets[i][1])
        smask.copy_(sets[i][2])
        sg.copy_(sets[i][3])
        graph.replay()
        torch.cuda.synchronize()
        want_out, want_grad = eager(i)
        assert torch.equal(out.detach().view(torch.int32), want_out.view(torch.int32)), i
        assert torch.equal(grad.view(torch.int16), want_grad.view(torch.int16)), i
        again_out, again_grad = eager(i)                                         # eager twice: reproducible
        assert torch.equal(again_out, want_out) and torch.equal(again_grad.view(torch.int16), want_grad.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------- what it is for
def test_gradient_ascent_raises_the_ssim(dev):
    """10 steps of plain gradient ascent on y at a step size for which the float64 CPU run rises: the GPU run gains at least half of
    what the CPU run gains."""
    from video_vae_amd import ops
    g = torch.Generator().manual_seed(11)
    x = torch.rand((1, 2, 24, 28, 3), generator=g, dtype=torch.float64)
    y0 = (x + 0.15 * torch.randn(x.shape, generator=g, dtype=torch.float64)).float().double()
    x = x.float().double()
    mask, ones = torch.ones(1, 2), torch.ones(1, 2)
    lr = 20.0
    y = y0.clone()
    start = float(M.ssim_grad_reference(x, y, mask, ones, clamp=False)[0].mean())
    for _ in range(10):
        y = y + lr * M.ssim_grad_reference(x, y, mask, ones, clamp=False)[1]
    cpu_gain = float(M.ssim_grad_reference(x, y, mask, ones, clamp=False)[0].mean()) - start
    assert cpu_gain > 0.01, cpu_gain
    xg, yg, mg = x.float().to(dev), y0.float().to(dev), mask.to(dev)
    first = None
    for _ in range(10):
        leaf = yg.clone().requires_grad_(True)
        out = ops.ssim_frames(xg, leaf, mg, clamp=False)
        first = float(out.detach().mean()) if first is None else first
        (grad,) = torch.autograd.grad(out, leaf, ones.to(dev))
        yg = yg + lr * grad
    gpu_gain = float(ops.ssim_frames(xg, yg, mg, clamp=False).mean()) - first
    print(f"ssim {start:.4f}: float64 CPU gain {cpu_gain:.4f}, GPU gain {gpu_gain:.4f}")
    assert abs(first - start) <= 1e-4 and gpu_gain >= 0.5 * cpu_gain


# ---------------------------------------------------------------------------------------------------------------- the train step
def _small(flavour, seed=2):
    from video_vae_amd.infer import model_config
    import video_vae_amd as V
    from video_vae_amd import rl_model
    cls = rl_model.VideoVAE if flavour == "rl" else V.VideoVAE
    return cls(rngs=V.Rngs(seed), **model_config(SMALL, True))


def _batch(dev, seed=5, b=2, t=8):
    video = torch.rand((b, t, SMALL, SMALL, 3), generator=torch.Generator().manual_seed(seed)).to(dev).to(torch.bfloat16)
    mask = torch.ones(b, t)
    mask[1, t - 2:] = 0
    return video, mask.to(dev)


def _sampled_grads(opt):
    return {name: opt.g[o:o + p.numel()].clone() for name, p, o in zip(opt.names, opt.params, opt.offsets)
            if name.startswith("encoder.spatial_compression") or name.startswith("decoder.spatial_decompression")}


@pytest.mark.parametrize("flavour", ["model", "rl"])
def test_train_step_eager_and_graphed_with_the_ssim_term(dev, flavour, monkeypatch):
    """ssim_weight = 0.5 on the small model.  Eager: the loss is loss(off) + 0.5 (1 - aux["ssim"]) within the fp32 rounding of that sum
    (three roundings of numbers below 4: 2^-21), the gradients are finite and differ from the step without the key, and aux["ssim"] is
    frame_metrics' masked mean with clamp=False of the very reconstruction.  Graphed: no memset node (GraphedTrainStep raises on one) and
    loss and ssim bitwise the eager ones on the same noise.  Without the key: ops.ssim_frames is not entered and the loss and the sampled
    gradients are bitwise those of a second run without the key."""
    import video_vae_amd as V
    from video_vae_amd import loss as L, ops, optim
    from video_vae_amd.graph import GraphedTrainStep
    hw = (SMALL // 16) ** 2
    base = dict(L.HPARAMS)
    hparams = dict(base, ssim_weight=0.5)
    calls = []
    real = ops.ssim_frames
    monkeypatch.setattr(ops, "ssim_frames", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):                     # the driver's rule: ONE non-default stream for the whole run
        video, mask = _batch(dev)
        m = _small(flavour).to(dev)
        opt = optim.Optimizer(m, 0.0)                                           # lr = 0: the weights never move, so passes can be compared
        loss_0, aux_0 = L.train_step(m, opt, video, mask, base, hw, V.Rngs(3))
        grads_0 = _sampled_grads(opt)
        assert not calls and "ssim" not in aux_0 and len(grads_0) >= 2
        loss_0 = loss_0.clone()
        loss_s, aux_s = L.train_step(m, opt, video, mask, hparams, hw, V.Rngs(3))
        grads_s = _sampled_grads(opt)
        assert len(calls) == 1 and torch.isfinite(loss_s)
        ssim = aux_s["ssim"]
        print(f"{flavour}: loss {float(loss_0)!r} -> {float(loss_s)!r}, ssim {float(ssim)!r}")
        assert aux_s.keys() == aux_0.keys() | {"ssim"} and torch.isfinite(ssim) and -1.0 <= float(ssim) <= 1.0
        want = float(loss_0) + 0.5 * (1.0 - float(ssim))
        assert abs(float(loss_s) - want) <= 2.0 ** -21 * max(1.0, abs(want))
        differ = 0
        for name, g0 in grads_0.items():
            assert bool(torch.isfinite(grads_s[name]).all()), name
            differ += int(not torch.equal(g0, grads_s[name]))
        assert differ > 0
        # aux["ssim"] from the evaluation side's metric on the reconstruction of the same forward
        loss_e, aux_e = L.eval_step(m, video, mask, hparams, hw, V.Rngs(3))
        recon = aux_e["reconstruction"]
        div = 2 if flavour == "rl" else 1
        om = mask.repeat_interleave(div, dim=0)
        fm = M.frame_metrics(video.repeat_interleave(div, dim=0), recon, om, clamp=False).ssim
        masked_mean = ((fm * om).sum(dim=1) / om.sum(dim=1).clamp(min=1.0)).mean()
        assert abs(float(aux_e["ssim"]) - float(masked_mean)) <= 1e-6
        assert torch.equal(aux_e["ssim"], ssim) and torch.equal(loss_e, loss_s)
        del loss_s, aux_s, aux_0, aux_e, recon
        gc.collect()
        step = GraphedTrainStep(m, opt, video, mask, hparams, hw, V.Rngs(4), warmup=1, stream=torch.cuda.current_stream())
        assert step.census[0] is not None and all(c.get("memset", 0) == 0 for c in step.census), step.census
        video2, _ = _batch(dev, seed=6)
        for v in (video, video2):
            loss_g, aux_g = step(v, mask)
            torch.cuda.synchronize()
            loss_g, ssim_g = loss_g.clone(), aux_g["ssim"].clone()
            rngs = V.Rngs(9)
            for name, (_, buf) in step.noise.items():
                rngs.inject(name, buf.clone())
            loss_e, aux_e = L.eval_step(m, v, mask, hparams, hw, rngs)           # the loss with train=True: the same forward, eagerly
            print(f"{flavour}: loss graph {float(loss_g)!r} eager {float(loss_e)!r}; ssim graph {float(ssim_g)!r} eager {float(aux_e['ssim'])!r}")
            assert torch.equal(loss_g, loss_e) and torch.equal(ssim_g, aux_e["ssim"])
        # without the key: nothing is launched for the term and the numbers are those of the first run, bit for bit
        n = len(calls)
        m.zero_grad(set_to_none=True)
        loss_b, aux_b = L.train_step(m, opt, video, mask, base, hw, V.Rngs(3))
        assert len(calls) == n and "ssim" not in aux_b and torch.equal(loss_b, loss_0)
        for name, g0 in _sampled_grads(opt).items():
            assert torch.equal(g0, grads_0[name]), name
        torch.cuda.synchronize()


def _train(args, timeout=300, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), PYTHONUNBUFFERED="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "video_vae_amd.train"] + args, cwd=ROOT, env=env,
                       capture_output=True, text=True)
    if ok:
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r


def _lines(out):
    """The step lines without their clock field."""
    lines = [l for l in out.splitlines() if l.startswith("Epoch 0, Step ")]
    return [", ".join(f for f in l.split(", ") if not f.startswith("time = ")) for l in lines]


def test_train_driver_logs_ssim_only_with_the_flag(dev):
    """train --small --steps 6 --ssim-weight 0.5: every line carries ssim, the step is captured once with the term, no nan.  Without the
    flag (the parent's command line) no line carries it and the fields are the other run's without it; that this run's numbers are the
    parent's is the train-step test's bitwise comparison with the key absent."""
    common = ["--small", "--size", "32", "--per_device_batch_size", "2", "--max_frames", "8", "--steps", "6", "--log_every", "1"]
    out = _train(common + ["--ssim-weight", "0.5"]).stdout
    lines = _lines(out)
    assert len(lines) == 6, out
    for l in lines:
        assert -1.0 <= float(l.split("ssim = ")[1].split(",")[0]) <= 1.0, l
    assert "nan" not in out.lower(), out
    assert out.count("captured the train step") == 1 and "capture failed" not in out, out
    assert [l.split("mode = ")[1].split(",")[0] for l in lines] == ["eager"] + ["hipgraph"] * 5
    plain = _lines(_train(common).stdout)
    assert len(plain) == 6 and not any("ssim" in l for l in plain)
    assert [l.split(" = ")[0] for l in plain[0].split(", ")] == [f for f in (l.split(" = ")[0] for l in lines[0].split(", ")) if f != "ssim"]
    assert [l.split("Loss = ")[1].split(",")[0] for l in plain] != [l.split("Loss = ")[1].split(",")[0] for l in lines]
