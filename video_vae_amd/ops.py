"""torch.autograd.Function wrappers over the C ABI (include/vvae_hip.h).

PyTorch is plumbing here: it owns device memory and streams; every op below
runs a hand-written HIP kernel from libvvae_hip.so on the current stream.
Tensors must live on a GPU -- there is no CPU path (three exceptions: latent_fake_quant and latent_rate restate their arithmetic from
framework ops for CPU tensors, and ssim_frames runs metrics.ssim_frames_composed for them).
"""
import ctypes
import os
import sys

import torch
import torch.nn.functional as F

from ._lib import lib, check, VvaeError

DT = {torch.float32: 0, torch.bfloat16: 1}

_NOTED = set()


def note_fallback(key, message):
    """Say ONCE per process (rank 0, stderr) that a launch left the path the benchmark measures: a conv that is too large for the bf16
    matrix-core kernels' 32-bit buffer offsets and runs the fp32 generic kernels instead, a layer shape the fused HIP kernels do not take and
    that runs a framework op.  Fallbacks are allowed; invisible performance cliffs are not."""
    if key in _NOTED:
        return
    _NOTED.add(key)
    import os
    import sys
    if os.environ.get("RANK", "0") == "0":
        print(f"[video_vae_amd] fallback: {message}", file=sys.stderr, flush=True)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(t):
    if not t.is_cuda:
        raise VvaeError("video_vae_amd ops need GPU tensors (no CPU fallback); got device " + str(t.device))
    if t.dtype not in DT:
        raise VvaeError(f"unsupported activation dtype {t.dtype} (float32 or bfloat16)")
    return DT[t.dtype]


def rows(t):
    """(tensor, row pitch) with the tensor usable as (rows, C) with a uniform pitch; copies only if it must."""
    if t.dim() < 2:
        raise VvaeError("need at least 2 dims")
    ok = t.stride(-1) == 1 and t.stride(-2) >= t.size(-1)
    if ok:
        for i in range(t.dim() - 2):
            if t.size(i) != 1 and t.stride(i) != t.stride(i + 1) * t.size(i + 1):
                ok = False
                break
    if not ok:
        t = t.contiguous()
    return t, t.stride(-2)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def _ws(nbytes, device):
    if nbytes == 0:
        return None, 0
    buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return buf, nbytes


def fold_partials(part, p0, p1, n0):
    """Column sums of the per-workgroup partial rows ``part`` (rows, cols): columns [0, n0) are the gradient of parameter
    ``p0``, the rest that of ``p1`` (None: dropped).  Inside ``deferred_wgrad`` (and when the parameters own flat-buffer slots)
    the fold is parked and runs with up to 63 others in one launch straight into those slots: returns (None, None).  Otherwise
    returns the two sums."""
    q = WGRAD_QUEUE[0]
    if (q is not None and p0 is not None and part.is_cuda and getattr(p0, "gview", None) is not None and p0.numel() == n0
            and (p1 is None or (getattr(p1, "gview", None) is not None and p1.numel() == part.numel() // part.shape[0] - n0))):
        q.append_fold(part, p0, p1)
        return None, None
    tot = sum_rows(part).reshape(-1)
    return tot[:n0], tot[n0:]


def copy_grouped(dsts, srcs):
    """dst[i].copy_(src[i]) for lists of contiguous fp32 GPU tensors of equal sizes, 64 pairs per launch (gradient landing)."""
    for i0 in range(0, len(dsts), FOLD_MAX):
        d, s_ = dsts[i0:i0 + FOLD_MAX], srcs[i0:i0 + FOLD_MAX]
        n = len(d)
        VP, LA = ctypes.c_void_p * n, ctypes.c_long * n
        check(lib().vvae_copy_grouped(VP(*[t.data_ptr() for t in s_]), VP(*[t.data_ptr() for t in d]), LA(*[t.numel() for t in d]), n,
                                      _stream()), "vvae_copy_grouped")


def copy_grouped_ok(dst, src):
    return (dst.is_cuda and src.is_cuda and dst.dtype == torch.float32 and src.dtype == torch.float32 and dst.is_contiguous()
            and src.is_contiguous() and dst.numel() == src.numel() and dst.numel() > 0)


def _tall_narrow_split(rows, cols):
    """How a tall and narrow partial buffer (one row per attention workgroup) is folded: (rows, cols) is read as (r, c) = (rows/k, k*cols) so
    that many workgroups share the first pass, then the k partial rows are summed.  -> (r, c, k); k = 1: one pass over the buffer as it is."""
    r, c, k = rows, cols, 1
    while r > 1024 and r % 2 == 0 and c * 2 <= 8192:
        r //= 2; c *= 2; k *= 2
    return r, c, k


def sum_rows(part):
    """Column sums of a (rows, ...) fp32 partial buffer in fixed order -> shape part.shape[1:] (no memset, no atomics).

    Tall-and-narrow buffers are folded in two launches (_tall_narrow_split)."""
    cols0 = part.numel() // part.shape[0]
    r, cols, k = _tall_narrow_split(part.shape[0], cols0)
    out = torch.empty((k,) + tuple(part.shape[1:]), dtype=torch.float32, device=part.device)
    check(lib().vvae_sum_rows(_p(part), r, cols, _p(out), _stream()), "vvae_sum_rows")
    if k == 1:
        return out[0]
    out2 = torch.empty(part.shape[1:], dtype=torch.float32, device=part.device)
    check(lib().vvae_sum_rows(_p(out), k, cols0, _p(out2), _stream()), "vvae_sum_rows")
    return out2


class KernelTimer:
    """Per-launch HIP-event timing of tagged kernels on the current stream (bench.py's roofline leg).

    ``records[tag] = [algorithmic_bytes, flops, kernel_name, [(start, end), ...]]``; durations are read after a sync.
    """

    def __init__(self, gate_us=25):
        self.records = {}
        # a short delay kernel in front of every timed launch: the opening event, the launch and the closing event are then all queued
        # before the first of them executes, and the interval is the kernel's duration -- not kernel + the host's launch latency, which is
        # what an event pair reads on an idle stream (eager steps are host-bound: the stream IS idle at every launch).  0 = off.
        self.gate_us = int(gate_us)

    def launch(self, tag, alg_bytes, flops, kernel, fn):
        rec = self.records.setdefault(tag, [alg_bytes, flops, kernel, []])
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if self.gate_us > 0:
            check(lib().vvae_delay_us(self.gate_us, _stream()), "vvae_delay_us")
        a.record()
        rc = fn()
        b.record()
        rec[3].append((a, b))
        return rc

    def summary(self):
        """-> {tag: dict(n, avg_ms, total_ms, bytes, flops, kernel)} (call after torch.cuda.synchronize())."""
        out = {}
        for tag, (nbytes, flops, kernel, evs) in self.records.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            out[tag] = dict(n=len(ms), avg_ms=sum(ms) / len(ms), total_ms=sum(ms), bytes=nbytes, flops=flops, kernel=kernel)
        return out


TIMER = None      # set to a KernelTimer to time tagged launches


def _launch(tag, alg_bytes, flops, kernel, fn):
    if TIMER is None:
        return fn()
    return TIMER.launch(tag, alg_bytes, flops, kernel, fn)


BF16_SPAN_LIMIT = 1 << 31          # the bf16 conv kernels address through buffer descriptors: 32-bit byte offsets (conv3d_bf16.hip launch_roll)


def _bf16_fast(cin, cout, kt, kh, kw, ld_in, ld_out, which, dt, vox=0):
    """May this conv run the bf16 matrix-core kernels?  ``vox``: voxels of the launch -- a tensor of 2 GB or more (more than 512 frames of a
    32-channel 256 x 256 level) is beyond their 32-bit offsets and takes the generic fp32-matrix-core kernels, which is said once."""
    ok = dt == 1 and not _FORCE_GENERIC[0] and lib().vvae_conv3d_bf16_supported(cin, cout, kt, kh, kw, ld_in, ld_out, which, 0)
    if ok and vox and ((vox - 1) * max(ld_in, ld_out) + max(cin, cout)) * 2 >= BF16_SPAN_LIMIT:
        note_fallback(("conv3d>2GB", cin, cout, kt, kh, kw),
                      f"conv3d {cin}->{cout} k{kt}{kh}{kw} over {vox} voxels spans >= 2 GB: the bf16 MFMA kernels (32-bit buffer offsets) "
                      "decline it, the fp32 generic kernels run instead (several times slower) -- split the batch to stay on the fast path")
        return False
    return ok


_FORCE_GENERIC = [False]


def force_generic_conv(on):
    """Test hook: route every conv through the generic fp32-matrix-core path."""
    _FORCE_GENERIC[0] = bool(on)
    lib().vvae_conv3d_force_generic(1 if on else 0)


def _conv_cost(name, dims, esz, price=None):
    """-> (launch tag, algorithmic bytes, FLOPs) of a conv launch ("fwd", "dgrad" or "wgrad") for ops.TIMER.  ``price``: (Cin, Cout) the
    layer really has when its tensors are zero-padded to the kernels' 16-channel granule: the algorithmic bytes / FLOPs bench.py quotes
    are those of the true layer, not of the padded launch."""
    n, t, h, w, cin, cout, kt, kh, kw = dims
    ck, co = (cout, cin) if name == "dgrad" else (cin, cout)
    vox = n * t * h * w
    pci, pco = price if price is not None else (cin, cout)
    return f"conv3d_{name} {ck}->{co} k{kt}{kh}{kw} @{h}x{w}", vox * (pci + pco) * esz, 2 * vox * kt * kh * kw * pci * pco


def _conv_bf16(x, ldx, kernel, bias, dgrad, out=None, x2=None, ysplit=0, gn=None, packed=None, k_real=0, price=None):
    """The one launch path of the bf16 matrix-core conv: forward (dgrad=0) or input gradient (dgrad=1, ``x`` is dy) of ``kernel`` (fp32,
    (kt, kh, kw, Cin, Cout)) over ``x`` with row pitch ``ldx`` (from rows()); the caller knows the kernels take the layer.
    ``x2``: the forward's input is concat([x, x2], channels) held as two tensors.  ``ysplit``: the input gradient leaves as two dense
    tensors, its first ``ysplit`` channels and the rest.  ``gn``: (groups, rows per sample): also the GroupNorm partials of the rounded
    outputs.  ``packed``: the weights packed for the whole step (conv3d_prepack), else they are packed here.  ``k_real``: how many of
    the layer's K channels are not zero padding (0 = all): the kernels that know the count skip the padded part of the product (the
    12-of-16 channel patch mixer).  ``price``: see _conv_cost.  -> (out, second output or None, partials or None)."""
    n, t, h, w, _ = x.shape
    kt, kh, kw, cin, cout = kernel.shape
    dims = (n, t, h, w, cin, cout, kt, kh, kw)
    co = cin if dgrad else cout
    flags = dgrad | (int(k_real) << 8)                               # include/vvae_hip.h: vvae_conv3d_fwd_bf16
    if packed is not None:
        ws, wsb = packed, packed.numel()
    else:
        ws, wsb = _ws(lib().vvae_conv3d_bf16_ws_bytes(*dims, dgrad), x.device)
        check(lib().vvae_conv3d_pack_bf16(_p(kernel), _p(ws), wsb, cin, cout, kt, kh, kw, flags, _stream()), "vvae_conv3d_pack_bf16")
    if out is None:
        out = torch.empty((n, t, h, w, ysplit or co), dtype=x.dtype, device=x.device)
    out2 = torch.empty((n, t, h, w, co - ysplit), dtype=x.dtype, device=x.device) if ysplit else None
    groups, nblk = gn if gn is not None else (0, 0)
    part = torch.empty((n, nblk, groups, 2), dtype=torch.float32, device=x.device) if nblk else None
    ldo = out.stride(-2)
    if x2 is not None or out2 is not None:
        x2, ldx2 = rows(x2) if x2 is not None else (None, 0)
        fn, args = lib().vvae_conv3d_fwd_bf16_cat2, (_p(x), ldx, _p(x2), ldx2, _p(bias), _p(out), ldo, _p(out2), co - ysplit if ysplit else 0,
                                                     ysplit or x.shape[-1], *dims, dgrad, _p(ws), wsb, _p(part), groups, _stream())
    elif part is not None:
        fn, args = lib().vvae_conv3d_fwd_bf16_gn, (_p(x), ldx, None, _p(bias), _p(out), ldo, *dims, 1, _p(ws), wsb, _p(part), groups, _stream())
    else:
        fn, args = lib().vvae_conv3d_fwd_bf16, (_p(x), ldx, None, _p(bias), _p(out), ldo, *dims, flags, 1, _p(ws), wsb, _stream())
    tag, alg, flops = _conv_cost("dgrad" if dgrad else "fwd", dims, x.element_size(), price)
    check(_launch(tag, alg, flops, "conv3d_bf16_roll_kernel|conv3d_bf16_deep_kernel", lambda: fn(*args)), fn.__name__)
    return out, out2, part


def _conv_fwd_like(x, kernel, bias, out, dgrad, packed=None, k_real=0, price=None):
    """conv3d_fwd_raw (dgrad=0) and conv3d_dgrad_raw (dgrad=1, ``x`` is dy): the bf16 matrix-core launch where _bf16_fast says so, else
    the dispatcher's generic kernels.  ``packed``, ``k_real``, ``price``: see _conv_bf16."""
    x, ldx = rows(x)
    n, t, h, w, ck = x.shape
    kt, kh, kw, cin, cout = kernel.shape
    assert ck == (cout if dgrad else cin), (ck, cin, cout)
    if out is None:
        out = torch.empty((n, t, h, w, cin if dgrad else cout), dtype=x.dtype, device=x.device)
    ldo = out.stride(-2)
    dt = _dt(x)
    if _bf16_fast(cin, cout, kt, kh, kw, ldx, ldo, dgrad, dt, n * t * h * w):
        return _conv_bf16(x, ldx, kernel, bias, dgrad, out, packed=packed, k_real=k_real, price=price)[0]
    dims = (n, t, h, w, cin, cout, kt, kh, kw)
    name = "dgrad" if dgrad else "fwd"
    tag, alg, flops = _conv_cost(name, dims, x.element_size(), price)
    if dgrad:
        call = lambda: lib().vvae_conv3d_dgrad(_p(x), ldx, _p(kernel), _p(out), ldo, *dims, dt, None, 0, _stream())
    else:
        call = lambda: lib().vvae_conv3d_fwd(_p(x), ldx, _p(kernel), _p(bias), _p(out), ldo, *dims, dt, None, 0, _stream())
    check(_launch(tag, alg, flops, "conv3d_f32mfma_kernel", call), "vvae_conv3d_" + name)
    return out


# --------------------------------------------------------------------------------------------- grouped zero-padding of small weights
def _pad_group_launch(srcs, dsts, rows_, s01, d01, unpad):
    n = len(srcs)
    VP, LA, IA = ctypes.c_void_p * n, ctypes.c_long * n, ctypes.c_int * n
    check(lib().vvae_pad_last2_grouped(VP(*[t.data_ptr() for t in srcs]), VP(*[t.data_ptr() for t in dsts]), LA(*rows_),
                                       IA(*[a for a, _ in s01]), IA(*[b for _, b in s01]), IA(*[a for a, _ in d01]), IA(*[b for _, b in d01]),
                                       n, 1 if unpad else 0, _stream()), "vvae_pad_last2_grouped")


def _last2(shape):
    return (shape[-2], shape[-1]) if len(shape) >= 2 else (1, shape[-1])


class _PadLast2Group(torch.autograd.Function):
    """Zero-pad the last two dims of up to 8 small fp32 parameters in one launch (vvae_pad_last2_grouped); the backward cuts the padded
    gradients back in one launch too -- inside ``deferred_wgrad`` straight into the parameters' slots of the flat gradient buffer."""

    @staticmethod
    def forward(ctx, targets, *srcs):
        ctx.params = srcs
        ctx.targets = targets
        s32 = [_f32(t) for t in srcs]
        outs = [torch.empty(tuple(t.shape[:-len(tg)]) + tuple(tg), dtype=torch.float32, device=t.device) for t, tg in zip(s32, targets)]
        s01 = [_last2(t.shape) for t in s32]
        d01 = [_last2(o.shape) for o in outs]
        _pad_group_launch(s32, outs, [t.numel() // (a * b) for t, (a, b) in zip(s32, s01)], s01, d01, False)
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        q = WGRAD_QUEUE[0]
        todo, res = [], []
        for p, g in zip(ctx.params, gs):
            if g is None:
                res.append(None)
                continue
            g = g.to(torch.float32).contiguous()
            direct = q is not None and getattr(p, "gview", None) is not None and p.dtype == torch.float32
            dst = p.gview.view(p.shape) if direct else torch.empty(p.shape, dtype=torch.float32, device=g.device)
            todo.append((g, dst, p, direct))
            res.append(None if direct else dst)
        if todo:
            s01 = [_last2(d.shape) for _, d, _, _ in todo]
            d01 = [_last2(g.shape) for g, _, _, _ in todo]
            _pad_group_launch([g for g, _, _, _ in todo], [d for _, d, _, _ in todo],
                              [d.numel() // (a * b) for (_, d, _, _), (a, b) in zip(todo, s01)], s01, d01, True)
            for _, _, p, direct in todo:
                if direct:
                    q.opt.mark_external(p)
        return (None,) + tuple(r if r is None else r.to(p.dtype) for r, p in zip(res, ctx.params))


def pad_last2_group(tensors, targets):
    """-> zero-padded fp32 copies of ``tensors`` (GPU parameters): ``targets[i]`` is the new size of the last two dims (one dim for a
    vector).  One launch forward, one backward, however many tensors (<= 8)."""
    return _PadLast2Group.apply(tuple(tuple(t) for t in targets), *tensors)


# --------------------------------------------------------------------------------------------- Conv3d
def conv3d_fwd_raw(x, kernel, bias, out=None, packed=None, k_real=0, price=None):
    return _conv_fwd_like(x, kernel, bias, out, 0, packed, k_real, price)


def conv3d_dgrad_raw(dy, kernel, out=None, packed=None, k_real=0, price=None):
    return _conv_fwd_like(dy, kernel, None, out, 1, packed, k_real, price)


class ConvPack:
    """Packed bf16 weight fragments of one conv layer for one optimizer step: ``fwd`` and ``dgrad`` are uint8 views of one buffer."""
    __slots__ = ("fwd", "dgrad")

    def __init__(self, fwd, dgrad):
        self.fwd, self.dgrad = fwd, dgrad


def conv3d_prepack(kernels, reals=None):
    """Pack the weights of every conv layer of a network -- forward and flipped input-gradient forms -- in ONE launch
    (vvae_conv3d_pack_grouped_bf16).  ``kernels``: fp32 GPU tensors (3, kh, kw, Cin, Cout); -> list of ConvPack (None for a layer
    the bf16 matrix-core kernels do not take).  Weights change once per optimizer step; packing per call was 28 launches a step.
    ``reals``: per kernel None or (real Cin, real Cout) of a zero-padded layer (conv3d's ``real``)."""
    reals = reals if reals is not None else [None] * len(kernels)
    specs, sizes = [], []
    for k in kernels:
        kt, kh, kw, cin, cout = k.shape
        ok = (k.is_cuda and k.dtype == torch.float32 and kt == 3 and kh == kw and kh in (3, 7) and not _FORCE_GENERIC[0]
              and lib().vvae_conv3d_bf16_supported(cin, cout, kt, kh, kw, 8, 8, 0, 0) == 1
              and lib().vvae_conv3d_bf16_supported(cin, cout, kt, kh, kw, 8, 8, 1, 0) == 1)
        specs.append(ok)
        if ok:
            for which in (0, 1):
                sizes.append((lib().vvae_conv3d_bf16_ws_bytes(1, 1, 1, 1, cin, cout, kt, kh, kw, which) + 255) // 256 * 256)
    if not sizes:
        return [None] * len(kernels)
    buf = torch.empty(sum(sizes), dtype=torch.uint8, device=kernels[0].device)
    packs, off, ent = [], 0, []
    it = iter(sizes)
    for k, ok, real in zip(kernels, specs, reals):
        if not ok:
            packs.append(None)
            continue
        views = []
        for which in (0, 1):
            nb = next(it)
            v = buf[off:off + nb]
            off += nb
            views.append(v)
            ent.append((k.contiguous(), v, which | ((int(real[which]) << 8) if real is not None else 0)))
        packs.append(ConvPack(views[0], views[1]))
    for i0 in range(0, len(ent), 64):
        e = ent[i0:i0 + 64]
        n = len(e)
        VP, IA, SA = ctypes.c_void_p * n, ctypes.c_int * n, ctypes.c_size_t * n
        check(lib().vvae_conv3d_pack_grouped_bf16(VP(*[k.data_ptr() for k, _, _ in e]), VP(*[v.data_ptr() for _, v, _ in e]),
                                                  SA(*[v.numel() for _, v, _ in e]), IA(*[k.shape[3] for k, _, _ in e]),
                                                  IA(*[k.shape[4] for k, _, _ in e]), IA(*[k.shape[1] for k, _, _ in e]),
                                                  IA(*[w for _, _, w in e]), n, _stream()), "vvae_conv3d_pack_grouped_bf16")
    return packs


def conv3d_wgrad_raw(x, dy, kshape, want_bias=True, dw_out=None, db_out=None, price=None, x2=None):
    """-> (dw, db) fp32; dw_out / db_out: contiguous fp32 buffers to overwrite instead of fresh ones (flat-buffer slots).  ``x2``: the
    layer's input is concat([x, x2], channels) held as two tensors (conv3d_cat2_ok: bf16 matrix-core kernels only)."""
    x, ldx = rows(x)
    dy, lddy = rows(dy)
    n, t, h, w, _ = x.shape
    kt, kh, kw, cin, cout = kshape
    dims = (n, t, h, w, cin, cout, kt, kh, kw)
    dw = dw_out if dw_out is not None else torch.empty(kshape, dtype=torch.float32, device=x.device)
    db = (db_out if db_out is not None else torch.empty((cout,), dtype=torch.float32, device=x.device)) if want_bias else None
    if x2 is None:
        dt = _dt(x)
        ws, wsb = _ws(lib().vvae_conv3d_workspace_bytes(*dims, dt, 2), x.device)
        _bf16_fast(cin, cout, kt, kh, kw, ldx, lddy, 2, dt, n * t * h * w)   # says so once if the launch is too large for the bf16 kernels (the dispatcher then goes generic)
        fn, args = lib().vvae_conv3d_wgrad, (_p(x), ldx, _p(dy), lddy, _p(dw), _p(db), *dims, dt, _p(ws), wsb, _stream())
    else:
        x2, ldx2 = rows(x2)
        ws, wsb = _ws(lib().vvae_conv3d_wgrad_bf16_ws_bytes(*dims), x.device)
        fn, args = lib().vvae_conv3d_wgrad_bf16_cat2, (_p(x), ldx, _p(x2), ldx2, x.shape[-1], _p(dy), lddy, _p(dw), _p(db), *dims, _p(ws), wsb,
                                                       _stream())
    tag, alg, flops = _conv_cost("wgrad", dims, x.element_size(), price)
    check(_launch(tag, alg, flops, "conv3d_wgrad", lambda: fn(*args)), fn.__name__)
    return dw, db


def conv3d_gn_blocks(x, kernel, groups, x2=None):
    """Rows per sample of the GroupNorm partial buffer the rolling forward kernel can emit for this layer; 0: not eligible.  ``x2``: the
    input is concat([x, x2], channels) held as two tensors (the caller checked conv3d_cat2_ok)."""
    if not (x.is_cuda and x.dtype == torch.bfloat16) or _FORCE_GENERIC[0] or groups <= 0:
        return 0
    n, t, h, w, _ = x.shape
    kt, kh, kw, cin, cout = kernel.shape
    return lib().vvae_conv3d_gn_blocks(n, t, h, w, cin, cout, kt, kh, kw, 8 if x2 is not None else x.stride(-2), cout, groups)


def conv3d_fwd_gn_raw(x, kernel, bias, groups, nblk, packed=None, price=None):
    """conv3d_fwd_raw + the per-(sample, workgroup, group) sums of the rounded outputs: -> (y, part (n, nblk, groups, 2) fp32)."""
    x, ldx = rows(x)
    y, _, part = _conv_bf16(x, ldx, kernel, bias, 0, gn=(groups, nblk), packed=packed, price=price)
    return y, part


def _conv_wgrad(ctx, x, dy, k32, x2=None):
    """Weight and bias gradient of a conv node (_Conv3d, _PointwiseAdd) -> (dw, db).  Inside ops.deferred_wgrad, when the kernel (and the
    bias, if the layer has one) owns a slot of the flat gradient buffer and needs its gradient, the slab-reduce kernel overwrites those
    slots directly: no gradient tensor, no landing copy (and no clone by autograd.grad inside a captured graph) -> (None, None)."""
    q = WGRAD_QUEUE[0]
    kp, bp = ctx.kparam, ctx.bparam
    kt, kh, kw, cin, cout = k32.shape
    # _bf16_fast: the generic kernels behind the dispatcher take no destination of the caller's; the two-tensor form runs on the bf16
    # kernels or not at all, so there is nothing to ask
    if (q is not None and ctx.needs_input_grad[1] and getattr(kp, "gview", None) is not None and kp.dtype == torch.float32
            and (bp is None or (ctx.needs_input_grad[2] and getattr(bp, "gview", None) is not None and bp.dtype == torch.float32))
            and (x2 is not None or _bf16_fast(cin, cout, kt, kh, kw, x.stride(-2), dy.stride(-2), 2, _dt(x), x.numel() // cin))):
        q.claim(kp)
        conv3d_wgrad_raw(x, dy, tuple(k32.shape), bp is not None, kp.gview, bp.gview if bp is not None else None, ctx.price, x2)
        q.opt.mark_external(kp)
        if bp is not None:
            q.opt.mark_external(bp)
        return None, None
    dw, db = conv3d_wgrad_raw(x, dy, tuple(k32.shape), ctx.has_bias, price=ctx.price, x2=x2)
    return dw.to(ctx.kdtype), db


class _Conv3d(torch.autograd.Function):
    """``x2``: the conv runs over concat([x, x2], -1) without the concatenated tensor (reference train/unet.py:79-81; conv3d_cat2_ok)."""

    @staticmethod
    def forward(ctx, x, kernel, bias, gn_groups=0, gn_blocks=0, pack=None, real=None, price=None, x2=None):
        k32 = _f32(kernel)
        b32 = _f32(bias) if bias is not None else None
        ctx.save_for_backward(*((x, k32) if x2 is None else (x, k32, x2)))
        ctx.real = real                                  # (real Cin, real Cout) of a zero-padded layer, or None
        ctx.price = price if price is not None else real    # (Cin, Cout) the roofline accounting uses (_conv_cost)
        ctx.has_bias = bias is not None
        ctx.kdtype = kernel.dtype
        ctx.kparam, ctx.bparam = kernel, bias            # for ops.deferred_wgrad: where the gradient may be written directly
        ctx.pack = pack                                  # this step's packed weights (conv3d_prepack), or None: pack per call
        pk = pack.fwd if pack is not None else None
        if x2 is not None:
            res = conv3d_cat2_fwd_raw(x, x2, k32, b32, gn_groups, gn_blocks, pk)
        elif gn_blocks:
            res = conv3d_fwd_gn_raw(x, k32, b32, gn_groups, gn_blocks, pk, ctx.price)
        else:
            res = conv3d_fwd_raw(x, k32, b32, packed=pk, k_real=real[0] if real is not None else 0, price=ctx.price)
        if gn_blocks:
            ctx.mark_non_differentiable(res[1])
            ctx.set_materialize_grads(False)             # no zero-filled gradient tensor for the partials in backward
        return res

    @staticmethod
    def backward(ctx, dy, dpart=None):
        dx, dw, db, dx2 = _Conv3d._backward(ctx, dy)
        return dx, dw, db, None, None, None, None, None, dx2

    @staticmethod
    def _backward(ctx, dy):
        x, k32, *x2 = ctx.saved_tensors
        x2 = x2[0] if x2 else None
        dy = dy.to(x.dtype)
        dx = dx2 = None
        pk = ctx.pack.dgrad if ctx.pack is not None else None
        if x2 is not None:
            if ctx.needs_input_grad[0] or ctx.needs_input_grad[8]:
                dx, dx2 = conv3d_cat2_dgrad_raw(dy, k32, x.shape[-1], pk)
        elif ctx.needs_input_grad[0]:
            dx = conv3d_dgrad_raw(dy, k32, packed=pk, k_real=ctx.real[1] if ctx.real is not None else 0, price=ctx.price)
        dw = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = _conv_wgrad(ctx, x, dy, k32, x2)
        return dx, dw, db, dx2


class _PointwiseAdd(torch.autograd.Function):
    """addend + conv1x1x1(x) in one launch (vvae_conv_pointwise_fwd_add): the decoder's ``coarse + UNet(features)`` (reference
    train/model.py:97) inside the product that ends the UNet.  Backward = _Conv3d's, and the gradient itself for the addend."""

    @staticmethod
    def forward(ctx, x, kernel, bias, addend):
        k32 = _f32(kernel)
        b32 = _f32(bias) if bias is not None else None
        ctx.save_for_backward(x, k32)
        ctx.real = ctx.price = ctx.pack = None
        ctx.has_bias = bias is not None
        ctx.kdtype = kernel.dtype
        ctx.kparam, ctx.bparam = kernel, bias
        xr, ldx = rows(x)
        ar, lda = rows(addend)
        cin, cout = k32.shape[-2], k32.shape[-1]
        out = torch.empty(addend.shape, dtype=x.dtype, device=x.device)
        vox = x.numel() // cin
        h, w = x.shape[-3], x.shape[-2]
        check(_launch(f"conv3d_fwd+add {cin}->{cout} k111 @{h}x{w}", vox * (cin + 2 * cout) * x.element_size(), 2 * vox * cin * cout, "pw_fwd_kernel",
                      lambda: lib().vvae_conv_pointwise_fwd_add(_p(xr), ldx, _p(k32), _p(b32), _p(ar), lda, _p(out), out.stride(-2), vox, cin, cout,
                                                                _dt(x), _stream())), "vvae_conv_pointwise_fwd_add")
        return out

    @staticmethod
    def backward(ctx, dy):
        dx, dw, db, _ = _Conv3d._backward(ctx, dy)
        return dx, dw, db, dy


class _PointwiseFork(torch.autograd.Function):
    """(conv1x1x1(x), x) from one node, for a tensor with a second consumer (the un-patchified features feed the coarse projection AND the
    UNet, reference train/layers.py:60-79, train/model.py:95-97): the other consumer's gradient reaches THIS backward and is added inside
    the input-gradient launch (vvae_conv_pointwise_dgrad_add) instead of by the engine's 134 MB accumulation launch."""

    @staticmethod
    def forward(ctx, x, kernel, bias):
        k32 = _f32(kernel)
        b32 = _f32(bias) if bias is not None else None
        ctx.save_for_backward(x, k32)
        ctx.has_bias = bias is not None
        ctx.kdtype = kernel.dtype
        ctx.set_materialize_grads(False)
        return conv3d_fwd_raw(x, k32, b32), x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dother):
        x, k32 = ctx.saved_tensors
        if dy is None:
            return dother, None, None
        dy = dy.to(x.dtype)
        xr, ldx = rows(x)
        dyr, lddy = rows(dy)
        cin, cout = k32.shape[-2], k32.shape[-1]
        vox = xr.numel() // cin
        dx = torch.empty(xr.shape, dtype=xr.dtype, device=xr.device)
        ad, lda = (None, 0) if dother is None else rows(dother.to(x.dtype))
        check(lib().vvae_conv_pointwise_dgrad_add(_p(dyr), lddy, _p(k32), _p(ad), lda, _p(dx), dx.stride(-2), vox, cin, cout, _dt(xr), _stream()),
              "vvae_conv_pointwise_dgrad_add")
        dw, db = conv3d_wgrad_raw(x, dy, tuple(k32.shape), ctx.has_bias)
        return dx, dw.to(ctx.kdtype), db


def conv3d_pointwise_fork_ok(x, kernel):
    kt, kh, kw, cin, cout = kernel.shape
    return (x.is_cuda and not _FORCE_GENERIC[0] and x.dtype in DT and x.shape[-1] == cin and x.is_contiguous()
            and lib().vvae_conv_pointwise_supported(cin, cout, kt, kh, kw, x.stride(-2), DT[x.dtype], _p(x)) == 1)


def conv3d_pointwise_fork(x, kernel, bias):
    """-> (conv3d(x, kernel (1,1,1,Cin,Cout), bias), x): use the returned x for the tensor's other consumer, whose gradient then joins inside
    the projection's input-gradient launch."""
    return _PointwiseFork.apply(x, kernel, bias)


def conv3d_pointwise_add_ok(x, kernel, addend):
    kt, kh, kw, cin, cout = kernel.shape
    return (x.is_cuda and not _FORCE_GENERIC[0] and x.dtype == addend.dtype and x.dtype in DT and x.shape[-1] == cin
            and addend.shape == (*x.shape[:-1], cout) and x.stride(-1) == 1 and addend.stride(-1) == 1
            and lib().vvae_conv_pointwise_supported(cin, cout, kt, kh, kw, x.stride(-2), DT[x.dtype], _p(x)) == 1)


def conv3d_pointwise_add(x, kernel, bias, addend):
    """addend + conv3d(x, kernel (1,1,1,Cin,Cout), bias), one pass and one rounding."""
    return _PointwiseAdd.apply(x, kernel, bias, addend)


# ---- conv over concat([xa, xb], channels) held as two dense tensors (the decoder's 16 + 16 channel level) ----
def conv3d_cat2_shape_ok(c_split, kernel_shape):
    """The rolling bf16 kernels take a (kt, kh, kw, Cin, Cout) layer with its input in two tensors, the first of ``c_split`` channels
    (forward, input gradient and weight gradient)."""
    kt, kh, kw, cin, cout = kernel_shape
    return not _FORCE_GENERIC[0] and lib().vvae_conv3d_cat2_supported(cin, cout, c_split, kt, kh, kw) == 1


def conv3d_cat2_ok(xa, xb, kernel):
    """conv3d_cat2_shape_ok for these two bf16 GPU tensors."""
    return (xa.is_cuda and xa.dtype == torch.bfloat16 and xb.dtype == torch.bfloat16 and xa.shape[:-1] == xb.shape[:-1]
            and kernel.shape[3] == xa.shape[-1] + xb.shape[-1] and conv3d_cat2_shape_ok(xa.shape[-1], kernel.shape))


def conv3d_cat2_fwd_raw(xa, xb, kernel, bias, groups=0, nblk=0, packed=None):
    """-> y, or (y, part) with the GroupNorm partials when nblk > 0 (conv3d_fwd_gn_raw)."""
    xa, lda = rows(xa)
    y, _, part = _conv_bf16(xa, lda, kernel, bias, 0, x2=xb, gn=(groups, nblk), packed=packed)
    return (y, part) if nblk else y


def conv3d_cat2_dgrad_raw(dy, kernel, ca, packed=None):
    """-> (dxa, dxb): the input gradient's first ``ca`` channels and the rest, each dense."""
    dy, lddy = rows(dy)
    return _conv_bf16(dy, lddy, kernel, None, 1, ysplit=ca, packed=packed)[:2]


def conv3d_cat2_wgrad_raw(xa, xb, dy, kshape, want_bias=True, dw_out=None, db_out=None):
    return conv3d_wgrad_raw(xa, dy, kshape, want_bias, dw_out, db_out, x2=xb)


def conv3d(x, kernel, bias=None, pack=None, real=None):
    """NDHWC Conv3d, SAME, stride 1 (nnx.Conv; reference train/unet.py:13-21).  ``pack``: from conv3d_prepack.  ``real``: (Cin, Cout)
    actually in use when x / kernel / bias are zero-padded to the kernels' channel granule (must match the prepack call's)."""
    return _Conv3d.apply(x, kernel, bias, 0, 0, pack, real)


def conv3d_with_gn_stats(x, kernel, bias, groups, pack=None, price=None, x2=None):
    """-> (conv3d(x), stats) where stats is None or (partial sums, rows per sample) for group_norm_silu(..., stats=...): on
    the rolling bf16 kernel the conv's epilogue also sums its rounded outputs per GroupNorm group, so the norm behind it
    (reference train/unet.py:13-23) skips its own statistics pass over the tensor.  ``x2``: the conv runs over concat([x, x2], -1)
    held as two tensors; the caller checked conv3d_cat2_ok."""
    nblk = conv3d_gn_blocks(x, kernel, groups, x2) if bias is not None else 0
    if not nblk:
        return _Conv3d.apply(x, kernel, bias, 0, 0, pack, None, price, x2), None
    y, part = _Conv3d.apply(x, kernel, bias, groups, nblk, pack, None, price, x2)
    return y, (part, nblk)


def unpatch_pad(src, dst, frames, h, w, p, cu, c, backward):
    """PatchUnEmbedding's rearrange fused with the channel padding (layers._UnpatchPad); bf16 GPU tensors, contiguous."""
    fn = lib().vvae_unpatch_pad_bwd if backward else lib().vvae_unpatch_pad_fwd
    check(fn(_p(src), _p(dst), frames, h, w, p, cu, c, _dt(src), _stream()), "vvae_unpatch_pad")


# --------------------------------------------------------------------------------------------- GroupNorm + SiLU
def gn_stats_raw(x, groups):
    x, ldx = rows(x)
    n, c = x.shape[0], x.shape[-1]
    s = x.numel() // (n * c)
    sums = torch.empty((n, groups, 2), dtype=torch.float64, device=x.device)
    part = torch.empty((lib().vvae_gn_part_floats(n, s, c),), dtype=torch.float32, device=x.device)
    check(lib().vvae_gn_stats(_p(x), ldx, n, s, c, groups, _p(sums), _p(part), _dt(x), _stream()), "vvae_gn_stats")
    return sums


def gn_silu_fwd_raw(x, sums, scale, bias, groups, eps, out=None):
    x, ldx = rows(x)
    n, c = x.shape[0], x.shape[-1]
    s = x.numel() // (n * c)
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    check(lib().vvae_gn_silu_fwd(_p(x), ldx, _p(out), out.stride(-2), _p(sums), _p(scale), _p(bias), n, s, c, groups, eps,
                                 _dt(x), _stream()), "vvae_gn_silu_fwd")
    return out


def gn_silu_bwd_raw(x, dy, sums, scale, bias, groups, eps, out=None):
    x, ldx = rows(x)
    dy, lddy = rows(dy)
    n, c = x.shape[0], x.shape[-1]
    s = x.numel() // (n * c)
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    csum = torch.empty((n, c, 2), dtype=torch.float64, device=x.device)
    part = torch.empty((lib().vvae_gn_part_floats(n, s, c),), dtype=torch.float32, device=x.device)
    dg = torch.empty((c,), dtype=torch.float32, device=x.device)
    db = torch.empty((c,), dtype=torch.float32, device=x.device)
    check(lib().vvae_gn_silu_bwd(_p(x), ldx, _p(dy), lddy, _p(out), out.stride(-2), _p(sums), _p(scale), _p(bias), _p(csum),
                                 _p(part), _p(dg), _p(db), n, s, c, groups, eps, _dt(x), _stream()), "vvae_gn_silu_bwd")
    return out, dg, db


GN_POOL_FWD_FUSED = [True]       # test / A-B hook: False = GroupNorm + SiLU, then the pool as a launch of its own


def gn_silu_pool_ok(x, groups, out=None):
    """May group_norm_silu(..., pool=True) run?  (vvae_gn_silu_pool_fwd: 5-D NDHWC on the GPU, even H and W, 16-byte channel vectors.)"""
    if not (x.is_cuda and x.dim() == 5 and x.dtype in DT and x.stride(-1) == 1) or _FORCE_GENERIC[0] or not GN_POOL_FWD_FUSED[0]:
        return False
    h, w, c = x.shape[-3], x.shape[-2], x.shape[-1]
    ldy = out.stride(-2) if out is not None else c
    return lib().vvae_gn_silu_pool_supported(h, w, c, groups, x.stride(-2), ldy, c, DT[x.dtype]) == 1


class _GnSilu(torch.autograd.Function):
    """silu(GroupNorm(x)).  ``pool``: also return its (1,2,2) max-pool from the same launch (the encoder levels' conv2 -> GN -> SiLU ->
    max_pool, reference train/unet.py:44-51); the backward then first routes the pool's gradient to the window maxima and adds the skip's
    (maxpool_bwd_raw, as ops.max_pool_fork did) and runs the GroupNorm backward on the sum."""

    @staticmethod
    def forward(ctx, x, scale, bias, groups, eps, out=None, part=None, nblk=0, pool=False):
        s32, b32 = _f32(scale), _f32(bias)
        if part is not None:                             # the producing conv already summed its outputs (conv3d_with_gn_stats)
            sums = torch.empty((x.shape[0], groups, 2), dtype=torch.float64, device=x.device)
            check(lib().vvae_gn_finalize(_p(part), x.shape[0], nblk, groups, _p(sums), _stream()), "vvae_gn_finalize")
        else:
            sums = gn_stats_raw(x, groups)
        ctx.groups, ctx.eps, ctx.pdtype, ctx.pool = groups, eps, scale.dtype, bool(pool)
        ctx.set_materialize_grads(False)
        if not pool:
            ctx.save_for_backward(x, sums, s32, b32)
            return gn_silu_fwd_raw(x, sums, s32, b32, groups, eps, out)
        xr, ldx = rows(x)
        n, t, h, w, c = xr.shape
        y = out if out is not None else torch.empty(xr.shape, dtype=xr.dtype, device=xr.device)
        pooled = torch.empty((n, t, h // 2, w // 2, c), dtype=xr.dtype, device=xr.device)
        check(lib().vvae_gn_silu_pool_fwd(_p(xr), ldx, _p(y), y.stride(-2), _p(pooled), c, _p(sums), _p(s32), _p(b32), n, t, h, w, c, groups,
                                          eps, _dt(xr), _stream()), "vvae_gn_silu_pool_fwd")
        ctx.save_for_backward(x, sums, s32, b32, y)
        return y, pooled

    @staticmethod
    def backward(ctx, dy, dpool=None):
        if ctx.pool:
            x, sums, s32, b32, y = ctx.saved_tensors
            if dpool is not None:
                dy = maxpool_bwd_raw(y, dpool.to(y.dtype), None if dy is None else dy.to(y.dtype))
        else:
            x, sums, s32, b32 = ctx.saved_tensors
        if dy is None:
            return (None,) * 9
        dx, dg, db = gn_silu_bwd_raw(x, dy.to(x.dtype), sums, s32, b32, ctx.groups, ctx.eps)
        return dx, dg.to(ctx.pdtype), db.to(ctx.pdtype), None, None, None, None, None, None


def group_norm_silu(x, scale, bias, groups, eps=1e-6, out=None, stats=None, pool=False):
    """silu(GroupNorm(x)) over (t,h,w,C/G) per sample (reference train/unet.py:22-23,28-29).  ``out``: a channel slice of a
    wider NDHWC buffer to write into (see join_channels).  ``stats``: from conv3d_with_gn_stats.  ``pool`` (gn_silu_pool_ok): -> (y, max_pool_1x2x2(y))."""
    if stats is not None:
        return _GnSilu.apply(x, scale, bias, groups, eps, out, stats[0], stats[1], pool)
    return _GnSilu.apply(x, scale, bias, groups, eps, out, None, 0, pool)


# --------------------------------------------------------------------------------------------- max-pool (1,2,2)
def maxpool_fwd_raw(x, out=None):
    x, ldx = rows(x)
    n, t, h, w, c = x.shape
    if out is None:
        out = torch.empty((n, t, h // 2, w // 2, c), dtype=x.dtype, device=x.device)
    check(lib().vvae_maxpool_1x2x2_fwd(_p(x), ldx, _p(out), out.stride(-2), n * t, h, w, c, _dt(x), _stream()),
          "vvae_maxpool_1x2x2_fwd")
    return out


def maxpool_bwd_raw(x, dpool, dskip=None, out=None):
    x, ldx = rows(x)
    dpool, lddp = rows(dpool)
    ldds = 0
    if dskip is not None:
        dskip, ldds = rows(dskip)
    n, t, h, w, c = x.shape
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    check(lib().vvae_maxpool_1x2x2_bwd(_p(x), ldx, _p(dpool), lddp, _p(dskip), ldds, _p(out), out.stride(-2), n * t, h, w, c,
                                       _dt(x), _stream()), "vvae_maxpool_1x2x2_bwd")
    return out


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return maxpool_fwd_raw(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return maxpool_bwd_raw(x, dy.to(x.dtype))


def max_pool_1x2x2(x):
    """nnx.max_pool(x, (1,2,2), strides=(1,2,2)) (reference train/unet.py:50)."""
    return _MaxPool.apply(x)


class _MaxPoolFork(torch.autograd.Function):
    """DownBlock3D's ``return max_pool(x), x`` (reference train/unet.py:50-51) as one node: the second output is x itself, so the
    gradient of the skip connection arrives HERE and is added inside the pool-backward kernel (its ``dskip`` operand, any row
    pitch) instead of by a separate add launch over the largest activations of the network."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        ctx.set_materialize_grads(False)
        return maxpool_fwd_raw(x), x.view_as(x)

    @staticmethod
    def backward(ctx, dpool, dskip):
        (x,) = ctx.saved_tensors
        if dpool is None:
            return dskip
        return maxpool_bwd_raw(x, dpool.to(x.dtype), None if dskip is None else dskip.to(x.dtype))


def max_pool_fork(x):
    """-> (max_pool_1x2x2(x), x) with the skip gradient folded into the pool's backward kernel."""
    return _MaxPoolFork.apply(x)


# --------------------------------------------------------------------------------------------- ConvTranspose (1,2,2)
def _convt_fast(x, cin, cout, ld_in, ld_out):
    return (x.dtype == torch.bfloat16 and not _FORCE_GENERIC[0]
            and lib().vvae_convt_bf16_supported(cin, cout, ld_in, ld_out) == 1)


def _convt_bf16(x, ldx, kernel, bias, out, nt, h, w, cin, cout, dgrad, packed=None):
    """bf16 MFMA ConvTranspose (h, w = low resolution).  dgrad=1: x is dy at 2h x 2w, out is dx at h x w.
    ``packed``: this direction's weights already packed for the whole step (convt_prepack)."""
    if packed is not None:
        ws, wsb, flags = packed, packed.numel(), dgrad | 0x100
    else:
        wsb = lib().vvae_convt_bf16_ws_bytes(cin, cout)
        ws, wsb = _ws(wsb, x.device)
        flags = dgrad
    vox = nt * h * w
    alg = vox * (cin + 4 * cout) * 2
    tag = f"convt_{'dgrad' if dgrad else 'fwd'} {cin}->{cout} @{h}x{w}"
    check(_launch(tag, alg, 2 * vox * 4 * cin * cout, "convt_bf16_kernel",
                  lambda: lib().vvae_convt_1x2x2_bf16(_p(x), ldx, _p(kernel), _p(bias), _p(out), out.stride(-2), nt, h, w, cin, cout,
                                                      flags, _p(ws), wsb, _stream())), "vvae_convt_1x2x2_bf16")
    return out


def convt_prepack(kernels):
    """Pack the forward and input-gradient forms of every ConvTranspose kernel (1, 2, 2, Cin, Cout) of a network in ONE launch
    (vvae_convt_pack_grouped_bf16) -> list of ConvPack (None where the bf16 matrix-core path does not take the layer)."""
    todo = [k for k in kernels if k.is_cuda and k.dtype == torch.float32 and not _FORCE_GENERIC[0]
            and lib().vvae_convt_bf16_supported(k.shape[-2], k.shape[-1], 8, 8) == 1]
    if not todo:
        return [None] * len(kernels)
    sizes = [(lib().vvae_convt_bf16_ws_bytes(k.shape[-2], k.shape[-1]) + 255) // 256 * 256 for k in todo]
    buf = torch.empty(2 * sum(sizes), dtype=torch.uint8, device=todo[0].device)
    packs, ent, off = {}, [], 0
    for k, nb in zip(todo, sizes):
        views = []
        for which in (0, 1):
            v = buf[off:off + nb]
            off += nb
            views.append(v)
            ent.append((k.contiguous(), v, which))
        packs[id(k)] = ConvPack(views[0], views[1])
    n = len(ent)
    VP, IA = ctypes.c_void_p * n, ctypes.c_int * n
    check(lib().vvae_convt_pack_grouped_bf16(VP(*[k.data_ptr() for k, _, _ in ent]), VP(*[v.data_ptr() for _, v, _ in ent]),
                                             IA(*[k.shape[-2] for k, _, _ in ent]), IA(*[k.shape[-1] for k, _, _ in ent]),
                                             IA(*[w for _, _, w in ent]), n, _stream()), "vvae_convt_pack_grouped_bf16")
    return [packs.get(id(k)) for k in kernels]


def convt_fwd_raw(x, kernel, bias, out=None, packed=None):
    x, ldx = rows(x)
    n, t, h, w, cin = x.shape
    cout = kernel.shape[-1]
    if out is None:
        out = torch.empty((n, t, 2 * h, 2 * w, cout), dtype=x.dtype, device=x.device)
    if _convt_fast(x, cin, cout, ldx, out.stride(-2)):
        return _convt_bf16(x, ldx, kernel, bias, out, n * t, h, w, cin, cout, 0, packed)
    check(lib().vvae_convt_1x2x2_fwd(_p(x), ldx, _p(kernel), _p(bias), _p(out), out.stride(-2), n * t, h, w, cin, cout,
                                     _dt(x), _stream()), "vvae_convt_1x2x2_fwd")
    return out


def convt_dgrad_raw(dy, kernel, out=None, packed=None):
    dy, lddy = rows(dy)
    n, t, h2, w2, cout = dy.shape
    cin = kernel.shape[-2]
    if out is None:
        out = torch.empty((n, t, h2 // 2, w2 // 2, cin), dtype=dy.dtype, device=dy.device)
    if _convt_fast(dy, cin, cout, lddy, out.stride(-2)):
        return _convt_bf16(dy, lddy, kernel, None, out, n * t, h2 // 2, w2 // 2, cin, cout, 1, packed)
    check(lib().vvae_convt_1x2x2_dgrad(_p(dy), lddy, _p(kernel), _p(out), out.stride(-2), n * t, h2 // 2, w2 // 2, cin, cout,
                                       _dt(dy), _stream()), "vvae_convt_1x2x2_dgrad")
    return out


def convt_wgrad_raw(x, dy, kshape):
    x, ldx = rows(x)
    dy, lddy = rows(dy)
    n, t, h, w, cin = x.shape
    cout = kshape[-1]
    dw = torch.empty(kshape, dtype=torch.float32, device=x.device)
    ws, wsb = _ws(lib().vvae_convt_1x2x2_wgrad_ws_bytes(n * t, h, w, cin, cout), x.device)
    check(lib().vvae_convt_1x2x2_wgrad(_p(x), ldx, _p(dy), lddy, _p(dw), n * t, h, w, cin, cout, _dt(x), _p(ws), wsb, _stream()),
          "vvae_convt_1x2x2_wgrad")
    return dw


def convt_wgrad_db_raw(x, dy, kshape):
    """-> (dw (1,2,2,Cin,Cout) fp32, db (Cout) fp32): one bf16 matrix-core launch pair where the layer qualifies, else the generic
    weight gradient plus a column sum."""
    x, ldx = rows(x)
    dy, lddy = rows(dy)
    n, t, h, w, cin = x.shape
    cout = kshape[-1]
    if (x.dtype == torch.bfloat16 and not _FORCE_GENERIC[0]
            and lib().vvae_convt_wgrad_bf16_supported(cin, cout, ldx, lddy) == 1):
        dw = torch.empty(kshape, dtype=torch.float32, device=x.device)
        db = torch.empty((cout,), dtype=torch.float32, device=x.device)
        wsb = lib().vvae_convt_wgrad_bf16_ws_bytes(n * t, h, w, cin, cout)
        ws, wsb = _ws(wsb, x.device)
        vox = n * t * h * w
        check(_launch(f"convt_wgrad {cin}->{cout} @{h}x{w}", vox * (cin + 4 * cout) * 2, 8 * vox * cin * cout, "convt_wgrad_bf16_kernel",
                      lambda: lib().vvae_convt_1x2x2_wgrad_bf16(_p(x), ldx, _p(dy), lddy, _p(dw), _p(db), n * t, h, w, cin, cout,
                                                                _p(ws), wsb, _stream())), "vvae_convt_1x2x2_wgrad_bf16")
        return dw, db
    return convt_wgrad_raw(x, dy, kshape), colsum_raw(dy)


def colsum_raw(x):
    x, ld = rows(x)
    c = x.shape[-1]
    out = torch.empty((c,), dtype=torch.float32, device=x.device)
    v = x.numel() // c
    part = torch.empty((lib().vvae_colsum_blocks(v), c), dtype=torch.float32, device=x.device)
    check(lib().vvae_colsum(_p(x), ld, v, c, _p(out), _p(part), _dt(x), _stream()), "vvae_colsum")
    return out


class _ConvT(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, bias, out=None, pack=None):
        k32, b32 = _f32(kernel), _f32(bias)
        ctx.save_for_backward(x, k32)
        ctx.kdtype = kernel.dtype
        ctx.pack = pack
        return convt_fwd_raw(x, k32, b32, out, pack.fwd if pack is not None else None)

    @staticmethod
    def backward(ctx, dy):
        x, k32 = ctx.saved_tensors
        dy = dy.to(x.dtype)
        dx = convt_dgrad_raw(dy, k32, packed=ctx.pack.dgrad if ctx.pack is not None else None) if ctx.needs_input_grad[0] else None
        dw, db = convt_wgrad_db_raw(x, dy, tuple(k32.shape))
        return dx, dw.to(ctx.kdtype), db.to(ctx.kdtype), None, None


def conv_transpose_1x2x2(x, kernel, bias, out=None, pack=None):
    """nnx.ConvTranspose((1,2,2), strides (1,2,2)) (reference train/unet.py:61-69).  ``out``: a channel slice of a wider
    NDHWC buffer to write into (see join_channels).  ``pack``: this step's packed weights (convt_prepack)."""
    return _ConvT.apply(x, kernel, bias, out, pack)


class _JoinChannels(torch.autograd.Function):
    """concat([a, b], -1) without the copy (reference train/unet.py:79): a and b ARE the two channel slices of ``buf`` -- their
    producers wrote them there through the kernels' row pitch -- so forward only re-labels the buffer and backward hands each
    producer its slice of the incoming gradient (a pitched view; every consumer takes a row pitch)."""

    @staticmethod
    def forward(ctx, a, b, buf):
        ca, cb = a.shape[-1], b.shape[-1]
        if (buf.shape[-1] != ca + cb or not buf.is_contiguous() or a.data_ptr() != buf.data_ptr()
                or b.data_ptr() != buf.data_ptr() + ca * buf.element_size() or a.stride() != buf.stride() or b.stride() != buf.stride()
                or a.shape[:-1] != buf.shape[:-1] or b.shape[:-1] != buf.shape[:-1]):
            raise VvaeError("join_channels: operands are not the channel slices of the joint buffer")
        ctx.ca = ca
        return buf.view_as(buf)

    @staticmethod
    def backward(ctx, g):
        return g[..., :ctx.ca], g[..., ctx.ca:], None


def join_channels(a, b, buf):
    return _JoinChannels.apply(a, b, buf)


_ROPE_TABS = {}


def _rope_tabs(cos, sin, dtype):
    """RoPE tables rounded ONCE to the activation dtype (the fused kernels take them pre-rounded; reference layers.py:113-114)."""
    if dtype == torch.float32:
        return cos, sin
    key = (cos.data_ptr(), sin.data_ptr(), dtype)
    hit = _ROPE_TABS.get(key)
    if hit is None or hit[0] is not cos or hit[1] is not sin:
        hit = (cos, sin, cos.to(dtype).to(torch.float32).contiguous(), sin.to(dtype).to(torch.float32).contiguous())
        _ROPE_TABS[key] = hit
    return hit[2], hit[3]


# --------------------------------------------------------------------------------------------- temporal attention core
ATTN_FORCE_GENERIC = [False]      # test hook: use the generic (any head_dim) kernels


class _TemporalAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, q_scale, k_scale, cos, sin, mask, mask_div, heads, eps, inner=1):
        qkv, ld = rows(qkv)
        dt = _dt(qkv)
        c3 = qkv.shape[-1]
        d = c3 // (3 * heads)
        if inner > 1:                      # (b, t, hw, C): sequences stride over frames, no transpose copies
            bsz, t, hw = qkv.shape[:3]
            assert hw == inner
            a = bsz * hw
        else:
            a, t = qkv.shape[:2]
        qs, ks = _f32(q_scale), _f32(k_scale)
        cos, sin = _rope_tabs(cos, sin, qkv.dtype)
        out = torch.empty(qkv.shape[:-1] + (heads * d,), dtype=qkv.dtype, device=qkv.device)
        fast = (not ATTN_FORCE_GENERIC[0]) and lib().vvae_temporal_attn_fast_supported(t, d, ld, heads * d, dt) == 1
        if inner > 1 and not fast:
            raise VvaeError("strided temporal attention needs the lane-per-frame kernels (head_dim 8/16/32/64)")
        lse = None
        nbytes = a * t * heads * d * 4 * qkv.element_size()
        if fast:
            lse = torch.empty((a * heads, t), dtype=torch.float32, device=qkv.device)
            check(_launch(f"temporal_attn_fwd T{t} D{d}", nbytes, 4 * a * heads * t * t * d, "tattn_fwd_fast",
                          lambda: lib().vvae_temporal_attn_fwd_fast(_p(qkv), ld, _p(out), heads * d, _p(lse), _p(qs), _p(ks), _p(cos),
                                                                    _p(sin), _p(mask), mask_div, inner, a, t, heads, d, eps, dt, _stream())),
                  "vvae_temporal_attn_fwd_fast")
        else:
            check(lib().vvae_temporal_attn_fwd(_p(qkv), ld, _p(out), heads * d, _p(qs), _p(ks), _p(cos), _p(sin), _p(mask), mask_div,
                                               a, t, heads, d, eps, dt, _stream()), "vvae_temporal_attn_fwd")
        ctx.qparam, ctx.kparam = q_scale, k_scale
        ctx.save_for_backward(qkv, qs, ks, cos, sin, mask, out, lse)
        ctx.args = (mask_div, heads, eps, q_scale.dtype, fast, inner, a, t)
        return out

    @staticmethod
    def backward(ctx, do):
        qkv, qs, ks, cos, sin, mask, out, lse = ctx.saved_tensors
        mask_div, heads, eps, pdtype, fast, inner, a, t = ctx.args
        qkv, ld = rows(qkv)
        do, lddo = rows(do.to(qkv.dtype))
        c3 = qkv.shape[-1]
        d = c3 // (3 * heads)
        dt = _dt(qkv)
        dqkv = torch.empty(qkv.shape, dtype=qkv.dtype, device=qkv.device)
        if fast:
            nblk = lib().vvae_temporal_attn_fast_blocks(a, t, heads, d, dt)
            part = torch.empty((nblk, 2 * d), dtype=torch.float32, device=qkv.device)
            nbytes = a * t * heads * d * 8 * qkv.element_size()
            check(_launch(f"temporal_attn_bwd T{t} D{d}", nbytes, 10 * a * heads * t * t * d, "tattn_bwd_fast",
                          lambda: lib().vvae_temporal_attn_bwd_fast(_p(qkv), ld, _p(out), heads * d, _p(do), lddo, _p(lse), _p(dqkv), c3,
                                                                    _p(qs), _p(ks), _p(cos), _p(sin), _p(mask), mask_div, inner,
                                                                    _p(part), a, t, heads, d, eps, dt, _stream())),
                  "vvae_temporal_attn_bwd_fast")
            dqs, dks = fold_partials(part, ctx.qparam, ctx.kparam, d)
            if dqs is None:
                return dqkv, None, None, None, None, None, None, None, None, None
        else:
            dqs = torch.empty((d,), dtype=torch.float32, device=qkv.device)
            dks = torch.empty((d,), dtype=torch.float32, device=qkv.device)
            ws, wsb = _ws(lib().vvae_temporal_attn_bwd_ws_bytes(a, heads, d), qkv.device)
            check(lib().vvae_temporal_attn_bwd(_p(qkv), ld, _p(do), lddo, _p(dqkv), c3, _p(qs), _p(ks), _p(cos), _p(sin), _p(mask),
                                               mask_div, _p(dqs), _p(dks), a, t, heads, d, eps, dt, _p(ws), wsb, _stream()),
                  "vvae_temporal_attn_bwd")
        return dqkv, dqs.to(pdtype), dks.to(pdtype), None, None, None, None, None, None, None


def temporal_attention_core(qkv, q_scale, k_scale, cos, sin, mask_u8, mask_div, heads, eps=1e-6, inner=1):
    """q_norm/k_norm -> RoPE -> masked softmax(QK^T/sqrt(D)) V (reference train/layers.py:159-170).

    inner = 1: qkv is (A, T, 3*heads*D), one sequence per leading index.  inner = hw: qkv is (b, T, hw, 3*heads*D) and
    sequence a = b*hw + i strides over frames (the FactoredAttention layout, no transposes).  Output has qkv's leading shape.
    mask_u8: uint8 (ceil(A/mask_div), T), 1 = attend, or None.  cos/sin: fp32 (>=T, D) RoPE tables.
    """
    return _TemporalAttn.apply(qkv, q_scale, k_scale, cos, sin, mask_u8, mask_div, heads, eps, inner)


def temporal_attention_fast_supported(t, d, c3, dtype):
    return dtype in DT and lib().vvae_temporal_attn_fast_supported(t, d, c3, c3 // 3, DT[dtype]) == 1


# --------------------------------------------------------------------------------------------- spatial attention (prep + library core)
def _tok_head(t, a, s):
    """(a, heads, s, d) gradient -> (tensor, token stride, head stride) with one uniform token stride; copies only if it must."""
    if not (t.stride(3) == 1 and t.stride(0) == s * t.stride(2)):
        t = t.transpose(1, 2).contiguous().transpose(1, 2)
    return t, t.stride(2), t.stride(1)


def qk_prep_fwd_raw(qkv, qs, ks, cos, sin, heads, eps=1e-6):
    """qkv (a, s, 3*heads*D) contiguous -> (a, s, 2*heads*D) = [rope(q_norm(q)) | rope(k_norm(k))] (no autograd)."""
    a, s, c3 = qkv.shape
    hd = c3 // 3
    d = hd // heads
    cos, sin = _rope_tabs(cos, sin, qkv.dtype)
    qk = torch.empty((a, s, 2 * hd), dtype=qkv.dtype, device=qkv.device)
    tokens = a * s
    check(_launch(f"qk_prep_fwd S{s} D{d}", tokens * 4 * hd * qkv.element_size(), 0, "qk_prep_fwd_kernel",
                  lambda: lib().vvae_qk_prep_fwd(_p(qkv), c3, _p(qk), 2 * hd, _p(qs), _p(ks), _p(cos), _p(sin), tokens, s, heads, d,
                                                 eps, _dt(qkv), _stream())), "vvae_qk_prep_fwd")
    return qk


def qk_prep_bwd_raw(qkv, dq, dk, dv, qs, ks, cos, sin, heads, eps=1e-6, params=None):
    """dq, dk, dv: (a, heads, s, D) gradients (any strides) -> (dqkv (a, s, 3*heads*D), dq_scale (D), dk_scale (D)) (no autograd)."""
    a, s, c3 = qkv.shape
    hd = c3 // 3
    d = hd // heads
    dq, dq_ts, dq_hs = _tok_head(dq, a, s)
    dk, dk_ts, dk_hs = _tok_head(dk, a, s)
    dv, dv_ts, dv_hs = _tok_head(dv, a, s)
    cos, sin = _rope_tabs(cos, sin, qkv.dtype)
    tokens = a * s
    dqkv = torch.empty((a, s, c3), dtype=qkv.dtype, device=qkv.device)
    nblk = lib().vvae_qk_prep_blocks(tokens, heads, d)
    part = torch.empty((nblk, 2, d), dtype=torch.float32, device=qkv.device)
    check(_launch(f"qk_prep_bwd S{s} D{d}", tokens * 8 * hd * qkv.element_size(), 0, "qk_prep_bwd_kernel",
                  lambda: lib().vvae_qk_prep_bwd(_p(qkv), c3, _p(dq), dq_ts, dq_hs, _p(dk), dk_ts, dk_hs, _p(dv), dv_ts, dv_hs,
                                                 _p(dqkv), c3, _p(qs), _p(ks), _p(cos), _p(sin), _p(part), tokens, s, heads, d, eps,
                                                 _dt(qkv), _stream())), "vvae_qk_prep_bwd")
    g0, g1 = fold_partials(part, params[0], params[1], d) if params is not None else fold_partials(part, None, None, d)
    return dqkv, g0, g1


SPATIAL_FORCE_LIBRARY_CORE = [False]      # test hook: keep the prep kernels + library flash core even where the fused kernels apply


def spatial_attn_fused_supported(qkv, heads):
    a, s, c3 = qkv.shape
    return (qkv.is_cuda and qkv.dtype == torch.bfloat16
            and lib().vvae_spatial_attn_supported(s, c3 // (3 * heads), DT[qkv.dtype]) == 1)


def spatial_attn_fwd_raw(qkv, qs, ks, cos, sin, heads, eps=1e-6):
    """Fused q/k-norm + RoPE + attention forward on (a, s, 3*heads*64) bf16 -> (out (a, s, heads*64), lse2 (a*heads, s)) (no autograd)."""
    a, s, c3 = qkv.shape
    hd = c3 // 3
    d = hd // heads
    cos, sin = _rope_tabs(cos, sin, qkv.dtype)
    out = torch.empty((a, s, hd), dtype=qkv.dtype, device=qkv.device)
    lse2 = torch.empty((a * heads, s), dtype=torch.float32, device=qkv.device)
    nbytes = a * s * (c3 + hd) * qkv.element_size()
    check(_launch(f"spatial_attn_fwd S{s} D{d}", nbytes, 4 * a * heads * s * s * d, "sattn_fwd_kernel",
                  lambda: lib().vvae_spatial_attn_fwd(_p(qkv), c3, _p(out), hd, _p(lse2), _p(qs), _p(ks), _p(cos), _p(sin), a, s, heads, d,
                                                      eps, _dt(qkv), _stream())), "vvae_spatial_attn_fwd")
    return out, lse2


def spatial_attn_bwd_raw(qkv, out, lse2, dout, qs, ks, cos, sin, heads, eps=1e-6, params=None):
    """-> (dqkv (a, s, 3*heads*64), dq_scale (64), dk_scale (64)) of the fused spatial attention (no autograd)."""
    a, s, c3 = qkv.shape
    hd = c3 // 3
    d = hd // heads
    cos, sin = _rope_tabs(cos, sin, qkv.dtype)
    dqkv = torch.empty((a, s, c3), dtype=qkv.dtype, device=qkv.device)
    part = torch.empty((a * heads, 2, d), dtype=torch.float32, device=qkv.device)
    nbytes = a * s * (2 * c3 + 2 * hd) * qkv.element_size()
    check(_launch(f"spatial_attn_bwd S{s} D{d}", nbytes, 14 * a * heads * s * s * d, "sattn_bwd_kernel",
                  lambda: lib().vvae_spatial_attn_bwd(_p(qkv), c3, _p(out), hd, _p(dout), hd, _p(lse2), _p(dqkv), c3, _p(qs), _p(ks),
                                                      _p(cos), _p(sin), _p(part), a, s, heads, d, eps, _dt(qkv), _stream())),
          "vvae_spatial_attn_bwd")
    g0, g1 = fold_partials(part, params[0], params[1], d) if params is not None else fold_partials(part, None, None, d)
    return dqkv, g0, g1


class _SpatialAttnFused(torch.autograd.Function):
    """q/k-norm + RoPE + softmax(QK^T/sqrt(D))V, one hand-written kernel per direction (reference train/layers.py:153-170, :217-221)."""

    @staticmethod
    def forward(ctx, qkv, q_scale, k_scale, cos, sin, heads, eps):
        qkv = qkv.contiguous()
        qs, ks = _f32(q_scale), _f32(k_scale)
        out, lse2 = spatial_attn_fwd_raw(qkv, qs, ks, cos, sin, heads, eps)
        ctx.save_for_backward(qkv, qs, ks, cos, sin, out, lse2)
        ctx.misc = (heads, eps, q_scale.dtype)
        ctx.qparam, ctx.kparam = q_scale, k_scale
        return out

    @staticmethod
    def backward(ctx, do):
        qkv, qs, ks, cos, sin, out, lse2 = ctx.saved_tensors
        heads, eps, pdtype = ctx.misc
        do = do.to(qkv.dtype).contiguous()
        dqkv, dqs, dks = spatial_attn_bwd_raw(qkv, out, lse2, do, qs, ks, cos, sin, heads, eps, (ctx.qparam, ctx.kparam))
        if dqs is None:
            return dqkv, None, None, None, None, None, None
        return dqkv, dqs.to(pdtype), dks.to(pdtype), None, None, None, None


class _SpatialAttn(torch.autograd.Function):
    """q/k-norm + RoPE prep (HIP, one launch) -> library flash-attention core -> (backward) core -> prep backward (HIP, one launch).

    The custom Function owns the whole span so autograd never materialises the slice / cat / transpose gradients of the
    q, k, v views (reference train/layers.py:153-170 with the mask-free spatial call of :217-221).
    """

    @staticmethod
    def _views(qkv, qk, heads):
        a, s, c3 = qkv.shape
        hd = c3 // 3
        d = hd // heads
        q = qk[..., :hd].view(a, s, heads, d).transpose(1, 2)
        k = qk[..., hd:].view(a, s, heads, d).transpose(1, 2)
        v = qkv[..., 2 * hd:].view(a, s, heads, d).transpose(1, 2)
        return q, k, v

    @staticmethod
    def forward(ctx, qkv, q_scale, k_scale, cos, sin, heads, eps):
        qkv = qkv.contiguous()
        a, s, c3 = qkv.shape
        qs, ks = _f32(q_scale), _f32(k_scale)
        qk = qk_prep_fwd_raw(qkv, qs, ks, cos, sin, heads, eps)
        q, k, v = _SpatialAttn._views(qkv, qk, heads)
        out, lse, cq, ck, mq, mk, seed, off, _ = torch.ops.aten._scaled_dot_product_flash_attention(q, k, v, 0.0, False, False)
        ctx.save_for_backward(qkv, qs, ks, cos, sin, qk, out, lse, seed, off)
        ctx.misc = (cq, ck, mq, mk, heads, eps, q_scale.dtype)
        ctx.qparam, ctx.kparam = q_scale, k_scale
        return out.transpose(1, 2).reshape(a, s, c3 // 3)

    @staticmethod
    def backward(ctx, do):
        qkv, qs, ks, cos, sin, qk, out, lse, seed, off = ctx.saved_tensors
        cq, ck, mq, mk, heads, eps, pdtype = ctx.misc
        a, s, c3 = qkv.shape
        q, k, v = _SpatialAttn._views(qkv, qk, heads)
        do4 = do.to(qkv.dtype).reshape(a, s, heads, c3 // (3 * heads)).transpose(1, 2)
        dq, dk, dv = torch.ops.aten._scaled_dot_product_flash_attention_backward(do4, q, k, v, out, lse, cq, ck, mq, mk, 0.0, False,
                                                                                 seed, off)
        dqkv, dqs, dks = qk_prep_bwd_raw(qkv, dq, dk, dv, qs, ks, cos, sin, heads, eps, (ctx.qparam, ctx.kparam))
        if dqs is None:
            return dqkv, None, None, None, None, None, None
        return dqkv, dqs.to(pdtype), dks.to(pdtype), None, None, None, None


def spatial_attention_supported(qkv, heads, max_len):
    """bf16 GPU tensors with a head_dim the prep kernels take (fp32 and masked calls stay on the composed path)."""
    if not (qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 3 and qkv.shape[1] <= max_len):
        return False
    d = qkv.shape[-1] // (3 * heads)
    return lib().vvae_qk_prep_supported(d, DT[qkv.dtype]) == 1


def spatial_attention_core(qkv, q_scale, k_scale, cos, sin, heads, eps=1e-6):
    """q_norm/k_norm -> RoPE -> softmax(QK^T/sqrt(D)) V over (a, s, 3*heads*D), no mask (reference train/layers.py:153-170)."""
    if spatial_attn_fused_supported(qkv, heads) and not SPATIAL_FORCE_LIBRARY_CORE[0]:
        return _SpatialAttnFused.apply(qkv, q_scale, k_scale, cos, sin, heads, eps)
    if not SPATIAL_FORCE_LIBRARY_CORE[0]:
        note_fallback(("sattn-core", tuple(qkv.shape[1:]), heads),
                      f"spatial attention over (s, 3 h d) = {tuple(qkv.shape[1:])}, {heads} heads: the fused HIP kernel takes head_dim 64, s <= 256; "
                      "the library flash-attention core runs between two HIP prep launches instead")
    return _SpatialAttn.apply(qkv, q_scale, k_scale, cos, sin, heads, eps)


# --------------------------------------------------------------------------------------------- reparameterise + KL
def _loss_part(b, m, device):
    """Scratch for the per-workgroup partial sums of a per-sample loss reduction (folded in fixed order: no float atomics)."""
    return torch.empty((lib().vvae_loss_part_floats(b, m),), dtype=torch.float32, device=device)


class _ReparamKl(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, logvar, eps, mask, want_z, want_kl):
        mean, logvar = mean.contiguous(), logvar.contiguous()
        b, t = mean.shape[0], mean.shape[1]
        per = mean.numel() // (b * t)
        z = torch.empty(mean.shape, dtype=torch.float32, device=mean.device) if want_z else None
        kl = torch.empty((b,), dtype=torch.float32, device=mean.device) if want_kl else None
        eps = eps.to(torch.float32).contiguous() if eps is not None else None
        mask = mask.to(torch.float32).contiguous() if mask is not None else None
        part = _loss_part(b, t * per, mean.device) if want_kl else None
        check(lib().vvae_reparam_kl_fwd(_p(mean), _p(logvar), _p(eps), _p(mask), _p(z), _p(kl), _p(part), b, t, per, _dt(mean),
                                        _stream()), "vvae_reparam_kl_fwd")
        ctx.save_for_backward(mean, logvar, eps, mask)
        ctx.flags = (want_z, want_kl)
        outs = tuple(o for o in (z, kl) if o is not None)
        return outs if len(outs) > 1 else outs[0]

    @staticmethod
    def backward(ctx, *grads):
        mean, logvar, eps, mask = ctx.saved_tensors
        want_z, want_kl = ctx.flags
        grads = list(grads)
        dz = grads.pop(0) if want_z else None
        gkl = grads.pop(0) if want_kl else None
        dz = dz.to(torch.float32).contiguous() if dz is not None else None
        gkl = gkl.to(torch.float32).contiguous() if gkl is not None else None
        b, t = mean.shape[0], mean.shape[1]
        per = mean.numel() // (b * t)
        dmean, dlogvar = torch.empty_like(mean), torch.empty_like(logvar)
        check(lib().vvae_reparam_kl_bwd(_p(mean), _p(logvar), _p(eps), _p(mask), _p(dz), _p(gkl), _p(dmean), _p(dlogvar), b, t,
                                        per, _dt(mean), _stream()), "vvae_reparam_kl_bwd")
        return dmean, dlogvar, None, None, None, None


def reparameterise(mean, logvar, eps):
    """z = mean + eps * exp(logvar / 2), fp32 out (reference train/model.py:124-128)."""
    return _ReparamKl.apply(mean, logvar, eps, None, True, False)


def kl_per_sample(mean, logvar, mask_bt):
    """mean_{t,hw,c}[0.5 (e^lv - 1 - lv + mu^2) m_t / len] per sample (reference train/rl_nonadversarial.py:146-147)."""
    return _ReparamKl.apply(mean, logvar, None, mask_bt, False, True)


def reparameterise_kl(mean, logvar, eps, mask_bt):
    """Both in one pass over (mean, logvar): -> (z, kl_per_sample)."""
    return _ReparamKl.apply(mean, logvar, eps, mask_bt, True, True)


# --------------------------------------------------------------------------------------------- masked MSE / MAE
class _MaskedMseMae(torch.autograd.Function):
    @staticmethod
    def forward(ctx, video, recon, mask, video_div, partials=False):
        recon = recon.contiguous()
        video = video.to(recon.dtype).contiguous()
        mask = mask.to(torch.float32).contiguous()
        b, t = recon.shape[0], recon.shape[1]
        p = recon.numel() // (b * t)
        assert video.shape[0] * video_div == b and video.shape[1:] == recon.shape[1:]
        part = _loss_part(b, t * p, recon.device)
        if partials:                                     # (b, chunks) per-workgroup partial sums: the loss tail adds them up, no fold launch
            mse = mae = None
        else:
            mse = torch.empty((b,), dtype=torch.float32, device=recon.device)
            mae = torch.empty((b,), dtype=torch.float32, device=recon.device)
        check(lib().vvae_masked_mse_mae_fwd(_p(video), _p(recon), _p(mask), _p(mse), _p(mae), _p(part), b, t, p, video_div,
                                            _dt(recon), _stream()), "vvae_masked_mse_mae_fwd")
        ctx.save_for_backward(video, recon, mask)
        ctx.video_div = video_div
        ctx.set_materialize_grads(False)                 # an unused output's gradient stays None (the kernel takes NULL), no zero fill
        if partials:
            chunks = part.numel() // (2 * b)
            return part[:b * chunks].view(b, chunks), part[b * chunks:].view(b, chunks)
        return mse, mae

    @staticmethod
    def backward(ctx, gmse, gmae):
        video, recon, mask = ctx.saved_tensors
        if gmse is None and gmae is None:
            return None, None, None, None, None
        b, t = recon.shape[0], recon.shape[1]
        p = recon.numel() // (b * t)
        # partial-sum outputs: every partial of a sample carries the sample's gradient (a stride-0 expansion, what a plain sum over the
        # partials or the loss tails hand back): column 0 is it.  Anything else (partials weighted differently) is not what this op supports.
        for gg in (gmse, gmae):
            if gg is not None and gg.dim() == 2 and gg.shape[1] > 1 and gg.stride(1) != 0:
                raise VvaeError("masked_mse_mae(partials=True): the partial sums of a sample must enter the loss through their plain sum")
        gmse = (gmse[:, 0] if gmse.dim() == 2 else gmse).to(torch.float32).contiguous() if gmse is not None else None
        gmae = (gmae[:, 0] if gmae.dim() == 2 else gmae).to(torch.float32).contiguous() if gmae is not None else None
        dr = torch.empty_like(recon)
        check(lib().vvae_masked_mse_mae_bwd(_p(video), _p(recon), _p(mask), _p(gmse), _p(gmae), _p(dr), b, t, p, ctx.video_div,
                                            _dt(recon), _stream()), "vvae_masked_mse_mae_bwd")
        return None, dr, None, None, None


def masked_mse_mae(video, recon, mask_bt, video_div=1, partials=False):
    """Per-sample masked MSE and MAE (reference train/rl_nonadversarial.py:114-121); gradient flows to recon only.
    ``partials``: return each as (b, chunks) partial sums instead (their row sums are the per-sample values; ops.plain_loss_tail takes them)."""
    return _MaskedMseMae.apply(video, recon, mask_bt, video_div, partials)


_UNIT_GRAD = {}


def unit_grad(like):
    """A cached fp32 scalar 1.0 on ``like``'s device: the root gradient of ``loss.backward`` / ``torch.autograd.grad(loss, ...)``.  Handing it
    over explicitly (``gradient=`` / ``grad_outputs=``) spares the engine's ``ones_like`` fill launch, and a backward that recognises it by
    its storage (_PlainLossTail) spares the multiplication by it: two ~5 us launches of every replayed step."""
    key = (like.device.type, like.device.index)
    t = _UNIT_GRAD.get(key)
    if t is None:
        t = _UNIT_GRAD[key] = torch.ones((), dtype=torch.float32, device=like.device)
    return t


class _PlainLossTail(torch.autograd.Function):
    """The scalar end of loss.loss_fn_plain in one launch, gradients included (vvae_loss_tail_plain)."""

    @staticmethod
    def forward(ctx, mse_ps, kl_ps, selection, mask, max_rate, magnify, gamma1, gamma2):
        b, t = mask.shape
        out = torch.empty((5,), dtype=torch.float32, device=mse_ps.device)
        grads = torch.empty((2 * b + b * t,), dtype=torch.float32, device=mse_ps.device)
        sel = selection.reshape(b, t).to(torch.float32).contiguous()
        kl_cols = kl_ps.numel() // b                     # (b,) or (b, k) partial sums of the per-sample term (ops.encoder_head: one per frame)
        mse_cols = mse_ps.numel() // b                   # likewise (ops.masked_mse_mae(partials=True): one per workgroup)
        check(lib().vvae_loss_tail_plain(_p(mse_ps.contiguous()), mse_cols, _p(kl_ps.contiguous()), kl_cols, _p(sel), _p(mask), b, t, float(max_rate),
                                         float(magnify), float(gamma1), float(gamma2), _p(out), _p(grads), _stream()),
              "vvae_loss_tail_plain")
        ctx.save_for_backward(grads)
        ctx.bt, ctx.sel_shape, ctx.sel_dtype, ctx.kl_shape, ctx.mse_shape = (b, t), selection.shape, selection.dtype, kl_ps.shape, mse_ps.shape
        aux = out[1:]
        ctx.mark_non_differentiable(aux)
        ctx.set_materialize_grads(False)
        return out[0], aux

    @staticmethod
    def backward(ctx, go, _gaux):
        if go is None:
            return (None,) * 8
        (grads,) = ctx.saved_tensors
        b, t = ctx.bt
        unit = _UNIT_GRAD.get((go.device.type, go.device.index))
        # one launch for the three gradients -- none when the root gradient is the constant 1.0 of unit_grad (same storage)
        g = grads if (unit is not None and go.data_ptr() == unit.data_ptr() and go.numel() == 1) else grads * go
        gmse, gkl = g[:b], g[b:2 * b]
        if len(ctx.kl_shape) == 2:                       # every partial sum of a sample has the sample's gradient: a stride-0 view, no launch
            gkl = gkl.unsqueeze(1).expand(ctx.kl_shape)
        if len(ctx.mse_shape) == 2:
            gmse = gmse.unsqueeze(1).expand(ctx.mse_shape)
        return gmse, gkl, g[2 * b:].view(ctx.sel_shape).to(ctx.sel_dtype), None, None, None, None, None


def plain_loss_tail_ok(mse_ps, kl_ps, selection, mask):
    return (mse_ps.is_cuda and mse_ps.dtype == torch.float32 and kl_ps.dtype == torch.float32 and mask.dtype == torch.float32
            and mask.dim() == 2 and mask.is_contiguous() and mask.shape[0] <= 1024 and selection.numel() == mask.numel()
            and kl_ps.dim() in (1, 2) and kl_ps.shape[0] == mask.shape[0] and mse_ps.dim() in (1, 2) and mse_ps.shape[0] == mask.shape[0])


def plain_loss_tail(mse_ps, kl_ps, selection, mask, hparams):
    """-> (loss, (MSE, selection_loss, kl_loss, kept_frame_density)) of loss.loss_fn_plain from the per-sample sums."""
    loss, aux = _PlainLossTail.apply(mse_ps, kl_ps, selection, mask, hparams["max_compression_rate"], hparams["magnify_negatives_rate"],
                                     hparams["gamma1"], hparams["gamma2"])
    return loss, aux.unbind(0)


class _RlLossTail(torch.autograd.Function):
    """The scalar end of loss.loss_fn (the rl flavour's pair / REINFORCE loss) in one launch, gradients included (vvae_loss_tail_rl)."""

    @staticmethod
    def forward(ctx, mse, mae, perc, kl, selection, actions, mask, max_rate, magnify, g1, g2, g3, g4, w):
        b2, t = mask.shape
        out = torch.empty((9,), dtype=torch.float32, device=mask.device)
        grads = torch.empty((4 * b2 + b2 * t,), dtype=torch.float32, device=mask.device)
        sel = selection.reshape(b2, t).to(torch.float32).contiguous()
        act = actions.reshape(b2, t).to(torch.float32).contiguous()
        cols = mse.numel() // b2
        kl_cols = kl.numel() // b2                       # (2b,) or (2b, k) partial sums of the per-sample term (ops.encoder_head_rl: one per frame)
        pc = perc.to(torch.float32).contiguous() if perc is not None else None
        check(lib().vvae_loss_tail_rl(_p(mse.contiguous()), _p(mae.contiguous()), cols, _p(pc), _p(kl.to(torch.float32).contiguous()), kl_cols, _p(sel), _p(act),
                                      _p(mask), b2, t, float(max_rate), float(magnify), float(g1), float(g2), float(g3), float(g4), float(w), _p(out),
                                      _p(grads), _stream()), "vvae_loss_tail_rl")
        ctx.save_for_backward(grads)
        ctx.meta = (b2, t, mse.shape, mae.shape, perc is not None, selection.shape, selection.dtype, kl.shape)
        aux = out[1:]
        ctx.mark_non_differentiable(aux)
        ctx.set_materialize_grads(False)
        return out[0], aux

    @staticmethod
    def backward(ctx, go, _gaux):
        if go is None:
            return (None,) * 14
        (grads,) = ctx.saved_tensors
        b2, t, mse_shape, mae_shape, has_perc, sel_shape, sel_dtype, kl_shape = ctx.meta
        unit = _UNIT_GRAD.get((go.device.type, go.device.index))
        g = grads if (unit is not None and go.data_ptr() == unit.data_ptr() and go.numel() == 1) else grads * go
        gmse, gmae = g[:b2], g[b2:2 * b2]
        if len(mse_shape) == 2:
            gmse = gmse.unsqueeze(1).expand(mse_shape)
        if len(mae_shape) == 2:
            gmae = gmae.unsqueeze(1).expand(mae_shape)
        gkl = g[3 * b2:4 * b2]
        if len(kl_shape) == 2:                           # every partial sum of a sample has the sample's gradient: a stride-0 view, no launch
            gkl = gkl.unsqueeze(1).expand(kl_shape)
        return (gmse, gmae, g[2 * b2:3 * b2] if has_perc else None, gkl, g[4 * b2:].view(sel_shape).to(sel_dtype), None, None,
                None, None, None, None, None, None, None)


def rl_loss_tail_ok(mse, mae, kl, selection, actions, mask):
    return (mse.is_cuda and all(x.dtype == torch.float32 for x in (mse, mae, kl, mask)) and mask.dim() == 2 and mask.is_contiguous()
            and mask.shape[0] % 2 == 0 and mask.shape[0] <= 1024 and selection.numel() == mask.numel() and actions.numel() == mask.numel()
            and mse.dim() in (1, 2) and mse.shape == mae.shape and mse.shape[0] == mask.shape[0] and kl.dim() in (1, 2) and kl.shape[0] == mask.shape[0])


def rl_loss_tail(mse, mae, perc, kl, selection, actions, mask, hparams):
    """-> (loss, (MSE, perceptual_loss, selection_loss, kl_loss, kept_frame_density, mean_trajectory_prob, rl_loss, per_sample_MAE)) of loss.loss_fn from
    the per-sample sums (``mse`` / ``mae`` may be (2b, chunks) partial sums), the selection probabilities, the sampled actions and the mask."""
    loss, aux = _RlLossTail.apply(mse, mae, perc, kl, selection, actions, mask, hparams["max_compression_rate"], hparams["magnify_negatives_rate"],
                                  hparams["gamma1"], hparams["gamma2"], hparams["gamma3"], hparams["gamma4"], hparams["rl_loss_weight"])
    return loss, aux.unbind(0)


# --------------------------------------------------------------------------------------------- encoder heads + latent gate
def encoder_head_shape_ok(b, t, hw, ld, w1, b1, w2, b2, fill):
    """fp32 parameters of the shapes nnx.Linear(ld, 1) / nnx.Linear(hw, 1) give and a fill token of ld, ld a multiple of 8, a frame the
    kernels' LDS holds: what the fused heads ask beyond bf16 GPU activations (b, t, hw, ld)."""
    return (w1.numel() == ld and b1.numel() == 1 and w2.numel() == hw and b2.numel() == 1 and fill.numel() == ld
            and all(p.dtype == torch.float32 for p in (w1, b1, w2, b2, fill)) and bool(lib().vvae_encoder_head_ok(b, t, hw, ld)))


def encoder_head_eval_ok(mean, w1, b1, w2, b2, fill):
    """May encoder_head_eval run?  bf16 GPU mean (b, t, hw, ld), fp32 parameters, a shape the fused heads cover."""
    return (mean.is_cuda and mean.dim() == 4 and mean.dtype == torch.bfloat16
            and encoder_head_shape_ok(*mean.shape, w1, b1, w2, b2, fill))


def encoder_head_ok(mean, v, w1, b1, w2, b2, fill):
    """May encoder_head / encoder_head_rl run?  What encoder_head_eval asks, and a bf16 v of mean's shape."""
    return encoder_head_eval_ok(mean, w1, b1, w2, b2, fill) and v.dtype == torch.bfloat16 and v.shape == mean.shape


def _head_operands(mean, v, params, mask_bt, train):
    """What the three head entries are handed: contiguous activations (``v`` may be None), fp32 copies of (w1, b1, w2, b2, fill), the frame mask
    as fp32 rows of unit stride with their pitch (0: one row for all samples; None stays None) and, for the train forward, the buffers y (b t)
    and s1 (b t, hw) it keeps for the backward."""
    b, t, hw, ld = mean.shape
    mean = mean.contiguous()
    if v is not None:
        v = v.contiguous()
    mp = 0
    if mask_bt is not None:
        if mask_bt.dtype != torch.float32 or (mask_bt.shape[1] > 1 and mask_bt.stride(1) != 1):
            mask_bt = mask_bt.to(torch.float32).contiguous()
        mp = mask_bt.stride(0) if mask_bt.shape[0] > 1 else 0
    y = torch.empty((b * t,), dtype=torch.float32, device=mean.device) if train else None
    s1 = torch.empty((b * t, hw), dtype=torch.float32, device=mean.device) if train else None
    return mean, v, tuple(_f32(p) for p in params), mask_bt, mp, y, s1


def _head_forward(ctx, rl, mean, v, w1, b1, w2, b2, fill, u, eps, mask_bt):
    """vvae_encoder_head_fwd in either flavour -> (logvar, mean2, comp, sel, mask2, kl).  rl: every output pair-doubled (2b samples), ``sel`` the
    probability, ``mask2`` the sampled frame masks; model: mean2 and mask2 are None."""
    b, t, hw, ld = mean.shape
    mean, v, (w1f, b1f, w2f, b2f, ff), mask_bt, mp, y, s1 = _head_operands(mean, v, (w1, b1, w2, b2, fill), mask_bt, True)
    dev, n = mean.device, (2 * b if rl else b)
    u = u.reshape(n, t).to(torch.float32).contiguous()
    eps = eps.to(torch.float32).contiguous()
    logvar, comp = (torch.empty((n, t, hw, ld), dtype=mean.dtype, device=dev) for _ in range(2))
    mean2 = torch.empty_like(logvar) if rl else None
    sel = torch.empty((n, t, 1, 1), dtype=torch.float32, device=dev)
    mask2 = torch.empty_like(sel) if rl else None
    kl = torch.empty((n, t), dtype=torch.float32, device=dev)
    check(lib().vvae_encoder_head_fwd(_p(mean), _p(v), _p(w1f), _p(b1f), _p(w2f), _p(b2f), _p(u), _p(eps), _p(mask_bt), mp, _p(ff), int(rl),
                                      _p(logvar), _p(mean2), _p(comp), _p(sel), _p(mask2), _p(y), _p(s1), _p(kl), b, t, hw, ld, _stream()),
          "vvae_encoder_head_fwd")
    ctx.save_for_backward(mean, v, eps, mask_bt, ff, w1f, w2f, y, s1, mask2 if rl else sel, logvar)
    ctx.params = (w1, b1, w2, b2, fill)
    ctx.mask_pitch = mp
    if rl:
        ctx.mark_non_differentiable(mask2)
    ctx.set_materialize_grads(False)
    return logvar, mean2, comp, sel, mask2, kl


def _head_backward(ctx, rl, dlv, dcomp, dsel, gkl):
    """vvae_encoder_head_bwd in either flavour and the folds of its partial rows -> the gradients of _head_forward's operands.  ``dlv`` is the
    gradient at a log-variance of mean's shape; dcomp, dsel and gkl arrive as the forward's outputs are shaped (rl: pair-doubled).  Each may be
    None.  The parameter gradients leave the kernel as one partial row per frame and join the grouped folds of ``deferred_wgrad``."""
    mean, v, eps, mask_bt, ff, w1f, w2f, y, s1, sel, logvar = ctx.saved_tensors
    w1, b1, w2, b2, fill = ctx.params
    b, t, hw, ld = mean.shape
    if dcomp is not None:
        dcomp = dcomp.to(torch.bfloat16).contiguous()
    if dlv is not None:
        dlv = dlv.to(torch.bfloat16).contiguous()
    if dsel is not None:
        dsel = dsel.to(torch.float32).contiguous()
    gb = gt = 0
    if gkl is not None:
        if gkl.dtype != torch.float32:
            gkl = gkl.to(torch.float32)
        gb, gt = gkl.stride(0), gkl.stride(1)
    dmean, dv = torch.empty_like(mean), torch.empty_like(v)
    f = b * t
    part = torch.empty((2 * f * ld + f * hw + 8 * f,), dtype=torch.float32, device=mean.device)      # row widths: multiples of four floats (the folds)
    p1, p2, p3 = part[:f * ld].view(f, ld), part[f * ld:f * (ld + hw)].view(f, hw), part[f * (ld + hw):f * (2 * ld + hw)].view(f, ld)
    pb = part[f * (2 * ld + hw):].view(2, f, 4)
    check(lib().vvae_encoder_head_bwd(_p(mean), _p(v), _p(logvar), _p(eps), _p(mask_bt), ctx.mask_pitch, _p(ff), _p(w1f), _p(w2f), _p(y), _p(s1),
                                      _p(sel), _p(dcomp), _p(dsel), _p(gkl), gb, gt, _p(dlv), int(rl), _p(dmean), _p(dv), _p(p1), _p(p2), _p(p3),
                                      _p(pb), b, t, hw, ld, _stream()), "vvae_encoder_head_bwd")
    dw1, _ = fold_partials(p1, w1, None, ld)
    dw2, _ = fold_partials(p2, w2, None, hw)
    dfill, _ = fold_partials(p3, fill, None, ld)
    db1, _ = fold_partials(pb[0], b1, None, 1)
    db2, _ = fold_partials(pb[1], b2, None, 1)
    like = lambda g, p: None if g is None else g.reshape(p.shape).to(p.dtype)
    return (dmean, dv, like(dw1, w1), like(db1, b1), like(dw2, w2), like(db2, b2), like(dfill, fill), None, None, None)


class _EncoderHead(torch.autograd.Function):
    """log-variance, selection logits, Gumbel-sigmoid STE, reparameterisation, per-frame KL and the latent gate of the model.py flavour in
    ONE launch each way (vvae_encoder_head_fwd / _bwd with rl = 0; reference train/model.py:53-59,121-133, train/layers.py:226-252)."""

    @staticmethod
    def forward(ctx, *operands):
        logvar, _, comp, sel, _, kl = _head_forward(ctx, False, *operands)
        return logvar, comp, sel, kl

    @staticmethod
    def backward(ctx, dlv, dcomp, dsel, gkl):
        return _head_backward(ctx, False, dlv, dcomp, dsel, gkl)


class _EncoderHeadRl(torch.autograd.Function):
    """The rl flavour's heads + reparameterisation + KL + pair doubling + Bernoulli frame masks + latent gate in ONE launch each way
    (vvae_encoder_head_fwd / _bwd with rl = 1; reference train/rl_model.py:50-60,119-147): what rl_model.VideoVAE.forward did with softplus,
    log, two addmm, add, sigmoid, ops.reparameterise_kl, five repeat_interleave and ops.rl_gate (and their backward launches)."""

    @staticmethod
    def forward(ctx, *operands):
        return _head_forward(ctx, True, *operands)

    @staticmethod
    def backward(ctx, dlv2, dmean2, dcomp2, dsel2, _dmask2, gkl):
        # gradients arriving at the pair-doubled log-variance / mean copies (the loss reads them only through kl2; a caller that does
        # use them pays two small framework launches): a pair's two rows add up
        pair_sum = lambda g: None if g is None else g.reshape(g.shape[0] // 2, 2, *g.shape[1:]).sum(1)
        grads = _head_backward(ctx, True, pair_sum(dlv2), dcomp2, dsel2, gkl)
        if dmean2 is not None:
            grads = (grads[0] + pair_sum(dmean2).to(grads[0].dtype),) + grads[1:]
        return grads


def encoder_head(mean, v, w1, b1, w2, b2, fill, u, eps, mask_bt):
    """-> (log_variance bf16, compressed_representation bf16, selection (b, t, 1, 1) in {0, 1} with the straight-through gradient,
    kl (b, t): the per-sample KL term as one partial sum per frame)."""
    return _EncoderHead.apply(mean, v, w1, b1, w2, b2, fill, u, eps, mask_bt)


def encoder_head_rl(mean, v, w1, b1, w2, b2, fill, u2, eps, mask_bt):
    """-> (log_variance, mean, compressed_representation: bf16 (2b, t, hw, ld), pair-doubled; selection probability (2b, t, 1, 1) fp32;
    selection_mask (2b, t, 1, 1) in {0, 1}; kl (2b, t): the per-sample KL term of the doubled batch as one partial sum per frame)."""
    return _EncoderHeadRl.apply(mean, v, w1, b1, w2, b2, fill, u2, eps, mask_bt)


def encoder_head_eval(mean, v, w1, b1, w2, b2, fill, u=None, mask_bt=None, rl=False):
    """The eval heads in one launch (vvae_encoder_head_eval_fwd; reference train/model.py:121-131 with train=False, train/rl_model.py:50-60
    without the pair doubling).  No autograd: call under torch.no_grad().  ``v`` (pre-softplus) None: no log-variance.  ``u`` (b, t) uniforms
    (rl only) or None: the rint(prob) threshold.  ``mask_bt`` (b, t) frame mask or None: frames it marks 0 are dropped (selection 0, the fill
    token), whatever the padding held.  -> (log_variance bf16 (b, t, hw, ld) or None, compressed_representation bf16 (b, t, hw, ld),
    selection fp32 (b, t) in {0, 1}, probability fp32 (b, t) (rl) or None).  Outputs are fresh torch.empty tensors every kernel element of
    which is written (no fill launch: safe inside a captured hipGraph)."""
    b, t, hw, ld = mean.shape
    mean, v, (w1f, b1f, w2f, b2f, ff), mask_bt, mp, _, _ = _head_operands(mean, v, (w1, b1, w2, b2, fill), mask_bt, False)
    dev = mean.device
    u = u.reshape(b * t).to(torch.float32).contiguous() if rl and u is not None else None
    logvar = torch.empty_like(mean) if v is not None else None
    comp = torch.empty_like(mean)
    sel = torch.empty((b, t), dtype=torch.float32, device=dev)
    prob = torch.empty((b, t), dtype=torch.float32, device=dev) if rl else None
    check(lib().vvae_encoder_head_eval_fwd(_p(mean), _p(v), _p(w1f), _p(b1f), _p(w2f), _p(b2f), _p(u), _p(mask_bt), mp, _p(ff),
                                           1 if rl else 0, _p(logvar), _p(comp), _p(sel), _p(prob), b, t, hw, ld, _stream()),
          "vvae_encoder_head_eval_fwd")
    return logvar, comp, sel, prob


# ---- the rl flavour's latent gate alone: the path for shapes the fused heads refuse (rl_model.FUSED_HEADS) ----
class _RlGate(torch.autograd.Function):
    """Pair doubling + Bernoulli frame masks + fill * (1 - mask) + z * mask of rl_model.VideoVAE (reference train/rl_model.py:136-145) in one
    launch each way (vvae_rl_gate_fwd / _bwd) -> (compressed_representation bf16 (2b, t, hw, ld), selection_mask fp32 (2b, t, 1, 1))."""

    @staticmethod
    def forward(ctx, z, prob, u, fill):
        b, t, hw, ld = z.shape
        z = z.contiguous()
        pr = prob.reshape(b, t).to(torch.float32).contiguous()
        uu = u.reshape(2 * b, t).to(torch.float32).contiguous()
        ff = _f32(fill).reshape(-1)
        comp = torch.empty((2 * b, t, hw, ld), dtype=torch.bfloat16, device=z.device)
        mask = torch.empty((2 * b, t, 1, 1), dtype=torch.float32, device=z.device)
        check(lib().vvae_rl_gate_fwd(_p(z), _p(pr), _p(uu), _p(ff), _p(comp), _p(mask), 2 * b, t, hw * ld, ld, _stream()), "vvae_rl_gate_fwd")
        ctx.save_for_backward(mask)
        ctx.fill = fill
        ctx.zshape = z.shape
        ctx.mark_non_differentiable(mask)
        ctx.set_materialize_grads(False)
        return comp, mask

    @staticmethod
    def backward(ctx, dcomp, _dmask):
        if dcomp is None:
            return None, None, None, None
        (mask,) = ctx.saved_tensors
        b, t, hw, ld = ctx.zshape
        dcomp = dcomp.to(torch.bfloat16).contiguous()
        dz = torch.empty(ctx.zshape, dtype=torch.float32, device=dcomp.device)
        part = torch.empty((lib().vvae_rl_gate_blocks(2 * b, t, hw * ld), ld), dtype=torch.float32, device=dcomp.device)
        check(lib().vvae_rl_gate_bwd(_p(dcomp), _p(mask), _p(dz), _p(part), 2 * b, t, hw * ld, ld, _stream()), "vvae_rl_gate_bwd")
        dfill, _ = fold_partials(part, ctx.fill, None, ld)
        return dz, None, None, (None if dfill is None else dfill.reshape(ctx.fill.shape).to(ctx.fill.dtype))


def rl_gate_ok(z, prob, fill):
    return (z.is_cuda and z.dim() == 4 and z.dtype == torch.float32 and fill.numel() == z.shape[-1] and fill.dtype == torch.float32
            and prob.numel() == z.shape[0] * z.shape[1] and lib().vvae_rl_gate_ok(2 * z.shape[0], z.shape[1], z.shape[2] * z.shape[3], z.shape[3]) == 1)


def rl_gate(z, prob, u, fill):
    """-> (comp bf16 (2b, t, hw, ld), selection_mask fp32 (2b, t, 1, 1)): samples 2k, 2k + 1 share z[k]; mask = u < prob[k]."""
    return _RlGate.apply(z, prob, u, fill)


def _recon_metrics(name, limits, video, recon, mask, clamp):
    """The body of ``recon_metrics`` and ``recon_metrics_wide``: the entries vvae_<name>_{supported, part_floats, fwd}."""
    b, t, h, w, c = video.shape
    dx, dy = _dt(video), _dt(recon)
    if not getattr(lib(), f"vvae_{name}_supported")(h, w, c, dx, dy):
        raise VvaeError(f"{name}: frames {h}x{w}x{c} ({video.dtype} / {recon.dtype}) are outside what the kernel takes ({limits})")
    video, recon = video.contiguous(), recon.contiguous()
    mask = mask.reshape(b, t).to(torch.float32).contiguous()
    dev = video.device
    mse, psnr, ssim = (torch.empty((b, t), dtype=torch.float32, device=dev) for _ in range(3))
    part = torch.empty(int(getattr(lib(), f"vvae_{name}_part_floats")(b, t, h, w, c)), dtype=torch.float32, device=dev)
    nbytes = b * t * h * w * c * (video.element_size() + recon.element_size())
    fwd = getattr(lib(), f"vvae_{name}_fwd")
    check(_launch(f"{name} {h}x{w}x{c}", nbytes, 0, "metrics_fwd_kernel",
                  lambda: fwd(_p(video), dx, _p(recon), dy, _p(mask), _p(mse), _p(psnr), _p(ssim), _p(part), b, t, h, w, c,
                              1 if clamp else 0, _stream())),
          f"vvae_{name}_fwd")
    return mse, psnr, ssim


def recon_metrics(video, recon, mask, clamp=True):
    """Per-frame MSE, PSNR and SSIM of ``recon`` against ``video`` (vvae_recon_metrics_fwd: one pass over both plus a fold over the bands;
    the definition is metrics.py's).  video, recon (b, t, h, w, c) GPU fp32 or bf16, independently; mask (b, t), nonzero = valid frame.
    -> (mse, psnr, ssim) fp32 (b, t), 0 on masked frames.  A shape or dtype the kernel does not take raises VvaeError.  No autograd, no fill
    launch: safe inside a captured hipGraph."""
    return _recon_metrics("recon_metrics", "H, W >= 11, 1 <= C <= 4, W C <= 2048", video, recon, mask, clamp)


def recon_metrics_wide(video, recon, mask, clamp=True):
    """``recon_metrics`` for frames of any width 11 <= W <= 8192 (vvae_recon_metrics_wide_fwd: column strips past W C = 2048; a shape
    ``recon_metrics`` takes gives bitwise its results).  Same arguments and outputs."""
    return _recon_metrics("recon_metrics_wide", "H >= 11, 11 <= W <= 8192, 1 <= C <= 4", video, recon, mask, clamp)


SSIM_LOSS_LIMITS = "H, W >= 11, 1 <= C <= 4, W C <= 2048, B T <= 65535"


def ssim_frames_supported(b, t, h, w, c, video_dtype=torch.bfloat16, recon_dtype=torch.bfloat16):
    """Do vvae_ssim_loss_fwd / _bwd take ``b`` x ``t`` frames of ``h`` x ``w`` x ``c`` (``SSIM_LOSS_LIMITS``)?"""
    return (video_dtype in DT and recon_dtype in DT and bool(lib().vvae_ssim_loss_supported(h, w, c, DT[video_dtype], DT[recon_dtype]))
            and int(lib().vvae_ssim_loss_ws_floats(b, t, h, w, c)) > 0)


class _SsimFrames(torch.autograd.Function):
    """Forward: vvae_ssim_loss_fwd (the metrics pass storing the maps A, Bm, Cm, and the fold); backward: vvae_ssim_loss_bwd (one
    launch).  The workspace with the maps is held by ctx.  recon receives the gradient; video and mask none."""

    @staticmethod
    def forward(ctx, video, recon, mask, video_div, clamp):
        b, t, h, w, c = recon.shape
        dx, dy = DT[video.dtype], DT[recon.dtype]
        ssim = torch.empty((b, t), dtype=torch.float32, device=recon.device)
        ws = torch.empty(int(lib().vvae_ssim_loss_ws_floats(b, t, h, w, c)), dtype=torch.float32, device=recon.device)
        nbytes = b * t * h * w * c * (video.element_size() + recon.element_size()) + 12 * b * t * (h - 10) * (w - 10) * c
        check(_launch(f"ssim_loss_fwd {h}x{w}x{c}", nbytes, 0, "metrics_fwd_kernel",
                      lambda: lib().vvae_ssim_loss_fwd(_p(video), dx, _p(recon), dy, _p(mask), _p(ssim), _p(ws), b, t, h, w, c, video_div,
                                                       clamp, _stream())),
              "vvae_ssim_loss_fwd")
        ctx.save_for_backward(video, recon, mask)
        ctx.ws, ctx.video_div, ctx.clamp = ws, video_div, clamp
        ctx.set_materialize_grads(False)                 # an unused output's gradient stays None: no launch, no zero fill
        return ssim

    @staticmethod
    def backward(ctx, gout):
        if gout is None:
            return None, None, None, None, None
        video, recon, mask = ctx.saved_tensors
        b, t, h, w, c = recon.shape
        gout = gout.detach().to(torch.float32).contiguous()
        dr = torch.empty_like(recon)
        nbytes = b * t * h * w * c * (video.element_size() + 2 * recon.element_size()) + 12 * b * t * (h - 10) * (w - 10) * c
        check(_launch(f"ssim_loss_bwd {h}x{w}x{c}", nbytes, 0, "ssim_bwd_kernel",
                      lambda: lib().vvae_ssim_loss_bwd(_p(video), DT[video.dtype], _p(recon), DT[recon.dtype], _p(mask), _p(gout),
                                                       _p(ctx.ws), _p(dr), b, t, h, w, c, ctx.video_div, ctx.clamp, _stream())),
              "vvae_ssim_loss_bwd")
        return None, dr, None, None, None


def ssim_frames(video, recon, mask_bt, video_div=1, clamp=True):
    """Per-frame SSIM (metrics.py's definition) of ``recon`` (b, t, h, w, c) against sample i // video_div of ``video``
    (b / video_div, t, h, w, c) -> fp32 (b, t), 0 on masked frames, differentiable with respect to ``recon`` only (the closed form of
    metrics.ssim_grad_reference).  fp32 or bf16, independently; mask_bt (b, t), nonzero = valid frame.

    GPU tensors: vvae_ssim_loss_fwd, bit for bit ``recon_metrics``' ssim, and one launch of vvae_ssim_loss_bwd in the backward pass; no
    atomics, memset or fill launch, so both are safe inside a captured hipGraph.  The forward keeps 12 bytes per valid position and
    channel (the maps A, Bm, Cm) until the backward has run.  A shape outside ``SSIM_LOSS_LIMITS`` raises VvaeError before any launch.
    CPU tensors run metrics.ssim_frames_composed (float64, framework autograd)."""
    devs = {video.device, recon.device, mask_bt.device}
    if len(devs) != 1:
        raise VvaeError(f"ssim_frames: video, recon and mask must be on one device; got {sorted(str(d) for d in devs)}")
    if (video.dim() != 5 or recon.dim() != 5 or video_div < 1 or video.shape[0] * video_div != recon.shape[0]
            or video.shape[1:] != recon.shape[1:] or tuple(mask_bt.shape) != tuple(recon.shape[:2])):
        raise VvaeError(f"ssim_frames: video {tuple(video.shape)}, recon {tuple(recon.shape)}, mask {tuple(mask_bt.shape)}: "
                        f"(b / {video_div}, t, h, w, c), (b, t, h, w, c) and (b, t)")
    if not recon.is_cuda:
        from .metrics import ssim_frames_composed
        return ssim_frames_composed(video, recon, mask_bt, clamp, video_div)
    b, t, h, w, c = recon.shape
    _dt(video), _dt(recon)
    if not ssim_frames_supported(b, t, h, w, c, video.dtype, recon.dtype):
        raise VvaeError(f"ssim_frames: {b}x{t} frames of {h}x{w}x{c} ({video.dtype} / {recon.dtype}) are outside what the kernels take "
                        f"({SSIM_LOSS_LIMITS})")
    return _SsimFrames.apply(video.detach().contiguous(), recon.contiguous(), mask_bt.detach().to(torch.float32).contiguous(),
                             int(video_div), 1 if clamp else 0)


def ms_ssim(video, recon, mask, clamp=True, weights=(0.0448, 0.2856, 0.3001, 0.2363, 0.1333), want_terms=False):
    """Per-frame multi-scale SSIM of ``recon`` against ``video`` (vvae_ms_ssim_fwd: per level a per-channel moment pass, a 2 x 2 mean pool
    to the next level, then one fold over the levels; the definition is metrics.py's).  video, recon (b, t, h, w, c) GPU fp32 or bf16,
    independently; mask (b, t), nonzero = valid frame; ``weights``: one non-negative float per scale, 1 to 5 of them.
    -> (ms_ssim fp32 (b, t), terms fp32 (b, t, scales, c) or None), 0 on masked frames.  A shape or dtype the kernels do not take raises
    VvaeError.  No autograd, no fill launch: safe inside a captured hipGraph."""
    b, t, h, w, c = video.shape
    dx, dy = _dt(video), _dt(recon)
    wts = [float(v) for v in weights]
    m = len(wts)
    if not 1 <= m <= 5 or any(not 0.0 <= v < float("inf") for v in wts):
        raise VvaeError(f"ms_ssim: weights {tuple(weights)}: 1 to 5 non-negative floats, one per scale")
    nws = int(lib().vvae_ms_ssim_ws_floats(b, t, h, w, c, m)) if lib().vvae_ms_ssim_supported(h, w, c, m, dx, dy) else 0
    if nws == 0:
        raise VvaeError(f"ms_ssim: {b}x{t} frames of {h}x{w}x{c} ({video.dtype} / {recon.dtype}) at {m} scales are outside what the "
                        f"kernels take (H, W >= {11 << (m - 1)} at {m} scales, W <= 8192, 1 <= C <= 4, B T <= 65535)")
    video, recon = video.contiguous(), recon.contiguous()
    mask = mask.reshape(b, t).to(torch.float32).contiguous()
    dev = video.device
    out = torch.empty((b, t), dtype=torch.float32, device=dev)
    terms = torch.empty((b, t, m, c), dtype=torch.float32, device=dev) if want_terms else None
    ws = torch.empty(nws, dtype=torch.float32, device=dev)
    # level 0 is read twice (moments, pool) unless it is the only level; every pyramid level is written once and read once or twice
    n0 = b * t * h * w * c
    nbytes = n0 * (video.element_size() + recon.element_size()) * (2 if m > 1 else 1)
    nbytes += sum(2 * 4 * b * t * (h >> j) * (w >> j) * c * (3 if j < m - 1 else 2) for j in range(1, m))
    wts += [0.0] * (5 - m)
    check(_launch(f"ms_ssim {h}x{w}x{c} m{m}", nbytes, 0, "metrics_fwd_kernel",
                  lambda: lib().vvae_ms_ssim_fwd(_p(video), dx, _p(recon), dy, _p(mask), _p(out), _p(terms), _p(ws), b, t, h, w, c, m,
                                                 *wts, 1 if clamp else 0, _stream())),
          "vvae_ms_ssim_fwd")
    return out, terms


_U8_LUT = {}


def _u8_lut(device):
    """The 256 fp32 values torch's ``u8.float() / 255`` gives on ``device`` (built once per device, outside any capture): what the gather
    writes for each byte, so that it is bitwise the eager conversion."""
    key = str(device)
    if key not in _U8_LUT:
        _U8_LUT[key] = torch.arange(256, dtype=torch.uint8, device=device).float() / 255.0
    return _U8_LUT[key]


def tile_gather(frames, grid, first, count, out):
    """Tiles ``first .. first + count - 1`` (flat order window, ty, tx) of uint8 ``frames`` (N, T, H, W, C) on ``grid`` (tiling.TileGrid)
    -> ``out[:count]`` fp32 (>= count, T, S, S, C), each value bitwise ``u8.float() / 255`` (vvae_tile_gather_u8; edge-replicated past
    the frame).  ``out`` is written in place (the static input of a captured graph); returns it."""
    n, t, h, w, c = frames.shape
    s, o = grid.tile, grid.overlap
    if frames.dtype != torch.uint8 or not frames.is_cuda:
        raise VvaeError(f"tile_gather: frames must be uint8 on a GPU; got {frames.dtype} on {frames.device}")
    if (h, w) != (grid.height, grid.width) or not lib().vvae_tile_gather_supported(h, w, c, s, o):
        raise VvaeError(f"tile_gather: frames {h}x{w}x{c} on a grid of {grid.height}x{grid.width}, tile {s}, overlap {o}: not supported")
    if (out.dtype != torch.float32 or not out.is_contiguous() or out.device != frames.device or tuple(out.shape[1:]) != (t, s, s, c)
            or out.shape[0] < count):
        raise VvaeError(f"tile_gather: out must be contiguous fp32 (>= {count}, {t}, {s}, {s}, {c}); got {out.dtype} {tuple(out.shape)}")
    frames = frames.contiguous()
    lut = _u8_lut(frames.device)
    nbytes = count * t * s * s * c * 5
    check(_launch(f"tile_gather {s}x{s}x{c}", nbytes, 0, "tile_gather_kernel",
                  lambda: lib().vvae_tile_gather_u8(_p(frames), _p(lut), _p(out), n, t, h, w, c, s, o, grid.ny, grid.nx, first, count,
                                                    _stream())),
          "vvae_tile_gather_u8")
    return out


def tile_blend(tiles, grid, out=None):
    """Tiles (N ny nx, T, S, S, C) fp32 or bf16 on ``grid`` -> frames fp32 (N, T, H, W, C): the weighted blend of tiling.py
    (vvae_tile_blend: gather form, fixed order, every output word written; safe inside a captured hipGraph).  ``out``: optional
    contiguous fp32 destination."""
    nk, t, s, s2, c = tiles.shape
    k = grid.ny * grid.nx
    dt = _dt(tiles)
    if s != grid.tile or s2 != grid.tile or nk % k or not lib().vvae_tile_blend_supported(grid.height, grid.width, c, s, grid.overlap, dt):
        raise VvaeError(f"tile_blend: tiles {tuple(tiles.shape)} do not fit a grid of {grid.height}x{grid.width}, tile {grid.tile}, "
                        f"overlap {grid.overlap} ({k} tiles per window)")
    n = nk // k
    tiles = tiles.contiguous()
    shape = (n, t, grid.height, grid.width, c)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=tiles.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != tiles.device:
        raise VvaeError(f"tile_blend: out must be contiguous fp32 {shape}; got {out.dtype} {tuple(out.shape)}")
    nbytes = tiles.numel() * tiles.element_size() + out.numel() * 4
    check(_launch(f"tile_blend {grid.height}x{grid.width}x{c}", nbytes, 0, "tile_blend_kernel",
                  lambda: lib().vvae_tile_blend(_p(tiles), dt, _p(out), n, t, grid.height, grid.width, c, s, grid.overlap, grid.ny, grid.nx,
                                                _stream())),
          "vvae_tile_blend")
    return out


def window_blend(tiles, plan, grid, f_lo, f_hi, out, ring=None):
    """The tiles of a clip's windows (``ring`` slots, ny nx, F, S, S, C) fp32 or bf16, window w in slot w % ring (``ring`` defaults to
    tiles.shape[0]) on ``plan`` (tiling.WindowPlan) x ``grid`` -> frames ``f_lo .. f_hi - 1`` of ``out``, a contiguous fp32 (L, H, W, C)
    clip buffer, written in place: the blend of tiling.py (vvae_window_blend: fixed order, every word of the range written, no word
    outside it).  The windows covering the range must be at most ``ring`` consecutive ones.  Returns ``out``."""
    r, k, f, s, s2, c = tiles.shape
    ring = r if ring is None else int(ring)
    dt = _dt(tiles)
    if (k != grid.tiles or f != plan.frames or s != grid.tile or s2 != grid.tile or ring != r or
            not lib().vvae_window_blend_supported(plan.length, plan.frames, plan.overlap, grid.height, grid.width, c, s, grid.overlap, dt)):
        raise VvaeError(f"window_blend: tiles {tuple(tiles.shape)} do not fit {plan!r} x {grid!r}")
    shape = (plan.length, grid.height, grid.width, c)
    if out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != tiles.device:
        raise VvaeError(f"window_blend: out must be contiguous fp32 {shape}; got {out.dtype} {tuple(out.shape)}")
    tiles = tiles.contiguous()
    nbytes = (f_hi - f_lo) * grid.height * grid.width * c * 4 + min(tiles.numel(), (f_hi - f_lo) * k * s * s * c) * tiles.element_size()
    check(_launch(f"window_blend {grid.height}x{grid.width}x{c}", nbytes, 0, "window_blend_kernel",
                  lambda: lib().vvae_window_blend(_p(tiles), dt, ring, _p(out), plan.length, plan.frames, plan.overlap, plan.windows,
                                                  int(f_lo), int(f_hi), grid.height, grid.width, c, s, grid.overlap, grid.ny, grid.nx,
                                                  _stream())),
          "vvae_window_blend")
    return out


def temporal_mse(video, recon, clamp=True):
    """Temporal-difference error of consecutive frames (vvae_temporal_mse_fwd; the definition is metrics.py's).  video, recon (b, t, h, w, c)
    GPU fp32 or bf16, independently -> fp32 (b, t - 1): mean over h w c of ((y_t - y_{t-1}) - (x_t - x_{t-1}))^2.  No fill launch: safe
    inside a captured hipGraph."""
    b, t, h, w, c = video.shape
    dx, dy = _dt(video), _dt(recon)
    if not lib().vvae_temporal_mse_supported(h, w, c, dx, dy):
        raise VvaeError(f"temporal_mse: frames {h}x{w}x{c} ({video.dtype} / {recon.dtype}) are outside what the kernel takes (1 <= C <= 4)")
    dev = video.device
    out = torch.empty((b, t - 1), dtype=torch.float32, device=dev)
    if t < 2:
        return out
    video, recon = video.contiguous(), recon.contiguous()
    part = torch.empty(int(lib().vvae_temporal_mse_part_floats(b, t, h, w, c)), dtype=torch.float32, device=dev)
    nbytes = b * t * h * w * c * (video.element_size() + recon.element_size()) * 2
    check(_launch(f"temporal_mse {h}x{w}x{c}", nbytes, 0, "tmse_part_kernel",
                  lambda: lib().vvae_temporal_mse_fwd(_p(video), dx, _p(recon), dy, _p(out), _p(part), b, t, h, w, c, 1 if clamp else 0,
                                                      _stream())),
          "vvae_temporal_mse_fwd")
    return out


_SCENE_TABS = {}
SCENE_SPACES = {"hsv": 0, "gray": 1}


def _scene_tabs(hist_size, space, device):
    """The int32 tables of scenes.tables(hist_size, space) on ``device`` (built once per (size, space, device), outside any capture)."""
    key = (int(hist_size), space, str(device))
    if key not in _SCENE_TABS:
        from .scenes import tables
        _SCENE_TABS[key] = torch.from_numpy(tables(hist_size, space)).to(device)
    return _SCENE_TABS[key]


def scene_hist(clip, hist_size=64, space="hsv"):
    """Per-frame histograms of a uint8 RGB clip (L, H, W, 3) on a GPU and the correlation of consecutive ones (vvae_scene_hist_fwd; the
    definitions are scenes.py's) -> (counts int32 (L, bins), corr float64 (L - 1,)).  Exact integer counts, bitwise reproducible.  A
    shape or size the kernel does not take raises VvaeError."""
    if clip.dtype != torch.uint8 or not clip.is_cuda or clip.dim() != 4 or clip.shape[3] != 3:
        raise VvaeError(f"scene_hist: clip must be uint8 (L, H, W, 3) on a GPU; got {clip.dtype} {tuple(clip.shape)} on {clip.device}")
    if space not in SCENE_SPACES:
        raise VvaeError(f"scene_hist: space {space!r}: one of {sorted(SCENE_SPACES)}")
    l, h, w, _ = clip.shape
    sp = SCENE_SPACES[space]
    if l < 1 or not lib().vvae_scene_hist_supported(h, w, hist_size, sp):
        raise VvaeError(f"scene_hist: {l} frames of {h}x{w}, {space} with {hist_size} bins per axis are outside what the kernel takes "
                        "(H <= 16384, W <= 8192, hist_size <= 64 for hsv, <= 256 for gray)")
    clip = clip.contiguous()
    dev = clip.device
    bins = hist_size * hist_size if space == "hsv" else hist_size
    tabs = _scene_tabs(hist_size, space, dev)
    counts = torch.empty((l, bins), dtype=torch.int32, device=dev)
    corr = torch.empty((l - 1,), dtype=torch.float64, device=dev)
    part, _ = _ws(int(lib().vvae_scene_hist_part_bytes(l, h, w, hist_size, sp)), dev)
    check(_launch(f"scene_hist {space} {h}x{w}", clip.numel(), 0, "scene_hist_part_kernel",
                  lambda: lib().vvae_scene_hist_fwd(_p(clip), _p(tabs), _p(counts), _p(corr) if l > 1 else None, _p(part), l, h, w,
                                                    int(hist_size), sp, _stream())),
          "vvae_scene_hist_fwd")
    return counts, corr


def scene_corr(counts):
    """cv2.HISTCMP_CORREL of consecutive rows of int32 counts (L, bins) on a GPU (vvae_scene_hist_corr) -> float64 (L - 1,)."""
    if counts.dtype != torch.int32 or not counts.is_cuda or counts.dim() != 2:
        raise VvaeError(f"scene_corr: counts must be int32 (L, bins) on a GPU; got {counts.dtype} {tuple(counts.shape)} on {counts.device}")
    l, bins = counts.shape
    corr = torch.empty((max(l - 1, 0),), dtype=torch.float64, device=counts.device)
    if l < 2:
        return corr
    counts = counts.contiguous()
    check(lib().vvae_scene_hist_corr(_p(counts), _p(corr), l, bins, _stream()), "vvae_scene_hist_corr")
    return corr


def _crop_resize(name, frames, top, left, crop_h, crop_w, out_h, out_w, dtype, out, entry):
    """The checks and the one launch crop_resize_u8 and crop_resize_norm share; ``entry(frames, out, n, h, w, c, ...)`` calls the library."""
    if frames.dtype != torch.uint8 or not frames.is_cuda or frames.dim() != 4:
        raise VvaeError(f"{name}: frames must be uint8 (n, H, W, C) on a GPU; got {frames.dtype} {tuple(frames.shape)} on "
                        f"{frames.device}")
    n, h, w, c = frames.shape
    top, left, crop_h, crop_w, out_h, out_w = (int(v) for v in (top, left, crop_h, crop_w, out_h, out_w))
    if not lib().vvae_crop_resize_supported(h, w, c, crop_h, crop_w, out_h, out_w):
        raise VvaeError(f"{name}: frames {h}x{w}x{c}, crop {crop_h}x{crop_w} -> {out_h}x{out_w} are outside what the kernel takes "
                        "(every extent 1 .. 16384, 1 <= C <= 4, the crop no larger than the frame)")
    if top < 0 or left < 0 or top + crop_h > h or left + crop_w > w:
        raise VvaeError(f"{name}: the crop {crop_h}x{crop_w} at ({top}, {left}) does not lie inside frames of {h}x{w}")
    shape = (n, out_h, out_w, c)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=frames.device)
    elif out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous() or out.device != frames.device:
        raise VvaeError(f"{name}: out must be contiguous {dtype} {shape} on {frames.device}; got {out.dtype} {tuple(out.shape)}")
    if n == 0:
        return out
    frames = frames.contiguous()
    nbytes = n * (crop_h * crop_w + out_h * out_w * out.element_size()) * c
    check(_launch(f"{name.removesuffix('_u8')} {crop_h}x{crop_w}->{out_h}x{out_w}x{c}", nbytes, 0, "crop_resize_kernel",
                  lambda: entry(_p(frames), _p(out), n, h, w, c, top, left, crop_h, crop_w, out_h, out_w, _stream())),
          f"vvae_{name}")
    return out


def crop_resize_u8(frames, top, left, crop_h, crop_w, out_h, out_w, out=None):
    """The crop [top, top + crop_h) x [left, left + crop_w) of uint8 ``frames`` (n, H, W, C) on a GPU, resized to uint8 (n, out_h, out_w, C):
    bilinear, half-pixel centres, bitwise data.resize_reference_u8 of the crop (vvae_crop_resize_u8: one launch for any n, every output
    byte written once; safe inside a captured hipGraph).  ``out``: optional contiguous uint8 destination of that shape.  A wrong dtype or
    device, a crop outside the frame or a shape the kernel does not take raises VvaeError before anything is launched."""
    return _crop_resize("crop_resize_u8", frames, top, left, crop_h, crop_w, out_h, out_w, torch.uint8, out, lib().vvae_crop_resize_u8)


def crop_resize_norm(frames, top, left, crop_h, crop_w, out_h, out_w, dtype=torch.float32, out=None):
    """crop_resize_u8 with every byte q written as float32(q) / 255 (an IEEE division: what ``torch.div(u8.float(), tensor(255.))`` gives),
    in ``dtype`` float32 or bfloat16 (the quotient rounded to nearest even): (n, out_h, out_w, C) on the GPU, on the current stream
    (vvae_crop_resize_norm: one launch for any n, every element written once; safe inside a captured hipGraph).  It is the training
    loader's resize and uint8 -> [0, 1] conversion in one launch.  ``out``: optional contiguous destination of that shape and dtype.  The
    checks are crop_resize_u8's; any other ``dtype`` raises VvaeError too."""
    if dtype not in DT:
        raise VvaeError(f"crop_resize_norm: dtype must be float32 or bfloat16; got {dtype}")
    bf16 = DT[dtype]
    return _crop_resize("crop_resize_norm", frames, top, left, crop_h, crop_w, out_h, out_w, dtype, out,
                        lambda src, dst, *rest: lib().vvae_crop_resize_norm(src, dst, bf16, *rest))


YUV_CHROMA = {"420": 0, "444": 1, "mono": 2}
YUV_SITING = {"centre": 0, "mpeg2": 1}
YUV_MATRIX = {"bt601": 0, "bt709": 1}


def yuv_supported(h, w, chroma="420"):
    """Do vvae_yuv_to_rgb_u8 / vvae_rgb_to_yuv take frames of ``h`` x ``w`` in the ``chroma`` form ("420", "444", "mono")?"""
    return chroma in YUV_CHROMA and bool(lib().vvae_yuv_supported(int(h), int(w), YUV_CHROMA[chroma]))


def _yuv_codes(name, chroma, matrix, siting="centre"):
    if chroma not in YUV_CHROMA or matrix not in YUV_MATRIX or siting not in YUV_SITING:
        raise VvaeError(f"{name}: chroma {chroma!r} (one of {sorted(YUV_CHROMA)}), siting {siting!r} (one of {sorted(YUV_SITING)}), "
                        f"matrix {matrix!r} (one of {sorted(YUV_MATRIX)})")
    return YUV_CHROMA[chroma], YUV_SITING[siting], YUV_MATRIX[matrix]


def _yuv_plane(name, what, t, shape):
    """The frame stride in bytes of the plane view ``t``: uint8 on a GPU, ``shape`` = (n, rows, cols), rows dense inside a frame, any
    frame stride >= 0 (an axis of extent 1 has no stride to speak of)."""
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or not t.is_cuda or tuple(t.shape) != tuple(shape):
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else repr(type(t))
        raise VvaeError(f"{name}: {what} must be uint8 {tuple(shape)} on a GPU; got {got}")
    n, r, c = shape
    if (c > 1 and t.stride(2) != 1) or (r > 1 and t.stride(1) != c) or (n > 1 and t.stride(0) < 0):
        raise VvaeError(f"{name}: {what} must have dense rows inside a frame (strides (any, {c}, 1)); got strides {tuple(t.stride())}")
    return int(t.stride(0)) if n > 1 else r * c


def yuv_to_rgb_u8(y, u, v, chroma="420", siting="centre", matrix="bt601", full=False, out=None):
    """Planes uint8 ``y`` (n, H, W), ``u``, ``v`` (n, CH, CW) on a GPU (None for "mono") -> uint8 RGB (n, H, W, 3): bitwise
    y4m.yuv_to_rgb_reference (vvae_yuv_to_rgb_u8: one launch for any n, integer arithmetic, every output byte written once; safe inside a
    captured hipGraph).  The planes are taken as views: any frame stride (u and v the same one), any base alignment, rows dense inside a
    frame -- the planes of frame records uploaded as they lie in a .y4m file.  ``out``: optional contiguous uint8 destination.  A CPU
    tensor, a wrong dtype, chroma planes whose shape does not fit (H, W), rows that are not dense or a size the kernel does not take
    raise VvaeError before anything is launched."""
    name = "yuv_to_rgb_u8"
    ch, st, mx = _yuv_codes(name, chroma, matrix, siting)
    if not torch.is_tensor(y) or y.dim() != 3:
        raise VvaeError(f"{name}: y must be uint8 (n, H, W) on a GPU; got {tuple(y.shape) if torch.is_tensor(y) else type(y)}")
    n, h, w = y.shape
    ys = _yuv_plane(name, "y", y, (n, h, w))
    cs = 0
    if chroma != "mono":
        cshape = (n, (h + 1) // 2, (w + 1) // 2) if chroma == "420" else (n, h, w)
        cs = _yuv_plane(name, "u", u, cshape)
        if _yuv_plane(name, "v", v, cshape) != cs:
            raise VvaeError(f"{name}: u and v must share one frame stride; got {u.stride(0)} and {v.stride(0)}")
        if u.device != y.device or v.device != y.device:
            raise VvaeError(f"{name}: the planes must be on one device")
    if not lib().vvae_yuv_supported(h, w, ch):
        raise VvaeError(f"{name}: frames of {h}x{w} are outside what the kernel takes (sides 1 .. 16384)")
    shape = (n, h, w, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=y.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != y.device:
        raise VvaeError(f"{name}: out must be contiguous uint8 {shape} on {y.device}; got {out.dtype} {tuple(out.shape)} on {out.device}")
    if n == 0:
        return out
    cbytes = 0 if chroma == "mono" else 2 * u.shape[1] * u.shape[2]
    check(_launch(f"yuv_to_rgb {chroma} {h}x{w}", n * (h * w * 4 + cbytes), 0, "yuv_to_rgb_kernel",
                  lambda: lib().vvae_yuv_to_rgb_u8(_p(y), _p(u) if cbytes else None, _p(v) if cbytes else None, ys, cs, _p(out), n, h, w, ch,
                                                   st, mx, 1 if full else 0, _stream())),
          "vvae_yuv_to_rgb_u8")
    return out


def rgb_to_yuv(rgb, chroma="420", matrix="bt601", full=False, out=None):
    """uint8 RGB ``rgb`` (n, H, W, 3) on a GPU -> planes (y (n, H, W), u, v (n, CH, CW)) uint8 there, 4:2:0 (centre siting) or 4:4:4: bitwise
    y4m.rgb_to_yuv_reference (vvae_rgb_to_yuv: one launch for any n, integer arithmetic, every output byte written once; safe inside a
    captured hipGraph).  ``out``: optional (y, u, v) of contiguous uint8 destinations.  Anything else raises VvaeError before a launch."""
    name = "rgb_to_yuv"
    if chroma == "mono":
        raise VvaeError(f"{name}: chroma 'mono': the forms written are '420' and '444'")
    ch, _, mx = _yuv_codes(name, chroma, matrix)
    if not torch.is_tensor(rgb) or rgb.dtype != torch.uint8 or not rgb.is_cuda or rgb.dim() != 4 or rgb.shape[3] != 3:
        got = f"{rgb.dtype} {tuple(rgb.shape)} on {rgb.device}" if torch.is_tensor(rgb) else repr(type(rgb))
        raise VvaeError(f"{name}: rgb must be uint8 (n, H, W, 3) on a GPU; got {got}")
    n, h, w, _ = rgb.shape
    if not lib().vvae_yuv_supported(h, w, ch):
        raise VvaeError(f"{name}: frames of {h}x{w} are outside what the kernel takes (sides 1 .. 16384)")
    cshape = (n, (h + 1) // 2, (w + 1) // 2) if chroma == "420" else (n, h, w)
    shapes = ((n, h, w), cshape, cshape)
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.uint8, device=rgb.device) for s in shapes)
    else:
        out = tuple(out)
        if len(out) != 3 or any(not torch.is_tensor(o) or o.dtype != torch.uint8 or tuple(o.shape) != s or not o.is_contiguous()
                                or o.device != rgb.device for o, s in zip(out, shapes)):
            raise VvaeError(f"{name}: out must be three contiguous uint8 tensors {shapes} on {rgb.device}")
    if n == 0:
        return out
    rgb = rgb.contiguous()
    y, u, v = out
    check(_launch(f"rgb_to_yuv {chroma} {h}x{w}", n * (h * w * 4 + 2 * cshape[1] * cshape[2]), 0, "rgb_to_yuv_kernel",
                  lambda: lib().vvae_rgb_to_yuv(_p(rgb), _p(y), _p(u), _p(v), n, h, w, ch, mx, 1 if full else 0, _stream())),
          "vvae_rgb_to_yuv")
    return out


def yuv_window_supported(h, w, chroma, out_h, out_w):
    """Does vvae_yuv_window_resize_norm take windows whose luma crop is ``h`` x ``w`` in the ``chroma`` form, resized to out_h x out_w?"""
    return chroma in YUV_CHROMA and bool(lib().vvae_yuv_window_supported(int(h), int(w), YUV_CHROMA[chroma], int(out_h), int(out_w)))


def yuv_window_span():
    """The output pixels of a row one workgroup of the window kernel spans."""
    return int(lib().vvae_yuv_window_span())


def _yuv_dense(name, what, t, shape, device=None):
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or not t.is_cuda or tuple(t.shape) != tuple(shape) or not t.is_contiguous() \
            or (device is not None and t.device != device):
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}, contiguous: {t.is_contiguous()}" if torch.is_tensor(t) else repr(type(t))
        raise VvaeError(f"{name}: {what} must be dense uint8 {tuple(shape)} on {'a GPU' if device is None else device}; got {got}")


def yuv_window_resize_norm(y, u, v, clip_params, frames_per_clip, chroma="420", siting="centre", matrix="bt601", out_h=None, out_w=None,
                           dtype=torch.float32, out=None):
    """Windows of Y'CbCr planes on a GPU (y4m.Y4MClip.window: ``y`` uint8 (n, h, w), ``u``, ``v`` of y4m.window_chroma_shape, None for
    "mono") -> (n, out_h, out_w, 3) in ``dtype`` float32 or bfloat16: y4m.window_to_rgb_reference, then data.resize_reference_u8, then
    float32(q) / 255, bit for bit, in one launch on the current stream (vvae_yuv_window_resize_norm: every element written once; safe
    inside a captured hipGraph).  ``clip_params`` int32 (ceil(n / frames_per_clip), 4) on the GPU: (top & 1, left & 1, full range, 0) of
    the clip that frames [i frames_per_clip, (i + 1) frames_per_clip) belong to.  ``out``: optional contiguous destination.  A wrong
    device, dtype, shape, density or params shape raises VvaeError before anything is launched."""
    name = "yuv_window_resize_norm"
    ch, st, mx = _yuv_codes(name, chroma, matrix, siting)
    if dtype not in DT:
        raise VvaeError(f"{name}: dtype must be float32 or bfloat16; got {dtype}")
    if not torch.is_tensor(y) or y.dim() != 3:
        raise VvaeError(f"{name}: y must be uint8 (n, h, w) on a GPU; got {tuple(y.shape) if torch.is_tensor(y) else type(y)}")
    n, h, w = y.shape
    out_h, out_w = int(h if out_h is None else out_h), int(w if out_w is None else out_w)
    frames_per_clip = int(frames_per_clip)
    _yuv_dense(name, "y", y, (n, h, w))
    if chroma != "mono":
        cshape = (n, h // 2 + 3, w // 2 + 3) if chroma == "420" else (n, h, w)
        _yuv_dense(name, "u", u, cshape, y.device)
        _yuv_dense(name, "v", v, cshape, y.device)
    if frames_per_clip < 1:
        raise VvaeError(f"{name}: frames_per_clip must be >= 1; got {frames_per_clip}")
    pshape = (-(-n // frames_per_clip), 4)
    if not torch.is_tensor(clip_params) or clip_params.dtype != torch.int32 or tuple(clip_params.shape) != pshape \
            or not clip_params.is_contiguous() or clip_params.device != y.device:
        got = f"{clip_params.dtype} {tuple(clip_params.shape)} on {clip_params.device}" if torch.is_tensor(clip_params) else repr(type(clip_params))
        raise VvaeError(f"{name}: clip_params must be contiguous int32 {pshape} on {y.device} ({n} frames, {frames_per_clip} per clip); got {got}")
    if not lib().vvae_yuv_window_supported(h, w, ch, out_h, out_w):
        raise VvaeError(f"{name}: windows of {h}x{w} -> {out_h}x{out_w} are outside what the kernel takes (every extent 1 .. 16384)")
    shape = (n, out_h, out_w, 3)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=y.device)
    elif not torch.is_tensor(out) or out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous() or out.device != y.device:
        got = f"{out.dtype} {tuple(out.shape)} on {out.device}" if torch.is_tensor(out) else repr(type(out))
        raise VvaeError(f"{name}: out must be contiguous {dtype} {shape} on {y.device}; got {got}")
    if n == 0:
        return out
    cbytes = 0 if chroma == "mono" else 2 * u.shape[1] * u.shape[2]
    check(_launch(f"yuv_window {chroma} {h}x{w}->{out_h}x{out_w}", n * (h * w + cbytes + out_h * out_w * 3 * out.element_size()), 0,
                  "yuv_window_kernel",
                  lambda: lib().vvae_yuv_window_resize_norm(_p(y), _p(u) if cbytes else None, _p(v) if cbytes else None, _p(clip_params),
                                                            _p(out), DT[dtype], n, frames_per_clip, h, w, ch, st, mx, out_h, out_w, _stream())),
          "vvae_yuv_window_resize_norm")
    return out


def plane_metrics_supported(h, w, chroma="420"):
    """Does vvae_plane_metrics_u8 take frames of ``h`` x ``w`` in the ``chroma`` form ("420", "444", "mono")?"""
    return chroma in YUV_CHROMA and bool(lib().vvae_plane_metrics_supported(int(h), int(w), YUV_CHROMA[chroma]))


def plane_metrics_u8(ref_planes, test_planes, chroma="420"):
    """The reference's and the test's planes, each (y (n, H, W), u, v (n, CH, CW)) uint8 on a GPU (u, v None for "mono") -> (sse int64
    (n, 3): the exact sums of (ref - test)^2 over the Y, U and V planes, 0 for the chroma of mono; ssim_y fp32 (n,): metrics.py's SSIM of
    the Y planes as one-channel frames y / 255).  vvae_plane_metrics_u8: one pass over the bytes, integer sums, no atomics, no fill launch,
    bitwise reproducible, safe inside a captured hipGraph.  The planes are taken as views, as ``yuv_to_rgb_u8`` takes them: any frame
    stride (u and v of an operand the same one), any base alignment, rows dense inside a frame.  A CPU tensor, a dtype other than uint8,
    chroma planes that do not fit (H, W), rows that are not dense, operands of different shapes or a size outside 11 <= H, W <= 8192
    raise VvaeError before anything is launched."""
    name = "plane_metrics_u8"
    ch, _, _ = _yuv_codes(name, chroma, "bt601")
    if len(ref_planes) != 3 or len(test_planes) != 3:
        raise VvaeError(f"{name}: each operand is (y, u, v)")
    ay, by = ref_planes[0], test_planes[0]
    if not torch.is_tensor(ay) or ay.dim() != 3:
        raise VvaeError(f"{name}: y must be uint8 (n, H, W) on a GPU; got {tuple(ay.shape) if torch.is_tensor(ay) else type(ay)}")
    n, h, w = ay.shape
    if not torch.is_tensor(by) or tuple(by.shape) != (n, h, w):
        raise VvaeError(f"{name}: the operands must have one shape; got y {(n, h, w)} and {tuple(by.shape) if torch.is_tensor(by) else type(by)}")
    cshape = None if chroma == "mono" else (n, (h + 1) // 2, (w + 1) // 2) if chroma == "420" else (n, h, w)
    strides = []
    for what, (y, u, v) in (("the reference's ", ref_planes), ("the test's ", test_planes)):
        ys, cs = _yuv_plane(name, what + "y", y, (n, h, w)), 0
        if cshape is not None:
            cs = _yuv_plane(name, what + "u", u, cshape)
            if _yuv_plane(name, what + "v", v, cshape) != cs:
                raise VvaeError(f"{name}: {what}u and v must share one frame stride; got {u.stride(0)} and {v.stride(0)}")
            if u.device != ay.device or v.device != ay.device:
                raise VvaeError(f"{name}: the planes must be on one device")
        if y.device != ay.device:
            raise VvaeError(f"{name}: the planes must be on one device")
        strides.append((ys, cs))
    if not lib().vvae_plane_metrics_supported(h, w, ch):
        raise VvaeError(f"{name}: frames of {h}x{w} are outside what the kernel takes (11 <= H, W <= 8192)")
    sse = torch.empty((n, 3), dtype=torch.int64, device=ay.device)
    ssim = torch.empty((n,), dtype=torch.float32, device=ay.device)
    if n == 0:
        return sse, ssim
    ws = torch.empty(int(lib().vvae_plane_metrics_ws_bytes(n, h, w, ch)), dtype=torch.uint8, device=ay.device)
    cp = (lambda t: _p(t)) if cshape is not None else (lambda t: None)
    (ays, acs), (bys, bcs) = strides
    nbytes = 2 * n * (h * w + (2 * cshape[1] * cshape[2] if cshape is not None else 0))
    check(_launch(f"plane_metrics {chroma} {h}x{w}", nbytes, 0, "plane_metrics_y_kernel",
                  lambda: lib().vvae_plane_metrics_u8(_p(ay), cp(ref_planes[1]), cp(ref_planes[2]), ays, acs, _p(by), cp(test_planes[1]),
                                                      cp(test_planes[2]), bys, bcs, _p(sse), _p(ssim), _p(ws), n, h, w, ch, _stream())),
          "vvae_plane_metrics_u8")
    return sse, ssim


def latent_quantise_supported(hw, ld, dtype):
    """Does vvae_latent_quantise take frames of ``hw`` tokens x ``ld`` channels in ``dtype`` (float32 / bfloat16)?"""
    return dtype in DT and bool(lib().vvae_latent_quantise_supported(int(hw), int(ld), DT[dtype]))


def _quant_operands(name, x, keep, bits, what="x"):
    """What latent_quantise, latent_fake_quant and latent_rate ask of their operands alike: ``bits`` in 2 .. 8, ``x`` a float32 or bfloat16
    tensor, contiguous (..., hw, ld), ``keep`` a tensor of one flag per frame (the leading dimensions of ``x``) on x's device
    -> (lead, frames).  VvaeError otherwise."""
    from .quant import qmax_of
    try:
        qmax_of(bits)
    except (ValueError, TypeError) as e:
        raise VvaeError(f"{name}: {e}") from None
    if not torch.is_tensor(x) or x.dtype not in DT:
        raise VvaeError(f"{name}: {what} must be a float32 or bfloat16 tensor; got {getattr(x, 'dtype', type(x))}")
    if x.dim() < 3 or not x.is_contiguous():
        raise VvaeError(f"{name}: {what} must be contiguous (..., hw, ld); got {tuple(x.shape)} strides {x.stride()}")
    lead = tuple(x.shape[:-2])
    frames = 1
    for v in lead:
        frames *= v
    if not torch.is_tensor(keep) or keep.numel() != frames:
        raise VvaeError(f"{name}: keep must hold one flag per frame ({frames})")
    if keep.device != x.device:
        raise VvaeError(f"{name}: {what} is on {x.device}, keep on {keep.device}: one device expected")
    return lead, frames


def latent_quantise(latent, keep, bits, dequantise_in_place=False, out=None):
    """Quantise the frames of ``latent`` (..., hw, ld) (bf16 or fp32, contiguous, on a GPU) whose ``keep`` flag (one float per frame, the
    leading dimensions of ``latent``) is nonzero, to ``bits`` in 2 .. 8: quant.quantise_reference on every bit (vvae_latent_quantise: one
    launch, every output element written, safe inside a captured hipGraph) -> QuantisedLatents(codes int8 (..., hw, ld), step fp32
    (..., ld), counts int32 (..., 256)).  Frames whose flag is zero get zero codes, steps and counts and stay untouched in ``latent``;
    ``dequantise_in_place`` writes float(q) * step over the kept frames of ``latent``.  ``out``: a QuantisedLatents of contiguous
    tensors of those shapes to write into.  A shape the kernel does not take raises VvaeError."""
    from .quant import QuantisedLatents
    dt = _dt(latent)
    lead, frames = _quant_operands("latent_quantise", latent, keep, bits, what="latent")
    hw, ld = latent.shape[-2:]
    if not lib().vvae_latent_quantise_supported(hw, ld, dt):
        raise VvaeError(f"latent_quantise: frames of {hw} x {ld} are outside what the kernel takes (ld a multiple of 8 in 8 .. 1024, "
                        "hw ld <= 2^30)")
    if keep.dtype != torch.float32 or not keep.is_contiguous():
        keep = keep.to(torch.float32).contiguous()
    dev = latent.device
    if out is None:
        out = QuantisedLatents(torch.empty(tuple(latent.shape), dtype=torch.int8, device=dev),
                               torch.empty(lead + (ld,), dtype=torch.float32, device=dev),
                               torch.empty(lead + (256,), dtype=torch.int32, device=dev))
    else:
        want = ((tuple(latent.shape), torch.int8), (lead + (ld,), torch.float32), (lead + (256,), torch.int32))
        for t, (shape, dtype) in zip(out, want):
            if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev:
                raise VvaeError(f"latent_quantise: out must hold contiguous {dtype} {shape} on {dev}; got {t.dtype} {tuple(t.shape)}")
    if frames == 0:
        return out
    nbytes = frames * hw * ld * (latent.element_size() * (2 if dequantise_in_place else 1) + 1)
    check(_launch(f"latent_quantise {hw}x{ld} b{int(bits)}", nbytes, 0, "latent_quantise_kernel",
                  lambda: lib().vvae_latent_quantise(_p(latent), dt, _p(keep), _p(out.codes), _p(out.step), _p(out.counts), frames, hw, ld,
                                                     int(bits), int(bool(dequantise_in_place)), _stream())),
          "vvae_latent_quantise")
    return out


def _channel_scales(xf, qmax):
    """The quantiser's scales from framework ops, as quant.quantise_reference derives them: xf fp32 (frames, hw, ld) -> (dead, inv, step),
    (frames, ld) each; inv and step are 0 in a dead channel."""
    amax = xf.abs().amax(dim=1)                                  # a NaN or an infinity in a channel stays in its maximum
    dead = ~torch.isfinite(amax) | (amax < 1e-30)
    safe = torch.where(dead, torch.ones_like(amax), amax)
    zero, qm = torch.zeros_like(amax), torch.full_like(amax, qmax)
    # qm / safe, tensor / tensor: a Python scalar on the left would be reciprocal * scalar
    return dead, torch.where(dead, zero, qm / safe), torch.where(dead, zero, safe / qm)


def _fake_quant_framework(x3, keep, qmax, counts):
    """quant.fake_quant_reference from framework ops, through the integer code (so a code 0 gives +0.0): x3 (frames, hw, ld), keep
    (frames,) fp32; counts int32 (frames, 256) or None is filled like the kernel's."""
    xf = x3.to(torch.float32)
    dead, inv, step = _channel_scales(xf, qmax)
    r = torch.clamp(torch.round(xf * inv[:, None, :]), -qmax, qmax)
    q = torch.where(dead[:, None, :], torch.zeros_like(r), r).to(torch.int32)
    kept = keep != 0
    if counts is not None:
        c = torch.zeros_like(counts).scatter_add_(1, (q + 128).reshape(q.shape[0], -1).long(),
                                                  torch.ones((1, 1), dtype=counts.dtype, device=counts.device).expand(q.shape[0], q[0].numel()))
        counts.copy_(c * kept[:, None])
    return torch.where(kept[:, None, None], (q.to(torch.float32) * step[:, None, :]).to(x3.dtype), x3)


class _LatentFakeQuant(torch.autograd.Function):
    """Forward: vvae_latent_fake_quant (one launch, out of place); backward: the straight-through estimator, the incoming gradient itself.
    The clamp never binds (step = amax / qmax), so no element is masked."""

    @staticmethod
    def forward(ctx, x, keep, bits, counts):
        hw, ld = x.shape[-2:]
        frames = x.numel() // (hw * ld)
        if not x.is_cuda or not lib().vvae_latent_quantise_supported(hw, ld, DT[x.dtype]):
            if x.is_cuda:
                note_fallback(("latent_fake_quant", hw, ld), f"latent_fake_quant: frames of {hw} x {ld} run framework ops")
            from .quant import qmax_of
            c2 = counts.view(frames, 256) if counts is not None else None
            return _fake_quant_framework(x.reshape(frames, hw, ld), keep.reshape(frames), float(qmax_of(bits)), c2).reshape(x.shape)
        out = torch.empty_like(x)
        nbytes = frames * hw * ld * 2 * x.element_size()
        check(_launch(f"latent_fake_quant {hw}x{ld} b{bits}", nbytes, 0, "latent_fake_quant_kernel",
                      lambda: lib().vvae_latent_fake_quant(_p(x), _p(out), DT[x.dtype], _p(keep), _p(counts), frames, hw, ld, bits, _stream())),
              "vvae_latent_fake_quant")
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return grad_out, None, None, None


def latent_fake_quant(x, keep, bits, counts=None):
    """The latent quantiser as the train step sees it: ``x`` (..., hw, ld) (bf16 or fp32, contiguous) -> a new tensor that holds
    float(q) * step on the frames whose ``keep`` flag (one float per frame: the leading dimensions of ``x``) is nonzero and ``x``'s own bits
    on the others; quant.fake_quant_reference on every bit.  ``x`` is left as it is.  ``counts``: an int32 (..., 256) tensor that receives
    the per-frame code histogram (zeros for a dropped frame), or None.  On a GPU one launch of vvae_latent_fake_quant, safe inside a
    captured hipGraph; CPU tensors, and shapes the kernel does not take, run the same arithmetic from framework ops.  The gradient is the
    straight-through estimator: x receives the incoming gradient itself, ``keep`` none."""
    lead, frames = _quant_operands("latent_fake_quant", x, keep, bits)
    if not keep.is_floating_point():
        raise VvaeError(f"latent_fake_quant: keep must hold one float per frame ({frames})")
    if counts is not None and (not torch.is_tensor(counts) or tuple(counts.shape) != lead + (256,) or counts.dtype != torch.int32
                               or not counts.is_contiguous() or counts.device != x.device):
        raise VvaeError(f"latent_fake_quant: counts must be a contiguous int32 tensor {lead + (256,)} on {x.device}")
    if frames == 0 or x.numel() == 0:
        return x.clone()
    return _LatentFakeQuant.apply(x, keep.detach().to(torch.float32).contiguous(), int(bits), counts)


def _rate_framework(x3, keep, qmax, cost):
    """quant.rate_reference from framework ops, bit for bit: x3 (frames, hw, ld), keep (frames,) fp32, cost fp32 (256,) ->
    (terms, slope), fp32 (frames, hw, ld) each."""
    xf = x3.to(torch.float32)
    dead, inv, _ = _channel_scales(xf, qmax)
    inv = inv[:, None, :]
    off = dead[:, None, :] | (keep == 0)[:, None, None]
    v = torch.where(dead[:, None, :], torch.zeros_like(xf), xf * inv)
    kf = torch.clamp(torch.floor(v), -qmax, qmax - 1.0)
    k = kf.to(torch.int64) + 128
    lo = cost[k]
    d = cost[k + 1] - lo
    zeros = torch.zeros_like(xf)
    return torch.where(off, zeros, lo + (v - kf) * d), torch.where(off, zeros, d * inv)


class _LatentRate(torch.autograd.Function):
    """Forward: vvae_latent_rate (one launch); backward: vvae_latent_rate_grad (one launch), the gradient of x with amax and the cost table
    held constant.  keep and cost receive none."""

    @staticmethod
    def forward(ctx, x, keep, bits, cost):
        hw, ld = x.shape[-2:]
        frames = x.numel() // (hw * ld)
        ctx.bits = bits
        ctx.save_for_backward(x, keep, cost)
        ctx.kernel = x.is_cuda and bool(lib().vvae_latent_quantise_supported(hw, ld, DT[x.dtype]))
        if not ctx.kernel:
            if x.is_cuda:
                note_fallback(("latent_rate", hw, ld), f"latent_rate: frames of {hw} x {ld} run framework ops")
            from .quant import qmax_of
            terms, _ = _rate_framework(x.reshape(frames, hw, ld), keep, float(qmax_of(bits)), cost)
            return terms.sum(dim=(1, 2)).reshape(x.shape[:-2])
        rate = torch.empty(tuple(x.shape[:-2]), dtype=torch.float32, device=x.device)
        check(_launch(f"latent_rate {hw}x{ld} b{bits}", frames * hw * ld * x.element_size(), 0, "latent_rate_kernel",
                      lambda: lib().vvae_latent_rate(_p(x), DT[x.dtype], _p(keep), _p(cost), _p(rate), frames, hw, ld, bits, _stream())),
              "vvae_latent_rate")
        return rate

    @staticmethod
    def backward(ctx, grad_rate):
        x, keep, cost = ctx.saved_tensors
        hw, ld = x.shape[-2:]
        frames = x.numel() // (hw * ld)
        g = grad_rate.detach().to(torch.float32).contiguous().reshape(frames)
        if not ctx.kernel:
            from .quant import qmax_of
            _, slope = _rate_framework(x.reshape(frames, hw, ld), keep, float(qmax_of(ctx.bits)), cost)
            off = ((g == 0) | (keep == 0))[:, None, None]                                  # zero words, as the kernel writes them
            grad = torch.where(off, torch.zeros_like(slope), g[:, None, None] * slope)
            return grad.to(x.dtype).reshape(x.shape), None, None, None
        grad = torch.empty_like(x)
        check(_launch(f"latent_rate_grad {hw}x{ld} b{ctx.bits}", frames * hw * ld * 2 * x.element_size(), 0, "latent_rate_grad_kernel",
                      lambda: lib().vvae_latent_rate_grad(_p(x), DT[x.dtype], _p(keep), _p(cost), _p(g), _p(grad), frames, hw, ld, ctx.bits,
                                                          _stream())),
              "vvae_latent_rate_grad")
        return grad, None, None, None


def latent_rate(x, keep, bits, cost):
    """The relaxed cost in bits of the codes of ``x`` (..., hw, ld) (bf16 or fp32, contiguous) under the table ``cost`` fp32 (256,)
    (loss.rate_cost_table / quant.rate_cost_reference) -> rate fp32 of x's leading dimensions: per frame the sum of the table interpolated
    linearly at the unrounded codes (quant.rate_reference), 0 for a frame whose ``keep`` flag (one float per frame) is zero.  On a GPU one
    launch of vvae_latent_rate, and one of vvae_latent_rate_grad in the backward pass, both safe inside a captured hipGraph; CPU tensors,
    and shapes the kernel does not take, run the same arithmetic from framework ops.  x receives d rate / d x with the channel maxima and the
    table held constant (rounded to x's dtype; zeros on a dropped frame); ``keep`` and ``cost`` receive no gradient."""
    lead, frames = _quant_operands("latent_rate", x, keep, bits)
    if not keep.is_floating_point():
        raise VvaeError(f"latent_rate: keep must hold one float per frame ({frames})")
    if not torch.is_tensor(cost) or cost.dtype != torch.float32 or cost.numel() != 256 or cost.device != x.device:
        raise VvaeError(f"latent_rate: cost must be a float32 tensor of 256 entries on {x.device}")
    if frames == 0 or x.numel() == 0:
        return torch.zeros(lead, dtype=torch.float32, device=x.device)
    return _LatentRate.apply(x, keep.detach().to(torch.float32).contiguous().reshape(frames), int(bits),
                             cost.detach().contiguous().reshape(256))


def rans_supported(hw, ld, bits):
    """Do vvae_rans_encode / vvae_rans_decode take frames of ``hw`` tokens x ``ld`` channels at ``bits``?"""
    return bool(lib().vvae_rans_supported(int(hw), int(ld), int(bits)))


def _rans_table(name, freq, bits, dev, contexts=None):
    """The frequency table of entropy.py as a uint16 tensor on ``dev``: (2 qmax + 1,), or with ``contexts`` the context coder's
    (contexts, 2 qmax + 1).  A host array (or CPU tensor) is checked against the definition (its shape, its rows' sum 4096) and uploaded;
    a tensor already on ``dev`` (uint16 or int16, as inside a captured graph) is taken as it is: the kernels stay inside their tables for
    any content."""
    import numpy as np
    from .entropy import _table, table_size
    try:
        size = table_size(bits)
        if torch.is_tensor(freq) and freq.is_cuda:
            fits = freq.numel() == size if contexts is None else tuple(freq.shape) == (contexts, size)
            if freq.device != dev or freq.dtype not in (torch.uint16, torch.int16) or not fits or not freq.is_contiguous():
                want = f"table must be contiguous uint16 ({size},)" if contexts is None else f"tables must be contiguous uint16 ({contexts}, {size})"
                raise ValueError(f"the {want} on {dev}; got {freq.dtype} {tuple(freq.shape)} on {freq.device}")
            return freq
        host = freq.detach().numpy() if torch.is_tensor(freq) else np.asarray(freq)
        _table(host, bits, contexts)
        return torch.from_numpy(np.ascontiguousarray(host.astype(np.uint16))).to(dev)
    except ValueError as e:
        raise VvaeError(f"{name}: {e}") from None


def _rans_frames(name, codes, keep):
    """(lead, hw, ld, frames, keep as contiguous fp32) of the codes (..., hw, ld) and flags of an encoder-side rANS op."""
    if not torch.is_tensor(codes) or not codes.is_cuda:
        raise VvaeError(f"{name}: video_vae_amd ops need GPU tensors (no CPU fallback)")
    if codes.dtype != torch.int8 or codes.dim() < 3 or not codes.is_contiguous():
        raise VvaeError(f"{name}: codes must be contiguous int8 (..., hw, ld); got {codes.dtype} {tuple(codes.shape)} strides {codes.stride()}")
    lead, (hw, ld) = tuple(codes.shape[:-2]), codes.shape[-2:]
    frames = 1
    for v in lead:
        frames *= v
    if not torch.is_tensor(keep) or keep.device != codes.device or keep.numel() != frames:
        raise VvaeError(f"{name}: keep must hold one flag per frame ({frames}) on {codes.device}")
    if keep.dtype != torch.float32 or not keep.is_contiguous():
        keep = keep.to(torch.float32).contiguous()
    return lead, hw, ld, frames, keep


def _rans_supported(name, hw, ld, bits):
    if not lib().vvae_rans_supported(int(hw), int(ld), int(bits)):
        raise VvaeError(f"{name}: frames of {hw} x {ld} at {bits} bits are outside what the kernel takes (bits 2 .. 8, hw, ld >= 1, "
                        "hw ld <= 2^30)")


def _rans_coded_out(name, out, lead, hw, ld, dev):
    """The CodedFrames an encoder writes into, in the capacity layout: ``out`` checked, or new tensors."""
    from .entropy import CodedFrames, LANES, capacity
    want = ((lead + (capacity(hw * ld),), torch.uint16), (lead, torch.int32), (lead + (LANES,), torch.uint32))
    if out is None:
        return CodedFrames(*[torch.empty(shape, dtype=dtype, device=dev) for shape, dtype in want])
    for t, (shape, dtype) in zip(out, want):
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev:
            raise VvaeError(f"{name}: out must hold contiguous {dtype} {shape} on {dev}; got {t.dtype} {tuple(t.shape)}")
    return out


def _rans_streams(name, words, offsets, n_words, state, hw, ld):
    """The decoder-side arguments checked -> (frames, offsets int64, n_words int32, new codes int8 (frames, hw, ld), new ok int32 (frames,))."""
    from .entropy import LANES
    if not torch.is_tensor(words) or not words.is_cuda:
        raise VvaeError(f"{name}: video_vae_amd ops need GPU tensors (no CPU fallback)")
    dev = words.device
    if words.dtype not in (torch.uint16, torch.int16) or not words.is_contiguous():
        raise VvaeError(f"{name}: words must be contiguous uint16; got {words.dtype} {tuple(words.shape)} strides {words.stride()}")
    for what, t in (("offsets", offsets), ("n_words", n_words), ("state", state)):
        if not torch.is_tensor(t) or t.device != dev:
            raise VvaeError(f"{name}: {what} must be a tensor on {dev}")
    frames = n_words.numel()
    if offsets.numel() != frames or offsets.is_floating_point() or n_words.is_floating_point():
        raise VvaeError(f"{name}: offsets {tuple(offsets.shape)} and n_words {tuple(n_words.shape)} must be integers, one per frame")
    if state.dtype not in (torch.uint32, torch.int32) or state.numel() != frames * LANES or not state.is_contiguous():
        raise VvaeError(f"{name}: state must be contiguous uint32 ({frames}, {LANES}); got {state.dtype} {tuple(state.shape)}")
    return (frames, offsets.to(torch.int64).contiguous(), n_words.to(torch.int32).contiguous(),
            torch.empty((frames, int(hw), int(ld)), dtype=torch.int8, device=dev), torch.empty((frames,), dtype=torch.int32, device=dev))


def rans_encode(codes, keep, freq, bits, out=None):
    """Entropy-code the frames of ``codes`` (..., hw, ld) (int8, contiguous, on a GPU; within +-qmax of ``bits``) whose ``keep`` flag (one per
    frame, the leading dimensions) is nonzero, with the table ``freq`` (entropy.normalise_counts; positive on every code of a kept frame):
    entropy.encode_reference on every word, count and state (vvae_rans_encode: one launch, one wavefront per frame, safe inside a captured
    hipGraph) -> entropy.CodedFrames of GPU tensors in the capacity layout: ``words`` uint16 (..., capacity) with capacity = ceil(hw ld / 64)
    64 and a frame's stream in the LAST n_words entries of its row (the head of the row is not written), ``n_words`` int32 (...),
    ``state`` uint32 (..., 64).  A frame whose flag is zero is not read: n_words 0, states 2^16.  entropy.gather_streams brings the result to
    the host layout.  ``out``: a CodedFrames of contiguous tensors of those shapes to write into."""
    lead, hw, ld, frames, keep = _rans_frames("rans_encode", codes, keep)
    _rans_supported("rans_encode", hw, ld, bits)
    table = _rans_table("rans_encode", freq, bits, codes.device)
    out = _rans_coded_out("rans_encode", out, lead, hw, ld, codes.device)
    if frames == 0:
        return out
    check(_launch(f"rans_encode {hw}x{ld} b{int(bits)}", frames * hw * ld * 2, 0, "rans_encode_kernel",
                  lambda: lib().vvae_rans_encode(_p(codes), _p(keep), _p(table), _p(out.words), _p(out.n_words), _p(out.state), frames, hw, ld,
                                                 int(bits), _stream())),
          "vvae_rans_encode")
    return out


def rans_decode(words, offsets, n_words, state, freq, bits, hw, ld):
    """Decode frames of ``hw`` x ``ld`` codes: frame f's stream is ``words.reshape(-1)[offsets[f] : offsets[f] + n_words[f]]`` (words uint16,
    contiguous, any shape: the capacity layout of ``rans_encode`` with offsets f capacity + capacity - n_words[f], or streams concatenated
    as in a latent file), ``state`` uint32 (frames, 64) the encoder's final states, ``freq`` the stored table: entropy.decode_reference on
    every code (vvae_rans_decode: one launch, safe inside a captured hipGraph) -> (codes int8 (frames, hw, ld), ok int32 (frames,)).
    ``ok`` is 1 where the stream lies inside ``words``, every word of it was consumed and every lane came back to 2^16 -- the caller
    checks it; no read leaves the frame's stream whatever the counts and states hold."""
    _rans_supported("rans_decode", hw, ld, bits)
    frames, offsets, n_words, codes, ok = _rans_streams("rans_decode", words, offsets, n_words, state, hw, ld)
    table = _rans_table("rans_decode", freq, bits, words.device)
    if frames == 0:
        return codes, ok
    check(_launch(f"rans_decode {hw}x{ld} b{int(bits)}", frames * hw * ld * 2, 0, "rans_decode_kernel",
                  lambda: lib().vvae_rans_decode(_p(words), int(words.numel()), _p(offsets), _p(n_words), _p(state), _p(table), _p(codes), _p(ok),
                                                 frames, int(hw), int(ld), int(bits), _stream())),
          "vvae_rans_decode")
    return codes, ok


RANS_SLOT_FORMS = {None: -1, "compact": 0, "full": 1}


def rans_context_supported(hw, ld, bits, grid_w):
    """Do vvae_rans_context_counts / vvae_rans_encode_ctx / vvae_rans_decode_ctx take frames of ``hw`` tokens x ``ld`` channels at ``bits``
    laid out ``grid_w`` tokens wide?  (What vvae_rans_supported takes, hw <= 4096, grid_w >= 1 and (grid_w - 1) ld >= 63.)"""
    return bool(lib().vvae_rans_context_supported(int(hw), int(ld), int(bits), int(grid_w)))


def _rans_context(name, hw, ld, bits, grid_w, thr):
    """(grid_w, thr0, thr1) as ints, the frame checked against what the context kernels take."""
    if not rans_context_supported(hw, ld, bits, grid_w):
        raise VvaeError(f"{name}: frames of {hw} x {ld} at {bits} bits, {grid_w} tokens wide, are outside what the kernel takes (bits 2 .. 8, "
                        "hw in 1 .. 4096, ld >= 1, hw ld <= 2^30, grid_w >= 1, (grid_w - 1) ld >= 63)")
    thr0, thr1 = (int(v) for v in thr)
    if not (0 <= thr0 < 2 ** 31 and 0 <= thr1 < 2 ** 31):
        raise VvaeError(f"{name}: thresholds {thr0}, {thr1} outside 0 .. 2^31 - 1")
    return int(grid_w), thr0, thr1


def rans_context_counts(codes, keep, bits, grid_w, thr):
    """The code histograms per context of the frames of ``codes`` (..., hw, ld) (int8, contiguous, on a GPU) whose ``keep`` flag is
    nonzero, for the layout ``grid_w`` and the thresholds ``thr = (thr0, thr1)``: entropy.context_counts on every count
    (vvae_rans_context_counts: one launch, one workgroup per frame, safe inside a captured hipGraph) -> int32 (..., 4, 256),
    counts[..., ctx, q + 128]; zeros for a frame whose flag is zero, which is not read.  The caller sums the frames."""
    lead, hw, ld, frames, keep = _rans_frames("rans_context_counts", codes, keep)
    grid_w, thr0, thr1 = _rans_context("rans_context_counts", hw, ld, bits, grid_w, thr)
    counts = torch.empty(lead + (4, 256), dtype=torch.int32, device=codes.device)
    if frames == 0:
        return counts
    check(_launch(f"rans_context_counts {hw}x{ld} w{grid_w}", frames * hw * ld * 2, 0, "rans_context_counts_kernel",
                  lambda: lib().vvae_rans_context_counts(_p(codes), _p(keep), _p(counts), frames, hw, ld, int(bits), grid_w, thr0, thr1, _stream())),
          "vvae_rans_context_counts")
    return counts


def rans_encode_context(codes, keep, freq4, bits, grid_w, thr, out=None):
    """``rans_encode`` with the context coder's four tables ``freq4`` (entropy.normalise_context_counts; every row positive on the codes of
    its context), the layout ``grid_w`` and the thresholds ``thr``: entropy.encode_context_reference on every word, count and state
    (vvae_rans_encode_ctx) -> entropy.CodedFrames of GPU tensors in ``rans_encode``'s capacity layout."""
    from .entropy import CONTEXTS
    lead, hw, ld, frames, keep = _rans_frames("rans_encode_context", codes, keep)
    grid_w, thr0, thr1 = _rans_context("rans_encode_context", hw, ld, bits, grid_w, thr)
    tables = _rans_table("rans_encode_context", freq4, bits, codes.device, CONTEXTS)
    out = _rans_coded_out("rans_encode_context", out, lead, hw, ld, codes.device)
    if frames == 0:
        return out
    check(_launch(f"rans_encode_ctx {hw}x{ld} b{int(bits)} w{grid_w}", frames * hw * ld * 3, 0, "rans_encode_ctx_kernel",
                  lambda: lib().vvae_rans_encode_ctx(_p(codes), _p(keep), _p(tables), _p(out.words), _p(out.n_words), _p(out.state), frames, hw,
                                                     ld, int(bits), grid_w, thr0, thr1, _stream())),
          "vvae_rans_encode_ctx")
    return out


def rans_decode_context(words, offsets, n_words, state, freq4, bits, hw, ld, grid_w, thr, slot_form=None):
    """``rans_decode`` for a stream of the context coder: ``freq4`` the stored tables (4, 2 qmax + 1), ``grid_w`` and ``thr`` the stored layout
    and thresholds: entropy.decode_context_reference on every code (vvae_rans_decode_ctx: one launch, safe inside a captured hipGraph) ->
    (codes int8 (frames, hw, ld), ok int32 (frames,)), ``ok`` as in ``rans_decode``.  ``slot_form``: "full" (four full slot tables in 64 KB of
    dynamic LDS, one table read per step, one wave per CU), "compact" (a byte per slot and a second table read, three waves per CU), or
    None: the library picks "full" while every frame gets a CU of its own and "compact" beyond; both compute the same."""
    from .entropy import CONTEXTS
    grid_w, thr0, thr1 = _rans_context("rans_decode_context", hw, ld, bits, grid_w, thr)
    form = RANS_SLOT_FORMS.get(slot_form)
    if form is None:
        raise VvaeError(f"rans_decode_context: slot_form {slot_form!r}: None, 'compact' or 'full' expected")
    frames, offsets, n_words, codes, ok = _rans_streams("rans_decode_context", words, offsets, n_words, state, hw, ld)
    tables = _rans_table("rans_decode_context", freq4, bits, words.device, CONTEXTS)
    if frames == 0:
        return codes, ok
    check(_launch(f"rans_decode_ctx {hw}x{ld} b{int(bits)} w{grid_w}", frames * hw * ld * 2, 0,
                  "rans_decode_ctx_kernel",
                  lambda: lib().vvae_rans_decode_ctx(_p(words), int(words.numel()), _p(offsets), _p(n_words), _p(state), _p(tables), _p(codes),
                                                     _p(ok), frames, int(hw), int(ld), int(bits), grid_w, thr0, thr1, form, _stream())),
          "vvae_rans_decode_ctx")
    return codes, ok


def rans_temporal_supported(hw, ld, bits):
    """Do vvae_rans_temporal_counts / vvae_rans_encode_temporal / vvae_rans_decode_temporal take frames of ``hw`` tokens x ``ld`` channels
    at ``bits``?  (What vvae_rans_supported takes: the temporal coder needs no condition on the token grid.)"""
    return bool(lib().vvae_rans_temporal_supported(int(hw), int(ld), int(bits)))


def _rans_temporal(name, hw, ld, bits, thr):
    """The thresholds as the C array the launchers read (on the host: kernel arguments), the frame checked against what the kernels take."""
    import numpy as np
    from .entropy import TEMPORAL_CLASSES
    if not rans_temporal_supported(hw, ld, bits):
        raise VvaeError(f"{name}: frames of {hw} x {ld} at {bits} bits are outside what the kernel takes (bits 2 .. 8, hw, ld >= 1, "
                        "hw ld <= 2^30)")
    t = [int(v) for v in np.asarray(thr.detach().cpu() if torch.is_tensor(thr) else thr).reshape(-1)]
    if len(t) != TEMPORAL_CLASSES - 1 or any(b < a for a, b in zip(t, t[1:])) or t[0] < -2 ** 31 or t[-1] >= 2 ** 31:
        raise VvaeError(f"{name}: thresholds {t}: {TEMPORAL_CLASSES - 1} ascending 32-bit integers expected")
    return (ctypes.c_int * len(t))(*t)


def _rans_index(name, what, t, n, dev):
    """``t`` as the contiguous int32 (n,) tensor on ``dev`` a temporal kernel reads: a host array is uploaded, a tensor on ``dev`` (as inside
    a captured graph) must be int32 already."""
    import numpy as np
    if torch.is_tensor(t) and t.is_cuda:
        if t.device != dev or t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous():
            raise VvaeError(f"{name}: {what} must be contiguous int32 ({n},) on {dev}; got {t.dtype} {tuple(t.shape)} on {t.device}")
        return t
    host = np.asarray(t.detach().numpy() if torch.is_tensor(t) else t)
    if host.dtype.kind not in "ui" or host.size != n:
        raise VvaeError(f"{name}: {what} must hold {n} integers; got {host.dtype} {host.shape}")
    return torch.from_numpy(np.ascontiguousarray(host.reshape(-1).astype(np.int32))).to(dev)


def rans_temporal_counts(codes, keep, prev, bits, thr):
    """The code histograms per table row of the temporal coder, of the frames of ``codes`` (..., hw, ld) (int8, contiguous, on a GPU) whose
    ``keep`` flag is nonzero.  ``prev`` (one per frame; entropy.chain_prev): the flat index of the frame a kept frame is coded against, -1
    for one that starts a chain; ``thr`` the seven thresholds: entropy.temporal_counts on every count (vvae_rans_temporal_counts: one launch,
    one workgroup per frame, safe inside a captured hipGraph when ``prev`` is an int32 tensor on the GPU) -> int32 (..., 9, 256),
    counts[..., row, q + 128]; zeros for a frame whose flag is zero, which is not read.  The caller sums the frames."""
    from .entropy import TEMPORAL_TABLES
    lead, hw, ld, frames, keep = _rans_frames("rans_temporal_counts", codes, keep)
    thr = _rans_temporal("rans_temporal_counts", hw, ld, bits, thr)
    prev = _rans_index("rans_temporal_counts", "prev", prev, frames, codes.device)
    counts = torch.empty(lead + (TEMPORAL_TABLES, 256), dtype=torch.int32, device=codes.device)
    if frames == 0:
        return counts
    check(_launch(f"rans_temporal_counts {hw}x{ld}", frames * hw * ld * 2, 0, "rans_temporal_counts_kernel",
                  lambda: lib().vvae_rans_temporal_counts(_p(codes), _p(keep), _p(prev), _p(counts), frames, hw, ld, int(bits), thr, _stream())),
          "vvae_rans_temporal_counts")
    return counts


def rans_encode_temporal(codes, keep, prev, freq9, bits, thr, out=None):
    """``rans_encode`` with the temporal coder's nine tables ``freq9`` (entropy.normalise_temporal_counts; every row positive on the codes
    that use it), ``prev`` and ``thr`` as in ``rans_temporal_counts``: entropy.encode_temporal_reference on every word, count and state of the
    kept frames (vvae_rans_encode_temporal: one wavefront per frame) -> entropy.CodedFrames of GPU tensors in ``rans_encode``'s capacity
    layout."""
    from .entropy import TEMPORAL_TABLES
    lead, hw, ld, frames, keep = _rans_frames("rans_encode_temporal", codes, keep)
    thr = _rans_temporal("rans_encode_temporal", hw, ld, bits, thr)
    prev = _rans_index("rans_encode_temporal", "prev", prev, frames, codes.device)
    tables = _rans_table("rans_encode_temporal", freq9, bits, codes.device, TEMPORAL_TABLES)
    out = _rans_coded_out("rans_encode_temporal", out, lead, hw, ld, codes.device)
    if frames == 0:
        return out
    check(_launch(f"rans_encode_temporal {hw}x{ld} b{int(bits)}", frames * hw * ld * 3, 0, "rans_encode_temporal_kernel",
                  lambda: lib().vvae_rans_encode_temporal(_p(codes), _p(keep), _p(prev), _p(tables), _p(out.words), _p(out.n_words),
                                                          _p(out.state), frames, hw, ld, int(bits), thr, _stream())),
          "vvae_rans_encode_temporal")
    return out


def rans_decode_temporal(words, offsets, n_words, state, freq9, bits, hw, ld, chain_start, thr):
    """``rans_decode`` for a stream of the temporal coder: ``freq9`` the stored tables (9, 2 qmax + 1), ``thr`` the stored thresholds,
    ``chain_start`` (chains + 1,) (entropy.chain_starts of the stored chain flags; a host array, or an int32 tensor on the GPU as inside a
    captured graph): chain c holds the coded frames chain_start[c] .. chain_start[c + 1] - 1.  entropy.decode_temporal_reference on every
    code (vvae_rans_decode_temporal: one launch, one wavefront per chain, safe inside a captured hipGraph) -> (codes int8 (frames, hw,
    ld), ok int32 (frames,)), ``ok`` per frame as in ``rans_decode``; a frame behind an invalid frame of its chain is decoded from what that
    frame produced, so the caller trusts a chain up to its first ``ok == 0``."""
    from .entropy import TEMPORAL_TABLES
    frames, offsets, n_words, codes, ok = _rans_streams("rans_decode_temporal", words, offsets, n_words, state, hw, ld)
    thr = _rans_temporal("rans_decode_temporal", hw, ld, bits, thr)
    tables = _rans_table("rans_decode_temporal", freq9, bits, words.device, TEMPORAL_TABLES)
    chains = int(chain_start.numel() if torch.is_tensor(chain_start) else len(chain_start)) - 1
    if frames == 0:
        return codes, ok
    if not 1 <= chains <= frames:
        raise VvaeError(f"rans_decode_temporal: {chains} chains for {frames} frames")
    chain_start = _rans_index("rans_decode_temporal", "chain_start", chain_start, chains + 1, words.device)
    check(_launch(f"rans_decode_temporal {hw}x{ld} b{int(bits)}", frames * hw * ld * 3, 0, "rans_decode_temporal_kernel",
                  lambda: lib().vvae_rans_decode_temporal(_p(words), int(words.numel()), _p(offsets), _p(n_words), _p(state), _p(tables),
                                                          _p(codes), _p(ok), _p(chain_start), chains, frames, int(hw), int(ld), int(bits), thr,
                                                          _stream())),
          "vvae_rans_decode_temporal")
    return codes, ok


# --------------------------------------------------------------------------------------------- LayerNorm
def _rows2(x):
    """x (..., C) as rows with two-level strides: row r at (r // inner) * outer_pitch + (r % inner) * inner_pitch.

    Returns (tensor, rows, inner, outer_pitch, inner_pitch); copies only if the layout cannot be expressed that way."""
    c = x.shape[-1]
    n = x.numel() // c
    if x.is_contiguous():
        return x, n, 1, c, 0
    if x.dim() >= 3 and x.stride(-1) == 1:
        inner, ip = x.shape[-2], x.stride(-2)
        lead = x.shape[:-2]
        ok, pitch = True, None
        # leading dims must collapse to one uniform outer pitch
        strides = [x.stride(i) for i in range(len(lead))]
        for i in range(len(lead) - 1):
            if lead[i] != 1 and strides[i] != strides[i + 1] * lead[i + 1]:
                ok = False
        if ok and len(lead) >= 1:
            pitch = strides[-1]
            return x, n, inner, pitch, ip
    x = x.contiguous()
    return x, n, 1, c, 0


class _LayerNorm(torch.autograd.Function):
    """fork=True is the pre-norm residual form ``x + f(LN(x))``: forward also hands x back (an alias), so the gradient of the skip
    path arrives in THIS node's backward and is added inside the LayerNorm-backward kernel instead of by a separate add launch."""

    @staticmethod
    def forward(ctx, x_in, scale, bias, eps, fork):
        x, n, inner, op, ip = _rows2(x_in)
        c = x.shape[-1]
        dt = _dt(x)
        s32 = _f32(scale)
        b32 = _f32(bias) if bias is not None else None
        y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        mean = torch.empty((n,), dtype=torch.float32, device=x.device)
        rstd = torch.empty((n,), dtype=torch.float32, device=x.device)
        check(_launch(f"layernorm_fwd C{c}", 2 * x.numel() * x.element_size(), 0, "layernorm_fwd_kernel",
                      lambda: lib().vvae_layernorm_fwd(_p(x), _p(y), _p(s32), _p(b32), _p(mean), _p(rstd), None, None, n, c, inner, op, ip,
                                                       eps, dt, _stream())), "vvae_layernorm_fwd")
        ctx.save_for_backward(x, s32, mean, rstd)
        ctx.args = (n, c, inner, op, ip, scale.dtype, bias is not None)
        ctx.sparam, ctx.bparam = scale, bias
        ctx.set_materialize_grads(False)
        if fork:
            return y, x_in.view_as(x_in)
        return y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        dx, dsc, dbi = _ln_backward(ctx, dy, dskip)
        return dx, dsc, dbi, None, None


def _ln_backward(ctx, dy, dskip):
    """Shared by _LayerNorm and _AddLayerNorm: LayerNorm backward with the residual-stream gradient added in the kernel."""
    x, s32, mean, rstd = ctx.saved_tensors
    n, c, inner, op, ip, pdtype, has_bias = ctx.args
    dt = _dt(x)
    if dy is None:                                   # only the skip path was used
        return dskip, None, None
    dy = dy.to(x.dtype).contiguous()
    if dskip is not None:
        dskip = dskip.to(x.dtype).contiguous()
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    nblk = lib().vvae_layernorm_bwd_blocks(n, c, dt)
    part = torch.empty((nblk, 2, c), dtype=torch.float32, device=x.device)
    nstreams = 4 if dskip is not None else 3
    check(_launch(f"layernorm_bwd C{c}" + ("+skip" if dskip is not None else ""), nstreams * x.numel() * x.element_size(), 0,
                  "layernorm_bwd_kernel",
                  lambda: lib().vvae_layernorm_bwd(_p(x), _p(dy), _p(s32), _p(mean), _p(rstd), _p(dskip), _p(dx), _p(part), n, c, inner,
                                                   op, ip, dt, _stream())), "vvae_layernorm_bwd")
    g0, g1 = fold_partials(part, ctx.sparam, ctx.bparam, c)
    if g0 is None:
        return dx, None, None
    return dx, g0.to(pdtype), (g1.to(pdtype) if has_bias else None)


class _AddLayerNorm(torch.autograd.Function):
    """(LayerNorm(skip + o), skip + o) in one pass: the residual add that closes a pre-norm block fused with the LayerNorm that opens
    the next one.  Backward is LayerNorm backward + the gradient of the sum, which goes to both addends unchanged."""

    @staticmethod
    def forward(ctx, skip, o, scale, bias, eps):
        skip = skip.contiguous()
        o = o.to(skip.dtype).reshape(skip.shape).contiguous()
        n, c = skip.numel() // skip.shape[-1], skip.shape[-1]
        dt = _dt(skip)
        s32 = _f32(scale)
        b32 = _f32(bias) if bias is not None else None
        y = torch.empty(skip.shape, dtype=skip.dtype, device=skip.device)
        xs = torch.empty(skip.shape, dtype=skip.dtype, device=skip.device)
        mean = torch.empty((n,), dtype=torch.float32, device=skip.device)
        rstd = torch.empty((n,), dtype=torch.float32, device=skip.device)
        check(_launch(f"add_layernorm_fwd C{c}", 4 * skip.numel() * skip.element_size(), 0, "layernorm_fwd_kernel",
                      lambda: lib().vvae_layernorm_fwd(_p(skip), _p(y), _p(s32), _p(b32), _p(mean), _p(rstd), _p(o), _p(xs), n, c, 1, c, 0,
                                                       eps, dt, _stream())), "vvae_layernorm_fwd")
        ctx.save_for_backward(xs, s32, mean, rstd)
        ctx.args = (n, c, 1, c, 0, scale.dtype, bias is not None)
        ctx.sparam, ctx.bparam = scale, bias
        ctx.set_materialize_grads(False)
        return y, xs

    @staticmethod
    def backward(ctx, dy, dxs=None):
        dx, dsc, dbi = _ln_backward(ctx, dy, dxs)
        return dx, dx, dsc, dbi, None


def layer_norm_supported(x):
    return x.is_cuda and x.dtype in DT and lib().vvae_layernorm_supported(x.shape[-1], DT[x.dtype]) == 1


def layer_norm(x, scale, bias=None, eps=1e-6):
    """nnx.LayerNorm over the last axis, fp32 statistics (reference train/layers.py:17,152,155-156,178)."""
    return _LayerNorm.apply(x, scale, bias, eps, False)


def add_layer_norm_fork(skip, o, scale, bias=None, eps=1e-6):
    """-> (LayerNorm(skip + o), skip + o), one kernel pass (reference train/layers.py:212-221: ``x = x + f(...)`` followed by the
    next block's LayerNorm)."""
    return _AddLayerNorm.apply(skip, o, scale, bias, eps)


def layer_norm_fork(x, scale, bias=None, eps=1e-6):
    """-> (LayerNorm(x), x): the second output is x itself, routed through the node so that in ``x_skip + f(y)`` the skip
    gradient is added inside the LayerNorm-backward kernel (pre-norm residual blocks, reference train/layers.py:212-221)."""
    return _LayerNorm.apply(x, scale, bias, eps, True)


def silu_bf16(x):
    """silu(x) for a contiguous bf16 GPU tensor (no autograd: layers._SiluLinearBf16 owns the backward)."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and x.numel() % 8 == 0 and x.data_ptr() % 16 == 0):
        return F.silu(x)
    y = torch.empty_like(x)
    check(_launch(f"silu {x.numel() >> 20}M", 4 * x.numel(), 0, "silu_bf16_kernel", lambda: lib().vvae_silu_bf16(_p(x), _p(y), x.numel(), _stream())),
          "vvae_silu_bf16")
    return y


# --------------------------------------------------------------------------------------------- Linear + bias + residual (library GEMM)
_LT_WS = {}


def linear_residual_ok(x2, wb, bb, res):
    """bf16 GPU operands the residual-accumulating library product takes (contiguous rows, 16-byte aligned)."""
    ts = (x2, wb, res) if bb is None else (x2, wb, res, bb)
    return (all(t.is_cuda and t.dtype == torch.bfloat16 for t in ts) and x2.dim() == 2 and res.dim() == 2 and x2.stride(1) == 1
            and wb.is_contiguous() and res.stride(1) == 1 and res.shape == (x2.shape[0], wb.shape[1]) and x2.shape[1] == wb.shape[0]
            and x2.shape[1] % 8 == 0 and wb.shape[1] % 8 == 0 and x2.stride(0) % 8 == 0 and res.stride(0) % 8 == 0
            and x2.data_ptr() % 16 == 0 and res.data_ptr() % 16 == 0)


def linear_residual(x2, wb, bb, res, wt=None):
    """-> x2 @ wb + bb + res (bf16, fp32 accumulation, one rounding): vvae_linear_residual_bf16.  ``res`` None = plain Linear.
    ``wt``: wb's (N, K) contiguous transpose, if the caller keeps one: the library's faster operand form (vvae_linear_residual_wt_bf16)."""
    m, k = x2.shape
    n = wb.shape[1]
    out = torch.empty((m, n), dtype=torch.bfloat16, device=x2.device)
    ws = _LT_WS.get(x2.device)
    if ws is None:
        ws = _LT_WS[x2.device] = torch.empty(32 << 20, dtype=torch.uint8, device=x2.device)
    ldr = res.stride(0) if res is not None else 0
    if wt is not None and wt.is_contiguous() and wt.shape == (n, k) and wt.dtype == torch.bfloat16:
        entry, w, ldw = lib().vvae_linear_residual_wt_bf16, wt, k
    else:
        entry, w, ldw = lib().vvae_linear_residual_bf16, wb, n
    check(_launch(f"linear+residual {m}x{n} K{k}", (m * k + k * n + (2 if res is not None else 1) * m * n) * 2, 2 * m * n * k, "Cijk_",
                  lambda: entry(_p(x2), x2.stride(0), _p(w), ldw, _p(bb), 1, _p(res), ldr, _p(out), n, m, n, k, _p(ws), ws.numel(), _stream())),
          "vvae_linear_residual_bf16")
    return out


# --------------------------------------------------------------------------------------------- dense NT GEMM (Linear fwd / dgrad)
EPI_NONE, EPI_RES, EPI_SILU, EPI_MUL_DSILU = 0, 1, 2, 3


def gemm_nt_supported(a, b):
    return (a.is_cuda and a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and a.dim() == 2 and b.dim() == 2
            and a.stride(1) == 1 and b.stride(1) == 1 and a.shape[1] == b.shape[1]
            and lib().vvae_gemm_nt_supported(a.shape[0], b.shape[0], a.shape[1], a.stride(0), b.stride(0), b.shape[0]) == 1)


def gemm_nt(a, b, bias=None, res=None, epi=EPI_NONE, form=None):
    """epi(a (M, K) @ b (N, K)^T + bias) in bf16 with fp32 accumulation (no autograd).  epi = EPI_RES adds ``res`` (M, N);
    EPI_SILU returns (silu(h), h); EPI_MUL_DSILU multiplies by silu'(res).  The product runs on csrc/gemm_pp.hip where that takes the
    shape, else on gemm_nt.hip (K = 64, N above its bias limit); ``form``: "nt" / "pp" forces one of the two (the tests' reference)."""
    m, k = a.shape
    n = b.shape[0]
    c = torch.empty((m, n), dtype=torch.bfloat16, device=a.device)
    c2 = torch.empty((m, n), dtype=torch.bfloat16, device=a.device) if epi == EPI_SILU else None
    if res is not None:
        res = res.reshape(m, n)
        if res.stride(1) != 1:
            res = res.contiguous()
    nbytes = (m * k + n * k + m * n * (1 + (epi != EPI_NONE))) * 2
    pp = form != "nt" and lib().vvae_gemm_pp_supported(m, n, k, a.stride(0), b.stride(0), n) == 1
    if form == "pp" and not pp:
        raise VvaeError(f"gemm_pp does not take {m} x {n} x {k}")
    name = "gemm_pp" if pp else "gemm_nt"
    entry = getattr(lib(), f"vvae_{name}_bf16")
    check(_launch(f"{name} {m}x{n} K{k} epi{epi}", nbytes, 2 * m * n * k, f"{name}_kernel",
                  lambda: entry(_p(a), a.stride(0), _p(b), b.stride(0), _p(c), n, _p(bias), _p(res), res.stride(0) if res is not None else 0,
                                _p(c2), n, epi, m, n, k, _stream())),
          f"vvae_{name}_bf16")
    return (c, c2) if epi == EPI_SILU else c


# --------------------------------------------------------------------------------------------- (out, in) bf16 weight shadows
def transpose_grouped(pairs):
    """(src (in, out), dst (out, in)) bf16 pairs -> dst = src^T, one grouped launch per 64 pairs."""
    for i0 in range(0, len(pairs), 64):
        e = pairs[i0:i0 + 64]
        n = len(e)
        VP, IA = ctypes.c_void_p * n, ctypes.c_int * n
        check(lib().vvae_transpose_grouped_bf16(VP(*[a.data_ptr() for a, _ in e]), VP(*[b.data_ptr() for _, b in e]),
                                                IA(*[a.shape[0] for a, _ in e]), IA(*[a.shape[1] for a, _ in e]), n, _stream()),
              "vvae_transpose_grouped_bf16")


def transposed_shadows(params, device):
    """``p.bf16_t`` (out, in), the weight operand of gemm_nt's forward products, for every parameter the layers marked ``want_t``: views
    of one zeroed buffer -> (buffer or None, [(p.bf16, p.bf16_t)]); the caller fills them (transpose_grouped) after every write of p.bf16.
    The grouped transpose moves 64 x 64 tiles between 16-byte aligned operands: a marked parameter with another shape, or whose p.bf16
    slot sits behind an odd-sized one, gets no such shadow and its forward runs the library product."""
    want = [p for p in params if getattr(p, "want_t", False) and p.dim() == 2 and p.shape[0] % 64 == 0 and p.shape[1] % 64 == 0
            and p.bf16.data_ptr() % 16 == 0]
    if not want:
        return None, []
    buf = torch.zeros(sum(p.numel() for p in want), dtype=torch.bfloat16, device=device)
    o = 0
    for p in want:
        p.bf16_t = buf[o:o + p.numel()].view(p.shape[1], p.shape[0])
        o += p.numel()
    return buf, [(p.bf16, p.bf16_t) for p in want]


# --------------------------------------------------------------------------------------------- deferred, grouped dense weight gradients
WGRAD_QUEUE = [None]          # a list while a ``deferred_wgrad`` block is open: Linear backward parks (x, dy, kernel, bias) there
GROUP_MAX = 64                # products per grouped launch (kernel-argument table)
GROUP_TILES = 512             # close a group once it holds about this many 256x256 tiles: two full rounds over 256 CUs
GROUP_MIN_TILES = 128         # below this many 256x256 tiles a launch cannot fill the chip without splitting K: per-product path


class deferred_wgrad:
    """``with deferred_wgrad(optimizer): loss.backward()``.

    Weight gradients are not on backward's critical path (only the input gradients are), so the Linear layers of the transformer
    trunk park their (input, output-gradient) pairs instead of launching one split-K product each; whenever about GROUP_TILES
    256x256 tiles have been parked (and on exit) the pairs are multiplied in ONE grouped launch -- hundreds of whole-K tiles at
    once, so nothing is split and nothing is reduced -- straight into the parameters' slots of the optimizer's flat gradient buffer
    (``param.gview``).  The optimizer is told (``optimizer.mark_external``) so that it neither zeroes nor copies those slots and
    can hand completed gradient buckets to the data-parallel reducer while backward is still running.
    """

    def __init__(self, optimizer):
        self.opt = optimizer

    def __enter__(self):
        WGRAD_QUEUE[0] = _WgradQueue(self.opt)
        return self

    def __exit__(self, et, ev, tb):
        q, WGRAD_QUEUE[0] = WGRAD_QUEUE[0], None
        if et is None:
            q.flush()
            q.flush_folds()
        return False


FOLD_MAX = 64                 # partial buffers per grouped fold launch


class _WgradQueue:
    def __init__(self, optimizer):
        self.opt, self.items, self.tiles, self.k, self.seen = optimizer, [], 0, None, set()
        self.folds = []                                      # parked (partial rows, param0, param1) of LayerNorm / q-k-norm scales

    def append_fold(self, part, p0, p1):
        self.folds.append((part, p0, p1))
        if len(self.folds) == FOLD_MAX:
            self.flush_folds()

    @staticmethod
    def _fold_launch(entries):
        """entries: (part pointer, d0 pointer, d1 pointer or None, rows, cols, n0), at most FOLD_MAX per launch."""
        for i0 in range(0, len(entries), FOLD_MAX):
            e = entries[i0:i0 + FOLD_MAX]
            n = len(e)
            VP, IA = ctypes.c_void_p * n, ctypes.c_int * n
            check(lib().vvae_fold_rows_grouped(VP(*[x[0] for x in e]), VP(*[x[1] for x in e]), VP(*[x[2] for x in e]),
                                               IA(*[x[3] for x in e]), IA(*[x[4] for x in e]), IA(*[x[5] for x in e]), n, _stream()),
                  "vvae_fold_rows_grouped")

    def flush_folds(self):
        folds, self.folds = self.folds, []
        if not folds:
            return
        first, second, keep = [], [], []
        for part, p0, p1 in folds:
            rows = part.shape[0]
            cols = part.numel() // rows
            d0, d1 = p0.gview.data_ptr(), (p1.gview.data_ptr() if p1 is not None else None)
            r, c, k = _tall_narrow_split(rows, cols)
            if k == 1:
                first.append((part.data_ptr(), d0, d1, rows, cols, p0.numel()))
            else:
                tmp = torch.empty((k, cols), dtype=torch.float32, device=part.device)
                keep.append(tmp)
                first.append((part.data_ptr(), tmp.data_ptr(), None, r, c, c))
                second.append((tmp.data_ptr(), d0, d1, k, cols, p0.numel()))
        self._fold_launch(first)
        self._fold_launch(second)
        for _, p0, p1 in folds:
            self.opt.mark_external(p0)
            if p1 is not None:
                self.opt.mark_external(p1)

    def claim(self, kernel):
        if id(kernel) in self.seen:                          # a weight used twice in one step would need accumulation
            raise VvaeError("deferred_wgrad: a kernel was used twice in one backward pass")
        self.seen.add(id(kernel))

    def append(self, item):
        x2, dy2, kernel, bias = item
        self.claim(kernel)
        t = (x2.shape[1] // 256) * (dy2.shape[1] // 256)
        if self.items and (x2.shape[0] != self.k or len(self.items) == GROUP_MAX or self.tiles + t > GROUP_TILES):
            self.flush()
        self.items.append(item); self.tiles += t; self.k = x2.shape[0]

    def flush(self):
        items, tiles, k = self.items, self.tiles, self.k
        self.items, self.tiles = [], 0
        if items:
            flush_wgrad(items, self.opt, tiles, k)


def wgrad_deferrable(x2, dy2, kernel, bias):
    """Linear.backward asks: may this product be parked?  (bf16 GPU operands, flat-buffer slots present, 256-multiples.)"""
    if WGRAD_QUEUE[0] is None or getattr(kernel, "gview", None) is None or (bias is not None and getattr(bias, "gview", None) is None):
        return False
    k, m = x2.shape
    n = dy2.shape[1]
    return (x2.is_cuda and x2.dtype == torch.bfloat16 and dy2.dtype == torch.bfloat16 and x2.stride(1) == 1 and dy2.stride(1) == 1
            and m % 256 == 0 and n % 256 == 0 and k % 32 == 0 and x2.stride(0) % 8 == 0 and dy2.stride(0) % 8 == 0
            and x2.data_ptr() % 16 == 0 and dy2.data_ptr() % 16 == 0)


def flush_wgrad(items, optimizer, tiles=None, k=None):
    """Multiply the parked pairs ``(x (K, M), dy (K, N), kernel, bias)`` (all with the same K, at most GROUP_MAX of them)."""
    if not items:
        return
    if tiles is None:
        tiles = sum((x2.shape[1] // 256) * (dy2.shape[1] // 256) for x2, dy2, _, _ in items)
        k = items[0][0].shape[0]
    if os.environ.get("VVAE_WGRAD_DEBUG"):
        print(f"[vvae] dense dW flush: {len(items)} products, {tiles} tiles of 256 x 256, K {k}: " + ("grouped" if tiles >= GROUP_MIN_TILES else "per product"), file=sys.stderr)
    if tiles >= GROUP_MIN_TILES:
        _gemm_tn_grouped(items, k)
    else:                                                    # too few tiles to fill the chip without splitting K
        for x2, dy2, kernel, bias in items:                  # straight into the flat-buffer slots: no copies behind the product
            gemm_tn(x2, dy2, bias is not None, kernel.gview, bias.gview if bias is not None else None)
    for _, _, kernel, bias in items:
        optimizer.mark_external(kernel)
        if bias is not None:
            optimizer.mark_external(bias)


def _gemm_tn_grouped(chunk, k):
    n = len(chunk)
    VP, IA = ctypes.c_void_p * n, ctypes.c_int * n
    a = VP(*[x2.data_ptr() for x2, _, _, _ in chunk])
    b = VP(*[dy2.data_ptr() for _, dy2, _, _ in chunk])
    c = VP(*[kn.gview.data_ptr() for _, _, kn, _ in chunk])
    db = VP(*[(bi.gview.data_ptr() if bi is not None else None) for _, _, _, bi in chunk])
    lda = IA(*[x2.stride(0) for x2, _, _, _ in chunk])
    ldb = IA(*[dy2.stride(0) for _, dy2, _, _ in chunk])
    ms = IA(*[x2.shape[1] for x2, _, _, _ in chunk])
    ns = IA(*[dy2.shape[1] for _, dy2, _, _ in chunk])
    flops = sum(2 * k * x2.shape[1] * dy2.shape[1] for x2, dy2, _, _ in chunk)
    nbytes = sum(k * (x2.shape[1] + dy2.shape[1]) * 2 + x2.shape[1] * dy2.shape[1] * 4 for x2, dy2, _, _ in chunk)
    check(_launch(f"gemm_tn_grouped x{n} K{k}", nbytes, flops, "gemm_tn256_grouped_kernel",
                  lambda: lib().vvae_gemm_tn_grouped_bf16(a, lda, b, ldb, c, db, ms, ns, n, k, _stream())), "vvae_gemm_tn_grouped_bf16")


# --------------------------------------------------------------------------------------------- dense weight-gradient GEMM
def gemm_tn_supported(a, b):
    return (a.is_cuda and a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and a.dim() == 2 and b.dim() == 2
            and a.stride(1) == 1 and b.stride(1) == 1
            and lib().vvae_gemm_tn_supported(a.shape[1], b.shape[1], a.shape[0], a.stride(0), b.stride(0)) == 1)


def gemm_tn(a, b, want_colsum=True, out=None, out_colsum=None):
    """(a^T @ b, b.sum(0)) in fp32 for bf16 token-major a (K, M), b (K, N): dW and db of a Linear layer in one pass.
    ``out`` / ``out_colsum``: contiguous fp32 destinations (the parameters' slots of the flat gradient buffer) instead of fresh tensors."""
    k, m = a.shape
    n = b.shape[1]
    c = out if out is not None else torch.empty((m, n), dtype=torch.float32, device=a.device)
    db = (out_colsum if out_colsum is not None else torch.empty((n,), dtype=torch.float32, device=a.device)) if want_colsum else None
    assert c.is_contiguous() and c.dtype == torch.float32 and c.shape == (m, n)
    wsb = lib().vvae_gemm_tn_ws_bytes(m, n, k)
    ws, wsb = _ws(wsb, a.device)
    kern = ("gemm_tn256_kernel" if m % 256 == 0 and n % 256 == 0 and k % 32 == 0 else "gemm_tn_bf16_kernel") + " + gemm_tn_reduce_kernel"
    check(_launch(f"gemm_tn {m}x{n} K{k}", (k * (m + n)) * 2 + m * n * 4, 2 * m * n * k, kern,
                  lambda: lib().vvae_gemm_tn_bf16(_p(a), a.stride(0), _p(b), b.stride(0), _p(c), _p(db), m, n, k, _p(ws), wsb, _stream())),
          "vvae_gemm_tn_bf16")
    return c, db
