#!/usr/bin/env python3
"""Generates tests/golden/optim_parent_bits.json: what the optimizer tail of csrc/loss_optim.hip computed BEFORE its five entries
(vvae_sqnorm_partials / ..2, vvae_adam_clip_step / .._ema_step / .._acc_step) became two that select the kernel variant from ``acc`` and
``ema``, and the streaming passes shared one grid helper, bit for bit.

    python tests/golden/make_optim_parent_bits.py [ROOT [OUT]]            (needs the GPU)

records the built ``video_vae_amd`` package under ROOT (default: this checkout) into OUT (default: the fixture beside this script).  The
script looks at which entries the library exports and calls the five-entry ABI where it finds it, so it records from the commit before as
it stands.  tests/test_gpu_loss_optim_sweeps.py calls ``record()`` on the library it runs in and compares every member.  Operands are
seeded on the CPU, so they are the same everywhere; the fixture holds outputs only, each as dtype, shape and the SHA-256 of its raw bytes.
It is written with sorted keys, so a second run reproduces it byte for byte.

Members:
  adam_n<n>_ema<0|1>_acc<0|1>_<clip|noclip>_step<1..3>_<name>     three consecutive updates (count 1 to 3, a new gradient each) of one state, all
                                    four kernel variants, the clip biting (max_norm 1) and not (max_norm 1e6), at n = 4099 (a quad tail, one
                                    sweep) and n = 2 * 2^20 + 4099 (the sweeps test's N1: more than one sweep of both grids).  <name>: p, m, v,
                                    sh (the bf16 shadow), ema (where there is one), part (the fp64 partials), gnorm_sq.  Every buffer is
                                    hashed with its 8 guard elements
  fold_off<0|1>_<add|ovw>_dst       vvae_grad_fold_f32 at n = 4099, 16-byte aligned and one element off, with the guards on either side
  swap_off<0|1>_{a,b,sh}            vvae_swap_refresh_f32 at n = 4099 with a shadow, the same two alignments

A mismatch is a defect of the change, never a reason to record again: find the expression whose form moved and restore it.
"""
import ctypes
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "optim_parent_bits.json")
LENGTHS = (4099, 2 * 1048576 + 4099)
GUARD = 8
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, decay=0.99)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ok(code, what):
    assert code == 0, f"{what} returned {code}"


def _sqnorm(lib, g, acc, n, part, s):
    if not hasattr(lib, "vvae_sqnorm_partials2"):
        _ok(lib.vvae_sqnorm_partials(_vp(g), _vp(acc), n, _vp(part), s), "vvae_sqnorm_partials")
    elif acc is not None:
        _ok(lib.vvae_sqnorm_partials2(_vp(g), _vp(acc), n, _vp(part), s), "vvae_sqnorm_partials2")
    else:
        _ok(lib.vvae_sqnorm_partials(_vp(g), n, _vp(part), s), "vvae_sqnorm_partials")


def _adam(lib, p, g, acc, m, v, sh, ema, decay, tail, s):
    """``tail``: the arguments from n to count, the same in every form of the entry."""
    if not hasattr(lib, "vvae_adam_clip_acc_step"):
        _ok(lib.vvae_adam_clip_step(_vp(p), _vp(g), _vp(acc), _vp(m), _vp(v), _vp(sh), *tail, _vp(ema), decay if ema is not None else 0.0, s),
            "vvae_adam_clip_step")
    elif acc is not None:
        _ok(lib.vvae_adam_clip_acc_step(_vp(p), _vp(g), _vp(acc), _vp(m), _vp(v), _vp(sh), *tail, _vp(ema), decay if ema is not None else 0.0, s),
            "vvae_adam_clip_acc_step")
    elif ema is not None:
        _ok(lib.vvae_adam_clip_ema_step(_vp(p), _vp(g), _vp(m), _vp(v), _vp(sh), *tail, _vp(ema), decay, s), "vvae_adam_clip_ema_step")
    else:
        _ok(lib.vvae_adam_clip_step(_vp(p), _vp(g), _vp(m), _vp(v), _vp(sh), *tail, s), "vvae_adam_clip_step")


def describe(value):
    """{dtype, shape, sha256 of the raw bytes} of a tensor: what the fixture holds of a member."""
    raw = value.cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
    return {"dtype": str(value.dtype), "shape": list(value.shape), "sha256": hashlib.sha256(raw).hexdigest()}


def record(lib, dev="cuda"):
    """{member: describe(its tensor)} from the loaded library ``lib`` (video_vae_amd._lib.lib()) on ``dev``."""
    rec = {}
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator().manual_seed(20)
    rnd = lambda k: torch.randn(k, generator=gen)
    h = HYPER
    for n in LENGTHS:
        nb = n + GUARD
        p0, e0, a0 = rnd(nb), rnd(nb), rnd(nb).to(dev)
        gs = [rnd(nb).to(dev) for _ in range(3)]
        nparts = lib.vvae_sqnorm_blocks(n)
        for ema_on in (False, True):
            for acc_on in (False, True):
                for regime, max_norm in (("clip", 1.0), ("noclip", 1e6)):
                    p, m, v = p0.to(dev), torch.zeros(nb, device=dev), torch.zeros(nb, device=dev)
                    sh = torch.zeros(nb, dtype=torch.bfloat16, device=dev)
                    ema = e0.to(dev) if ema_on else None
                    acc = a0 if acc_on else None
                    part = torch.full((nparts + GUARD,), -1.0, dtype=torch.float64, device=dev)
                    out = torch.full((1 + GUARD,), -1.0, dtype=torch.float64, device=dev)
                    for step, g in enumerate(gs, 1):
                        _sqnorm(lib, g, acc, n, part, s)
                        tail = (n, _vp(part), nparts, _vp(out), 0.5 if acc_on else 1.0, max_norm, h["lr"], h["b1"], h["b2"], h["eps"], step)
                        _adam(lib, p, g, acc, m, v, sh, ema, h["decay"], tail, s)
                        key = f"adam_n{n}_ema{int(ema_on)}_acc{int(acc_on)}_{regime}_step{step}"
                        members = dict(p=p, m=m, v=v, sh=sh, part=part, gnorm_sq=out)
                        if ema_on:
                            members["ema"] = ema
                        for name, value in members.items():
                            rec[f"{key}_{name}"] = describe(value)
    n = LENGTHS[0]
    nb = n + 2 * GUARD + 1
    for off in (0, 1):
        lo = GUARD + off
        for name, overwrite in (("add", 0), ("ovw", 1)):
            dst, src = rnd(nb).to(dev), rnd(nb).to(dev)
            assert (dst[lo:].data_ptr() % 16 == 0) == (off == 0) and (src[lo:].data_ptr() % 16 == 0) == (off == 0)
            _ok(lib.vvae_grad_fold_f32(_vp(dst[lo:]), _vp(src[lo:]), n, overwrite, s), "vvae_grad_fold_f32")
            rec[f"fold_off{off}_{name}_dst"] = describe(dst)
        a, b = rnd(nb).to(dev), rnd(nb).to(dev)
        sh = torch.zeros(nb, dtype=torch.bfloat16, device=dev)
        _ok(lib.vvae_swap_refresh_f32(_vp(a[lo:]), _vp(b[lo:]), _vp(sh[lo:]), n, s), "vvae_swap_refresh_f32")
        rec.update({f"swap_off{off}_a": describe(a), f"swap_off{off}_b": describe(b), f"swap_off{off}_sh": describe(sh)})
    return rec


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE)))
    import video_vae_amd
    from video_vae_amd._lib import lib
    out = sys.argv[2] if len(sys.argv) > 2 else OUT
    with open(out, "w") as fh:
        json.dump(record(lib()), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(out, "recorded from", os.path.dirname(os.path.abspath(video_vae_amd.__file__)),
          "(five-entry ABI)" if hasattr(lib(), "vvae_adam_clip_acc_step") else "(two-entry ABI)")
