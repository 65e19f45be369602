#!/usr/bin/env python3
"""Generates tests/golden/metrics_parent_bits.npz: what the evaluation kernels (frame_metrics, frame_metrics_wide, ms_ssim, plane_metrics,
temporal_mse on GPU tensors) computed BEFORE the narrow and the strip form of the SSIM moment pass shared one plan, one launch path and
one kernel body, and before these kernels shared csrc/ssim_window.hpp, bit for bit.

    python tests/golden/make_metrics_parent_bits.py [ROOT]            (needs the GPU)

records the built ``video_vae_amd`` package under ROOT (default: this checkout).  tests/test_gpu_metrics.py calls ``record()`` on the
package it runs in and compares every member with ``torch.equal``.  Operands come from seeded CPU generators (and the committed
plane_metrics_*.y4m), so they are the same everywhere; the file holds outputs only: float32, and the int64 ``sse`` of the plane metrics.
It is written with fixed member dates, so a second run reproduces it byte for byte.

Every masked call has a masked frame: frame 1 of the flat (B T) order, or, for a one-frame shape, a second call with its only frame masked
(members ``..._masked``).  Members:
  fm_<shape>_<xy>_{mse,psnr,ssim}     frame_metrics; <xy> the operand dtypes (f = fp32, b = bf16); FM_SHAPES
  fmo_<shape>_<xy>_...                the same with x one element off a 16-byte boundary: the element-wise loads on a shape of 16-B rows
  fw_<shape>_<xy>_...                 frame_metrics_wide; FW_SHAPES (the first two are frame_metrics' limits: equal to their fm_ members)
  ms_<shape>_m<scales>_<xy>_{ms,terms}  ms_ssim with the terms; MS_CASES
  pm_{sse,ssim_y}                     plane_metrics of the planes of plane_metrics_ref.y4m / plane_metrics_test.y4m
  tm_<form>_<xy>                      temporal_mse of the two files' RGB frames / 255: ``odd`` whole frames (13 x 17 x 3 values, element-wise
                                      loads), ``vec`` their top left 12 x 16 (16-B loads)
"""
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "metrics_parent_bits.npz")
DTYPES = {"f": torch.float32, "b": torch.bfloat16}
PAIRS = ("ff", "fb", "bf", "bb")
# one window; rows not a multiple of 4 and three bands with halos; one channel; four; the widest rows of one strip (512 threads)
FM_SHAPES = [(1, 1, 11, 11, 3), (2, 3, 37, 53, 3), (2, 3, 24, 40, 1), (1, 2, 13, 17, 4), (1, 1, 16, 2048, 1), (1, 1, 16, 680, 3)]
FMO_SHAPE = (2, 3, 24, 40, 1)
# the two limits; one column past the limit (a second strip of a few columns); four channels; three strips
FW_SHAPES = [(1, 1, 16, 2048, 1), (1, 1, 16, 680, 3), (1, 1, 16, 681, 3), (1, 2, 16, 700, 4), (2, 2, 24, 3000, 1)]
# odd sides; strips at both levels; strips at level 0 and exactly the one-strip limit at level 1
MS_CASES = [((2, 2, 48, 48, 3), 3), ((1, 2, 44, 47, 3), 3), ((1, 2, 24, 1400, 3), 2), ((1, 1, 22, 4096, 1), 2)]
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def operands(shape, seed):
    """fp32 (x, y) on the CPU: y leaves [0, 1] in places, so clamping matters."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g)
    return x, x + 0.1 * torch.randn(shape, generator=g)


def masks(shape):
    """[(member suffix, (B, T) mask)]: every call sees a masked frame."""
    b, t = shape[:2]
    if b * t == 1:
        return [("", torch.ones(1, 1)), ("_masked", torch.zeros(1, 1))]
    m = torch.ones(b * t)
    m[1] = 0
    return [("", m.reshape(b, t))]


def off_by_one(v, dev):
    """``v`` on ``dev``, contiguous, its first element one element past an aligned allocation."""
    flat = torch.empty(v.numel() + 1, dtype=v.dtype, device=dev)
    flat[1:] = v.reshape(-1).to(dev)
    return flat[1:].view(v.shape)


def tag(shape):
    return "x".join(map(str, shape))


def y4m_operands():
    """((y, u, v) of the reference, of the test, RGB frames (n, H, W, 3) uint8 of each), numpy, from the committed .y4m pair."""
    from video_vae_amd import y4m
    out = []
    for name in ("plane_metrics_ref.y4m", "plane_metrics_test.y4m"):
        clip = y4m.Y4MClip(os.path.join(HERE, name))
        runs = [clip.planes(s, e) for s, e in clip.runs()]
        out.append((tuple(np.concatenate([np.array(r[p]) for r in runs]) for p in range(3)), clip[:]))
    return out


def record(dev="cuda"):
    """{member: tensor on the CPU} from the importable ``video_vae_amd`` on ``dev``."""
    from video_vae_amd import metrics, ops
    rec = {}

    def frames(prefix, fn, shapes, seed, prep=lambda v: v.to(dev)):
        for k, shape in enumerate(shapes):
            x32, y32 = operands(shape, seed + k)
            for pair in PAIRS:
                x, y = prep(x32.to(DTYPES[pair[0]])), y32.to(DTYPES[pair[1]]).to(dev)
                for sfx, mask in masks(shape):
                    fm = fn(x, y, mask.to(dev))
                    for name, v in zip(("mse", "psnr", "ssim"), fm):
                        rec[f"{prefix}_{tag(shape)}_{pair}{sfx}_{name}"] = v.cpu()

    frames("fm", metrics.frame_metrics, FM_SHAPES, 100)
    frames("fmo", metrics.frame_metrics, [FMO_SHAPE], 200, prep=lambda v: off_by_one(v, dev))
    frames("fw", metrics.frame_metrics_wide, FW_SHAPES, 100 + FM_SHAPES.index(FW_SHAPES[0]))      # the limits: fm's operands
    for k, (shape, m) in enumerate(MS_CASES):
        x32, y32 = operands(shape, 300 + k)
        for pair in PAIRS:
            x, y = x32.to(DTYPES[pair[0]]).to(dev), y32.to(DTYPES[pair[1]]).to(dev)
            for sfx, mask in masks(shape):
                ms, terms = metrics.ms_ssim(x, y, mask.to(dev), weights=MS_WEIGHTS[:m], return_terms=True)
                rec[f"ms_{tag(shape)}_m{m}_{pair}{sfx}_ms"] = ms.cpu()
                rec[f"ms_{tag(shape)}_m{m}_{pair}{sfx}_terms"] = terms.cpu()
    (pa, fa), (pb, fb) = y4m_operands()
    up = lambda planes: tuple(torch.from_numpy(p).to(dev) for p in planes)
    sse, ssim = ops.plane_metrics_u8(up(pa), up(pb), "420")
    rec["pm_sse"], rec["pm_ssim_y"] = sse.cpu(), ssim.cpu()
    xa, xb = (torch.from_numpy(f).float().div(255.0)[None] for f in (fa, fb))
    for form, crop in (("odd", (slice(None), slice(None))), ("vec", (slice(0, 12), slice(0, 16)))):
        a, b = (v[(slice(None), slice(None)) + crop].contiguous() for v in (xa, xb))
        for pair in PAIRS:
            rec[f"tm_{form}_{pair}"] = metrics.temporal_mse(a.to(DTYPES[pair[0]]).to(dev), b.to(DTYPES[pair[1]]).to(dev)).cpu()
    torch.cuda.synchronize()
    return rec


def write(path, rec):
    """np.savez_compressed with every member dated 1980-01-01, so that the bytes depend on the arrays alone."""
    with zipfile.ZipFile(path, "w") as zf:
        for name, value in rec.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with zf.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.asanyarray(value.numpy()), allow_pickle=False)


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE)))
    write(OUT, record())
    print(OUT)
