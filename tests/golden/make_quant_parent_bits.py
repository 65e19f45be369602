#!/usr/bin/env python3
"""Generates tests/golden/quant_parent_bits.json: what ops.latent_quantise, ops.latent_fake_quant and ops.latent_rate (forward and backward)
computed BEFORE the four kernels of csrc/quant.hip shared one front end, one frame loop, one launcher and one argument prologue, bit for
bit.  The other quantiser tests compare with quant.py on every bit except ``rate[f]``, which they hold to a summation bound: a changed order
of the fp32 sum would pass them.  Here its bits are recorded too.

    python tests/golden/make_quant_parent_bits.py [ROOT [OUT]]            (needs the GPU)

records the built ``video_vae_amd`` package under ROOT (default: this checkout).  tests/test_gpu_rate.py calls ``record()`` on the package it
runs in and compares every member.  Operands come from that file's recipe (``_case``, ``_keeps``, ``_gs``), seeded on the CPU, so they are the
same everywhere, and only the public ops are called; the fixture holds outputs only, each as dtype, shape and the SHA-256 of its raw bytes.
It is written with sorted keys, so a second run reproduces it byte for byte.

Members, for (frames, hw, ld) over tests/test_gpu_rate.py's SHAPES, <dtype> = bf16, fp32, bits 2, 4, 8 and k = 0, 1, 2 the entries of
``_keeps(frames)`` (one dropped frame; all kept; all dropped):
  F<frames>_HW<hw>_LD<ld>_<dtype>_b<bits>_k<k>_<name>, <name> one of
    codes, step, counts, dequantised     ops.latent_quantise(dequantise_in_place=True): its three outputs and the latent afterwards
    fake, fake_counts                    ops.latent_fake_quant: the new tensor and the histogram
    rate, rate_grad                      ops.latent_rate and the gradient its backward gives x under the incoming ``_gs(frames)``

A mismatch is a defect of the change, never a reason to record again: find the expression whose form moved and restore it.
"""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "quant_parent_bits.json")
BITS = (2, 4, 8)


def record(R, dev="cuda"):
    """{member: tensor on the CPU} from the importable ``video_vae_amd`` on ``dev``.  ``R``: the module tests/test_gpu_rate.py."""
    from video_vae_amd import ops
    rec = {}
    for frames, hw, ld in R.SHAPES:
        for dtype, dt in R.DTYPES.items():
            for bits in BITS:
                x, cost = R._case(frames, hw, ld, dtype, bits)
                ct, gt = torch.from_numpy(cost).to(dev), torch.from_numpy(R._gs(frames)).to(dev)
                for k, keep in enumerate(R._keeps(frames)):
                    xt = torch.from_numpy(x).to(dev).to(dt)
                    kd = torch.from_numpy(keep).to(dev)
                    lat = xt.clone()
                    q = ops.latent_quantise(lat, kd, bits, dequantise_in_place=True)
                    counts = torch.full((frames, 256), -7, dtype=torch.int32, device=dev)
                    fake = ops.latent_fake_quant(xt, kd, bits, counts)
                    leaf = xt.clone().requires_grad_(True)
                    rate = ops.latent_rate(leaf, kd, bits, ct)
                    rate.backward(gt)
                    members = {"codes": q.codes, "step": q.step, "counts": q.counts, "dequantised": lat, "fake": fake, "fake_counts": counts,
                               "rate": rate, "rate_grad": leaf.grad}
                    for name, value in members.items():
                        rec[f"F{frames}_HW{hw}_LD{ld}_{dtype}_b{bits}_k{k}_{name}"] = value.detach().cpu()
    torch.cuda.synchronize()
    return rec


def describe(rec):
    """{member: {dtype, shape, sha256 of the raw bytes}}: what the fixture holds."""
    out = {}
    for name, value in rec.items():
        raw = value.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
        out[name] = {"dtype": str(value.dtype), "shape": list(value.shape), "sha256": hashlib.sha256(raw).hexdigest()}
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE)))
    sys.path.insert(0, os.path.dirname(HERE))
    import test_gpu_rate
    import video_vae_amd
    out = sys.argv[2] if len(sys.argv) > 2 else OUT
    with open(out, "w") as fh:
        json.dump(describe(record(test_gpu_rate)), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(out, "recorded from", os.path.dirname(os.path.abspath(video_vae_amd.__file__)))
