#!/usr/bin/env python3
"""Generates tests/golden/heads_parent_bits.json: what ops.encoder_head, ops.encoder_head_rl and ops.encoder_head_eval computed BEFORE the
three head kernels of csrc/encoder_head.hip shared one prologue, one phase A and one log-variance helper, the five launch entries became
three with an ``rl`` flag and the two autograd nodes one forward and one backward helper, bit for bit.

    python tests/golden/make_heads_parent_bits.py [ROOT]            (needs the GPU)

records the built ``video_vae_amd`` package under ROOT (default: this checkout).  tests/test_gpu_heads_exact.py calls ``record()`` on the
package it runs in and compares every member.  Operands come from that file's builders (``g_case``, ``e_case`` + ``eval_inputs``), which are
seeded on the CPU, and go through its runners (``run_head``, ``run_eval``), so they are the same everywhere; the fixture holds outputs only,
each as dtype, shape and the SHA-256 of its raw bytes.  It is written with sorted keys, so a second run reproduces it byte for byte.

Members (B = 2, T = 3 as the builders have it; <geo> = HW<hw>_LD<ld> over GEOMETRIES; <flavour> = model, rl):
  <flavour>_<geo>_all_<name>        Family G with all four upstream gradients present.  <name>: every forward output (lv, comp, sel, kl; rl also
                                    mean2, mask2), every gradient (dmean, dv, dw1, db1, dw2, db2, dfill) and the per-frame partial rows the
                                    backward kernel wrote, part1 (dW1), part2 (dW2), part3 (d fill), partb1, partb2 (db1, db2), as handed to
                                    ops.fold_partials in that order
  <flavour>_HW16_LD96_<combo>_...   the same members for every entry of COMBOS: each optional operand of the backward absent in turn, gkl
                                    with strides (T, 1), one mask row for all samples
  eval_HW16_LD96_<flavour>_<form>_{lv,comp,sel,prob}     every EVAL_FORMS entry on the Family E model case (None outputs are left out)

A mismatch is a defect of the change, never a reason to record again: find the expression whose form moved and restore it.
"""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "heads_parent_bits.json")
# one wavefront with 4 active threads; TY = HW; 2.5 trips with idle lanes; production, one row in the last trip
GEOMETRIES = [(4, 8), (16, 96), (100, 200), (256, 96)]
DRAWS = {("rl", 4, 8): 1}      # g_case refuses the first draw of this geometry (a uniform within 0.05 of a frame's probability): the second
PARTS = ("part1", "part2", "part3", "partb1", "partb2")


def head_with_partial_rows(H, k, dev, cfg):
    """H.run_head, and the five partial buffers its backward handed to ops.fold_partials (dW1, dW2, d fill, db1, db2 rows, one per frame)."""
    from video_vae_amd import ops
    rows, fold = [], ops.fold_partials

    def spy(part, p0, p1, n0):
        rows.append(part.detach().clone())
        return fold(part, p0, p1, n0)

    ops.fold_partials = spy
    try:
        res = H.run_head(k, dev, cfg)
    finally:
        ops.fold_partials = fold
    assert len(rows) == len(PARTS), (len(rows), "the backward no longer folds five partial buffers")
    res.update({name: r.cpu() for name, r in zip(PARTS, rows)})
    return res


def record(H, dev="cuda"):
    """{member: tensor on the CPU} from the importable ``video_vae_amd`` on ``dev``.  ``H``: the module tests/test_gpu_heads_exact.py."""
    rec = {}

    def put(prefix, res):
        for name, value in res.items():
            if value is not None:
                rec[f"{prefix}_{name}"] = value.detach().cpu()

    for flavour in ("model", "rl"):
        for hw, ld in GEOMETRIES:
            put(f"{flavour}_HW{hw}_LD{ld}_all", head_with_partial_rows(H, H.g_case(flavour, hw, ld, DRAWS.get((flavour, hw, ld), 0)), dev, H.CFG_G))
        for cfg in H.COMBOS:
            put(f"{flavour}_HW16_LD96_{H._cfg_id(cfg)}", head_with_partial_rows(H, H.g_case(flavour, 16, 96), dev, cfg))
    k = H.e_case("model", 16, 96)
    for flavour, form in H.EVAL_FORMS:
        put(f"eval_HW16_LD96_{flavour}_{form}", H.run_eval(k, dev, flavour, form))
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
    import test_gpu_heads_exact
    import video_vae_amd
    with open(OUT, "w") as fh:
        json.dump(describe(record(test_gpu_heads_exact)), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(OUT, "recorded from", os.path.dirname(os.path.abspath(video_vae_amd.__file__)))
