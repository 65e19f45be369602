#!/usr/bin/env python3
"""Generates tests/golden/metrics_plans.json: the integers that the planner entry points of the evaluation kernels return (shapes taken,
scratch sizes) over a sweep of shapes, recorded BEFORE the narrow and the strip form of the SSIM moment pass shared one planner.

    python tests/golden/make_metrics_plans.py [ROOT]

records the built library of the ``video_vae_amd`` package under ROOT (default: this checkout).  Host code only: no GPU is needed.
tests/test_metrics_host.py calls ``record()`` on the package it runs in and compares row by row with the committed file: the one
planner must plan what the two planners planned.

A row is (C, H, W, B, T) followed by the values of COLUMNS.  The sweep: C 1 .. 5; W 10, 11, 53, 8192, 8193 and both sides of the narrow
form's limits (W C = 2048 and one more; at C = 3 the 512-thread bound, 680 / 681 / 682); H 10, 11, 16, 37, 256, 720; (B, T) up to
256 x 256 (past 65535 frames).  Every (C, W) meets every H, the (B, T) pairs rotating; the widths at the limits meet every (B, T) at two
heights.  The plane metrics take n = B T frames of H x W and the chroma form C % 3; dtypes are fp32 / fp32 throughout.
"""
import json
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "metrics_plans.json")
HS = (10, 11, 16, 37, 256, 720)
WS = (10, 11, 53, 8192, 8193)
BTS = ((1, 1), (2, 3), (4, 16), (64, 16), (256, 256))
COLUMNS = (["rm_supported", "rm_part_floats", "rm_wide_supported", "rm_wide_part_floats"] + [f"ms_supported_{m}" for m in range(1, 6)] +
           [f"ms_ws_floats_{m}" for m in range(1, 6)] + ["pm_supported", "pm_ws_bytes", "tm_part_floats"])


def limit_widths(c):
    ws = [2048 // c, 2048 // c + 1]
    return ws + [680, 681] if c == 3 else ws


def shapes():
    """(C, H, W, B, T), each once, in a fixed order."""
    seen = []
    for c in range(1, 6):
        for iw, w in enumerate(sorted(set(WS + tuple(limit_widths(c))))):
            for ih, h in enumerate(HS):
                seen.append((c, h, w) + BTS[(c + iw + ih) % len(BTS)])
        for w in limit_widths(c):
            for h in (37, 720):
                seen += [(c, h, w) + bt for bt in BTS]
    return sorted(set(seen))


def record():
    """[[C, H, W, B, T, *COLUMNS], ...] from the importable ``video_vae_amd``."""
    from video_vae_amd._lib import lib
    l = lib()
    rows = []
    for c, h, w, b, t in shapes():
        row = [c, h, w, b, t, l.vvae_recon_metrics_supported(h, w, c, 0, 0), l.vvae_recon_metrics_part_floats(b, t, h, w, c),
               l.vvae_recon_metrics_wide_supported(h, w, c, 0, 0), l.vvae_recon_metrics_wide_part_floats(b, t, h, w, c)]
        row += [l.vvae_ms_ssim_supported(h, w, c, m, 0, 0) for m in range(1, 6)]
        row += [l.vvae_ms_ssim_ws_floats(b, t, h, w, c, m) for m in range(1, 6)]
        row += [l.vvae_plane_metrics_supported(h, w, c % 3), l.vvae_plane_metrics_ws_bytes(b * t, h, w, c % 3),
                l.vvae_temporal_mse_part_floats(b, t, h, w, c)]
        rows.append([int(v) for v in row])
    return rows


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.dirname(OUT))))
    rows = record()
    with open(OUT, "w") as fh:
        fh.write('{"columns": ' + json.dumps(["C", "H", "W", "B", "T"] + COLUMNS) + ',\n"rows": [\n')
        fh.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
        fh.write("\n]}\n")
    print(OUT, len(rows))
