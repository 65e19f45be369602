#!/usr/bin/env python3
"""Generates tests/golden/entropy_context_stream.npz: two frames of 33 x 24 codes at 4 bits laid out 5 tokens wide (a partial last row
and a partial last step), their thresholds and four tables, and the rANS stream the context coder's definition
(video_vae_amd/entropy.py: encode_context_reference) makes of them.

    python tests/golden/make_entropy_context_stream.py [ROOT]

records ``video_vae_amd.entropy`` under ROOT (default: this checkout).  tests/test_entropy_context_host.py calls ``record()`` on the package
it runs in and compares every member with the committed file, so the format cannot drift unnoticed.
"""
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "entropy_context_stream.npz")
FRAMES, HW, GRID_W, LD, BITS = 2, 33, 5, 24, 4


def mixture_codes(frames, hw, grid_w, ld, bits, seed):
    """Seeded int8 codes whose spread changes slowly along the token columns, so that a token's activity says something about the token
    below it; clipped to +-qmax."""
    qmax = (1 << (bits - 1)) - 1
    rng = np.random.default_rng(seed)
    col = np.arange(hw) % grid_w
    sigma = np.exp(1.5 * np.sin(2.0 * np.pi * col / grid_w))[None, :, None] * qmax / 6.0
    return np.clip(np.rint(rng.standard_normal((frames, hw, ld)) * sigma), -qmax, qmax).astype(np.int8)


def record():
    from video_vae_amd.entropy import context_counts, context_thresholds, encode_context_reference, normalise_context_counts, token_energy
    codes = mixture_codes(FRAMES, HW, GRID_W, LD, BITS, 2025)
    thr = np.array(context_thresholds(token_energy(codes), GRID_W), dtype=np.int64)
    freq4 = normalise_context_counts(context_counts(codes, GRID_W, thr), BITS)
    coded = encode_context_reference(codes, freq4, BITS, GRID_W, thr)
    return {"codes": codes, "grid_w": np.int64(GRID_W), "thr": thr, "freq": freq4, "words": coded.words, "n_words": coded.n_words,
            "state": coded.state, "bits": np.int64(BITS)}


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.dirname(OUT))))
    np.savez(OUT, **record())
    print(OUT)
