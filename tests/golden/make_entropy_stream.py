#!/usr/bin/env python3
"""Generates tests/golden/entropy_stream.npz: two frames of 4 x 24 codes at 4 bits, their table (pooled over more frames than are coded),
and the rANS stream the definition (video_vae_amd/entropy.py) makes of them.

    python tests/golden/make_entropy_stream.py [ROOT]

records ``video_vae_amd.entropy`` under ROOT (default: this checkout).  tests/test_entropy_host.py calls ``record()`` on the package it
runs in and compares every member with the committed file, so the stream format cannot drift unnoticed.
"""
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "entropy_stream.npz")
FRAMES, HW, LD, BITS, POOL = 2, 4, 24, 4, 64


def laplacian_codes(shape, bits, scale, seed):
    """Seeded int8 codes with a Laplacian histogram, clipped to +-qmax."""
    qmax = (1 << (bits - 1)) - 1
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.laplace(size=shape) * scale), -qmax, qmax).astype(np.int8)


def record():
    """The table is pooled over POOL frames, the first FRAMES of which are coded: among 192 codes no symbol is rare enough to push a
    lane (one or two symbols each) over its renormalisation bound, so rare pairs are planted on a few lanes that hold two symbols."""
    from video_vae_amd.entropy import encode_reference, normalise_counts
    from video_vae_amd.quant import code_counts
    pool = laplacian_codes((POOL, HW, LD), BITS, 0.8, 2024)
    flat = pool.reshape(POOL, HW * LD)
    for f in range(FRAMES):
        for k, lane in enumerate(range(f, 32, 3)):         # symbols lane and lane + 64 share a lane
            flat[f, lane] = (7, -7, 6, -6)[k % 4]
            flat[f, lane + 64] = (-6, 7, -7, 6)[k % 4]
    codes = pool[:FRAMES].copy()
    freq = normalise_counts(code_counts(pool), BITS)
    coded = encode_reference(codes, freq, BITS)
    return {"codes": codes, "freq": freq, "words": coded.words, "n_words": coded.n_words, "state": coded.state, "bits": np.int64(BITS)}


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.dirname(OUT))))
    np.savez(OUT, **record())
    print(OUT)
