#!/usr/bin/env python3
"""Generates tests/golden/entropy_temporal_stream.npz: two small clips of quantised codes, their chain flags, thresholds and nine tables,
and the rANS streams the temporal coder's definition (video_vae_amd/entropy.py: encode_temporal_reference) makes of them.

  * ``a_``: eight frames of 16 x 24 codes at 4 bits in chains of 1, 2 and 5 frames;
  * ``z_``: three frames of 5 x 7 codes (35 symbols: one step with idle lanes) at 6 bits in one chain whose first frame is all zeros, so
    row 0 is a one-symbol table (``freq << 20`` is 2^32) and the second frame sees one class only.

    python tests/golden/make_entropy_temporal_stream.py [ROOT]

records ``video_vae_amd.entropy`` under ROOT (default: this checkout).  tests/test_entropy_temporal_host.py calls ``record()`` on the package
it runs in and compares every member with the committed file, so the format cannot drift unnoticed; tests/test_gpu_entropy_temporal.py
holds the kernels against the same file.
"""
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "entropy_temporal_stream.npz")
CHAINS = (1, 2, 5)                                         # the chain lengths of the general case


def ar1_latents(frames, hw, ld, seed, rho=0.9, starts=(0,)):
    """Seeded float32 latents (frames, hw, ld): a scale mixture (one scale per channel, one per token) whose time axis is AR(1) with
    correlation ``rho``; a frame in ``starts`` is drawn afresh (a new sequence)."""
    rng = np.random.default_rng(seed)
    scale = np.exp(rng.standard_normal((1, ld))) * np.exp(0.5 * rng.standard_normal((hw, 1)))
    x = np.zeros((frames, hw, ld))
    for t in range(frames):
        noise = rng.standard_normal((hw, ld))
        x[t] = noise if t in starts else rho * x[t - 1] + np.sqrt(1.0 - rho * rho) * noise
    return (x * scale).astype(np.float32)


def chain_of(lengths):
    """The chain flags uint8 of consecutive chains of these lengths."""
    return np.concatenate([[0] + [1] * (n - 1) for n in lengths]).astype(np.uint8)


def ar1_codes(lengths, hw, ld, bits, seed, rho=0.9):
    """(codes int8 (sum of lengths, hw, ld), chain uint8): every chain an AR(1) sequence of its own, quantised by quant.quantise_reference."""
    from video_vae_amd.quant import quantise_reference
    chain = chain_of(lengths)
    x = ar1_latents(chain.shape[0], hw, ld, seed, rho, starts=tuple(np.nonzero(chain == 0)[0].tolist()))
    return quantise_reference(x, bits)[0], chain


def zero_start_codes(hw, ld, bits, seed):
    """(codes, chain) of one chain of three frames whose first frame is all zeros."""
    codes, _ = ar1_codes((3,), hw, ld, bits, seed)
    codes[0] = 0
    return codes, chain_of((3,))


def model_of(codes, chain, bits):
    """(thr, freq9) of a clip, as ``infer encode --entropy-temporal`` forms them."""
    from video_vae_amd.entropy import normalise_temporal_counts, temporal_counts, temporal_thresholds
    thr = temporal_thresholds(codes, chain)
    return thr, normalise_temporal_counts(temporal_counts(codes, chain, thr), bits)


def record():
    from video_vae_amd.entropy import encode_temporal_reference
    out = {}
    for tag, (codes, chain), bits in (("a", ar1_codes(CHAINS, 16, 24, 4, 2026), 4), ("z", zero_start_codes(5, 7, 6, 2027), 6)):
        thr, freq9 = model_of(codes, chain, bits)
        coded = encode_temporal_reference(codes, freq9, bits, chain, thr)
        out.update({f"{tag}_codes": codes, f"{tag}_chain": chain, f"{tag}_thr": thr, f"{tag}_freq": freq9, f"{tag}_words": coded.words,
                    f"{tag}_n_words": coded.n_words, f"{tag}_state": coded.state, f"{tag}_bits": np.int64(bits)})
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.dirname(OUT))))
    np.savez(OUT, **record())
    print(OUT)
