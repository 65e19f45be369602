#!/usr/bin/env python3
"""Generates tests/golden/entropy_parent_streams.npz: the streams that the definition (video_vae_amd/entropy.py) made of a handful of
small frames BEFORE the static and the context coder were folded into one loop each, recorded from that earlier tree as plain data.

    python tests/golden/make_entropy_parent_streams.py [ROOT]

records ``video_vae_amd.entropy`` under ROOT (default: this checkout).  tests/test_entropy_host.py calls ``record()`` on the package it
runs in and compares every member with the committed file: the one loop must make what the two loops made, word for word.  The file is
written with fixed member dates, so a second run reproduces it byte for byte.

Members ``<case>_<name>``.  Static cases (``s*``): codes, freq, words, n_words, state, bits.  Context cases (``c*``): the same with freq
(4, 2 qmax + 1), and grid_w, thr.
"""
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "entropy_parent_streams.npz")
sys.path.insert(0, HERE)
from make_entropy_context_stream import mixture_codes  # noqa: E402
from make_entropy_stream import laplacian_codes  # noqa: E402

# (frames, hw, ld, bits): fewer symbols than lanes; a partial last step; 7 steps, the last one partial
STATIC = [(2, 1, 8, 2), (1, 1, 96, 8), (2, 17, 24, 6)]
# (frames, hw, grid_w, ld, bits): a partial last row and step; the bound of the support condition, energies by bytes; 2 and 8 bits
CONTEXT = [(2, 15, 5, 24, 6), (2, 30, 10, 7, 4), (2, 64, 8, 24, 2), (2, 64, 8, 24, 8)]
EQUAL_THR = (40, 40)                                       # on one frame of 64 x 24 at 6 bits, 8 wide: context 2 is empty


def record():
    from video_vae_amd.entropy import (context_counts, context_thresholds, encode_context_reference, encode_reference,
                                       normalise_context_counts, normalise_counts, token_energy)
    from video_vae_amd.quant import code_counts, qmax_of
    rec = {}

    def static(case, codes, bits):
        freq = normalise_counts(code_counts(codes), bits)
        coded = encode_reference(codes, freq, bits)
        rec.update({f"{case}_codes": codes, f"{case}_freq": freq, f"{case}_words": coded.words, f"{case}_n_words": coded.n_words,
                    f"{case}_state": coded.state, f"{case}_bits": np.int64(bits)})

    def context(case, codes, grid_w, bits, thr=None):
        if thr is None:
            thr = context_thresholds(token_energy(codes), grid_w)
        thr = np.array(thr, dtype=np.int64)
        counts = context_counts(codes, grid_w, thr)
        freq4 = normalise_context_counts(counts, bits)
        coded = encode_context_reference(codes, freq4, bits, grid_w, thr)
        rec.update({f"{case}_codes": codes, f"{case}_freq": freq4, f"{case}_words": coded.words, f"{case}_n_words": coded.n_words,
                    f"{case}_state": coded.state, f"{case}_bits": np.int64(bits), f"{case}_grid_w": np.int64(grid_w), f"{case}_thr": thr})
        return counts

    for k, (frames, hw, ld, bits) in enumerate(STATIC):
        static(f"s{k}", laplacian_codes((frames, hw, ld), bits, qmax_of(bits) / 6.0 + 0.4, 3000 + k), bits)
    static(f"s{len(STATIC)}", np.zeros((1, 4, 24), dtype=np.int8), 6)                           # one symbol owns the table: freq << 20 is 2^32
    for k, (frames, hw, grid_w, ld, bits) in enumerate(CONTEXT):
        context(f"c{k}", mixture_codes(frames, hw, grid_w, ld, bits, 4000 + k), grid_w, bits)
    counts = context(f"c{len(CONTEXT)}", mixture_codes(1, 64, 8, 24, 6, 4100), 8, 6, EQUAL_THR)
    assert counts[:, 2].sum() == 0 and counts[:, 1].sum() > 0 and counts[:, 3].sum() > 0      # an empty context between two used ones
    return rec


def write(path, rec):
    """np.savez_compressed with every member dated 1980-01-01, so that the bytes depend on the arrays alone."""
    with zipfile.ZipFile(path, "w") as zf:
        for name, value in rec.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with zf.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.asanyarray(value), allow_pickle=False)


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE)))
    write(OUT, record())
    print(OUT)
