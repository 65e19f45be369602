"""Writes the YUV4MPEG2 fixtures of tests/test_y4m_host.py and tests/test_gpu_y4m.py:

  y4m_small.y4m        5 x 7, 3 frames, C420jpeg, an A tag, an X tag that is not XCOLORRANGE, one FRAME line with a parameter
  y4m_small_mpeg2.y4m  the same planes tagged C420mpeg2, no I tag
  y4m_small_444.y4m    C444, XCOLORRANGE=FULL
  y4m_small_mono.y4m   Cmono, I?
  y4m_small_rgb.npz    the expected RGB of every file for both matrices and both ranges: "<form>_<matrix>_<range>" uint8 (3, 5, 7, 3)

The files are put together byte by byte here and the expected RGB comes from a per-pixel scalar Python loop over plain ints written from
the format's definition: nothing is shared with video_vae_amd/y4m.py, which the tests hold against it.

    python tests/golden/make_y4m_fixture.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
H, W, T = 5, 7, 3
CH, CW = (H + 1) // 2, (W + 1) // 2

# inverse coefficients times 2^14: cy crv cgu cgv cbu
INV = {("bt601", "limited"): (19077, 26149, -6419, -13320, 33050), ("bt601", "full"): (16384, 22970, -5638, -11700, 29032),
       ("bt709", "limited"): (19077, 29372, -3494, -8731, 34610), ("bt709", "full"): (16384, 25802, -3069, -7670, 30402)}


def chroma16(plane, form, y, x):
    """The chroma of luma pixel (y, x) with 4 extra bits; ``plane`` a list of rows of ints."""
    if form == "444":
        return 16 * plane[y][x]
    if form == "mono":
        return 2048
    r0 = y // 2
    r1 = min(r0 + 1, CH - 1) if y % 2 else max(r0 - 1, 0)
    rows = ((r0, 3), (r1, 1))
    c0 = x // 2
    if form == "420":
        cols = ((c0, 3), (min(c0 + 1, CW - 1) if x % 2 else max(c0 - 1, 0), 1))
    else:                                                          # 420mpeg2: co-sited with the even luma columns
        cols = ((c0, 2), (min(c0 + 1, CW - 1), 2)) if x % 2 else ((c0, 4), (min(c0 + 1, CW - 1), 0))
    return sum(wr * wc * plane[r][c] for r, wr in rows for c, wc in cols)


def clip(v):
    return 0 if v < 0 else 255 if v > 255 else v


def to_rgb(yp, up, vp, form, matrix, rng):
    cy, crv, cgu, cgv, cbu = INV[(matrix, rng)]
    off = 16 if rng == "limited" else 0
    out = np.zeros((T, H, W, 3), dtype=np.uint8)
    for t in range(T):
        yl = [[int(a) for a in row] for row in yp[t]]
        ul = None if up is None else [[int(a) for a in row] for row in up[t]]
        vl = None if vp is None else [[int(a) for a in row] for row in vp[t]]
        for y in range(H):
            for x in range(W):
                u = chroma16(ul, form, y, x) - 2048
                v = chroma16(vl, form, y, x) - 2048
                l = 16 * cy * (yl[y][x] - off)
                out[t, y, x] = (clip((l + crv * v + 2 ** 17) >> 18), clip((l + cgu * u + cgv * v + 2 ** 17) >> 18),
                                clip((l + cbu * u + 2 ** 17) >> 18))
    return out


def main():
    rng = np.random.default_rng(20)
    yp = rng.integers(0, 256, size=(T, H, W), dtype=np.uint8)
    u2, v2 = (rng.integers(0, 256, size=(T, CH, CW), dtype=np.uint8) for _ in range(2))
    u4, v4 = (rng.integers(0, 256, size=(T, H, W), dtype=np.uint8) for _ in range(2))
    files = {
        "420": ("y4m_small.y4m", b"YUV4MPEG2 W7 H5 F30000:1001 Ip A1:1 C420jpeg XYSCSS=420JPEG\n", u2, v2),
        "420mpeg2": ("y4m_small_mpeg2.y4m", b"YUV4MPEG2 H5 W7 C420mpeg2 F25:1\n", u2, v2),
        "444": ("y4m_small_444.y4m", b"YUV4MPEG2 W7 H5 F24:1 Ip C444 XCOLORRANGE=FULL\n", u4, v4),
        "mono": ("y4m_small_mono.y4m", b"YUV4MPEG2 W7 H5 F24:1 I? Cmono\n", None, None),
    }
    expected = {}
    for form, (name, head, up, vp) in files.items():
        with open(os.path.join(HERE, name), "wb") as fh:
            fh.write(head)
            for t in range(T):
                fh.write(b"FRAME Ip\n" if (form == "420" and t == 1) else b"FRAME\n")
                fh.write(yp[t].tobytes())
                if up is not None:
                    fh.write(up[t].tobytes())
                    fh.write(vp[t].tobytes())
        for matrix in ("bt601", "bt709"):
            for r in ("limited", "full"):
                expected[f"{form}_{matrix}_{r}"] = to_rgb(yp, up, vp, form, matrix, r)
    np.savez(os.path.join(HERE, "y4m_small_rgb.npz"), **expected)
    print({k: v.shape for k, v in expected.items()})


if __name__ == "__main__":
    main()
