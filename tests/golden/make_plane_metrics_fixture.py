"""Writes the fixtures of tests/test_plane_metrics_host.py and tests/test_gpu_plane_metrics.py:

  plane_metrics_ref.y4m    13 x 17, 3 frames, C420jpeg, FRAME lines of 6 bytes ("FRAME\\n"): a pattern
  plane_metrics_test.y4m   the same size and form, FRAME lines of 9 bytes ("FRAME Ip\\n"): a perturbed copy of the pattern
  plane_metrics_small.npz  "sse" int64 (3, 3): the sums of squared differences of the Y, U and V planes of every frame;
                           "ssim_y" float64 (3,): the SSIM of the Y planes / 255 (11-tap Gaussian, sigma 1.5, valid positions only,
                           C1 = 0.01^2, C2 = 0.03^2)

The files are put together byte by byte here and the expectations come from scalar Python loops over plain ints and floats (math.fsum for
the sums) written from the definition: nothing is shared with video_vae_amd/plane_metrics.py, which the tests hold against them.

    python tests/golden/make_plane_metrics_fixture.py
"""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
H, W, T = 13, 17, 3
CH, CW = (H + 1) // 2, (W + 1) // 2


def sse(a, b):
    return sum((int(p) - int(q)) ** 2 for ra, rb in zip(a, b) for p, q in zip(ra, rb))


def ssim(a, b):
    """One plane pair, rows of ints 0 .. 255."""
    g = [math.exp(-((k - 5) ** 2) / (2 * 1.5 * 1.5)) for k in range(11)]
    tot = math.fsum(g)
    g = [v / tot for v in g]
    x = [[p / 255.0 for p in row] for row in a]
    y = [[p / 255.0 for p in row] for row in b]
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    vals = []
    for r in range(5, H - 5):
        for c in range(5, W - 5):
            win = [(g[i] * g[j], x[r - 5 + i][c - 5 + j], y[r - 5 + i][c - 5 + j]) for i in range(11) for j in range(11)]
            mx = math.fsum(w * p for w, p, _ in win)
            my = math.fsum(w * q for w, _, q in win)
            vx = math.fsum(w * p * p for w, p, _ in win) - mx * mx
            vy = math.fsum(w * q * q for w, _, q in win) - my * my
            vxy = math.fsum(w * p * q for w, p, q in win) - mx * my
            vals.append((2 * mx * my + c1) * (2 * vxy + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2)))
    return math.fsum(vals) / len(vals)


def main():
    rng = np.random.default_rng(23)
    planes = {}
    for name, (r, c) in (("y", (H, W)), ("u", (CH, CW)), ("v", (CH, CW))):
        yy, xx = np.meshgrid(np.arange(r), np.arange(c), indexing="ij")
        base = np.stack([(40 + 9 * yy + 5 * xx + 17 * t + 30 * np.sin(0.9 * xx + t) * np.cos(0.7 * yy)) for t in range(T)])
        ref = np.clip(np.rint(base + rng.integers(-6, 7, size=base.shape)), 0, 255).astype(np.uint8)
        test = np.clip(ref.astype(np.int64) + rng.integers(-9, 10, size=base.shape) * (rng.random(base.shape) < 0.6), 0, 255).astype(np.uint8)
        planes[name] = (ref, test)
    for side, (name, line) in enumerate((("plane_metrics_ref.y4m", b"FRAME\n"), ("plane_metrics_test.y4m", b"FRAME Ip\n"))):
        with open(os.path.join(HERE, name), "wb") as fh:
            fh.write(b"YUV4MPEG2 W17 H13 F25:1 Ip C420jpeg XCOLORRANGE=LIMITED\n")
            for t in range(T):
                fh.write(line)
                for p in ("y", "u", "v"):
                    fh.write(planes[p][side][t].tobytes())
    rows = lambda p: [[int(v) for v in row] for row in p]
    want_sse = np.array([[sse(rows(planes[p][0][t]), rows(planes[p][1][t])) for p in ("y", "u", "v")] for t in range(T)], dtype=np.int64)
    want_ssim = np.array([ssim(rows(planes["y"][0][t]), rows(planes["y"][1][t])) for t in range(T)], dtype=np.float64)
    np.savez(os.path.join(HERE, "plane_metrics_small.npz"), sse=want_sse, ssim_y=want_ssim)
    print(want_sse.tolist(), want_ssim.tolist())


if __name__ == "__main__":
    main()
