"""Writes tests/golden/ssim_grad_small.npz: inputs and the expected per-frame SSIM and its gradient with respect to the reconstruction, in
float64, for tests/test_ssim_loss_host.py.

Shares nothing with video_vae_amd/metrics.py: its own taps, its own moments (scalar loops over the 11 x 11 window, not separable) and its
own closed form, in scatter form: every valid position p hands w(p - q) (dS/dmy + 2 y(q) dS/dE[yy] + x(q) dS/dE[xy]) to each of the 121
elements q under its window.

    python tests/golden/make_ssim_grad_fixture.py
"""
import math
import os

import numpy as np

K1, K2 = 0.01 ** 2, 0.03 ** 2


def window():
    t = [math.exp(-((k - 5) ** 2) / (2 * 1.5 ** 2)) for k in range(11)]
    s = sum(t)
    t = [v / s for v in t]
    return [[t[i] * t[j] for j in range(11)] for i in range(11)]


def frame(x, y, gout, clamp):
    """x, y (H, W, C) float64 -> (ssim, dy (H, W, C)) of one frame with upstream gradient gout."""
    h, w, c = x.shape
    yraw = y
    if clamp:
        x, y = np.minimum(np.maximum(x, 0.0), 1.0), np.minimum(np.maximum(y, 0.0), 1.0)
    w2 = window()
    n = c * (h - 10) * (w - 10)
    total = 0.0
    dy = np.zeros((h, w, c))
    for ch in range(c):
        for pi in range(5, h - 5):
            for pj in range(5, w - 5):
                ex = ey = exx = eyy = exy = 0.0
                for di in range(11):
                    for dj in range(11):
                        wt = w2[di][dj]
                        xv, yv = x[pi - 5 + di, pj - 5 + dj, ch], y[pi - 5 + di, pj - 5 + dj, ch]
                        ex += wt * xv
                        ey += wt * yv
                        exx += wt * xv * xv
                        eyy += wt * yv * yv
                        exy += wt * xv * yv
                varx, vary, cov = exx - ex * ex, eyy - ey * ey, exy - ex * ey
                num1, num2 = 2 * ex * ey + K1, 2 * cov + K2
                den1, den2 = ex * ex + ey * ey + K1, varx + vary + K2
                s = num1 * num2 / (den1 * den2)
                total += s
                # S as a function of (ey, eyy, exy): cov = exy - ex ey, vary = eyy - ey^2
                d_ey = (2 * ex * num2 - 2 * ex * num1) / (den1 * den2) - s * (2 * ey / den1) + s * (2 * ey / den2)
                d_eyy = -s / den2
                d_exy = 2 * num1 / (den1 * den2)
                for di in range(11):
                    for dj in range(11):
                        qi, qj = pi - 5 + di, pj - 5 + dj
                        dy[qi, qj, ch] += w2[di][dj] * (d_ey + 2 * y[qi, qj, ch] * d_eyy + x[qi, qj, ch] * d_exy)
    dy *= gout / n
    if clamp:
        dy[(yraw < 0.0) | (yraw > 1.0)] = 0.0
    return total / n, dy


def case(x, y, mask, gout, clamp, video_div):
    b, t = y.shape[:2]
    ssim = np.zeros((b, t))
    dy = np.zeros(y.shape)
    for i in range(b):
        for j in range(t):
            if mask[i, j] != 0:
                ssim[i, j], dy[i, j] = frame(x[i // video_div, j], y[i, j], gout[i, j], clamp)
    return ssim, dy


def main():
    rng = np.random.default_rng(20240607)
    cases = []
    # 11 x 11 x 1: a single valid position
    x = rng.random((1, 2, 11, 11, 1))
    y = x + 0.1 * rng.standard_normal(x.shape)
    cases.append((x, y, np.ones((1, 2)), np.array([[1.0, -0.75]]), False, 1))
    # 13 x 27 x 3, pair doubling, one masked frame
    x = rng.random((1, 2, 13, 27, 3))
    y = np.repeat(x, 2, axis=0) + 0.2 * rng.standard_normal((2, 2, 13, 27, 3))
    cases.append((x, y, np.array([[1.0, 1.0], [0.0, 1.0]]), np.array([[0.5, 1.0], [2.0, -1.5]]), False, 2))
    # clamp: values below 0, above 1 and exactly 0 and 1
    x = rng.random((1, 1, 12, 13, 2)) * 1.4 - 0.2
    y = x + 0.3 * rng.standard_normal(x.shape)
    flat = y.reshape(-1)
    flat[0::7] = 0.0
    flat[1::7] = 1.0
    flat[2::7] = -0.25
    flat[3::7] = 1.5
    cases.append((x, y, np.ones((1, 1)), np.array([[1.25]]), True, 1))
    out = {"cases": np.array(len(cases))}
    for k, (x, y, mask, gout, clamp, div) in enumerate(cases):
        x, y = x.astype(np.float32), y.astype(np.float32)         # the operands are stored as fp32 values; everything else is float64
        ssim, dy = case(x.astype(np.float64), y.astype(np.float64), mask, gout, clamp, div)
        out.update({f"x{k}": x, f"y{k}": y, f"mask{k}": mask, f"gout{k}": gout, f"clamp{k}": np.array(int(clamp)),
                    f"video_div{k}": np.array(div), f"ssim{k}": ssim, f"drecon{k}": dy})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ssim_grad_small.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
