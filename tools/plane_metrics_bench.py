"""Speed of the plane-wise Y'CbCr metrics (csrc/plane_metrics.hip) beside the route that gave the same numbers before it existed.

Two synthetic 4:2:0 clips of --frames frames of 1280 x 720 (seeded random planes; the second a perturbed copy of the first), written as
.y4m files into a temporary folder, one GPU.  HIP events around bursts of --burst calls, the median of --repeats bursts, per call:

  * ops.plane_metrics_u8 on views of the two uploaded record buffers (FRAME lines of 6 bytes in one file and of 9 in the other: with
    them every other frame's planes lie 2 bytes off a dword in the first, and the second's planes lie 1 .. 3 bytes off in every frame);
  * ops.plane_metrics_u8 on dense copies of the planes (every plane on a dword);
  * the widened route: both Y planes to fp32 / 255 by torch, ops.recon_metrics at C = 1 (its mse times 255^2 H W is the squared error,
    in fp32, not exact), and torch for the chroma squared errors ((a - b)^2 summed in int64 per frame and plane);
  * the widened route's metrics kernel alone, on operands widened beforehand.

Microseconds, and the bytes of the planes (both operands, read once: what the new entry has to move) per second for each.

    python tools/plane_metrics_bench.py [--frames 64] [--burst 20] [--repeats 15] [--out FILE]
"""
import argparse
import os
import sys
import tempfile

sys.path.insert(0, ".")
import numpy as np
import torch

H, W = 720, 1280
CH, CW = (H + 1) // 2, (W + 1) // 2


def _median(v):
    return sorted(v)[len(v) // 2]


def _bursts(fn, burst, repeats):
    """Seconds per call: HIP events around ``burst`` calls, (median, best) of ``repeats`` bursts."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(burst):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / burst)
    return _median(ms) * 1e-3, min(ms) * 1e-3


def _write(path, planes, line):
    y, u, v = planes
    with open(path, "wb") as fh:
        fh.write(f"YUV4MPEG2 W{W} H{H} F30:1 Ip C420jpeg XCOLORRANGE=LIMITED\n".encode())
        for f in range(y.shape[0]):
            fh.write(line + y[f].tobytes() + u[f].tobytes() + v[f].tobytes())


def _views(clip, dev):
    n = clip.shape[0]
    rec, line, stride = clip.records(0, n)
    buf = torch.from_numpy(np.array(rec)).to(dev)
    view = lambda off, r, c: buf.as_strided((n, r, c), (stride, c, 1), off)
    return (view(line, H, W), view(line + H * W, CH, CW), view(line + H * W + CH * CW, CH, CW)), line, stride


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64, help="frames of the clips")
    ap.add_argument("--burst", type=int, default=20, help="calls between two events")
    ap.add_argument("--repeats", type=int, default=15, help="timed bursts")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plane_metrics_bench needs a GPU")
    from video_vae_amd import ops, y4m
    from video_vae_amd import plane_metrics as PM
    dev = torch.device("cuda", 0)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    n = args.frames
    rng = np.random.default_rng(0)
    ref = tuple(rng.integers(0, 256, size=(n, r, c), dtype=np.uint8) for r, c in ((H, W), (CH, CW), (CH, CW)))
    test = tuple(np.clip(p.astype(np.int16) + rng.integers(-6, 7, size=p.shape, dtype=np.int16), 0, 255).astype(np.uint8) for p in ref)
    with tempfile.TemporaryDirectory() as tmp:
        _write(os.path.join(tmp, "ref.y4m"), ref, b"FRAME\n")
        _write(os.path.join(tmp, "test.y4m"), test, b"FRAME Ip\n")
        ca, cb = y4m.Y4MClip(os.path.join(tmp, "ref.y4m")), y4m.Y4MClip(os.path.join(tmp, "test.y4m"))
        (va, la, sa), (vb, lb, sb) = _views(ca, dev), _views(cb, dev)
    log(f"plane_metrics_bench: 2 x {n} frames of {W}x{H}, 4:2:0; bursts of {args.burst} calls, median of {args.repeats}")
    log(f"  record views: Y bases mod 4 by frame, reference {[(la + f * sa) % 4 for f in range(4)]} ..., test "
        f"{[(lb + f * sb) % 4 for f in range(4)]} ...")
    da, db = tuple(p.contiguous() for p in va), tuple(p.contiguous() for p in vb)
    moved = 2 * n * (H * W + 2 * CH * CW)

    def widen():
        return da[0].float().div_(255.0)[None, ..., None], db[0].float().div_(255.0)[None, ..., None]
    ones = torch.ones((1, n), dtype=torch.float32, device=dev)

    def chroma_torch():
        return torch.stack([((da[p].to(torch.int32) - db[p].to(torch.int32)) ** 2).sum(dim=(1, 2), dtype=torch.int64) for p in (1, 2)], dim=1)

    def widened():
        x, y = widen()
        mse, _, ssim = ops.recon_metrics(x, y, ones, clamp=False)
        return mse, ssim, chroma_torch()
    wx, wy = widen()

    # the routes agree before they are timed
    want = PM.plane_metrics_reference(tuple(p[:2] for p in ref), tuple(p[:2] for p in test), "420")
    sse_v, ssim_v = ops.plane_metrics_u8(va, vb, "420")
    sse_d, ssim_d = ops.plane_metrics_u8(da, db, "420")
    mse_w, ssim_w, csse_w = widened()
    exact = np.array_equal(sse_v[:2].cpu().numpy(), want.sse) and torch.equal(sse_v, sse_d) and torch.equal(ssim_v, ssim_d)
    log(f"  the new entry equals the host reference on the first 2 frames (sse exact: {exact}; max |ssim_y - ref| = "
        f"{np.abs(ssim_v[:2].cpu().numpy().astype(np.float64) - want.ssim_y).max():.2e}); record views and dense planes bitwise equal")
    sse_w = mse_w[0].double() * 255.0 ** 2 * H * W
    log(f"  the widened route: chroma sse equal: {torch.equal(csse_w, sse_v[:, 1:])}; its Y sse from the fp32 mse is off by up to "
        f"{(sse_w - sse_v[:, 0].double()).abs().max().item():.0f} of {sse_v[:, 0].max().item()}; max |ssim - ssim_y| = "
        f"{(ssim_w[0].double() - ssim_v.double()).abs().max().item():.2e}")
    if not exact:
        raise SystemExit("plane_metrics_bench: the kernel differs from the reference")
    rows = (("plane_metrics_u8, record views", lambda: ops.plane_metrics_u8(va, vb, "420")),
            ("plane_metrics_u8, dense planes", lambda: ops.plane_metrics_u8(da, db, "420")),
            ("widened: fp32 / 255, recon_metrics C=1, torch chroma", widened),
            ("  of which recon_metrics C=1 alone (operands widened before)", lambda: ops.recon_metrics(wx, wy, ones, clamp=False)))
    res = {}
    for name, fn in rows:
        med, best = _bursts(fn, args.burst, args.repeats)
        res[name] = med
        log(f"  {name:62s} median {med * 1e6:9.1f} us  best {best * 1e6:9.1f} us  {n / med:9.0f} frames/s  "
            f"{moved / med / 1e12:6.3f} TB/s of the planes' {moved / 1e6:.1f} MB")
    new, old = res[rows[1][0]], res[rows[2][0]]
    log(f"  widened route / new entry (dense planes): {old / new:5.2f} x;  / new entry (record views): {old / res[rows[0][0]]:5.2f} x")
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
