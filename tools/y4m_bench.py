"""Speed of the YUV4MPEG2 colour conversion on the device, beside the crop + resize it feeds, and of the stage end to end.

A synthetic 4:2:0 clip of --frames frames of 1280 x 720 (seeded random planes, written as a .y4m file into a temporary folder), one GPU, at
most 16 host threads.

  * kernels: HIP events around bursts of --burst launches, the median of --repeats bursts, per launch: ops.yuv_to_rgb_u8 on views of the
    uploaded record buffer (FRAME lines included: with lines of 6 bytes every other frame's planes lie 2 bytes off a dword) and on dense
    copies of the planes (every plane on a dword), ops.rgb_to_yuv of its result, and ops.crop_resize_u8 (the centre square to 256 x 256)
    of the same frames in the same run; microseconds, and the bytes each has to move (read + written, counted from the shapes) per
    second, against the 6.3 TB/s a float4 copy reaches (MI355X_MICROARCH.md).
  * the stage end to end, file -> RGB on the device, frames/s, the median of --calls calls that end in a synchronise:
    host: y4m.Y4MClip[:] (the numpy reference) and the upload of the RGB;  device: data.upload_rgb (the records uploaded as they lie in
    the file, converted there).  Both read the file through the page cache.

    python tools/y4m_bench.py [--frames 64] [--burst 50] [--repeats 20] [--calls 3] [--out FILE]
"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, ".")
import numpy as np
import torch

COPY_TBS = 6.3
H, W, SIZE = 720, 1280, 256
THREADS = 16


def _median(v):
    return sorted(v)[len(v) // 2]


def _bursts(fn, burst, repeats):
    """Seconds per launch: HIP events around ``burst`` launches, (median, best) of ``repeats`` bursts."""
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


def _walls(fn, calls):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return _median(t), min(t)


def kernels(clip, args, log):
    from video_vae_amd import data as D
    from video_vae_amd import ops
    dev = torch.device("cuda", 0)
    n = clip.shape[0]
    ch, cw = clip.header.chroma_shape
    rec, line, stride = clip.records(0, n)
    buf = torch.from_numpy(np.array(rec)).to(dev)
    view = lambda off, r, c: buf.as_strided((n, r, c), (stride, c, 1), off)
    y, u, v = view(line, H, W), view(line + H * W, ch, cw), view(line + H * W + ch * cw, ch, cw)
    rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    planes = tuple(torch.empty(s, dtype=torch.uint8, device=dev) for s in ((n, H, W), (n, ch, cw), (n, ch, cw)))
    sq = torch.empty((n, SIZE, SIZE, 3), dtype=torch.uint8, device=dev)
    ops.yuv_to_rgb_u8(y, u, v, clip.chroma, clip.siting, clip.matrix, clip.full, out=rgb)
    same = np.array_equal(rgb[:2].cpu().numpy(), clip[0:2])
    log(f"  device result equals the host reference on the first 2 frames: {same}")
    if not same:
        raise SystemExit("y4m_bench: the device conversion differs from the reference")
    top, left, s = D.centre_square_crop(H, W)
    moved = n * (H * W * 4 + 2 * ch * cw)                           # planes on one side, RGB on the other
    dense = tuple(p.contiguous() for p in (y, u, v))               # the same planes, each on a dword in every frame
    log(f"  record views: FRAME lines of {line} bytes, stride {stride} = {stride % 4} mod 4: plane bases mod 4 by frame "
        f"{[(line + f * stride) % 4 for f in range(min(n, 4))]} ...")
    rows = (("yuv_to_rgb_u8 4:2:0, records", moved, lambda: ops.yuv_to_rgb_u8(y, u, v, clip.chroma, clip.siting, clip.matrix, clip.full, out=rgb)),
            ("yuv_to_rgb_u8 4:2:0, dense", moved, lambda: ops.yuv_to_rgb_u8(*dense, clip.chroma, clip.siting, clip.matrix, clip.full, out=rgb)),
            ("rgb_to_yuv 4:2:0", moved, lambda: ops.rgb_to_yuv(rgb, "420", clip.matrix, clip.full, out=planes)),
            (f"crop_resize_u8 {s}² -> {SIZE}²", n * (s * s + SIZE * SIZE) * 3, lambda: ops.crop_resize_u8(rgb, top, left, s, s, SIZE, SIZE, out=sq)))
    res = {}
    for name, nbytes, fn in rows:
        med, best = _bursts(fn, args.burst, args.repeats)
        tbs = nbytes / med / 1e12
        res[name] = tbs
        log(f"  {name:30s} median {med * 1e6:9.1f} us  best {best * 1e6:9.1f} us  {n / med:9.0f} frames/s  {nbytes / 1e6:7.1f} MB  "
            f"{tbs:5.2f} TB/s = {100 * tbs / COPY_TBS:5.1f} % of {COPY_TBS} TB/s  ({med * 1e6 / n:5.2f} us per frame)")
    return res


def stage(clip, args, log):
    from video_vae_amd import data as D
    dev = torch.device("cuda", 0)
    n = clip.shape[0]
    host = lambda: torch.from_numpy(clip[:]).to(dev)
    device = lambda: D.upload_rgb(clip, dev)
    same = torch.equal(host(), device())
    log(f"  both stages give the same bytes on the device: {same}")
    out = {}
    for name, fn in (("host reference + RGB upload", host), ("record upload + kernel", device)):
        med, best = _walls(fn, args.calls)
        out[name] = n / med
        log(f"  {name:30s} median {med * 1e3:9.2f} ms  best {best * 1e3:9.2f} ms  {n / med:9.1f} frames/s")
    a, b = out["host reference + RGB upload"], out["record upload + kernel"]
    log(f"  device / host: {b / a:6.1f} x  ({torch.get_num_threads()} host threads)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64, help="frames of the clip")
    ap.add_argument("--burst", type=int, default=50, help="launches between two events")
    ap.add_argument("--repeats", type=int, default=20, help="timed bursts")
    ap.add_argument("--calls", type=int, default=3, help="timed calls of each end-to-end stage")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.set_num_threads(min(THREADS, torch.get_num_threads()))
    if not torch.cuda.is_available():
        raise SystemExit("y4m_bench needs a GPU")
    from video_vae_amd import y4m
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(0)
    planes = (rng.integers(0, 256, size=(args.frames, H, W), dtype=np.uint8),
              rng.integers(0, 256, size=(args.frames, (H + 1) // 2, (W + 1) // 2), dtype=np.uint8),
              rng.integers(0, 256, size=(args.frames, (H + 1) // 2, (W + 1) // 2), dtype=np.uint8))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "clip.y4m")
        y4m.write(path, planes, chroma="420")
        clip = y4m.Y4MClip(path)
        log(f"y4m_bench: {args.frames} frames of {W}x{H}, 4:2:0 ({os.path.getsize(path) / 1e6:.1f} MB on disk, {clip.matrix}, "
            f"{'full' if clip.full else 'limited'} range); bursts of {args.burst} launches, median of {args.repeats}")
        kernels(clip, args, log)
        stage(clip, args, log)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
