"""Speed of multi-scale SSIM (vvae_ms_ssim_fwd: per level a per-channel moment pass and a 2 x 2 pool, then one fold) beside the
single-scale metrics of the same run (vvae_recon_metrics_fwd / vvae_recon_metrics_wide_fwd), through metrics.ms_ssim and
metrics.frame_metrics / frame_metrics_wide as eval calls them (their output and workspace allocations included).

  shape 1: 4 x 16 x 256 x 256 x 3, an fp32 clip against a bf16 reconstruction (the plain eval batch)
  shape 2: one 16-frame 1280 x 720 window, fp32 against fp32 (what the tiled and windowed modes hold; levels 0 and 1 run in column strips)

HIP events around --burst back-to-back calls, median of --repeats bursts, per call.  The figure to record is the ratio to frame_metrics in
the same run: by position count five scales are 1.33 x the single-scale pass, and the pools read level 0 a second time.

    python tools/ms_ssim_bench.py [--scales 5] [--repeats 20] [--burst 50] [--out profiles/r21_ms_ssim_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, ".")
import torch


def _median(v):
    return sorted(v)[len(v) // 2]


def _time(fn, args):
    for _ in range(args.burst):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.burst):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / args.burst)
    return _median(us), min(us)


def stage(args, log, dev, name, shape, dy, single):
    from video_vae_amd.metrics import MS_SSIM_WEIGHTS, ms_ssim
    g = torch.Generator().manual_seed(0)
    x = torch.rand(shape, generator=g).to(dev)
    y = (x + 0.1 * torch.randn(shape, generator=g).to(dev)).to(dy)
    mask = torch.ones(shape[:2], device=dev)
    w = MS_SSIM_WEIGHTS[:args.scales]
    one = _time(lambda: single(x, y, mask), args)
    ms = _time(lambda: ms_ssim(x, y, mask, weights=w), args)
    nbytes = x.numel() * (x.element_size() + y.element_size())
    log(f"{name}: {'x'.join(map(str, shape))} fp32 / {str(dy)[6:]} ({nbytes / 1e6:.0f} MB a pair): {single.__name__} median {one[0]:8.2f} us "
        f"best {one[1]:8.2f} us ({nbytes / one[0] / 1e6:.2f} TB/s), ms_ssim at {args.scales} scales median {ms[0]:8.2f} us best {ms[1]:8.2f} us "
        f"({2 * args.scales} launches) = {ms[0] / one[0]:.3f} x {single.__name__} ({args.burst} per burst, {args.repeats} bursts)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ms_ssim_bench needs a GPU")
    from video_vae_amd.metrics import frame_metrics, frame_metrics_wide
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    log(f"ms_ssim_bench: multi-scale SSIM beside the single-scale metrics (csrc/metrics.hip), {torch.cuda.get_device_name(0)}")
    stage(args, log, dev, "eval batch", (4, 16, 256, 256, 3), torch.bfloat16, frame_metrics)
    stage(args, log, dev, "720p window", (1, 16, 720, 1280, 3), torch.float32, frame_metrics_wide)
    if args.out:
        if os.path.dirname(args.out):
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
