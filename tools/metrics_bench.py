"""Speed of the reconstruction-metrics kernel (vvae_recon_metrics_fwd: the per-band pass plus the fold) and what the metrics add to a
replayed inference graph.

  * kernel: the median of per-call HIP-event times after a warm-up, as algorithmic bandwidth = valid frames x H W C x (bytes per x element
    + bytes per y element) over the time, against the 8 TB/s HBM peak and the 6.3 TB/s a float4 copy reaches.  Shapes: the production
    batch (4 x 16 x 256² x 3, fp32 video, bf16 reconstruction: 75 MB, inside the 256 MiB Infinity Cache) and one well past the cache
    (16 x 32 x 256² x 3, both fp32: 805 MB).
  * graphs: the replayed "evaluate" graph (reconstruct + frame_metrics) against the replayed "reconstruct" graph, full depth, B = 4,
    16 x 256² frames, alternated over several rounds (bench.py's protocol per round: warm-up, settle, median of per-replay times).

    python tools/metrics_bench.py [--steps 50] [--rounds 3] [--skip-graphs] [--out FILE]
"""
import argparse
import ctypes
import gc
import statistics
import sys
import time

sys.path.insert(0, ".")
import torch

import video_vae_amd as V
from video_vae_amd import ops
from video_vae_amd._lib import check, lib
from video_vae_amd.infer import GraphedInference, InferenceWeights, model_config

PEAK_TBS, COPY_TBS = 8.0, 6.3


def event_median(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    evs[0].record()
    for i in range(steps):
        fn()
        evs[i + 1].record()
    torch.cuda.synchronize()
    return statistics.median(evs[i].elapsed_time(evs[i + 1]) for i in range(steps))


def kernel_case(b, t, h, w, c, dx, dy, steps, warmup, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand((b, t, h, w, c), generator=g, device=dev).to(dx)
    y = (x.float() + 0.05 * torch.randn((b, t, h, w, c), generator=g, device=dev)).to(dy)
    mask = torch.ones((b, t), device=dev)
    mse, psnr, ssim = (torch.empty((b, t), device=dev) for _ in range(3))
    part = torch.empty(int(lib().vvae_recon_metrics_part_floats(b, t, h, w, c)), device=dev)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = [ctypes.c_void_p(x.data_ptr()), ops.DT[dx], ctypes.c_void_p(y.data_ptr()), ops.DT[dy], ctypes.c_void_p(mask.data_ptr()),
            ctypes.c_void_p(mse.data_ptr()), ctypes.c_void_p(psnr.data_ptr()), ctypes.c_void_p(ssim.data_ptr()),
            ctypes.c_void_p(part.data_ptr()), b, t, h, w, c, 1, s]
    ms = event_median(lambda: check(lib().vvae_recon_metrics_fwd(*args), "vvae_recon_metrics_fwd"), steps, warmup)
    nbytes = b * t * h * w * c * (x.element_size() + y.element_size())
    tbs = nbytes / (ms * 1e-3) / 1e12
    return (f"kernel {b}x{t}x{h}x{w}x{c} {str(dx)[6:]}/{str(dy)[6:]}: {nbytes / 1e6:8.1f} MB  {ms * 1e3:8.1f} us  {tbs:5.2f} TB/s  "
            f"{tbs / PEAK_TBS * 100:5.1f} % of {PEAK_TBS:g} TB/s peak, {tbs / COPY_TBS * 100:5.1f} % of the {COPY_TBS:g} TB/s copy")


def replay_median(gi, x, mask, steps, warmup, settle):
    for _ in range(warmup):
        gi(x, mask)
    torch.cuda.synchronize()
    t_end = time.perf_counter() + settle
    while time.perf_counter() < t_end:
        gi(x, mask)
        torch.cuda.synchronize()
    return event_median(lambda: gi(x, mask), steps, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--settle-seconds", type=float, default=1.0)
    ap.add_argument("--skip-graphs", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"metrics_bench: median of {args.steps} per-call HIP-event times after {args.warmup} warm-up calls"]

    def report(msg):
        print(msg, flush=True)
        lines.append(msg)

    f32, bf = torch.float32, torch.bfloat16
    for case in [(4, 16, 256, 256, 3, f32, bf), (4, 16, 256, 256, 3, f32, f32), (16, 32, 256, 256, 3, f32, f32),
                 (16, 32, 256, 256, 3, f32, bf)]:
        report(kernel_case(*case, args.steps, args.warmup, dev))
        gc.collect()
        torch.cuda.empty_cache()
    if not args.skip_graphs:
        b, t, size = 4, 16, 256
        model = V.VideoVAE(rngs=V.Rngs(2), **model_config(size, False)).to(dev)
        w = InferenceWeights(model)
        x = torch.rand((b, t, size, size, 3), generator=torch.Generator().manual_seed(0)).to(dev)
        mask = torch.ones((b, t), device=dev)
        graphs = {mode: GraphedInference(model, w, b, t, mode) for mode in ("reconstruct", "evaluate")}
        times = {mode: [] for mode in graphs}
        for _ in range(args.rounds):
            for mode, gi in graphs.items():
                times[mode].append(replay_median(gi, x, mask, args.steps // 2, args.warmup, args.settle_seconds))
        for mode in graphs:
            report(f"B={b} replayed {mode:11s}: " + "  ".join(f"{ms:7.3f}" for ms in times[mode]) + " ms per round;  graph "
                   f"{graphs[mode].census}")
        r, e = statistics.median(times["reconstruct"]), statistics.median(times["evaluate"])
        report(f"evaluate / reconstruct = {e / r:.4f} ({(e - r) * 1e3:+.1f} us per replay, medians over {args.rounds} rounds)")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
