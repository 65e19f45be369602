"""Frames/s of the replayed inference graphs (infer.GraphedInference: encode, decode, reconstruct) at 16 x 256 x 256 frames, full depth, bf16,
against the eager ``forward(train=False)`` without a weights holder, measured in the same process; and the peak allocation of each leg.

Protocol as bench.py's: warm-up, a settle phase of untimed replays (--settle-seconds), then the median of per-replay HIP-event times.

    python tools/infer_bench.py [--batches 4 16] [--steps 20] [--warmup 3] [--settle-seconds 1] [--flavour model|rl] [--out FILE]
"""
import argparse
import gc
import statistics
import sys
import time

sys.path.insert(0, ".")
import torch

import video_vae_amd as V
from video_vae_amd import rl_model
from video_vae_amd.infer import GraphedInference, InferenceWeights, model_config


def timed(fn, steps, warmup, settle):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t_end = time.perf_counter() + settle
    while time.perf_counter() < t_end:
        fn()
        torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    evs[0].record()
    for i in range(steps):
        fn()
        evs[i + 1].record()
    torch.cuda.synchronize()
    return statistics.median(evs[i].elapsed_time(evs[i + 1]) for i in range(steps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-seconds", type=float, default=1.0)
    ap.add_argument("--flavour", default="model", choices=["model", "rl"])
    ap.add_argument("--modes", nargs="+", default=["encode", "decode", "reconstruct", "eager"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cls = rl_model.VideoVAE if args.flavour == "rl" else V.VideoVAE
    lines = [f"infer_bench: {args.flavour} flavour, full depth, bf16, {args.frames} x {args.size} x {args.size} frames; median of {args.steps} "
             f"per-replay HIP-event times after {args.warmup} warm-up + {args.settle_seconds:g} s settle"]

    def report(msg):
        print(msg, flush=True)
        lines.append(msg)

    for b in args.batches:
        g = torch.Generator().manual_seed(b)
        x = torch.rand((b, args.frames, args.size, args.size, 3), generator=g).to(dev)
        mask = torch.ones((b, args.frames), device=dev)
        if "eager" in args.modes:
            # the baseline: forward(train=False) of a model that has no weights holder (per-call weight casts, library products), eager
            plain = cls(rngs=V.Rngs(2), **model_config(args.size, False)).to(dev)
            emask = mask.reshape(b, 1, 1, args.frames)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            with torch.no_grad():
                ms = timed(lambda: plain(x, emask, V.Rngs(3), train=False), args.steps, args.warmup, args.settle_seconds)
            peak = torch.cuda.max_memory_allocated() / 2 ** 30
            report(f"B={b:3d} eager forward(train=False), no weights holder: {ms:8.3f} ms  {b * args.frames / ms * 1e3:9.1f} frames/s  "
                   f"peak {peak:6.2f} GiB")
            del plain
            gc.collect()
            torch.cuda.empty_cache()
        model = cls(rngs=V.Rngs(2), **model_config(args.size, False)).to(dev)
        w = InferenceWeights(model)
        comp = model.encode(x, mask).compressed_representation.clone()
        for mode in ("encode", "decode", "reconstruct"):
            if mode not in args.modes:
                continue
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            gi = GraphedInference(model, w, b, args.frames, mode)
            inp = comp if mode == "decode" else x
            ms = timed(lambda: gi(inp, mask), args.steps, args.warmup, args.settle_seconds)
            peak = torch.cuda.max_memory_allocated() / 2 ** 30
            report(f"B={b:3d} replayed {mode:11s}: {ms:8.3f} ms  {b * args.frames / ms * 1e3:9.1f} frames/s  peak {peak:6.2f} GiB  "
                   f"graph {gi.census}")
            del gi
            gc.collect()
            torch.cuda.empty_cache()
        del model, w, comp
        gc.collect()
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
