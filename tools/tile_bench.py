"""Speed of tiled native-resolution reconstruction (tiling.TiledInference) and of its three kernels.

  * end to end: tiled "reconstruct" of 1280 x 720 clips in 16-frame windows with the full C3 model at 256² (tile 256, overlap 32: 4 x 6
    tiles), B = 4 tiles per replay, host clock around whole calls that end in a device synchronise, after a warm-up call: frames/s and
    megapixels/s of native frames, and the ratio of tile pixels to frame pixels from the grid.
  * --kernels: only the gather (24 tiles of a window, one launch), the blend (one window of bf16 tiles) and frame_metrics_wide (one
    window, fp32 / fp32), --steps times each, for a separate ``rocprofv3 --kernel-trace --stats`` run.
  * --report STATS_CSV: per-window kernel time of the three from that run's kernel_stats.csv, and the achieved bytes/s (the bytes each
    must move, from shapes) against the 6.3 TB/s a float4 copy reaches (MI355X_MICROARCH.md).

    python tools/tile_bench.py [--windows 2] [--calls 3] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o tile -- python tools/tile_bench.py --kernels
    python tools/tile_bench.py --report DIR/.../tile_kernel_stats.csv
"""
import argparse
import csv
import sys
import time

sys.path.insert(0, ".")
import torch

COPY_TBS = 6.3
H, W, C, S, O, T = 720, 1280, 3, 256, 32, 16


def window_bytes(grid):
    """Bytes each kernel must move for one 16-frame window: gather = u8 in + fp32 out per tile value; blend = bf16 tiles in + fp32 frame
    out; metrics = both fp32 frames in."""
    tile_vals = grid.tiles * T * S * S * C
    frame_vals = T * H * W * C
    return {"tile_gather_kernel": tile_vals * 5, "tile_blend_kernel": tile_vals * 2 + frame_vals * 4, "metrics_fwd_kernel": frame_vals * 8}


def end_to_end(args, log):
    from video_vae_amd.infer import InferenceWeights, build_model
    from video_vae_amd.tiling import TileGrid, TiledInference
    dev = torch.device("cuda", 0)
    grid = TileGrid(H, W, S, O)
    model = build_model("model", S, False, None, dev)
    weights = InferenceWeights(model)
    ti = TiledInference(model, weights, grid, 4, T, "reconstruct")
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (args.windows, T, H, W, C), generator=g, dtype=torch.uint8).to(dev)
    mask = torch.ones(args.windows, T, device=dev)
    ti(frames, mask)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        ti(frames, mask)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    best, med = min(times), sorted(times)[len(times) // 2]
    nf = args.windows * T
    log(f"tile_bench: tiled reconstruct, full C3 model, {H}x{W} frames, {T}-frame windows, tile {S}, overlap {O}: {grid.ny}x{grid.nx} = "
        f"{grid.tiles} tiles per frame, B = 4 tiles per replay, {args.windows} windows per call")
    log(f"tile pixels / frame pixels = {grid.pixel_ratio():.4f}")
    log(f"per call ({nf} frames): median {med * 1e3:.1f} ms, best {best * 1e3:.1f} ms over {args.calls} calls")
    log(f"  {nf / med:.1f} frames/s, {nf * H * W / med / 1e6:.1f} megapixels/s (median); {med / args.windows * 1e3:.1f} ms per window")


def kernels(args):
    from video_vae_amd.metrics import frame_metrics_wide
    from video_vae_amd.tiling import TileGrid, blend_tiles, gather_tiles
    dev = torch.device("cuda", 0)
    grid = TileGrid(H, W, S, O)
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (1, T, H, W, C), generator=g, dtype=torch.uint8).to(dev)
    tiles = torch.empty((grid.tiles, T, S, S, C), dtype=torch.float32, device=dev)
    btiles = torch.rand((grid.tiles, T, S, S, C), generator=g).to(dev).to(torch.bfloat16)
    ref = frames.float() / 255.0
    recon = (ref + 0.01).contiguous()
    mask = torch.ones(1, T, device=dev)
    for _ in range(args.steps):
        gather_tiles(frames, grid, 0, grid.tiles, out=tiles)
        blend_tiles(btiles, grid)
        frame_metrics_wide(ref, recon, mask)
    torch.cuda.synchronize()
    print(f"tile_bench --kernels: {args.steps} x (gather, blend, wide metrics) of one {H}x{W} window", flush=True)


def report(args, log):
    from video_vae_amd.tiling import TileGrid
    need = window_bytes(TileGrid(H, W, S, O))
    rows = list(csv.DictReader(open(args.report)))
    log(f"kernel times per {T}-frame {H}x{W} window (rocprofv3 --kernel-trace --stats: {args.report})")
    for key, nbytes in need.items():
        hit = [r for r in rows if key in r["Name"] and ("true, true" in r["Name"] if key == "metrics_fwd_kernel" else True)]
        if not hit:
            log(f"  {key}: not measured")
            continue
        ns = sum(float(r["TotalDurationNs"]) for r in hit) / sum(int(r["Calls"]) for r in hit)
        tbs = nbytes / (ns * 1e-9) / 1e12
        log(f"  {key:20s} {ns / 1e3:8.1f} us  {nbytes / 1e6:7.1f} MB  {tbs:5.2f} TB/s = {100 * tbs / COPY_TBS:5.1f} % of {COPY_TBS} TB/s")
    fold = [r for r in rows if "metrics_fold_kernel" in r["Name"]]
    if fold:
        log(f"  metrics_fold_kernel  {sum(float(r['TotalDurationNs']) for r in fold) / sum(int(r['Calls']) for r in fold) / 1e3:8.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=2)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--report", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    if args.kernels:
        return kernels(args)
    if args.report:
        report(args, log)
    else:
        end_to_end(args, log)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
