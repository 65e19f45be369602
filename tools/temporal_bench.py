"""Speed of overlapped temporal windows (tiling.ClipInference) against hard cuts (tiling.TiledInference), and of the two new kernels.

  * end to end: "reconstruct" of one 1280 x 720 clip of --clip-frames frames (default 96) with the full C3 model at 256² (tile 256,
    overlap 32: 4 x 6 tiles), --frames 16, B = 4 tiles per replay: hard cuts (TiledInference over the clip's 16-frame windows) and
    ClipInference at temporal overlap 0 / 4 / 8, host clock around whole calls that end in a device synchronise, after a warm-up
    call.  Reports frames/s of clip frames, the windows and stored_ratio (model frames per clip frame) of each plan, and the time per
    model window, so the stitching overhead is the difference at equal work (hard cuts vs overlap 0).
  * --kernels: only the window blend (the streaming schedule of a 96-frame clip at overlap 4: one launch per final frame range, bf16
    tiles) and temporal_mse (one 16-frame window, fp32 / fp32), --steps times each, for a separate ``rocprofv3 --kernel-trace --stats``.
  * --report STATS_CSV: per-16-frame-window kernel time of both from that run's kernel_stats.csv, and the achieved bytes/s (from shapes)
    against the 6.3 TB/s a float4 copy reaches (MI355X_MICROARCH.md).

    python tools/temporal_bench.py [--clip-frames 96] [--calls 3] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o temporal -- python tools/temporal_bench.py --kernels
    python tools/temporal_bench.py --report DIR/.../temporal_kernel_stats.csv
"""
import argparse
import csv
import sys
import time

sys.path.insert(0, ".")
import torch

COPY_TBS = 6.3
H, W, C, S, O, T = 720, 1280, 3, 256, 32, 16
KERNEL_CLIP, KERNEL_OVERLAP = 96, 4


def window_bytes(grid, plan):
    """Bytes per 16 output frames each kernel must move: blend = the covering windows' bf16 tiles in (every tile value of every window
    read once over the clip) + fp32 frames out; tmse = both fp32 operands once (a frame is read as the later and as the earlier of a
    pair; the second read is not counted)."""
    tile_vals = plan.windows * grid.tiles * T * S * S * C
    frame_vals = T * H * W * C
    per16 = T / plan.length
    return {"window_blend_kernel": tile_vals * 2 * per16 + frame_vals * 4, "tmse_part_kernel": T * H * W * C * 4 * 2}


def _timed(fn, calls):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return sorted(times)[len(times) // 2], min(times)


def end_to_end(args, log):
    from video_vae_amd.infer import InferenceWeights, build_model
    from video_vae_amd.tiling import ClipInference, TiledInference, TileGrid, WindowPlan
    dev = torch.device("cuda", 0)
    grid = TileGrid(H, W, S, O)
    model = build_model("model", S, False, None, dev)
    weights = InferenceWeights(model)
    n = args.clip_frames
    if n % T:
        raise SystemExit(f"--clip-frames {n}: a multiple of {T} (hard cuts without a padded window)")
    g = torch.Generator().manual_seed(0)
    clip = torch.randint(0, 256, (n, H, W, C), generator=g, dtype=torch.uint8).to(dev)
    log(f"temporal_bench: reconstruct of one {n}-frame {H}x{W} clip, full C3 model, {T}-frame windows, tile {S}, overlap {O}: "
        f"{grid.ny}x{grid.nx} tiles, B = 4 tiles per replay, {args.calls} timed calls after a warm-up")
    ti = TiledInference(model, weights, grid, 4, T, "reconstruct")
    mask = torch.ones(n // T, T, device=dev)
    med, best = _timed(lambda: ti(clip.view(n // T, T, H, W, C), mask), args.calls)
    log(f"  hard cuts          {n // T:3d} windows  stored_ratio 1.000  median {med * 1e3:8.1f} ms  best {best * 1e3:8.1f} ms  "
        f"{n / med:7.1f} frames/s  {med / (n // T) * 1e3:6.1f} ms per window")
    ci = ClipInference(model, weights, grid, 4, T, 0, "reconstruct")
    for o in (0, 4, 8):
        c = ci.with_grid(grid, o)
        plan = WindowPlan(n, T, o)
        med, best = _timed(lambda: c(clip), args.calls)
        log(f"  temporal overlap {o} {plan.windows:3d} windows  stored_ratio {plan.stored_ratio():.3f}  median {med * 1e3:8.1f} ms  "
            f"best {best * 1e3:8.1f} ms  {n / med:7.1f} frames/s  {med / plan.windows * 1e3:6.1f} ms per window")


def kernels(args):
    from video_vae_amd.metrics import temporal_mse
    from video_vae_amd.tiling import TileGrid, WindowPlan, blend_windows
    dev = torch.device("cuda", 0)
    grid = TileGrid(H, W, S, O)
    plan = WindowPlan(KERNEL_CLIP, T, KERNEL_OVERLAP)
    g = torch.Generator(device=dev).manual_seed(0)
    tiles = torch.rand((plan.windows, grid.tiles, T, S, S, C), generator=g, device=dev).to(torch.bfloat16)
    out = torch.empty((plan.length, H, W, C), dtype=torch.float32, device=dev)
    x = torch.rand((1, T, H, W, C), generator=g, device=dev)
    y = (x + 0.01).contiguous()
    for _ in range(args.steps):
        for w in range(plan.windows):
            blend_windows(tiles, plan, grid, plan.starts[w] if w else 0, plan.final(w), out=out)
        temporal_mse(x, y)
    torch.cuda.synchronize()
    print(f"temporal_bench --kernels: {args.steps} x (window blend of a {KERNEL_CLIP}-frame clip at overlap {KERNEL_OVERLAP} in "
          f"{plan.windows} launches, temporal_mse of one {T}-frame window) at {H}x{W}", flush=True)


def report(args, log):
    from video_vae_amd.tiling import TileGrid, WindowPlan
    plan = WindowPlan(KERNEL_CLIP, T, KERNEL_OVERLAP)
    need = window_bytes(TileGrid(H, W, S, O), plan)
    rows = list(csv.DictReader(open(args.report)))
    log(f"kernel times per {T}-frame {H}x{W} window (rocprofv3 --kernel-trace --stats: {args.report})")
    for key, nbytes in need.items():
        hit = [r for r in rows if key in r["Name"]]
        if not hit:
            log(f"  {key}: not measured")
            continue
        tot = sum(float(r["TotalDurationNs"]) for r in hit)
        calls = sum(int(r["Calls"]) for r in hit)
        if key == "window_blend_kernel":              # one clip = plan.windows launches; per 16 output frames
            ns = tot / (calls / plan.windows) * T / plan.length
            what = f"({plan.length}-frame clip at overlap {KERNEL_OVERLAP}, {plan.windows} launches, per {T} frames)"
        else:
            ns = tot / calls
            what = f"({T - 1} pairs)"
        tbs = nbytes / (ns * 1e-9) / 1e12
        log(f"  {key:20s} {ns / 1e3:8.1f} us  {nbytes / 1e6:7.1f} MB  {tbs:5.2f} TB/s = {100 * tbs / COPY_TBS:5.1f} % of {COPY_TBS} TB/s "
            f"{what}")
    fold = [r for r in rows if "tmse_fold_kernel" in r["Name"]]
    if fold:
        log(f"  tmse_fold_kernel     {sum(float(r['TotalDurationNs']) for r in fold) / sum(int(r['Calls']) for r in fold) / 1e3:8.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clip-frames", dest="clip_frames", type=int, default=96)
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
