"""Speed of scene-cut detection (csrc/scenes.hip) on its own and as a share of an encode.

  * end to end: "encode" of one 1280 x 720 clip of --clip-frames frames (default 96) with one cut in the middle (two scenes of distinct
    colour), the full C3 model at 256² (tile 256, overlap 32: 4 x 6 tiles), --frames 16, temporal overlap 4, B = 4 tiles per replay --
    what ``infer encode --tile --temporal-overlap 4 [--scene-cuts]`` runs per clip once the clip is on the GPU: ClipInference without
    cuts, detection alone (scenes.scene_cuts: the kernels and the host's change-point loop, ending with the correlations on the host),
    and detection + ClipInference with the cuts.  Host clock around whole calls that end in a device synchronise, after a warm-up call.
  * --kernels: ops.scene_hist on --kernel-frames frames (default 96) at 720p and 1080p, HSV (64 x 64 bins) and gray (64 bins), random and
    solid-colour frames (every pixel in one bin: the LDS-add contention case), --steps launches each in that order, for a separate
    ``rocprofv3 --kernel-trace --stats``.
  * --report TRACE_CSV: per configuration the time of the three launches (LDS histograms, chunk fold, correlations) from that run's
    kernel_trace.csv (dispatches in order), and the achieved bytes/s of the histogram launch (the clip's bytes, read once) against the
    6.3 TB/s a float4 copy reaches (MI355X_MICROARCH.md).

    python tools/scene_bench.py [--clip-frames 96] [--calls 3] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o scenes -- python tools/scene_bench.py --kernels
    python tools/scene_bench.py --report DIR/.../scenes_kernel_trace.csv
"""
import argparse
import csv
import sys
import time

sys.path.insert(0, ".")
import torch

COPY_TBS = 6.3
S, O, T, OT = 256, 32, 16, 4
SHAPES = [(720, 1280), (1080, 1920)]
SPACES = [("hsv", 64), ("gray", 64)]
CONTENT = ["random", "solid"]
KERNELS = ("scene_hist_part_kernel", "scene_hist_fold_kernel", "scene_corr_kernel")


def configs():
    return [(hw, sp, n, c) for hw in SHAPES for sp, n in SPACES for c in CONTENT]


def _clip(frames, h, w, content, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    if content == "solid":
        x = torch.empty((frames, h, w, 3), dtype=torch.uint8, device=dev)
        x[..., 0], x[..., 1], x[..., 2] = 30, 170, 90
        return x
    return torch.randint(0, 256, (frames, h, w, 3), generator=g, dtype=torch.uint8, device=dev)


def two_scenes(frames, h, w, dev):
    """Random reddish frames, then random bluish ones from frames // 2 on: one cut."""
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randint(0, 64, (frames, h, w, 3), generator=g, dtype=torch.uint8, device=dev)
    half = frames // 2
    x[:half, ..., 0] += 160
    x[half:, ..., 2] += 160
    return x


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
    from video_vae_amd.scenes import scene_cuts
    from video_vae_amd.tiling import ClipInference, TileGrid
    dev = torch.device("cuda", 0)
    h, w = SHAPES[0]
    grid = TileGrid(h, w, S, O)
    model = build_model("model", S, False, None, dev)
    weights = InferenceWeights(model)
    n = args.clip_frames
    clip = two_scenes(n, h, w, dev)
    cuts = scene_cuts(clip)
    log(f"scene_bench: encode of one {n}-frame {h}x{w} clip (two scenes), full C3 model, {T}-frame windows at temporal overlap {OT}, "
        f"tile {S}, overlap {O}: {grid.ny}x{grid.nx} tiles, B = 4 tiles per replay, {args.calls} timed calls after a warm-up; cuts found: "
        f"{cuts}")
    ci = ClipInference(model, weights, grid, 4, T, OT, "encode")
    med0, best0 = _timed(lambda: ci(clip), args.calls)
    log(f"  encode, no cuts        {ci.plan(n).windows:3d} windows  median {med0 * 1e3:8.1f} ms  best {best0 * 1e3:8.1f} ms  "
        f"{n / med0:7.1f} frames/s")
    medd, bestd = _timed(lambda: scene_cuts(clip), args.calls)
    log(f"  detection alone (hsv 64)          median {medd * 1e3:8.3f} ms  best {bestd * 1e3:8.3f} ms  "
        f"{100 * medd / med0:6.3f} % of the encode")
    med1, best1 = _timed(lambda: ci(clip, cuts=scene_cuts(clip)), args.calls)
    log(f"  detection + encode     {ci.plan(n, cuts).windows:3d} windows  median {med1 * 1e3:8.1f} ms  best {best1 * 1e3:8.1f} ms  "
        f"{n / med1:7.1f} frames/s")


def kernels(args):
    from video_vae_amd import ops
    dev = torch.device("cuda", 0)
    for (h, w), sp, n, content in configs():
        clip = _clip(args.kernel_frames, h, w, content, dev)
        for _ in range(args.steps):
            ops.scene_hist(clip, n, sp)
        torch.cuda.synchronize()
        del clip
    print(f"scene_bench --kernels: {args.steps} x scene_hist of {args.kernel_frames} frames per configuration, in the order "
          f"{[(hw, sp, c) for hw, sp, _, c in configs()]}", flush=True)


def report(args, log):
    rows = [r for r in csv.DictReader(open(args.report)) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    part = [r for r in rows if KERNELS[0] in r["Kernel_Name"]]
    cfgs = configs()
    if len(part) % len(cfgs):
        raise SystemExit(f"{len(part)} histogram launches for {len(cfgs)} configurations")
    steps = len(part) // len(cfgs)
    log(f"scene_hist per launch of {args.kernel_frames} frames (rocprofv3 --kernel-trace: {args.report}), median of {steps} launches")
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    for i, ((h, w), sp, n, content) in enumerate(cfgs):
        t0 = int(part[i * steps]["Start_Timestamp"])
        t1 = int(part[(i + 1) * steps]["Start_Timestamp"]) if i + 1 < len(cfgs) else 1 << 62
        mine = [r for r in rows if t0 <= int(r["Start_Timestamp"]) < t1]
        med = {}
        for k in KERNELS:
            d = sorted(dur(r) for r in mine if k in r["Kernel_Name"])
            med[k] = d[len(d) // 2] if d else 0.0
        nbytes = args.kernel_frames * h * w * 3
        tbs = nbytes / (med[KERNELS[0]] * 1e-6) / 1e12
        log(f"  {h:4d}p {sp:4s} {n:2d} {content:6s}  hist {med[KERNELS[0]]:7.1f} us  fold {med[KERNELS[1]]:5.1f} us  "
            f"corr {med[KERNELS[2]]:5.1f} us  {nbytes / 1e6:6.1f} MB  {tbs:5.2f} TB/s = {100 * tbs / COPY_TBS:5.1f} % of {COPY_TBS} TB/s "
            f"({sum(med.values()) / args.kernel_frames:5.2f} us per frame in all)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clip-frames", dest="clip_frames", type=int, default=96)
    ap.add_argument("--kernel-frames", dest="kernel_frames", type=int, default=96)
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
