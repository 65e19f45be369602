"""Speed of the training loader with the resize on the host and on the device (``train --crop_size 512 --device-resize``).

Synthetic 1280 x 720 clips (data.write_synthetic_clips) in a temporary folder, one GPU, the reference's recipe: one random 512 x 512 crop
per clip resized to 256 x 256, batches of 4 clips x 16 frames, --workers worker processes (4; a number from the command line, never the
machine's core count).  Host and device runs alternate; every figure is frames/s unless it says otherwise.

  (a) loader only: data.create_batched_dataloader(as_uint8=True) without and with device_resize=True, iterated on the host with nothing
      behind it: wall clock of --batches batches after 2 untimed ones.
  (b) front end: one resident uint8 batch on the GPU, HIP events around ops.crop_resize_norm (512 -> 256, / 255, bf16: one launch) and
      around the three framework launches of the default DevicePrefetcher (.float(), div, .to(bf16)) on the 256 x 256 bytes of the same
      batch (what the host-resizing loader uploads); median of --repeats.
  (c) the replayed C3 train step (bench.py's model and shape, one captured GraphedTrainStep) fed by DevicePrefetcher over each loader,
      next to the same replay on a resident batch: wall clock of --steps steps after --warmup untimed ones.

``--y4m`` runs the three legs on YUV4MPEG2 clips instead (``train --data Y4MDIR --device-yuv``): the same synthetic frames written as 4:2:0
.y4m files (y4m.write) and, for comparison, as .npy files.

  (a) loader only: the host-conversion loader on the .y4m files (the workers convert whole frames in numpy; --host-batches timed batches,
      it is slow), the device_yuv loader on the same files (the workers copy plane bytes), the device-resize loader on the .npy files.
  (b) front end: one resident batch of windows, HIP events around bursts of --burst launches of ops.yuv_window_resize_norm at 512 -> 256
      and 256 -> 256 (bf16), and of the two-launch route on the same frame count: ops.yuv_to_rgb_u8 on dense crop-sized planes, then
      ops.crop_resize_norm.  The two routes are checked to agree bitwise first.
  (c) the replayed C3 step fed from the .y4m files without and with device_yuv, next to the resident replay.

    python tools/loader_bench.py [--workers 4] [--clips 16] [--batches 24] [--repeats 20] [--steps 40] [--warmup 8] [--runs 2] [--out FILE]
    python tools/loader_bench.py --y4m [--host-batches 8] [--burst 10] [... as above]
"""
import argparse
import gc
import itertools
import os
import sys
import tempfile
import time

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from resize_bench import THREADS, _events, _median          # the protocol of the round-12 tool: medians, HIP events around one call

H, W, CROP, SIZE, T, B = 720, 1280, 512, 256, 16, 4
PROD = dict(height=SIZE, width=SIZE, channels=3, patch_size=16, encoder_depth=9, decoder_depth=12, mlp_dim=1536, num_heads=8,
            qkv_features=512, max_temporal_len=64, spatial_compression_rate=8, unembedding_upsample_rate=4)     # bench.py's C3 model


def _loader(data, args, device_resize, **kw):
    from video_vae_amd import data as D
    return D.create_batched_dataloader(data, batch_size=B, max_frames=T, resize=(SIZE, SIZE), crop_size=CROP, shuffle=True, seed=0,
                                       num_workers=args.workers, prefetch_size=4 * args.workers, drop_remainder=True, num_epochs=None,
                                       as_uint8=True, device_resize=device_resize, **kw)


def _burst(fn, repeats, burst):
    """Median and best seconds per call of ``fn``: HIP events around ``burst`` back-to-back calls, ``repeats`` times."""
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


def y4m_loader_only(npy, y4m, args, log):
    legs = {"y4m host conversion": lambda: _loader(y4m, args, True), "y4m device_yuv": lambda: _loader(y4m, args, False, device_yuv=True),
            "npy device-resize": lambda: _loader(npy, args, True)}
    res = {k: [] for k in legs}
    for r in range(args.runs):
        for tag, make in legs.items():
            batches = args.host_batches if tag == "y4m host conversion" else args.batches
            it = iter(make())
            for _ in range(args.workers if tag == "y4m host conversion" else 2):      # one untimed round of the workers
                shapes = {k: tuple(v.shape) for k, v in next(it).items()}
            t0 = time.perf_counter()
            for _ in range(batches):
                next(it)
            dt = time.perf_counter() - t0
            del it
            res[tag].append(batches * B * T / dt)
            log(f"    run {r} {tag:20s}  {batches} batches of {shapes} in {dt:7.3f} s = {res[tag][-1]:8.1f} frames/s")
    for tag in legs:
        log(f"    median {tag:20s}  {_median(res[tag]):8.1f} frames/s")
    return {k: _median(v) for k, v in res.items()}


def y4m_front_end(args, log):
    import numpy as np
    from video_vae_amd import ops
    dev = torch.device("cuda", 0)
    n = B * T
    g = torch.Generator().manual_seed(0)
    params = torch.tensor([[i & 1, (i >> 1) & 1, 0, 0] for i in range(B)], dtype=torch.int32, device=dev)
    for crop in (CROP, SIZE):
        y = torch.randint(0, 256, (n, crop, crop), dtype=torch.uint8, generator=g).to(dev)
        u, v = (torch.randint(0, 256, (n, crop // 2, crop // 2), dtype=torch.uint8, generator=g).to(dev) for _ in range(2))
        # the window of the dense planes taken as the whole frame (top = left = 0): the clamped gather of y4m.Y4MClip.window
        idx = torch.from_numpy(np.clip(np.arange(crop // 2 + 3) - 1, 0, crop // 2 - 1)).to(dev)
        wu, wv = (c[:, idx][:, :, idx].contiguous() for c in (u, v))
        zero = torch.zeros_like(params)
        out = torch.empty((n, SIZE, SIZE, 3), dtype=torch.bfloat16, device=dev)
        rgb = torch.empty((n, crop, crop, 3), dtype=torch.uint8, device=dev)
        out2 = torch.empty_like(out)
        fused = lambda p=params: ops.yuv_window_resize_norm(y, wu, wv, p, T, "420", "centre", "bt601", SIZE, SIZE, dtype=torch.bfloat16, out=out)

        def two():
            ops.yuv_to_rgb_u8(y, u, v, out=rgb)
            return ops.crop_resize_norm(rgb, 0, 0, crop, crop, SIZE, SIZE, dtype=torch.bfloat16, out=out2)
        same = torch.equal(fused(zero).view(torch.int16), two().view(torch.int16))
        log(f"    {crop} -> {SIZE}: the fused launch equals yuv_to_rgb_u8 + crop_resize_norm bitwise: {same}")
        if not same:
            raise SystemExit("loader_bench: the fused front end differs from the two-launch route")
        for r in range(args.runs):
            m2, b2 = _burst(two, args.repeats, args.burst)
            m1, b1 = _burst(fused, args.repeats, args.burst)
            nbytes = y.numel() + wu.numel() * 2 + out.numel() * 2
            log(f"    run {r} {crop} -> {SIZE} two launches (yuv_to_rgb_u8, crop_resize_norm)  median {m2 * 1e6:8.1f} us  best {b2 * 1e6:8.1f} us")
            log(f"    run {r} {crop} -> {SIZE} yuv_window_resize_norm, one launch            median {m1 * 1e6:8.1f} us  best {b1 * 1e6:8.1f} us  "
                f"{nbytes / 1e6:6.1f} MB = {nbytes / m1 / 1e12:5.2f} TB/s  ({n / m1:9.0f} frames/s)")


def loader_only(data, args, log):
    res = {"host": [], "device": []}
    for r in range(args.runs):
        for tag in ("host", "device"):
            it = iter(_loader(data, args, tag == "device"))
            for _ in range(2):
                shape = tuple(next(it)["video"].shape)
            t0 = time.perf_counter()
            for _ in range(args.batches):
                next(it)
            dt = time.perf_counter() - t0
            del it
            res[tag].append(args.batches * B * T / dt)
            log(f"    run {r} {tag:6s}  {args.batches} batches of {shape} in {dt:7.3f} s = {res[tag][-1]:8.1f} frames/s")
    for tag in ("host", "device"):
        log(f"    median {tag:6s}  {_median(res[tag]):8.1f} frames/s")
    return _median(res["host"]), _median(res["device"])


def front_end(args, log):
    from video_vae_amd import ops
    dev = torch.device("cuda", 0)
    u8 = torch.randint(0, 256, (B, T, CROP, CROP, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
    flat = u8.view(B * T, CROP, CROP, 3)
    small = ops.crop_resize_u8(flat, 0, 0, CROP, CROP, SIZE, SIZE)          # the bytes the host-resizing loader would upload
    div255 = torch.full((), 255.0, dtype=torch.float32, device=dev)
    out = torch.empty((B * T, SIZE, SIZE, 3), dtype=torch.bfloat16, device=dev)
    three = lambda: torch.div(small.float(), div255).to(torch.bfloat16)
    one = lambda: ops.crop_resize_norm(flat, 0, 0, CROP, CROP, SIZE, SIZE, dtype=torch.bfloat16, out=out)
    same = torch.equal(one().view(torch.int16), three().view(torch.int16))
    log(f"    the launch's batch equals resize + the three ops bitwise: {same}")
    if not same:
        raise SystemExit("loader_bench: the device front end differs from the framework's")
    m3, b3 = _events(three, args.repeats)
    m1, b1 = _events(one, args.repeats)
    nbytes = flat.numel() + out.numel() * 2
    log(f"    three framework launches on {tuple(small.shape)} uint8     median {m3 * 1e6:8.1f} us  best {b3 * 1e6:8.1f} us")
    log(f"    crop_resize_norm {CROP} -> {SIZE}, / 255, bf16: one launch      median {m1 * 1e6:8.1f} us  best {b1 * 1e6:8.1f} us  "
        f"{nbytes / 1e6:6.1f} MB = {nbytes / m1 / 1e12:5.2f} TB/s  ({B * T / m1:9.0f} frames/s)")
    return m3, m1


def fed_step(data, args, log, yuv=False):
    import video_vae_amd as V
    from video_vae_amd import data as D, loss as L, optim
    from video_vae_amd.graph import GraphedTrainStep
    dev = torch.device("cuda", 0)
    model = V.VideoVAE(rngs=V.Rngs(2), dtype=torch.bfloat16, **PROD).to(dev)
    opt = optim.Optimizer(model, optim.reference_schedule(batch_size=B))
    video = torch.rand((B, T, SIZE, SIZE, 3), generator=torch.Generator().manual_seed(0)).to(dev, torch.bfloat16)
    mask = torch.ones((B, T), device=dev)
    t0 = time.perf_counter()
    step = GraphedTrainStep(model, opt, video, mask, L.HPARAMS, (SIZE // PROD["patch_size"]) ** 2, V.Rngs(3))
    log(f"    captured the C3 step ({B} x {T} x {SIZE}², bf16) in {time.perf_counter() - t0:.1f} s")

    def run(feed):
        for i in range(args.warmup + args.steps):
            if i == args.warmup:
                torch.cuda.synchronize()
                t = time.perf_counter()
            if feed is None:
                loss, _ = step()
            else:
                b = next(feed)
                loss, _ = step(b["video"], b["mask"])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        assert torch.isfinite(loss).all()
        return args.steps * B * T / dt

    res = {"resident": [], "host": [], "device": []}                      # yuv: host = host conversion + host resize, device = device_yuv
    for r in range(args.runs):
        for tag in ("resident", "host", "device"):
            feed = None
            if tag != "resident":
                # exactly the batches the run takes: the prefetcher's thread ends behind them and the loader's workers with it, so no
                # run works against the workers of the one before
                host = _loader(data, args, False, device_yuv=True) if yuv and tag == "device" else _loader(data, args, tag == "device")
                some = itertools.islice(iter(host), args.warmup + args.steps)
                feed = D.DevicePrefetcher(some, dev, dtype=torch.bfloat16, resize=(SIZE, SIZE) if tag == "device" else None,
                                          yuv=host.yuv if yuv and tag == "device" else None)
            res[tag].append(run(feed))
            if feed is not None:
                feed.thread.join()
                del some, feed
                gc.collect()
            log(f"    run {r} {tag:8s}  {args.steps} replayed steps = {res[tag][-1]:8.1f} frames/s")
    for tag in res:
        log(f"    median {tag:8s}  {_median(res[tag]):8.1f} frames/s")
    return {k: _median(v) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=4, help="worker processes of each loader")
    ap.add_argument("--clips", type=int, default=16, help="synthetic clips of T + 4 frames at 1280 x 720")
    ap.add_argument("--batches", type=int, default=24, help="timed batches of the loader-only leg")
    ap.add_argument("--repeats", type=int, default=20, help="timed launches of the front-end leg")
    ap.add_argument("--steps", type=int, default=40, help="timed steps of the fed-step leg")
    ap.add_argument("--warmup", type=int, default=8, help="untimed steps of the fed-step leg")
    ap.add_argument("--runs", type=int, default=2, help="runs per path, alternating")
    ap.add_argument("--skip-step", dest="skip_step", action="store_true")
    ap.add_argument("--y4m", action="store_true", help="the legs on .y4m clips: host conversion against device_yuv")
    ap.add_argument("--host-batches", dest="host_batches", type=int, default=8, help="--y4m: timed batches of the host-conversion loader")
    ap.add_argument("--burst", type=int, default=10, help="--y4m: launches between two HIP events of the front-end leg")
    ap.add_argument("--skip-loader", dest="skip_loader", action="store_true", help="--y4m: leave out leg (a)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.set_num_threads(min(THREADS, torch.get_num_threads()))
    if not torch.cuda.is_available():
        raise SystemExit("loader_bench needs a GPU")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    from video_vae_amd import data as D
    if args.y4m:
        with tempfile.TemporaryDirectory() as tmp:
            npy, y4m = os.path.join(tmp, "npy"), os.path.join(tmp, "y4m")
            D.write_synthetic_clips(npy, args.clips, T + 4, H, W, seed=1)
            D.write_synthetic_clips(y4m, args.clips, T + 4, H, W, seed=1, ext=".y4m")
            log(f"loader_bench --y4m: {args.clips} clips of up to {T + 4} frames of {H}x{W} as 4:2:0 .y4m and as .npy, crop {CROP}² -> {SIZE}², "
                f"batches of {B} x {T}, {args.workers} workers, OMP_NUM_THREADS {os.environ.get('OMP_NUM_THREADS', 'unset')}")
            if not args.skip_loader:
                log("  (a) loader only, frames/s on the host")
                a = y4m_loader_only(npy, y4m, args, log)
                log(f"    device_yuv / host conversion: {a['y4m device_yuv'] / a['y4m host conversion']:6.1f} x; "
                    f"device_yuv / npy device-resize: {a['y4m device_yuv'] / a['npy device-resize']:5.2f} x")
            log("  (b) front end on a resident batch, HIP events around bursts")
            y4m_front_end(args, log)
            if not args.skip_step:
                log("  (c) the replayed C3 step, fed from the .y4m files (host = host conversion and resize, device = device_yuv)")
                c = fed_step(y4m, args, log, yuv=True)
                log(f"    of the resident rate: host conversion {100 * c['host'] / c['resident']:5.1f} %, device_yuv {100 * c['device'] / c['resident']:5.1f} %")
        if args.out:
            with open(args.out, "a") as fh:
                fh.write("\n".join(lines) + "\n")
        return
    with tempfile.TemporaryDirectory() as tmp:
        D.write_synthetic_clips(tmp, args.clips, T + 4, H, W, seed=1)
        log(f"loader_bench: {args.clips} clips of up to {T + 4} frames of {H}x{W}, crop {CROP}² -> {SIZE}², batches of {B} x {T}, "
            f"{args.workers} workers, OMP_NUM_THREADS {os.environ.get('OMP_NUM_THREADS', 'unset')}")
        log("  (a) loader only, frames/s on the host")
        a_host, a_dev = loader_only(tmp, args, log)
        log(f"    device-resize loader / host-resize loader: {a_dev / a_host:5.2f} x")
        log("  (b) front end on a resident batch, HIP events")
        front_end(args, log)
        if not args.skip_step:
            log("  (c) the replayed C3 step, fed")
            c = fed_step(tmp, args, log)
            log(f"    fed by the device-resize loader / by the host-resize loader: {c['device'] / c['host']:5.2f} x; "
                f"of the resident rate: host {100 * c['host'] / c['resident']:5.1f} %, device {100 * c['device'] / c['resident']:5.1f} %")
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
