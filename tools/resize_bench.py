"""Speed of the centre-square crop + resize of ``infer`` on the host and on the device, and what ``--device-resize`` does to an encode.

Synthetic 1280 x 720 clips (data.write_synthetic_clips) in a temporary folder, one GPU, at most 16 host threads, --size 256.

  * host: infer.centre_square (data._resize_u8: torch's interpolate on the CPU) of one clip, frames/s, median of --calls calls.
  * device: data.device_centre_square (csrc/resize.hip) of the same clip already on the GPU, HIP events around one launch, median of
    --repeats launches, frames/s and bytes/s (crop bytes read + result bytes written) against the 6.3 TB/s a float4 copy reaches
    (MI355X_MICROARCH.md); data.upload_centre_square of the clip from host memory (the upload and the launches), HIP events likewise.
  * end to end: ``python -m video_vae_amd.infer encode`` (full C3 model, a checkpoint of a seeded model saved once, --frames 16,
    --batch 4) over --clips clips without and with --device-resize, alternately, each a child process under a time limit; wall clock of
    the whole command, and of the clips after the first (from the command's per-clip lines: the model load and the graph capture are
    over by then), frames/s.  --e2e-extra="--scene-cuts" (or any other flags) repeats the pair with those flags.

    python tools/resize_bench.py [--frames 48] [--clips 6] [--calls 3] [--repeats 20] [--runs 2] [--out FILE]
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, ".")
import numpy as np
import torch

COPY_TBS = 6.3
H, W, SIZE, T, B = 720, 1280, 256, 16, 4
THREADS = 16


def _median(v):
    return sorted(v)[len(v) // 2]


def host_stage(clip, args, log):
    from video_vae_amd.infer import centre_square
    centre_square(clip[:2], SIZE)
    times = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        centre_square(clip, SIZE)
        times.append(time.perf_counter() - t0)
    med = _median(times)
    log(f"  host centre_square ({torch.get_num_threads()} threads)      median {med * 1e3:9.2f} ms  best {min(times) * 1e3:9.2f} ms  "
        f"{clip.shape[0] / med:9.1f} frames/s")
    return clip.shape[0] / med


def _events(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return _median(ms) * 1e-3, min(ms) * 1e-3


def device_stage(clip, args, log):
    from video_vae_amd import data as D
    from video_vae_amd.infer import centre_square
    dev = torch.device("cuda", 0)
    n = clip.shape[0]
    u8 = torch.from_numpy(clip).to(dev)
    out = torch.empty((n, SIZE, SIZE, 3), dtype=torch.uint8, device=dev)
    same = np.array_equal(D.device_centre_square(u8[:4], SIZE).cpu().numpy(), centre_square(clip[:4], SIZE))
    log(f"  device result equals the host path on the first 4 frames: {same}")
    if not same:
        raise SystemExit("resize_bench: the device resize differs from the host path")
    s = min(H, W)
    nbytes = n * (s * s + SIZE * SIZE) * 3
    med, best = _events(lambda: D.device_centre_square(u8, SIZE, out=out), args.repeats)
    tbs = nbytes / med / 1e12
    log(f"  device_centre_square, clip on the GPU  median {med * 1e6:9.1f} us  best {best * 1e6:9.1f} us  {n / med:9.0f} frames/s  "
        f"{nbytes / 1e6:6.1f} MB  {tbs:5.2f} TB/s = {100 * tbs / COPY_TBS:5.1f} % of {COPY_TBS} TB/s  ({med * 1e6 / n:5.2f} us per frame)")
    medu, bestu = _events(lambda: D.upload_centre_square(clip, SIZE, dev), max(3, args.repeats // 4))
    log(f"  upload_centre_square, clip on the host median {medu * 1e3:9.2f} ms  best {bestu * 1e3:9.2f} ms  {n / medu:9.0f} frames/s  "
        f"({clip.nbytes / medu / 1e9:5.1f} GB/s of raw frames through the upload)")
    return n / med, n / medu


def _encode(cmd, limit):
    """Run one encode as a child under a time limit -> (wall clock of the command, seconds from its first per-clip line to its last,
    frames in all, frames of the clips after the first)."""
    t0 = time.perf_counter()
    p = subprocess.Popen(["timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    stamps, tail = [], []
    for line in p.stdout:
        tail = (tail + [line])[-30:]
        if " frames" in line and ".npy:" in line:
            stamps.append((time.perf_counter(), int(line.split(".npy:")[1].split(" frames")[0])))
    if p.wait() != 0 or len(stamps) < 2:
        raise SystemExit(f"resize_bench: {' '.join(cmd)} ended with status {p.returncode} after {len(stamps)} clips\n{''.join(tail)}")
    wall = time.perf_counter() - t0
    return wall, stamps[-1][0] - stamps[0][0], sum(n for _, n in stamps), sum(n for _, n in stamps[1:])


def end_to_end(tmp, args, log):
    import video_vae_amd as V
    from video_vae_amd import data as D, model_loader, rl_model
    from video_vae_amd.infer import model_config
    data = os.path.join(tmp, "clips")
    D.write_synthetic_clips(data, args.clips, args.frames, H, W, seed=1)
    ckpt = os.path.join(tmp, "ckpt")
    model_loader.save_checkpoint(rl_model.VideoVAE(rngs=V.Rngs(2), **model_config(SIZE, False)), None, ckpt)
    base = [sys.executable, "-m", "video_vae_amd.infer", "encode", "--model_path", ckpt, "--data", data, "--size", str(SIZE), "--frames", str(T),
            "--batch", str(B), "--threshold"]
    env_threads = os.environ.get("OMP_NUM_THREADS", "unset")
    for extra in [[]] + [e.split() for e in args.e2e_extra]:
        log(f"  infer encode {' '.join(extra) or '(plain)'}: {args.clips} clips of up to {args.frames} frames of {H}x{W}, full C3 model at {SIZE}², "
            f"--frames {T} --batch {B}, OMP_NUM_THREADS {env_threads}, {args.runs} alternating runs each")
        res = {"host": [], "device": []}
        for r in range(args.runs):
            for tag, flag in (("host", []), ("device", ["--device-resize"])):
                wall, steady, frames, after = _encode(base + extra + flag + ["--out", os.path.join(tmp, f"lat_{tag}_{r}")], args.limit)
                res[tag].append((wall, steady, frames, after))
                log(f"    run {r} {tag:6s}  whole command {wall:7.2f} s = {frames / wall:8.1f} frames/s   clips after the first "
                    f"{steady:7.3f} s = {after / steady:8.1f} frames/s")
        for tag in ("host", "device"):
            wall = _median([x[0] for x in res[tag]])
            steady = _median([x[1] for x in res[tag]])
            log(f"    median {tag:6s}  whole command {wall:7.2f} s = {res[tag][0][2] / wall:8.1f} frames/s   clips after the first "
                f"{steady:7.3f} s = {res[tag][0][3] / steady:8.1f} frames/s")
        same = True
        for f in sorted(os.listdir(os.path.join(tmp, "lat_host_0"))):
            with np.load(os.path.join(tmp, "lat_host_0", f)) as a, np.load(os.path.join(tmp, "lat_device_0", f)) as b:
                same = same and sorted(a.files) == sorted(b.files) and all(a[k].tobytes() == b[k].tobytes() for k in a.files)
        log(f"    every array of the two paths' latent files bitwise equal: {same}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48, help="frames per clip")
    ap.add_argument("--clips", type=int, default=6, help="clips of the end-to-end encode")
    ap.add_argument("--calls", type=int, default=3, help="timed host calls")
    ap.add_argument("--repeats", type=int, default=20, help="timed device launches")
    ap.add_argument("--runs", type=int, default=2, help="end-to-end runs per path, alternating")
    ap.add_argument("--limit", type=int, default=240, help="time limit of one encode command, seconds")
    ap.add_argument("--e2e-extra", dest="e2e_extra", action="append", default=[], help="flags of a further end-to-end pair, written with '=': --e2e-extra='--scene-cuts'")
    ap.add_argument("--skip-e2e", dest="skip_e2e", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.set_num_threads(min(THREADS, torch.get_num_threads()))
    if not torch.cuda.is_available():
        raise SystemExit("resize_bench needs a GPU")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    clip = np.random.default_rng(0).integers(0, 256, size=(args.frames, H, W, 3), dtype=np.uint8)
    log(f"resize_bench: centre square of {args.frames} frames of {H}x{W} -> {SIZE}x{SIZE} (crop {min(H, W)}² at left {(W - min(H, W)) // 2})")
    host_fps = host_stage(clip, args, log)
    dev_fps, up_fps = device_stage(clip, args, log)
    log(f"  device / host: {dev_fps / host_fps:8.1f} x with the clip on the GPU, {up_fps / host_fps:6.1f} x with the upload")
    if not args.skip_e2e:
        with tempfile.TemporaryDirectory() as tmp:
            end_to_end(tmp, args, log)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
