"""Rate and distortion of ``--quantise-bits``, and what the quantiser costs.

Synthetic clips (data.write_synthetic_clips) in a temporary folder, one GPU, the full C3 model with seeded random weights (or
--model_path) at --size 256, --frames 16, --batch 4, the deterministic gate.  For bits in {off, 8, 6, 4, 3, 2}:

  * PSNR / SSIM (frame-weighted over the clips) of the replayed "evaluate" graph, through the quantiser when it is on;
  * bpp_entropy (quant.rate_summary: the zeroth-order entropy of the pooled codes plus the side information) and bpp_file (8 x the bytes
    of the clip's latent file, infer.pack_latents + save_latents, over its pixels), ratios of sums over the clips;
  * eval time per clip: the host clock around a clip's replays (uploads, replays, the copies of metrics and counts back, ending in a
    synchronise), windows prepared beforehand, median over the clips of --passes passes, the graphs with and without the quantiser
    alternating within a pass.
  * the kernel alone: ops.latent_quantise on the means of one batch (batch x frames frames of hw x ld, bf16), HIP events around --burst
    back-to-back launches, median of --repeats bursts, per launch, with and without the in-place dequantisation, and its bytes over time.

Random weights have no meaningful rate-distortion curve: the numbers are recorded, not judged.

    python tools/quant_bench.py [--clips 4] [--clip-frames 48] [--passes 3] [--repeats 20] [--out profiles/r13_quant_bench.txt]
"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, ".")
import numpy as np
import torch

SIZE, T, B = 256, 16, 4
BITS = (None, 8, 6, 4, 3, 2)


def _median(v):
    return sorted(v)[len(v) // 2]


def kernel_stage(mean, keep, args, log):
    from video_vae_amd import ops
    frames = mean.shape[0] * mean.shape[1]
    hw, ld = mean.shape[2:]
    for in_place in (False, True):
        for bits in (8, 4):
            lat = mean.clone()
            out = ops.latent_quantise(lat, keep, bits, dequantise_in_place=in_place)
            fn = lambda: ops.latent_quantise(lat, keep, bits, dequantise_in_place=in_place, out=out)
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
            nbytes = frames * hw * ld * (2 * (2 if in_place else 1) + 1) + frames * (ld * 4 + 1024)
            med = _median(us)
            log(f"  latent_quantise {frames} frames of {hw}x{ld} bf16, {bits} bits, {'in place' if in_place else 'codes only'}: median "
                f"{med:7.2f} us  best {min(us):7.2f} us per launch ({args.burst} per burst, {args.repeats} bursts)  {nbytes / 1e6:5.2f} MB  "
                f"{nbytes / med / 1e6:5.2f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--clip-frames", dest="clip_frames", type=int, default=48)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--model_path", default=None)
    ap.add_argument("--small", action="store_true", help="the depth-1 model (a quick check of the tool)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quant_bench needs a GPU")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from video_vae_amd import data as D
    from video_vae_amd import infer as I
    from video_vae_amd import ops
    from video_vae_amd.quant import rate_dataset, rate_summary
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    model = I.build_model("model", SIZE, args.small, args.model_path, dev)
    weights = I.InferenceWeights(model)
    ld = model.encoder.selection_layer1.kernel.shape[0]
    log(f"quant_bench: {args.clips} clips of up to {args.clip_frames} frames at {SIZE}x{SIZE}, {'small' if args.small else 'full C3'} model "
        f"({'seeded random weights' if not args.model_path else args.model_path}), --frames {T} --batch {B}")
    with tempfile.TemporaryDirectory() as tmp:
        D.write_synthetic_clips(os.path.join(tmp, "clips"), args.clips, args.clip_frames, 360, 480, seed=1)
        clips = [I.clip_windows(p, SIZE, T) for p in I._clip_paths(os.path.join(tmp, "clips"))]
        runners = {bits: I.GraphedInference(model, weights, B, T, "evaluate", quant_bits=bits) for bits in BITS}
        encoder = I.GraphedInference(model, weights, B, T, "encode", want_log_variance=False)

        def evaluate(bits, items):
            """One clip through the "evaluate" graph -> (psnr, ssim, selection per real frame, pooled counts or None)."""
            per = {"psnr": [], "ssim": [], "selection": []}
            pooled = np.zeros(256, dtype=np.int64)
            for grp, real in I._batches(items, B):
                grp = grp + [grp[-1]] * (B - real)
                out = runners[bits](I._window_batch(grp, dev), torch.from_numpy(np.stack([g[1] for g in grp])).to(dev))
                fm, sel = out[1], out[2]
                got = {"psnr": fm.psnr.cpu().numpy(), "ssim": fm.ssim.cpu().numpy(), "selection": sel.cpu().numpy()}
                cnt = out[3].cpu().numpy().astype(np.int64) if bits is not None else None
                for i in range(real):
                    for k in per:
                        per[k].append(got[k][i, :grp[i][2]])
                    if cnt is not None:
                        pooled += cnt[i, :grp[i][2]].sum(axis=0)
            torch.cuda.synchronize()
            return {k: np.concatenate(v).astype(np.float64) for k, v in per.items()}, pooled

        def file_bytes(bits, items, path):
            """The clip's latent file as infer encode writes it -> bytes."""
            means, sels, codes, steps = [], [], [], []
            for grp, real in I._batches(items, B):
                grp = grp + [grp[-1]] * (B - real)
                lat = encoder(I._window_batch(grp, dev), torch.from_numpy(np.stack([g[1] for g in grp])).to(dev))
                if bits is not None:
                    q = ops.latent_quantise(lat.mean.contiguous(), lat.selection, bits)
                for i in range(real):
                    c = grp[i][2]
                    means.append(lat.mean[i, :c].float().cpu())
                    sels.append(lat.selection[i, :c].cpu())
                    if bits is not None:
                        codes.append(q.codes[i, :c].cpu())
                        steps.append(q.step[i, :c].cpu())
            arrays = I.pack_latents(torch.cat(means), torch.cat(sels), quant=None if bits is None else (torch.cat(codes), torch.cat(steps), bits))
            return I.save_latents(path, arrays)

        times = {bits: [] for bits in BITS}
        for items in clips:                                   # every graph and every shape once before anything is timed
            for bits in BITS:
                evaluate(bits, items)
        for _ in range(args.passes):
            for items in clips:
                for bits in BITS:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    evaluate(bits, items)
                    times[bits].append(time.perf_counter() - t0)
        log(f"  {'bits':>5s} {'psnr dB':>9s} {'ssim':>8s} {'kept':>6s} {'bpp_entropy':>12s} {'bpp_raw':>9s} {'bpp_file':>9s} {'eval ms/clip':>13s}")
        for bits in BITS:
            frames = psnr = ssim = kept = nbytes = 0
            rates = []
            for ci, items in enumerate(clips):
                per, pooled = evaluate(bits, items)
                n = per["psnr"].shape[0]
                frames, psnr, ssim, kept = frames + n, psnr + per["psnr"].sum(), ssim + per["ssim"].sum(), kept + per["selection"].sum()
                nbytes += file_bytes(bits, items, os.path.join(tmp, f"lat_{bits}_{ci}.npz"))
                if bits is not None:
                    rates.append(rate_summary(pooled, per["selection"], n, SIZE, SIZE, ld, bits))
            d = rate_dataset(rates) if rates else None
            log(f"  {'off' if bits is None else bits:>5} {psnr / frames:9.3f} {ssim / frames:8.4f} {kept / frames:6.3f} "
                f"{d['bpp_entropy'] if d else float('nan'):12.4f} {d['bpp_raw'] if d else float('nan'):9.4f} "
                f"{8.0 * nbytes / (frames * SIZE * SIZE):9.4f} {_median(times[bits]) * 1e3:13.2f}")
        items = clips[0]
        grp = (items + [items[-1]] * B)[:B]
        lat = encoder(I._window_batch(grp, dev), torch.ones((B, T), device=dev))
        kernel_stage(lat.mean.clone().contiguous(), torch.ones((B, T), device=dev), args, log)         # every frame kept: the full work
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
