"""What the SSIM distortion term costs: the op beside the metrics pass it extends, and the replayed train step with it.

  (a) ops.ssim_frames forward (vvae_ssim_loss_fwd: the moment pass storing the maps A, Bm, Cm, and the fold) and forward + backward
      (vvae_ssim_loss_bwd) beside ops.recon_metrics (the same pass without the map stores, and the fold) in the same run, on 64 and 128
      frames of 256 x 256 x 3 bf16, clamp off.  HIP events around --burst back-to-back calls, per call; the three forms alternate inside
      every repeat; median and best of --repeats.  The SSIM values of the forms are compared bit for bit before anything is timed.
  (b) The replayed C3 train step (bench.py's model and batch: B = 4 clips of 16 x 256 x 256 x 3, bf16), both flavours, one
      GraphedTrainStep with the term off (the step as it was) and one at --weight, on the same model and optimizer.  Legs of --steps
      replays, per-step HIP events, median per leg; off and on legs alternate, --rounds of each; the difference of the medians of the leg
      medians is reported beside the spread (max - min) of the off legs' medians, which is what a difference has to exceed to mean anything;
      and the kernel-node counts of both graphs.

Recorded, not judged.

    python tools/ssim_loss_bench.py [--weight 0.5] [--repeats 20] [--burst 20] [--steps 20] [--rounds 4] [--small] [--out profiles/ssim_loss_bench.txt]
"""
import argparse
import gc
import statistics
import sys
from types import SimpleNamespace

sys.path.insert(0, ".")
import torch

H, W, C = 256, 256, 3


def _timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def op_stage(args, log):
    from video_vae_amd import ops
    dev = torch.device("cuda", 0)
    for frames in (64, 128):
        g = torch.Generator().manual_seed(frames)
        x = torch.rand((frames // 16, 16, H, W, C), generator=g).to(dev).to(torch.bfloat16)
        y = (x.float() + 0.05 * torch.randn(x.shape, generator=g).to(dev)).to(torch.bfloat16)
        mask = torch.ones((frames // 16, 16), device=dev)
        gout = torch.full((frames // 16, 16), 1.0 / frames, device=dev)
        leaf = y.clone().requires_grad_(True)
        held = {}

        def metrics():
            held["metrics"] = ops.recon_metrics(x, y, mask, False)[2]

        def fwd():
            with torch.no_grad():
                held["fwd"] = ops.ssim_frames(x, y, mask, clamp=False)

        def fwd_bwd():
            held["grad"] = torch.autograd.grad(ops.ssim_frames(x, leaf, mask, clamp=False), leaf, gout)[0]

        metrics(), fwd(), fwd_bwd()
        torch.cuda.synchronize()
        same = torch.equal(held["metrics"].view(torch.int32), held["fwd"].view(torch.int32))
        n = frames * H * W * C
        maps = 12 * frames * (H - 10) * (W - 10) * C
        log(f"  {frames} frames of {H}x{W}x{C} bf16: ssim of recon_metrics and ssim_frames bitwise equal: {same}; the maps hold {maps / 1e6:.1f} MB")
        forms = {"recon_metrics (pass + fold)": metrics, "ssim_frames fwd (pass + maps + fold)": fwd, "ssim_frames fwd + bwd": fwd_bwd}
        nbytes = {"recon_metrics (pass + fold)": 4 * n, "ssim_frames fwd (pass + maps + fold)": 4 * n + maps,
                  "ssim_frames fwd + bwd": 4 * n + maps + 6 * n + maps}
        runs = {name: (lambda fn=fn: [fn() for _ in range(args.burst)]) for name, fn in forms.items()}
        for fn in runs.values():
            fn()
        torch.cuda.synchronize()
        us = {name: [] for name in forms}
        for _ in range(args.repeats):
            for name in forms:                                   # the forms alternate inside a repeat
                us[name].append(_timed(runs[name], args.burst))
        med = {}
        for name in forms:
            med[name] = statistics.median(us[name])
            log(f"    {name:38s} median {med[name]:8.2f} us  best {min(us[name]):8.2f} us per call ({args.burst} per burst, {args.repeats} "
                f"bursts)  {nbytes[name] / 1e6:7.2f} MB  {nbytes[name] / med[name] / 1e6:5.2f} TB/s")
        a, b, c = (med[k] for k in forms)
        log(f"    fwd / recon_metrics = {b / a:.3f}; the backward alone (fwd + bwd - fwd) = {c - b:.2f} us")
        del runs, held, leaf
        gc.collect()
        torch.cuda.empty_cache()


def step_stage(args, log):
    import bench
    import video_vae_amd as V
    from video_vae_amd import loss as L, optim
    from video_vae_amd.graph import GraphedTrainStep
    dev = torch.device("cuda", 0)
    B, T, S = (2, 8, 32) if args.small else (4, 16, 256)
    torch.cuda.synchronize()
    # ONE non-default stream for models, captures and replays, as the train driver has it
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):
        for flavour in ("model", "rl"):
            if args.small:
                from video_vae_amd import rl_model
                from video_vae_amd.infer import model_config
                cfg = model_config(S, True)
                model = (rl_model.VideoVAE if flavour == "rl" else V.VideoVAE)(rngs=V.Rngs(2), **cfg).to(dev)
            else:
                model, cfg = bench.build_model(SimpleNamespace(size=S, workload="vae", flavour=flavour), dev, torch.bfloat16)
            opt = optim.Optimizer(model, optim.reference_schedule(batch_size=B))
            video = torch.rand((B, T, S, S, 3), generator=torch.Generator().manual_seed(0)).to(dev, torch.bfloat16)
            mask = torch.ones((B, T), device=dev)
            hw = (S // cfg["patch_size"]) ** 2
            steps = {"off": GraphedTrainStep(model, opt, video, mask, dict(L.HPARAMS), hw, V.Rngs(3), warmup=1, stream=torch.cuda.current_stream()),
                     "on": GraphedTrainStep(model, opt, video, mask, dict(L.HPARAMS, ssim_weight=args.weight), hw, V.Rngs(4), warmup=1,
                                               stream=torch.cuda.current_stream())}
            nodes = {k: (s.census[0] or {}).get("kernel") for k, s in steps.items()}

            def leg(step):
                evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
                for i in range(args.steps):
                    evs[i].record()
                    loss, aux = step()
                evs[-1].record()
                torch.cuda.synchronize()
                return statistics.median(evs[i].elapsed_time(evs[i + 1]) for i in range(args.steps)), loss, aux

            for step in steps.values():                              # every graph warm before anything is timed
                leg(step)
            meds = {"off": [], "on": []}
            for _ in range(args.rounds):
                for k in ("off", "on"):
                    ms, loss, aux = leg(steps[k])
                    meds[k].append(ms)
                    if k == "on":
                        ssim = float(aux["ssim"])
                    finite = bool(torch.isfinite(loss))
            off, on = statistics.median(meds["off"]), statistics.median(meds["on"])
            log(f"  {flavour:5s} B={B} T={T} {S}x{S} replayed step, kernel nodes off {nodes['off']} on {nodes['on']}: off legs "
                f"{' '.join(f'{m:.3f}' for m in meds['off'])} ms, on (weight {args.weight}) legs {' '.join(f'{m:.3f}' for m in meds['on'])} ms "
                f"(median of {args.steps} steps each)")
            log(f"        off {off:.3f} ms  on {on:.3f} ms  on - off = {on - off:+.3f} ms ({100.0 * (on - off) / off:+.2f} %)  spread of the off legs "
                f"{max(meds['off']) - min(meds['off']):.3f} ms  ssim {ssim:.4f}  loss finite {finite}")
            del steps, step, opt, model, loss, aux
            gc.collect()
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weight", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--small", action="store_true", help="the depth-1 model at 32 x 32 in stage (b): a quick check of the tool")
    ap.add_argument("--skip-steps", dest="skip_steps", action="store_true", help="stage (a) only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_loss_bench needs a GPU")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"ssim_loss_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, --weight {args.weight}")
    log("(a) ops.ssim_frames beside ops.recon_metrics")
    op_stage(args, log)
    if not args.skip_steps:
        log("(b) the replayed train step, SSIM term off / on")
        step_stage(args, log)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
