"""What the rate term of quantisation-aware training costs: its two kernels alone, and the replayed train step with it.

  (a) ops.latent_rate's forward (vvae_latent_rate) and backward (vvae_latent_rate_grad) launches, and ops.latent_fake_quant beside them as
      the yardstick (the same front end, one more pass of stores), on 64 and 128 frames of 256 x 96 bf16 at --bits, every frame kept, the
      table of the frames' own codes.  HIP events around --burst back-to-back calls, per call; the three alternate inside every repeat;
      median and best of --repeats.  Twice: issued eagerly and as a captured graph of --burst calls (what a replayed step pays).  Rate and
      gradient are compared with quant.rate_reference on the first frames before anything is timed.
  (b) The replayed C3 train step (bench.py's model and batch: B = 4 clips of 16 x 256 x 256 x 3, bf16), both flavours, at quant_bits =
      --bits: one GraphedTrainStep without rate_weight (the quantisation-aware step as it was) and one with it, on the same model and
      optimizer.  Legs of --steps replays, per-step HIP events, median per leg; off and on legs alternate, --rounds of each; the difference
      of the medians of the leg medians is reported beside the spread (max - min) of the off legs' medians, which is what a difference
      has to exceed to mean anything, with the kernel node counts of both graphs.

Recorded, not judged.

    python tools/rate_bench.py [--bits 6] [--weight 0.01] [--repeats 20] [--burst 50] [--steps 20] [--rounds 4] [--small]
                               [--out profiles/rate_bench.txt]
"""
import argparse
import gc
import statistics
import sys
from types import SimpleNamespace

sys.path.insert(0, ".")
import numpy as np
import torch

HW, LD = 256, 96


def _timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def _graph_of(fn, burst):
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        for _ in range(burst):
            fn()
    return g


def kernel_stage(args, log):
    from video_vae_amd import loss as L, ops
    from video_vae_amd._lib import check, lib
    from video_vae_amd.quant import rate_reference
    dev = torch.device("cuda", 0)
    for frames in (64, 128):
        src = (torch.randn((frames, HW, LD), generator=torch.Generator().manual_seed(frames)) * 1.5).to(dev).to(torch.bfloat16)
        keep = torch.ones(frames, device=dev)
        counts = torch.empty((frames, 256), dtype=torch.int32, device=dev)
        ops.latent_fake_quant(src, keep, args.bits, counts)
        cost = L.rate_cost_table(counts, args.bits).contiguous()
        g = torch.linspace(0.5, 1.5, frames, device=dev)
        rate = torch.empty(frames, device=dev)
        grad = torch.empty_like(src)
        held = {}

        def fwd():
            check(lib().vvae_latent_rate(ops._p(src), 1, ops._p(keep), ops._p(cost), ops._p(rate), frames, HW, LD, args.bits, ops._stream()),
                  "vvae_latent_rate")

        def bwd():
            check(lib().vvae_latent_rate_grad(ops._p(src), 1, ops._p(keep), ops._p(cost), ops._p(g), ops._p(grad), frames, HW, LD, args.bits,
                                              ops._stream()), "vvae_latent_rate_grad")

        def fake():
            held["fake"] = ops.latent_fake_quant(src, keep, args.bits, counts)

        fwd(), bwd(), fake()
        torch.cuda.synchronize()
        n = 2
        terms, slope = rate_reference(src[:n].float().cpu().numpy(), np.ones(n, dtype=np.float32), args.bits, cost.cpu().numpy())
        exact = terms.astype(np.float64).sum(axis=(1, 2))
        err = float(np.abs(rate[:n].cpu().numpy().astype(np.float64) - exact).max())
        want = torch.from_numpy(g[:n].cpu().numpy()[:, None, None] * slope).to(torch.bfloat16)
        same = torch.equal(grad[:n].cpu().view(torch.int16), want.view(torch.int16))
        log(f"  {frames} frames of {HW}x{LD} bf16, {args.bits} bits: rate {float(rate.mean()) / (HW * LD):.3f} bits per code, max |rate - float64 sum "
            f"of the reference's terms| {err:.3e} of {exact.max():.1f}; gradient bitwise the reference's: {same}")
        forms = {"latent_rate (forward)": fwd, "latent_rate_grad (backward)": bwd, "latent_fake_quant (yardstick)": fake}
        elem = frames * HW * LD
        nbytes = {"latent_rate (forward)": elem * 2 + frames * 4, "latent_rate_grad (backward)": elem * 4,
                  "latent_fake_quant (yardstick)": elem * 4 + frames * 1024}
        for how in ("eager", "graph"):
            runs = {}
            for name, fn in forms.items():
                if how == "eager":
                    runs[name] = (lambda fn=fn: [fn() for _ in range(args.burst)])
                else:
                    runs[name] = _graph_of(fn, args.burst).replay
                runs[name]()
            torch.cuda.synchronize()
            us = {name: [] for name in forms}
            for _ in range(args.repeats):
                for name in forms:                               # the forms alternate inside a repeat
                    us[name].append(_timed(runs[name], args.burst))
            for name in forms:
                med = statistics.median(us[name])
                log(f"    {how:5s} {name:30s} median {med:7.2f} us  best {min(us[name]):7.2f} us per call ({args.burst} per burst, "
                    f"{args.repeats} bursts)  {nbytes[name] / 1e6:5.2f} MB  {nbytes[name] / med / 1e6:5.2f} TB/s")
            del runs
            gc.collect()


def step_stage(args, log):
    import bench
    import video_vae_amd as V
    from video_vae_amd import loss as L, optim
    from video_vae_amd.graph import GraphedTrainStep
    dev = torch.device("cuda", 0)
    B, T, S = (2, 8, 32) if args.small else (4, 16, 256)
    torch.cuda.synchronize()
    # ONE non-default stream for models, captures and replays, as the train driver has it: both graphs of a flavour share a model and an
    # optimizer, the way a re-captured shape does there
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
            base = dict(L.HPARAMS, quant_bits=args.bits)
            steps = {"off": GraphedTrainStep(model, opt, video, mask, base, hw, V.Rngs(3), warmup=1, stream=torch.cuda.current_stream()),
                     "on": GraphedTrainStep(model, opt, video, mask, dict(base, rate_weight=args.weight), hw, V.Rngs(4), warmup=1,
                                               stream=torch.cuda.current_stream())}
            nodes = {k: (s.census[0] or {}).get("kernel") for k, s in steps.items()}
            memsets = {k: (s.census[0] or {}).get("memset", 0) for k, s in steps.items()}

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
                        bpp, entropy = float(aux["rate_bpp"]), float(aux["code_entropy"])
                    finite = bool(torch.isfinite(loss))
            off, on = statistics.median(meds["off"]), statistics.median(meds["on"])
            log(f"  {flavour:5s} B={B} T={T} {S}x{S} replayed step at {args.bits} bits, kernel nodes off {nodes['off']} on {nodes['on']}, memset "
                f"nodes off {memsets['off']} on {memsets['on']}: off legs {' '.join(f'{m:.3f}' for m in meds['off'])} ms, on (rate_weight "
                f"{args.weight}) legs {' '.join(f'{m:.3f}' for m in meds['on'])} ms (median of {args.steps} steps each)")
            log(f"        off {off:.3f} ms  on {on:.3f} ms  on - off = {on - off:+.3f} ms ({100.0 * (on - off) / off:+.2f} %)  spread of the off legs "
                f"{max(meds['off']) - min(meds['off']):.3f} ms  rate_bpp {bpp:.4f}  code_entropy {entropy:.3f} bits  loss finite {finite}")
            del steps, step, opt, model, loss, aux
            gc.collect()
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=6, choices=range(2, 9))
    ap.add_argument("--weight", type=float, default=0.01, help="rate_weight of the on legs")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--small", action="store_true", help="the depth-1 model at 32 x 32 in stage (b): a quick check of the tool")
    ap.add_argument("--skip-steps", dest="skip_steps", action="store_true", help="stage (a) only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rate_bench needs a GPU")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"rate_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, --bits {args.bits}, --weight {args.weight}")
    log("(a) the two kernels alone, ops.latent_fake_quant beside them")
    kernel_stage(args, log)
    if not args.skip_steps:
        log("(b) the replayed quantisation-aware train step, rate_weight off / on")
        step_stage(args, log)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
